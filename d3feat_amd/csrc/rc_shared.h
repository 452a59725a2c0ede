// RANSAC registration of every pair at every keypoint count (d3f_register_pairs_counts): what the two halves of the call share.
// registration.hip (rp_register_counts.h) owns the entry point, the nearest descriptors and the hypotheses; radius_neighbors.hip
// (nb_register_counts.h) owns everything that walks the cell grid, whose internals stay private to it: the stack of the blocks' xyz,
// the grid over it, the scoring of the hypotheses and the selection of the winner.
#pragma once
#include "common.h"

struct RcCounts {
    int k[D3F_REPEAT_COUNTS_MAX];     // strictly ascending
    int off[D3F_REPEAT_COUNTS_MAX];   // off[c] = k[0] + ... + k[c-1]
    int n, total;                     // total = sum of k
};

// what the hypotheses kernel leaves per (pair, count) -- lists of max_validation entries, (pair, count) = p * n + c
struct RcLists {
    const float* Tlist;      // f32[P, n, max_validation, 12]
    const int* itlist;       // i32[P, n, max_validation]
    const int* validations;  // i32[P, n]
    int* cnt;                // i32[P, n, max_validation]   scratch of the scoring
    unsigned long long* sd2; // u64[P, n, max_validation]
    int max_validation;
};
struct RcOut {
    float* T_out; int* inliers; unsigned long long* sumd2; int* best_iteration; int* nearest;   // nearest may be null
};

// bytes of the stack, its lengths and the grid over n_blocks blocks of at most `rows` rows
size_t nb_rc_workspace_bytes(int n_blocks, int rows);
// gather -> grid build -> score -> select on `stream`; `rows` = min(K, largest count)
int nb_rc_score_select(const float* kp, int n_blocks, int K, int ld, const int* count_dev, const int* pairs_dev, int P, const RcCounts& prm,
                       int rows, float radius, const RcLists& lists, const RcOut& out, void* workspace, size_t workspace_bytes,
                       hipStream_t stream);

// ---- shared by the RANSAC hypotheses (registration.hip) and the ICP finish kernel (nb_icp.h): the operations below are pinned bit for
// bit by the registration tests -- change none of them.
#ifdef __HIPCC__
// Horn 1987: rotation maximising sum t_i . R s_i from the cross-covariance S = sum (s_i - ms)(t_i - mt)^T: unit quaternion =
// eigenvector of the largest eigenvalue of the symmetric 4x4 matrix N(S); cyclic Jacobi in fp64 (a fixed number of sweeps).
__device__ inline void rg_horn(const double S[3][3], double R[3][3]) {
    double N[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {0, S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {0, 0, -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {0, 0, 0, -S[0][0] - S[1][1] + S[2][2]}};
    for (int i = 0; i < 4; ++i) for (int j = 0; j < i; ++j) N[i][j] = N[j][i];
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = N[p][q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (N[q][q] - N[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {   // columns p, q of N
                    const double nkp = N[k][p], nkq = N[k][q];
                    N[k][p] = c * nkp - s * nkq;
                    N[k][q] = s * nkp + c * nkq;
                }
                for (int k = 0; k < 4; ++k) {   // rows p, q of N
                    const double npk = N[p][k], nqk = N[q][k];
                    N[p][k] = c * npk - s * nqk;
                    N[q][k] = s * npk + c * nqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int i = 1; i < 4; ++i) if (N[i][i] > N[m][m]) m = i;
    double w = V[0][m], x = V[1][m], y = V[2][m], z = V[3][m];
    const double nrm = sqrt(w * w + x * x + y * y + z * z);
    w /= nrm; x /= nrm; y /= nrm; z /= nrm;
    R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - w * z);     R[0][2] = 2 * (x * z + w * y);
    R[1][0] = 2 * (x * y + w * z);     R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - w * x);
    R[2][0] = 2 * (x * z - w * y);     R[2][1] = 2 * (y * z + w * x);     R[2][2] = 1 - 2 * (x * x + y * y);
}
#endif
