// RANSAC registration of every pair at every keypoint count (d3f_register_pairs_counts): what the two halves of the call share.
// registration.hip (rp_register_counts.h) owns the entry point, the nearest descriptors and the hypotheses; radius_neighbors.hip
// (nb_register_counts.h) owns everything that walks the cell grid, whose internals stay private to it: the stack of the blocks' xyz,
// the grid over it, the scoring of the hypotheses and the selection of the winner.
#pragma once
#include "common.h"

// the keypoint counts of a call, as every kernel that sweeps them takes them (d3f_match_pairs, d3f_register_pairs_counts,
// d3f_repeatability_pairs)
struct RcCounts {
    int k[D3F_REPEAT_COUNTS_MAX];     // strictly ascending
    int off[D3F_REPEAT_COUNTS_MAX];   // off[c] = k[0] + ... + k[c-1]
    int n, total;                     // total = sum of k
};
// k, off, total from the host list; false when a count is outside 1 .. kmax, n outside 1 .. D3F_REPEAT_COUNTS_MAX or the counts do not
// strictly ascend
static inline bool rc_counts(const int* num_keypts_host, int n, int kmax, RcCounts& out) {
    if (!num_keypts_host || n < 1 || n > D3F_REPEAT_COUNTS_MAX) return false;
    out.n = n;
    out.total = 0;
    for (int c = 0; c < D3F_REPEAT_COUNTS_MAX; ++c) out.k[c] = out.off[c] = 0;
    for (int c = 0; c < n; ++c) {
        const int k = num_keypts_host[c];
        if (k < 1 || k > kmax || (c > 0 && k <= num_keypts_host[c - 1])) return false;
        out.k[c] = k;
        out.off[c] = out.total;
        out.total += k;
    }
    return true;
}

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

// ---- shared by the kernels of registration.hip and radius_neighbors.hip: the operations below are pinned bit for bit by the
// registration tests -- change none of them.
#ifdef __HIPCC__
// p = M x + t, M the 12 floats of a row-major [R | t]: the fmaf nest of every fp32 transform of this library
__device__ __forceinline__ void rc_apply(const float* M, float x, float y, float z, float& qx, float& qy, float& qz) {
    qx = fmaf(M[0], x, fmaf(M[1], y, fmaf(M[2], z, M[3])));
    qy = fmaf(M[4], x, fmaf(M[5], y, fmaf(M[6], z, M[7])));
    qz = fmaf(M[8], x, fmaf(M[9], y, fmaf(M[10], z, M[11])));
}
// the squared distance of every fp32 search: no contraction, (dx^2 + dy^2) + dz^2
__device__ __forceinline__ float rc_d2(float qx, float qy, float qz, float x, float y, float z) {
    const float dx = __fsub_rn(qx, x), dy = __fsub_rn(qy, y), dz = __fsub_rn(qz, z);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the mixing function of every counter-based draw of this library (splitmix64's finaliser): d3f_ransac_draw (registration.hip) and
// d3f_training_draw (nb_training_pairs.h) are built on it
__host__ __device__ __forceinline__ unsigned long long rg_splitmix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The winner among the validated hypotheses of a pair.  better(a, b): larger count, then smaller sumd2, then earlier place in the list
// (= earlier iteration)
struct RcBest { int c; unsigned long long s; int v; };
__device__ __forceinline__ bool rc_better(const RcBest& x, const RcBest& y) {
    if (x.c != y.c) return x.c > y.c;
    if (x.s != y.s) return x.s < y.s;
    return x.v < y.v;
}
// the best of the 256 threads' candidates (red: 256 entries of LDS), in every thread; the first barrier ends an earlier use of red
__device__ __forceinline__ RcBest rc_block_best(const RcBest& me, RcBest* red) {
    __syncthreads();
    red[threadIdx.x] = me;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && rc_better(red[threadIdx.x + s], red[threadIdx.x])) red[threadIdx.x] = red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
// nothing validated: the identity (T: the 12 floats of the pair's result), no inliers, best_iteration -1.  The whole workgroup.
__device__ __forceinline__ void rc_store_none(float* T, int* inliers, unsigned long long* sumd2, int* best_iteration) {
    if (threadIdx.x < 12) T[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.f : 0.f;
    if (threadIdx.x == 0) { *inliers = 0; *sumd2 = 0ull; *best_iteration = -1; }
}

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
