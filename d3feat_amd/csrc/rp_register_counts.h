// RANSAC registration of every pair at every keypoint count (d3f_register_pairs_counts; geometric_registration/evaluate.py:45-50,
// 67-99 with its num_keypts swept over 5000 / 2500 / 1000 / 500 / 250).  (included by registration.hip after rp_matching.h: the
// rp_* / mp_* kernels, rg_sample and rg_fit are theirs; the half that walks the cell grid is nb_register_counts.h.)
//
// Per pair and count k what d3f_register_pairs computes for num_keypts = k, without its limit of D3F_PAIRS_KMAX rows: no kernel
// here keeps a block in LDS.  Launches, whatever P and the counts are:
//   mp_nearest_kernel      the nearest descriptor of every row at every count, both directions, as RANKS (rp_matching.h)
//   mp_count_kernel        mutual_count and gt_inliers per (pair, count)
//   rc_nn_rows_kernel      rank -> row: rank r of a block with n_k used rows is row n_k - 1 - r of the rows register_keypoints numbers
//                          at count k, so nn[off_c + i] = nt_k - 1 - st[off_c + (ns_k - 1 - i)]: the array rg_sample draws from
//   rc_hypotheses_kernel   one workgroup per (pair, count): rp_hypotheses_walk on the rows of that count
//   rc_gather_kernel, the five launches of d3f_neighbor_grid_build, rc_score_kernel, rc_select_kernel   (nb_register_counts.h)
// Nothing is cleared: every entry that is read was written by an earlier launch of the same call.
#pragma once
#include "rc_shared.h"

// grid (counts, pairs)
__global__ void __launch_bounds__(256) rc_nn_rows_kernel(int n_blocks, int K, const int* __restrict__ count, const int* __restrict__ pairs,
                                                         int P, RcCounts prm, const int* __restrict__ ranks, int* __restrict__ nn) {
    const int c = blockIdx.x, kc = prm.k[c];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const int ns = rp_rows(count, pairs, p, 0, n_blocks, K, kc).n, nt = rp_rows(count, pairs, p, 1, n_blocks, K, kc).n;
        const int* st = ranks + (size_t)p * 2 * prm.total + prm.off[c];
        int* out = nn + (size_t)p * prm.total + prm.off[c];
        for (int i = threadIdx.x; i < ns; i += 256) {
            const int j = st[ns - 1 - i];                                  // -1, or a rank < nt
            out[i] = (j >= 0 && j < nt) ? nt - 1 - j : -1;
        }
    }
}

// grid (counts, pairs)
__global__ void __launch_bounds__(256) rc_hypotheses_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                            const int* __restrict__ count, const int* __restrict__ pairs, int P,
                                                            RcCounts prm, const int* __restrict__ nn, int n, float radius, float edge_sim,
                                                            float dist_thr, unsigned long long seed, int max_iteration,
                                                            int max_validation, float* __restrict__ Tlist, int* __restrict__ itlist,
                                                            int* __restrict__ validations, int* __restrict__ iterations) {
    __shared__ int wsum[4];
    __shared__ int cand[RP_CHUNK];
    const int c = blockIdx.x, kc = prm.k[c];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, kc), b = rp_rows(count, pairs, p, 1, n_blocks, K, kc);
        const size_t pc = (size_t)p * prm.n + c;
        rp_hypotheses_walk(kp + ((size_t)a.blk * K + a.r0) * ld, a.n, kp + ((size_t)b.blk * K + b.r0) * ld, b.n, ld,
                           nn + (size_t)p * prm.total + prm.off[c], n, radius, edge_sim, dist_thr, seed, max_iteration, max_validation,
                           Tlist + pc * max_validation * 12, itlist + pc * max_validation, validations + pc, iterations + pc, wsum, cand);
        __syncthreads();                                                   // wsum and cand are reused by the next pair
    }
}

static inline int rc_rows(int K, const RcCounts& prm) { return prm.k[prm.n - 1] < K ? prm.k[prm.n - 1] : K; }   // most rows of a block any pair uses

extern "C" size_t d3f_register_pairs_counts_workspace_bytes(int P, int n_blocks, int K, const int* num_keypts_host, int n_counts,
                                                            int max_validation) {
    RcCounts prm;
    if (P < 0 || n_blocks < 1 || n_blocks > D3F_MAX_BATCH || K < 1 || max_validation < 1 || !rc_counts(num_keypts_host, n_counts, D3F_MATCH_KMAX, prm)) return 0;
    const size_t p = (size_t)(P > 0 ? P : 1), pv = p * (size_t)n_counts * (size_t)max_validation;
    return d3f_align(p * 2 * (size_t)prm.total * 4) + d3f_align(p * (size_t)prm.total * 4) + d3f_align(pv * 48) + 2 * d3f_align(pv * 4) +
           d3f_align(pv * 8) + nb_rc_workspace_bytes(n_blocks, rc_rows(K, prm)) + 256;
}

extern "C" int d3f_register_pairs_counts(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev,
                                         int P, const int* num_keypts_host, int n_counts, float max_correspondence_distance, int ransac_n,
                                         float edge_similarity, float checker_distance, int max_iteration, int max_validation, uint64_t seed,
                                         const float* gt, float distance_threshold, float* T_out, int* inliers, uint64_t* sumd2,
                                         int* validations, int* iterations, int* best_iteration, int* mutual_count, int* gt_inliers,
                                         int* nearest, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RcCounts prm;
    if (P < 0 || n_blocks < 1 || n_blocks > D3F_MAX_BATCH || K < 1 || (C != 16 && C != 32 && C != 64) || ld < C + 4) return D3F_ERR_ARG;
    if (!rc_counts(num_keypts_host, n_counts, D3F_MATCH_KMAX, prm) || ransac_n < 3 || ransac_n > RG_MAXN) return D3F_ERR_ARG;
    if (max_iteration < 0 || max_iteration > (1 << 30) || max_validation < 1 || max_validation > (1 << 20)) return D3F_ERR_ARG;
    if (!(max_correspondence_distance == max_correspondence_distance) || !(distance_threshold == distance_threshold)) return D3F_ERR_ARG;
    if (P == 0) return D3F_OK;
    if (!kp || !count_dev || !pairs_dev || !T_out || !inliers || !sumd2 || !validations || !iterations || !best_iteration ||
        !mutual_count || (gt && !gt_inliers))
        return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_register_pairs_counts_workspace_bytes(P, n_blocks, K, num_keypts_host, n_counts, max_validation))
        return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    const size_t pv = (size_t)P * n_counts * max_validation;
    int* ranks = ar.take<int>((size_t)P * 2 * (size_t)prm.total);
    int* nn = ar.take<int>((size_t)P * (size_t)prm.total);
    float* Tlist = ar.take<float>(pv * 12);
    int* itlist = ar.take<int>(pv);
    int* cnt = ar.take<int>(pv);
    unsigned long long* sd2 = ar.take<unsigned long long>(pv);
    const int rows = rc_rows(K, prm);
    const size_t gb = nb_rc_workspace_bytes(n_blocks, rows);
    char* gws = ar.take<char>(gb);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const float r = max_correspondence_distance, thr2 = distance_threshold * distance_threshold;
    const int pz = P < 65535 ? P : 65535;
    const dim3 grid(d3f_cdiv(rows, 256), 2, pz), per_count(n_counts, pz);
    rg_dispatch_C(C, [&](auto c) { mp_nearest_kernel<decltype(c)::value><<<grid, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, P, prm, ranks); });
    mp_count_kernel<<<per_count, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, P, gt, thr2, prm, ranks, mutual_count,
                                                   gt ? gt_inliers : nullptr);
    rc_nn_rows_kernel<<<per_count, 256, 0, stream>>>(n_blocks, K, count_dev, pairs_dev, P, prm, ranks, nn);
    rc_hypotheses_kernel<<<per_count, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, P, prm, nn, ransac_n, r, edge_similarity,
                                                        checker_distance, seed, max_iteration, max_validation, Tlist, itlist, validations,
                                                        iterations);
    D3F_LAUNCH_CHECK();
    const RcLists lists{Tlist, itlist, validations, cnt, sd2, max_validation};
    const RcOut out{T_out, inliers, (unsigned long long*)sumd2, best_iteration, nearest};
    return nb_rc_score_select(kp, n_blocks, K, ld, count_dev, pairs_dev, P, prm, rows, r, lists, out, gws, gb, stream);
}
