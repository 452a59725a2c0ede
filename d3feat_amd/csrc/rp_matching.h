// Feature-matching recall of every pair at every keypoint count (d3f_match_pairs; geometric_registration/evaluate.py:45-50, 67-82).
// (included by registration.hip after the rp_* kernels: rp_rows, rg_desc_d2 and RG_TB are theirs; RcCounts, rc_apply, rc_d2: rc_shared.h.)
//
// For each requested count k: the last min(count, k) rows of both blocks, the nearest descriptor in both directions, the mutually
// nearest pairs and how many of them lie inside the threshold under the ground truth -- what rp_match_kernel computes for ONE count
// of at most D3F_PAIRS_KMAX rows.  The blocks are in ascending score order, so with rank 0 the LAST (best) row of a block the rows of
// count k are the ranks < k of both blocks, nested in k: the nearest descriptor of a query among the ranks < k of the other block is
// a running minimum over that block walked in rank order.  One walk over the largest count serves every count:
//   mp_nearest_kernel   grid (256-rank tiles of the largest count, 2 directions, pairs).  A thread owns the query of rank r
//                       (descriptor in registers); the other block goes through an LDS tile in rank order, i.e. DESCENDING row
//                       index, with d2 <= best: the later, lower row wins an exact tie, which is what the ascending strict-< scan
//                       of rp_nn_pass keeps, at every prefix.  When the walk reaches min(k_c, rows of the other block) the threads
//                       with r < k_c store their best as a RANK (which does not depend on the count) at [pair, direction, off_c + r],
//                       off_c = k_0 + ... + k_{c-1}: sum_c k_c ints per (pair, direction), never pairs x counts x Kmax.
//   mp_count_kernel     one workgroup per (pair, count): source rank i is mutual iff ts[st[i]] == i (the ranks of one count map one
//                       to one onto the rows rp_match_kernel numbers, so the test is the same); the inlier test of rp_match_kernel
//                       on the records; integer sums through LDS, thread 0 writes both outputs.
// Every workspace entry that is read was written by the first launch (st[i] < min(k_c, rows of the target) by construction), so
// nothing is cleared; no atomics, no workgroup waits for another, the launch count does not depend on P or on the counts.
#pragma once

// block pairs[p][which] and the rows it holds, clamp(count, 0, K); no rows for an index outside [0, n_blocks) (rp_rows)
__device__ __forceinline__ RpRows mp_block(const int* __restrict__ count, const int* __restrict__ pairs, int p, int which, int n_blocks, int K) {
    return rp_rows(count, pairs, p, which, n_blocks, K, K);
}

template <int C>
__global__ void __launch_bounds__(256) mp_nearest_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                         const int* __restrict__ count, const int* __restrict__ pairs, int P,
                                                         RcCounts prm, int* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float tile[RG_TB * C];
    const int dir = blockIdx.y, kmax = prm.k[prm.n - 1];
    const int r = blockIdx.x * 256 + threadIdx.x;                                  // rank of this thread's query
    for (int p = blockIdx.z; p < P; p += gridDim.z) {
        const RpRows q = mp_block(count, pairs, p, dir, n_blocks, K), o = mp_block(count, pairs, p, dir ^ 1, n_blocks, K);
        if ((int)blockIdx.x * 256 >= min(q.n, kmax)) continue;                      // no query in this tile: the whole workgroup
        const int no = min(o.n, kmax);                                              // ranks of the other block that any count uses
        const float* Q = kp + (size_t)q.blk * K * ld + 3;
        const float* O = kp + (size_t)o.blk * K * ld + 3;
        float a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = (r < q.n) ? Q[(size_t)(q.n - 1 - r) * ld + c] : 0.f;
        // rp_nn_pass accepts its first candidate iff d2 < FLT_MAX; the test here is <=, so the start is one ulp below
        float best = __uint_as_float(0x7f7ffffeu);
        int bj = -1;
        int* out = ws + ((size_t)p * 2 + dir) * prm.total;
        int c = 0;
        // the counts whose prefix of the other block ends after `pos` ranks: the nearest so far is theirs
        auto flush = [&](int pos) {
            while (c < prm.n && min(prm.k[c], no) <= pos) {
                if (r < min(prm.k[c], q.n)) out[prm.off[c] + r] = bj;
                ++c;
            }
        };
        flush(0);
        for (int t0 = 0; t0 < no; t0 += RG_TB) {
            const int nt = min(RG_TB, no - t0);
            __syncthreads();
            for (int e = threadIdx.x; e < nt * C; e += 256) tile[e] = O[(size_t)(o.n - 1 - (t0 + e / C)) * ld + (e % C)];
            __syncthreads();
            int j = 0;
            while (j < nt) {                                                        // c < prm.n here: the last count ends the walk
                const int je = min(nt, min(prm.k[c], no) - t0);
                for (; j < je; ++j) {
                    const float d2 = rg_desc_d2<C>(a, tile + j * C);
                    if (d2 <= best) { best = d2; bj = t0 + j; }                     // descending rows: ties end on the lowest row
                }
                flush(t0 + j);
            }
        }
        __syncthreads();                                                            // the tile is reused by the next pair
    }
}

// grid (counts, pairs).  st / ts: the two lists of mp_nearest_kernel for the pair.
__global__ void __launch_bounds__(256) mp_count_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                       const int* __restrict__ count, const int* __restrict__ pairs, int P,
                                                       const float* __restrict__ gt, float thr2, RcCounts prm, const int* __restrict__ ws,
                                                       int* __restrict__ mutual_count, int* __restrict__ gt_inliers) {
    __shared__ int red[256];
    const int c = blockIdx.x, kc = prm.k[c];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const RpRows a = mp_block(count, pairs, p, 0, n_blocks, K), b = mp_block(count, pairs, p, 1, n_blocks, K);
        const int ns = min(a.n, kc);
        const float* S = kp + (size_t)a.blk * K * ld;
        const float* T = kp + (size_t)b.blk * K * ld;
        const int* st = ws + (size_t)p * 2 * prm.total + prm.off[c];
        const int* ts = st + prm.total;
        int nm = 0, ng = 0;
        for (int i = threadIdx.x; i < ns; i += 256) {
            const int j = st[i];                                                    // -1, or a rank < min(kc, b.n)
            if (j >= 0 && j < min(kc, b.n) && ts[j] == i) {
                ++nm;
                if (gt) {   // gt takes the TARGET frame into the SOURCE frame (evaluate.py:70-77), as rp_match_kernel
                    const float* t = T + (size_t)(b.n - 1 - j) * ld;
                    const float* s = S + (size_t)(a.n - 1 - i) * ld;
                    float qx, qy, qz;
                    rc_apply(gt + (size_t)p * 12, t[0], t[1], t[2], qx, qy, qz);
                    ng += rc_d2(qx, qy, qz, s[0], s[1], s[2]) < thr2 ? 1 : 0;
                }
            }
        }
        nm = d3f_block_sum(nm, red);                                                // (its first barrier: the previous pair is done with red)
        ng = d3f_block_sum(ng, red);
        if (threadIdx.x == 0) {
            mutual_count[(size_t)p * prm.n + c] = nm;
            if (gt) gt_inliers[(size_t)p * prm.n + c] = ng;
        }
    }
}

extern "C" size_t d3f_match_pairs_workspace_bytes(int P, const int* num_keypts_host, int n_counts) {
    RcCounts prm;
    if (P < 0 || !rc_counts(num_keypts_host, n_counts, D3F_MATCH_KMAX, prm)) return 0;
    return d3f_align((size_t)(P > 0 ? P : 1) * 2 * (size_t)prm.total * 4) + 256;
}

extern "C" int d3f_match_pairs(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev, int P,
                               const float* gt, float distance_threshold, const int* num_keypts_host, int n_counts, int* mutual_count,
                               int* gt_inliers, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RcCounts prm;
    if (P < 0 || n_blocks < 1 || K < 1 || (C != 16 && C != 32 && C != 64) || ld < C + 3) return D3F_ERR_ARG;
    if (!rc_counts(num_keypts_host, n_counts, D3F_MATCH_KMAX, prm) || !(distance_threshold == distance_threshold)) return D3F_ERR_ARG;
    if ((gt != nullptr) != (gt_inliers != nullptr)) return D3F_ERR_ARG;
    if (P == 0) return D3F_OK;
    if (!kp || !count_dev || !pairs_dev || !mutual_count) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_match_pairs_workspace_bytes(P, num_keypts_host, n_counts)) return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    int* ws = ar.take<int>((size_t)P * 2 * (size_t)prm.total);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const float thr2 = distance_threshold * distance_threshold;
    const int kmax = prm.k[n_counts - 1] < K ? prm.k[n_counts - 1] : K;   // most ranks of a block any pair uses
    const int pz = P < 65535 ? P : 65535;
    const dim3 grid(d3f_cdiv(kmax, 256), 2, pz);
    rg_dispatch_C(C, [&](auto c) { mp_nearest_kernel<decltype(c)::value><<<grid, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, P, prm, ws); });
    mp_count_kernel<<<dim3(n_counts, pz), 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, P, gt, thr2, prm, ws, mutual_count,
                                                          gt_inliers);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
