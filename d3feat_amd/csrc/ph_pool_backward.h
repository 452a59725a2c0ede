// Backward of the two gathers at a level boundary: the strided shortcut's max pooling (d3f_ind_max_pool_backward) and the decoder's
// nearest upsampling + skip concatenation (d3f_closest_pool_cat_backward).  Included by pool_head.hip behind ph_batch_norm.h, whose
// tile helpers (bn_geo, bn_lane, bn_ld4, bn_st4, bn_total) are reused as they are.  The definitions (tie rules, summation orders) are in
// include/d3feat_amd.h; nothing here uses an atomic on float data, and two calls give equal bits.
//
// One thread mapping under all four kernels: lanes run across columns, a QUAD of four consecutive columns per lane, LQ lanes per row
// (the power of two >= ceil(C / 4), at most 16), R = 256 / LQ rows per workgroup, grid.y = column blocks of 4 LQ columns.  The <true>
// instantiations move a quad as one 16-byte access (C % 4 == 0, every leading dimension a multiple of 4, every base pointer 16-byte
// aligned), the <false> ones as four guarded 4-byte accesses; rows and columns map to threads in the same way, so no sum depends on
// the path.
//
// d3f_ind_max_pool_backward, three launches:
//   1  pb_colmin_kernel   per slice of fine rows: the ordered-uint column minimum (the forward's) and the number of rows that hold it;
//                         clears the ticket of launch 2
//   2  pb_row_kernel      per pooled row: the tie count T over the K slots, gs = g / T into the workspace, the row's shadow term; per
//                         slice of pooled rows the float64 partial of S.  The LAST workgroup (d3f_last_block) folds the slices:
//                         colmin[c], M[c], S[c] -> share[c] = S / M
//   3  pb_gather_kernel   per fine row: gs over the row's segment of the transposed table in edge order, where the row holds the
//                         pooled maximum; plus share where the row holds the column minimum
// d3f_closest_pool_cat_backward, one launch: up_gather_kernel, the segment sum of the first C1 columns of g.
#pragma once
#include "ph_batch_norm.h"

// A column's (ordered minimum, number of entries that equal it AS VALUES): -0 orders below +0 but equals it, so counts are compared on
// the key of the value with its zero made positive.  Integer work throughout: any merge order gives the same pair.
__device__ __forceinline__ unsigned pb_key(unsigned om) { return d3f_f2ord(d3f_ord2f(om) + 0.f); }
__device__ __forceinline__ void pb_min_take(unsigned& om, int& cnt, unsigned om2, int cnt2) {
    const unsigned ka = cnt > 0 ? pb_key(om) : 0xFFFFFFFFu, kb = cnt2 > 0 ? pb_key(om2) : 0xFFFFFFFFu;
    const int ca = ka <= kb ? cnt : 0, cb = kb <= ka ? cnt2 : 0;
    cnt = ca + cb;
    om = min(om, om2);
}

template <bool VEC>
__global__ void __launch_bounds__(256) pb_colmin_kernel(const float* __restrict__ x, int ldx, int N1, const int* __restrict__ N1_dev, int C,
                                                        int S, int LQ, unsigned* __restrict__ pmin, int* __restrict__ pcnt,
                                                        unsigned* __restrict__ ticket) {
    __shared__ unsigned sMin[256 * 4];
    __shared__ int sCnt[256 * 4];
    const int n = d3f_dyn(N1, N1_dev);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ticket = 0u;
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const BnLane t = bn_lane(n, S, LQ, C);
    const int R = 256 / LQ, tid = threadIdx.x;
    unsigned om[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    int cnt[4] = {0, 0, 0, 0};
    if (t.live)
        for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) pb_min_take(om[j], cnt[j], d3f_f2ord(v[u][j]), 1);
                }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sMin[tid * 4 + j] = om[j]; sCnt[tid * 4 + j] = cnt[j]; }
    __syncthreads();
    for (int s = R >> 1; s > 0; s >>= 1) {
        if (t.r < s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned a = sMin[tid * 4 + j];
                int n = sCnt[tid * 4 + j];
                pb_min_take(a, n, sMin[(tid + s * LQ) * 4 + j], sCnt[(tid + s * LQ) * 4 + j]);
                sMin[tid * 4 + j] = a;
                sCnt[tid * 4 + j] = n;
            }
        }
        __syncthreads();
    }
    if (t.r == 0 && t.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c + j < C) {
                pmin[(size_t)blockIdx.x * C + t.c + j] = sMin[tid * 4 + j];
                pcnt[(size_t)blockIdx.x * C + t.c + j] = sCnt[tid * 4 + j];
            }
    }
}

// the slice partials of launch 1 folded for column c (integers and minima: any order gives the same result)
__device__ __forceinline__ void pb_colmin_total(const unsigned* __restrict__ pmin, const int* __restrict__ pcnt, int nsl, int C, int c,
                                                unsigned& om, int& cnt) {
    om = 0xFFFFFFFFu;
    cnt = 0;
    for (int sl = 0; sl < nsl; ++sl) pb_min_take(om, cnt, pmin[(size_t)sl * C + c], pcnt[(size_t)sl * C + c]);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
pb_row_kernel(const float* __restrict__ x, int ldx, int N1, const int* __restrict__ N1_dev, int C, const int* __restrict__ idx, int N2,
              const int* __restrict__ N2_dev, int ld_idx, int K, const float* __restrict__ y, int ldy, const float* __restrict__ g, int ldg,
              int S1, int S2, int LQ, const unsigned* __restrict__ pmin, const int* __restrict__ pcnt, float* __restrict__ gs, int ldgs,
              double* Spart, unsigned* ticket, float* __restrict__ colmin, float* __restrict__ share) {
    __shared__ double red[256 * 4];
    __shared__ float sMin[64];
    __shared__ int sHas[64];
    const int n1 = d3f_dyn(N1, N1_dev), n2 = d3f_dyn(N2, N2_dev);
    const int nsl1 = (int)(((long long)n1 + S1 - 1) / S1), nsl2 = max(1, (int)(((long long)n2 + S2 - 1) / S2));
    if ((int)blockIdx.x >= nsl2) return;             // (slice 0 always takes part: the fold below runs for n2 == 0 too)
    const BnLane t = bn_lane(n2, S2, LQ, C);
    const int R = 256 / LQ, tid = threadIdx.x;
    if (tid < LQ * 4) {
        const int c = blockIdx.y * LQ * 4 + tid;
        unsigned om = 0xFFFFFFFFu;
        int cnt = 0;
        if (c < C) pb_colmin_total(pmin, pcnt, nsl1, C, c, om, cnt);
        sMin[tid] = d3f_ord2f(om);
        sHas[tid] = cnt;
    }
    __syncthreads();
    float cm[4];
    bool has[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { cm[j] = sMin[(tid % LQ) * 4 + j]; has[j] = sHas[(tid % LQ) * 4 + j] > 0; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.live)
        for (int row = t.n0 + t.r; row < t.n1; row += R) {
            float yv[4], gv[4];
            bn_ld4<VEC>(y + (size_t)row * ldy, t.c, C, yv);
            bn_ld4<VEC>(g + (size_t)row * ldg, t.c, C, gv);
            const int* irow = idx + (size_t)row * ld_idx;
            int T[4] = {0, 0, 0, 0}, nsh = 0;
            for (int k0 = 0; k0 < K; k0 += 4) {       // four gathered rows in flight
                int id[4];
                float v[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) id[u] = k0 + u < K ? irow[k0 + u] : -2;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (id[u] >= 0 && id[u] < n1) bn_ld4<VEC>(x + (size_t)id[u] * ldx, t.c, C, v[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u >= K) continue;
                    if (id[u] >= 0 && id[u] < n1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) T[j] += v[u][j] == yv[j] ? 1 : 0;
                    } else {
                        ++nsh;                         // a shadow slot: gathers the column minima
                    }
                }
            }
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tie = (has[j] && cm[j] == yv[j]) ? nsh : 0;
                const int Tj = T[j] + tie;
                o[j] = Tj > 0 ? gv[j] / (float)Tj : 0.f;
                if (tie > 0) acc[j] += (double)((float)tie * o[j]);
            }
            bn_st4<true>(gs + (size_t)row * ldgs, t.c, C, o);   // (the workspace's rows are padded to whole quads)
        }
    bn_chain_tree(acc, red, LQ);
    if (t.r == 0 && t.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c + j < C) Spart[(size_t)blockIdx.x * C + t.c + j] = acc[j];
    }
    if (!d3f_last_block(ticket, (unsigned)nsl2 * gridDim.y)) return;
    for (int c = tid; c < C; c += 256) {
        unsigned om;
        int cnt;
        pb_colmin_total(pmin, pcnt, nsl1, C, c, om, cnt);
        const double Sc = bn_total(Spart, nsl2, C, c);
        colmin[c] = d3f_ord2f(om);
        share[c] = cnt > 0 ? (float)(Sc / (double)cnt) : 0.f;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
pb_gather_kernel(const float* __restrict__ x, int ldx, int N1, const int* __restrict__ N1_dev, int C, int N2, const int* __restrict__ N2_dev,
                 int K, const float* __restrict__ y, int ldy, const int* __restrict__ start, const int* __restrict__ edges,
                 const float* __restrict__ gs, int ldgs, int LQ, const float* __restrict__ colmin, const float* __restrict__ share,
                 float* __restrict__ gx, int ldgx) {
    const int n1 = d3f_dyn(N1, N1_dev), n2 = d3f_dyn(N2, N2_dev);
    const int R = 256 / LQ;
    if ((long long)blockIdx.x * R >= (long long)n1) return;
    const BnLane t = bn_lane(n1, R, LQ, C);
    const int row = t.n0 + t.r;
    if (!t.live || row >= t.n1) return;
    float xv[4], cm[4], sh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    bn_ld4<VEC>(x + (size_t)row * ldx, t.c, C, xv);
    bn_ldcol(colmin, t.c, C, 0.f, cm);
    bn_ldcol(share, t.c, C, 0.f, sh);
    // the row's segment (the table is the caller's: positions and edges are range-checked, never trusted)
    const long long items = (long long)n2 * K;
    const int lim = (int)min(items, (long long)N2 * K);
    const int s0 = min(max(start[row], 0), lim), s1 = min(max(start[row + 1], s0), lim);
    for (int p = s0; p < s1; p += 4) {                 // four (y, gs) row pairs in flight, added in edge order
        float yv[4][4], gv[4][4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = p + u < s1 ? edges[p + u] : -1;
            ok[u] = e >= 0 && e < lim;
            if (ok[u]) {
                const int i = (int)((unsigned)e / (unsigned)K);
                bn_ld4<VEC>(y + (size_t)i * ldy, t.c, C, yv[u]);
                bn_ld4<true>(gs + (size_t)i * ldgs, t.c, C, gv[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xv[j] == yv[u][j]) acc[j] += gv[u][j];
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (xv[j] == cm[j]) acc[j] += sh[j];
    bn_st4<VEC>(gx + (size_t)row * ldgx, t.c, C, acc);
}

static inline bool pb_sizes_ok(int N1, int N2, int K, int C) {
    return N1 >= 0 && N2 >= 0 && K >= 0 && C >= 1 && C <= (1 << 20) && nt_sizes_ok(N2, K);
}
static inline int pb_quad_cols(int C) { return d3f_cdiv(C, 4) * 4; }

extern "C" size_t d3f_ind_max_pool_backward_workspace_bytes(int N1, int N2, int K, int C) {
    if (!pb_sizes_ok(N1, N2, K, C)) return 0;
    const size_t sl1 = (size_t)d3f_cdiv(N1 > 0 ? N1 : 1, d3f_slice_rows(N1)), sl2 = (size_t)d3f_cdiv(N2 > 0 ? N2 : 1, d3f_slice_rows(N2));
    return d3f_align(4) + 2 * d3f_align(sl1 * C * 4) + d3f_align(sl2 * C * 8) + 2 * d3f_align((size_t)C * 4) +
           d3f_align((size_t)N2 * pb_quad_cols(C) * 4);
}

extern "C" int d3f_ind_max_pool_backward(const void* x_, int N1, int ldx, int C, const int* idx, int N2, int ld_idx, int K, const void* y_,
                                         int ldy, const float* gy, int ldg, const int* start, const int* edges, float* gx, int ldgx,
                                         const int* N1_dev, const int* N2_dev, int feat_bf16, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (feat_bf16 || !pb_sizes_ok(N1, N2, K, C) || ldx < C || ldy < C || ldg < C || ldgx < C || ld_idx < K) return D3F_ERR_ARG;
    if (N1 == 0) return D3F_OK;
    const long long items = (long long)N2 * K;
    if (!x_ || !gx || !start || (N2 > 0 && (!y_ || !gy)) || (items > 0 && (!idx || !edges))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_ind_max_pool_backward_workspace_bytes(N1, N2, K, C)) return D3F_ERR_WORKSPACE;
    const float* x = (const float*)x_;
    const float* y = (const float*)y_;
    const int S1 = d3f_slice_rows(N1), S2 = d3f_slice_rows(N2);
    const int sl1 = d3f_cdiv(N1, S1), sl2 = d3f_cdiv(N2 > 0 ? N2 : 1, S2);
    const int Cp = pb_quad_cols(C);
    // (tests/test_gpu_pool_backward.py::test_column_minimum_held_as_zeros_of_both_signs reads colmin at the offset this order gives:
    // a change of the order or of the alignment goes with a change there)
    D3fArena ar(workspace, workspace_bytes);
    unsigned* ticket = ar.take<unsigned>(1);
    unsigned* pmin = ar.take<unsigned>((size_t)sl1 * C);
    int* pcnt = ar.take<int>((size_t)sl1 * C);
    double* Spart = ar.take<double>((size_t)sl2 * C);
    float* colmin = ar.take<float>(C);
    float* share = ar.take<float>(C);
    float* gs = ar.take<float>((size_t)N2 * Cp);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const BnGeo geo = bn_geo(N1, C);       // (LQ, R and the column blocks depend on C only)
    const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldg % 4 == 0 && ldgx % 4 == 0 &&
                     (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gy | (uintptr_t)gx) & 15) == 0;
    const dim3 g1(sl1, geo.cblocks), g2(sl2, geo.cblocks), g3(d3f_cdiv(N1, geo.R), geo.cblocks);
#define PB_RUN(VEC)                                                                                                                        \
    do {                                                                                                                                   \
        pb_colmin_kernel<VEC><<<g1, 256, 0, stream>>>(x, ldx, N1, N1_dev, C, S1, geo.LQ, pmin, pcnt, ticket);                                \
        pb_row_kernel<VEC><<<g2, 256, 0, stream>>>(x, ldx, N1, N1_dev, C, idx, N2, N2_dev, ld_idx, K, y, ldy, gy, ldg, S1, S2, geo.LQ, pmin, \
                                                   pcnt, gs, Cp, Spart, ticket, colmin, share);                                            \
        pb_gather_kernel<VEC><<<g3, 256, 0, stream>>>(x, ldx, N1, N1_dev, C, N2, N2_dev, K, y, ldy, start, edges, gs, Cp, geo.LQ, colmin,   \
                                                      share, gx, ldgx);                                                                    \
    } while (0)
    if (vec) PB_RUN(true);
    else PB_RUN(false);
#undef PB_RUN
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ------------------------------------------------------------------------------------------------
// d3f_closest_pool_cat_backward: gx[j, :] = the sum of g[n, 0:C1] over the fine rows n whose first index names coarse row j, in
// ascending n -- the segment of row j in the transposed table of the ONE-column index matrix (edge e = n).
// ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256)
up_gather_kernel(const float* __restrict__ g, int ldg, int C1, const int* __restrict__ idx, int ld_idx, int N2, const int* __restrict__ N2_dev,
                 int N1, const int* __restrict__ N1_dev, const int* __restrict__ start, const int* __restrict__ edges, int LQ,
                 float* __restrict__ gx, int ldgx) {
    const int n1 = d3f_dyn(N1, N1_dev), n2 = d3f_dyn(N2, N2_dev);
    const int R = 256 / LQ;
    if ((long long)blockIdx.x * R >= (long long)n1) return;
    const BnLane t = bn_lane(n1, R, LQ, C1);
    const int row = t.n0 + t.r;
    if (!t.live || row >= t.n1) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int s0 = min(max(start[row], 0), n2), s1 = min(max(start[row + 1], s0), n2);
    for (int p = s0; p < s1; p += 4) {                 // four gradient rows in flight, added in edge order
        float v[4][4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = p + u < s1 ? edges[p + u] : -1;
            ok[u] = e >= 0 && e < n2 && idx[(size_t)e * ld_idx] == row;   // (range-checked and held against the indices, never trusted)
            if (ok[u]) bn_ld4<VEC>(g + (size_t)e * ldg, t.c, C1, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += v[u][j];
            }
    }
    bn_st4<VEC>(gx + (size_t)row * ldgx, t.c, C1, acc);
}

extern "C" int d3f_closest_pool_cat_backward(const float* g, int N2, int ldg, int C1, const int* idx, int ld_idx, int N1, const int* start,
                                             const int* edges, float* gx, int ldgx, const int* N1_dev, const int* N2_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N1 < 0 || N2 < 0 || C1 < 1 || C1 > (1 << 20) || ldg < C1 || ldgx < C1 || ld_idx < 1 || !nt_sizes_ok(N2, 1)) return D3F_ERR_ARG;
    if (N1 == 0) return D3F_OK;
    if (!gx || !start || (N2 > 0 && (!g || !idx || !edges))) return D3F_ERR_ARG;
    const BnGeo geo = bn_geo(N1, C1);
    const dim3 grid(d3f_cdiv(N1, geo.R), geo.cblocks);
    const bool vec = C1 % 4 == 0 && ldg % 4 == 0 && ldgx % 4 == 0 && (((uintptr_t)g | (uintptr_t)gx) & 15) == 0;
    if (vec) up_gather_kernel<true><<<grid, 256, 0, stream>>>(g, ldg, C1, idx, ld_idx, N2, N2_dev, N1, N1_dev, start, edges, geo.LQ, gx, ldgx);
    else up_gather_kernel<false><<<grid, 256, 0, stream>>>(g, ldg, C1, idx, ld_idx, N2, N2_dev, N1, N1_dev, start, edges, geo.LQ, gx, ldgx);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
