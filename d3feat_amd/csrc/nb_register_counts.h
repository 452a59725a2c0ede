// RANSAC registration of every pair at every keypoint count, the half that walks the cell grid (d3f_register_pairs_counts; the other
// half and the entry point: rp_register_counts.h in registration.hip).  (included by radius_neighbors.hip; the metric of every search:
// d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA, strict d2 < r2, ties by the smaller index.)
//
// d3f_register_pairs stages both blocks of a pair in LDS arrays of D3F_PAIRS_KMAX rows and finds the nearest target point by brute
// force; here the blocks stay in memory and ONE grid serves every pair and every count:
//   rc_gather_kernel   the xyz of the last min(count, rows) rows of every block, rows = min(K, largest count), stacked block after
//                      block in row order, and the lengths on the device -- the input of d3f_neighbor_grid_build with B = n_blocks
//   (grid build)       five launches of d3f_neighbor_grid_build, radius = max_correspondence_distance
//   rc_score_kernel    workgroup = (RC_SLICE validated hypotheses, count, pair): the hypotheses in LDS, a thread per source row, the
//                      27-cell stencil of the target's element walked as nine runs whose 18 bounds are fetched together; hits and the
//                      fixed-point sum of d2 reduced per wavefront, then integer LDS atomics; one writer per (pair, count, hypothesis)
//   rc_select_kernel   workgroup = (count, pair): largest count, then smallest sumd2, then earliest iteration; the winner's nearest
//                      target row of every source row through the same walk
// ONE GRID, EVERY COUNT.  Element b of the grid holds the n_max = min(count_b, rows) last rows of block b, record index i = row
// count_b - n_max + i.  Count k uses the last n_k = min(count_b, k) <= n_max of them: the records with i >= n_max - n_k, and the row
// that register_keypoints numbers j at count k is the record i = j + (n_max - n_k).  Skipping the records below the shift leaves
// exactly the rows of count k; the shift is the same for all of them, so (d2, i) orders them as (d2, j) does: the minimum is the same
// row, and i - shift is its number at count k.
#pragma once
#include "rc_shared.h"

#define RC_SLICE 16   // validated hypotheses per workgroup of rc_score_kernel

__global__ void __launch_bounds__(256) rc_gather_kernel(const float* __restrict__ kp, int K, int ld, const int* __restrict__ count, int rows,
                                                        float* __restrict__ stack, int* __restrict__ lens) {
    const int b = blockIdx.y;
    int off = 0;
    for (int j = 0; j < b; ++j) off += min(min(max(count[j], 0), K), rows);
    const int cb = min(max(count[b], 0), K), n = min(cb, rows);
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[b] = n;
    const float* src = kp + ((size_t)b * K + (cb - n)) * ld;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) stack[3 * (size_t)(off + r) + d] = src[(size_t)r * ld + d];
    }
}

// block pairs[p][which] at count kc: its element of the grid, the first record the count uses (in the numbering of the stack) and
// the rows it uses; no rows for an index outside [0, B) (rp_rows)
struct RcBlock { int blk, first, n; };
__device__ __forceinline__ RcBlock rc_block(const int* __restrict__ soffs, const int* __restrict__ pairs, int p, int which, int B, int kc) {
    RcBlock r{0, 0, 0};
    const int b = pairs[2 * (size_t)p + which];
    if (b < 0 || b >= B) return r;
    const int lo = soffs[b], len = soffs[b + 1] - lo;
    r.blk = b;
    r.n = min(len, kc);
    r.first = lo + (len - r.n);
    return r;
}

// the nearest record of element e strictly inside r2 among those with stack index >= first, by (d2, index); its index minus
// `first`, -1 for none.  The walk of nb_overlap_kernel.
__device__ __forceinline__ int rc_nearest(const NbElem& e, const int* __restrict__ cell_start, const int* __restrict__ cell_base,
                                          const float4* __restrict__ sorted, int first, float qx, float qy, float qz, float r2, float& bd2) {
    bd2 = 3.4e38f;
    int bidx = -1;
    int cx, cy, cz;
    nb_cell_of(e, qx, qy, qz, cx, cy, cz);
    cx = min(max(cx, -2), e.dims[0] + 1);
    cy = min(max(cy, -2), e.dims[1] + 1);
    cz = min(max(cz, -2), e.dims[2] + 1);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, e.dims[0] - 1);
    if (x0 > x1) return -1;
    // the 18 bounds of the nine (y, z) rows in one round trip, then the walks
    int rlo[9], rhi[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int y = cy + (j % 3) - 1, z = cz + (j / 3) - 1;
        rlo[j] = rhi[j] = 0;
        if (y >= 0 && y < e.dims[1] && z >= 0 && z < e.dims[2]) {
            const int rowbase = e.cbase + e.dims[0] * (y + e.dims[1] * z);
            rlo[j] = d3f_scan_at(cell_start, cell_base, rowbase + x0);
            rhi[j] = d3f_scan_at(cell_start, cell_base, rowbase + x1 + 1);
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        for (int t = rlo[j]; t < rhi[j]; ++t) {
            const float4 sp = sorted[t];
            const float d2 = rc_d2(qx, qy, qz, sp.x, sp.y, sp.z);
            const int si = __float_as_int(sp.w) - first;               // < 0: a row this count does not use
            if (si >= 0 && d2 < r2 && (d2 < bd2 || (d2 == bd2 && si < bidx))) { bd2 = d2; bidx = si; }
        }
    }
    return bidx;
}

// grid (slices of RC_SLICE hypotheses, counts, pairs).  cnt / sd2 [P, n, max_validation]: every entry that rc_select_kernel reads has
// exactly one writer.
__global__ void __launch_bounds__(256) rc_score_kernel(const NbElem* __restrict__ el, const int* __restrict__ soffs,
                                                       const int* __restrict__ cell_start, const int* __restrict__ cell_base,
                                                       const float4* __restrict__ sorted, const float* __restrict__ stack, int B,
                                                       const int* __restrict__ pairs, int P, RcCounts prm, RcLists L, float r2) {
    __shared__ float M[RC_SLICE * 12];
    __shared__ int c_l[RC_SLICE];
    __shared__ unsigned long long s_l[RC_SLICE];
    const int c = blockIdx.y, v0 = blockIdx.x * RC_SLICE, kc = prm.k[c];
    for (int p = blockIdx.z; p < P; p += gridDim.z) {
        const size_t pc = (size_t)p * prm.n + c;
        const int nv = min(L.validations[pc] - v0, RC_SLICE);
        if (nv <= 0) continue;                                           // the whole workgroup
        const RcBlock a = rc_block(soffs, pairs, p, 0, B, kc), b = rc_block(soffs, pairs, p, 1, B, kc);
        __syncthreads();                                                 // the previous pair's sums have been stored
        if ((int)threadIdx.x < nv * 12) M[threadIdx.x] = L.Tlist[(pc * L.max_validation + v0) * 12 + threadIdx.x];
        if (threadIdx.x < RC_SLICE) { c_l[threadIdx.x] = 0; s_l[threadIdx.x] = 0ull; }
        __syncthreads();
        const NbElem e = el[b.blk];
        const float* S = stack + 3 * (size_t)a.first;
        for (int i0 = 0; i0 < a.n; i0 += 256) {
            const int i = i0 + threadIdx.x;
            const bool live = i < a.n;
            const float sx = live ? S[3 * (size_t)i] : 0.f, sy = live ? S[3 * (size_t)i + 1] : 0.f, sz = live ? S[3 * (size_t)i + 2] : 0.f;
            for (int v = 0; v < nv; ++v) {
                bool hit = false;
                unsigned long long add = 0ull;
                if (live) {
                    float qx, qy, qz, bd2;
                    rc_apply(M + 12 * v, sx, sy, sz, qx, qy, qz);
                    if (rc_nearest(e, cell_start, cell_base, sorted, b.first, qx, qy, qz, r2, bd2) >= 0) {
                        hit = true;
                        add = (unsigned long long)((double)bd2 * 4294967296.0);
                    }
                }
                // per wavefront, then one LDS atomic each (integers: independent of the order of arrival)
                const int hits = __popcll(__ballot(hit));
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) add += __shfl_xor(add, o, 64);
                if ((threadIdx.x & 63) == 0 && hits) {
                    atomicAdd(&c_l[v], hits);
                    atomicAdd(&s_l[v], add);
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < nv) {
            L.cnt[pc * L.max_validation + v0 + threadIdx.x] = c_l[threadIdx.x];
            L.sd2[pc * L.max_validation + v0 + threadIdx.x] = s_l[threadIdx.x];
        }
    }
}

// grid (counts, pairs)
__global__ void __launch_bounds__(256) rc_select_kernel(const NbElem* __restrict__ el, const int* __restrict__ soffs,
                                                        const int* __restrict__ cell_start, const int* __restrict__ cell_base,
                                                        const float4* __restrict__ sorted, const float* __restrict__ stack, int B,
                                                        const int* __restrict__ pairs, int P, RcCounts prm, RcLists L, float r2, RcOut out) {
    __shared__ RcBest red[256];
    __shared__ float M[12];
    const int c = blockIdx.x, kc = prm.k[c];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const size_t pc = (size_t)p * prm.n + c;
        const int V = L.validations[pc];
        RcBest me{-1, ~0ull, 0x7fffffff};
        for (int v = threadIdx.x; v < V; v += 256) {
            const RcBest x{L.cnt[pc * L.max_validation + v], L.sd2[pc * L.max_validation + v], v};
            if (rc_better(x, me)) me = x;
        }
        const RcBest w = rc_block_best(me, red);                         // (its first barrier: the previous pair is done with red and M)
        int* near = out.nearest ? out.nearest + (size_t)p * prm.total + prm.off[c] : nullptr;
        if (V <= 0) {   // nothing validated: the identity, no correspondences
            rc_store_none(out.T_out + pc * 12, out.inliers + pc, out.sumd2 + pc, out.best_iteration + pc);
            if (near)
                for (int i = threadIdx.x; i < kc; i += 256) near[i] = -1;
            continue;
        }
        if (threadIdx.x < 12) out.T_out[pc * 12 + threadIdx.x] = M[threadIdx.x] = L.Tlist[(pc * L.max_validation + w.v) * 12 + threadIdx.x];
        if (threadIdx.x == 0) { out.inliers[pc] = w.c; out.sumd2[pc] = w.s; out.best_iteration[pc] = L.itlist[pc * L.max_validation + w.v]; }
        __syncthreads();
        if (!near) continue;
        const RcBlock a = rc_block(soffs, pairs, p, 0, B, kc), b = rc_block(soffs, pairs, p, 1, B, kc);
        const NbElem e = el[b.blk];
        const float* S = stack + 3 * (size_t)a.first;
        for (int i = threadIdx.x; i < kc; i += 256) {
            int j = -1;
            if (i < a.n) {
                float qx, qy, qz, bd2;
                rc_apply(M, S[3 * (size_t)i], S[3 * (size_t)i + 1], S[3 * (size_t)i + 2], qx, qy, qz);
                j = rc_nearest(e, cell_start, cell_base, sorted, b.first, qx, qy, qz, r2, bd2);
            }
            near[i] = j;
        }
    }
}

static inline size_t rc_stack_rows(int n_blocks, int rows) { return (size_t)(n_blocks > 0 ? n_blocks : 1) * (size_t)(rows > 0 ? rows : 1); }

size_t nb_rc_workspace_bytes(int n_blocks, int rows) {
    const size_t ns = rc_stack_rows(n_blocks, rows);
    return d3f_align(ns * 3 * sizeof(float)) + d3f_align((size_t)n_blocks * sizeof(int)) + d3f_neighbor_grid_bytes((int)ns, n_blocks) + 256;
}

int nb_rc_score_select(const float* kp, int n_blocks, int K, int ld, const int* count_dev, const int* pairs_dev, int P, const RcCounts& prm,
                       int rows, float radius, const RcLists& lists, const RcOut& out, void* workspace, size_t workspace_bytes,
                       hipStream_t stream) {
    if (n_blocks < 1 || n_blocks > D3F_MAX_BATCH || rows < 1 || rows > K || P < 1) return D3F_ERR_ARG;
    const size_t ns = rc_stack_rows(n_blocks, rows);
    D3fArena ar(workspace, workspace_bytes);
    float* stack = ar.take<float>(ns * 3);
    int* lens = ar.take<int>(n_blocks);
    const size_t gb = d3f_neighbor_grid_bytes((int)ns, n_blocks);
    char* grid = ar.take<char>(gb);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    rc_gather_kernel<<<dim3(d3f_cdiv(rows, 256), n_blocks), 256, 0, stream>>>(kp, K, ld, count_dev, rows, stack, lens);
    D3F_LAUNCH_CHECK();
    const float r = radius > 0.f ? radius : 0.f;                        // radius <= 0: nothing was validated, the grid is not walked
    int rc = d3f_neighbor_grid_build(stack, (int)ns, lens, n_blocks, r, grid, gb, stream);
    if (rc != D3F_OK) return rc;
    NbGrid g = nb_carve(grid, gb, (int)ns, n_blocks);
    if (!g.ok) return D3F_ERR_WORKSPACE;
    const int pz = P < 65535 ? P : 65535;
    rc_score_kernel<<<dim3(d3f_cdiv(lists.max_validation, RC_SLICE), prm.n, pz), 256, 0, stream>>>(g.el, g.soffs, g.cell_start, g.stmp, g.sorted,
                                                                                                  stack, n_blocks, pairs_dev, P, prm, lists, r * r);
    rc_select_kernel<<<dim3(prm.n, pz), 256, 0, stream>>>(g.el, g.soffs, g.cell_start, g.stmp, g.sorted, stack, n_blocks, pairs_dev, P, prm,
                                                          lists, r * r, out);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
