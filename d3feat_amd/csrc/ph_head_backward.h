// Backward of the descriptor / detection head (d3f_detect_head_backward) and the transposed neighbour table it scatters through
// (d3f_neighbor_transpose).  Included by pool_head.hip after the forward kernels: head_max_init_kernel / head_max_kernel are reused
// as they are.  The definition (tie rules, summation orders) is in include/d3feat_amd.h; nothing here uses a float atomic, and no
// workgroup waits for another.
#pragma once
#include "common.h"

// radix_sort.h defines its kernels with external linkage and grid_subsample.hip includes it too: this translation unit gets its
// own internal copies
namespace {
#include "radix_sort.h"
}

// ------------------------------------------------------------------------------------------------
// d3f_neighbor_transpose.  Edge e = i * K + k names row idx[i, k]; the table is the stable sort of the valid edges by the row they
// name.  radix_sort.h is a stable LSD sort whose pass-0 payload is the item's position, so: key = named row (shadow slots: n, the
// one key above every row, so they end up behind every valid edge), position = e.  Launches: the key kernel (keys + digit-0
// histogram + the sort's description), RS_MAX_PASSES scatter and RS_MAX_PASSES - 1 histogram launches (passes above the
// significant bits of n return at once), and one finishing kernel -- nine, whatever N, K and B are.
// ------------------------------------------------------------------------------------------------
// the keys of one tile, written once for both tables: nq rows name, rows 0 .. ns - 1 are named (the square table: nq == ns == n)
__device__ __forceinline__ void nt_keys_tile(const int* __restrict__ idx, int nq, int ns, int ld_idx, int K, RsMeta* __restrict__ meta,
                                             unsigned* __restrict__ key0, unsigned* __restrict__ hist, unsigned* sHist) {
    const int n = ns;
    const int items = nq * K;                                                   // N * K <= 2^31 - RS_TILE: checked by the launcher
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        RsMeta m;
        m.n = items;
        m.bits = n > 0 ? 32 - __clz(n) : 1;                                     // keys are 0 .. n
        m.npass = (m.bits + 7) / 8;
        m.kb = n;                                                               // (caller's field: the row count, for the finishing kernel)
        *meta = m;
    }
    const int tile = blockIdx.x;
    if ((long long)tile * RS_TILE >= (long long)items) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int base = tile * RS_TILE + w * RS_WAVE_ITEMS + lane;
    unsigned key[RS_ROUNDS], vm = 0u;
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const int pos = base + r * 64;
        key[r] = 0u;
        if (pos < items) {
            const int i = (int)((unsigned)pos / (unsigned)K), k = pos - i * K;
            const int v = idx[(size_t)i * ld_idx + k];
            key[r] = (v >= 0 && v < n) ? (unsigned)v : (unsigned)n;             // the head's shadow rule
            key0[pos] = key[r];
            vm |= 1u << r;
        }
    }
    rs_tile_histogram(key, vm, 0, sHist, hist + (size_t)tile * 256);
}

__global__ void __launch_bounds__(RS_THREADS) nt_keys_kernel(const int* __restrict__ idx, int N, int ld_idx, int K,
                                                             const int* __restrict__ lens, int B, RsMeta* __restrict__ meta,
                                                             unsigned* __restrict__ key0, unsigned* __restrict__ hist) {
    __shared__ unsigned sHist[256];
    __shared__ int sN;
    if (threadIdx.x == 0) sN = 0;
    __syncthreads();
    if ((int)threadIdx.x < B) atomicAdd(&sN, max(lens[threadIdx.x], 0));       // (integers: any order gives the same sum)
    __syncthreads();
    const int n = min(max(sN, 0), N);
    nt_keys_tile(idx, n, n, ld_idx, K, meta, key0, hist, sHist);
}

// the rectangular table (d3f_neighbor_transpose_qs): nq query rows name ns support rows, both read on the device
__global__ void __launch_bounds__(RS_THREADS) nt_keys_qs_kernel(const int* __restrict__ idx, int Nq, int ld_idx, int K,
                                                                const int* __restrict__ Nq_dev, int Ns, const int* __restrict__ Ns_dev,
                                                                RsMeta* __restrict__ meta, unsigned* __restrict__ key0,
                                                                unsigned* __restrict__ hist) {
    __shared__ unsigned sHist[256];
    nt_keys_tile(idx, max(d3f_dyn(Nq, Nq_dev), 0), max(d3f_dyn(Ns, Ns_dev), 0), ld_idx, K, meta, key0, hist, sHist);
}

// thread t < items: sorted position t -> edges[t] (valid edges only; they come first).  thread j <= N: start[j] = the first sorted
// position whose key is >= min(j, n), by bisection -- no atomic, no scan, rows nobody names included.
__global__ void __launch_bounds__(256) nt_finish_kernel(const RsMeta* __restrict__ meta, int N, const unsigned* __restrict__ key0,
                                                        const unsigned* __restrict__ key1, const unsigned* __restrict__ val0,
                                                        const unsigned* __restrict__ val1, int* __restrict__ start,
                                                        int* __restrict__ edges) {
    const int items = meta->n, n = meta->kb;
    const bool odd = meta->npass & 1;
    const unsigned* __restrict__ sk = odd ? key1 : key0;
    const unsigned* __restrict__ sv = odd ? val1 : val0;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < items && sk[t] < (unsigned)n) edges[t] = (int)sv[t];
    if (t <= N) {
        const unsigned target = (unsigned)min((int)t, n);
        int lo = 0, hi = items;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (sk[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        start[t] = lo;
    }
}

// the sort (and nt_keys_kernel) addresses whole RS_TILE-slot tiles with int positions: the last tile must end below 2^31
static inline bool nt_sizes_ok(int N, int K) { return N >= 0 && K >= 0 && (long long)N * K <= (1ll << 31) - RS_TILE; }

extern "C" size_t d3f_neighbor_transpose_workspace_bytes(int N, int K) {
    if (!nt_sizes_ok(N, K)) return 0;
    const size_t items = (size_t)N * K;
    return 4 * d3f_align(items * 4) + d3f_align(rs_hist_words((int)items) * 4) + d3f_align(sizeof(RsMeta));
}

// the sort and the finishing kernel behind a key kernel: shared by both tables.  rows: the capacity of the named side (start has
// rows + 1 entries); items: the slots of the index matrix
struct NtBuffers {
    unsigned *key0, *key1, *val0, *val1, *hist;
    RsMeta* meta;
};
static inline bool nt_take(D3fArena& ar, int items, NtBuffers& b) {
    b.key0 = ar.take<unsigned>(items);
    b.key1 = ar.take<unsigned>(items);
    b.val0 = ar.take<unsigned>(items);
    b.val1 = ar.take<unsigned>(items);
    b.hist = ar.take<unsigned>(rs_hist_words(items));
    b.meta = ar.take<RsMeta>(1);
    return ar.ok;
}
static inline int nt_sort_finish(const NtBuffers& b, int items, int rows, int* start, int* edges, hipStream_t stream) {
    const int rc = rs_sort_launch(b.meta, items, b.key0, b.key1, b.val0, b.val1, b.hist, stream);
    if (rc != D3F_OK) return rc;
    const long long threads = items > rows + 1 ? (long long)items : (long long)rows + 1;
    nt_finish_kernel<<<d3f_cdiv(threads, 256), 256, 0, stream>>>(b.meta, rows, b.key0, b.key1, b.val0, b.val1, start, edges);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

extern "C" int d3f_neighbor_transpose(const int* idx, int N, int ld_idx, int K, const int* lens_dev, int B, int* start, int* edges,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!nt_sizes_ok(N, K) || ld_idx < K || B < 1 || B > D3F_MAX_BATCH) return D3F_ERR_ARG;
    const int items = N * K;
    if (!start || !lens_dev || (items > 0 && (!edges || !idx))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_neighbor_transpose_workspace_bytes(N, K)) return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    NtBuffers b;
    if (!nt_take(ar, items, b)) return D3F_ERR_WORKSPACE;
    nt_keys_kernel<<<rs_tiles(items), RS_THREADS, 0, stream>>>(idx, N, ld_idx, K, lens_dev, B, b.meta, b.key0, b.hist);
    D3F_LAUNCH_CHECK();
    return nt_sort_finish(b, items, N, start, edges, stream);
}

extern "C" int d3f_neighbor_transpose_qs(const int* idx, int Nq, int ld_idx, int K, const int* Nq_dev, int Ns, const int* Ns_dev,
                                         int* start, int* edges, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!nt_sizes_ok(Nq, K) || Ns < 0 || ld_idx < K) return D3F_ERR_ARG;
    const int items = Nq * K;
    if (!start || (items > 0 && (!edges || !idx))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_neighbor_transpose_workspace_bytes(Nq, K)) return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    NtBuffers b;
    if (!nt_take(ar, items, b)) return D3F_ERR_WORKSPACE;
    nt_keys_qs_kernel<<<rs_tiles(items), RS_THREADS, 0, stream>>>(idx, Nq, ld_idx, K, Nq_dev, Ns, Ns_dev, b.meta, b.key0, b.hist);
    D3F_LAUNCH_CHECK();
    return nt_sort_finish(b, items, Ns, start, edges, stream);
}

// ------------------------------------------------------------------------------------------------
// d3f_detect_head_backward: four launches behind the two per-cloud maximum launches of the forward.
//   A  hb_row_kernel     recomputes the row's forward (the arithmetic of head_kernel), writes the row's own terms of gy, gS[i, :] =
//                        -g_d / num_i, and the row's count of entries equal to m_b
//   B  hb_gather_kernel  gy[j, :] += the gS rows of row j's segment of the transposed table, one fp32 chain per channel in edge
//                        order; the row's float64 partial of sum_c gy * y
//   C  hb_cloud_kernel   one workgroup per cloud: the fixed float64 tree over the partials, the tie count, gden_b / ties
//   D  hb_finish_kernel  gx = gy / den_b + the tie share + the backward of the L2 normalisation
// One half-wave per row, lane l holds channels l, l + 32, ... (CPL of them), as head_kernel<CPL>.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int hb_half_sum_i(int v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float hb_half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float hb_half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int CPL>
__global__ void __launch_bounds__(256)
hb_row_kernel(const float* __restrict__ x, int N, int ldx, int C, const int* __restrict__ idx, int ld_idx, int K,
              const int* __restrict__ offs, int B, const unsigned* __restrict__ mx, const float* __restrict__ gscore, int ldgs,
              float* __restrict__ gS, float* __restrict__ gy, int* __restrict__ cntm) {
    N = min(N, offs[B]);
    if ((int)(blockIdx.x * 8) >= N) return;
    const int half = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const bool active = half < N;
    const int n = active ? half : 0;
    const int b = d3f_find_elem(offs, B, n);
    const float m = d3f_ord2f(mx[b]);
    const float den = m + 1e-6f;
    float xv[CPL], yv[CPL], sum[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = l + 32 * j;
        xv[j] = (c < C) ? x[(size_t)n * ldx + c] : 0.f;
        yv[j] = xv[j] / den;
        sum[j] = 0.f;
    }
    // the neighbour sum and the count of rows with a non-zero sum: head_kernel's loop, operation for operation
    int cnt = 0;
    const int hbase = threadIdx.x & 32;
    for (int k0 = 0; k0 < K; k0 += 32) {
        const int mine = (k0 + l < K) ? idx[(size_t)n * ld_idx + k0 + l] : -1;
        const int kn = min(32, K - k0);
        for (int kk = 0; kk < kn; kk += 4) {
            int id[4];
            float dn[4];
            float v[4][CPL];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                id[j] = __shfl(mine, hbase + min(kk + j, 31), 64);
                if (kk + j >= kn || id[j] < 0 || id[j] >= N) id[j] = -1;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dn[j] = 1.f;
                if (id[j] >= 0) dn[j] = d3f_ord2f(mx[d3f_find_elem(offs, B, id[j])]) + 1e-6f;
#pragma unroll
                for (int jj = 0; jj < CPL; ++jj) {
                    const int c = l + 32 * jj;
                    v[j][jj] = (id[j] >= 0 && c < C) ? x[(size_t)id[j] * ldx + c] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float rs = 0.f;
#pragma unroll
                for (int jj = 0; jj < CPL; ++jj) {
                    const float y = v[j][jj] / dn[j];
                    sum[jj] += y;
                    rs += y;
                }
                rs = hb_half_sum(rs);
                cnt += (id[j] >= 0 && rs != 0.f) ? 1 : 0;
            }
        }
    }
    const float fc = (float)max(cnt, 1);
    float ymax = -3.402823466e38f;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
        if (l + 32 * j < C) ymax = fmaxf(ymax, yv[j]);
    ymax = hb_half_max(ymax);
    const float w1 = 1e-6f + ymax;
    float alpha[CPL], beta[CPL], a[CPL], sig[CPL];
    float best = -3.402823466e38f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const float d = yv[j] - sum[j] / fc;
        float sp;
        if (d > 15.f) sp = d;
        else if (d < -15.f) sp = expf(d);
        else sp = log1pf(expf(d));
        alpha[j] = sp;
        sig[j] = 1.f / (1.f + expf(-d));
        beta[j] = yv[j] / w1;
        a[j] = sp * beta[j];
        if (l + 32 * j < C) best = fmaxf(best, a[j]);
    }
    best = hb_half_max(best);
    int nT = 0, nW = 0, nM = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        if (l + 32 * j < C) {
            nT += a[j] == best ? 1 : 0;
            nW += yv[j] == ymax ? 1 : 0;
            nM += xv[j] == m ? 1 : 0;
        }
    }
    nT = hb_half_sum_i(nT);
    nW = hb_half_sum_i(nW);
    nM = hb_half_sum_i(nM);
    const float gs = gscore ? gscore[(size_t)n * ldgs] : 0.f;
    const float gt = gs / (float)max(nT, 1);
    float gd[CPL], gb[CPL];
    float gwp = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const float ga = (l + 32 * j < C && a[j] == best) ? gt : 0.f;
        gd[j] = ga * beta[j] * sig[j];
        gb[j] = ga * alpha[j];
        gwp += gb[j] * yv[j];
    }
    gwp = hb_half_sum(gwp);
    const float gw = -gwp / (w1 * w1);
    const float gwt = gw / (float)max(nW, 1);
    if (active) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = l + 32 * j;
            if (c < C) {
                float g = gd[j] + gb[j] / w1;
                if (yv[j] == ymax) g += gwt;
                gy[(size_t)n * C + c] = g;
                gS[(size_t)n * C + c] = -gd[j] / fc;
            }
        }
        if (l == 0) cntm[n] = nM;
    }
}

template <int CPL>
__global__ void __launch_bounds__(256)
hb_gather_kernel(const float* __restrict__ x, int N, int ldx, int C, int K, const int* __restrict__ offs, int B,
                 const unsigned* __restrict__ mx, const int* __restrict__ start, const int* __restrict__ edges,
                 const float* __restrict__ gS, float* __restrict__ gy, double* __restrict__ part) {
    N = min(N, offs[B]);
    if ((int)(blockIdx.x * 8) >= N) return;
    const int half = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const bool active = half < N;
    const int n = active ? half : 0;
    const float den = d3f_ord2f(mx[d3f_find_elem(offs, B, n)]) + 1e-6f;
    float acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
    // row n's segment (the table is the caller's: positions and edges are range-checked, never trusted)
    const int items = N * K;
    const int s0 = min(max(start[n], 0), items), s1 = min(max(start[n + 1], s0), items);
    const int hbase = threadIdx.x & 32;
    for (int p0 = s0; p0 < s1; p0 += 32) {
        const int mine = (p0 + l < s1) ? edges[p0 + l] : -1;      // 32 edges per half-wave load
        const int kn = min(32, s1 - p0);
        for (int q = 0; q < kn; q += 4) {                          // four gS rows in flight, added in edge order
            float v[4][CPL];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = __shfl(mine, hbase + min(q + u, 31), 64);
                int i = -1;
                if (q + u < kn && e >= 0 && e < items) i = (int)((unsigned)e / (unsigned)K);
#pragma unroll
                for (int jj = 0; jj < CPL; ++jj) {
                    const int c = l + 32 * jj;
                    v[u][jj] = (i >= 0 && c < C) ? gS[(size_t)i * C + c] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int jj = 0; jj < CPL; ++jj) acc[jj] += v[u][jj];
        }
    }
    double ps = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = l + 32 * j;
        if (c < C) {
            const float g = gy[(size_t)n * C + c] + acc[j];
            const float y = x[(size_t)n * ldx + c] / den;
            if (active) gy[(size_t)n * C + c] = g;
            ps += (double)g * (double)y;
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
    if (active && l == 0) part[n] = ps;
}

// one workgroup per cloud.  Thread t adds the partials of the cloud's rows t, t + 256, ... (counted from the cloud's first row) in
// ascending order, then the 256 sums are halved 128, 64, ..., 1 (sum[t] += sum[t + o]): a tree that depends on the cloud's length only.
__global__ void __launch_bounds__(256) hb_cloud_kernel(int N, int C, const int* __restrict__ lens, const int* __restrict__ include_zero_dev,
                                                       int group, const int* __restrict__ offs, int B, const unsigned* __restrict__ mx,
                                                       const double* __restrict__ part, const int* __restrict__ cntm,
                                                       float* __restrict__ share) {
    __shared__ double sD[256];
    __shared__ long long sC[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int lo = min(offs[b], N), hi = min(offs[b + 1], N);
    double s = 0.0;
    long long c = 0;
    for (int i = lo + t; i < hi; i += 256) {
        s += part[i];
        c += cntm[i];
    }
    sD[t] = s;
    sC[t] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            sD[t] += sD[t + o];
            sC[t] += sC[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        // pad slots of the cloud's row of in_batches (datasets/common.py:453-496): longest - len, plus one when all clouds of the
        // stack (or group) are equally long; every slot gathers a zero ROW of C entries
        int pads;
        if (include_zero_dev) pads = max(include_zero_dev[b], 0);
        else {
            const int g = group > 0 ? group : B;
            const int g0 = b / g * g, g1 = min(g0 + g, B);
            int longest = 0, all_eq = 1;
            for (int j = g0; j < g1; ++j) longest = max(longest, lens[j]);
            for (int j = g0; j < g1; ++j) all_eq &= (lens[j] == longest);
            pads = longest - lens[b] + all_eq;
        }
        const float m = d3f_ord2f(mx[b]);
        long long ties = sC[0];
        if (pads > 0 && m == 0.f) ties += (long long)pads * C;
        const double gden = -sD[0] / (double)(m + 1e-6f);
        share[b] = ties > 0 ? (float)(gden / (double)ties) : 0.f;
    }
}

template <int CPL>
__global__ void __launch_bounds__(256)
hb_finish_kernel(const float* __restrict__ x, int N, int ldx, int C, const int* __restrict__ offs, int B,
                 const unsigned* __restrict__ mx, const float* __restrict__ gy, const float* __restrict__ share,
                 const float* __restrict__ gdesc, int ldg, float* __restrict__ gx, int ldgx) {
    N = min(N, offs[B]);
    if ((int)(blockIdx.x * 8) >= N) return;
    const int half = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const bool active = half < N;
    const int n = active ? half : 0;
    const int b = d3f_find_elem(offs, B, n);
    const float m = d3f_ord2f(mx[b]);
    const float den = m + 1e-6f;
    const float sh = share[b];
    float xv[CPL], g[CPL], out[CPL];
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = l + 32 * j;
        xv[j] = (c < C) ? x[(size_t)n * ldx + c] : 0.f;
        g[j] = (c < C && gdesc) ? gdesc[(size_t)n * ldg + c] : 0.f;
        out[j] = (c < C) ? gy[(size_t)n * C + c] / den : 0.f;
        if (xv[j] == m) out[j] += sh;
        sq += xv[j] * xv[j];
    }
    sq = hb_half_sum(sq);
    if (gdesc) {
        if (sq >= 1e-10f) {
            const float inv = rsqrtf(sq);
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < CPL; ++j) dot += (xv[j] * inv) * g[j];
            dot = hb_half_sum(dot);
#pragma unroll
            for (int j = 0; j < CPL; ++j) out[j] += inv * (g[j] - (xv[j] * inv) * dot);
        } else {
            const float inv = rsqrtf(1e-10f);
#pragma unroll
            for (int j = 0; j < CPL; ++j) out[j] += g[j] * inv;
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (l + 32 * j < C) gx[(size_t)n * ldgx + l + 32 * j] = out[j];
    }
}

static inline bool hb_sizes_ok(int N, int C, int B) { return N >= 0 && C >= 1 && C <= 128 && B >= 1 && B <= D3F_MAX_BATCH; }

extern "C" size_t d3f_detect_head_backward_workspace_bytes(int N, int C, int B) {
    if (!hb_sizes_ok(N, C, B)) return 0;
    const size_t rows = (size_t)N * C * 4;
    return d3f_align((size_t)(2 * B + 1) * 4) + 2 * d3f_align(rows) + d3f_align((size_t)N * 8) + d3f_align((size_t)N * 4) +
           d3f_align((size_t)B * 4);
}

extern "C" int d3f_detect_head_backward(const float* x, int N, int ldx, int C, const int* idx, int ld_idx, int K, const int* lens_dev,
                                        const int* include_zero_dev, int stack_group, int B, const int* start, const int* edges,
                                        const float* gdesc, int ldg, const float* gscore, int ldgs, float* gx, int ldgx,
                                        void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!hb_sizes_ok(N, C, B) || ldx < C || ldgx < C || K < 0 || ld_idx < K || stack_group < 0 || !nt_sizes_ok(N, K) ||
        (gdesc && ldg < C) || (gscore && ldgs < 1))
        return D3F_ERR_ARG;
    if (N == 0) return D3F_OK;
    if (!x || !lens_dev || !start || !gx || (K > 0 && (!idx || !edges))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_detect_head_backward_workspace_bytes(N, C, B)) return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    int* scratch = ar.take<int>(2 * B + 1);
    float* gS = ar.take<float>((size_t)N * C);
    float* gy = ar.take<float>((size_t)N * C);
    double* part = ar.take<double>(N);
    int* cntm = ar.take<int>(N);
    float* share = ar.take<float>(B);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    unsigned* mx = (unsigned*)scratch;  // [B]
    int* offs = scratch + B;            // [B+1]
    // the per-cloud maxima: the forward's two launches, as d3f_detect_head issues them
    head_max_init_kernel<<<1, 256, 0, stream>>>(lens_dev, include_zero_dev, stack_group, B, mx, offs);
    int chunks = d3f_cdiv((long long)N * C, 256 * 16);
    const int fill = d3f_cdiv(512, B);
    if (chunks > fill) chunks = fill;
    if (chunks < 1) chunks = 1;
    if (ldx == C && C % 4 == 0 && ((uintptr_t)x & 15) == 0) head_max_kernel<true><<<dim3(chunks, B), 256, 0, stream>>>(x, N, ldx, C, offs, B, mx);
    else head_max_kernel<false><<<dim3(chunks, B), 256, 0, stream>>>(x, N, ldx, C, offs, B, mx);
    const int blocks = d3f_cdiv((long long)N * 32, 256);
#define HB_ROWS(CPL)                                                                                                                     \
    do {                                                                                                                                 \
        hb_row_kernel<CPL><<<blocks, 256, 0, stream>>>(x, N, ldx, C, idx, ld_idx, K, offs, B, mx, gscore, ldgs, gS, gy, cntm);            \
        hb_gather_kernel<CPL><<<blocks, 256, 0, stream>>>(x, N, ldx, C, K, offs, B, mx, start, edges, gS, gy, part);                      \
        hb_cloud_kernel<<<B, 256, 0, stream>>>(N, C, lens_dev, include_zero_dev, stack_group, offs, B, mx, part, cntm, share);            \
        hb_finish_kernel<CPL><<<blocks, 256, 0, stream>>>(x, N, ldx, C, offs, B, mx, gy, share, gdesc, ldg, gx, ldgx);                    \
    } while (0)
    if (C <= 32) HB_ROWS(1);
    else if (C <= 64) HB_ROWS(2);
    else HB_ROWS(4);
#undef HB_ROWS
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
