// The optimiser's step of every variable in one call: weight decay folded into the gradient, the per-variable clip by norm, the momentum
// accumulator and the update (d3f_momentum_sgd), with the host-side chunk table (d3f_momentum_sgd_plan).  Included by pool_head.hip
// behind ph_pool_backward.h.  The definition, the roundings and the summation orders are in include/d3feat_amd.h; nothing here uses an
// atomic on float data, and two calls give equal bits.
//
// Work is cut into CHUNKS of D3F_SGD_CHUNK elements of ONE variable (the table: (variable, first element) per chunk; a variable's chunks
// are contiguous and ascending).  One workgroup of 256 threads per chunk in both launches; thread t holds the QUADS t, t + 256, ... of
// its chunk (quad q = elements 4 q .. 4 q + 3 of the chunk).  A quad is one 16-byte access when v, g and a of the variable are all
// 16-byte aligned and the quad lies inside the variable, four guarded 4-byte accesses otherwise: the same elements in the same threads
// on both paths, so no sum depends on the path.
//
//   1  sgd_norm_kernel     per chunk the float64 partials of S = sum g1^2 and, on a decayed variable, of R = sum 0.5 v^2: a thread's
//                          chain over its elements in ascending order from 0.0, the wave tree acc += shfl_down(acc, s), s = 32 .. 1, the
//                          tree over the four waves red[w] += red[w + s], s = 2, 1.  A chunk of a skipped variable writes zeros: every
//                          partial is written by every call, the workspace's bytes before the call do not matter.
//   2  sgd_update_kernel   every workgroup adds the partials of ITS variable in chunk order (staged through LDS in tiles, added by one
//                          thread), takes n and s, and updates its chunk; workgroup 0 also adds the partials of R in table order and
//                          writes the regularisation loss.
// (A middle launch, one workgroup per variable, would spare the chunks of a long variable the re-adding: 960 float64 adds out of LDS
// for the largest variable of the shipped architecture, against a launch of its own for about a hundred variables of one chunk.)
#pragma once
#include "common.h"

static_assert(D3F_SGD_CHUNK % 1024 == 0, "a chunk is a whole number of quads per thread");
static_assert(sizeof(d3f_sgd_var) == 32, "the descriptor is built as four 64-bit words by the callers");
#define SGD_QUADS (D3F_SGD_CHUNK / 1024)      // quads per thread
#define SGD_TILE 1024                         // partials staged at a time

// The chunk's variable and place, range-checked: the tables are the caller's and are never trusted.  -> false: nothing to do here.
struct SgdChunk {
    d3f_sgd_var d;
    int begin, n, first, nt;      // first element, elements of this chunk, the variable's first chunk, its number of chunks
    bool vec;
};
__device__ __forceinline__ bool sgd_chunk(const d3f_sgd_var* __restrict__ desc, int T, const int* __restrict__ chunks, int nchunks, int c,
                                          SgdChunk& k) {
    const int t = chunks[2 * c], b = chunks[2 * c + 1];
    if (t < 0 || t >= T || b < 0 || (b % D3F_SGD_CHUNK) != 0) return false;
    k.d = desc[t];
    if (!k.d.g || !k.d.v || !k.d.a || b >= k.d.count) return false;         // (a NULL gradient: the variable is skipped whole)
    k.begin = b;
    k.n = min(D3F_SGD_CHUNK, k.d.count - b);
    k.nt = (int)(((long long)k.d.count + D3F_SGD_CHUNK - 1) / D3F_SGD_CHUNK);
    k.first = c - b / D3F_SGD_CHUNK;
    k.vec = ((((uintptr_t)k.d.v) | ((uintptr_t)k.d.g) | ((uintptr_t)k.d.a)) & 15) == 0;
    return k.first >= 0 && (long long)k.first + k.nt <= (long long)nchunks;
}

// elements e .. e + 3 of a chunk of n elements; beyond n: zeros
template <bool VEC>
__device__ __forceinline__ void sgd_ld4(const float* p, int e, int n, float v[4]) {
    if (VEC && e + 4 <= n) {
        const float4 f = *(const float4*)(p + e);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (e + j < n) ? p[e + j] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void sgd_st4(float* p, int e, int n, const float v[4]) {
    if (VEC && e + 4 <= n) {
        *(float4*)(p + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < n) p[e + j] = v[j];
    }
}
// g1: the gradient with the decay's folded in, each operation rounded on its own
__device__ __forceinline__ float sgd_g1(float g, float v, float wd, int decay) { return decay ? __fadd_rn(g, __fmul_rn(wd, v)) : g; }

template <bool VEC>
__device__ __forceinline__ void sgd_chunk_sums(const SgdChunk& k, float wd, double& S, double& R) {
    const float* g = k.d.g + k.begin;
    const float* v = k.d.v + k.begin;
    float gv[SGD_QUADS][4], vv[SGD_QUADS][4];
#pragma unroll
    for (int q = 0; q < SGD_QUADS; ++q) {                  // every load requested before any is used
        const int e = (q * 256 + (int)threadIdx.x) * 4;
        sgd_ld4<VEC>(g, e, k.n, gv[q]);
        if (k.d.decay) sgd_ld4<VEC>(v, e, k.n, vv[q]);
    }
#pragma unroll
    for (int q = 0; q < SGD_QUADS; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // (an element beyond the chunk is a zero: it adds +0.0)
            const float g1 = sgd_g1(gv[q][j], k.d.decay ? vv[q][j] : 0.f, wd, k.d.decay);
            S += (double)g1 * (double)g1;
            if (k.d.decay) R += 0.5 * (double)vv[q][j] * (double)vv[q][j];
        }
    }
}

// the workgroup's tree over its 256 thread chains: the total arrives in thread 0.  All 256 threads call this.
__device__ __forceinline__ double sgd_block_tree(double acc, double* red) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();                                       // (ends an earlier use of red)
    if ((threadIdx.x & 63) == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        red[0] += red[2];
        red[1] += red[3];
        red[0] += red[1];
    }
    __syncthreads();
    return red[0];
}

__global__ void __launch_bounds__(256) sgd_norm_kernel(const d3f_sgd_var* __restrict__ desc, int T, const int* __restrict__ chunks,
                                                       int nchunks, const float* __restrict__ hyper, double* __restrict__ partS,
                                                       double* __restrict__ partR) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    SgdChunk k;
    double S = 0.0, R = 0.0;
    if (sgd_chunk(desc, T, chunks, nchunks, c, k)) {       // (uniform over the workgroup)
        const float wd = hyper[3];
        if (k.vec) sgd_chunk_sums<true>(k, wd, S, R);
        else sgd_chunk_sums<false>(k, wd, S, R);
    }
    S = sgd_block_tree(S, red);
    R = sgd_block_tree(R, red);
    if (threadIdx.x == 0) {
        partS[c] = S;
        partR[c] = R;
    }
}

// part[0 .. n) added in ascending order from 0.0 by thread 0, staged through LDS by all: the total is thread 0's.  All 256 threads call this.
__device__ __forceinline__ double sgd_ordered_sum(const double* part, int n, double* tile) {
    double s = 0.0;
    for (int b = 0; b < n; b += SGD_TILE) {
        const int m = min(SGD_TILE, n - b);
        __syncthreads();                                   // (ends an earlier use of tile)
        for (int i = threadIdx.x; i < m; i += 256) tile[i] = part[b + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) s += tile[i];
    }
    return s;
}

template <bool VEC>
__device__ __forceinline__ void sgd_chunk_update(const SgdChunk& k, float lr, float mom, float wd, float s, int zero_grad) {
    float* g = k.d.g + k.begin;
    float* v = k.d.v + k.begin;
    float* a = k.d.a + k.begin;
    float gv[SGD_QUADS][4], vv[SGD_QUADS][4], av[SGD_QUADS][4];
#pragma unroll
    for (int q = 0; q < SGD_QUADS; ++q) {
        const int e = (q * 256 + (int)threadIdx.x) * 4;
        sgd_ld4<VEC>(g, e, k.n, gv[q]);
        sgd_ld4<VEC>(v, e, k.n, vv[q]);
        sgd_ld4<VEC>(a, e, k.n, av[q]);
    }
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < SGD_QUADS; ++q) {
        const int e = (q * 256 + (int)threadIdx.x) * 4;
        if (e >= k.n) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g2 = __fmul_rn(sgd_g1(gv[q][j], vv[q][j], wd, k.d.decay), s);
            av[q][j] = __fadd_rn(__fmul_rn(mom, av[q][j]), g2);
            vv[q][j] = __fsub_rn(vv[q][j], __fmul_rn(lr, av[q][j]));
        }
        sgd_st4<VEC>(a, e, k.n, av[q]);
        sgd_st4<VEC>(v, e, k.n, vv[q]);
        if (zero_grad) sgd_st4<VEC>(g, e, k.n, zero);
    }
}

__global__ void __launch_bounds__(256) sgd_update_kernel(const d3f_sgd_var* __restrict__ desc, int T, const int* __restrict__ chunks,
                                                         int nchunks, const float* __restrict__ hyper, int zero_grad,
                                                         const double* partS, const double* partR, float* __restrict__ reg_loss_out) {
    __shared__ double tile[SGD_TILE];
    __shared__ float sScale;
    const float lr = hyper[0], mom = hyper[1], clip = hyper[2], wd = hyper[3];
    const int c = blockIdx.x;
    if (c == 0 && reg_loss_out) {                          // the designated workgroup: R in table order
        const double R = sgd_ordered_sum(partR, nchunks, tile);
        if (threadIdx.x == 0) *reg_loss_out = (float)((double)wd * R);
    }
    if (c >= nchunks) return;
    SgdChunk k;
    if (!sgd_chunk(desc, T, chunks, nchunks, c, k)) return;
    const double S = sgd_ordered_sum(partS + k.first, k.nt, tile);
    if (threadIdx.x == 0) {
        const float n = (float)__dsqrt_rn(S);
        // max(n, clip) that keeps a NaN norm (a NaN gradient poisons its own variable, as the torch statement does)
        sScale = clip > 0.f ? __fdiv_rn(clip, !(n <= clip) ? n : clip) : 1.f;
    }
    __syncthreads();
    const float s = sScale;
    if (k.vec) sgd_chunk_update<true>(k, lr, mom, wd, s, zero_grad);
    else sgd_chunk_update<false>(k, lr, mom, wd, s, zero_grad);
}

static inline bool sgd_sizes_ok(int T, int nchunks) { return T >= 0 && nchunks >= 0; }

extern "C" int d3f_momentum_sgd_plan(const int* counts, int T, int* chunks_out, int chunks_cap) {
    if (T < 0 || chunks_cap < 0 || (T > 0 && !counts)) return D3F_ERR_ARG;
    long long total = 0;
    for (int t = 0; t < T; ++t) {
        if (counts[t] < 0) return D3F_ERR_ARG;
        for (long long b = 0; b < counts[t]; b += D3F_SGD_CHUNK, ++total)
            if (chunks_out && total < chunks_cap) {
                chunks_out[2 * total] = t;
                chunks_out[2 * total + 1] = (int)b;
            }
        if (total > (1ll << 30)) return D3F_ERR_ARG;
    }
    return (int)total;
}

extern "C" size_t d3f_momentum_sgd_workspace_bytes(int T, int nchunks) {
    if (!sgd_sizes_ok(T, nchunks)) return 0;
    return 2 * d3f_align((size_t)(nchunks > 0 ? nchunks : 1) * 8);
}

extern "C" int d3f_momentum_sgd(const void* desc_, int T, const int* chunks, int nchunks, const float* hyper, int zero_grad,
                                float* reg_loss_out, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!sgd_sizes_ok(T, nchunks) || !hyper || (T > 0 && (!desc_ || (nchunks > 0 && !chunks)))) return D3F_ERR_ARG;
    if (T == 0) return D3F_OK;
    if (!workspace || workspace_bytes < d3f_momentum_sgd_workspace_bytes(T, nchunks)) return D3F_ERR_WORKSPACE;
    const d3f_sgd_var* desc = (const d3f_sgd_var*)desc_;
    D3fArena ar(workspace, workspace_bytes);
    double* partS = ar.take<double>(nchunks > 0 ? nchunks : 1);
    double* partR = ar.take<double>(nchunks > 0 ? nchunks : 1);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    if (nchunks > 0) sgd_norm_kernel<<<nchunks, 256, 0, stream>>>(desc, T, chunks, nchunks, hyper, partS, partR);
    if (nchunks > 0 || reg_loss_out)                       // (no element anywhere: the loss alone, a zero)
        sgd_update_kernel<<<nchunks > 0 ? nchunks : 1, 256, 0, stream>>>(desc, T, chunks, nchunks, hyper, zero_grad ? 1 : 0, partS, partR,
                                                                         reg_loss_out);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
