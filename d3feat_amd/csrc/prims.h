// Fused building blocks of the preprocessing pipelines (grid subsampling, neighbour grid).
//
// A fragment is ~400 launches, three quarters of them tiny preprocessing kernels; inside a replayed HIP graph every
// node costs a few microseconds of dispatch whatever its size.  These templates cut the node count:
//   * begin_kernel      one launch for all "reset" work of an op: up to four fills, lens -> offsets, bounding-box
//                       initialisation, ticket counters;
//   * bbox_kernel<Epi>  per-element bounding boxes + an epilogue run by the LAST workgroup to finish (ticket counter), e.g.
//                       the per-element grid geometry that needs the complete boxes;
//   * scan_fold_kernel<In, Epi>  exclusive scan in ONE launch: every workgroup scans its 1024-item tile (`local`), the last
//                       workgroup to finish scans the tile sums into `base` and runs an epilogue with the grand total.
//                       Consumers read  local[i] + base[i / D3F_SCAN_TILE]  (d3f_scan_at) instead of a third "add" pass.
//   * d3f_block_excl_scan<T>  the exclusive scan over the T threads of a workgroup that every scanning kernel calls (on top of
//                       d3f_wave_incl_scan, common.h).
// Inter-workgroup hand-off ("last workgroup") follows cdna_hip_programming.md G16: every workgroup's stores, then
// __syncthreads, then one lane: agent-scope release fence + s_waitcnt + device-scope atomic ticket; the last arriver
// issues an agent-scope acquire fence before its (first-touch) reads of the other workgroups' results.
#pragma once
#include "common.h"

#define D3F_SCAN_TILE 1024

struct D3fFill {
    unsigned* p;
    unsigned long long n;   // 32-bit words
    unsigned v;
};

__device__ __forceinline__ bool d3f_last_block(unsigned* counter, unsigned nblocks) {
    __shared__ int last_flag;
    // every wave waits for ITS OWN stores to be acknowledged before the barrier: the workgroup-scope release inside
    // __syncthreads may omit vmcnt(0) outside tgsplit mode, and lane 0's agent-scope release below only covers its own wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = atomicAdd(counter, 1u);
        last_flag = (t == nblocks - 1u) ? 1 : 0;
        if (last_flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return last_flag != 0;
}

// one fill, spread over the whole launch (tid / stride: the thread's index in the launch and the launch's thread count)
__device__ __forceinline__ void d3f_fill_words(const D3fFill& f, size_t tid, size_t stride) {
    unsigned* p = f.p;
    const size_t n = (size_t)f.n;
    if (n == 0) return;
    const size_t n4 = (((uintptr_t)p & 15) == 0) ? n / 4 : 0;
    const uint4 v4 = make_uint4(f.v, f.v, f.v, f.v);
    for (size_t j = tid; j < n4; j += stride) ((uint4*)p)[j] = v4;
    for (size_t j = n4 * 4 + tid; j < n; j += stride) p[j] = f.v;
}

// offs[0..B] = prefix sums of lens; bbox[b*6 + {0,1,2}] = 0xFFFFFFFF (min slots), {3,4,5} = 0 (max slots); counters = 0;
// fills f0..f3 (n = 0: unused).  Any grid size; 256 threads.
static __global__ void __launch_bounds__(256) begin_kernel(const int* __restrict__ lens, int B, int* __restrict__ offs,
                                                    unsigned* __restrict__ bbox, unsigned* __restrict__ counters,
                                                    int ncounters, D3fFill f0, D3fFill f1, D3fFill f2, D3fFill f3) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && lens) {
            int s = 0;
            for (int b = 0; b < B; ++b) { offs[b] = s; s += lens[b]; }
            offs[B] = s;
        }
        if (bbox)
            for (int i = threadIdx.x; i < B * 6; i += blockDim.x) bbox[i] = ((i % 6) < 3) ? 0xFFFFFFFFu : 0u;
        for (int i = threadIdx.x; i < ncounters; i += blockDim.x) counters[i] = 0u;
    }
    d3f_fill_words(f0, tid, stride);
    d3f_fill_words(f1, tid, stride);
    d3f_fill_words(f2, tid, stride);
    d3f_fill_words(f3, tid, stride);
}

static inline int d3f_begin_launch(const int* lens, int B, int* offs, unsigned* bbox, unsigned* counters, int ncounters,
                                   D3fFill f0, D3fFill f1, D3fFill f2, D3fFill f3, hipStream_t stream) {
    const unsigned long long words = f0.n + f1.n + f2.n + f3.n;
    long long blocks = (long long)(words / 4 / 256) + 1;
    if (blocks > 1024) blocks = 1024;
    begin_kernel<<<(int)blocks, 256, 0, stream>>>(lens, B, offs, bbox, counters, ncounters, f0, f1, f2, f3);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// Bounding boxes per batch element, grid (chunks, B); min / max are exact and order independent, so the result equals
// cpp_utils/cloud/cloud.cpp:27-66 bit for bit.  epi(b_first, b_step) is run by the last workgroup with all 256 threads.
// ptrs != NULL: element b's points are read IN PLACE from ptrs[b] (its own array, rows 0 .. len_b - 1) instead of from rows
// [offs[b], offs[b + 1]) of the stacked array `pts` (the stage-0 clouds of a replay are never copied into one buffer).
template <class Epi>
__global__ void __launch_bounds__(256) bbox_kernel(const float* __restrict__ pts, const float* const* __restrict__ ptrs,
                                                   const int* __restrict__ offs, int B,
                                                   unsigned* __restrict__ bbox, unsigned* __restrict__ counter, Epi epi) {
    const int b = blockIdx.y;
    const int lo = offs[b], hi = offs[b + 1];
    if (ptrs) pts = ptrs[b] - 3 * (size_t)lo;          // virtual base: row i of the stack = row i - lo of the element
    unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    // four points per thread and trip: twelve loads in flight (one point per trip was a chain of dependent HBM round trips --
    // 60 us for the 1.2 M points of a stage-0 stack)
    const int stride = gridDim.x * blockDim.x;
    for (int i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += 4 * stride) {
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int iu = min(i + u * stride, hi - 1);       // (a repeated point changes no minimum)
#pragma unroll
            for (int d = 0; d < 3; ++d) v[u][d] = pts[3 * (size_t)iu + d];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned x = d3f_f2ord(v[u][d]);
                mn[d] = min(mn[d], x);
                mx[d] = max(mx[d], x);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = min(mn[d], (unsigned)__shfl_xor((int)mn[d], o, 64));
            mx[d] = max(mx[d], (unsigned)__shfl_xor((int)mx[d], o, 64));
        }
    }
    // one atomic per block and slot (same-address atomics serialise in L2 at ~12 ns each)
    __shared__ unsigned red[4][6];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { red[wv][d] = mn[d]; red[wv][3 + d] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 6 && lo < hi) {
        unsigned v = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) v = (threadIdx.x < 3) ? min(v, red[k][threadIdx.x]) : max(v, red[k][threadIdx.x]);
        if (threadIdx.x < 3) atomicMin(&bbox[b * 6 + threadIdx.x], v);
        else atomicMax(&bbox[b * 6 + threadIdx.x], v);
    }
    if (d3f_last_block(counter, gridDim.x * gridDim.y)) epi();
}

template <class Epi>
static inline int d3f_bbox_launch_t(const float* pts, const int* offs, int B, int N, unsigned* bbox, unsigned* counter, Epi epi,
                                    hipStream_t stream, const float* const* ptrs = nullptr) {
    // about one workgroup per CU over all elements: every workgroup ends with a ticket on ONE counter, and same-address
    // atomics serialise at ~12 ns each, so thousands of (mostly idle) workgroups cost more than the boxes themselves
    // (N is the whole stack: an element holds about N / B points; eight points per thread)
    int chunks = d3f_cdiv(d3f_cdiv(N > 0 ? N : 1, B), 256 * 8);
    const int per_elem = 512 / B > 1 ? 512 / B : 1;
    if (chunks > per_elem) chunks = per_elem;
    bbox_kernel<Epi><<<dim3(chunks, B), 256, 0, stream>>>(pts, ptrs, offs, B, bbox, counter, epi);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---- bounding boxes accumulated by the kernel that WRITES the points --------------------------------------------------
// Min and max do not depend on the order of their operands, so a box gathered by the producer of a cloud equals the one
// bbox_kernel finds by reading the cloud again, bit for bit.  bbox[b * 6 ..] must hold the initial values (min slots
// 0xFFFFFFFF, max slots 0) before the producer runs.
// Atomics on one cache line serialise in L2 at ~12 ns each, and all boxes of a cloud share a line: what counts is the number of
// atomics per cloud, so the reduction goes wavefront -> workgroup (runs of wavefronts that belong to one element are merged) and
// a slot whose value would not change is skipped after a plain read (the stored bound only tightens: a stale read can cost an
// atomic, never lose one).
// EVERY thread of the workgroup calls this (blockDim.x a multiple of 64, <= 1024; no early return before it).  b < 0: the thread
// contributes nothing.  Elements must not decrease with the thread index.  A wavefront that straddles two elements falls back to
// one atomic per lane and slot.
__device__ __forceinline__ void d3f_box_flush(unsigned* __restrict__ bbox, int b, int slot, unsigned v) {
    unsigned* p = &bbox[b * 6 + slot];
    const unsigned old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot < 3) { if (v < old) atomicMin(p, v); }
    else if (v > old) atomicMax(p, v);
}
__device__ __forceinline__ void d3f_box_accum_block(unsigned* __restrict__ bbox, int b, float x, float y, float z) {
    __shared__ unsigned sBox[16][6];
    __shared__ int sElem[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned v[6] = {d3f_f2ord(x), d3f_f2ord(y), d3f_f2ord(z), 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        v[3 + d] = b < 0 ? 0u : v[d];
        v[d] = b < 0 ? 0xFFFFFFFFu : v[d];
    }
    const unsigned long long live = __ballot(b >= 0);
    int bw = -1;                                           // the wavefront's element; -1: nothing left for the workgroup step
    if (live) {
        bw = __shfl(b, __ffsll((long long)live) - 1, 64);
        if (__ballot(b >= 0 && b != bw)) {
            // one element after the other: its lanes reduced, six lanes flush the six slots side by side (a chain of six
            // read-then-atomic pairs per lane held the whole launch up)
            unsigned long long rem = live;
            while (rem) {
                const int bs = __shfl(b, __ffsll((long long)rem) - 1, 64);
                const bool mine = b == bs;
                unsigned r[6], sel = 0u;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    r[t] = mine ? v[t] : (t < 3 ? 0xFFFFFFFFu : 0u);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned q = (unsigned)__shfl_xor((int)r[t], o, 64);
                        r[t] = t < 3 ? min(r[t], q) : max(r[t], q);
                    }
                    sel = lane == t ? r[t] : sel;
                }
                if (lane < 6) d3f_box_flush(bbox, bs, lane, sel);
                rem &= ~__ballot(mine);
            }
            bw = -1;
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    v[d] = min(v[d], (unsigned)__shfl_xor((int)v[d], o, 64));
                    v[3 + d] = max(v[3 + d], (unsigned)__shfl_xor((int)v[3 + d], o, 64));
                }
            }
        }
    }
    if (lane == 0) {
        sElem[w] = bw;
#pragma unroll
        for (int t = 0; t < 6; ++t) sBox[w][t] = v[t];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int t = threadIdx.x;
        int cur = -1;
        unsigned acc = 0u;
        for (int k = 0; k <= nw; ++k) {
            const int bk = k < nw ? sElem[k] : -2;         // (-2: the end, flushes the last run)
            if (bk == -1) continue;
            if (bk != cur) {
                if (cur >= 0) d3f_box_flush(bbox, cur, t, acc);
                cur = bk;
                acc = k < nw ? sBox[k][t] : 0u;
            } else {
                acc = t < 3 ? min(acc, sBox[k][t]) : max(acc, sBox[k][t]);
            }
        }
    }
}

// ---- workgroup sum by a fixed tree ----------------------------------------------------------------------------------
// Sum of v over the 256 threads of the workgroup (red: 256 T's of LDS); the result in every thread.  The order is part of the float64
// results of its callers (d3f_pose_errors, d3f_validation_pairs): strides 128 .. 1, red[t] += red[t + s] for t < s -- no wave shuffles.
// The first barrier ends an earlier use of red, so calls may follow one another.
template <class T>
__device__ __forceinline__ T d3f_block_sum(T v, T* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// ---- one-launch exclusive scan --------------------------------------------------------------------------------------
// Exclusive scan of v over the T threads of the workgroup (all of them call this), the grand total in every thread: wave scan
// (d3f_wave_incl_scan), wave sums in wsum[T / 64] (LDS), every thread adds up the waves before its own.  The second barrier
// frees wsum, so calls may follow one another.
template <int T>
__device__ __forceinline__ int d3f_block_excl_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = d3f_wave_incl_scan(v);
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < T / 64; ++q) {
        const int s = wsum[q];
        if (q < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

__device__ __forceinline__ int d3f_scan_at(const int* __restrict__ local, const int* __restrict__ base, int i) {
    return local[i] + base[i / D3F_SCAN_TILE];
}

// in(i) -> item i (i < n).  local[i] = exclusive scan inside i's tile; base[t] = sum of the tiles before t (written by the
// last workgroup); epi(total) runs in the last workgroup (all 256 threads) after `base` is complete.
template <class In, class Epi>
__global__ void __launch_bounds__(256) scan_fold_kernel(In in, int n, const int* __restrict__ n_dev, int* __restrict__ local,
                                                        int* __restrict__ base, unsigned* __restrict__ counter, Epi epi) {
    __shared__ int lds[4];
    n = d3f_dyn(n, n_dev);   // items beyond the device-side count are zeros that are neither read nor written
    // capacity-sized launch: only the tiles that hold items take part (and take a ticket); tile 0 always does, so that the
    // epilogue runs for an empty input too
    const int live = max(1, (n + D3F_SCAN_TILE - 1) / D3F_SCAN_TILE);
    if ((int)blockIdx.x >= live) return;
    const int i0 = blockIdx.x * D3F_SCAN_TILE + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (i0 + k < n) ? in(i0 + k) : 0;
        s += v[k];
    }
    int tot;
    int ex = d3f_block_excl_scan<256>(s, lds, &tot);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) local[i0 + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) base[blockIdx.x] = tot;
    if (!d3f_last_block(counter, (unsigned)live)) return;
    const int nblocks = live;
    int carry = 0;
    for (int c = 0; c < nblocks; c += 256) {
        const int i = c + threadIdx.x;
        const int x = (i < nblocks) ? __hip_atomic_load(&base[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        int t;
        const int e = d3f_block_excl_scan<256>(x, lds, &t);
        if (i < nblocks) base[i] = carry + e;
        carry += t;
    }
    __syncthreads();
    epi(carry);
}

struct D3fScanIn {   // plain array input
    const int* p;
    __device__ __forceinline__ int operator()(int i) const { return p[i]; }
};
struct D3fNoEpi {
    __device__ __forceinline__ void operator()(int) const {}
    __device__ __forceinline__ void operator()() const {}
};

static inline size_t d3f_scan_base_ints(int n) { return (size_t)d3f_cdiv(n > 0 ? n : 1, D3F_SCAN_TILE) + 64; }

template <class In, class Epi>
static inline int d3f_scan_fold_launch(In in, int n, const int* n_dev, int* local, int* base, unsigned* counter, Epi epi,
                                       hipStream_t stream) {
    const int nb = d3f_cdiv(n > 0 ? n : 1, D3F_SCAN_TILE);
    scan_fold_kernel<In, Epi><<<nb, 256, 0, stream>>>(in, n, n_dev, local, base, counter, epi);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
