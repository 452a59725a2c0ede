// Pieces of the KPConv aggregation kernels that the rigid (kpconv.hip) and the deformable (kpconv_deform.hip) operators share:
// the kernel-point slot count, the 24-bit row addressing predicate, the buffer-resource feature gather, the index fetch of a
// (query, neighbour) pair and the LDS image of its 16 influences.
#pragma once
#include "common.h"

#define KP_MAXP D3F_NUM_KP_MAX  // 16 slots, 15 used by the reference

// (row addressing by one 24-bit multiply: common.h, d3f_fits_u24)
// (and the feature matrix must fit a buffer resource: rows * ld * 4 bytes < 2^32)
static inline bool kp_fits_u24(int Nq, int Ns, int ld_idx, int ldf) {
    return d3f_fits_u24(Nq, ld_idx) && d3f_fits_u24(Ns, ldf) && (long long)Ns * ldf < (1ll << 30);
}
// one 16-byte piece (channels c4 .. c4+3) of feature row `id`, fetched with a BUFFER load: the feature matrix is described by a
// buffer resource (base + size in SGPRs), the lane supplies a 32-bit byte offset -- no 64-bit address arithmetic per gather -- and
// a shadow neighbour (id < 0) supplies an offset beyond the buffer: the hardware's range check returns exact zeros for it, with no
// branch, no select and no zero fill.  (Round 3 read row 0 for shadows and relied on their influences being exactly 0: a
// non-finite value in row 0 turned 0 * Inf into NaN for every query with a shadow slot -- ADVICE r03.)
template <class FT> struct KpFeatBuf {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ KpFeatBuf(const FT* f, int rows, int ldf) {
        const unsigned long long bytes = (unsigned long long)(rows > 0 ? rows : 1) * (unsigned)ldf * sizeof(FT);   // < 2^32: kp_fits_u24
        r = __builtin_amdgcn_make_buffer_rsrc((void*)f, 0, (int)(unsigned)bytes, 0x00020000);
    }
};
__device__ __forceinline__ float4 kp_gather4(const KpFeatBuf<float>& B, int id, int ldf, int c4) {
    const unsigned off = id >= 0 ? (__umul24((unsigned)id, (unsigned)ldf) + (unsigned)c4) * 4u : 0xfffffff0u;
    typedef unsigned kp_u4 __attribute__((ext_vector_type(4)));
    const kp_u4 v = __builtin_amdgcn_raw_buffer_load_b128(B.r, (int)off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float4 kp_gather4(const KpFeatBuf<unsigned short>& B, int id, int ldf, int c4) {
    const unsigned off = id >= 0 ? (__umul24((unsigned)id, (unsigned)ldf) + (unsigned)c4) * 2u : 0xfffffff0u;
    typedef unsigned kp_u2 __attribute__((ext_vector_type(2)));
    const kp_u2 w = __builtin_amdgcn_raw_buffer_load_b64(B.r, (int)off, 0, 0);
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
}

__device__ __forceinline__ int kp_pair_index(const int* __restrict__ idrow, bool live, int k, int K, int Ns) {
    return (live && k < K) ? idrow[k] : Ns;
}

// The 16 influences of one (query, neighbour) pair in LDS: four 16-byte quads at base + 16*slot floats.  Eight adjacent
// lanes store their pairs with ds_write_b128 at a 64-byte stride, i.e. on two bank groups only (4-way conflict: a third of the
// LDS-active cycles of these kernels); rotating the quad order by slot/2 spreads them over all eight.  Readers undo it.
__device__ __forceinline__ void kp_store_w(float* __restrict__ pair_base, int slot, const float* w) {
    float4* dst = (float4*)pair_base;
    const int r = slot >> 1;
    dst[(0 + r) & 3] = make_float4(w[0], w[1], w[2], w[3]);
    dst[(1 + r) & 3] = make_float4(w[4], w[5], w[6], w[7]);
    dst[(2 + r) & 3] = make_float4(w[8], w[9], w[10], w[11]);
    dst[(3 + r) & 3] = make_float4(w[12], w[13], w[14], w[15]);
}
__device__ __forceinline__ void kp_load_w(const float* __restrict__ pair_base, int slot, float* w) {
    const float4* src = (const float4*)pair_base;
    const int r = slot >> 1;
    const float4 w0 = src[(0 + r) & 3], w1 = src[(1 + r) & 3], w2 = src[(2 + r) & 3], w3 = src[(3 + r) & 3];
    w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
    w[8] = w2.x; w[9] = w2.y; w[10] = w2.z; w[11] = w2.w; w[12] = w3.x; w[13] = w3.y; w[14] = w3.z; w[15] = w3.w;
}
