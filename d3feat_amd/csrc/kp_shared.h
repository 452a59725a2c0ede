// Pieces of the KPConv aggregation kernels that the rigid (kpconv.hip) and the deformable (kpconv_deform.hip) operators share:
// the kernel-point slot count, the 24-bit row addressing predicate, the buffer-resource feature gather, the influence routines
// (general and FAST), a thread's query (kp_query), the fetch of a (query, neighbour) pair, the LDS image of its 16 influences,
// phase B of the neighbour loop (kp_phase_b: gathers + 60 FMAs per lane) and the Cin -> lanes-per-query launch ladder.
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

// ---- influences of one neighbour (relative position r) for all kernel points, written once for both operators -------------------
// What differs between them is a parameter: inv_scale (the linear influence is 1 - d / (2 extent) in the rigid operator, 1 - d / extent
// in the deformable one), RANGE (the deformable operator drops a neighbour that is within KP_extent of no kernel point: the result
// is that test, from P.e2 = extent^2, and 'constant' is 1 only in range; RANGE = false reads no e2 and returns true) and where the
// kernel points come from (kx / ky / kz: the kernel-argument arrays of the rigid operator, which the compiler reads as scalar
// operands, or a query's own deformed points in registers).  P: KpParams or KpdParams (num_kp, extent, influence, aggregation).
template <bool RANGE, class PT>
__device__ __forceinline__ bool kp_influences(const PT& P, float inv_scale, const float* kx, const float* ky, const float* kz, float rx,
                                              float ry, float rz, float* w) {
    float best = 3.4e38f;
    int bestp = 0;
    bool in = !RANGE;
#pragma unroll
    for (int p = 0; p < KP_MAXP; ++p) {
        if (p < P.num_kp) {
            const float dx = rx - kx[p], dy = ry - ky[p], dz = rz - kz[p];
            const float d2 = dx * dx + dy * dy + dz * dz;
            bool near = true;
            if constexpr (RANGE) { near = d2 < P.e2; in = in || near; }
            float v;
            // v_sqrt_f32 (1 ulp) and a reciprocal multiply instead of the correctly rounded sqrt / divide sequences:
            // ~1e-7 relative on a weight in [0,1], four orders below the 1e-4 parity bar, and 3x fewer VALU instructions
            if (P.influence == 1) v = fmaxf(1.0f - __builtin_amdgcn_sqrtf(d2 + 1e-10f) * inv_scale, 0.0f);
            else if (P.influence == 0) v = near ? 1.0f : 0.0f;
            else { const float sig = P.extent * 0.3f; v = expf(-d2 / (2.0f * sig * sig + 1e-9f)); }
            w[p] = v;
            if (d2 < best) { best = d2; bestp = p; }
        } else {
            w[p] = 0.f;
        }
    }
    if (P.aggregation == 1) {
#pragma unroll
        for (int p = 0; p < KP_MAXP; ++p)
            if (p != bestp) w[p] = 0.f;
    }
    return in;
}

// The configuration every shipped model uses (linear influence, 'sum' aggregation, 15 kernel points -- parameters.txt:
// KP_influence = linear, convolution_mode = sum, num_kernel_points = 15) as straight-line code: 15 x {3 subtractions,
// 3 multiply-adds, add, v_sqrt, multiply-subtract, max}, no mode branches.  FAST = false keeps the general function above
// (other modes / fewer kernel points).
// These kernels are bound by VALU issue (r03 x14: 597 vector instructions per 8-neighbour chunk and wavefront, 285 of them the
// aggregation's FMAs), so the influences are computed two kernel points at a time with the packed fp32 forms (v_pk_add / v_pk_mul /
// v_pk_fma_f32: two IEEE operations per lane and issue slot, the same roundings as the scalar sequence -> bit-identical results).
typedef float kp_f2 __attribute__((ext_vector_type(2)));
template <bool FAST, bool RANGE, class PT>
__device__ __forceinline__ bool kp_influences_t(const PT& P, float inv_scale, const float* kx, const float* ky, const float* kz, float rx,
                                                float ry, float rz, float* w) {
    if constexpr (FAST) {
        const kp_f2 rx2 = {rx, rx}, ry2 = {ry, ry}, rz2 = {rz, rz};
        const kp_f2 one = {1.0f, 1.0f}, ninv = {-inv_scale, -inv_scale}, tiny = {1e-10f, 1e-10f};
        float dmin = 3.4e38f;
#pragma unroll
        for (int p = 0; p < KP_MAXP - 2; p += 2) {
            const kp_f2 kx2 = {kx[p], kx[p + 1]}, ky2 = {ky[p], ky[p + 1]}, kz2 = {kz[p], kz[p + 1]};
            const kp_f2 dx = rx2 - kx2, dy = ry2 - ky2, dz = rz2 - kz2;
            const kp_f2 d2 = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
            if constexpr (RANGE) dmin = fminf(dmin, fminf(d2.x, d2.y));
            const kp_f2 d2t = d2 + tiny;
            const kp_f2 sq = {__builtin_amdgcn_sqrtf(d2t.x), __builtin_amdgcn_sqrtf(d2t.y)};
            const kp_f2 v = __builtin_elementwise_fma(sq, ninv, one);      // fma(-sqrt, inv_scale, 1) as the scalar form
            w[p] = fmaxf(v.x, 0.0f);
            w[p + 1] = fmaxf(v.y, 0.0f);
        }
        {
            constexpr int p = KP_MAXP - 2;
            const float dx = rx - kx[p], dy = ry - ky[p], dz = rz - kz[p];
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if constexpr (RANGE) dmin = fminf(dmin, d2);
            w[p] = fmaxf(fmaf(-__builtin_amdgcn_sqrtf(d2 + 1e-10f), inv_scale, 1.0f), 0.0f);
        }
        w[KP_MAXP - 1] = 0.f;
        if constexpr (RANGE) return dmin < P.e2;
        else return true;
    } else {
        return kp_influences<RANGE>(P, inv_scale, kx, ky, kz, rx, ry, rz, w);
    }
}
static inline bool kp_fast_config(int num_kp, int influence, int aggregation) {
    return num_kp == KP_MAXP - 1 && influence == 1 && aggregation == 0;
}

// ---- a thread's query: the prologue of every aggregation kernel ------------------------------------------------------------------
// Slot `slot` of the visiting order (tile * TQ + ql) is query q_order[slot] when the caller passes the cell-sorted order of the
// neighbour grid -- the TQ queries of a workgroup then share most of their neighbours, whose feature rows are fetched once into
// L1 / L2 instead of TQ times from all over the cloud -- and query `slot` otherwise.  ONE liveness test, slot < Nq: q_order[slot] is
// read only for slot < Nq and q_order holds a permutation of [0, Nq), so g < Nq and slot < Nq agree for every slot.
__device__ __forceinline__ int kp_query_index(const int* __restrict__ q_order, int slot, int Nq) {
    return (q_order && slot < Nq) ? q_order[slot] : slot;
}
struct KpQuery {
    int slot;            // position in the visiting order
    int g;               // global query index
    bool live;           // slot < Nq
    float x, y, z;       // query point (0 for a dead slot)
    const int* idrow;    // the query's row of the index matrix (row 0 for a dead slot, never read: kp_pair_index)
};
__device__ __forceinline__ KpQuery kp_query(int slot, int Nq, const int* __restrict__ q_order, const float* __restrict__ q,
                                            const int* __restrict__ idx, int ld_idx) {
    KpQuery Q;
    Q.slot = slot;
    Q.g = kp_query_index(q_order, slot, Nq);
    Q.live = slot < Nq;
    Q.x = Q.y = Q.z = 0.f;
    if (Q.live) { Q.x = q[3 * (size_t)Q.g]; Q.y = q[3 * (size_t)Q.g + 1]; Q.z = q[3 * (size_t)Q.g + 2]; }
    Q.idrow = idx + (Q.live ? __umul24((unsigned)Q.g, (unsigned)ld_idx) : 0u);   // (rows, leading dimensions < 2^24: kp_fits_u24)
    return Q;
}
// the 60 accumulators of a lane, 15 kernel points x 4 channels, declared and zeroed.  A macro, not a function that takes the array by
// reference: with the zeroing AND phase B behind function boundaries the compiler pairs the accumulators for the packed FMAs in two
// different lane orders and keeps both sets alive (gfx950, ROCm 7: +45 .. +60 VGPRs in every kend-masked kernel, occupancy 3 -> 2,
// 170 .. 230 bytes of scratch in kpconv_fused_kernel; profiles/README.md, kpconv_loop).  Phase B alone behind a function is free.
typedef float KpAcc[KP_MAXP - 1][4];
#define KP_ZEROED_ACC(ACC)                                                                                     \
    KpAcc ACC;                                                                                                 \
    _Pragma("unroll") for (int p_ = 0; p_ < KP_MAXP - 1; ++p_) ACC[p_][0] = ACC[p_][1] = ACC[p_][2] = ACC[p_][3] = 0.f

__device__ __forceinline__ int kp_pair_index(const int* __restrict__ idrow, bool live, int k, int K, int Ns) {
    return (live && k < K) ? idrow[k] : Ns;
}

// Phase-A operands of one (query, neighbour) pair, fetched AHEAD of their chunk so that no chunk starts with a chain of dependent
// round trips (index -> support point): the index of chunk j + 1 is requested at the top of chunk j (it depends on nothing), the
// point and row flag it names at the top of chunk j's phase B (the index has had phase A to arrive) and land under phase B's
// gathers and FMAs.  A shadow neighbour (index outside [0, Ns)) reads row 0 and is moved to 1e6 by the callers -- the reference's
// own shadow point (kernels/convolution_ops.py:186-188): every influence of the shipped (linear) configuration is exactly 0, no branch.
// ROWFLAG = false (the deformable operator: no neighbour count) issues no load of rowpos, which may be NULL.
struct KpPair {
    int id;              // neighbour index, -1: shadow
    float x, y, z;       // support point
    bool pos;            // row flag of the support (the neighbour-count test); false without ROWFLAG
};
template <bool ROWFLAG>
__device__ __forceinline__ KpPair kp_pair_fetch(int id, int Ns, const float* __restrict__ s, const unsigned char* __restrict__ rowpos) {
    KpPair r;
    const bool ok = id >= 0 && id < Ns;
    const unsigned row = ok ? (unsigned)id : 0u;
    const float* sp = s + 3u * row;
    r.x = sp[0]; r.y = sp[1]; r.z = sp[2];
    r.pos = false;
    if constexpr (ROWFLAG) r.pos = rowpos[row] != 0;
    r.id = ok ? id : -1;
    return r;
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

// ---- phase B of one chunk: thread = (query, channels 4*cl .. 4*cl+3) ---------------------------------------------------------------
// lidx_q / lw_q: the query's rows of the parked neighbour indices and influences (phase A).  Feature rows are requested in groups
// of PF before any is consumed: the gathers are independent, so their latencies overlap instead of adding up (the kernels are
// bound by these round trips, not by the FMAs).  A slot whose index is -1 for every query of the wavefront (shadow or dropped
// neighbour, or beyond kend) is skipped (wavefront-uniform test): its gather returned the buffer's zeros, nothing to add.
// KCT > 0: every chunk holds KCT slots (slots beyond K were parked as -1): compile-time trip count, no kend mask, fully unrolled.
// KCT = 0: slots kend .. of the chunk hold the previous chunk's indices and are masked.
template <int PF, bool MASKED, class FT>   // one group of PF slots kg .. kg + PF - 1
__device__ __forceinline__ void kp_phase_b_group(const KpFeatBuf<FT>& fbuf, int ldf, const int* __restrict__ lidx_q,
                                                 const float* __restrict__ lw_q, int kg, int kend, int cl, KpAcc& acc) {
    float4 fv[PF];
    int ids[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        ids[u] = (!MASKED || kg + u < kend) ? lidx_q[kg + u] : -1;
        fv[u] = kp_gather4(fbuf, ids[u], ldf, 4 * cl);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        if (!__any(ids[u] >= 0)) continue;
        float w[16];
        kp_load_w(&lw_q[(kg + u) * 16], kg + u, w);
#pragma unroll
        for (int p = 0; p < KP_MAXP - 1; ++p) {
            acc[p][0] = fmaf(w[p], fv[u].x, acc[p][0]);
            acc[p][1] = fmaf(w[p], fv[u].y, acc[p][1]);
            acc[p][2] = fmaf(w[p], fv[u].z, acc[p][2]);
            acc[p][3] = fmaf(w[p], fv[u].w, acc[p][3]);
        }
    }
}
template <int PF, int KCT, class FT>
__device__ __forceinline__ void kp_phase_b(const KpFeatBuf<FT>& fbuf, int ldf, const int* __restrict__ lidx_q, const float* __restrict__ lw_q,
                                           int kend, int cl, KpAcc& acc) {
    if constexpr (KCT > 0) {
#pragma unroll
        for (int kg = 0; kg < KCT; kg += PF) kp_phase_b_group<PF, false>(fbuf, ldf, lidx_q, lw_q, kg, KCT, cl, acc);
    } else {
        for (int kg = 0; kg < kend; kg += PF) kp_phase_b_group<PF, true>(fbuf, ldf, lidx_q, lw_q, kg, kend, cl, acc);
    }
}

// ---- the Cin -> lanes-per-query ladder of the two aggregate entry points ---------------------------------------------------------
// Cin = 4 LQ in {4 .. 1024} launches KERNEL<LQ, fast> over d3f_cdiv(Nq, TQ) workgroups of TQ * LQ threads, TQ = min(256 / LQ, TQMAX),
// with the argument list that follows; any other Cin launches nothing and sets ON_LADDER = false.
#define KP_LADDER_STEP(KERNEL, LQ_, TQMAX, FAST, NQ, STREAM, ...)                                         \
    do {                                                                                                  \
        constexpr int TQ_ = (256 / LQ_) < (TQMAX) ? (256 / LQ_) : (TQMAX);                                \
        if (FAST) KERNEL<LQ_, true><<<d3f_cdiv(NQ, TQ_), TQ_ * LQ_, 0, STREAM>>>(__VA_ARGS__);            \
        else KERNEL<LQ_, false><<<d3f_cdiv(NQ, TQ_), TQ_ * LQ_, 0, STREAM>>>(__VA_ARGS__);                \
    } while (0)
#define KP_LADDER(ON_LADDER, KERNEL, TQMAX, CIN, FAST, NQ, STREAM, ...)                                   \
    switch (CIN) {                                                                                        \
    case 4: KP_LADDER_STEP(KERNEL, 1, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                       \
    case 8: KP_LADDER_STEP(KERNEL, 2, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                       \
    case 16: KP_LADDER_STEP(KERNEL, 4, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                      \
    case 32: KP_LADDER_STEP(KERNEL, 8, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                      \
    case 64: KP_LADDER_STEP(KERNEL, 16, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                     \
    case 128: KP_LADDER_STEP(KERNEL, 32, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                    \
    case 256: KP_LADDER_STEP(KERNEL, 64, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                    \
    case 512: KP_LADDER_STEP(KERNEL, 128, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                   \
    case 1024: KP_LADDER_STEP(KERNEL, 256, TQMAX, FAST, NQ, STREAM, __VA_ARGS__); break;                  \
    default: ON_LADDER = false;                                                                           \
    }
