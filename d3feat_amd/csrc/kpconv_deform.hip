// Deformable KPConv on gfx950, phase 1: neighbour gather + influences of PER-QUERY kernel points + weighted aggregation.
//
// Reference: kernels/convolution_ops.py:379-499 (KPConv_deform_ops), called from KPConv_deformable (:258-376) with the output of the
// rigid offset convolution (:331-339).  Per query n, from that convolution's RAW output (offset_scale = KP_extent, mod_logits):
//   KP'[n,p]  = KP[p] + off[n, 3p .. 3p+2] * offset_scale                                (:344-359, :424)
//   mod[n,p]  = 2 * sigmoid(mod_in[n, p])                          (modulated only)      (:348)
// or from the operator's own arguments (offset_scale = 1, the modulations as they are).
//   in[n,k]   = any_p || (s[idx[n,k]] - q[n]) - KP'[n,p] ||^2 < KP_extent^2              (:435)
//   wf[n,p,c] = mod[n,p] * sum_{k : in[n,k]} h(|| (s[idx[n,k]] - q[n]) - KP'[n,p] ||) * f[idx[n,k], c]     (:453-490)
// What differs from the rigid operator (kpconv.hip):
//   * the kernel points differ per query, so they cannot ride in scalar operands: the TQ queries of a workgroup stage theirs in
//     LDS once (kpd_stage_points) and phase A reads them back with 16-byte broadcasts;
//   * a neighbour that is within KP_extent of NO deformed point is dropped (the reference compacts the kept neighbours with top_k /
//     batch_gather; dropping is the same sum): it parks id = -1 like a shadow, so its gather returns the buffer's zeros;
//   * linear influence divides by KP_extent (:461), not 2 KP_extent (:215); 'constant' is d2 < KP_extent^2 per kernel point (:456);
//   * no neighbour count, no normalisation (:497-499); the modulations scale the accumulators in the epilogue.
// The shadow point of the reference sits at 1000 here (:414), not 1e6: it is never in range and its feature row is the zero row,
// so a shadow slot (index outside [0, Ns)) contributes nothing, exactly as a dropped neighbour.
//
// Kernels, modelled on kpconv_agg_vec4 / kpconv_agg_scalar:
//  * kpconv_deform_agg_vec4<LQ, FAST> (Cin = 4 LQ): TQ = min(256 / LQ, 64) queries per workgroup of TQ * LQ threads, the same two
//    phases, chunks of KC = LQ neighbours, buffer-resource gathers, q_order and Nq_dev / Ns_dev.  LDS per query (KPD_DS = 68
//    floats): x'[16] y'[16] z'[16] mod[16] + 4 floats that de-phase the b128 broadcasts of adjacent queries (a 16-lane group of
//    ds_read_b128 that holds 16 different queries then touches 16 different 16-byte slots of the 256-byte bank row).
//    FAST: linear / sum / 15 points as straight-line packed fp32 code.
//  * kpconv_deform_agg_scalar: any other Cin, alignment or address range; one thread per (query, channel), the deformed points in
//    registers.
// The neighbour loop is the rigid operator's, and so is its code (kp_shared.h): kp_query, kp_pair_fetch<false> (no row flag is loaded),
// kp_influences / kp_influences_t with RANGE = true, inv_scale = 1 / KP_extent and the query's own points, kp_phase_b, and the
// Cin -> LQ launch ladder (KP_LADDER).  This file holds what is the deformable operator's own: the parameters, the staging of the
// deformed points, phase A's range filter and the modulations of the epilogue.
#include "common.h"
#include "kp_shared.h"

#define KPD_DS (4 * KP_MAXP + 4)     // floats per query in LDS

struct KpdParams {
    float kp[KP_MAXP * 3];
    int num_kp;
    float extent;
    float inv_extent;   // 1 / extent
    float e2;           // extent^2 (the in-range test, rounded once from the double product)
    int influence;      // 0 constant, 1 linear, 2 gaussian
    int aggregation;    // 0 sum, 1 closest
    float off_scale;    // deformed point = kernel point + offset * off_scale
    int modulated;      // 0: none, 1: the modulations as given, 2: 2 * sigmoid(given)
};
static inline KpdParams kpd_make_params(const float* kp_host, int num_kp, float KP_extent, int influence, int aggregation, float off_scale,
                                        int modulated) {
    KpdParams P;
    for (int i = 0; i < KP_MAXP * 3; ++i) P.kp[i] = i < num_kp * 3 ? kp_host[i] : 0.f;
    P.num_kp = num_kp; P.extent = KP_extent; P.inv_extent = 1.0f / KP_extent; P.e2 = (float)((double)KP_extent * (double)KP_extent);
    P.influence = influence; P.aggregation = aggregation; P.off_scale = off_scale; P.modulated = modulated;
    return P;
}

// deformed kernel point p of one query and its modulation: a product and an add per coordinate, as the reference's
// `offsets *= KP_extent` (:359) and `offsets + K_points` (:424) round (off_scale = 1: the product is exact)
__device__ __forceinline__ void kpd_point(const KpdParams& P, const float* __restrict__ orow, const float* __restrict__ mrow, int p, float& x,
                                          float& y, float& z, float& m) {
    x = P.kp[3 * p] + orow[3 * p] * P.off_scale;
    y = P.kp[3 * p + 1] + orow[3 * p + 1] * P.off_scale;
    z = P.kp[3 * p + 2] + orow[3 * p + 2] * P.off_scale;
    m = P.modulated == 2 ? 2.0f / (1.0f + expf(-mrow[p])) : P.modulated == 1 ? mrow[p] : 1.0f;
}

// the 16 x 3 deformed points (+ 16 modulations) of query slot ql -> dp[ql * KPD_DS ..]; one thread per query, the kernel points
// indexed statically (they are kernel arguments: a per-lane index would move them to scratch).  Unused slots hold 0.
__device__ __forceinline__ void kpd_stage_points(const KpdParams& P, const float* __restrict__ orow, const float* __restrict__ mrow,
                                                 float* __restrict__ dst) {
#pragma unroll
    for (int p = 0; p < KP_MAXP; ++p) {
        float x = 0.f, y = 0.f, z = 0.f, m = 0.f;
        if (orow && p < P.num_kp) kpd_point(P, orow, mrow, p, x, y, z, m);
        dst[p] = x; dst[KP_MAXP + p] = y; dst[2 * KP_MAXP + p] = z; dst[3 * KP_MAXP + p] = m;
    }
}
__device__ __forceinline__ void kpd_load16(const float* __restrict__ src, float* v) {
    const float4* s4 = (const float4*)src;
    const float4 a = s4[0], b = s4[1], c = s4[2], d = s4[3];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w; v[12] = d.x; v[13] = d.y; v[14] = d.z; v[15] = d.w;
}

template <int LQ, bool FAST>  // lanes per query = Cin / 4; FAST: linear / sum / 15 kernel points
__global__ void __launch_bounds__(256)
kpconv_deform_agg_vec4(const float* __restrict__ q, int Nq, const float* __restrict__ s, int Ns, const int* __restrict__ idx,
                       int ld_idx, int K, const float* __restrict__ f, int ldf, const float* __restrict__ off, int ld_off,
                       const float* __restrict__ mod, int ld_mod, KpdParams P, float* __restrict__ wf, const int* __restrict__ Nq_dev, const int* __restrict__ Ns_dev,
                       const int* __restrict__ q_order) {
    constexpr int TQ = (256 / LQ) < 64 ? (256 / LQ) : 64;   // queries per workgroup
    constexpr int NT = TQ * LQ;                              // threads per workgroup (64 / 128 at LQ = 1 / 2, else 256)
    Nq = d3f_dyn(Nq, Nq_dev);
    Ns = d3f_dyn(Ns, Ns_dev);
    const KpFeatBuf<float> fbuf(f, Ns, ldf);
    if ((int)(blockIdx.x * TQ) >= Nq) return;   // capacity-sized grid: whole block beyond the real query count
    const int tile = (int)d3f_xcd_tile(blockIdx.x, (unsigned)((Nq + TQ - 1) / TQ));
    constexpr int KC = LQ;           // neighbours per chunk (TQ * KC pairs = one per thread)
    constexpr int WS = KC * 16 + 4;  // per-query stride of the influences (floats)
    __shared__ __attribute__((aligned(16))) float lw[TQ * WS];
    __shared__ __attribute__((aligned(16))) float ldp[TQ * KPD_DS];
    __shared__ int lidx[TQ * KC];
    const int tid = threadIdx.x;
    const int ql = tid / LQ, cl = tid % LQ;  // query-in-block, channel group
    const KpQuery Q = kp_query(tile * TQ + ql, Nq, q_order, q, idx, ld_idx);
    const int Cin = LQ * 4;
    // ---- the workgroup's deformed kernel points: thread t < TQ stages query slot t ----
    for (int t = tid; t < TQ; t += NT) {
        const int ts = tile * TQ + t;
        const int tg = kp_query_index(q_order, ts, Nq);
        kpd_stage_points(P, ts < Nq ? off + (size_t)tg * ld_off : nullptr, mod ? mod + (size_t)(ts < Nq ? tg : 0) * ld_mod : nullptr,
                         &ldp[t * KPD_DS]);
    }
    KP_ZEROED_ACC(acc);
    KpPair pr = kp_pair_fetch<false>(kp_pair_index(Q.idrow, Q.live, cl, K, Ns), Ns, s, nullptr);   // chunk 0's pair (no row flag: no count)
    __syncthreads();
    const float* dp = &ldp[ql * KPD_DS];
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int id_next = kp_pair_index(Q.idrow, Q.live, k0 + KC + cl, K, Ns);            // in flight during phase A
        // ---- phase A: thread = (query ql, neighbour k0 + cl) ----
        {
            float kx[KP_MAXP], ky[KP_MAXP], kz[KP_MAXP], w[KP_MAXP];
            kpd_load16(dp, kx); kpd_load16(dp + KP_MAXP, ky); kpd_load16(dp + 2 * KP_MAXP, kz);
            const bool ok = pr.id >= 0;
            const bool in = kp_influences_t<FAST, true>(P, P.inv_extent, kx, ky, kz, ok ? pr.x - Q.x : 1e6f, ok ? pr.y - Q.y : 1e6f,
                                                        ok ? pr.z - Q.z : 1e6f, w);
            const bool keep = ok && in;
            if (!FAST) {        // gaussian is not 0 out of range and 'closest' picks a point anyway: zero a dropped pair's weights
#pragma unroll                  // (the FAST weights are finite and meet the zeros the gather returns for id = -1)
                for (int p = 0; p < KP_MAXP; ++p) w[p] = keep ? w[p] : 0.f;
            }
            lidx[ql * KC + cl] = keep ? pr.id : -1;
            kp_store_w(&lw[ql * WS + cl * 16], cl, w);
        }
        __syncthreads();
        pr = kp_pair_fetch<false>(id_next, Ns, s, nullptr);                                 // in flight during phase B
        // ---- phase B: thread = (query ql, channels 4*cl .. 4*cl+3), up to eight feature rows in flight ----
        kp_phase_b<(KC < 8 ? KC : 8), 0>(fbuf, ldf, &lidx[ql * KC], &lw[ql * WS], min(KC, K - k0), cl, acc);
        __syncthreads();
    }
    if (Q.live) {
        float m[KP_MAXP];
        kpd_load16(dp + 3 * KP_MAXP, m);
        float* o = wf + (size_t)Q.g * P.num_kp * Cin + 4 * cl;
#pragma unroll
        for (int p = 0; p < KP_MAXP - 1; ++p)
            if (p < P.num_kp) {
                const float mp = P.modulated ? m[p] : 1.0f;
                *(float4*)&o[(size_t)p * Cin] = make_float4(acc[p][0] * mp, acc[p][1] * mp, acc[p][2] * mp, acc[p][3] * mp);
            }
    }
}

// generic path: one thread per (query, channel), the query's deformed points in registers
__global__ void __launch_bounds__(256)
kpconv_deform_agg_scalar(const float* __restrict__ q, int Nq, const float* __restrict__ s, int Ns, const int* __restrict__ idx,
                         int ld_idx, int K, const float* __restrict__ f, int ldf, int Cin, const float* __restrict__ off, int ld_off,
                         const float* __restrict__ mod, int ld_mod, KpdParams P, float* __restrict__ wf, const int* __restrict__ Nq_dev, const int* __restrict__ Ns_dev) {
    Nq = d3f_dyn(Nq, Nq_dev);
    Ns = d3f_dyn(Ns, Ns_dev);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)Nq * Cin) return;
    const int qg = (int)(t / Cin), c = (int)(t % Cin);
    const float qx = q[3 * (size_t)qg], qy = q[3 * (size_t)qg + 1], qz = q[3 * (size_t)qg + 2];
    const float* orow = off + (size_t)qg * ld_off;
    const float* mrow = mod ? mod + (size_t)qg * ld_mod : nullptr;
    float kx[KP_MAXP], ky[KP_MAXP], kz[KP_MAXP], acc[KP_MAXP];
#pragma unroll
    for (int p = 0; p < KP_MAXP; ++p) {
        float m;
        kx[p] = ky[p] = kz[p] = acc[p] = 0.f;
        if (p < P.num_kp) kpd_point(P, orow, mrow, p, kx[p], ky[p], kz[p], m);
    }
    for (int k = 0; k < K; ++k) {
        const int id = idx[(size_t)qg * ld_idx + k];
        if (id < 0 || id >= Ns) continue;
        float w[KP_MAXP];
        if (!kp_influences<true>(P, P.inv_extent, kx, ky, kz, s[3 * (size_t)id] - qx, s[3 * (size_t)id + 1] - qy, s[3 * (size_t)id + 2] - qz, w)) continue;
        const float fv = f[(size_t)id * ldf + c];
#pragma unroll
        for (int p = 0; p < KP_MAXP; ++p) acc[p] = fmaf(w[p], fv, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < KP_MAXP; ++p)
        if (p < P.num_kp) {
            float x, y, z, m;
            kpd_point(P, orow, mrow, p, x, y, z, m);
            wf[((size_t)qg * P.num_kp + p) * Cin + c] = P.modulated ? acc[p] * m : acc[p];
        }
}

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" int d3f_kpconv_deform_aggregate(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                                           const void* f_, int ldf, int Cin, const float* offsets, int ld_off, float offset_scale,
                                           const float* modulations, int ld_mod, int mod_logits, const float* kp_host, int num_kp, float KP_extent, int influence, int aggregation,
                                           float* wf, const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16,
                                           void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const float* f = (const float*)f_;
    if (feat_bf16) return D3F_ERR_ARG;      // fp32 feature rows only
    if (Nq < 0 || Ns < 0 || (Ns == 0 && Nq > 0) || K < 0 || ld_idx < K || Cin < 1 || ldf < Cin || num_kp < 1 || num_kp > KP_MAXP - 1 || influence < 0 ||
        influence > 2 || aggregation < 0 || aggregation > 1 || !(KP_extent > 0.f) || !(offset_scale == offset_scale) ||
        ld_off < 3 * num_kp || (modulations && ld_mod < num_kp) || mod_logits < 0 || mod_logits > 1)
        return D3F_ERR_ARG;
    if (Nq == 0) return D3F_OK;
    if (!q || !s || !idx || !f || !offsets || !kp_host || !wf) return D3F_ERR_ARG;
    const KpdParams P = kpd_make_params(kp_host, num_kp, KP_extent, influence, aggregation, offset_scale,
                                        modulations ? 1 + mod_logits : 0);
    // (the vector kernels address rows with 24-bit multiplies; larger problems take the one-thread-per-output kernel)
    const bool vec = (Cin % 4 == 0) && (ldf % 4 == 0) && (((uintptr_t)f & 15) == 0) && (((uintptr_t)wf & 15) == 0) &&
                     kp_fits_u24(Nq, Ns, ld_idx, ldf);
    const bool fast = kp_fast_config(num_kp, influence, aggregation);
    bool on_ladder = vec;
    if (vec)       // TQ = min(256 / LQ, 64) queries per workgroup of TQ * LQ threads
        KP_LADDER(on_ladder, kpconv_deform_agg_vec4, 64, Cin, fast, Nq, stream, q, Nq, s, Ns, idx, ld_idx, K, f, ldf, offsets, ld_off,
                  modulations, ld_mod, P, wf, Nq_dev, Ns_dev, q_order);
    if (!on_ladder)
        kpconv_deform_agg_scalar<<<d3f_cdiv((long long)Nq * Cin, 256), 256, 0, stream>>>(q, Nq, s, Ns, idx, ld_idx, K, f, ldf, Cin,
                                                                                          offsets, ld_off, modulations, ld_mod, P, wf, Nq_dev, Ns_dev);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
