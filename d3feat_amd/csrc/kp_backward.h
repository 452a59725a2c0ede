// Backward of the rigid KPConv (d3f_kpconv_backward): from the gradient with respect to the output of KPConv_ops to the gradients with
// respect to the support feature rows (gf) and K_values (gW).  Included at the end of kpconv.hip: the forward is recomputed by the
// entry points above as they are (d3f_row_positive, d3f_kpconv_aggregate), and the message kernel is the query-centred mirror of
// kpconv_agg_vec4 built from the same pieces of kp_shared.h.  The definition and the summation orders are in include/d3feat_amd.h;
// nothing here uses an atomic on global memory, and no workgroup waits for another.
//
// Launches, behind the table of d3f_neighbor_transpose_qs (the caller's):
//   1  row flags                    d3f_row_positive
//   2  wf, inv_cnt                  d3f_kpconv_aggregate
//   3  kpb_scale_kernel             g = gout * inv_cnt, contiguous: both contractions read the same rows whatever ldg is
//   4  kpb_gw_kernel                (gW wanted) per slice of query rows: part[slice] = wf^T g, v_mfma_f32_32x32x2_f32
//   5  kpb_gw_reduce_kernel         (gW wanted) gW = the slice partials added in ascending slice order
//   6  kpb_transpose_kernel         (gf wanted) Wt[o, m] = W[m, o]
//   7  d3f_gemm_f32                 (gf wanted) gwf = g Wt into wf's buffer (wf is dead after 4)
//   8  kpb_msg_vec4 / _scalar       (gf wanted) msg[e, :] = sum_p h[n, k, p] gwf[n, p, :] for every valid edge e = n K + k
//   9  kpb_gather_kernel            (gf wanted) gf[j, :] = the chain over row j's segment of msg[edges[t], :]
#pragma once

// ---- gW: the contraction over the query rows, in slices ---------------------------------------------------------------------------
// The slice length depends on the CAPACITY Nq only: 256 rows, doubled until at most 128 slices cover the capacity (common.h).
static inline int kpb_slice_rows(int Nq) { return d3f_slice_rows(Nq); }

// g[n, o] = gout[n, o] * inv_cnt[n] for the nq real rows
__global__ void __launch_bounds__(256) kpb_scale_kernel(const float* __restrict__ gout, int ldg, const float* __restrict__ inv_cnt, int Nq,
                                                        const int* __restrict__ Nq_dev, int Cout, float* __restrict__ g) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)d3f_dyn(Nq, Nq_dev) * Cout) return;
    const int n = (int)(t / Cout), o = (int)(t % Cout);
    g[t] = gout[(size_t)n * ldg + o] * inv_cnt[n];
}

// one wavefront per (32 rows of gW's M = num_kp * Cin, 32 output channels, slice): D[32 x 32] += A[32 x 2] B[2 x 32] per pair of query
// rows, A[i][k] = wf[n + k, m0 + i] (the 32 lanes of a half read 128 consecutive bytes of one wf row), B[k][j] = g[n + k, o0 + j].
// One accumulator chain over the slice's rows in ascending order, eight rows requested before any is multiplied.  ldw / ldg: the
// leading dimensions of wf and g (d3f_kpconv_backward passes M and Cout, d3f_gemm_tn_f32 its callers' own).
__global__ void __launch_bounds__(64) kpb_gw_kernel(const float* __restrict__ wf, int ldw, const float* __restrict__ g, int ldg, int Nq,
                                                    const int* __restrict__ Nq_dev, int M, int Cout, int S, float* __restrict__ part) {
    const int nq = d3f_dyn(Nq, Nq_dev);
    const int slice = blockIdx.z;
    const long long n0l = (long long)slice * S;
    if (n0l >= (long long)nq) return;
    const int n0 = (int)n0l, n1 = (int)min((long long)nq, n0l + S);
    const int lane = threadIdx.x, i = lane & 31, kh = lane >> 5;
    const int m = blockIdx.x * 32 + i, o = blockIdx.y * 32 + i;
    const bool mok = m < M, ook = o < Cout;
    kp_f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    for (int n = n0; n < n1; n += 8) {
        float a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = n + 2 * u + kh;
            const bool ok = r < n1;
            a[u] = (ok && mok) ? wf[(size_t)r * ldw + m] : 0.f;
            b[u] = (ok && ook) ? g[(size_t)r * ldg + o] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (n + 2 * u < n1) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], c, 0, 0, 0);
    }
    float* dst = part + (size_t)slice * M * Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mm = blockIdx.x * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (mm < M && ook) dst[(size_t)mm * Cout + o] = c[r];
    }
}

__global__ void __launch_bounds__(256) kpb_gw_reduce_kernel(const float* __restrict__ part, int Nq, const int* __restrict__ Nq_dev,
                                                            size_t words, int S, float* __restrict__ gW) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= words) return;
    const int nq = max(d3f_dyn(Nq, Nq_dev), 0);
    const int nsl = nq / S + (nq % S ? 1 : 0);
    float sum = 0.f;
    for (int sl = 0; sl < nsl; ++sl) sum += part[(size_t)sl * words + t];
    gW[t] = sum;
}

__global__ void __launch_bounds__(256) kpb_transpose_kernel(const float* __restrict__ W, int M, int Cout, float* __restrict__ Wt) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)M * Cout) return;
    const size_t o = t / M, m = t - o * M;
    Wt[t] = W[m * Cout + o];
}

// ---- messages ---------------------------------------------------------------------------------------------------------------------
// kpconv_agg_vec4 turned round: phase A is the forward's (the influences of a chunk of pairs go to LDS); in phase B a lane holds
// gwf[n, 0 .. 14, 4 cl .. 4 cl + 3] in registers, loaded once per query, and stores one float4 of msg per valid neighbour slot: four
// chains of fused multiply-adds over ascending p, started at zero.  Shadow slots store nothing: no segment lists them.
template <int LQ, bool FAST>
__global__ void __launch_bounds__(256)
kpb_msg_vec4(const float* __restrict__ q, int Nq, const float* __restrict__ s, int Ns, const int* __restrict__ idx, int ld_idx, int K,
             KpParams P, const float* __restrict__ gwf, float* __restrict__ msg, const int* __restrict__ Nq_dev,
             const int* __restrict__ Ns_dev, const int* __restrict__ q_order) {
    constexpr int TQ = 256 / LQ;
    Nq = d3f_dyn(Nq, Nq_dev);
    Ns = d3f_dyn(Ns, Ns_dev);
    if ((int)(blockIdx.x * TQ) >= Nq) return;
    const int tile = (int)d3f_xcd_tile(blockIdx.x, (unsigned)((Nq + TQ - 1) / TQ));
    constexpr int KC = LQ;
    constexpr int WS = KC * 16 + 4;
    __shared__ __attribute__((aligned(16))) float lw[TQ * WS];
    __shared__ int lidx[TQ * KC];
    const int tid = threadIdx.x;
    const int ql = tid / LQ, cl = tid % LQ;
    const KpQuery Q = kp_query(tile * TQ + ql, Nq, q_order, q, idx, ld_idx);
    constexpr int Cin = LQ * 4;
    float g[KP_MAXP - 1][4];
#pragma unroll
    for (int p = 0; p < KP_MAXP - 1; ++p) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (Q.live && p < P.num_kp) v = *(const float4*)&gwf[((size_t)Q.g * P.num_kp + p) * Cin + 4 * cl];
        g[p][0] = v.x; g[p][1] = v.y; g[p][2] = v.z; g[p][3] = v.w;
    }
    float* mrow = msg + (size_t)(Q.live ? Q.g : 0) * K * Cin + 4 * cl;
    KpPair pr = kp_pair_fetch<false>(kp_pair_index(Q.idrow, Q.live, cl, K, Ns), Ns, s, nullptr);   // chunk 0's pair
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int id_next = kp_pair_index(Q.idrow, Q.live, k0 + KC + cl, K, Ns);
        {   // ---- phase A: thread = (query ql, neighbour k0 + cl) ----
            float w[KP_MAXP];
            kp_pair_influences<FAST>(P, pr, Q.x, Q.y, Q.z, w);
            lidx[ql * KC + cl] = pr.id;
            kp_store_w(&lw[ql * WS + cl * 16], cl, w);
        }
        __syncthreads();
        pr = kp_pair_fetch<false>(id_next, Ns, s, nullptr);
        // ---- phase B: thread = (query ql, channels 4*cl .. 4*cl+3) ----
        const int kend = min(KC, K - k0);
        for (int kk = 0; kk < kend; ++kk) {
            if (lidx[ql * KC + kk] < 0) continue;            // shadow slot (a dead query's slots are all shadows)
            float w[16];
            kp_load_w(&lw[ql * WS + kk * 16], kk, w);
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
#pragma unroll
            for (int p = 0; p < KP_MAXP - 1; ++p) {
                m0 = fmaf(w[p], g[p][0], m0);
                m1 = fmaf(w[p], g[p][1], m1);
                m2 = fmaf(w[p], g[p][2], m2);
                m3 = fmaf(w[p], g[p][3], m3);
            }
            *(float4*)&mrow[(size_t)(k0 + kk) * Cin] = make_float4(m0, m1, m2, m3);
        }
        __syncthreads();
    }
}

// any other Cin (1 included), unaligned rows, stacks beyond the 24-bit row addressing: one thread per (query, channel)
__global__ void __launch_bounds__(256)
kpb_msg_scalar(const float* __restrict__ q, int Nq, const float* __restrict__ s, int Ns, const int* __restrict__ idx, int ld_idx, int K,
               int Cin, KpParams P, const float* __restrict__ gwf, float* __restrict__ msg, const int* __restrict__ Nq_dev,
               const int* __restrict__ Ns_dev) {
    Nq = d3f_dyn(Nq, Nq_dev);
    Ns = d3f_dyn(Ns, Ns_dev);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)Nq * Cin) return;
    const int qg = (int)(t / Cin), c = (int)(t % Cin);
    const float qx = q[3 * (size_t)qg], qy = q[3 * (size_t)qg + 1], qz = q[3 * (size_t)qg + 2];
    float g[KP_MAXP - 1];
#pragma unroll
    for (int p = 0; p < KP_MAXP - 1; ++p) g[p] = p < P.num_kp ? gwf[((size_t)qg * P.num_kp + p) * Cin + c] : 0.f;
    for (int k = 0; k < K; ++k) {
        const int id = idx[(size_t)qg * ld_idx + k];
        if (id < 0 || id >= Ns) continue;
        float w[KP_MAXP];
        kp_influences(P, s[3 * (size_t)id] - qx, s[3 * (size_t)id + 1] - qy, s[3 * (size_t)id + 2] - qz, w);
        float m = 0.f;
#pragma unroll
        for (int p = 0; p < KP_MAXP - 1; ++p) m = fmaf(w[p], g[p], m);
        msg[((size_t)qg * K + k) * Cin + c] = m;
    }
}

// ---- segment gather ---------------------------------------------------------------------------------------------------------------
// 2^LOG lanes per support row, VEC channels per lane and pass: gf[j, :] is one fp32 chain per channel over row j's segment of the
// table, in ascending position -- the rule (and the four-rows-in-flight loop) of hb_gather_kernel, for any Cin.  The table is the
// caller's: positions and edges are range-checked, never trusted.
template <int VEC>
__global__ void __launch_bounds__(256)
kpb_gather_kernel(const float* __restrict__ msg, int Nq, int K, int Cin, const int* __restrict__ Nq_dev, int Ns,
                  const int* __restrict__ Ns_dev, const int* __restrict__ start, const int* __restrict__ edges,
                  float* __restrict__ gf, int ldgf, int log_lanes) {
    const int nq = max(d3f_dyn(Nq, Nq_dev), 0), ns = d3f_dyn(Ns, Ns_dev);
    const int lanes = 1 << log_lanes;
    const long long rowl = (long long)blockIdx.x * (256 >> log_lanes) + (threadIdx.x >> log_lanes);
    if (rowl >= (long long)ns) return;
    const int row = (int)rowl, l = threadIdx.x & (lanes - 1);
    const int items = nq * K;                                   // Nq * K <= 2^31 - 8192: checked by the launcher
    const int s0 = min(max(start[row], 0), items), s1 = min(max(start[row + 1], s0), items);
    for (int c0 = l * VEC; c0 < Cin; c0 += lanes * VEC) {
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        for (int t = s0; t < s1; t += 4) {
            float v[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = (t + u < s1) ? edges[t + u] : -1;
                const bool ok = e >= 0 && e < items;
                if constexpr (VEC == 4) {
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (ok) x = *(const float4*)&msg[(size_t)e * Cin + c0];
                    v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
                } else {
                    v[u][0] = ok ? msg[(size_t)e * Cin + c0] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (t + u < s1) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] += v[u][j];
                }
        }
        float* o = gf + (size_t)row * ldgf + c0;
        if constexpr (VEC == 4) *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else o[0] = acc[0];
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
static inline bool kpb_sizes_ok(int Nq, int Ns, int K, int Cin, int Cout, int num_kp) {
    return Nq >= 0 && Ns >= 0 && K >= 0 && Cin >= 1 && Cout >= 1 && Cin <= (1 << 20) && Cout <= (1 << 20) && num_kp >= 1 &&
           num_kp <= KP_MAXP - 1 && (long long)Nq * K <= (1ll << 31) - 8192 && !(Ns == 0 && Nq > 0);
}

struct KpbSizes {
    size_t rowpos, inv_cnt, g, wf, msg, part, wt, gemm;
};
static inline KpbSizes kpb_sizes(int Nq, int Ns, int K, int Cin, int Cout, int num_kp) {
    const size_t M = (size_t)num_kp * Cin;
    KpbSizes z;
    z.rowpos = Ns > 0 ? (size_t)Ns : 1;
    z.inv_cnt = (size_t)Nq;
    z.g = (size_t)Nq * Cout;
    z.wf = (size_t)Nq * M;
    z.msg = (size_t)Nq * K * Cin;
    z.part = (size_t)d3f_cdiv(Nq, kpb_slice_rows(Nq)) * M * Cout;
    z.wt = M * Cout;
    z.gemm = d3f_gemm_workspace_bytes(Nq, (int)M, Cout, 0);
    return z;
}

extern "C" size_t d3f_kpconv_backward_workspace_bytes(int Nq, int Ns, int K, int Cin, int Cout, int num_kp) {
    if (!kpb_sizes_ok(Nq, Ns, K, Cin, Cout, num_kp)) return 0;
    const KpbSizes z = kpb_sizes(Nq, Ns, K, Cin, Cout, num_kp);
    return d3f_align(z.rowpos) + d3f_align(z.inv_cnt * 4) + d3f_align(z.g * 4) + d3f_align(z.wf * 4) + d3f_align(z.msg * 4) + d3f_align(z.part * 4) +
           d3f_align(z.wt * 4) + d3f_align(z.gemm);
}

extern "C" int d3f_kpconv_backward(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K, const void* f_,
                                   int ldf, int Cin, const float* kp_host, int num_kp, float KP_extent, int influence, int aggregation,
                                   const float* W, const float* gout, int ldg, int Cout, const int* start, const int* edges, float* gf,
                                   int ldgf, float* gW, const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const float* f = (const float*)f_;
    if (!kpb_sizes_ok(Nq, Ns, K, Cin, Cout, num_kp) || ld_idx < K || ldf < Cin || ldg < Cout || (gf && ldgf < Cin) || influence < 0 ||
        influence > 2 || aggregation < 0 || aggregation > 1 || !(KP_extent > 0.f) || feat_bf16 || (!gf && !gW))
        return D3F_ERR_ARG;
    if (!kp_host || !W || (gf && !start) || (Nq > 0 && (!q || !s || !f || !gout || (K > 0 && (!idx || (gf && !edges)))))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_kpconv_backward_workspace_bytes(Nq, Ns, K, Cin, Cout, num_kp)) return D3F_ERR_WORKSPACE;
    const KpbSizes z = kpb_sizes(Nq, Ns, K, Cin, Cout, num_kp);
    D3fArena ar(workspace, workspace_bytes);
    unsigned char* rowpos = ar.take<unsigned char>(z.rowpos);
    float* inv_cnt = ar.take<float>(z.inv_cnt);
    float* g = ar.take<float>(z.g);
    float* wf = ar.take<float>(z.wf);
    float* msg = ar.take<float>(z.msg);
    float* part = ar.take<float>(z.part);
    float* Wt = ar.take<float>(z.wt);
    void* gemm_ws = ar.take<char>(z.gemm);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const int M = num_kp * Cin;
    const size_t words = (size_t)M * Cout;
    const KpParams P = kp_make_params(kp_host, num_kp, KP_extent, influence, aggregation);
    // without a query or without a neighbour slot there is no edge: both gradients are exact zeros, written by the two kernels that
    // write the outputs (no slice to add, empty segments)
    const bool work = Nq > 0 && K > 0;
    // the forward's quantities, by the forward's own entry points
    if (work) {
        int rc = d3f_row_positive(f, Ns, ldf, Cin, rowpos, Ns_dev, 0, stream_);
        if (rc != D3F_OK) return rc;
        rc = d3f_kpconv_aggregate(q, Nq, s, Ns, idx, ld_idx, K, f, ldf, Cin, rowpos, kp_host, num_kp, KP_extent, influence, aggregation, wf,
                                  inv_cnt, Nq_dev, Ns_dev, q_order, 0, stream_);
        if (rc != D3F_OK) return rc;
        kpb_scale_kernel<<<d3f_cdiv((long long)Nq * Cout, 256), 256, 0, stream>>>(gout, ldg, inv_cnt, Nq, Nq_dev, Cout, g);
        D3F_LAUNCH_CHECK();
    }
    if (gW) {
        const int S = kpb_slice_rows(Nq);
        if (work) {
            const dim3 grid(d3f_cdiv(M, 32), d3f_cdiv(Cout, 32), d3f_cdiv(Nq, S));
            kpb_gw_kernel<<<grid, 64, 0, stream>>>(wf, M, g, Cout, Nq, Nq_dev, M, Cout, S, part);
        }
        kpb_gw_reduce_kernel<<<d3f_cdiv((long long)words, 256), 256, 0, stream>>>(part, work ? Nq : 0, Nq_dev, words, S, gW);
        D3F_LAUNCH_CHECK();
    }
    if (gf) {
        if (work) {
            kpb_transpose_kernel<<<d3f_cdiv((long long)words, 256), 256, 0, stream>>>(W, M, Cout, Wt);
            D3F_LAUNCH_CHECK();
            float* gwf = wf;                                     // wf is dead: the gW launches above are ahead on the stream
            const int rc = d3f_gemm_f32(g, Cout, Wt, M, gwf, M, Nq, M, Cout, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.f, gemm_ws, z.gemm,
                                        Nq_dev, 0, stream_);
            if (rc != D3F_OK) return rc;
            const bool vec = (Cin % 4 == 0) && kp_fits_u24(Nq, Ns, ld_idx, ldf);
            const bool fast = kp_fast_config(num_kp, influence, aggregation);
            bool on_ladder = vec;
            if (vec)
                KP_LADDER(on_ladder, kpb_msg_vec4, 256, Cin, fast, Nq, stream, q, Nq, s, Ns, idx, ld_idx, K, P, gwf, msg, Nq_dev, Ns_dev,
                          q_order);
            if (!on_ladder)
                kpb_msg_scalar<<<d3f_cdiv((long long)Nq * Cin, 256), 256, 0, stream>>>(q, Nq, s, Ns, idx, ld_idx, K, Cin, P, gwf, msg, Nq_dev,
                                                                                       Ns_dev);
            D3F_LAUNCH_CHECK();
        }
        if (Ns > 0) {
            const bool vec = (Cin % 4 == 0) && (ldgf % 4 == 0) && (((uintptr_t)gf & 15) == 0);
            const int per = vec ? Cin / 4 : Cin;
            int lg = 0;
            while (lg < 6 && (1 << lg) < per) ++lg;
            const int blocks = d3f_cdiv(Ns, 256 >> lg);
            if (vec) kpb_gather_kernel<4><<<blocks, 256, 0, stream>>>(msg, Nq, K, Cin, Nq_dev, Ns, Ns_dev, start, edges, gf, ldgf, lg);
            else kpb_gather_kernel<1><<<blocks, 256, 0, stream>>>(msg, Nq, K, Cin, Nq_dev, Ns, Ns_dev, start, edges, gf, ldgf, lg);
            D3F_LAUNCH_CHECK();
        }
    }
    return D3F_OK;
}

// ---- out = A^T B ------------------------------------------------------------------------------------------------------------------
// d3f_gemm_tn_f32: the gW contraction above on the caller's own operands (the backward of a unary convolution: gW = x^T gy).  The same
// two kernels, the same slices, the same order: on contiguous operands the bits of d3f_kpconv_backward's gW for the same rows.
static inline bool kpb_tn_sizes_ok(int M, int Ca, int Cb) { return M >= 0 && Ca >= 1 && Cb >= 1 && Ca <= (1 << 20) && Cb <= (1 << 20); }

extern "C" size_t d3f_gemm_tn_workspace_bytes(int M, int Ca, int Cb) {
    if (!kpb_tn_sizes_ok(M, Ca, Cb)) return 0;
    return d3f_align((size_t)d3f_cdiv(M, kpb_slice_rows(M)) * Ca * Cb * 4 + 4);
}

extern "C" int d3f_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, int M, int Ca, int Cb, float* out, const int* M_dev,
                               void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!kpb_tn_sizes_ok(M, Ca, Cb) || lda < Ca || ldb < Cb || !out || (M > 0 && (!A || !B))) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_gemm_tn_workspace_bytes(M, Ca, Cb)) return D3F_ERR_WORKSPACE;
    float* part = (float*)workspace;
    const int S = kpb_slice_rows(M);
    const size_t words = (size_t)Ca * Cb;
    if (M > 0) {
        const dim3 grid(d3f_cdiv(Ca, 32), d3f_cdiv(Cb, 32), d3f_cdiv(M, S));
        kpb_gw_kernel<<<grid, 64, 0, stream>>>(A, lda, B, ldb, M, M_dev, Ca, Cb, S, part);
    }
    kpb_gw_reduce_kernel<<<d3f_cdiv((long long)words, 256), 256, 0, stream>>>(part, M, M_dev, words, S, out);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
