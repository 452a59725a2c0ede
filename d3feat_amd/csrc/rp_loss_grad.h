// Loss gradients of every training pair in one call (d3f_loss_gradients; the gradient of desc_loss + det_loss of models/
// KPFCNN_model.py:143-191 with respect to the rows of out_features and out_scores -- what a backward pass of the head and of the decoder
// takes as its seeds.  The regularisation term of :188-191 depends on the weights only and is not part of it).  (included by
// registration.hip after rp_validation.h: the forward's kernels, VP_ROWS / VP_TJ, vp_active, vp_span and vp_nmax are used as they are.)
//
// The definition is in include/d3feat_amd.h.  With G = d loss / d D [n, n] the row gradients are
//   d a_i = sum_j (G[i,j] / D[i,j]) (a_i - p_j)        d p_j = sum_i (G[i,j] / D[i,j]) (p_j - a_i)
// and G[i,j] is a function of D[i,j], KD[i,j] and of four numbers of row i,
//   co_i = (G's diagonal term, the share of a column that ties for cn_i, sg_i / (n se_i), cn_i)
// so the n x n matrix is never stored.  Five launches whatever P is:
//   vp_rows_kernel, vp_pair_kernel   the forward as d3f_validation_pairs runs it: fp, cn, se per row; values and status per pair
//   lg_entries_kernel<C, false>      grid (64-entry tiles, pairs), 256 threads.  Lane l of every wave owns list entry 64 t + l as an
//                     ANCHOR (a_i and its point in registers); the positives go through LDS in tiles of 64 and wave w takes columns
//                     16 w .. 16 w + 15 of each tile, as vp_rows_kernel does.  First sweep: |T_i|, the number of columns whose entry
//                     is bit-equal to cn_i.  Then co_i (float64, rounded once) and the entry's score gradient go to the workspace.
//                     Second sweep: d a_i, an fmaf chain per wave over its columns in ascending order; the four waves' partial sums
//                     are added in wave order and the entry's C numbers go to the workspace.  Its prologue writes zeros to every
//                     word of both outputs.
//   lg_entries_kernel<C, true>       the same body with the roles exchanged: a lane owns entry j as a POSITIVE and streams the
//                     anchors and their co_i; one sweep, d p_j per entry.
//   lg_resolve_kernel  one thread per list entry: the first entry that names a row (anchor list before positive list) adds the
//                     anchor entries that name it in list order, then the positive entries in list order (tf.gather's gradient),
//                     and writes the row.
// No float atomic, no workgroup waits for another; every sum in an order that depends on (n, P, the lists) only: two calls give
// equal bits, and P pairs in one call the bits of P calls.  One arithmetic for D in all three kernels (rg_desc_d2 squares the
// differences: exchanging its arguments changes no bit), so "ties for cn_i" and "live" mean the same in every kernel.
#pragma once

struct LgParams {
    float radius, pos_margin, neg_margin, log_scale, det_weight;
    int keypts_num, nmax, contrastive;
};

// the pair has a gradient: evaluated by the forward (the skip rule) with every index inside its rows
__device__ __forceinline__ bool lg_go(int n, const LgParams& prm, const int* __restrict__ status, int p) {
    return vp_active(n, prm.nmax, prm.keypts_num) && status[p] == 0;
}

template <int C, bool COLS>
__global__ void __launch_bounds__(256) lg_entries_kernel(const float* __restrict__ desc, int ldd, const float* __restrict__ score, int lds,
                                                         const float* __restrict__ pts, int ldp, int n_rows, const int* __restrict__ row0,
                                                         const int* __restrict__ anc, const int* __restrict__ pos, int ld_idx,
                                                         const int* __restrict__ n_dev, const int* __restrict__ status, int P, LgParams prm,
                                                         const double4* __restrict__ fw, float4* __restrict__ co, float* __restrict__ es,
                                                         float* __restrict__ ent, int ws_ld, float* __restrict__ gdesc, int ldg,
                                                         float* __restrict__ gscore, int ldgs) {
    __shared__ __attribute__((aligned(16))) float tile[VP_TJ * C];
    __shared__ float tpt[VP_TJ * 3];
    __shared__ float4 sco[VP_TJ];
    __shared__ int red_cnt[4][VP_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (!COLS) {
        // every word of both outputs: the resolve pass, two launches on, writes the named rows over these zeros
        const size_t step = (size_t)gridDim.x * gridDim.y * 256, words = (size_t)n_rows * (C + 1);
        for (size_t e = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; e < words; e += step) {
            const size_t r = e / (C + 1);
            const int c = (int)(e - r * (C + 1));
            if (c < C) gdesc[r * ldg + c] = 0.f;
            else gscore[r * ldgs] = 0.f;
        }
    }
    const float m = prm.neg_margin, L = prm.log_scale;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        // the same for the whole workgroup up to the tile loop
        const int n = n_dev[p];
        if (!lg_go(n, prm, status, p) || (int)blockIdx.x * VP_ROWS >= n) continue;
        const int base = row0[p], N = vp_span(base, row0[p + 1], n_rows);
        const int* A = anc + (size_t)p * ld_idx;
        const int* B = pos + (size_t)p * ld_idx;
        const int* S = COLS ? A : B;                                // the list whose descriptors are streamed
        const int e = blockIdx.x * VP_ROWS + lane;
        const int ia = e < n ? A[e] : -1, io = COLS ? (e < n ? B[e] : -1) : ia;
        const bool have = io >= 0 && io < N, have_a = ia >= 0 && ia < N;
        float own[C], g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            own[c] = have ? desc[(size_t)(base + io) * ldd + c] : 0.f;
            g[c] = 0.f;
        }
        const float px = have_a ? pts[(size_t)(base + ia) * ldp] : 0.f;
        const float py = have_a ? pts[(size_t)(base + ia) * ldp + 1] : 0.f;
        const float pz = have_a ? pts[(size_t)(base + ia) * ldp + 2] : 0.f;
        // (fp32 numbers kept as float64 by the forward: the conversion back is exact; -1 equals no entry)
        const float cn = (!COLS && e < n) ? (float)fw[(size_t)p * ws_ld + e].y : -1.f;
        float4 mine = make_float4(0.f, 0.f, 0.f, -1.f);
        int cnt = 0;
        for (int pass = COLS ? 1 : 0; pass < 2; ++pass) {
            for (int t0 = 0; t0 < n; t0 += VP_TJ) {
                const int nt = min(VP_TJ, n - t0);
                __syncthreads();                                   // the previous tile (or sweep, or pair) has been read
                for (int k = threadIdx.x; k < nt * C; k += 256) {
                    const int j = k / C, r = S[t0 + j];
                    tile[k] = (r >= 0 && r < N) ? desc[(size_t)(base + r) * ldd + (k - j * C)] : 0.f;
                }
                for (int k = threadIdx.x; k < nt * 3; k += 256) {
                    const int j = k / 3, r = A[t0 + j];
                    tpt[k] = (r >= 0 && r < N) ? pts[(size_t)(base + r) * ldp + (k - j * 3)] : 0.f;
                }
                if (COLS && (int)threadIdx.x < nt) sco[threadIdx.x] = co[(size_t)p * ws_ld + t0 + threadIdx.x];
                __syncthreads();
                const int je = min(16 * w + 16, nt);
                for (int j = 16 * w; j < je; ++j) {
                    const float* tr = tile + j * C;
                    const float d2 = rg_desc_d2<C>(own, tr);
                    const float D = __fsqrt_rn(d2 + 1e-12f);
                    const bool diag = (t0 + j == e);
                    const float val = diag ? D + 1e5f : D;         // the entry cn is the minimum of, in the forward's arithmetic
                    if (pass == 0) {
                        cnt += (val == cn) ? 1 : 0;
                        continue;
                    }
                    // KD[i,j] with i the row: the anchor's point minus the column's, as the forward subtracts them
                    const float dx = COLS ? tpt[3 * j] - px : px - tpt[3 * j];
                    const float dy = COLS ? tpt[3 * j + 1] - py : py - tpt[3 * j + 1];
                    const float dz = COLS ? tpt[3 * j + 2] - pz : pz - tpt[3 * j + 2];
                    const float kd = __fsqrt_rn(((dx * dx + dy * dy) + dz * dz) + 1e-12f);
                    const float4 k = COLS ? sco[j] : mine;         // co of the entry's ROW
                    const float u = m - D;
                    float G = diag ? k.x : 0.f;
                    if (val == k.w) G += k.y;
                    if (!diag && !(kd < prm.radius) && D < m) G -= (k.z * expf((L * u) * u)) * u;
                    const float q = G / D;
                    // rows: + q (a_i - p_j); columns: - q (a_i - p_j) = q (p_j - a_i): the owner's descriptor minus the streamed one
#pragma unroll
                    for (int c = 0; c < C; ++c) g[c] = fmaf(q, own[c] - tr[c], g[c]);
                }
            }
            if (pass == 0) {
                red_cnt[w][lane] = cnt;
                __syncthreads();
                if (w == 0) {
                    float4 k = make_float4(0.f, 0.f, 0.f, -1.f);
                    if (e < n) {
                        const double T = (double)(((red_cnt[0][lane] + red_cnt[1][lane]) + red_cnt[2][lane]) + red_cnt[3][lane]);
                        const double4 r = fw[(size_t)p * ws_ld + e];          // fp, cn, sum of exp, (sum of the negatives)
                        const double dn = (double)n, wd = (double)prm.det_weight;
                        const int ib = B[e];
                        const double sab = (prm.det_weight != 0.f && have_a && ib >= 0 && ib < N)
                            ? ((double)score[(size_t)(base + ia) * lds] + (double)score[(size_t)(base + ib) * lds]) + 1e-6 : 0.0;
                        double circ = 0.0, hp = 0.0, hn = 0.0;
                        if (prm.contrastive) {
                            hp = (r.x - (double)prm.pos_margin >= 0.0) ? 1.0 : 0.0;      // tf.maximum: the gradient goes to its first
                            hn = ((double)m - r.y >= 0.0) ? 1.0 : 0.0;                   // argument on equality
                        } else {
                            const double x = (double)L * (r.x - (double)prm.pos_margin) + log(r.z);
                            circ = (1.0 / (1.0 + exp(-x))) / dn;                           // softplus' = sigmoid
                        }
                        const double ws = prm.det_weight != 0.f ? wd * sab / dn : 0.0;
                        k.x = (float)((circ + hp / dn) + ws);
                        k.y = (float)(-((hn / dn + ws) / (T > 0.0 ? T : 1.0)));
                        k.z = (float)(circ / r.z);
                        k.w = (float)r.y;
                        co[(size_t)p * ws_ld + e] = k;
                        es[(size_t)p * ws_ld + e] = prm.det_weight != 0.f ? (float)(wd * (r.x - r.y) / dn) : 0.f;
                    }
                    sco[lane] = k;
                }
                __syncthreads();
                mine = sco[lane];
            }
        }
        // the four waves' partial sums, added to wave 0's in wave order through the tile's LDS ([c][lane]: no bank conflict)
        for (int ww = 1; ww < 4; ++ww) {
            __syncthreads();
            if (w == ww) {
#pragma unroll
                for (int c = 0; c < C; ++c) tile[c * VP_ROWS + lane] = g[c];
            }
            __syncthreads();
            if (w == 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] += tile[c * VP_ROWS + lane];
            }
        }
        if (w == 0 && e < n) {
            float4* dst = (float4*)(ent + ((size_t)p * ws_ld + e) * C);
#pragma unroll
            for (int c = 0; c < C; c += 4) dst[c / 4] = make_float4(g[c], g[c + 1], g[c + 2], g[c + 3]);
        }
        // (the next pair's first barrier orders these LDS reads before anything is written again)
    }
}

template <int C>
__device__ __forceinline__ void lg_add_entry(float* acc, const float* __restrict__ src) {
    const float4* s4 = (const float4*)src;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
        const float4 v = s4[c / 4];
        acc[c] += v.x; acc[c + 1] += v.y; acc[c + 2] += v.z; acc[c + 3] += v.w;
    }
}

template <int C>
__global__ void __launch_bounds__(256) lg_resolve_kernel(int n_rows, const int* __restrict__ row0, const int* __restrict__ anc,
                                                         const int* __restrict__ pos, int ld_idx, const int* __restrict__ n_dev,
                                                         const int* __restrict__ status, int P, LgParams prm, const float* __restrict__ es,
                                                         const float* __restrict__ ea, const float* __restrict__ ep, int ws_ld,
                                                         float* __restrict__ gdesc, int ldg, float* __restrict__ gscore, int ldgs) {
    __shared__ int sA[D3F_VALIDATION_NMAX], sB[D3F_VALIDATION_NMAX];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const int n = n_dev[p];
        if (!lg_go(n, prm, status, p) || (int)blockIdx.x * 256 >= 2 * n) continue;
        const int base = row0[p], N = vp_span(base, row0[p + 1], n_rows);
        __syncthreads();                                           // the previous pair's lists have been read
        for (int k = threadIdx.x; k < n; k += 256) {
            sA[k] = anc[(size_t)p * ld_idx + k];
            sB[k] = pos[(size_t)p * ld_idx + k];
        }
        __syncthreads();
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= 2 * n) continue;                                  // (no barrier follows in this iteration)
        const bool is_b = e >= n;
        const int i = is_b ? e - n : e, r = is_b ? sB[i] : sA[i];
        bool owner = r >= 0 && r < N;                              // (status 0 says so already)
        const float* esp = es + (size_t)p * ws_ld;
        float acc[C], sacc = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        // the first entry that names row r owns it: an anchor entry before every positive entry
        for (int k = 0; owner && k < n; ++k) {
            if (sA[k] != r) continue;
            if (is_b || k < i) { owner = false; break; }
            lg_add_entry<C>(acc, ea + ((size_t)p * ws_ld + k) * C);
            sacc += esp[k];
        }
        for (int k = 0; owner && k < n; ++k) {
            if (sB[k] != r) continue;
            if (is_b && k < i) { owner = false; break; }
            lg_add_entry<C>(acc, ep + ((size_t)p * ws_ld + k) * C);
            sacc += esp[k];
        }
        if (owner) {
            float* dst = gdesc + (size_t)(base + r) * ldg;
#pragma unroll
            for (int c = 0; c < C; ++c) dst[c] = acc[c];
            gscore[(size_t)(base + r) * ldgs] = sacc;
        }
    }
}

static inline size_t lg_ws_ld(int ld_idx) { return (size_t)d3f_cdiv(vp_nmax(ld_idx), VP_ROWS) * VP_ROWS; }

extern "C" size_t d3f_loss_gradients_workspace_bytes(int P, int ld_idx, int C) {
    if (P < 0 || ld_idx < 1 || (C != 16 && C != 32 && C != 64)) return 0;
    const size_t rows = (size_t)(P > 0 ? P : 1) * lg_ws_ld(ld_idx);
    return d3f_align(rows * sizeof(double4)) + d3f_align(rows * sizeof(float4)) + d3f_align(rows * sizeof(float))
        + 2 * d3f_align(rows * C * sizeof(float)) + 256;
}

extern "C" int d3f_loss_gradients(const float* desc, int ldd, int C, const float* score, int lds, const float* points, int ldp, int n_rows,
                                  const int* row0_dev, const int* anc_dev, const int* pos_dev, int ld_idx, const int* n_dev, int P,
                                  float safe_radius, int keypts_num, float det_loss_weight, float pos_margin, float neg_margin,
                                  float log_scale, int contrastive, float* grad_desc, int ldg, float* grad_score, int ldgs, float* values,
                                  int* status, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (C != 16 && C != 32 && C != 64) || ldd < C || lds < 1 || ldp < 3 || n_rows < 0 || ld_idx < 1 || keypts_num < 0) return D3F_ERR_ARG;
    if (ldg < C || ldgs < 1 || (contrastive != 0 && contrastive != 1)) return D3F_ERR_ARG;
    if (!(safe_radius == safe_radius) || !(det_loss_weight == det_loss_weight) || !(pos_margin == pos_margin)) return D3F_ERR_ARG;
    if (!(neg_margin > 0.f) || !(log_scale > 0.f) || !(log_scale * neg_margin * neg_margin <= 80.f)) return D3F_ERR_ARG;
    if (n_rows > 0 && (!grad_desc || !grad_score)) return D3F_ERR_ARG;
    if (P > 0 && (!desc || !score || !points || !row0_dev || !anc_dev || !pos_dev || !n_dev || !values || !status)) return D3F_ERR_ARG;
    LgParams prm;
    prm.radius = safe_radius; prm.pos_margin = pos_margin; prm.neg_margin = neg_margin; prm.log_scale = log_scale;
    prm.det_weight = det_loss_weight; prm.keypts_num = keypts_num; prm.nmax = vp_nmax(ld_idx); prm.contrastive = contrastive;
    const int fill = (int)(d3f_cdiv(n_rows, 1024) < 65535 ? d3f_cdiv(n_rows, 1024) : 65535);
    if (P == 0) {                                                    // no pairs: zeros
        if (n_rows > 0)
            rg_dispatch_C(C, [&](auto c) {
                lg_entries_kernel<decltype(c)::value, false><<<dim3(1, fill), 256, 0, stream>>>(
                    desc, ldd, score, lds, points, ldp, n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, status, 0, prm, nullptr, nullptr,
                    nullptr, nullptr, 0, grad_desc, ldg, grad_score, ldgs);
            });
        D3F_LAUNCH_CHECK();
        return D3F_OK;
    }
    if (!workspace || workspace_bytes < d3f_loss_gradients_workspace_bytes(P, ld_idx, C)) return D3F_ERR_WORKSPACE;
    const int nmax = prm.nmax, tiles = d3f_cdiv(nmax, VP_ROWS), ws_ld = tiles * VP_ROWS;
    const size_t rows = (size_t)P * ws_ld;
    D3fArena ar(workspace, workspace_bytes);
    double4* fw = ar.take<double4>(rows);
    float4* co = ar.take<float4>(rows);
    float* es = ar.take<float>(rows);
    float* ea = ar.take<float>(rows * C);
    float* ep = ar.take<float>(rows * C);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const int py = P < 65535 ? P : 65535;
    const dim3 grid(tiles, py), grid_fill(tiles, py > fill ? py : fill), grid_res(d3f_cdiv(2 * nmax, 256), py);
    rg_dispatch_C(C, [&](auto c) {
        constexpr int CC = decltype(c)::value;
        vp_rows_kernel<CC><<<grid, 256, 0, stream>>>(desc, ldd, points, ldp, n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, P, nmax,
                                                     safe_radius, keypts_num, neg_margin, log_scale, fw, ws_ld);
        vp_pair_kernel<<<py, 256, 0, stream>>>(score, lds, n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, P, nmax, keypts_num,
                                               det_loss_weight, pos_margin, neg_margin, log_scale, fw, ws_ld, values, status);
        lg_entries_kernel<CC, false><<<grid_fill, 256, 0, stream>>>(desc, ldd, score, lds, points, ldp, n_rows, row0_dev, anc_dev, pos_dev,
                                                                    ld_idx, n_dev, status, P, prm, fw, co, es, ea, ws_ld, grad_desc, ldg,
                                                                    grad_score, ldgs);
        lg_entries_kernel<CC, true><<<grid, 256, 0, stream>>>(desc, ldd, score, lds, points, ldp, n_rows, row0_dev, anc_dev, pos_dev, ld_idx,
                                                              n_dev, status, P, prm, fw, co, es, ep, ws_ld, grad_desc, ldg, grad_score,
                                                              ldgs);
        lg_resolve_kernel<CC><<<grid_res, 256, 0, stream>>>(n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, status, P, prm, es, ea, ep,
                                                            ws_ld, grad_desc, ldg, grad_score, ldgs);
    });
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
