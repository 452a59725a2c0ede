// Validation figures of every pair in one call (d3f_validation_pairs; models/KPFCNN_model.py:131-186 + utils/loss.py of the
// reference: circle loss, contrastive loss, detection loss, accuracy, mean positive / negative distance; the split totals of
// utils/trainer.py:442-452).  The forward; its gradient is rp_loss_grad.h, which runs these kernels first.  (included by registration.hip; of its kernels only rg_desc_d2 and rg_dispatch_C.)
//
// A pair is a stack [anchor; positive] of rows with n index pairs (ai, pi).  With D[i,j] = sqrt(|f[ai[i]] - f[pi[j]]|^2 + 1e-12) and
// KD[i,j] the same over the points of ai[i] and ai[j], every figure is a sum over i of a function of four per-row numbers
//   fp_i = D[i,i]     cn_i = min_j (D[i,j] + 1e5 [i == j])     se_i = sum_j exp(z[i,j])     ng_i = sum_j D[i,j] [i != j and KD >= r]
// so the n x n matrices of the reference (and its n x n x C differences) are never stored:
//   vp_rows_kernel    grid (64-row tiles of the longest list, pairs), 256 threads.  Lane l of every wave owns anchor row 64 t + l, its
//                     descriptor and point in registers; the positive rows go through LDS in tiles of 64, wave w takes columns
//                     16 w .. 16 w + 15 of each tile (every lane reads the same LDS address: a broadcast, no bank conflict).  The four
//                     partial results of a row are combined through LDS in wave order and the row's four numbers go to the workspace.
//   vp_pair_kernel    one workgroup per pair: range check of n and of every index, the skip rule, then the per-row terms (softplus,
//                     hinge, score weight) evaluated and summed in float64 by a fixed tree; thread 0 writes the pair's eight floats and its status.
//   vp_totals_kernel  one workgroup: the six filtered sums (float64) and their counts over the P pairs, fixed tree.
// Three launches whatever P is; no memset (every word that is read was written by the launch before), no atomics, no workgroup waits
// for another, every sum in an order that depends on (n, P) only: two calls give equal bits.
//
// One arithmetic for all entries: d2 is the fmaf chain over c ascending of (a[c] - b[c]), so two equal (ai, pi) entries give
// D[i,j] bit-equal to D[i,i] and the row counts as accurate, as in the reference.  The point metric is the library's: (dx dx + dy dy)
// + dz dz, never contracted.  z <= log_scale * neg_margin^2 (the launcher refuses a product above 80), so expf cannot overflow
// and no running maximum is kept.  An index outside the pair's rows is never dereferenced: the row or column is taken as zeros here
// and vp_pair_kernel replaces the pair's figures by the skip tuple and raises its status.
#pragma once

#define VP_ROWS 64          // anchor rows per workgroup (one per lane)
#define VP_TJ 64            // positive rows per LDS tile
#define VP_ST_INDEX 1       // D3F_VP_INDEX_RANGE
#define VP_ST_COUNT 2       // D3F_VP_COUNT_RANGE

// the pair takes part: n inside 1 .. nmax and not below half of keypts_num (KPFCNN_model.py:172-174: 0.5 * keypts_num <= n)
__device__ __forceinline__ bool vp_active(int n, int nmax, int keypts_num) {
    return n >= 1 && n <= nmax && 2 * (long long)n >= (long long)keypts_num;
}

// rows of the stack [base, end) of a pair; 0 when the offsets do not lie inside the n_rows rows of the arrays, so that every index
// of such a pair is out of range and nothing is read for it
__device__ __forceinline__ int vp_span(int base, int end, int n_rows) {
    return (base >= 0 && end >= base && end <= n_rows) ? end - base : 0;
}

template <int C>
__global__ void __launch_bounds__(256) vp_rows_kernel(const float* __restrict__ desc, int ldd, const float* __restrict__ pts, int ldp,
                                                      int n_rows, const int* __restrict__ row0, const int* __restrict__ anc,
                                                      const int* __restrict__ pos, int ld_idx, const int* __restrict__ n_dev, int P,
                                                      int nmax, float radius, int keypts_num, float neg_margin, float log_scale,
                                                      double4* __restrict__ ws, int ws_ld) {
    __shared__ __attribute__((aligned(16))) float tile[VP_TJ * C];
    __shared__ float tpt[VP_TJ * 3];
    __shared__ float red_fp[4][VP_ROWS], red_cn[4][VP_ROWS];
    __shared__ double red_se[4][VP_ROWS], red_ng[4][VP_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        // the same for the whole workgroup up to the tile loop
        const int n = n_dev[p];
        if (!vp_active(n, nmax, keypts_num) || (int)blockIdx.x * VP_ROWS >= n) continue;
        const int base = row0[p], N = vp_span(base, row0[p + 1], n_rows);
        const int* A = anc + (size_t)p * ld_idx;
        const int* B = pos + (size_t)p * ld_idx;
        const int i = blockIdx.x * VP_ROWS + lane;
        const int ai = i < n ? A[i] : -1;
        const bool have = ai >= 0 && ai < N;
        float a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = have ? desc[(size_t)(base + ai) * ldd + c] : 0.f;
        const float px = have ? pts[(size_t)(base + ai) * ldp] : 0.f;
        const float py = have ? pts[(size_t)(base + ai) * ldp + 1] : 0.f;
        const float pz = have ? pts[(size_t)(base + ai) * ldp + 2] : 0.f;
        float fp = 0.f, cn = 3.402823466e38f;
        double se = 0.0, ng = 0.0;
        for (int t0 = 0; t0 < n; t0 += VP_TJ) {
            const int nt = min(VP_TJ, n - t0);
            __syncthreads();                                       // the previous tile (or pair) has been read
            for (int e = threadIdx.x; e < nt * C; e += 256) {
                const int j = e / C, pj = B[t0 + j];
                tile[e] = (pj >= 0 && pj < N) ? desc[(size_t)(base + pj) * ldd + (e - j * C)] : 0.f;
            }
            for (int e = threadIdx.x; e < nt * 3; e += 256) {
                const int j = e / 3, aj = A[t0 + j];
                tpt[e] = (aj >= 0 && aj < N) ? pts[(size_t)(base + aj) * ldp + (e - j * 3)] : 0.f;
            }
            __syncthreads();
            float tng = 0.f, tse = 0.f;                            // at most 16 terms each in fp32, then widened
            const int je = min(16 * w + 16, nt);
            for (int j = 16 * w; j < je; ++j) {
                const float d2 = rg_desc_d2<C>(a, tile + j * C);   // (tile is 16-byte aligned: 128-bit LDS reads)
                const float D = __fsqrt_rn(d2 + 1e-12f);
                const float dx = px - tpt[3 * j], dy = py - tpt[3 * j + 1], dz = pz - tpt[3 * j + 2];
                const float kd = __fsqrt_rn(((dx * dx + dy * dy) + dz * dz) + 1e-12f);
                const bool diag = (t0 + j == i);
                const bool masked = diag || kd < radius;           // the positive itself, or a false negative (strict <)
                if (diag) fp = D;
                cn = fminf(cn, diag ? D + 1e5f : D);               // the safe radius is NOT applied here (loss.py:151)
                tng += masked ? 0.f : D;
                const float u = neg_margin - D;
                const float z = (masked || D >= neg_margin) ? 0.f : (log_scale * u) * u;
                tse += expf(z);                                     // a masked entry counts exp(0) = 1, as the reference's 1e8 terms do
            }
            ng += (double)tng;
            se += (double)tse;
        }
        red_fp[w][lane] = fp;
        red_cn[w][lane] = cn;
        red_se[w][lane] = se;
        red_ng[w][lane] = ng;
        __syncthreads();
        if (w == 0 && i < n) {
            // fp is D[i,i] in the one wave that met the diagonal and 0 elsewhere (D > 0): the maximum; the rest in wave order
            const float f = fmaxf(fmaxf(red_fp[0][lane], red_fp[1][lane]), fmaxf(red_fp[2][lane], red_fp[3][lane]));
            const float m = fminf(fminf(red_cn[0][lane], red_cn[1][lane]), fminf(red_cn[2][lane], red_cn[3][lane]));
            const double s = ((red_se[0][lane] + red_se[1][lane]) + red_se[2][lane]) + red_se[3][lane];
            const double g = ((red_ng[0][lane] + red_ng[1][lane]) + red_ng[2][lane]) + red_ng[3][lane];
            ws[(size_t)p * ws_ld + i] = make_double4((double)f, (double)m, s, g);
        }
        // (the next pair's first barrier orders these reads before anything is written to red_* again: two barriers lie between)
    }
}

__global__ void __launch_bounds__(256) vp_pair_kernel(const float* __restrict__ score, int lds, int n_rows, const int* __restrict__ row0,
                                                      const int* __restrict__ anc, const int* __restrict__ pos, int ld_idx,
                                                      const int* __restrict__ n_dev, int P, int nmax, int keypts_num, float det_weight,
                                                      float pos_margin, float neg_margin, float log_scale,
                                                      const double4* __restrict__ ws, int ws_ld, float* __restrict__ values,
                                                      int* __restrict__ status) {
    __shared__ double red[256];
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const int n = n_dev[p];
        const int base = row0[p], N = vp_span(base, row0[p + 1], n_rows);
        const int* A = anc + (size_t)p * ld_idx;
        const int* B = pos + (size_t)p * ld_idx;
        int st = (n < 0 || n > nmax) ? VP_ST_COUNT : 0;
        if (!st) {
            int bad = 0;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int x = A[i], y = B[i];
                bad |= (x < 0 || x >= N || y < 0 || y >= N) ? 1 : 0;
            }
            if (__syncthreads_or(bad)) st = VP_ST_INDEX;
        }
        float* out = values + (size_t)p * 8;
        if (st || !vp_active(n, nmax, keypts_num)) {                // the tuple of KPFCNN_model.py:179-184
            if (threadIdx.x == 0) {
                out[0] = out[1] = out[2] = 0.f;
                out[3] = -1.f;
                out[4] = out[5] = out[6] = 0.f;
                out[7] = (float)n;
                status[p] = st;
            }
            continue;
        }
        double circle = 0.0, contrastive = 0.0, det = 0.0, dpos = 0.0, dneg = 0.0, acc = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) {
            // fp, cn (fp32 distances), sum of exp, sum of the negatives.  From here on float64: the figures then carry the rounding
            // of the distances and of the exponentials only
            const double4 r = ws[(size_t)p * ws_ld + i];
            const double diff = r.x - r.y;
            acc += diff <= 0.0 ? 1.0 : 0.0;                          // (the difference of two floats: its sign is exact)
            const double x = (double)log_scale * (r.x - (double)pos_margin) + log(r.z);
            double sp;  // softplus with the shortcuts of TF's kernel, the form of head32_kernel: x, exp(x) or log1p(exp(x))
            if (x > 15.0) sp = x;
            else if (x < -15.0) sp = exp(x);
            else sp = log1p(exp(x));
            circle += sp / (double)log_scale;
            contrastive += fmax(r.x - (double)pos_margin, 0.0) + fmax((double)neg_margin - r.y, 0.0);
            if (det_weight != 0.f)
                det += diff * (((double)score[(size_t)(base + A[i]) * lds] + (double)score[(size_t)(base + B[i]) * lds]) + 1e-6);
            dpos += r.x;
            dneg += r.w;
        }
        circle = d3f_block_sum(circle, red);
        contrastive = d3f_block_sum(contrastive, red);
        det = d3f_block_sum(det, red);
        dpos = d3f_block_sum(dpos, red);
        dneg = d3f_block_sum(dneg, red);
        acc = d3f_block_sum(acc, red);
        if (threadIdx.x == 0) {
            const double dn = (double)n;
            const float fn = (float)n;
            out[0] = (float)(circle / dn);
            out[1] = (float)(contrastive / dn);
            out[2] = det_weight != 0.f ? (float)((double)det_weight * (det / dn)) : 0.f;
            out[3] = (float)acc / fn;
            out[4] = (float)(dpos / dn);
            // mean over all n * n entries, then * n / (n - 1) (loss.py:152); at n = 1 the reference's fp32 0 * 1 / 0 = NaN
            out[5] = n > 1 ? (float)(dneg / (dn * dn) * dn / (dn - 1.0)) : ((float)(dneg / (dn * dn)) * fn) / (fn - 1.f);
            out[6] = (float)acc;
            out[7] = fn;
            status[p] = 0;
        }
    }
}

// sums[k], counts[k], k = 0 .. 5 (circle, contrastive, det, accuracy, d_pos, d_neg): over the pairs whose figure is != 0 (a NaN is:
// utils/trainer.py:442-452 appends it), accuracy > 0
__global__ void __launch_bounds__(256) vp_totals_kernel(const float* __restrict__ values, int P, double* __restrict__ sums,
                                                        long long* __restrict__ counts) {
    __shared__ double red[256];
    for (int k = 0; k < 6; ++k) {
        double s = 0.0, c = 0.0;
        for (int p = threadIdx.x; p < P; p += 256) {
            const float v = values[(size_t)p * 8 + k];
            if (k == 3 ? v > 0.f : v != 0.f) { s += (double)v; c += 1.0; }
        }
        s = d3f_block_sum(s, red);
        c = d3f_block_sum(c, red);                                    // (whole numbers below 2^53: exact)
        if (threadIdx.x == 0) { sums[k] = s; counts[k] = (long long)c; }
    }
}

static inline int vp_nmax(int ld_idx) { return ld_idx < D3F_VALIDATION_NMAX ? ld_idx : D3F_VALIDATION_NMAX; }

extern "C" size_t d3f_validation_pairs_workspace_bytes(int P, int ld_idx) {
    if (P < 0 || ld_idx < 1) return 0;
    const size_t ws_ld = (size_t)d3f_cdiv(vp_nmax(ld_idx), VP_ROWS) * VP_ROWS;
    return d3f_align((size_t)(P > 0 ? P : 1) * ws_ld * sizeof(double4)) + 256;
}

extern "C" int d3f_validation_pairs(const float* desc, int ldd, int C, const float* score, int lds, const float* points, int ldp,
                                    int n_rows, const int* row0_dev, const int* anc_dev, const int* pos_dev, int ld_idx, const int* n_dev, int P,
                                    float safe_radius, int keypts_num, float det_loss_weight, float pos_margin, float neg_margin,
                                    float log_scale, float* values, int* status, double* sums, int64_t* counts, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (C != 16 && C != 32 && C != 64) || ldd < C || lds < 1 || ldp < 3 || n_rows < 0 || ld_idx < 1 || keypts_num < 0) return D3F_ERR_ARG;
    if (!(safe_radius == safe_radius) || !(det_loss_weight == det_loss_weight) || !(pos_margin == pos_margin)) return D3F_ERR_ARG;
    if (!(neg_margin > 0.f) || !(log_scale > 0.f) || !(log_scale * neg_margin * neg_margin <= 80.f)) return D3F_ERR_ARG;
    if (!sums || !counts) return D3F_ERR_ARG;
    if (P > 0 && (!desc || !score || !points || !row0_dev || !anc_dev || !pos_dev || !n_dev || !values || !status)) return D3F_ERR_ARG;
    if (P == 0) {                                                    // the totals of no pairs: zeros
        vp_totals_kernel<<<1, 256, 0, stream>>>(values, 0, sums, (long long*)counts);
        D3F_LAUNCH_CHECK();
        return D3F_OK;
    }
    if (!workspace || workspace_bytes < d3f_validation_pairs_workspace_bytes(P, ld_idx)) return D3F_ERR_WORKSPACE;
    const int nmax = vp_nmax(ld_idx), tiles = d3f_cdiv(nmax, VP_ROWS), ws_ld = tiles * VP_ROWS;
    D3fArena ar(workspace, workspace_bytes);
    double4* ws = ar.take<double4>((size_t)P * ws_ld);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const dim3 grid(tiles, P < 65535 ? P : 65535);
    rg_dispatch_C(C, [&](auto c) {
        vp_rows_kernel<decltype(c)::value><<<grid, 256, 0, stream>>>(desc, ldd, points, ldp, n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, P, nmax,
                                                                     safe_radius, keypts_num, neg_margin, log_scale, ws, ws_ld);
    });
    vp_pair_kernel<<<P < 65535 ? P : 65535, 256, 0, stream>>>(score, lds, n_rows, row0_dev, anc_dev, pos_dev, ld_idx, n_dev, P, nmax, keypts_num,
                                                              det_loss_weight, pos_margin, neg_margin, log_scale, ws, ws_ld, values, status);
    vp_totals_kernel<<<1, 256, 0, stream>>>(values, P, sums, (long long*)counts);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
