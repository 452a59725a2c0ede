// Batch normalisation in training mode with its epilogue (LeakyReLU, residual add), and its backward: d3f_batch_norm_train,
// d3f_batch_norm_backward.  Included by pool_head.hip beside d3f_affine_act.  The definition and the summation order are in
// include/d3feat_amd.h; nothing here uses an atomic on float data, and two calls give equal bits.
//
// One tile geometry under all five kernels, a function of the capacity M and of C only (bn_geo):
//   S    rows per slice: d3f_slice_rows(M) -- 256, doubled until at most 128 slices cover the capacity;
//   LQ   lanes across one row, each holding a QUAD of four consecutive columns: the power of two >= ceil(C / 4), at most 16, so a
//        workgroup covers 4 LQ <= 64 columns and a wavefront reads 64 / LQ whole runs of 16 LQ contiguous bytes: C <= 16 gives a
//        wavefront 16 .. 64 rows, C >= 64 gives it four rows of 256 bytes;
//   R    = 256 / LQ row chains per workgroup; chain r takes the rows n0 + r, n0 + r + R, ... of its slice in ascending order;
//   grid (slices of the capacity, ceil(ceil(C / 4) / LQ) column blocks); a slice at or beyond n leaves at once.
// Which kernel: the <true> instantiations (one 16-byte access per quad) when C % 4 == 0, every leading dimension is a multiple of 4
// and every base pointer is 16-byte aligned (bn_vec); the <false> ones (four guarded 4-byte accesses per quad) otherwise.  Both map
// rows and columns to threads in the same way, so the sums do not depend on the path.
// A column sum: every chain adds its rows in float64 from 0; the R chains are added by the tree  red[r] += red[r + s],  s = R / 2 .. 1;
// the slice partials go to the workspace and are added in ascending slice order from 0 by whoever needs the total.
//
// Forward, three launches:
//   1  bn_sum_kernel        part0[slice, c] = sum of x; clears the ticket of launch 2
//   2  bn_var_kernel        mean = (sum of part0) / n per workgroup; part1[slice, c] = sum of (x - mean)^2; the LAST workgroup
//                           (d3f_last_block) writes mean and rstd and updates the moving statistics
//   3  bn_apply_kernel      y = act((x - mean) rstd gamma + beta + residual)
//   (offset-only form: launch 3 alone.)
// Backward, two launches:
//   1  bn_bwd_sum_kernel    part0[slice, c] = sum of g, part1[slice, c] = sum of g xhat
//   2  bn_bwd_apply_kernel  every workgroup adds the partials of its <= 64 columns (a workspace's bytes are arbitrary before the first
//                           launch of a call, so there is no cleared ticket for a last-workgroup finish here: the finish is done by
//                           all, in the same order); gx, gres; the workgroups of slice 0 write ggamma and gbeta
#pragma once
#include <initializer_list>

#include "prims.h"

struct BnGeo {
    int S, slices, LQ, R, cblocks;
};
static inline BnGeo bn_geo(int M, int C) {
    BnGeo g;
    g.S = d3f_slice_rows(M);
    g.slices = d3f_cdiv(M, g.S);
    const int Cq = d3f_cdiv(C, 4);
    g.LQ = 1;
    while (g.LQ < Cq && g.LQ < 16) g.LQ *= 2;
    g.R = 256 / g.LQ;
    g.cblocks = d3f_cdiv(Cq, g.LQ);
    return g;
}

// this thread's place in the tile
struct BnLane {
    int r, c, n0, n1;      // row chain, first column of the quad, the slice's rows [n0, n1)
    bool live;             // the quad holds a column
};
__device__ __forceinline__ BnLane bn_lane(int n, int S, int LQ, int C) {
    BnLane t;
    t.r = threadIdx.x / LQ;
    t.c = (blockIdx.y * LQ + threadIdx.x % LQ) * 4;
    t.live = t.c < C;
    const long long n0 = (long long)blockIdx.x * S;
    t.n0 = (int)min(n0, (long long)n);
    t.n1 = (int)min(n0 + S, (long long)n);
    return t;
}

template <bool VEC>
__device__ __forceinline__ void bn_ld4(const float* p, int c, int C, float v[4]) {
    if (VEC) {
        const float4 f = *(const float4*)(p + c);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c + j < C) ? p[c + j] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void bn_st4(float* p, int c, int C, const float v[4]) {
    if (VEC) {
        *(float4*)(p + c) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C) p[c + j] = v[j];
    }
}
// a vector of C floats (mean, gamma, ...), NULL -> fill
__device__ __forceinline__ void bn_ldcol(const float* p, int c, int C, float fill, float v[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (p && c + j < C) ? p[c + j] : fill;
}

// the tree over the R chains of the workgroup; the totals arrive in the threads of chain 0.  All 256 threads call this.
__device__ __forceinline__ void bn_chain_tree(double acc[4], double* red, int LQ) {
    const int t = threadIdx.x, R = 256 / LQ, r = t / LQ;
    __syncthreads();                                          // (ends an earlier use of red)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[t * 4 + j] = acc[j];
    __syncthreads();
    for (int s = R >> 1; s > 0; s >>= 1) {
        if (r < s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[t * 4 + j] += red[(t + s * LQ) * 4 + j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = red[t * 4 + j];
}

// the slice partials of column c added in ascending slice order
__device__ __forceinline__ double bn_total(const double* part, int nsl, int C, int c) {
    double s = 0.0;
    for (int sl = 0; sl < nsl; sl += 16) {                    // sixteen partials requested before any is added: a chain of dependent
        double v[16];                                         // round trips to L2 would cost more than the rows of the slice
#pragma unroll
        for (int u = 0; u < 16; ++u)
            v[u] = sl + u < nsl ? __hip_atomic_load(&part[(size_t)(sl + u) * C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (sl + u < nsl) s += v[u];
    }
    return s;
}
// ... of the workgroup's <= 64 columns into tot[0 .. 63] (LDS); a barrier follows
__device__ __forceinline__ void bn_block_totals(const double* part, int nsl, int C, int LQ, double* tot) {
    const int c = blockIdx.y * LQ * 4 + threadIdx.x;
    if ((int)threadIdx.x < LQ * 4) tot[threadIdx.x] = c < C ? bn_total(part, nsl, C, c) : 0.0;
    __syncthreads();
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_sum_kernel(const float* __restrict__ x, int ldx, int M, const int* __restrict__ M_dev, int C, int S,
                                                     int LQ, double* __restrict__ part0, unsigned* __restrict__ ticket) {
    __shared__ double red[256 * 4];
    const int n = d3f_dyn(M, M_dev);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ticket = 0u;
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const BnLane t = bn_lane(n, S, LQ, C);
    const int R = 256 / LQ;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.live)
        for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += (double)v[u][j];
                }
        }
    bn_chain_tree(acc, red, LQ);
    if (t.r == 0 && t.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c + j < C) part0[(size_t)blockIdx.x * C + t.c + j] = acc[j];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_var_kernel(const float* __restrict__ x, int ldx, int M, const int* __restrict__ M_dev, int C, int S,
                                                     int LQ, const double* part0, double* part1, unsigned* ticket, float eps,
                                                     float one_minus_momentum, float* __restrict__ moving_mean,
                                                     float* __restrict__ moving_var, float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double red[256 * 4];
    __shared__ double tot[64];
    const int n = d3f_dyn(M, M_dev);
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const int nsl = (n + S - 1) / S;
    const BnLane t = bn_lane(n, S, LQ, C);
    const int R = 256 / LQ;
    bn_block_totals(part0, nsl, C, LQ, tot);
    double mu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mu[j] = tot[(threadIdx.x % LQ) * 4 + j] / (double)n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.live)
        for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double d = (double)v[u][j] - mu[j];
                        acc[j] += d * d;
                    }
                }
        }
    bn_chain_tree(acc, red, LQ);
    if (t.r == 0 && t.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c + j < C) part1[(size_t)blockIdx.x * C + t.c + j] = acc[j];
    }
    if (!d3f_last_block(ticket, (unsigned)nsl * gridDim.y)) return;
    for (int c = threadIdx.x; c < C; c += 256) {
        const double m = bn_total(part0, nsl, C, c) / (double)n;
        const double var = bn_total(part1, nsl, C, c) / (double)n;
        const float bm = (float)m, bv = (float)var;
        mean[c] = bm;
        mean[C + c] = (float)(m - (double)bm);                // the remainder: x - mean is taken as (x - mean[c]) - mean[C + c]
        rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (moving_mean) {
            const float mm = moving_mean[c], mv = moving_var[c];
            moving_mean[c] = mm - (mm - bm) * one_minus_momentum;          // (never contracted: -ffp-contract=off)
            moving_var[c] = mv - (mv - bv) * one_minus_momentum;
        }
    }
}

// y = act(z), z = (x - mean) rstd gamma + beta + residual, or x + beta + residual without gamma.  y may be the residual's buffer: a
// thread reads its quad of the residual before it writes the same quad of y.
template <bool VEC>
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* x, int ldx, int M, const int* __restrict__ M_dev, int C, int S, int LQ,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, const float* res,
                                                       int ldr, int leaky, float alpha, float* y, int ldy) {
    const int n = d3f_dyn(M, M_dev);
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const BnLane t = bn_lane(n, S, LQ, C);
    if (!t.live) return;
    const int R = 256 / LQ;
    float mu[4], ml[4], rs[4], ga[4], be[4];
    bn_ldcol(gamma ? mean : nullptr, t.c, C, 0.f, mu);
    bn_ldcol(gamma ? mean + C : nullptr, t.c, C, 0.f, ml);
    bn_ldcol(gamma ? rstd : nullptr, t.c, C, 1.f, rs);
    bn_ldcol(gamma, t.c, C, 1.f, ga);
    bn_ldcol(beta, t.c, C, 0.f, be);
    for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
        float v[4][4], q[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (row + u * R < t.n1) {
                bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
                if (res) bn_ld4<VEC>(res + (size_t)(row + u * R) * ldr, t.c, C, q[u]);
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (row + u * R < t.n1) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float z = gamma ? (((v[u][j] - mu[j]) - ml[j]) * rs[j]) * ga[j] + be[j] : v[u][j] + be[j];
                    if (res) z += q[u][j];
                    o[j] = (leaky && !(z > 0.f)) ? z * alpha : z;
                }
                bn_st4<VEC>(y + (size_t)(row + u * R) * ldy, t.c, C, o);
            }
    }
}

// g = gy (y > 0 ? 1 : alpha) under the activation (y == 0 takes alpha, as LeakyReluGrad), gy otherwise
__device__ __forceinline__ float bn_masked(float gy, float y, int leaky, float alpha) { return (leaky && !(y > 0.f)) ? gy * alpha : gy; }

template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_sum_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ y, int ldy,
                                                         const float* __restrict__ gy, int ldg, int M, const int* __restrict__ M_dev, int C,
                                                         int S, int LQ, int has_gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, int leaky, float alpha, double* __restrict__ part0,
                                                         double* __restrict__ part1) {
    __shared__ double red[256 * 4];
    const int n = d3f_dyn(M, M_dev);
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const BnLane t = bn_lane(n, S, LQ, C);
    const int R = 256 / LQ;
    float mu[4], ml[4], rs[4];
    bn_ldcol(has_gamma ? mean : nullptr, t.c, C, 0.f, mu);
    bn_ldcol(has_gamma ? mean + C : nullptr, t.c, C, 0.f, ml);
    bn_ldcol(has_gamma ? rstd : nullptr, t.c, C, 1.f, rs);
    double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.live)
        for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
            float v[4][4], a[4][4], g[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) {
                    bn_ld4<VEC>(gy + (size_t)(row + u * R) * ldg, t.c, C, g[u]);
                    if (leaky) bn_ld4<VEC>(y + (size_t)(row + u * R) * ldy, t.c, C, a[u]);
                    if (has_gamma) bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * R < t.n1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float gm = bn_masked(g[u][j], leaky ? a[u][j] : 1.f, leaky, alpha);
                        sb[j] += (double)gm;
                        if (has_gamma) sg[j] += (double)gm * (double)(((v[u][j] - mu[j]) - ml[j]) * rs[j]);
                    }
                }
        }
    bn_chain_tree(sb, red, LQ);
    if (has_gamma) bn_chain_tree(sg, red, LQ);
    if (t.r == 0 && t.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c + j < C) {
                part0[(size_t)blockIdx.x * C + t.c + j] = sb[j];
                if (has_gamma) part1[(size_t)blockIdx.x * C + t.c + j] = sg[j];
            }
    }
}

// gx = gamma rstd (g - gbeta / n - xhat ggamma / n), gres = g; without gamma gx = g.  gx or gres may be gy's buffer (not both): a
// thread reads its quad of gy before it writes the same quad.
template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* x, int ldx, const float* y, int ldy, const float* gy, int ldg, int M,
                                                           const int* __restrict__ M_dev, int C, int S, int LQ,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, int leaky, float alpha,
                                                           const double* __restrict__ part0, const double* __restrict__ part1, float* gx,
                                                           int ldgx, float* __restrict__ ggamma, float* __restrict__ gbeta, float* gres,
                                                           int ldgr) {
    __shared__ double totb[64], totg[64];
    const int n = d3f_dyn(M, M_dev);
    if ((long long)blockIdx.x * S >= (long long)n) return;
    const int nsl = (n + S - 1) / S;
    const BnLane t = bn_lane(n, S, LQ, C);
    const int R = 256 / LQ;
    bn_block_totals(part0, nsl, C, LQ, totb);
    if (gamma) bn_block_totals(part1, nsl, C, LQ, totg);
    if (blockIdx.x == 0 && (int)threadIdx.x < LQ * 4) {
        const int c = blockIdx.y * LQ * 4 + threadIdx.x;
        if (c < C) {
            gbeta[c] = (float)totb[threadIdx.x];
            if (gamma) ggamma[c] = (float)totg[threadIdx.x];
        }
    }
    if (!t.live) return;
    float mu[4], ml[4], rs[4], ga[4], kb[4], kg[4];
    bn_ldcol(gamma ? mean : nullptr, t.c, C, 0.f, mu);
    bn_ldcol(gamma ? mean + C : nullptr, t.c, C, 0.f, ml);
    bn_ldcol(gamma ? rstd : nullptr, t.c, C, 1.f, rs);
    bn_ldcol(gamma, t.c, C, 1.f, ga);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kb[j] = (float)(totb[(threadIdx.x % LQ) * 4 + j] / (double)n);
        kg[j] = gamma ? (float)(totg[(threadIdx.x % LQ) * 4 + j] / (double)n) : 0.f;
        ga[j] *= rs[j];
    }
    for (int row = t.n0 + t.r; row < t.n1; row += 4 * R) {
        float v[4][4], a[4][4], g[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (row + u * R < t.n1) {
                bn_ld4<VEC>(gy + (size_t)(row + u * R) * ldg, t.c, C, g[u]);
                if (leaky) bn_ld4<VEC>(y + (size_t)(row + u * R) * ldy, t.c, C, a[u]);
                if (gamma) bn_ld4<VEC>(x + (size_t)(row + u * R) * ldx, t.c, C, v[u]);
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (row + u * R < t.n1) {
                float gm[4], o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gm[j] = bn_masked(g[u][j], leaky ? a[u][j] : 1.f, leaky, alpha);
                    o[j] = gamma ? ga[j] * ((gm[j] - kb[j]) - (((v[u][j] - mu[j]) - ml[j]) * rs[j]) * kg[j]) : gm[j];
                }
                bn_st4<VEC>(gx + (size_t)(row + u * R) * ldgx, t.c, C, o);
                if (gres) bn_st4<VEC>(gres + (size_t)(row + u * R) * ldgr, t.c, C, gm);
            }
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
static inline bool bn_sizes_ok(int M, int C) { return M >= 0 && C >= 1 && C <= (1 << 20); }
static inline bool bn_vec(int C, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs) {
    if (C % 4) return false;
    for (int ld : lds)
        if (ld % 4) return false;
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15) return false;
    return true;
}

extern "C" size_t d3f_batch_norm_workspace_bytes(int M, int C) {
    if (!bn_sizes_ok(M, C)) return 0;
    const BnGeo g = bn_geo(M, C);
    return 256 + 2 * d3f_align((size_t)(g.slices > 0 ? g.slices : 1) * C * sizeof(double));
}

struct BnScratch {
    unsigned* ticket;
    double *part0, *part1;
};
static inline BnScratch bn_scratch(void* workspace, int M, int C) {
    const BnGeo g = bn_geo(M, C);
    BnScratch s;
    s.ticket = (unsigned*)workspace;
    s.part0 = (double*)((char*)workspace + 256);
    s.part1 = (double*)((char*)s.part0 + d3f_align((size_t)(g.slices > 0 ? g.slices : 1) * C * sizeof(double)));
    return s;
}

extern "C" int d3f_batch_norm_train(const float* x, int ldx, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                                    float* moving_mean, float* moving_var, const float* residual, int ldr, int leaky, float alpha, float* y,
                                    int ldy, float* mean, float* rstd, const int* M_dev, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!bn_sizes_ok(M, C) || ldx < C || ldy < C || (residual && ldr < C) || !beta || (gamma && (!mean || !rstd || !(eps > 0.f))) ||
        ((moving_mean != nullptr) != (moving_var != nullptr)) || (M > 0 && (!x || !y)))
        return D3F_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < d3f_batch_norm_workspace_bytes(M, C)) return D3F_ERR_WORKSPACE;
    if (M == 0) return D3F_OK;
    const BnGeo g = bn_geo(M, C);
    const BnScratch ws = bn_scratch(workspace, M, C);
    const dim3 grid(g.slices, g.cblocks);
    const bool vec = bn_vec(C, {ldx, ldy, residual ? ldr : 0}, {x, y, residual});
    if (gamma) {
        const float omm = (float)(1.0 - (double)momentum);
        if (vec) {
            bn_sum_kernel<true><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, ws.part0, ws.ticket);
            bn_var_kernel<true><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, ws.part0, ws.part1, ws.ticket, eps, omm, moving_mean,
                                                          moving_var, mean, rstd);
        } else {
            bn_sum_kernel<false><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, ws.part0, ws.ticket);
            bn_var_kernel<false><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, ws.part0, ws.part1, ws.ticket, eps, omm, moving_mean,
                                                           moving_var, mean, rstd);
        }
        D3F_LAUNCH_CHECK();
    }
    if (vec)
        bn_apply_kernel<true><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, gamma, beta, mean, rstd, residual, ldr, leaky, alpha, y,
                                                        ldy);
    else
        bn_apply_kernel<false><<<grid, 256, 0, stream>>>(x, ldx, M, M_dev, C, g.S, g.LQ, gamma, beta, mean, rstd, residual, ldr, leaky, alpha, y,
                                                         ldy);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

extern "C" int d3f_batch_norm_backward(const float* x, int ldx, const float* y, int ldy, const float* gy, int ldg, int M, int C,
                                       const float* gamma, const float* mean, const float* rstd, int leaky, float alpha, float* gx,
                                       int ldgx, float* ggamma, float* gbeta, float* gres, int ldgr, const int* M_dev, void* workspace,
                                       size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!bn_sizes_ok(M, C) || ldg < C || ldgx < C || (gres && ldgr < C) || (leaky && ldy < C) || !gbeta ||
        (gamma && (ldx < C || !mean || !rstd || !ggamma)) || (gres && gres == gx) ||
        (M > 0 && (!gy || !gx || (leaky && !y) || (gamma && !x))))
        return D3F_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < d3f_batch_norm_workspace_bytes(M, C)) return D3F_ERR_WORKSPACE;
    if (M == 0) return D3F_OK;
    const BnGeo g = bn_geo(M, C);
    const BnScratch ws = bn_scratch(workspace, M, C);
    const dim3 grid(g.slices, g.cblocks);
    const bool vec = bn_vec(C, {ldg, ldgx, gamma ? ldx : 0, leaky ? ldy : 0, gres ? ldgr : 0},
                            {gy, gx, gamma ? x : nullptr, leaky ? y : nullptr, gres});
    const int hg = gamma ? 1 : 0;
    if (vec) {
        bn_bwd_sum_kernel<true><<<grid, 256, 0, stream>>>(x, ldx, y, ldy, gy, ldg, M, M_dev, C, g.S, g.LQ, hg, mean, rstd, leaky, alpha, ws.part0,
                                                          ws.part1);
        bn_bwd_apply_kernel<true><<<grid, 256, 0, stream>>>(x, ldx, y, ldy, gy, ldg, M, M_dev, C, g.S, g.LQ, gamma, mean, rstd, leaky, alpha,
                                                            ws.part0, ws.part1, gx, ldgx, ggamma, gbeta, gres, ldgr);
    } else {
        bn_bwd_sum_kernel<false><<<grid, 256, 0, stream>>>(x, ldx, y, ldy, gy, ldg, M, M_dev, C, g.S, g.LQ, hg, mean, rstd, leaky, alpha, ws.part0,
                                                           ws.part1);
        bn_bwd_apply_kernel<false><<<grid, 256, 0, stream>>>(x, ldx, y, ldy, gy, ldg, M, M_dev, C, g.S, g.LQ, gamma, mean, rstd, leaky, alpha,
                                                             ws.part0, ws.part1, gx, ldgx, ggamma, gbeta, gres, ldgr);
    }
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
