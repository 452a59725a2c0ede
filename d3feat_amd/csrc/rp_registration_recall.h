// 3DMatch registration recall of every scene at every keypoint count in two launches (d3f_registration_recall; included by
// registration.hip after rp_scene_summary.h)
//
// geometric_registration/3dmatch/evaluate.m of the reference calls external/ElasticReconstruction/mrEvaluateRegistration.m on the .log
// file geometric_registration/evaluate.py:101-110 writes: :21-37 walk the result rows, :44-49 (mrComputeTransformationError) turn
// gt^-1 * result into p = er' * info * er / info(1,1), :51-59 (dcm2quat) give the quaternion.  Here for P pairs x n estimates at once, in
// float64 with every operation rounded on its own (the file is built with -ffp-contract=off; the intrinsics say so again), so that
// numpy restates it bit for bit (tests/recall_np.py):
//   rr_rows_kernel   one thread per row i (pair i / n, column i % n): error, flags
//   rr_scene_kernel  one workgroup per scene: per column five int64 sums over the pairs of the scene, thread t taking the pairs
//                    p0 + t, p0 + t + 256, ..., then the LDS halving tree of d3f_block_sum
// All sums are integers: nothing depends on a summation order.  No atomics, no memset, no workspace: every output element has exactly
// one writer; scene_start travels as a kernel argument, so the call is capturable.
//
// THE ORDER OF THE OPERATIONS (a(r,c): row r, column c; every product and every sum rounded; sums left to right as written).
//   inverse of an affine [A | t] (rr_invert), by cofactors over the determinant -- a general inverse, not A^T:
//     n00 = a11 a22 - a12 a21   n01 = a02 a21 - a01 a22   n02 = a01 a12 - a02 a11
//     n10 = a12 a20 - a10 a22   n11 = a00 a22 - a02 a20   n12 = a02 a10 - a00 a12
//     n20 = a10 a21 - a11 a20   n21 = a01 a20 - a00 a21   n22 = a00 a11 - a01 a10
//     det = (a00 n00 + a01 n10) + a02 n20;   B(r,c) = n(r,c) / det;   u(r) = -((B(r,0) t0 + B(r,1) t1) + B(r,2) t2)
//   E = gt^-1 * result, the affine product (the fourth rows are not read), G = gt^-1 = [B | u], result = [R | w]:
//     E(r,c) = (B(r,0) R(0,c) + B(r,1) R(1,c)) + B(r,2) R(2,c);   E(r,3) = ((B(r,0) w0 + B(r,1) w1) + B(r,2) w2) + u(r)
//   dcm2quat: s = ((1 + E00) + E11) + E22;  q0 = 0.5 sqrt(s);  d = 4 q0;
//     er = [E03, E13, E23, (E21 - E12) / d, (E02 - E20) / d, (E10 - E01) / d]      ([te; -q(2:4)] of the .m file, multiplied out)
//   v(r) = ((((info(r,0) er0 + info(r,1) er1) + info(r,2) er2) + info(r,3) er3) + info(r,4) er4) + info(r,5) er5
//   p = (((((er0 v0 + er1 v1) + er2 v2) + er3 v3) + er4 v4) + er5 v5) / info(0,0)
// Where s > 0 is false (NaN included) p is NaN: MATLAB would go complex for s < 0, which needs an error within rounding of 180 degrees.
// A NaN p is not <= err2: the row is bad.
#define RR_GOOD 1
#define RR_RESULT 2
#define RR_FALSE_POS 4
#define RR_GT 8

// out[0..11] = the inverse [B | u] of the affine a[0..11] (row-major [A | t])
__device__ __forceinline__ void rr_invert(const double* a, double* out) {
    const double a00 = a[0], a01 = a[1], a02 = a[2], a10 = a[4], a11 = a[5], a12 = a[6], a20 = a[8], a21 = a[9], a22 = a[10];
#define RR_N(x, y, z, w) __dsub_rn(__dmul_rn(x, y), __dmul_rn(z, w))
    const double n00 = RR_N(a11, a22, a12, a21), n01 = RR_N(a02, a21, a01, a22), n02 = RR_N(a01, a12, a02, a11);
    const double n10 = RR_N(a12, a20, a10, a22), n11 = RR_N(a00, a22, a02, a20), n12 = RR_N(a02, a10, a00, a12);
    const double n20 = RR_N(a10, a21, a11, a20), n21 = RR_N(a01, a20, a00, a21), n22 = RR_N(a00, a11, a01, a10);
#undef RR_N
    const double det = __dadd_rn(__dadd_rn(__dmul_rn(a00, n00), __dmul_rn(a01, n10)), __dmul_rn(a02, n20));
    const double B[9] = {__ddiv_rn(n00, det), __ddiv_rn(n01, det), __ddiv_rn(n02, det), __ddiv_rn(n10, det), __ddiv_rn(n11, det),
                         __ddiv_rn(n12, det), __ddiv_rn(n20, det), __ddiv_rn(n21, det), __ddiv_rn(n22, det)};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[4 * r] = B[3 * r]; out[4 * r + 1] = B[3 * r + 1]; out[4 * r + 2] = B[3 * r + 2];
        out[4 * r + 3] = -__dadd_rn(__dadd_rn(__dmul_rn(B[3 * r], a[3]), __dmul_rn(B[3 * r + 1], a[7])), __dmul_rn(B[3 * r + 2], a[11]));
    }
}

__global__ void __launch_bounds__(256) rr_rows_kernel(const void* __restrict__ T_est, int logged, const double* __restrict__ gt,
                                                      const double* __restrict__ info, const int* __restrict__ gt_flag,
                                                      const int* __restrict__ result_flag, const int* __restrict__ ids, int rows, int n,
                                                      double err2, double* __restrict__ error, int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int p = i / n;
    const int apart = ids[2 * p + 1] - ids[2 * p] > 1 ? 1 : 0;       // mrEvaluateRegistration.m:10,22: consecutive fragments count nowhere
    const int g = gt_flag[p] != 0 ? 1 : 0;
    const int r = result_flag ? (result_flag[p] != 0 ? 1 : 0) : g;
    int f = (apart & r ? RR_RESULT : 0) | (apart & g ? RR_GT : 0) | (apart & r & (g ^ 1) ? RR_FALSE_POS : 0);
    double e = 0.0;
    if (apart & r & g) {
        double R[12], G[12], E[12];
        if (logged) {                                                 // f64[4, 4] in the .log convention: the first three rows as they are
            const double* T = (const double*)T_est + (size_t)i * 16;
#pragma unroll
            for (int k = 0; k < 12; ++k) R[k] = T[k];
        } else {                                                      // f32[3, 4] source -> target: the log holds its inverse (evaluate.py:104)
            const float* T = (const float*)T_est + (size_t)i * 12;
            double W[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) W[k] = (double)T[k];
            rr_invert(W, R);
        }
        {
            const double* M = gt + (size_t)p * 16;
            double W[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) W[k] = M[k];
            rr_invert(W, G);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double v = __dadd_rn(__dadd_rn(__dmul_rn(G[4 * a], R[c]), __dmul_rn(G[4 * a + 1], R[4 + c])), __dmul_rn(G[4 * a + 2], R[8 + c]));
                E[4 * a + c] = c == 3 ? __dadd_rn(v, G[4 * a + 3]) : v;
            }
        }
        const double s = __dadd_rn(__dadd_rn(__dadd_rn(1.0, E[0]), E[5]), E[10]);
        if (s > 0.0) {
            const double d = __dmul_rn(4.0, __dmul_rn(0.5, __dsqrt_rn(s)));
            const double er[6] = {E[3], E[7], E[11], __ddiv_rn(__dsub_rn(E[9], E[6]), d), __ddiv_rn(__dsub_rn(E[2], E[8]), d),
                                  __ddiv_rn(__dsub_rn(E[4], E[1]), d)};
            const double* I = info + (size_t)p * 36;
            double num = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double v = __dmul_rn(I[6 * a], er[0]);
#pragma unroll
                for (int c = 1; c < 6; ++c) v = __dadd_rn(v, __dmul_rn(I[6 * a + c], er[c]));
                const double t = __dmul_rn(er[a], v);
                num = a ? __dadd_rn(num, t) : t;
            }
            e = __ddiv_rn(num, I[0]);
        } else {
            e = __longlong_as_double(0x7ff8000000000000ll);
        }
        if (e <= err2) f |= RR_GOOD;                                   // not strict (mrEvaluateRegistration.m:31); false for NaN
    }
    error[i] = e;
    flags[i] = f;
}

__global__ void __launch_bounds__(256) rr_scene_kernel(const int* __restrict__ flags, int n, SsStarts starts, long long* __restrict__ figures) {
    __shared__ long long red[256];
    const int s = blockIdx.x;
    const int p0 = starts.v[s], p1 = starts.v[s + 1];
    for (int c = 0; c < n; ++c) {
        long long good = 0, bad = 0, fpos = 0, gtn = 0, rsn = 0;
        for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
            const int f = flags[(size_t)p * n + c];
            good += f & RR_GOOD ? 1 : 0;
            bad += (f & (RR_GOOD | RR_RESULT | RR_FALSE_POS)) == RR_RESULT ? 1 : 0;          // a result with a ground truth that is not good
            fpos += f & RR_FALSE_POS ? 1 : 0;
            gtn += f & RR_GT ? 1 : 0;
            rsn += f & RR_RESULT ? 1 : 0;
        }
        good = d3f_block_sum(good, red); bad = d3f_block_sum(bad, red); fpos = d3f_block_sum(fpos, red);
        gtn = d3f_block_sum(gtn, red); rsn = d3f_block_sum(rsn, red);
        if (threadIdx.x == 0) {
            long long* o = figures + ((size_t)s * n + c) * 5;
            o[0] = good; o[1] = bad; o[2] = fpos; o[3] = gtn; o[4] = rsn;
        }
    }
}

extern "C" int d3f_registration_recall(const void* T_est, int logged, const double* gt, const double* info, const int* gt_flag,
                                       const int* result_flag, const int* ids, int P, int n, const int* scene_start_host, int S,
                                       const double* err2_host, double* error, int* flags, long long* figures, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n < 1 || n > D3F_REPEAT_COUNTS_MAX || (long long)P * n > 0x7fffffffll || !err2_host) return D3F_ERR_ARG;
    const double err2 = err2_host[0];
    if (!(err2 > 0.0)) return D3F_ERR_ARG;                            // NaN too
    SsStarts starts;
    if (!ss_starts(scene_start_host, S, P, starts)) return D3F_ERR_ARG;
    if (P > 0 && (!T_est || !gt || !info || !gt_flag || !ids || !error || !flags)) return D3F_ERR_ARG;
    if (S > 0 && !figures) return D3F_ERR_ARG;
    const int rows = P * n;
    if (rows > 0)
        rr_rows_kernel<<<d3f_cdiv(rows, 256), 256, 0, stream>>>(T_est, logged ? 1 : 0, gt, info, gt_flag, result_flag, ids, rows, n, err2, error, flags);
    if (S > 0) rr_scene_kernel<<<S, 256, 0, stream>>>(flags, n, starts, figures);
    if (rows > 0 || S > 0) D3F_LAUNCH_CHECK();
    return D3F_OK;
}
