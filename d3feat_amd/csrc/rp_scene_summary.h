// ETH generalisation test: np.nan_to_num of the descriptors and the per-scene matching summary (d3f_sanitize_descriptors,
// d3f_matching_summary; included by registration.hip after rp_pose_errors.h)
//
// geometric_registration_eth/evaluate_eth.py of the reference: :26-27 pass the descriptors through np.nan_to_num before matching;
// :67 writes the inlier ratio with 8 decimals, :151 reads it back, :153-163 turn the rows of a scene into recall, average inliers and
// average inlier ratio.  Here:
//   ss_sanitize_kernel  one thread per descriptor element; only an element that changes is written (idempotent, one writer each)
//   ss_rows_kernel      one thread per (pair, count): m = the integer with m / 1e8 == float("%.8f" % (a / b)), in integers
//   ss_scene_kernel     one workgroup per (scene, count): four int64 sums over the pairs of the scene
// All sums are integers: nothing depends on a summation order.  No atomics, no memset, no workspace; scene_start travels as a kernel
// argument, so the call is capturable.
//
// THE ROUNDING.  With a = gt_inliers, b = mutual_count, 0 <= a <= b, the rational x = a 10^8 / b is either exactly a half-integer (a
// tie) or at least 1 / (2 b) away from one; the double fl(a / b) 10^8 differs from x by less than 10^8 2^-53 <= 1.2e-8, far less than
// 1 / (2 b) for b <= 8192.  So away from a tie the correctly rounded decimal of the double is the rounding of the rational:
// m = floor((2 a 10^8 + b) / (2 b)).  On a tie ((2 a 10^8) mod 2 b == b, which needs 512 | b) the decimal conversion rounds the DOUBLE:
// e = fma(fl(a / b), b, -a) is exact (the residual of a correctly rounded quotient is representable), e > 0: the double is above the
// tie, up; e < 0: down; e == 0: the double is the rational, the tie goes to the even integer.
// b = 0 gives m = 0: the convention of registration.PairMatching.ratios (the reference would divide by zero there).  a is clamped to
// 0 .. b.  A pair with gt_flag == 0 gets m = 0 (evaluate_eth.py:43-47).
#define SS_SCENES_MAX D3F_SCENES_MAX
#define SS_E8 100000000ll

struct SsStarts { int v[SS_SCENES_MAX + 1]; };
// the S + 1 host ints of a call: S inside 0 .. SS_SCENES_MAX, ascending from 0 to P; the entries after S are P.  false otherwise.
static inline bool ss_starts(const int* scene_start_host, int S, int P, SsStarts& starts) {
    if (!scene_start_host || S < 0 || S > SS_SCENES_MAX) return false;
    for (int s = 0; s <= S; ++s) {
        starts.v[s] = scene_start_host[s];
        if (s ? starts.v[s] < starts.v[s - 1] : starts.v[s] != 0) return false;
    }
    if (starts.v[S] != P) return false;
    for (int s = S + 1; s <= SS_SCENES_MAX; ++s) starts.v[s] = P;
    return true;
}

__global__ void __launch_bounds__(256) ss_sanitize_kernel(float* __restrict__ kp, long long rows, int ld, int log2C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;                  // element i = row (i >> log2C), column (i mod C)
    if (i >= (rows << log2C)) return;
    float* p = kp + (size_t)(i >> log2C) * ld + 3 + (int)(i & ((1 << log2C) - 1));
    const unsigned u = __float_as_uint(*p);
    if ((u & 0x7f800000u) != 0x7f800000u) return;                     // finite: -0.0 and denormals keep their bits
    // np.nan_to_num: NaN (any sign, any payload) -> +0.0, +inf -> FLT_MAX, -inf -> -FLT_MAX
    *p = (u & 0x007fffffu) ? 0.0f : __uint_as_float((u & 0x80000000u) | 0x7f7fffffu);
}

__device__ __forceinline__ int ss_ratio_e8(int a, int b) {
    if (b <= 0) return 0;
    a = a < 0 ? 0 : (a > b ? b : a);
    const long long num = 2ll * a * SS_E8, den = 2ll * b;
    long long m = (num + b) / den;                                    // round half up of the rational
    if (num % den == b) {                                             // a tie: the double decides
        const double q = __ddiv_rn((double)a, (double)b);
        const double e = __fma_rn(q, (double)b, -(double)a);
        if (e < 0.0 || (e == 0.0 && (m & 1))) m -= 1;
    }
    return (int)m;
}

__global__ void __launch_bounds__(256) ss_rows_kernel(const int* __restrict__ mutual_count, const int* __restrict__ gt_inliers,
                                                      const int* __restrict__ gt_flag, int rows, int n, int* __restrict__ ratio_e8) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    ratio_e8[i] = gt_flag[i / n] ? ss_ratio_e8(gt_inliers[i], mutual_count[i]) : 0;
}

__global__ void __launch_bounds__(256) ss_scene_kernel(const int* __restrict__ gt_inliers, const int* __restrict__ gt_flag,
                                                       const int* __restrict__ ratio_e8, int n, SsStarts starts, double inlier_ratio,
                                                       long long* __restrict__ figures) {
    __shared__ long long red[256];
    const int s = blockIdx.x, c = blockIdx.y;
    const int p0 = starts.v[s], p1 = starts.v[s + 1];
    long long gt = 0, correct = 0, inl = 0, sum_m = 0;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        const size_t i = (size_t)p * n + c;
        const int m = ratio_e8[i];
        if (__ddiv_rn((double)m, 1e8) > inlier_ratio) correct += 1;   // every pair of the scene (evaluate_eth.py:154)
        if (gt_flag[p]) { gt += 1; inl += gt_inliers[i]; sum_m += m; }
    }
    gt = d3f_block_sum(gt, red); correct = d3f_block_sum(correct, red); inl = d3f_block_sum(inl, red); sum_m = d3f_block_sum(sum_m, red);
    if (threadIdx.x == 0) {
        long long* f = figures + ((size_t)s * n + c) * 4;
        f[0] = gt; f[1] = correct; f[2] = inl; f[3] = sum_m;
    }
}

extern "C" int d3f_sanitize_descriptors(float* kp, int n_blocks, int K, int ld, int C, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_blocks < 0 || K < 0 || (C != 16 && C != 32 && C != 64) || ld < C + 3) return D3F_ERR_ARG;
    const long long rows = (long long)n_blocks * K;
    if (rows * C > 0x7fffffffll * 256) return D3F_ERR_ARG;
    if (rows == 0) return D3F_OK;
    if (!kp) return D3F_ERR_ARG;
    ss_sanitize_kernel<<<(unsigned)d3f_cdiv(rows * C, 256), 256, 0, stream>>>(kp, rows, ld, C == 16 ? 4 : (C == 32 ? 5 : 6));
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

extern "C" int d3f_matching_summary(const int* mutual_count, const int* gt_inliers, const int* gt_flag, int P, int n,
                                    const int* scene_start_host, int S, const double* inlier_ratio_host, int* ratio_e8,
                                    long long* figures, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n < 1 || n > D3F_REPEAT_COUNTS_MAX || (long long)P * n > 0x7fffffffll || !inlier_ratio_host) return D3F_ERR_ARG;
    const double inlier_ratio = inlier_ratio_host[0];
    if (inlier_ratio != inlier_ratio) return D3F_ERR_ARG;
    SsStarts starts;
    if (!ss_starts(scene_start_host, S, P, starts)) return D3F_ERR_ARG;
    if (P > 0 && (!mutual_count || !gt_inliers || !gt_flag || !ratio_e8)) return D3F_ERR_ARG;
    if (S > 0 && !figures) return D3F_ERR_ARG;
    const int rows = P * n;
    if (rows > 0) ss_rows_kernel<<<d3f_cdiv(rows, 256), 256, 0, stream>>>(mutual_count, gt_inliers, gt_flag, rows, n, ratio_e8);
    if (S > 0) ss_scene_kernel<<<dim3(S, n), 256, 0, stream>>>(gt_inliers, gt_flag, ratio_e8, n, starts, inlier_ratio, figures);
    if (rows > 0 || S > 0) D3F_LAUNCH_CHECK();
    return D3F_OK;
}
