// KITTI test metric of every estimate in two launches (d3f_pose_errors; included by registration.hip after rp_validation.h)
//
// utils/tester.py:326-344 of the reference, per pair: rte = |t_est - t_gt|, rre = arccos((trace(R_est^T R_gt) - 1) / 2), the three
// AverageMeters updated under rte < 2 and rre < 5 degrees.  Here for P * per_pair estimates at once, in float64 with every operation
// rounded on its own (the file is built with -ffp-contract=off; the intrinsics say so again), so that numpy restates it bit for bit:
//   pe_rows_kernel    one thread per row i (pair i / per_pair, column i % per_pair): rte, rre_deg, flags
//   pe_meters_kernel  one workgroup: per column the eight sums of the header, thread t adding rows p = t, t + 256, ... in ascending
//                     order, then the LDS halving tree 128 .. 1 of d3f_block_sum
// No atomics, no ticket, no memset, no workspace: every output element has exactly one writer.
#define PE_PI 3.141592653589793238462643383279502884

__global__ void __launch_bounds__(256) pe_rows_kernel(const float* __restrict__ T_est, const float* __restrict__ gt, int rows, int per_pair,
                                                      double rte_max, double rre_max, double* __restrict__ rte_out,
                                                      double* __restrict__ rre_deg_out, int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const float* T = T_est + (size_t)i * 12;
    const float* G = gt + (size_t)(i / per_pair) * 12;
    const double d0 = __dsub_rn((double)T[3], (double)G[3]), d1 = __dsub_rn((double)T[7], (double)G[7]),
                 d2 = __dsub_rn((double)T[11], (double)G[11]);
    const double rte = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2)));
    // trace(R_est^T R_gt) = sum_{k,i} T[k,i] G[k,i]: the nine products in row-major order, summed left to right
    double tr = __dmul_rn((double)T[0], (double)G[0]);
#pragma unroll
    for (int e = 1; e < 9; ++e) {
        const int k = (e / 3) * 4 + e % 3;
        tr = __dadd_rn(tr, __dmul_rn((double)T[k], (double)G[k]));
    }
    const double c = __ddiv_rn(__dsub_rn(tr, 1.0), 2.0);
    const double rre = acos(c);                                       // NaN outside [-1, 1]: kept, a failure (tester.py:330,335)
    const double rre_deg = __ddiv_rn(__dmul_rn(rre, 180.0), PE_PI);
    const int ok_t = rte < rte_max ? 1 : 0, ok_r = (rre == rre && rre < rre_max) ? 1 : 0;
    rte_out[i] = rte;
    rre_deg_out[i] = rre_deg;
    flags[i] = ok_t | (ok_r << 1) | ((ok_t & ok_r) << 2);
}

__global__ void __launch_bounds__(256) pe_meters_kernel(const double* __restrict__ rte, const double* __restrict__ rre_deg,
                                                        const int* __restrict__ flags, int P, int per_pair, double* __restrict__ meters) {
    __shared__ double red[256];
    for (int c = 0; c < per_pair; ++c) {
        double ts = 0.0, tq = 0.0, tn = 0.0, rs = 0.0, rq = 0.0, rn = 0.0, ok = 0.0;
        for (int p = threadIdx.x; p < P; p += 256) {
            const size_t i = (size_t)p * per_pair + c;
            const int f = flags[i];
            if (f & 1) { const double v = rte[i]; ts = __dadd_rn(ts, v); tq = __dadd_rn(tq, __dmul_rn(v, v)); tn += 1.0; }
            if (f & 2) { const double v = rre_deg[i]; rs = __dadd_rn(rs, v); rq = __dadd_rn(rq, __dmul_rn(v, v)); rn += 1.0; }
            if (f & 4) ok += 1.0;
        }
        ts = d3f_block_sum(ts, red); tq = d3f_block_sum(tq, red); tn = d3f_block_sum(tn, red);   // (counts: whole numbers below 2^53, exact)
        rs = d3f_block_sum(rs, red); rq = d3f_block_sum(rq, red); rn = d3f_block_sum(rn, red);
        ok = d3f_block_sum(ok, red);
        if (threadIdx.x == 0) {
            double* m = meters + (size_t)c * 8;
            m[0] = ts; m[1] = tq; m[2] = tn; m[3] = rs; m[4] = rq; m[5] = rn; m[6] = ok; m[7] = (double)P;
        }
    }
}

extern "C" int d3f_pose_errors(const float* T_est, const float* gt, int P, int per_pair, const double* thresholds_host, double* rte_dev,
                               double* rre_deg_dev, int* flags_dev, double* meters_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || per_pair < 1 || (long long)P * per_pair > 0x7fffffffll) return D3F_ERR_ARG;
    if (!T_est || !gt || !thresholds_host || !rte_dev || !rre_deg_dev || !flags_dev) return D3F_ERR_ARG;
    const double rte_max = thresholds_host[0], rre_max = thresholds_host[1];
    if (!(rte_max > 0.0) || !(rre_max > 0.0)) return D3F_ERR_ARG;    // NaN too
    const int rows = P * per_pair;
    if (rows > 0)
        pe_rows_kernel<<<d3f_cdiv(rows, 256), 256, 0, stream>>>(T_est, gt, rows, per_pair, rte_max, rre_max, rte_dev, rre_deg_dev, flags_dev);
    else if (!meters_dev)
        return D3F_OK;
    if (meters_dev) pe_meters_kernel<<<1, 256, 0, stream>>>(rte_dev, rre_deg_dev, flags_dev, P, per_pair, meters_dev);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
