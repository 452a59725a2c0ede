// Point-to-point ICP of B (source, target) pairs to convergence on the device (d3f_icp_pairs; included by radius_neighbors.hip, which
// owns the cell grid's internals).  The definition -- Open3D's registration_icp with TransformationEstimationPointToPoint(False),
// restated -- is in include/d3feat_amd.h; tests/icp_np.py is the same text in float64 numpy.
//
// Execution model: NO persistent kernel, NO cooperative grid sync, NO workgroup that waits for another.  One init launch, then per
// round two ordinary launches on the caller's stream:
//   icp_search_kernel   one thread per source row of every UNFINISHED pair, 256 consecutive rows of ONE pair per workgroup (chunk c
//                       of pair p = rows 256 c .. 256 c + 255 of that pair in original numbering).  p = T_k s in float64, the walk
//                       of nb_score_kernel over the cells the ball can touch with the float64 metric, then the workgroup's 16 sums
//                       and its count -> part[chunk], one writer each.
//   icp_finish_kernel   one workgroup per pair: the fixed tree over the pair's chunks, the figures, the stop test, the Horn fit and
//                       T_{k+1}.  It sets done[p]; both kernels return at once for a finished pair.
// Every output element and every partial has exactly one writer; there are no atomics of any kind and no memset.
//
// Kernel shape: a thread per query.  The reasons are REASONING, NOT MEASUREMENTS (no counter pass or kernel trace of this kernel has
// been taken; what is measured is the whole call, tools/icp_bench.py).  A round has (pairs x rows) independent queries -- 16 KITTI
// pairs are 1.9 M, about 3.7 times the 524 k threads the device holds resident at this kernel's 8 wavefronts per SIMD (256 CUs x 4
// SIMDs x 8 x 64) -- so occupancy, not lanes per query, should hide the dependent loads of the walk; consecutive rows of a Velodyne
// sweep are neighbours on a scan ring, so the lanes of a wavefront should walk the same few cells; and the float64 compare is 8
// operations per 16-byte candidate at half the fp32 vector rate.  Four lanes per query (nb_nearest.h) would cut the 256-row chunk
// that the summation order is defined on into 64-query workgroups and add a cross-lane (d2, index) minimum per query.
#pragma once
#include "rc_shared.h"

#define ICP_WG 256
#define ICP_NSUM 16     // sum d2 | sum p (3) | sum t (3) | sum p_a t_b (9, a outer)

struct IcpWs {
    int* soff;      // i32[B + 1]  first row of every pair's source cloud (lengths clamped to the capacity)
    int* coff;      // i32[B + 1]  first chunk of every pair
    int* done;      // i32[B]
    int* unfinished;// i32[4]      [0] pairs not done (written by icp_count_kernel only)
    double* part;   // f64[chunks, ICP_NSUM]
    int* pcount;    // i32[chunks]
    bool ok;
};
static inline size_t icp_chunks_cap(int N_src, int B) { return (size_t)d3f_cdiv(N_src > 0 ? N_src : 1, ICP_WG) + (size_t)B; }
static IcpWs icp_carve(void* ws, size_t bytes, int N_src, int B) {
    IcpWs w;
    D3fArena ar(ws, bytes);
    const size_t chunks = icp_chunks_cap(N_src, B);
    w.soff = ar.take<int>(B + 1);
    w.coff = ar.take<int>(B + 1);
    w.done = ar.take<int>(B);
    w.unfinished = ar.take<int>(4);
    w.part = ar.take<double>(chunks * ICP_NSUM);
    w.pcount = ar.take<int>(chunks);
    w.ok = ar.ok;
    return w;
}

extern "C" size_t d3f_icp_pairs_workspace_bytes(int N_src, int B) {
    if (N_src < 0 || B < 1 || B > D3F_MAX_BATCH) return 0;
    const size_t chunks = icp_chunks_cap(N_src, B);
    return 2 * d3f_align((size_t)(B + 1) * sizeof(int)) + d3f_align((size_t)B * sizeof(int)) + d3f_align(4 * sizeof(int)) +
           d3f_align(chunks * ICP_NSUM * sizeof(double)) + d3f_align(chunks * sizeof(int)) + 256;
}

// one workgroup: offsets of rows and chunks (thread 0, B <= 255), then the state of every pair
__global__ void __launch_bounds__(256) icp_init_kernel(const int* __restrict__ lens, int B, int N_src, const double* __restrict__ init,
                                                       int* __restrict__ soff, int* __restrict__ coff, int* __restrict__ done,
                                                       double* __restrict__ T, int* __restrict__ count, double* __restrict__ sumd2,
                                                       double* __restrict__ fitness, double* __restrict__ rmse,
                                                       int* __restrict__ iterations, int* __restrict__ converged) {
    if (threadIdx.x == 0) {
        int s = 0, c = 0;
        for (int b = 0; b < B; ++b) {
            soff[b] = s; coff[b] = c;
            int len = lens[b];
            len = len < 0 ? 0 : (len > N_src - s ? N_src - s : len);      // never past the capacity
            s += len;
            c += (len + ICP_WG - 1) / ICP_WG;
        }
        soff[B] = s; coff[B] = c;
    }
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        for (int e = 0; e < 12; ++e) T[(size_t)b * 12 + e] = init[(size_t)b * 12 + e];
        done[b] = 0; count[b] = 0; sumd2[b] = 0.0; fitness[b] = 0.0; rmse[b] = 0.0; iterations[b] = 0; converged[b] = 0;
    }
}

// The cells a ball of radius r around the float64 point q can touch on one axis -> [lo, hi] inside [0, dim - 1] (lo > hi: none).
// SUPERSET ARGUMENT.  A target x counts iff d2 = (dx dx + dy dy) + dz dz < r r, all rounded float64.  Rounding is monotone and the
// terms are not negative, so fl(dx dx) <= d2 < fl(r r), hence |dx| < r (1 + 2^-51), and dx = fl(q - x) gives |q - x| < r (1 + 2^-50)
// on every axis.  The grid files x under floor(b), b = fl(fl(x - mn) inv_h) (nb_cell_of: x widened exactly, two roundings), and the
// same expression gives a for q.  With A, X the exact quotients (q - mn) / h and (x - mn) / h, inv_h = fl(1 / h):
//     |a - b| <= |A - X| (1 + 2^-51) + 2^-51 (|A| + |X|) <= rho (1 + 2^-50) + 2^-50 D,     rho = r (1 + 2^-50) / h,
// where D = the largest dimension + 1 bounds |X| (every target's cell is inside the grid by construction, nb_prep) and |A| <= |X| + rho.
// So with K = ceil(r inv_h (1 + 2^-40) + D 2^-49) >= |a - b| the target's cell lies in [floor(a) - K, floor(a) + K]: two reals less
// than an integer K apart have floors at most K apart.  K is computed here from the grid's own inv_h, whatever radius the grid was
// built with.  d3f_neighbor_grid_build with radius >= r makes h >= r (1 + 2^-20) (doubled while the cells exceed the budget of
// 2^28, so D <= 2^28 + 1): r inv_h (1 + 2^-40) + D 2^-49 <= 1 - 2^-20 + 2^-39 + 2^-20.9 < 1, K = 1, the 27-cell stencil.  A coarser or a
// finer grid widens or narrows the stencil; the result is the same.  (inv_h = 0, the one-cell grid of non-finite input: a = b = 0.)
__device__ __forceinline__ void icp_axis_range(double q, double mn, double inv_h, int dim, double K, int& lo, int& hi, double& au) {
    au = (q - mn) * inv_h;                             // the query's cell coordinate, two roundings as nb_cell_of
    double a = floor(au);
    if (!(a >= -2147483648.0)) a = -2147483648.0;      // NaN too: it matches nothing anyway
    if (a > 2147483648.0) a = 2147483648.0;
    const double l = fmax(a - K, 0.0), h = fmin(a + K, (double)(dim - 1));
    const bool any = l <= h;                           // then both are inside [0, dim - 1]
    lo = any ? (int)l : 0;
    hi = any ? (int)h : -1;
}
// PRUNING.  A target filed in cell c of an axis has c <= b < c + 1, so |a - b| >= g = max(c - a, a - (c + 1), 0).  By the inequality
// of the superset argument read the other way, |A - X| >= (g - 2^-50 (D + K + 1)) / (1 + 2^-51), the true |q - x| is that times h,
// and the rounded difference, its rounded square and the rounded sums lose at most 2^-50 of it.  So with s = (D + K + 2) 2^-48 (which
// also covers the rounding of g itself) every target of a (y, z) row of cells has a computed
//     d2 >= lb2 = (max(gy - s, 0)^2 + max(gz - s, 0)^2) h^2 (1 - 2^-40),        h = 1 / inv_h.
// A row with lb2 >= r r holds no correspondence, and one with lb2 > the best d2 so far holds neither a nearer target nor a tie: both
// are skipped, and the query's own row is walked first so that the bound bites.  The result does not depend on it.
__device__ __forceinline__ double icp_axis_gap(double au, int c, double s) {
    return fmax(fmax(fmax((double)c - au, au - (double)(c + 1)), 0.0) - s, 0.0);
}

__global__ void __launch_bounds__(ICP_WG) icp_search_kernel(const NbElem* __restrict__ el, const int* __restrict__ cell_start,
                                                            const int* __restrict__ cell_base, const float4* __restrict__ sorted,
                                                            const int* __restrict__ toffs, const float* __restrict__ src,
                                                            const int* __restrict__ soff, const int* __restrict__ coff, int B,
                                                            const double* __restrict__ T, const int* __restrict__ done, double r,
                                                            double r2, double* __restrict__ part, int* __restrict__ pcount,
                                                            int* __restrict__ nearest) {
    const int chunk = blockIdx.x;
    if (chunk >= coff[B]) return;
    const int p = d3f_find_elem(coff, B, chunk);       // the last pair whose first chunk is <= chunk: pairs without rows have none
    if (done[p]) return;
    const int local = (chunk - coff[p]) * ICP_WG + (int)threadIdx.x, len = soff[p + 1] - soff[p];
    const bool row = local < len;
    double v[ICP_NSUM];
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) v[j] = 0.0;     // a row without a correspondence adds +0.0 to every sum
    int bidx = -1;
    if (row) {
        const size_t i = (size_t)soff[p] + (size_t)local;
        const double* M = T + (size_t)p * 12;
        const double sx = (double)src[3 * i], sy = (double)src[3 * i + 1], sz = (double)src[3 * i + 2];
        // ((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r], every operation rounded on its own
        const double qx = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[0], sx), __dmul_rn(M[1], sy)), __dmul_rn(M[2], sz)), M[3]);
        const double qy = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[4], sx), __dmul_rn(M[5], sy)), __dmul_rn(M[6], sz)), M[7]);
        const double qz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[8], sx), __dmul_rn(M[9], sy)), __dmul_rn(M[10], sz)), M[11]);
        const NbElem e = el[p];
        const int dmax = max(e.dims[0], max(e.dims[1], e.dims[2]));
        const double K = ceil(r * e.inv_h * (1.0 + 0x1p-40) + (double)(dmax + 1) * 0x1p-49);
        int x0, x1, y0, y1, z0, z1;
        double ax, ay, az;
        icp_axis_range(qx, e.mn[0], e.inv_h, e.dims[0], K, x0, x1, ax);
        icp_axis_range(qy, e.mn[1], e.inv_h, e.dims[1], K, y0, y1, ay);
        icp_axis_range(qz, e.mn[2], e.inv_h, e.dims[2], K, z0, z1, az);
        const double slack = ((double)(dmax + 2) + K) * 0x1p-48, h = e.inv_h > 0.0 ? 1.0 / e.inv_h : 0.0, hh = h * h * (1.0 - 0x1p-40);
        double bd2 = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
        auto walk = [&](int y, int z) {
            const double gy = icp_axis_gap(ay, y, slack), gz = icp_axis_gap(az, z, slack), lb2 = (gy * gy + gz * gz) * hh;
            if (lb2 >= r2 || (bidx >= 0 && lb2 > bd2)) return;
            // x-adjacent cells are contiguous: one run per (y, z) row; every index is inside the element's cells
            const int rowbase = e.cbase + e.dims[0] * (y + e.dims[1] * z);
            const int lo = d3f_scan_at(cell_start, cell_base, rowbase + x0), hi = d3f_scan_at(cell_start, cell_base, rowbase + x1 + 1);
            for (int t = lo; t < hi; ++t) {
                const float4 sp = sorted[t];
                const double dx = __dsub_rn(qx, (double)sp.x), dy = __dsub_rn(qy, (double)sp.y), dz = __dsub_rn(qz, (double)sp.z);
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                const int si = __float_as_int(sp.w);
                // strict radius test; ties to the lowest index, whatever order the cells and their records come in
                if (d2 < r2 && (bidx < 0 || d2 < bd2 || (d2 == bd2 && si < bidx))) {
                    bd2 = d2; bidx = si; bx = (double)sp.x; by = (double)sp.y; bz = (double)sp.z;
                }
            }
        };
        if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
            // the query's own row of cells first (when it is inside the grid), then the others
            const double fy = floor(ay), fz = floor(az);
            const bool own = fy >= (double)y0 && fy <= (double)y1 && fz >= (double)z0 && fz <= (double)z1;
            const int cy = own ? (int)fy : -1, cz = own ? (int)fz : -1;
            if (own) walk(cy, cz);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y)
                    if (!(own && y == cy && z == cz)) walk(y, z);
        }
        if (nearest) nearest[i] = bidx >= 0 ? bidx - toffs[p] : -1;       // index inside target cloud p
        if (bidx >= 0) {
            v[0] = bd2;
            v[1] = qx; v[2] = qy; v[3] = qz;
            v[4] = bx; v[5] = by; v[6] = bz;
            v[7] = __dmul_rn(qx, bx); v[8] = __dmul_rn(qx, by); v[9] = __dmul_rn(qx, bz);
            v[10] = __dmul_rn(qy, bx); v[11] = __dmul_rn(qy, by); v[12] = __dmul_rn(qy, bz);
            v[13] = __dmul_rn(qz, bx); v[14] = __dmul_rn(qz, by); v[15] = __dmul_rn(qz, bz);
        }
    }
    // THE ORDER OF THE HEADER: inside each 64 rows the halving tree s = 32 .. 1 (x[t] += x[t + s] for t < s), then (g0 + g1) + (g2 + g3)
    // over the chunk's four groups.  Lanes >= s compute values nobody reads.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double gsum[4][ICP_NSUM];
    __shared__ int gcnt[4];
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) {
        double x = v[j];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) x = __dadd_rn(x, __shfl_down(x, s, 64));
        if (lane == 0) gsum[wave][j] = x;
    }
    const int cnt = __popcll(__ballot(bidx >= 0));
    if (lane == 0) gcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x < ICP_NSUM) {
        const int j = threadIdx.x;
        part[(size_t)chunk * ICP_NSUM + j] = __dadd_rn(__dadd_rn(gsum[0][j], gsum[1][j]), __dadd_rn(gsum[2][j], gsum[3][j]));
    }
    if (threadIdx.x == 0) pcount[chunk] = (gcnt[0] + gcnt[1]) + (gcnt[2] + gcnt[3]);
}

__global__ void __launch_bounds__(256) icp_finish_kernel(const int* __restrict__ soff, const int* __restrict__ coff,
                                                         const double* __restrict__ part, const int* __restrict__ pcount,
                                                         int max_iteration, double rel_fitness, double rel_rmse, int* __restrict__ done,
                                                         double* __restrict__ T, int* __restrict__ count, double* __restrict__ sumd2,
                                                         double* __restrict__ fitness, double* __restrict__ rmse,
                                                         int* __restrict__ iterations, int* __restrict__ converged) {
    const int p = blockIdx.x;
    if (done[p]) return;
    __shared__ double red[ICP_NSUM][256];
    __shared__ int redn[256];
    const int c0 = coff[p], nc = coff[p + 1] - c0, t = threadIdx.x;
    // thread t adds the chunks c = t, t + 256, ... in ascending order from 0.0; then s = 128 .. 1: partial[t] += partial[t + s], t < s
    double acc[ICP_NSUM];
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) acc[j] = 0.0;
    int n = 0;
    for (int c = t; c < nc; c += 256) {
        const double* q = part + (size_t)(c0 + c) * ICP_NSUM;
#pragma unroll
        for (int j = 0; j < ICP_NSUM; ++j) acc[j] = __dadd_rn(acc[j], q[j]);
        n += pcount[c0 + c];
    }
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) red[j][t] = acc[j];
    redn[t] = n;
    __syncthreads();
    // (not d3f_block_sum: one tree for all ICP_NSUM + 1 sums shares its eight barriers among them)
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int j = 0; j < ICP_NSUM; ++j) red[j][t] = __dadd_rn(red[j][t], red[j][t + s]);
            redn[t] += redn[t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    n = redn[0];
    const int len = soff[p + 1] - soff[p], k = iterations[p];
    const double sd2 = red[0][0];
    const double fit = len > 0 ? __ddiv_rn((double)n, (double)len) : 0.0;
    const double rms = n > 0 ? __dsqrt_rn(__ddiv_rn(sd2, (double)n)) : 0.0;
    const double fit_prev = fitness[p], rms_prev = rmse[p];
    count[p] = n; sumd2[p] = sd2; fitness[p] = fit; rmse[p] = rms;
    if (k >= 1 && fabs(__dsub_rn(fit, fit_prev)) < rel_fitness && fabs(__dsub_rn(rms, rms_prev)) < rel_rmse) {
        converged[p] = 1; done[p] = 1;
        return;
    }
    if (k >= max_iteration) {
        converged[p] = 0; done[p] = 1;
        return;
    }
    iterations[p] = k + 1;
    if (n == 0) return;                                 // U = identity: T stays bit for bit
    // The covariance in one pass, S = sum p t^T - (sum p) mt^T.  The cancellation costs log2(1 + |mp| |mt| / (sigma_p sigma_t)) bits:
    // a KITTI sweep is centred on the sensor, its centroid a few metres from the origin and its spread tens of metres, so the
    // subtracted term is below the result and at most a bit or two of the 53 go; a cloud 1 km from the origin with 1 m of spread
    // would still keep 33.  Centring first would need the centroids before the products: a third launch per round.
    const double dn = (double)n;
    double mp[3], mt[3], S[3][3], R[3][3], tu[3];
    for (int a = 0; a < 3; ++a) { mp[a] = __ddiv_rn(red[1 + a][0], dn); mt[a] = __ddiv_rn(red[4 + a][0], dn); }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S[a][b] = __dsub_rn(red[7 + 3 * a + b][0], __dmul_rn(red[1 + a][0], mt[b]));
    rg_horn(S, R);
    for (int a = 0; a < 3; ++a) tu[a] = mt[a] - (R[a][0] * mp[0] + R[a][1] * mp[1] + R[a][2] * mp[2]);
    // T_{k+1} = U T_k: R' = R_U R_k, t' = R_U t_k + t_U, each entry ((u0 m0 + u1 m1) + u2 m2) (+ t_U)
    double* M = T + (size_t)p * 12;
    double O[12];
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 4; ++c)
            O[4 * a + c] = __dadd_rn(__dadd_rn(__dmul_rn(R[a][0], M[c]), __dmul_rn(R[a][1], M[4 + c])), __dmul_rn(R[a][2], M[8 + c]));
        O[4 * a + 3] = __dadd_rn(O[4 * a + 3], tu[a]);
    }
    for (int e = 0; e < 12; ++e) M[e] = O[e];
}

__global__ void __launch_bounds__(256) icp_count_kernel(const int* __restrict__ done, int B, int* __restrict__ unfinished) {
    __shared__ int red[256];
    int n = 0;
    for (int b = threadIdx.x; b < B; b += 256) n += done[b] ? 0 : 1;
    n = d3f_block_sum(n, red);
    if (threadIdx.x == 0) unfinished[0] = n;
}

// criteria_host: THREE doubles on the host, [max_correspondence_distance, relative_fitness, relative_rmse], read before the call returns
extern "C" int d3f_icp_pairs(const void* grid, size_t grid_bytes, int N_tgt, const float* src, int N_src, const int* src_lens_dev, int B,
                             const double* init, const double* criteria_host, int max_iteration, int check_every, double* T,
                             int* count, double* sumd2, double* fitness, double* rmse, int* iterations, int* converged, int* nearest,
                             void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N_tgt < 0 || N_src < 0 || B < 1 || B > D3F_MAX_BATCH || max_iteration < 0 || check_every < 0 || !criteria_host) return D3F_ERR_ARG;
    const double r = criteria_host[0], rel_f = criteria_host[1], rel_r = criteria_host[2];
    if (!(r > 0.0) || !(r <= 1.7e38) || rel_f != rel_f || rel_r != rel_r) return D3F_ERR_ARG;      // NaN too
    if (!grid || !src_lens_dev || !init || !T || !count || !sumd2 || !fitness || !rmse || !iterations || !converged || (N_src > 0 && !src))
        return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_icp_pairs_workspace_bytes(N_src, B)) return D3F_ERR_WORKSPACE;
    NbGrid g = nb_carve((void*)grid, grid_bytes, N_tgt, B);
    if (!g.ok) return D3F_ERR_WORKSPACE;
    IcpWs w = icp_carve(workspace, workspace_bytes, N_src, B);
    if (!w.ok) return D3F_ERR_WORKSPACE;
    icp_init_kernel<<<1, 256, 0, stream>>>(src_lens_dev, B, N_src, init, w.soff, w.coff, w.done, T, count, sumd2, fitness, rmse, iterations,
                                           converged);
    D3F_LAUNCH_CHECK();
    const unsigned chunks = (unsigned)icp_chunks_cap(N_src, B);
    const double r2 = r * r;
    for (int round = 0; round <= max_iteration; ++round) {
        icp_search_kernel<<<chunks, ICP_WG, 0, stream>>>(g.el, g.cell_start, g.stmp, g.sorted, g.soffs, src, w.soff, w.coff, B, T, w.done, r, r2,
                                                         w.part, w.pcount, nearest);
        icp_finish_kernel<<<B, 256, 0, stream>>>(w.soff, w.coff, w.part, w.pcount, max_iteration, rel_f, rel_r, w.done, T, count, sumd2,
                                                 fitness, rmse, iterations, converged);
        D3F_LAUNCH_CHECK();
        if (check_every > 0 && (round + 1) % check_every == 0 && round < max_iteration) {
            int left = 0;
            icp_count_kernel<<<1, 256, 0, stream>>>(w.done, B, w.unfinished);
            D3F_LAUNCH_CHECK();
            if (hipMemcpyAsync(&left, w.unfinished, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess) return D3F_ERR_HIP;
            if (hipStreamSynchronize(stream) != hipSuccess) return D3F_ERR_HIP;
            if (left == 0) break;
        }
    }
    return D3F_OK;
}
