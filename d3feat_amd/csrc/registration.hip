// Downstream matching on gfx950: what the reference does with the descriptors after the hot path.
//
//   * feature nearest neighbours / mutual matches   geometric_registration/evaluate.py:11-27 (build_correspondence:
//       argmin over a [n x m] distance matrix of 32-d descriptors, both directions, keep the mutually closest pairs);
//   * RANSAC on feature matches                      evaluate.py:93-99, demo_registration.py:184-192
//       (open3d.registration_ransac_based_on_feature_matching: sample ransac_n source points, pair each with its nearest
//       target FEATURE, edge-length checker, rigid fit (no scaling), distance checker, score the fit by the nearest target
//       POINT of every transformed source point within max_correspondence_distance; best fitness, then lowest rmse).
//
// Open3D 0.7 is third-party code outside /root/reference with unspecified random sampling, so results are pinned to this
// repo's numpy restatement of the SAME algorithm with the SAME counter-based random numbers (oracle/registration_np.py),
// not to Open3D's stream: hypotheses are a pure function of (seed, iteration).
//
// Kernels: distance tiles on the VALU (C = 32: 64 flops per pair, B tile broadcast from LDS, row minima merged across column
// splits with one 64-bit atomicMin per row -- key = d2 bits << 32 | column, ties to the lowest column); one thread per RANSAC
// hypothesis (Horn's closed-form absolute orientation: largest eigenvector of a 4x4 symmetric matrix by cyclic Jacobi, fp64);
// scoring of the validated hypotheses against the neighbour grid of radius_neighbors.hip (d3f_neighbor_grid_score).
#include "prims.h"
#include "rc_shared.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------------------------------
// nearest feature: key[i] = min_j (||A_i - B_j||^2 bits << 32 | j)
// ---------------------------------------------------------------------------------------------------------------------
#define RG_TB 128   // B rows per LDS tile

// f(std::integral_constant<int, C>()) for the descriptor width C of a call that has checked it: 16, 32 or 64
template <class F>
static inline void rg_dispatch_C(int C, F&& f) {
    if (C == 16) f(std::integral_constant<int, 16>());
    else if (C == 32) f(std::integral_constant<int, 32>());
    else f(std::integral_constant<int, 64>());
}

// ||a - b||^2 of two descriptors of C floats: the fmaf chain over c ascending that every descriptor distance of this file is, bit for bit
template <int C>
__device__ __forceinline__ float rg_desc_d2(const float* a, const float* b) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float d = a[c] - b[c];
        d2 = fmaf(d, d, d2);
    }
    return d2;
}

// The rows [j0, j1) of B through the LDS tile, RG_TB at a time, the whole workgroup; a: this thread's descriptor.  best / bj come in
// with the caller's start values and leave as the smallest d2 and its row.  (Both passes of rp_nn_pass; rg_feature_nn_kernel holds the
// same loop written out, for its speed.)
template <int C>
__device__ __forceinline__ void rg_tile_scan(const float* a, const float* __restrict__ B, int j0, int j1, int ldb, float* tile,
                                             float& best, int& bj) {
    for (int t0 = j0; t0 < j1; t0 += RG_TB) {
        const int nt = min(RG_TB, j1 - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < nt * C; e += 256) tile[e] = B[(size_t)(t0 + e / C) * ldb + (e % C)];
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const float d2 = rg_desc_d2<C>(a, tile + j * C);
            if (d2 < best) { best = d2; bj = t0 + j; }   // strict: ties keep the lowest column
        }
    }
}

template <int C>
__global__ void __launch_bounds__(256) rg_feature_nn_kernel(const float* __restrict__ A, int Na, int lda,
                                                            const float* __restrict__ B, int Nb, int ldb,
                                                            unsigned long long* __restrict__ key) {
    __shared__ float tile[RG_TB * C];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = (i < Na) ? A[(size_t)i * lda + c] : 0.f;
    const int per = (Nb + gridDim.y - 1) / gridDim.y;
    const int j0 = blockIdx.y * per, j1 = min(Nb, j0 + per);
    float best = 3.402823466e38f;
    int bj = 0x7fffffff;
    // rg_tile_scan's loop, written out: through the helper this kernel compiles to other code and d3f_feature_nn measures 2 % (C = 64)
    // to 35 % (C = 16, 1000 rows) slower on an MI355X (profiles/pair_plumbing_feature_nn.json)
    for (int t0 = j0; t0 < j1; t0 += RG_TB) {
        const int nt = min(RG_TB, j1 - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < nt * C; e += 256) tile[e] = B[(size_t)(t0 + e / C) * ldb + (e % C)];
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const float d2 = rg_desc_d2<C>(a, tile + j * C);
            if (d2 < best) { best = d2; bj = t0 + j; }   // strict: ties keep the lowest column
        }
    }
    if (i < Na && bj != 0x7fffffff)
        atomicMin(&key[i], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bj);
}

__global__ void __launch_bounds__(256) rg_unpack_kernel(const unsigned long long* __restrict__ key, int N, int* __restrict__ idx,
                                                        float* __restrict__ d2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long k = key[i];
    idx[i] = (k == ~0ull) ? -1 : (int)(k & 0xffffffffull);
    if (d2) d2[i] = (k == ~0ull) ? 3.402823466e38f : __uint_as_float((unsigned)(k >> 32));
}

extern "C" size_t d3f_feature_nn_workspace_bytes(int Na) { return d3f_align((size_t)(Na > 0 ? Na : 1) * 8) + 256; }

// idx[i] = argmin_j ||A_i - B_j||^2 (lowest j on ties), d2_out[i] (optional) the minimum.  C in {16, 32, 64}.  A row without a
// distance below FLT_MAX (Nb == 0, a NaN row, every d2 overflowing) posts no key: idx -1, d2 FLT_MAX; a NaN column is never chosen.
extern "C" int d3f_feature_nn(const float* A, int Na, int lda, const float* B, int Nb, int ldb, int C, int* idx, float* d2_out,
                              void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (Na < 0 || Nb < 0 || lda < C || ldb < C || (C != 16 && C != 32 && C != 64)) return D3F_ERR_ARG;
    if (Na == 0) return D3F_OK;
    if (!A || !idx || (Nb > 0 && !B)) return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < (size_t)Na * 8) return D3F_ERR_WORKSPACE;
    unsigned long long* key = (unsigned long long*)workspace;
    int rc = d3f_fill_u32(key, (size_t)Na * 2, 0xFFFFFFFFu, stream);
    if (rc != D3F_OK) return rc;
    if (Nb > 0) {
        const int bx = d3f_cdiv(Na, 256);
        int by = d3f_cdiv(1024, bx);                       // ~1024 workgroups: four per CU
        const int by_max = d3f_cdiv(Nb, RG_TB);
        if (by > by_max) by = by_max;
        if (by < 1) by = 1;
        dim3 grid(bx, by);
        rg_dispatch_C(C, [&](auto c) { rg_feature_nn_kernel<decltype(c)::value><<<grid, 256, 0, stream>>>(A, Na, lda, B, Nb, ldb, key); });
    }
    rg_unpack_kernel<<<d3f_cdiv(Na, 256), 256, 0, stream>>>(key, Na, idx, d2_out);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// mutual matches (evaluate.py:21-26): pairs (i, ab[i]) with ba[ab[i]] == i, in ascending i
// ---------------------------------------------------------------------------------------------------------------------
struct RgMutualIn {
    const int* ab; const int* ba; int Nb;
    __device__ __forceinline__ int operator()(int i) const {
        const int j = ab[i];
        return (j >= 0 && j < Nb && ba[j] == i) ? 1 : 0;
    }
};
struct RgCountEpi {
    int* count;
    __device__ __forceinline__ void operator()(int total) const { if (threadIdx.x == 0) *count = total; }
};
__global__ void __launch_bounds__(256) rg_mutual_write_kernel(RgMutualIn in, int Na, const int* __restrict__ local,
                                                              const int* __restrict__ base, int* __restrict__ pairs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Na || !in(i)) return;
    const int p = d3f_scan_at(local, base, i);
    pairs[2 * p] = i;
    pairs[2 * p + 1] = in.ab[i];
}

extern "C" size_t d3f_mutual_matches_workspace_bytes(int Na) {
    return d3f_align((size_t)(Na > 0 ? Na : 1) * 4) + d3f_align(d3f_scan_base_ints(Na) * 4) + 512;
}

// pairs i32[<= Na, 2], count_dev i32[1] (device).  ab i32[Na] (A -> B nearest), ba i32[Nb] (B -> A nearest; may be NULL when Nb == 0).
extern "C" int d3f_mutual_matches(const int* ab, int Na, const int* ba, int Nb, int* pairs, int* count_dev, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (Na < 0 || Nb < 0 || !count_dev) return D3F_ERR_ARG;
    if (Na == 0) return d3f_fill_u32(count_dev, 1, 0u, stream);
    if (!ab || (Nb > 0 && !ba) || !pairs) return D3F_ERR_ARG;   // Nb == 0: ba is never read (RgMutualIn tests j < Nb first)
    D3fArena ar(workspace, workspace_bytes);
    int* local = ar.take<int>(Na);
    int* base = ar.take<int>(d3f_scan_base_ints(Na));
    unsigned* counter = ar.take<unsigned>(4);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    int rc = d3f_fill_u32(counter, 4, 0u, stream);
    if (rc != D3F_OK) return rc;
    RgMutualIn in{ab, ba, Nb};
    if ((rc = d3f_scan_fold_launch(in, Na, nullptr, local, base, counter, RgCountEpi{count_dev}, stream)) != D3F_OK) return rc;
    rg_mutual_write_kernel<<<d3f_cdiv(Na, 256), 256, 0, stream>>>(in, Na, local, base, pairs);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// RANSAC hypotheses: one thread per iteration
// ---------------------------------------------------------------------------------------------------------------------
// rg_splitmix: rc_shared.h -- shared with the training-pair draws of radius_neighbors.hip (nb_training_pairs.h)
// draw d of iteration it: uniform integer in [0, n)  (counter based: a pure function of (seed, it, d))
__host__ __device__ __forceinline__ int rg_draw(unsigned long long seed, unsigned long long it, int d, int n) {
    const unsigned long long r = rg_splitmix(seed ^ rg_splitmix(it * 64ull + (unsigned long long)d));
    return (int)((r >> 11) % (unsigned long long)n);
}

// rg_horn (Horn 1987, fp64 Jacobi): rc_shared.h -- shared with the ICP finish kernel of radius_neighbors.hip (nb_icp.h)

#define RG_MAXN 8

// Hypothesis of iteration `it`, in two steps that every caller runs in this order.  A pure function of (seed, it) and the data:
// every caller gets the same bits.  src / tgt: xyz rows of lds / ldt floats.
struct RgSample { double s[RG_MAXN][3], t[RG_MAXN][3]; };
// the sample: true iff the draws are distinct, every drawn point has a match and the edge-length checker (if edge_sim > 0) passes
__device__ __forceinline__ bool rg_sample(const float* __restrict__ src, int lds, int Ns, const float* __restrict__ tgt, int ldt, int Nt,
                                          const int* __restrict__ nn, int n, float edge_sim, unsigned long long seed,
                                          unsigned long long it, RgSample& q) {
    int si[RG_MAXN], ti[RG_MAXN];
    bool ok = true;
    for (int d = 0; d < n; ++d) {
        si[d] = rg_draw(seed, it, d, Ns);
        ti[d] = nn[si[d]];
        if (ti[d] < 0 || ti[d] >= Nt) ok = false;
        for (int e = 0; e < d; ++e) if (si[e] == si[d]) ok = false;
    }
    double (&s)[RG_MAXN][3] = q.s, (&t)[RG_MAXN][3] = q.t;
    if (ok) {
        for (int d = 0; d < n; ++d)
            for (int c = 0; c < 3; ++c) { s[d][c] = (double)src[(size_t)lds * si[d] + c]; t[d][c] = (double)tgt[(size_t)ldt * ti[d] + c]; }
        if (edge_sim > 0.f) {   // CorrespondenceCheckerBasedOnEdgeLength: every pair of edges similar in length both ways
            for (int a = 0; a < n && ok; ++a)
                for (int b = a + 1; b < n; ++b) {
                    double ds = 0, dt = 0;
                    for (int c = 0; c < 3; ++c) { ds += (s[a][c] - s[b][c]) * (s[a][c] - s[b][c]); dt += (t[a][c] - t[b][c]) * (t[a][c] - t[b][c]); }
                    ds = sqrt(ds); dt = sqrt(dt);
                    if (ds < dt * (double)edge_sim || dt < ds * (double)edge_sim) { ok = false; break; }
                }
        }
    }
    return ok;
}
// the rigid fit of a sample that passed: out = 12 floats (row-major 3x4 [R | t]); true iff the distance checker (if dist_thr > 0) passes
__device__ __forceinline__ bool rg_fit(const RgSample& q, int n, float dist_thr, float out[12]) {
    const double (&s)[RG_MAXN][3] = q.s, (&t)[RG_MAXN][3] = q.t;
    bool ok = true;
    double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
    for (int d = 0; d < n; ++d) for (int c = 0; c < 3; ++c) { ms[c] += s[d][c]; mt[c] += t[d][c]; }
    for (int c = 0; c < 3; ++c) { ms[c] /= n; mt[c] /= n; }
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int d = 0; d < n; ++d)
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) S[a][b] += (s[d][a] - ms[a]) * (t[d][b] - mt[b]);
    double R[3][3];
    rg_horn(S, R);
    double tr[3];
    for (int a = 0; a < 3; ++a) tr[a] = mt[a] - (R[a][0] * ms[0] + R[a][1] * ms[1] + R[a][2] * ms[2]);
    if (dist_thr > 0.f) {   // CorrespondenceCheckerBasedOnDistance on the aligned samples
        for (int d = 0; d < n; ++d) {
            double e2 = 0;
            for (int a = 0; a < 3; ++a) {
                const double v = R[a][0] * s[d][0] + R[a][1] * s[d][1] + R[a][2] * s[d][2] + tr[a] - t[d][a];
                e2 += v * v;
            }
            if (sqrt(e2) > (double)dist_thr) ok = false;
        }
    }
    for (int a = 0; a < 3; ++a) { out[4 * a] = (float)R[a][0]; out[4 * a + 1] = (float)R[a][1]; out[4 * a + 2] = (float)R[a][2]; out[4 * a + 3] = (float)tr[a]; }
    return ok;
}
// both steps: out is the identity when the sample fails, else the fit (whether or not the distance checker passes)
__device__ __forceinline__ bool rg_hypothesis(const float* __restrict__ src, int lds, int Ns, const float* __restrict__ tgt, int ldt,
                                              int Nt, const int* __restrict__ nn, int n, float edge_sim, float dist_thr,
                                              unsigned long long seed, unsigned long long it, float out[12]) {
    out[0] = 1; out[1] = 0; out[2] = 0; out[3] = 0; out[4] = 0; out[5] = 1; out[6] = 0; out[7] = 0; out[8] = 0; out[9] = 0; out[10] = 1; out[11] = 0;
    RgSample q;
    return rg_sample(src, lds, Ns, tgt, ldt, Nt, nn, n, edge_sim, seed, it, q) && rg_fit(q, n, dist_thr, out);
}

// T[h], valid[h]: rg_hypothesis of iteration it0 + h, one thread each.
__global__ void __launch_bounds__(256) rg_hypotheses_kernel(const float* __restrict__ src, int Ns, const float* __restrict__ tgt,
                                                            int Nt, const int* __restrict__ nn, int n,
                                                            float edge_sim, float dist_thr, unsigned long long seed,
                                                            unsigned long long it0, int H, float* __restrict__ T,
                                                            unsigned char* __restrict__ valid) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    float out[12];
    const bool ok = rg_hypothesis(src, 3, Ns, tgt, 3, Nt, nn, n, edge_sim, dist_thr, seed, it0 + (unsigned long long)h, out);
    for (int k = 0; k < 12; ++k) T[(size_t)h * 12 + k] = out[k];
    valid[h] = ok ? 1 : 0;
}

// H hypotheses for iterations it0 .. it0 + H - 1.  nn i32[Ns]: nearest target FEATURE of every source point.
extern "C" int d3f_ransac_hypotheses(const float* src, int Ns, const float* tgt, int Nt, const int* nn, int ransac_n,
                                     float edge_similarity, float checker_distance, uint64_t seed, uint64_t it0, int H,
                                     float* T_out, unsigned char* valid_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (Ns < 1 || Nt < 1 || ransac_n < 3 || ransac_n > RG_MAXN || H < 0) return D3F_ERR_ARG;
    if (H == 0) return D3F_OK;
    if (!src || !tgt || !nn || !T_out || !valid_out) return D3F_ERR_ARG;
    rg_hypotheses_kernel<<<d3f_cdiv(H, 256), 256, 0, stream>>>(src, Ns, tgt, Nt, nn, ransac_n, edge_similarity, checker_distance,
                                                               seed, it0, H, T_out, valid_out);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// host copy of the sampler (bindings / tests draw the very same indices)
extern "C" int d3f_ransac_draw(uint64_t seed, uint64_t iteration, int d, int n) {
    return n > 0 ? rg_draw(seed, iteration, d, n) : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched registration: every pair of a scene in four launches (d3f_register_pairs)
// ---------------------------------------------------------------------------------------------------------------------
// What registration.register_keypoints does for ONE pair through a host loop -- mutual nearest descriptors, RANSAC on the
// nearest features, the winner's correspondences -- for P pairs of keypoint blocks, with every decision taken on the device:
//   rp_match_kernel       one workgroup per pair: both nearest-descriptor directions (the loop of rg_feature_nn_kernel with the
//                         roles swapped for the second direction: t - s is the exact negation of s - t, so both passes see the
//                         same d2 bits), mutual pairs in ascending source order, inliers of the mutual pairs under gt
//   rp_hypotheses_kernel  one workgroup per pair walks the iterations RP_CHUNK at a time: rg_sample for all of them, rg_fit (the fp64
//                         Horn fit, 100 x the cost of a sample) for the few that pass, gathered onto dense lanes; the valid ones are
//                         appended in ITERATION order (ballot + prefix over the waves) until the pair's list holds max_validation
//   rp_score_kernel       workgroup = (pair, 16 validated hypotheses): the pair's points in LDS, a brute-force scan per (hypothesis,
//                         source point) with the metric, the radius test and the tie rule of nb_score_kernel; integer totals
//   rp_select_kernel      one workgroup per pair: largest count, then smallest sumd2, then earliest iteration; one more scan
//                         for the winner's correspondences
// No workgroup waits for another, nothing depends on the order of arrival, and the number of launches does not depend on P.
#define RP_SLICE 16   // validated hypotheses per workgroup of rp_score_kernel
#define RP_CHUNK 1024 // iterations whose samples rp_hypotheses_kernel tests before it fits the ones that passed

struct RpRows { int blk, r0, n; };
// rows [count - min(count, nk), count) of block pairs[p][which] (evaluate.py:45-50: the tail in ascending score order); an index
// outside [0, n_blocks) selects no rows
__device__ __forceinline__ RpRows rp_rows(const int* __restrict__ count, const int* __restrict__ pairs, int p, int which, int n_blocks,
                                          int K, int nk) {
    RpRows r{0, 0, 0};
    const int b = pairs[2 * (size_t)p + which];
    if (b < 0 || b >= n_blocks) return r;
    const int c = min(max(count[b], 0), K);
    r.blk = b;
    r.n = min(c, nk);
    r.r0 = c - r.n;
    return r;
}

// out[i] = argmin_j ||A_i - B_j||^2 for the rows of one pair (lowest j on ties, -1 without a candidate): the chain of
// rg_feature_nn_kernel, B through the LDS tile, the whole workgroup walking A 256 rows at a time.
template <int C>
__device__ __forceinline__ void rp_nn_pass(const float* __restrict__ A, int Na, int lda, const float* __restrict__ B, int Nb, int ldb,
                                           float* tile, int* out) {
    for (int i0 = 0; i0 < Na; i0 += 256) {
        const int i = i0 + threadIdx.x;
        float a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = (i < Na) ? A[(size_t)i * lda + c] : 0.f;
        float best = 3.402823466e38f;
        int bj = -1;
        rg_tile_scan<C>(a, B, 0, Nb, ldb, tile, best, bj);
        if (i < Na) out[i] = bj;
    }
    __syncthreads();
}

// exclusive prefix of `flag` over the 256 threads of the workgroup in thread order; total = the workgroup's sum (wsum: 4 ints of LDS)
__device__ __forceinline__ int rp_block_prefix(bool flag, int* wsum, int& total) {
    const unsigned long long bal = __ballot(flag);
    const int w = threadIdx.x >> 6;
    if (d3f_lane() == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < 4; ++k) { const int c = wsum[k]; base += (k < w) ? c : 0; total += c; }
    __syncthreads();
    return base + __popcll(bal & d3f_lanemask_lt());
}

// (rc_apply, rc_d2: the transform and the metric of nb_score_kernel, rc_shared.h)
// nearest of the n points pts[3 * j ..] strictly inside r2, lowest j on ties (the scan is ascending); -1 for none.  The grid walk of
// nb_score_kernel visits a superset of the points inside the radius and keeps the same minimum.
__device__ __forceinline__ int rp_nearest(const float* pts, int n, float qx, float qy, float qz, float r2, float& bd2) {
    int bidx = -1;
    bd2 = 3.4e38f;
    for (int j = 0; j < n; ++j) {
        const float d2 = rc_d2(qx, qy, qz, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
        if (d2 < r2 && d2 < bd2) { bd2 = d2; bidx = j; }
    }
    return bidx;
}
// xyz of `n` record rows into LDS, 3 floats per point
__device__ __forceinline__ void rp_stage_xyz(const float* __restrict__ rec, int n, int ld, float* dst) {
    for (int e = threadIdx.x; e < 3 * n; e += 256) dst[e] = rec[(size_t)(e / 3) * ld + (e % 3)];
}

template <int C>
__global__ void __launch_bounds__(256) rp_match_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                       const int* __restrict__ count, const int* __restrict__ pairs, int nk, int Kmax,
                                                       const float* __restrict__ gt, float thr2, int* __restrict__ nn_st_out,
                                                       int* __restrict__ mutual_count, int* __restrict__ mutual,
                                                       int* __restrict__ gt_inliers) {
    __shared__ float tile[RG_TB * C];
    __shared__ int nn_st[D3F_PAIRS_KMAX], nn_ts[D3F_PAIRS_KMAX];
    __shared__ int wsum[4];
    __shared__ int n_gt;
    const int p = blockIdx.x;
    const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, nk), b = rp_rows(count, pairs, p, 1, n_blocks, K, nk);
    const float* S = kp + ((size_t)a.blk * K + a.r0) * ld;
    const float* T = kp + ((size_t)b.blk * K + b.r0) * ld;
    if (threadIdx.x == 0) n_gt = 0;
    rp_nn_pass<C>(S + 3, a.n, ld, T + 3, b.n, ld, tile, nn_st);
    rp_nn_pass<C>(T + 3, b.n, ld, S + 3, a.n, ld, tile, nn_ts);
    int base = 0, mine_gt = 0;
    for (int i0 = 0; i0 < a.n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int j = (i < a.n) ? nn_st[i] : -1;
        if (i < a.n) nn_st_out[(size_t)p * Kmax + i] = j;
        const bool m = j >= 0 && j < b.n && nn_ts[j] == i;
        int total;
        const int slot = base + rp_block_prefix(m, wsum, total);
        base += total;
        if (m) {
            if (mutual) { mutual[((size_t)p * Kmax + slot) * 2] = i; mutual[((size_t)p * Kmax + slot) * 2 + 1] = j; }
            if (gt) {   // gt takes the TARGET frame into the SOURCE frame (evaluate.py:70-77)
                float qx, qy, qz;
                rc_apply(gt + (size_t)p * 12, T[(size_t)j * ld], T[(size_t)j * ld + 1], T[(size_t)j * ld + 2], qx, qy, qz);
                mine_gt += rc_d2(qx, qy, qz, S[(size_t)i * ld], S[(size_t)i * ld + 1], S[(size_t)i * ld + 2]) < thr2 ? 1 : 0;
            }
        }
    }
    if (threadIdx.x == 0) mutual_count[p] = base;
    if (mutual)   // padding rows
        for (int e = 2 * base + threadIdx.x; e < 2 * Kmax; e += 256) mutual[(size_t)p * Kmax * 2 + e] = -1;
    if (gt) {
        if (mine_gt) atomicAdd(&n_gt, mine_gt);
        __syncthreads();
        if (threadIdx.x == 0) gt_inliers[p] = n_gt;
    }
}

// The walk of one pair: S / T the rows it uses (ns / nt of them, ld floats apart), nn the nearest target FEATURE of every source row in
// that numbering; Tl / il its lists of max_validation entries, nval_out / iter_out its two counts.  The whole workgroup.
__device__ __forceinline__ void rp_hypotheses_walk(const float* __restrict__ S, int ns, const float* __restrict__ T, int nt, int ld,
                                                   const int* __restrict__ nn, int n, float radius, float edge_sim, float dist_thr,
                                                   unsigned long long seed, int max_iteration, int max_validation,
                                                   float* __restrict__ Tl, int* __restrict__ il, int* __restrict__ nval_out,
                                                   int* __restrict__ iter_out, int* wsum, int* cand) {
    if (ns < n || nt < n || radius <= 0.f) {   // registration.py: nothing is tried
        if (threadIdx.x == 0) { *nval_out = 0; *iter_out = 0; }
        return;
    }
    int nval = 0;
    for (int it0 = 0; it0 < max_iteration && nval < max_validation; it0 += RP_CHUNK) {
        // the cheap step for RP_CHUNK iterations: the ones whose sample passes, in iteration order
        int ncand = 0, total;
        for (int k = 0; k < RP_CHUNK; k += 256) {
            const int it = it0 + k + threadIdx.x;
            RgSample q;
            const bool pass = it < max_iteration && rg_sample(S, ld, ns, T, ld, nt, nn, n, edge_sim, seed, (unsigned long long)it, q);
            const int slot = ncand + rp_block_prefix(pass, wsum, total);
            if (pass) cand[slot] = it;
            ncand += total;
        }
        __syncthreads();
        // the fit (fp64 Horn) on dense lanes: only for those; the place in the list comes from the iteration index, never from arrival
        for (int c0 = 0; c0 < ncand && nval < max_validation; c0 += 256) {
            const int c = c0 + threadIdx.x, it = c < ncand ? cand[c] : 0;
            float out[12];
            bool ok = false;
            if (c < ncand) {
                RgSample q;
                rg_sample(S, ld, ns, T, ld, nt, nn, n, edge_sim, seed, (unsigned long long)it, q);
                ok = rg_fit(q, n, dist_thr, out);
            }
            const int slot = nval + rp_block_prefix(ok, wsum, total);
            if (ok && slot < max_validation) {
                for (int k = 0; k < 12; ++k) Tl[(size_t)slot * 12 + k] = out[k];
                il[slot] = it;
                if (slot == max_validation - 1) *iter_out = it + 1;
            }
            nval += total;
        }
    }
    if (threadIdx.x == 0) {
        *nval_out = min(nval, max_validation);
        if (nval < max_validation) *iter_out = max_iteration;
    }
}

__global__ void __launch_bounds__(256) rp_hypotheses_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                            const int* __restrict__ count, const int* __restrict__ pairs, int nk, int Kmax,
                                                            const int* __restrict__ nn_st, int n, float radius, float edge_sim,
                                                            float dist_thr, unsigned long long seed, int max_iteration,
                                                            int max_validation, float* __restrict__ Tlist, int* __restrict__ itlist,
                                                            int* __restrict__ validations, int* __restrict__ iterations) {
    __shared__ int wsum[4];
    __shared__ int cand[RP_CHUNK];
    const int p = blockIdx.x;
    const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, nk), b = rp_rows(count, pairs, p, 1, n_blocks, K, nk);
    rp_hypotheses_walk(kp + ((size_t)a.blk * K + a.r0) * ld, a.n, kp + ((size_t)b.blk * K + b.r0) * ld, b.n, ld, nn_st + (size_t)p * Kmax, n,
                       radius, edge_sim, dist_thr, seed, max_iteration, max_validation, Tlist + (size_t)p * max_validation * 12,
                       itlist + (size_t)p * max_validation, validations + p, iterations + p, wsum, cand);
}

// grid (P, slices of RP_SLICE hypotheses).  cnt / sd2 [P, max_validation]: every (pair, hypothesis) has exactly one writer.
__global__ void __launch_bounds__(256) rp_score_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                       const int* __restrict__ count, const int* __restrict__ pairs, int nk,
                                                       const float* __restrict__ Tlist, const int* __restrict__ validations,
                                                       int max_validation, float r2, int* __restrict__ cnt,
                                                       unsigned long long* __restrict__ sd2) {
    __shared__ float spt[3 * D3F_PAIRS_KMAX], tpt[3 * D3F_PAIRS_KMAX];
    __shared__ float M[RP_SLICE * 12];
    __shared__ int c_l[RP_SLICE];
    __shared__ unsigned long long s_l[RP_SLICE];
    const int p = blockIdx.x, v0 = blockIdx.y * RP_SLICE;
    const int nv = min(validations[p] - v0, RP_SLICE);
    if (nv <= 0) return;
    const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, nk), b = rp_rows(count, pairs, p, 1, n_blocks, K, nk);
    rp_stage_xyz(kp + ((size_t)a.blk * K + a.r0) * ld, a.n, ld, spt);
    rp_stage_xyz(kp + ((size_t)b.blk * K + b.r0) * ld, b.n, ld, tpt);
    if (threadIdx.x < nv * 12) M[threadIdx.x] = Tlist[((size_t)p * max_validation + v0) * 12 + threadIdx.x];
    if (threadIdx.x < RP_SLICE) { c_l[threadIdx.x] = 0; s_l[threadIdx.x] = 0ull; }
    __syncthreads();
    for (int e = threadIdx.x; e < nv * a.n; e += 256) {
        const int v = e / a.n, i = e - v * a.n;
        float qx, qy, qz, bd2;
        rc_apply(M + 12 * v, spt[3 * i], spt[3 * i + 1], spt[3 * i + 2], qx, qy, qz);
        if (rp_nearest(tpt, b.n, qx, qy, qz, r2, bd2) >= 0) {
            atomicAdd(&c_l[v], 1);
            atomicAdd(&s_l[v], (unsigned long long)((double)bd2 * 4294967296.0));
        }
    }
    __syncthreads();
    if (threadIdx.x < nv) {
        cnt[(size_t)p * max_validation + v0 + threadIdx.x] = c_l[threadIdx.x];
        sd2[(size_t)p * max_validation + v0 + threadIdx.x] = s_l[threadIdx.x];
    }
}

// (RcBest, rc_better, rc_block_best, rc_store_none: the choice of the winner, rc_shared.h)
__global__ void __launch_bounds__(256) rp_select_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                        const int* __restrict__ count, const int* __restrict__ pairs, int nk, int Kmax,
                                                        const float* __restrict__ Tlist, const int* __restrict__ itlist,
                                                        const int* __restrict__ cnt, const unsigned long long* __restrict__ sd2,
                                                        const int* __restrict__ validations, int max_validation, float r2,
                                                        float* __restrict__ T_out, int* __restrict__ inliers,
                                                        unsigned long long* __restrict__ sumd2, int* __restrict__ best_iteration,
                                                        int* __restrict__ nearest) {
    __shared__ float tpt[3 * D3F_PAIRS_KMAX];
    __shared__ RcBest red[256];
    __shared__ float M[12];
    const int p = blockIdx.x, V = validations[p];
    RcBest me{-1, ~0ull, 0x7fffffff};
    for (int v = threadIdx.x; v < V; v += 256) {
        const RcBest c{cnt[(size_t)p * max_validation + v], sd2[(size_t)p * max_validation + v], v};
        if (rc_better(c, me)) me = c;
    }
    const RcBest w = rc_block_best(me, red);
    int* near = nearest + (size_t)p * Kmax;
    if (V <= 0) {   // nothing validated: the identity, no correspondences
        rc_store_none(T_out + (size_t)p * 12, inliers + p, sumd2 + p, best_iteration + p);
        for (int i = threadIdx.x; i < Kmax; i += 256) near[i] = -1;
        return;
    }
    const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, nk), b = rp_rows(count, pairs, p, 1, n_blocks, K, nk);
    const float* S = kp + ((size_t)a.blk * K + a.r0) * ld;
    rp_stage_xyz(kp + ((size_t)b.blk * K + b.r0) * ld, b.n, ld, tpt);
    if (threadIdx.x < 12) T_out[(size_t)p * 12 + threadIdx.x] = M[threadIdx.x] = Tlist[((size_t)p * max_validation + w.v) * 12 + threadIdx.x];
    if (threadIdx.x == 0) { inliers[p] = w.c; sumd2[p] = w.s; best_iteration[p] = itlist[(size_t)p * max_validation + w.v]; }
    __syncthreads();
    for (int i = threadIdx.x; i < Kmax; i += 256) {
        int j = -1;
        if (i < a.n) {
            float qx, qy, qz, bd2;
            rc_apply(M, S[(size_t)i * ld], S[(size_t)i * ld + 1], S[(size_t)i * ld + 2], qx, qy, qz);
            j = rp_nearest(tpt, b.n, qx, qy, qz, r2, bd2);
        }
        near[i] = j;
    }
}

static inline int rp_kmax(int K, int num_keypts) { return (num_keypts > 0 && num_keypts < K) ? num_keypts : K; }

extern "C" size_t d3f_register_pairs_workspace_bytes(int P, int K, int num_keypts, int max_validation) {
    if (P < 0 || K < 1 || max_validation < 1) return 0;
    const size_t p = (size_t)(P > 0 ? P : 1), pv = p * (size_t)max_validation;
    return d3f_align(p * (size_t)rp_kmax(K, num_keypts) * 4) + d3f_align(pv * 48) + 2 * d3f_align(pv * 4) + d3f_align(pv * 8) + 256;
}

extern "C" int d3f_register_pairs(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev, int P,
                                  int num_keypts, float max_correspondence_distance, int ransac_n, float edge_similarity,
                                  float checker_distance, int max_iteration, int max_validation, uint64_t seed, const float* gt,
                                  float distance_threshold, float* T_out, int* inliers, uint64_t* sumd2, int* validations,
                                  int* iterations, int* best_iteration, int* mutual_count, int* nearest, int* mutual, int* gt_inliers,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n_blocks < 1 || K < 1 || (C != 16 && C != 32 && C != 64) || ld < C + 4) return D3F_ERR_ARG;
    const int Kmax = rp_kmax(K, num_keypts);
    if (Kmax > D3F_PAIRS_KMAX || ransac_n < 3 || ransac_n > RG_MAXN) return D3F_ERR_ARG;
    if (max_iteration < 0 || max_iteration > (1 << 30) || max_validation < 1 || max_validation > (1 << 20)) return D3F_ERR_ARG;
    if (!(max_correspondence_distance == max_correspondence_distance) || !(distance_threshold == distance_threshold)) return D3F_ERR_ARG;
    if (P == 0) return D3F_OK;
    if (!kp || !count_dev || !pairs_dev || !T_out || !inliers || !sumd2 || !validations || !iterations || !best_iteration ||
        !mutual_count || !nearest || (gt && !gt_inliers))
        return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_register_pairs_workspace_bytes(P, K, num_keypts, max_validation)) return D3F_ERR_WORKSPACE;
    D3fArena ar(workspace, workspace_bytes);
    const size_t pv = (size_t)P * max_validation;
    int* nn_st = ar.take<int>((size_t)P * Kmax);
    float* Tlist = ar.take<float>(pv * 12);
    int* itlist = ar.take<int>(pv);
    int* cnt = ar.take<int>(pv);
    unsigned long long* sd2 = ar.take<unsigned long long>(pv);
    if (!ar.ok) return D3F_ERR_WORKSPACE;
    const float r = max_correspondence_distance, thr2 = distance_threshold * distance_threshold;
    rg_dispatch_C(C, [&](auto c) {
        rp_match_kernel<decltype(c)::value><<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, Kmax, Kmax, gt, thr2, nn_st,
                                                                   mutual_count, mutual, gt_inliers);
    });
    rp_hypotheses_kernel<<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, Kmax, Kmax, nn_st, ransac_n, r, edge_similarity,
                                                checker_distance, seed, max_iteration, max_validation, Tlist, itlist, validations, iterations);
    rp_score_kernel<<<dim3(P, d3f_cdiv(max_validation, RP_SLICE)), 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, Kmax, Tlist,
                                                                                   validations, max_validation, r * r, cnt, sd2);
    rp_select_kernel<<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, Kmax, Kmax, Tlist, itlist, cnt, sd2, validations,
                                            max_validation, r * r, T_out, inliers, (unsigned long long*)sumd2, best_iteration, nearest);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Keypoint repeatability of every pair at every keypoint count in one pass (d3f_repeatability_pairs)
// ---------------------------------------------------------------------------------------------------------------------
// repeatability/evaluate_3dmatch_our.py:30-41 and evaluate_kitti_our.py:12-23, for each count k: the last k rows of both blocks, one of
// them moved with the ground truth in float64, cdist, and the number of TARGET keypoints whose nearest source keypoint is closer than
// the threshold (distance.min(axis=0) < thr), over k.  The blocks are in ascending score order, so the sets for different k are
// nested: with rank 0 the best row, the nearest-source distance of a target at count k is the running minimum over the sources of
// rank < k, and the target is counted at k iff its own rank is < k.  One walk over the sources in rank order with a test at every
// requested count gives all counts:
//   rp_repeat_kernel      one workgroup per pair: the source xyz in LDS in DESCENDING score order as doubles (3 x D3F_PAIRS_KMAX x 8 B),
//                         thread t owns the targets of rank t, t + 256, ... (moved coordinates and the running minimum d2 in
//                         registers), the walk is an LDS broadcast read; hits per count: ballot + popcount, the four waves through LDS
//   rp_repeat_sum_kernel  one workgroup: totals[c] = sum over the pairs of repeat[p, c], int64 (order independent)
// Arithmetic: records widened f32 -> f64, q_r = ((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r], d2 = (dx dx + dy dy) + dz dz, the test
// d2 < thr * thr (the rounded product); every operation rounded on its own (no contraction), so a numpy restatement has the same bits.
struct RpRepeatParams {
    double thr2;
    RcCounts cnt;                   // k and n are read
    int moved;                      // moved 0: gt takes the target frame into the source frame (target rows moved); 1: the source rows
};

__device__ __forceinline__ void rp_move_f64(const double* __restrict__ M, double x, double y, double z, double& qx, double& qy, double& qz) {
    qx = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[0], x), __dmul_rn(M[1], y)), __dmul_rn(M[2], z)), M[3]);
    qy = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[4], x), __dmul_rn(M[5], y)), __dmul_rn(M[6], z)), M[7]);
    qz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[8], x), __dmul_rn(M[9], y)), __dmul_rn(M[10], z)), M[11]);
}

// TS: target rows per thread (the largest requested count is at most 256 * TS)
template <int TS>
__global__ void __launch_bounds__(256) rp_repeat_kernel(const float* __restrict__ kp, int n_blocks, int K, int ld,
                                                        const int* __restrict__ count, const int* __restrict__ pairs,
                                                        const double* __restrict__ gt, RpRepeatParams prm, int* __restrict__ repeat) {
    __shared__ double sx[D3F_PAIRS_KMAX], sy[D3F_PAIRS_KMAX], sz[D3F_PAIRS_KMAX];
    __shared__ double M[12];
    __shared__ int wsum[4 * D3F_REPEAT_COUNTS_MAX];
    const int p = blockIdx.x, nk = prm.cnt.k[prm.cnt.n - 1];
    const RpRows a = rp_rows(count, pairs, p, 0, n_blocks, K, nk), b = rp_rows(count, pairs, p, 1, n_blocks, K, nk);
    const float* S = kp + ((size_t)a.blk * K + a.r0) * ld;
    const float* T = kp + ((size_t)b.blk * K + b.r0) * ld;
    if (threadIdx.x < 12) M[threadIdx.x] = gt[(size_t)p * 12 + threadIdx.x];
    __syncthreads();
    // source of rank j = row a.n - 1 - j
    for (int j = threadIdx.x; j < a.n; j += 256) {
        const float* s = S + (size_t)(a.n - 1 - j) * ld;
        double x = (double)s[0], y = (double)s[1], z = (double)s[2];
        if (prm.moved) rp_move_f64(M, x, y, z, x, y, z);
        sx[j] = x; sy[j] = y; sz[j] = z;
    }
    double qx[TS], qy[TS], qz[TS], best[TS];
#pragma unroll
    for (int s = 0; s < TS; ++s) {
        const int r = threadIdx.x + 256 * s;
        qx[s] = qy[s] = qz[s] = 0.0;
        best[s] = __longlong_as_double(0x7ff0000000000000ll);   // no source yet: nothing is closer than the threshold
        if (r < b.n) {
            const float* t = T + (size_t)(b.n - 1 - r) * ld;
            qx[s] = (double)t[0]; qy[s] = (double)t[1]; qz[s] = (double)t[2];
            if (!prm.moved) rp_move_f64(M, qx[s], qy[s], qz[s], qx[s], qy[s], qz[s]);
        }
    }
    __syncthreads();
    int j = 0;
    for (int c = 0; c < prm.cnt.n; ++c) {
        const int kc = prm.cnt.k[c], je = min(kc, a.n), re = min(kc, b.n);   // a count beyond the source rows: the whole walk
        for (; j < je; ++j) {
            const double x = sx[j], y = sy[j], z = sz[j];
#pragma unroll
            for (int s = 0; s < TS; ++s) {
                const double dx = __dsub_rn(qx[s], x), dy = __dsub_rn(qy[s], y), dz = __dsub_rn(qz[s], z);
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                best[s] = d2 < best[s] ? d2 : best[s];
            }
        }
        int hits = 0;
#pragma unroll
        for (int s = 0; s < TS; ++s) hits += __popcll(__ballot((int)threadIdx.x + 256 * s < re && best[s] < prm.thr2));
        if (d3f_lane() == 0) wsum[(threadIdx.x >> 6) * D3F_REPEAT_COUNTS_MAX + c] = hits;
    }
    __syncthreads();
    if ((int)threadIdx.x < prm.cnt.n) {
        const int c = threadIdx.x;
        repeat[(size_t)p * prm.cnt.n + c] = (wsum[c] + wsum[D3F_REPEAT_COUNTS_MAX + c]) + (wsum[2 * D3F_REPEAT_COUNTS_MAX + c] + wsum[3 * D3F_REPEAT_COUNTS_MAX + c]);
    }
}

__global__ void __launch_bounds__(256) rp_repeat_sum_kernel(const int* __restrict__ repeat, int P, int n, long long* __restrict__ totals) {
    __shared__ long long red[256];
    for (int c = 0; c < n; ++c) {
        long long mine = 0;
        for (int p = threadIdx.x; p < P; p += 256) mine += repeat[(size_t)p * n + c];
        mine = d3f_block_sum(mine, red);
        if (threadIdx.x == 0) totals[c] = mine;
    }
}

extern "C" int d3f_repeatability_pairs(const float* kp, int n_blocks, int K, int ld, const int* count_dev, const int* pairs_dev, int P,
                                       const double* gt_dev, int moved, const double* threshold_host, const int* num_keypts_host,
                                       int n_counts, int* repeat_dev, int64_t* totals_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n_blocks < 1 || K < 1 || ld < 3 || (moved != 0 && moved != 1)) return D3F_ERR_ARG;
    RpRepeatParams prm;
    if (!threshold_host || !rc_counts(num_keypts_host, n_counts, D3F_PAIRS_KMAX, prm.cnt)) return D3F_ERR_ARG;
    const double thr = *threshold_host;
    if (!(thr > 0.0)) return D3F_ERR_ARG;   // NaN too
    prm.thr2 = thr * thr;
    prm.moved = moved;
    if (P == 0) return D3F_OK;
    if (!kp || !count_dev || !pairs_dev || !gt_dev || !repeat_dev) return D3F_ERR_ARG;
    const int rows = prm.cnt.k[n_counts - 1] < K ? prm.cnt.k[n_counts - 1] : K;   // most rows of a block any pair uses
    switch (d3f_cdiv(rows, 256)) {
        case 1: rp_repeat_kernel<1><<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, gt_dev, prm, repeat_dev); break;
        case 2: rp_repeat_kernel<2><<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, gt_dev, prm, repeat_dev); break;
        case 3: rp_repeat_kernel<3><<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, gt_dev, prm, repeat_dev); break;
        default: rp_repeat_kernel<4><<<P, 256, 0, stream>>>(kp, n_blocks, K, ld, count_dev, pairs_dev, gt_dev, prm, repeat_dev); break;
    }
    if (totals_dev) rp_repeat_sum_kernel<<<1, 256, 0, stream>>>(repeat_dev, P, n_counts, (long long*)totals_dev);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Feature-matching recall of every pair at every keypoint count in two launches (d3f_match_pairs)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_matching.h"

// ---------------------------------------------------------------------------------------------------------------------
// RANSAC registration of every pair at every keypoint count in one call (d3f_register_pairs_counts)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_register_counts.h"

// ---------------------------------------------------------------------------------------------------------------------
// Validation figures of every pair in three launches (d3f_validation_pairs)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_validation.h"

// ---------------------------------------------------------------------------------------------------------------------
// Gradient of desc_loss + det_loss of every pair with respect to the descriptor and score rows, five launches (d3f_loss_gradients)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_loss_grad.h"

// ---------------------------------------------------------------------------------------------------------------------
// KITTI test metric (RTE, RRE, success, the running meters) of every estimate in two launches (d3f_pose_errors)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_pose_errors.h"

// ---------------------------------------------------------------------------------------------------------------------
// ETH test: np.nan_to_num of the descriptors and the per-scene matching summary (d3f_sanitize_descriptors, d3f_matching_summary)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_scene_summary.h"

// ---------------------------------------------------------------------------------------------------------------------
// 3DMatch registration recall of every scene at every keypoint count in two launches (d3f_registration_recall)
// ---------------------------------------------------------------------------------------------------------------------
#include "rp_registration_recall.h"
