// Training pairs on the device (d3f_training_pairs; included by radius_neighbors.hip, which owns the cell grid's internals): the
// correspondences, the sample and the augmentation that the reference's generators make per pair on the host (datasets/KITTI.py:
// 35-48, 182-206, 319-337; datasets/ThreeDMatch.py:24-45, 222-229, 266-273).  The definition -- the draws, the streams, the order of
// the matches, the sampling procedure and the arithmetic of the row pass -- is in include/d3feat_amd.h; tests/training_pairs_np.py
// is the same text in numpy.
//
// The stack holds 2 P clouds, cloud 2 p the anchor and cloud 2 p + 1 the positive of pair p.  Launches on the caller's stream:
//   tp_params_kernel   one workgroup: the offsets (thread 0, lengths cut at the capacity), row0, the step of this call, the ticket of
//                      the scan, and one thread per cloud for its parameters (R, scale, shift).
//   tp_rows_kernel     one thread per row: backup, the augmented row and -- radius form -- the number of matches of an anchor row.
//                      Radius form: the rows are visited as the grid's cell-sorted records (neighbouring lanes walk the same cells).
//   scan_fold_kernel   radius form: the one-launch scan of prims.h over the counts (one item more than rows: the total is read too).
//   tp_draw_kernel     one workgroup per pair: M, the flags, n, and the sample -- radius form: keypts_num distinct match numbers by
//                      Floyd's algorithm; list form: keypts_num entries of the pair's list with replacement, written at once.
//   tp_resolve_kernel  radius form: one thread per drawn match number t: the row by bisection of the scan, then the candidate of rank
//                      t - start[row] of that row in (d2, j) order.
// The match list is never stored.  Both walks of a row's stencil are tp_walk: the count kernel and the resolve kernel cannot disagree
// about what a match is.  The rank is found by repeated selection (the smallest key above the previous one, rank + 1 walks): it keeps
// one key in registers, so there is NO cap on the candidates of a row and no fallback.  A row of the KITTI settings (radius 0.45 on a
// 0.3 grid) has a handful of matches, so the walks are few; this is reasoning, not a measurement.
// Every output word has exactly one writer; there are no atomics but the scan's ticket and no memset.
#pragma once
#include "rc_shared.h"

#define TP_WG 256

// ---- the draws (include/d3feat_amd.h) ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned long long tp_key(unsigned long long seed, unsigned long long step, int pair, int stream) {
    const unsigned long long a = rg_splitmix(seed ^ rg_splitmix(step));
    return rg_splitmix(a ^ (((unsigned long long)(unsigned)pair << 8) | (unsigned long long)(unsigned)(stream & 255)));
}
__host__ __device__ __forceinline__ unsigned long long tp_draw(unsigned long long key, unsigned long long counter) {
    return rg_splitmix(key ^ counter);
}
// uniform in [0, 1): the top 24 bits, exact in fp32
__host__ __device__ __forceinline__ float tp_u24(unsigned long long r) { return (float)(r >> 40) * 5.9604644775390625e-8f; }

extern "C" int d3f_training_draw(uint64_t seed, uint64_t step, int pair, int stream, uint64_t counter, uint64_t* out) {
    if (!out || pair < 0 || stream < 0 || stream > 255) return D3F_ERR_ARG;
    *out = tp_draw(tp_key(seed, step, pair, stream), counter);
    return D3F_OK;
}

struct TpAugment { float noise; int rotation; float scale_min, scale_max, shift_range; };

struct TpWs {
    int* off;            // i32[2 P + 1]  first row of every cloud (lengths cut at the capacity)
    int* meta;           // i32[16]       [0] items of the scan (rows + 1); [2..3] the step of this call (u64); [4..7] the scan's ticket
    int* counts;         // i32[N + 1]    matches of every row, by original row number (positives: 0)
    int* slocal;         // i32[N + 1]    the scan (d3f_scan_at with sbase)
    int* sbase;
    int* tsel;           // i32[P, keypts_num]  the drawn match numbers
    bool ok;
};
static TpWs tp_carve(void* ws, size_t bytes, int N, int P, int k) {
    TpWs w;
    D3fArena ar(ws, bytes);
    const size_t items = (size_t)(N > 0 ? N : 0) + 1;
    w.off = ar.take<int>(2 * (size_t)P + 1);
    w.meta = ar.take<int>(16);
    w.counts = ar.take<int>(items);
    w.slocal = ar.take<int>(items);
    w.sbase = ar.take<int>(d3f_scan_base_ints((int)items));
    w.tsel = ar.take<int>((size_t)P * (size_t)k);
    w.ok = ar.ok;
    return w;
}
static bool tp_sizes_ok(int N, int P, int keypts_num) {
    return N >= 0 && N < 2147483647 && P >= 1 && 2 * P <= D3F_MAX_BATCH && keypts_num >= 1 && keypts_num <= D3F_TRAINING_KEYPTS_MAX;
}
extern "C" size_t d3f_training_pairs_workspace_bytes(int N, int P, int keypts_num) {
    if (!tp_sizes_ok(N, P, keypts_num)) return 0;
    const size_t items = (size_t)N + 1;
    return d3f_align((2 * (size_t)P + 1) * sizeof(int)) + d3f_align(16 * sizeof(int)) + 2 * d3f_align(items * sizeof(int)) +
           d3f_align(d3f_scan_base_ints((int)items) * sizeof(int)) + d3f_align((size_t)P * keypts_num * sizeof(int)) + 256;
}

// ---- parameters -------------------------------------------------------------------------------------------------------------------
// c = a b, 3 x 3 row-major, every entry (a0 b0 + a1 b1) + a2 b2 in fp32, never contracted
__device__ __forceinline__ void tp_mat3(const float* a, const float* b, float* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            c[3 * i + j] = __fadd_rn(__fadd_rn(__fmul_rn(a[3 * i], b[j]), __fmul_rn(a[3 * i + 1], b[3 + j])), __fmul_rn(a[3 * i + 2], b[6 + j]));
}

__global__ void __launch_bounds__(TP_WG) tp_params_kernel(const int* __restrict__ lens, int N, int P, unsigned long long seed,
                                                         const unsigned long long* __restrict__ step_dev, int use_host_step,
                                                         unsigned long long host_step, int pair0, TpAugment A, int* __restrict__ off,
                                                         int* __restrict__ meta, int* __restrict__ row0, float* __restrict__ params) {
    const unsigned long long step = use_host_step ? host_step : *step_dev;      // (step_dev is only written by the call's last kernel)
    if (threadIdx.x == 0) {
        int s = 0;
        for (int b = 0; b < 2 * P; ++b) {
            off[b] = s;
            if ((b & 1) == 0) row0[b >> 1] = s;
            int len = lens[b];
            len = len < 0 ? 0 : (len > N - s ? N - s : len);                    // never past the capacity
            s += len;
        }
        off[2 * P] = s;
        row0[P] = s;
        meta[0] = s + 1;
        *(unsigned long long*)(meta + 2) = step;
        meta[4] = meta[5] = meta[6] = meta[7] = 0;
    }
    for (int b = threadIdx.x; b < 2 * P; b += TP_WG) {
        const int pair = pair0 + (b >> 1), side = b & 1;
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        float theta0 = 0.f, axis0 = 0.f;
        const unsigned long long krot = tp_key(seed, step, pair, D3F_TP_STREAM_ROTATION + side);
        for (int d = 0; d < A.rotation; ++d) {
            // theta = rand() * 2 * pi as the reference writes it: (u 2) pi in float64, u the top 53 bits
            const double theta = ((double)(tp_draw(krot, 2ull * d) >> 11) * 0x1p-53 * 2.0) * 3.141592653589793;
            const int axis = A.rotation == 1 ? (int)((tp_draw(krot, 2ull * d + 1ull) >> 11) % 3ull) : d;
            const float c = (float)cos(theta), s = (float)sin(theta);
            float Rd[9] = {c, -s, -s, s, c, -s, s, s, c};
            for (int t = 0; t < 3; ++t) Rd[3 * t + axis] = Rd[3 * axis + t] = 0.f;
            Rd[4 * axis] = 1.f;
            if (d == 0) {
                for (int t = 0; t < 9; ++t) R[t] = Rd[t];
                theta0 = (float)theta;
                axis0 = (float)axis;
            } else {
                float Rn[9];
                tp_mat3(R, Rd, Rn);
                for (int t = 0; t < 9; ++t) R[t] = Rn[t];
            }
        }
        float* q = params + 16 * (size_t)b;
        for (int t = 0; t < 9; ++t) q[t] = R[t];
        // one scale per PAIR, one shift per CLOUD
        const float us = tp_u24(tp_draw(tp_key(seed, step, pair, D3F_TP_STREAM_SCALE), 0ull));
        q[9] = __fadd_rn(A.scale_min, __fmul_rn(__fsub_rn(A.scale_max, A.scale_min), us));
        const unsigned long long ksh = tp_key(seed, step, pair, D3F_TP_STREAM_SHIFT + side);
        for (int c = 0; c < 3; ++c)
            q[10 + c] = __fadd_rn(-A.shift_range, __fmul_rn(__fmul_rn(2.f, A.shift_range), tp_u24(tp_draw(ksh, (unsigned long long)c))));
        q[13] = theta0;
        q[14] = axis0;
        q[15] = (float)A.rotation;
    }
}

// ---- the row pass -----------------------------------------------------------------------------------------------------------------
// the anchor in the positive's frame: ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in fp32, never contracted (T: 16 floats, row-major)
__device__ __forceinline__ void tp_move(const float* __restrict__ T, float x, float y, float z, float& qx, float& qy, float& qz) {
    qx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
    qy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
    qz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
}

// out = ((p + u noise) @ R) scale + shift for row i (inside its cloud) of cloud `side` of `pair`
__device__ __forceinline__ void tp_augment_row(const float* __restrict__ q, unsigned long long knoise, int i, float noise, float x, float y,
                                               float z, float* __restrict__ out) {
    const unsigned long long c0 = 3ull * (unsigned long long)i;
    const float a0 = __fadd_rn(x, __fmul_rn(tp_u24(tp_draw(knoise, c0)), noise));
    const float a1 = __fadd_rn(y, __fmul_rn(tp_u24(tp_draw(knoise, c0 + 1ull)), noise));
    const float a2 = __fadd_rn(z, __fmul_rn(tp_u24(tp_draw(knoise, c0 + 2ull)), noise));
    const float scale = q[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float o = __fadd_rn(__fadd_rn(__fmul_rn(a0, q[j]), __fmul_rn(a1, q[3 + j])), __fmul_rn(a2, q[6 + j]));
        out[j] = __fadd_rn(__fmul_rn(o, scale), q[10 + j]);
    }
}

// Every positive point strictly inside the radius of the moved anchor point q: f(d2, index inside the stack) for each, in the order of
// the cells.  The stencil of nb_overlap_kernel: the 27 cells around q's cell of element e, nine runs of x-adjacent cells.
template <class F>
__device__ __forceinline__ void tp_walk(const NbElem& e, const int* __restrict__ cell_start, const int* __restrict__ cell_base,
                                        const float4* __restrict__ sorted, float qx, float qy, float qz, float r2, F& f) {
    int cx, cy, cz;
    nb_cell_of(e, qx, qy, qz, cx, cy, cz);
    cx = min(max(cx, -2), e.dims[0] + 1);
    cy = min(max(cy, -2), e.dims[1] + 1);
    cz = min(max(cz, -2), e.dims[2] + 1);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, e.dims[0] - 1);
    if (x0 > x1) return;
    for (int j = 0; j < 9; ++j) {
        const int y = cy + (j % 3) - 1, z = cz + (j / 3) - 1;
        if (y < 0 || y >= e.dims[1] || z < 0 || z >= e.dims[2]) continue;
        const int rowbase = e.cbase + e.dims[0] * (y + e.dims[1] * z);
        const int lo = d3f_scan_at(cell_start, cell_base, rowbase + x0), hi = d3f_scan_at(cell_start, cell_base, rowbase + x1 + 1);
        for (int t = lo; t < hi; ++t) {
            const float4 sp = sorted[t];
            const float d2 = rc_d2(qx, qy, qz, sp.x, sp.y, sp.z);
            if (d2 < r2) f(d2, __float_as_int(sp.w));
        }
    }
}
struct TpCount {
    int n;
    __device__ __forceinline__ void operator()(float, int) { ++n; }
};
// the smallest key (d2, j) strictly above (pd2, pj); any: one was found
struct TpNext {
    float pd2; int pj; float bd2; int bj; bool any;
    __device__ __forceinline__ void operator()(float d2, int j) {
        if (!(d2 > pd2 || (d2 == pd2 && j > pj))) return;
        if (!any || d2 < bd2 || (d2 == bd2 && j < bj)) { bd2 = d2; bj = j; any = true; }
    }
};

// RADIUS: the rows are the grid's records; else rows 0 .. n - 1 of `points`
template <bool RADIUS>
__global__ void __launch_bounds__(TP_WG) tp_rows_kernel(const float* __restrict__ points, int N, int P, const int* __restrict__ off,
                                                       const int* __restrict__ meta, unsigned long long seed, int pair0, float noise,
                                                       const float* __restrict__ params, const float* __restrict__ trans,
                                                       const NbElem* __restrict__ el, const int* __restrict__ cell_start,
                                                       const int* __restrict__ cell_base, const float4* __restrict__ sorted, float r2,
                                                       float* __restrict__ out, float* __restrict__ backup, int* __restrict__ counts) {
    const int B = 2 * P, n = min(off[B], N);
    const unsigned long long step = *(const unsigned long long*)(meta + 2);
    for (long long w0 = (long long)blockIdx.x * TP_WG + threadIdx.x; w0 <= n; w0 += (long long)gridDim.x * TP_WG) {
        const int w = (int)w0;
        if (w == n) {                                              // the scan's last item
            if (RADIUS) counts[n] = 0;
            break;
        }
        const int b = d3f_find_elem(off, B, w);                    // records are element-major: record w belongs to the cloud of row w
        float x, y, z;
        int row = w;
        if (RADIUS) {
            const float4 me = sorted[w];
            x = me.x; y = me.y; z = me.z;
            row = __float_as_int(me.w);
            if (row < off[b] || row >= off[b + 1]) continue;       // (a grid that was not built over these lengths: nothing is written)
        } else {
            x = points[3 * (size_t)w]; y = points[3 * (size_t)w + 1]; z = points[3 * (size_t)w + 2];
        }
        const int p = b >> 1, side = b & 1, i = row - off[b];
        float bx = x, by = y, bz = z;
        if (RADIUS) {
            int cnt = 0;
            if (side == 0) {
                tp_move(trans + 16 * (size_t)p, x, y, z, bx, by, bz);
                TpCount f{0};
                tp_walk(el[b + 1], cell_start, cell_base, sorted, bx, by, bz, r2, f);
                cnt = f.n;
            }
            counts[row] = cnt;
        }
        backup[3 * (size_t)row] = bx; backup[3 * (size_t)row + 1] = by; backup[3 * (size_t)row + 2] = bz;
        float o[3];
        tp_augment_row(params + 16 * (size_t)b, tp_key(seed, step, pair0 + p, D3F_TP_STREAM_NOISE + side), i, noise, x, y, z, o);
        out[3 * (size_t)row] = o[0]; out[3 * (size_t)row + 1] = o[1]; out[3 * (size_t)row + 2] = o[2];
    }
}

struct TpScanIn {
    const int* counts;
    __device__ __forceinline__ int operator()(int i) const { return counts[i]; }
};

// ---- the sample -------------------------------------------------------------------------------------------------------------------
// RADIUS: keypts_num DISTINCT match numbers of [0, M) by Floyd's algorithm: for i = 0 .. k - 1, j = M - k + i: t_i = draw(i) mod (j + 1);
// entry i is t_i unless an earlier entry holds t_i, then it is j (which no earlier entry can hold).  The membership test is resolved
// without the serial loop: an earlier entry holds t_i iff an earlier draw gave t_i (whatever became of it, t_l is in the set after step
// l), or t_i is the j of an earlier step l that fell back to it -- and whether step l fell back is the same question one level down, at
// a smaller index.  The result is the serial algorithm's, integer for integer.
// else: entry i = row (draw(i) mod len) of the pair's list, the positive's index shifted by the anchor's length.
template <bool RADIUS>
__global__ void __launch_bounds__(TP_WG) tp_draw_kernel(int P, int N, const int* __restrict__ off, const int* __restrict__ meta,
                                                       const int* __restrict__ slocal, const int* __restrict__ sbase,
                                                       const int* __restrict__ kp, int L, const int* __restrict__ pair_start,
                                                       unsigned long long seed, int pair0, int k, int min_matches, int* __restrict__ tsel,
                                                       int* __restrict__ anc, int* __restrict__ pos, int ld, int* __restrict__ n_out,
                                                       int* __restrict__ matches, int* __restrict__ status,
                                                       unsigned long long* __restrict__ step_dev, int bump) {
    __shared__ int t[D3F_TRAINING_KEYPTS_MAX];
    __shared__ unsigned char dup[D3F_TRAINING_KEYPTS_MAX];
    const int p = blockIdx.x;
    const unsigned long long step = *(const unsigned long long*)(meta + 2);
    if (bump && p == 0 && threadIdx.x == 0 && step_dev) *step_dev = step + 1ull;        // (nothing reads step_dev in this call any more)
    const unsigned long long key = tp_key(seed, step, pair0 + p, D3F_TP_STREAM_SAMPLE);
    int M, start = 0, st = 0;
    if (RADIUS) {
        M = d3f_scan_at(slocal, sbase, off[2 * p + 1]) - d3f_scan_at(slocal, sbase, off[2 * p]);
        if (M < min_matches) st |= D3F_TP_FEW_MATCHES;
        if (M < k) st |= D3F_TP_BELOW_KEYPTS;
    } else {
        start = pair_start[p];
        M = pair_start[p + 1] - start;
        if (start < 0 || M < 0 || (long long)start + (long long)M > (long long)L) { st |= D3F_TP_LIST_RANGE; M = 0; }
        else if (M < 1) st |= D3F_TP_BELOW_KEYPTS;
    }
    if (threadIdx.x == 0) { matches[p] = M; status[p] = st; n_out[p] = st ? 0 : k; }
    if (st) return;                                                                      // (the same for the whole workgroup)
    if (!RADIUS) {
        const int shift = off[2 * p + 1] - off[2 * p];
        for (int i = threadIdx.x; i < k; i += TP_WG) {
            const int r = start + (int)((tp_draw(key, (unsigned long long)i) >> 11) % (unsigned long long)M);
            anc[(size_t)p * ld + i] = kp[2 * (size_t)r];
            pos[(size_t)p * ld + i] = kp[2 * (size_t)r + 1] + shift;
        }
        return;
    }
    const int j0 = M - k;
    for (int i = threadIdx.x; i < k; i += TP_WG)
        t[i] = (int)((tp_draw(key, (unsigned long long)i) >> 11) % (unsigned long long)(j0 + i + 1));
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += TP_WG) {
        const int v = t[i];
        int d = 0;
        for (int l = 0; l < i; ++l) d |= (t[l] == v) ? 1 : 0;
        dup[i] = (unsigned char)d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += TP_WG) {
        bool fell = false;
        int cur = i;
        for (;;) {
            if (dup[cur]) { fell = true; break; }
            const int l = t[cur] - j0;                       // t[cur] is the j of step l
            if (l < 0 || l >= cur) break;
            cur = l;
        }
        tsel[(size_t)p * k + i] = fell ? j0 + i : t[i];
    }
}

// one thread per drawn match number
__global__ void __launch_bounds__(TP_WG) tp_resolve_kernel(const float* __restrict__ points, int P, const int* __restrict__ off,
                                                          const int* __restrict__ meta, const int* __restrict__ slocal,
                                                          const int* __restrict__ sbase, const float* __restrict__ trans,
                                                          const NbElem* __restrict__ el, const int* __restrict__ cell_start,
                                                          const int* __restrict__ cell_base, const float4* __restrict__ sorted, float r2,
                                                          int k, const int* __restrict__ tsel, const int* __restrict__ n_dev,
                                                          int* __restrict__ anc, int* __restrict__ pos, int ld,
                                                          unsigned long long* __restrict__ step_dev) {
    const long long tid = (long long)blockIdx.x * TP_WG + threadIdx.x;
    if (tid == 0 && step_dev) *step_dev = *(const unsigned long long*)(meta + 2) + 1ull;  // (nothing reads step_dev in this call any more)
    if (tid >= (long long)P * k) return;
    const int p = (int)(tid / k), i = (int)(tid % k);
    if (i >= n_dev[p]) return;
    const int a0 = off[2 * p], a1 = off[2 * p + 1], b0 = a1;
    const int target = d3f_scan_at(slocal, sbase, a0) + tsel[(size_t)p * k + i];
    // the LAST row of [a0, a1) whose start is <= target: target is below the start of a1 (t < M), so that row's count is not zero
    int lo = a0, hi = a1 - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (d3f_scan_at(slocal, sbase, mid) <= target) lo = mid; else hi = mid - 1;
    }
    const int row = lo, rank = target - d3f_scan_at(slocal, sbase, row);
    float qx, qy, qz;
    tp_move(trans + 16 * (size_t)p, points[3 * (size_t)row], points[3 * (size_t)row + 1], points[3 * (size_t)row + 2], qx, qy, qz);
    const NbElem e = el[2 * p + 1];
    float pd2 = -1.f;                                              // below every d2
    int pj = -1;
    for (int s = 0; s <= rank; ++s) {
        TpNext f{pd2, pj, 0.f, -1, false};
        tp_walk(e, cell_start, cell_base, sorted, qx, qy, qz, r2, f);
        if (!f.any) break;                                         // (cannot happen: the count kernel saw rank + 1 matches or more)
        pd2 = f.bd2; pj = f.bj;
    }
    anc[(size_t)p * ld + i] = row - a0;
    pos[(size_t)p * ld + i] = (pj - b0) + (a1 - a0);               // inside the pair's rows: shifted by the anchor's length
}

// ---- the entry point --------------------------------------------------------------------------------------------------------------
extern "C" int d3f_training_pairs(const void* grid, size_t grid_bytes, const float* points, int N, const int* lens_dev, int P,
                                  const float* trans, const int* keypts_pairs, int L, const int* pair_start_dev, float radius,
                                  int keypts_num, int min_matches, uint64_t seed, uint64_t* step_dev, int use_host_step,
                                  uint64_t host_step, int pair0, float augment_noise, int augment_rotation, float scale_min,
                                  float scale_max, float shift_range, float* out_points, float* backup, int* anc_idx, int* pos_idx,
                                  int ld_idx, int* n_dev, int* row0_dev, int* matches_dev, int* status_dev, float* params,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const bool by_radius = grid != nullptr;
    if (!tp_sizes_ok(N, P, keypts_num) || ld_idx < keypts_num || pair0 < 0 || L < 0) return D3F_ERR_ARG;
    if (by_radius && (!(radius > 0.f) || !(radius <= 1.8e19f) || !trans)) return D3F_ERR_ARG;          // (r2 stays finite)
    if (!by_radius && (!keypts_pairs || !pair_start_dev)) return D3F_ERR_ARG;
    if (augment_rotation != 0 && augment_rotation != 1 && augment_rotation != 3) return D3F_ERR_ARG;
    if (!(augment_noise == augment_noise) || !(scale_min == scale_min) || !(scale_max == scale_max) || !(shift_range == shift_range))
        return D3F_ERR_ARG;
    if (!use_host_step && !step_dev) return D3F_ERR_ARG;
    if (!lens_dev || !anc_idx || !pos_idx || !n_dev || !row0_dev || !matches_dev || !status_dev || !params ||
        (N > 0 && (!points || !out_points || !backup)))
        return D3F_ERR_ARG;
    if (!workspace || workspace_bytes < d3f_training_pairs_workspace_bytes(N, P, keypts_num)) return D3F_ERR_WORKSPACE;
    TpWs w = tp_carve(workspace, workspace_bytes, N, P, keypts_num);
    if (!w.ok) return D3F_ERR_WORKSPACE;
    NbGrid g{};
    if (by_radius) {
        if (grid_bytes < d3f_neighbor_grid_bytes(N, 2 * P)) return D3F_ERR_WORKSPACE;
        g = nb_carve((void*)grid, grid_bytes, N, 2 * P);
        if (!g.ok) return D3F_ERR_WORKSPACE;
    }
    const TpAugment A{augment_noise, augment_rotation, scale_min, scale_max, shift_range};
    const float r2 = radius * radius;
    tp_params_kernel<<<1, TP_WG, 0, stream>>>(lens_dev, N, P, seed, (const unsigned long long*)step_dev, use_host_step, host_step, pair0, A,
                                              w.off, w.meta, row0_dev, params);
    D3F_LAUNCH_CHECK();
    int blocks = d3f_cdiv((long long)N + 1, TP_WG);
    blocks = blocks > 65535 ? 65535 : blocks;
    if (by_radius) {
        tp_rows_kernel<true><<<blocks, TP_WG, 0, stream>>>(points, N, P, w.off, w.meta, seed, pair0, A.noise, params, trans, g.el, g.cell_start,
                                                           g.stmp, g.sorted, r2, out_points, backup, w.counts);
        D3F_LAUNCH_CHECK();
        int rc;
        if ((rc = d3f_scan_fold_launch(TpScanIn{w.counts}, N + 1, w.meta, w.slocal, w.sbase, (unsigned*)(w.meta + 4), D3fNoEpi{},
                                       stream)) != D3F_OK) return rc;
        tp_draw_kernel<true><<<P, TP_WG, 0, stream>>>(P, N, w.off, w.meta, w.slocal, w.sbase, nullptr, 0, nullptr, seed, pair0, keypts_num,
                                                      min_matches, w.tsel, anc_idx, pos_idx, ld_idx, n_dev, matches_dev, status_dev,
                                                      nullptr, 0);
        D3F_LAUNCH_CHECK();
        tp_resolve_kernel<<<d3f_cdiv((long long)P * keypts_num, TP_WG), TP_WG, 0, stream>>>(
            points, P, w.off, w.meta, w.slocal, w.sbase, trans, g.el, g.cell_start, g.stmp, g.sorted, r2, keypts_num, w.tsel, n_dev, anc_idx,
            pos_idx, ld_idx, (unsigned long long*)step_dev);
        D3F_LAUNCH_CHECK();
    } else {
        tp_rows_kernel<false><<<blocks, TP_WG, 0, stream>>>(points, N, P, w.off, w.meta, seed, pair0, A.noise, params, nullptr, nullptr,
                                                            nullptr, nullptr, nullptr, 0.f, out_points, backup, nullptr);
        D3F_LAUNCH_CHECK();
        tp_draw_kernel<false><<<P, TP_WG, 0, stream>>>(P, N, w.off, w.meta, nullptr, nullptr, keypts_pairs, L, pair_start_dev, seed, pair0,
                                                       keypts_num, min_matches, nullptr, anc_idx, pos_idx, ld_idx, n_dev, matches_dev,
                                                       status_dev, (unsigned long long*)step_dev, 1);
        D3F_LAUNCH_CHECK();
    }
    return D3F_OK;
}
