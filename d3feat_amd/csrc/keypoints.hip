// Keypoint selection: the K records of a cloud with the highest detection scores, in ascending score order.
//
// What the reference's testers and consumers do on the host (utils/tester.py:208-213, demo_registration.py:159-163:
// np.argsort(scores); geometric_registration/evaluate.py:45-50, utils/tester.py:283-284, demo_registration.py:249,261: the tail of
// it) as ONE launch for all kept clouds of a stack:
//
//     sel = np.argsort(s, kind="stable")[-K:];   out = records[sel]
//
// G workgroups of 1024 lanes per kept cloud (G = 1, 2, 4, 8 or 16: topk_split), each on a slice of ceil(n / G) consecutive rows.
//   1. keys: every score becomes a monotone 32-bit key in numpy's float32 order (-0.0 == +0.0, every NaN after +inf and all NaNs
//      tied).  The keys of the slice are kept in LDS (G = 1: in the caller's workspace when the cloud does not fit beside the
//      candidate arrays): the scores are read from HBM exactly once.
//   2. exact selection inside the slice, MSB-first radix select: four 8-bit digit histograms (LDS atomics) give the key T of the
//      slice's K-th largest score, the number of keys above it and the number of rows with key == T that are still wanted.  When
//      T's run of ties is longer than that, three more digit passes over the REFERENCE row of the tie rows (row_map when the inputs
//      are in an internal order) give the row threshold: stable ascending order keeps the HIGHEST rows of a tie in the tail.
//      The min(slice, K) candidates (key > T, or key == T and row >= threshold) are collected as (key << 32 | row, input row).
//   3. G > 1: the cloud's top K are among the G slices' top K.  Every workgroup leaves its candidates in the workspace and takes
//      a ticket; the last to arrive (prims.h: d3f_last_block) gathers the <= G * K candidates into LDS and repeats the radix select
//      on the 64-bit composites, which are unique (no tie rule left).  Digits that are the same in every candidate -- the high bytes
//      of the best scores of one cloud usually are -- are found with one AND / OR reduction and cost no histogram pass.
//   4. the candidates are ordered by (key, row) -- by counting ranks when there are at most 1024, else by a bitonic network in LDS --
//      and written as full records (16-byte stores when the layout allows).
// Integer keys only: nothing here rounds, every output value is a copy of an input value.
#include "prims.h"

#define TOPK_THREADS 1024
#define TOPK_LDS_BYTES (160 * 1024 - 1280)        // dynamic LDS a workgroup of this kernel may ask for (static part: 1056 bytes)

#define TOPK_RANK_MAX 1024                         // up to here the candidates are ordered by counting ranks

static inline int topk_pad(int K) {
    int p = 2;
    while (p < K) p <<= 1;
    return p;
}
// How a call is laid out.  G workgroups per cloud: doubling while a slice still holds >= 2048 rows and >= 4 K (so the second stage
// sees at most a quarter of the cloud) and the G * K gathered candidates stay small; one workgroup without ticket counters.
struct TopkPlan {
    int G, Kpad;
    bool keys_in_lds;       // G == 1 only: the cloud's keys fit in LDS beside the candidate arrays (else: workspace)
    size_t dyn, ws_bytes;
};
static inline TopkPlan topk_plan(int N, int B, int n_cap, int K, bool tickets) {
    TopkPlan p;
    p.Kpad = topk_pad(K);
    p.G = 1;
    if (tickets)
        while (p.G < 16 && 2 * p.G * p.Kpad <= 4096 && n_cap / (2 * p.G) >= 2048 && n_cap / (2 * p.G) >= 4 * K) p.G *= 2;
    const size_t cand = (size_t)p.Kpad * 12;
    if (p.G > 1) {
        const size_t a = (size_t)d3f_cdiv(n_cap, p.G) * 4, b = (size_t)p.G * K * 12;
        p.dyn = cand + (a > b ? a : b);
        if (p.dyn > (size_t)TOPK_LDS_BYTES) p.G = 1;
    }
    if (p.G > 1) {
        p.keys_in_lds = true;
        p.ws_bytes = (size_t)B * p.G * ((size_t)K * 12 + 4);
    } else {
        p.keys_in_lds = cand + (size_t)n_cap * 4 <= (size_t)TOPK_LDS_BYTES;
        p.dyn = cand + (p.keys_in_lds ? (size_t)n_cap * 4 : 0);
        p.ws_bytes = p.keys_in_lds ? 0 : (size_t)N * 4;
    }
    return p;
}

__device__ __forceinline__ unsigned topk_key(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;        // every NaN: after +inf, all tied
    if ((u << 1) == 0u) u = 0u;                                      // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The digit that holds the `remaining`-th largest entry of hist[256] (counted from digit 255 down): sel = {digit, entries above
// it, entries in it}.  Called by the whole workgroup; wave 0 does the work (lane l owns digits 255 - 4l .. 252 - 4l).
__device__ __forceinline__ void topk_pick(const unsigned* hist, unsigned remaining, unsigned* sel) {
    __syncthreads();
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        unsigned h[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * l - j]; s += h[j]; }
        unsigned above = d3f_wave_incl_scan(s) - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (above < remaining && remaining <= above + h[j]) { sel[0] = 255 - 4 * l - j; sel[1] = above; sel[2] = h[j]; }
            above += h[j];
        }
    }
    __syncthreads();
}

// Second stage: the key of the `want`-th largest of the M distinct 64-bit composites c[0..M) (key << 32 | row).  A digit that is
// the same in every composite (one AND / OR reduction tells) takes no histogram pass.
__device__ __forceinline__ unsigned long long topk_select64(const unsigned long long* c, int M, unsigned want, unsigned* hist,
                                                            unsigned* sel, unsigned* andor) {
    const int tid = threadIdx.x;
    if (tid == 0) { andor[0] = andor[1] = 0xffffffffu; andor[2] = andor[3] = 0u; }
    __syncthreads();
    unsigned long long a = ~0ull, o = 0ull;
    for (int i = tid; i < M; i += TOPK_THREADS) { a &= c[i]; o |= c[i]; }
    unsigned alo = (unsigned)a, ahi = (unsigned)(a >> 32), olo = (unsigned)o, ohi = (unsigned)(o >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        alo &= __shfl_xor(alo, off); ahi &= __shfl_xor(ahi, off);
        olo |= __shfl_xor(olo, off); ohi |= __shfl_xor(ohi, off);
    }
    if ((tid & 63) == 0) { atomicAnd(&andor[0], alo); atomicAnd(&andor[1], ahi); atomicOr(&andor[2], olo); atomicOr(&andor[3], ohi); }
    __syncthreads();
    const unsigned long long all_and = ((unsigned long long)andor[1] << 32) | andor[0];
    const unsigned long long differ = all_and ^ (((unsigned long long)andor[3] << 32) | andor[2]);
    unsigned long long T = 0ull;
    unsigned remaining = want;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (((differ >> shift) & 0xffull) == 0ull) { T |= all_and & (0xffull << shift); continue; }
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < M; i += TOPK_THREADS) {
            const unsigned long long v = c[i];
            if (shift == 56 || (v >> (shift + 8)) == (T >> (shift + 8))) atomicAdd(&hist[(unsigned)(v >> shift) & 255u], 1u);
        }
        topk_pick(hist, remaining, sel);
        T |= (unsigned long long)sel[0] << shift;
        remaining -= sel[1];
        if (sel[2] == remaining) break;            // the whole digit is wanted: the lower digits decide nothing
    }
    return T;
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_records_kernel(
    const float* __restrict__ xyz, int ldx, const float* __restrict__ desc, int ldd, int C, const float* __restrict__ score, int lds,
    int N, const int* __restrict__ N_dev, const int* __restrict__ lens_dev, int B, int group, int keep,
    const int* __restrict__ row_map, int n_cap, int K, int Kpad, int G, float* __restrict__ out, int ldo, int* __restrict__ idx_out,
    int* __restrict__ count_dev, unsigned* __restrict__ ws_keys, unsigned long long* comp_ws, int* src_ws, int* cnt_ws,
    unsigned* tickets, int vec) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[3];
    __shared__ unsigned andor[4];
    __shared__ int sStart, sLen;
    __shared__ int sCnt[16];
    __shared__ unsigned sCand;
    const int tid = threadIdx.x;
    const int j = blockIdx.x / G, g = blockIdx.x - j * G;                          // workgroup g of kept cloud j
    const int f = j / keep, b = f * group + (j - f * keep);                        // = cloud b of the stack
    unsigned long long* comp = (unsigned long long*)smem;                          // (key << 32) | reference row
    int* srcrow = (int*)(smem + (size_t)Kpad * 8);                                 // input row of the candidate (inside the cloud)
    unsigned char* region = smem + (size_t)Kpad * 12;                              // the slice's keys, later the gathered candidates
    if (tid < 64) {
        int s = 0;
        if (b < B)
            for (int t = tid; t < b; t += 64) s += max(lens_dev[t], 0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (tid == 0) { sStart = s; sCand = 0u; sLen = b < B ? max(lens_dev[b], 0) : 0; }
    }
    if (tid < 256) hist[tid] = 0u;
    for (int s = tid; s < Kpad; s += TOPK_THREADS) { comp[s] = ~0ull; srcrow[s] = 0; }
    __syncthreads();
    const int start = sStart;
    const int n = max(min(min(sLen, n_cap), d3f_dyn(N, N_dev) - start), 0);
    const int want = min(n, K);
    if (g == 0 && tid == 0 && count_dev) count_dev[j] = want;
    if (want == 0) return;                                                         // (all G workgroups of the cloud alike)
    // ---- this workgroup's slice: rows [lo, lo + m) of the cloud, of which the top wantL are its candidates
    const int slice = (n + G - 1) / G, lo = min(g * slice, n), m = min(slice, n - lo), wantL = min(m, K);
    if (wantL > 0) {
        unsigned* keybuf = ws_keys ? ws_keys + start + lo : (unsigned*)region;
        const float* sc = score + ((size_t)start + lo) * lds;
        const int* rmap = row_map ? row_map + start + lo : nullptr;
        // keys + first digit (the one pass over the scores)
        for (int base = 0; base < m; base += 4 * TOPK_THREADS) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * TOPK_THREADS + tid;
                v[u] = i < m ? sc[(size_t)i * lds] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * TOPK_THREADS + tid;
                if (i < m) {
                    const unsigned k = topk_key(v[u]);
                    keybuf[i] = k;
                    atomicAdd(&hist[k >> 24], 1u);
                }
            }
        }
        unsigned remaining = (unsigned)wantL;
        topk_pick(hist, remaining, sel);
        unsigned T = sel[0] << 24;
        remaining -= sel[1];
        unsigned ties = sel[2];
        // (a digit that is wanted whole ends the selection: the lower digits decide nothing, T's stay zero)
        for (int shift = 16; shift >= 0 && ties != remaining; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            for (int i = tid; i < m; i += TOPK_THREADS) {
                const unsigned k = keybuf[i];
                if ((k >> (shift + 8)) == (T >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            topk_pick(hist, remaining, sel);
            T |= sel[0] << shift;
            remaining -= sel[1];
            ties = sel[2];
        }
        // `remaining` of the `ties` rows with key == T are wanted: the ones with the highest reference rows
        unsigned rowT = 0u;
        if (ties > remaining) {
            for (int shift = 16; shift >= 0; shift -= 8) {
                if (tid < 256) hist[tid] = 0u;
                __syncthreads();
                for (int i = tid; i < m; i += TOPK_THREADS) {
                    if (keybuf[i] != T) continue;
                    const unsigned r = (unsigned)(rmap ? rmap[i] - start : lo + i) & 0xffffffu;
                    if ((r >> (shift + 8)) == (rowT >> (shift + 8))) atomicAdd(&hist[(r >> shift) & 255u], 1u);
                }
                topk_pick(hist, remaining, sel);
                rowT |= sel[0] << shift;
                remaining -= sel[1];
            }
        }
        for (int i = tid; i < m; i += TOPK_THREADS) {
            const unsigned k = keybuf[i];
            if (k < T) continue;
            const unsigned r = (unsigned)(rmap ? rmap[i] - start : lo + i) & 0xffffffu;
            if (k == T && r < rowT) continue;
            const unsigned s = atomicAdd(&sCand, 1u);
            if (s < (unsigned)wantL) { comp[s] = ((unsigned long long)k << 32) | r; srcrow[s] = lo + i; }
        }
    }
    if (G > 1) {
        // ---- hand the slice's candidates over; the last workgroup of the cloud selects among all of them
        __syncthreads();
        const size_t mine = ((size_t)j * G + g) * K;
        for (int s = tid; s < wantL; s += TOPK_THREADS) { comp_ws[mine + s] = comp[s]; src_ws[mine + s] = srcrow[s]; }
        if (tid == 0) cnt_ws[j * G + g] = wantL;
        if (!d3f_last_block(&tickets[j], (unsigned)G)) return;
        if (tid == 0) { tickets[j] = 0u; sCand = 0u; }                            // the counter is left as it was found: zero
        if (tid < G) sCnt[tid] = min(max(__hip_atomic_load(&cnt_ws[j * G + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0), K);
        __syncthreads();
        unsigned long long* c2 = (unsigned long long*)region;
        int* s2 = (int*)(c2 + (size_t)G * K);
        int M = 0;
        for (int gg = 0; gg < G; ++gg) {
            const int c = sCnt[gg];
            const size_t from = ((size_t)j * G + gg) * K;
            for (int s = tid; s < c; s += TOPK_THREADS) {
                c2[M + s] = __hip_atomic_load(&comp_ws[from + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s2[M + s] = __hip_atomic_load(&src_ws[from + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            M += c;
        }
        for (int s = tid; s < Kpad; s += TOPK_THREADS) { comp[s] = ~0ull; srcrow[s] = 0; }
        __syncthreads();
        const unsigned long long Tc = topk_select64(c2, M, (unsigned)min(want, M), hist, sel, andor);
        for (int i = tid; i < M; i += TOPK_THREADS) {
            if (c2[i] < Tc) continue;
            const unsigned s = atomicAdd(&sCand, 1u);
            if (s < (unsigned)want) { comp[s] = c2[i]; srcrow[s] = s2[i]; }
        }
    }
    __syncthreads();
    // ---- ascending (key, row)
    if (want <= TOPK_RANK_MAX) {
        unsigned long long me = 0ull;
        int ms = 0, rank = 0;
        if (tid < want) {
            me = comp[tid];
            ms = srcrow[tid];
            for (int i = 0; i < want; ++i) rank += comp[i] < me ? 1 : 0;
        }
        __syncthreads();
        if (tid < want) { comp[rank] = me; srcrow[rank] = ms; }
    } else {
        // bitonic network over Kpad entries (the padding sorts to the end)
        for (int k = 2; k <= Kpad; k <<= 1) {
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
                for (int t = tid; t < (Kpad >> 1); t += TOPK_THREADS) {
                    const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), p = i | jj;
                    const unsigned long long a = comp[i], c = comp[p];
                    if ((a > c) == ((i & k) == 0)) {
                        comp[i] = c; comp[p] = a;
                        const int sa = srcrow[i]; srcrow[i] = srcrow[p]; srcrow[p] = sa;
                    }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    // ---- records
    const int W = C + 4;
    float* o = out + (size_t)j * K * ldo;
    if (vec) {
        const int Q = W >> 2;
        for (int t = tid; t < want * Q; t += TOPK_THREADS) {
            const int r = t / Q, q = t - r * Q;
            if (comp[r] == ~0ull) continue;
            const size_t mrow = (size_t)start + srcrow[r];
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 4 * q + u;
                v[u] = c < 3 ? xyz[mrow * ldx + c] : (c < 3 + C ? desc[mrow * ldd + (c - 3)] : score[mrow * lds]);
            }
            *(float4*)(o + (size_t)r * ldo + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int t = tid; t < want * W; t += TOPK_THREADS) {
            const int r = t / W, c = t - r * W;
            if (comp[r] == ~0ull) continue;
            const size_t mrow = (size_t)start + srcrow[r];
            o[(size_t)r * ldo + c] = c < 3 ? xyz[mrow * ldx + c] : (c < 3 + C ? desc[mrow * ldd + (c - 3)] : score[mrow * lds]);
        }
    }
    if (idx_out)
        for (int r = tid; r < want; r += TOPK_THREADS)
            if (comp[r] != ~0ull) idx_out[(size_t)j * K + r] = (int)(unsigned)(comp[r] & 0xffffffffull);
}

extern "C" size_t d3f_topk_workspace_bytes(int N, int B, int n_cap, int K) {
    if (N < 0 || B < 1 || B > D3F_MAX_BATCH || n_cap < 0 || n_cap >= (1 << 24) || K < 1 || K > D3F_TOPK_MAX) return 0;
    const size_t a = topk_plan(N, B, n_cap, K, true).ws_bytes, b = topk_plan(N, B, n_cap, K, false).ws_bytes;
    return d3f_align((a > b ? a : b) + 256);
}

extern "C" int d3f_topk_records(const float* xyz, int ldx, const float* desc, int ldd, int C, const float* score, int lds, int N,
                                const int* N_dev, const int* lens_dev, int B, int group, int keep, const int* row_map_dev, int n_cap,
                                int K, float* out, int ldo, int* idx_out, int* count_dev, int* tickets_dev, void* workspace,
                                size_t workspace_bytes, void* stream_) {
    if (K < 1 || K > D3F_TOPK_MAX || N < 0 || C < 1 || ldx < 3 || ldd < C || lds < 1 || ldo < C + 4 || n_cap < 0 ||
        n_cap >= (1 << 24) || B < 1 || B > D3F_MAX_BATCH || group < 1 || keep < 1 || keep > group)
        return D3F_ERR_ARG;
    if (!lens_dev || !out || (N > 0 && (!xyz || !desc || !score))) return D3F_ERR_ARG;
    const TopkPlan p = topk_plan(N, B, n_cap, K, tickets_dev != nullptr);
    if (p.ws_bytes > 0 && (!workspace || workspace_bytes < p.ws_bytes)) return D3F_ERR_WORKSPACE;
    static std::atomic<unsigned long long> opted{0};
    static const void* const fns[] = {(const void*)topk_records_kernel};
    const int rc = d3f_opt_in_lds(opted, fns, TOPK_LDS_BYTES);
    if (rc != D3F_OK) return rc;
    const int clouds = d3f_cdiv(B, group) * keep;
    const int vec = (((C + 4) & 3) == 0 && (ldo & 3) == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    unsigned long long* comp_ws = nullptr;
    int *src_ws = nullptr, *cnt_ws = nullptr;
    if (p.G > 1) {
        const size_t lists = (size_t)clouds * p.G * K;
        comp_ws = (unsigned long long*)workspace;
        src_ws = (int*)(comp_ws + lists);
        cnt_ws = src_ws + lists;
    }
    topk_records_kernel<<<clouds * p.G, TOPK_THREADS, p.dyn, (hipStream_t)stream_>>>(
        xyz, ldx, desc, ldd, C, score, lds, N, N_dev, lens_dev, B, group, keep, row_map_dev, n_cap, K, p.Kpad, p.G, out, ldo, idx_out,
        count_dev, (p.G == 1 && !p.keys_in_lds) ? (unsigned*)workspace : nullptr, comp_ws, src_ws, cnt_ws, (unsigned*)tickets_dev, vec);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
