// libstdc++ unordered_map iteration order of a cloud's voxel keys (closed form: header of grid_subsample.hip), the pieces that
// every form of the subsampling shares (included by grid_subsample.hip after D3F_CHAIN_DEV):
//   gs_mod                                bucket of a key;
//   gs_bucket_reset / gs_bucket_insert    the three words of a bucket {first position, size, chain head}: used by the LDS rounds
//                                         below and by the grid-wide rounds (gs_order_insert / _scan_tiles / _place kernels);
//   gs_order_rounds_lds                   rounds 0 .. jmax of ONE cloud by ONE workgroup, all state in LDS: instantiated by
//                                         gs_order_small_kernel (hash / sort form, 64-bit keys, rounds up to 1109 buckets, then
//                                         the grid-wide kernels go on) and by gs_small_kernel (one-workgroup form, 32-bit keys,
//                                         every round).
#pragma once
#include "prims.h"

// key % nb for key < 2^56, nb < 2^31 without the 64-bit software division: double-precision quotient estimate
// (off by at most 1 or 2) and a branch-free correction.
__device__ __forceinline__ int gs_mod(unsigned long long key, unsigned nb, double inv_nb) {
    const unsigned long long q = (unsigned long long)((double)key * inv_nb);
    long long r = (long long)(key - q * (unsigned long long)nb);
    r += (r < 0) ? (long long)nb : 0;
    r += (r < 0) ? (long long)nb : 0;
    r -= (r >= (long long)nb) ? (long long)nb : 0;
    r -= (r >= (long long)nb) ? (long long)nb : 0;
    return (int)r;
}

// bucket i of a fresh table (bf / bc / bh: first insertion position, size, chain head = last insertion, in LDS or in memory)
__device__ __forceinline__ void gs_bucket_reset(int* bf, int* bc, int* bh, int i) {
    bf[i] = 0x7fffffff;
    bc[i] = 0;
    bh[i] = -1;
}
// position t goes into bucket bk; returns the chain link of t (the position inserted into bk before it, -1: none)
__device__ __forceinline__ int gs_bucket_insert(int* bf, int* bc, int* bh, int bk, int t) {
    atomicMin(&bf[bk], t);
    atomicAdd(&bc[bk], 1);
    return atomicExch(&bh[bk], t);
}

// LDS of the rounds: every array holds the largest round's bucket count (>= its positions) words
template <class K>
struct GsOrderLds {
    K* key;             // voxel keys by voxel id
    int *bf, *bc, *bh;  // buckets
    int* nx;            // chain links, per position
    int *cd, *bk;       // CACHE only: reverse-scan value and bucket of a position
    int *L0, *L1;       // list buffers (a round reads one and writes the other; the first reads none)
    int* wsum;          // T / 64 words for the workgroup scan
};

// Round j inserts the sequence {list[0 .. lo), lo .. hi - 1} (the list of round j - 1, then the voxels created after that
// rehash) into D3F_CHAIN_DEV[j] buckets and writes the new list order to the other buffer: four phases separated by barriers,
//   reset | insert (LDS atomics) | reverse exclusive scan of c[t] = (t first of its bucket) ? bucket size : 0 | placement at
//   scan value of the bucket + number of chain members behind t.
// CACHE: the bucket of a position is kept (S.bk) and the scan values have an array of their own (S.cd); otherwise the bucket is
// recomputed from the key in every phase and the scan value replaces the bucket's size (only its first position reads it) -- 7
// arrays instead of 9, what lets gs_small_kernel hold 5087 buckets.
// The round with M <= buckets is the last: `fin(Lb, id, dest)` writes its result (voxel id at position dest).
// Returns whether that round was among 0 .. jmax; `list` = the buffer written last, lo = its positions that go on to round jmax + 1.  Called by all T threads, M > 0;
// S.key is complete (a barrier behind it) on entry.
template <int T, class K, bool CACHE, class Fin>
__device__ __forceinline__ bool gs_order_rounds_lds(const GsOrderLds<K>& S, int M, int jmax, Fin fin, int& lo, const int*& list) {
    const int tid = threadIdx.x;
    int* La = S.L0;
    int* Lb = S.L1;
    lo = 0;
    list = La;
    for (int j = 0; j <= jmax && j < D3F_NCHAIN; ++j) {
        const int nb = (int)D3F_CHAIN_DEV[j];
        const double inv_nb = 1.0 / (double)nb;
        const bool last = M <= nb;
        const int hi = last ? M : nb;
        for (int t = tid; t < nb; t += T) gs_bucket_reset(S.bf, S.bc, S.bh, t);
        __syncthreads();
        for (int t = tid; t < hi; t += T) {
            const int id = (t < lo) ? La[t] : t;
            const int bk = gs_mod((unsigned long long)S.key[id], (unsigned)nb, inv_nb);
            S.nx[t] = gs_bucket_insert(S.bf, S.bc, S.bh, bk, t);
            if constexpr (CACHE) S.bk[t] = bk;
        }
        __syncthreads();
        int carry = 0;
        for (int c0 = 0; c0 < hi; c0 += T) {
            const int u = c0 + tid, t = hi - 1 - u;
            int c = 0, bk = 0;
            if (u < hi) {
                if constexpr (CACHE) {
                    bk = S.bk[t];
                } else {
                    const int id = (t < lo) ? La[t] : t;
                    bk = gs_mod((unsigned long long)S.key[id], (unsigned)nb, inv_nb);
                }
                c = (S.bf[bk] == t) ? S.bc[bk] : 0;
            }
            int tot;
            const int e = d3f_block_excl_scan<T>(c, S.wsum, &tot);
            if constexpr (CACHE) {
                if (u < hi) S.cd[t] = carry + e;
            } else {
                if (u < hi && S.bf[bk] == t) S.bc[bk] = carry + e;
            }
            carry += tot;
        }
        __syncthreads();
        for (int t = tid; t < hi; t += T) {
            const int id = (t < lo) ? La[t] : t;
            int bk;
            if constexpr (CACHE) bk = S.bk[t];
            else bk = gs_mod((unsigned long long)S.key[id], (unsigned)nb, inv_nb);
            int r = 0;
            for (int q = S.bh[bk]; q >= 0; q = S.nx[q]) r += (q > t) ? 1 : 0;
            int dest = r;
            if constexpr (CACHE) dest += S.cd[S.bf[bk]];
            else dest += S.bc[bk];
            if (last) fin(Lb, id, dest);
            else Lb[dest] = id;
        }
        __syncthreads();
        int* const tmp = La; La = Lb; Lb = tmp;
        list = La;
        if (last) return true;
        lo = hi;
    }
    return false;
}
