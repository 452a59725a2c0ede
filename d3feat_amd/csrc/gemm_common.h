// What the contraction kernels of gemm_f32.hip / gemm_dma.h / gemm_x3.h share: the operand and epilogue descriptions, the ordered
// reduction of a K split, the fp32 tile plan, the launchers' plumbing (argument rules, slab, EPI dispatch) and the k-tile step of
// the fp32 32 x 32 tile.
#pragma once
#include "common.h"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GM_BK 32

// Optional composite A operand (decoder of models/D3Feat.py:55-63): A = [ x'[gidx[m, 0]] | A2[m] ] -- the nearest-upsample
// gather (closest_pool, models/network_blocks.py:69-83: x' = x + zero row) and the skip concatenation feed the unary
// contraction directly, so the concatenated [N, C1 + C2] tensor is never written to / re-read from HBM.
struct GemmGather {
    const int* gidx;      // NULL: A rows are used in place
    int ld_gidx;
    int N1;               // rows of A (the gather source); indices outside [0, N1) read the zero row
    const int* N1_dev;
    const float* A2;      // NULL: no second operand
    int lda2;
    int K1;               // columns taken from A (multiple of 4 when A2 != NULL)
};

struct GemmEpi {
    const float* row_scale;
    const float* col_scale;
    const float* col_shift;
    const float* residual;
    int ldr;
    int leaky;
    float alpha;
    // Optional row gather of the residual operand (gemm_x3_kernel's direct epilogue and gemm_splitk_reduce_kernel only): row m adds
    // residual[ridx[m * ld_ridx]] instead of residual[m]; an index outside [0, res_rows) -- the shadow index of an upsampling
    // matrix, a negative one -- adds exact zeros (the zero row of closest_pool).  NULL: the residual row is m, as ever.
    const int* ridx;
    int ld_ridx;
    int res_rows;             // rows of the residual tensor (upper bound) and, optionally, its device-resident value
    const int* res_rows_dev;
};

// the residual row of output row m, or NULL when it is a zero row (see GemmEpi::ridx)
__device__ __forceinline__ const float* gemm_residual_row(const GemmEpi& E, int m) {
    if (!E.ridx) return E.residual + (size_t)m * E.ldr;
    const int r = E.ridx[(size_t)m * E.ld_ridx];
    return (r >= 0 && r < d3f_dyn(E.res_rows, E.res_rows_dev)) ? E.residual + (size_t)r * E.ldr : nullptr;
}

__device__ __forceinline__ float gemm_epilogue(float v, int m, int n, const GemmEpi& E) {
    if (E.row_scale) v *= E.row_scale[m];
    if (E.col_scale) v *= E.col_scale[n];
    if (E.col_shift) v += E.col_shift[n];
    if (E.residual) v += E.residual[(size_t)m * E.ldr + n];
    if (E.leaky) v = v > 0.f ? v : v * E.alpha;
    return v;
}

// ---- the fp32 32 x 32 tile of gemm_fast_kernel and gemm_dma_kernel ---------------------------------------------------------
// One 32-deep k-tile: lane (r, h) owns k = 16 h .. 16 h + 15 of row r of both operands, as[] / bs[] point at its row and q0 .. q3
// are the float offsets of its four 16-byte chunks: four ds_read_b128 per operand, then 16 v_mfma_f32_32x32x2_f32.
// (Their transposed-accumulator epilogues are still one copy per kernel: as a shared function -- E by value or by reference,
// plain or __restrict__ pointers, with or without their one-trip loops -- the generated code of all 16 instances changes, and
// the closest form measured 1-3 % slower on the 64 x 64 tile of gemm_fast_kernel and on 4 of 26 shapes of tools/gemm_bench.py.)
__device__ __forceinline__ void gemm_tile_mfma(f32x16& acc, const float* as, const float* bs, int q0, int q1, int q2, int q3) {
    const int coff[4] = {q0, q1, q2, q3};
    float4 fa[4], fb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        fa[q] = *(const float4*)&as[coff[q]];
        fb[q] = *(const float4*)&bs[coff[q]];
    }
    __builtin_amdgcn_sched_barrier(0);        // every fragment read is issued before the first MFMA waits on one
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = e == 0 ? fa[q].x : e == 1 ? fa[q].y : e == 2 ? fa[q].z : fa[q].w;
            const float b = e == 0 ? fb[q].x : e == 1 ? fb[q].y : e == 2 ? fb[q].z : fb[q].w;
            // operands swapped: the accumulator holds the TRANSPOSED tile, i.e. a lane owns one output row and four
            // consecutive columns per register quad -> 16-byte stores in the epilogue
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b, a, acc, 0, 0, 0);
        }
    }
}

// ---- K split: slabs and their ordered reduction ---------------------------------------------------------------------------
// res_bf16 / c_bf16: the residual operand / the output hold bfloat16 values (bf16 feature storage, d3f_gemm_bf16)
__global__ void __launch_bounds__(256)
gemm_splitk_reduce_kernel(const float* __restrict__ slab, int S, int M, int N, float* __restrict__ C, int ldc, GemmEpi E,
                          const int* __restrict__ M_dev, int res_bf16 = 0, int c_bf16 = 0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)d3f_dyn(M, M_dev) * N) return;
    const int m = (int)(i / N), n = (int)(i % N);
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += slab[((size_t)s * M + m) * N + n];
    if (res_bf16 && E.residual) {
        const float r = d3f_bf16_f32(((const unsigned short*)E.residual)[(size_t)m * E.ldr + n]);
        GemmEpi E2 = E;
        E2.residual = nullptr;
        E2.leaky = 0;
        v = gemm_epilogue(v, m, n, E2) + r;
        if (E.leaky) v = v > 0.f ? v : v * E.alpha;
    } else if (E.ridx && E.residual) {
        const float* rrow = gemm_residual_row(E, m);
        GemmEpi E2 = E;
        E2.residual = nullptr;
        E2.leaky = 0;
        v = gemm_epilogue(v, m, n, E2) + (rrow ? rrow[n] : 0.f);
        if (E.leaky) v = v > 0.f ? v : v * E.alpha;
    } else {
        v = gemm_epilogue(v, m, n, E);
    }
    if (c_bf16) ((unsigned short*)C)[(size_t)m * ldc + n] = (unsigned short)d3f_bf16_rne(v);
    else C[(size_t)m * ldc + n] = v;
}

// what a *_workspace_bytes function answers for S slices
static inline size_t gemm_slab_bytes(int S, int M, int N) { return S > 1 ? d3f_align((size_t)S * M * N * sizeof(float)) + 256 : 256; }

// the slab of S slices inside the caller's workspace (NULL when S == 1); D3F_ERR_WORKSPACE when it does not fit
static inline int gemm_slab(int S, int M, int N, void* workspace, size_t workspace_bytes, float*& slab) {
    slab = nullptr;
    if (S > 1) {
        if (!workspace || workspace_bytes < (size_t)S * M * N * sizeof(float)) return D3F_ERR_WORKSPACE;
        slab = (float*)workspace;
    }
    return D3F_OK;
}

// after the tile kernel of a split contraction: C = epilogue(sum of the slabs, in slice order)
static inline void gemm_reduce(const float* slab, int S, int M, int N, float* C, int ldc, const GemmEpi& E, const int* M_dev,
                               hipStream_t stream, int res_bf16 = 0, int c_bf16 = 0) {
    if (S > 1)
        gemm_splitk_reduce_kernel<<<d3f_cdiv((long long)M * N, 256), 256, 0, stream>>>(slab, S, M, N, C, ldc, E, M_dev, res_bf16, c_bf16);
}

// ---- launcher plumbing ---------------------------------------------------------------------------------------------------
// Argument rules of the entry points that take the composite operand [ A[idx[m, 0]] | skip[m] ] and a packed weight W
// (d3f_gemm_f32t, d3f_gemm_x3, d3f_gemm_bf16).  Common: C1, C2, lda, lds multiples of 4, W 16-byte aligned.
//   f32_io   fp32 operands and output, float4-addressable (f32t, x3): N, ldc, ldr multiples of 4; A, skip, C, residual and the
//            column vectors 16-byte aligned.  Otherwise (bf16) only A / skip are tested, against a_mask
//   kmul     K = C1 + C2 and, for a concatenated operand, C1 are multiples of it (x3: 32)
// -> D3F_ERR_ARG, or D3F_OK with empty = (M == 0: nothing to launch; pointers are not looked at then)
static inline int gemm_check_composite(bool f32_io, int kmul, unsigned a_mask, int M, int N, int N1, int C1, int C2, int lda, int ldc,
                                       int lds, int ldr, int ld_idx, const void* A, const void* W, const void* C, const int* idx,
                                       const void* skip, const void* residual, const float* col_scale, const float* col_shift,
                                       bool& empty) {
    const int q = f32_io ? 4 : 1;
    empty = false;
    if (M < 0 || N < 1 || N1 < 0 || C1 < 4 || C2 < 0 || (C1 % 4) || (C2 % 4) || (N % q) || lda < C1 || (lda % 4) || ldc < N || (ldc % q) ||
        (C2 > 0 && (lds < C2 || (lds % 4))) || (residual && (ldr < N || (ldr % q))) || (idx && ld_idx < 1) || (!idx && N1 < M))
        return D3F_ERR_ARG;
    if (((C1 + C2) % kmul) || (C2 > 0 && (C1 % kmul))) return D3F_ERR_ARG;
    empty = M == 0;
    if (empty) return D3F_OK;
    if (!A || !W || !C || (C2 > 0 && !skip) || ((uintptr_t)W & 15) || (((uintptr_t)A | (uintptr_t)skip) & a_mask)) return D3F_ERR_ARG;
    if (f32_io && (((uintptr_t)C | (uintptr_t)residual | (uintptr_t)col_scale | (uintptr_t)col_shift) & 15)) return D3F_ERR_ARG;
    return D3F_OK;
}

// f(std::integral_constant<int, EPI>) for the EPI of an epilogue: bit 0 per-row scale, bit 1 residual operand
template <class F> static inline void gemm_with_epi(const GemmEpi& E, F&& f) {
    switch ((E.row_scale ? 1 : 0) | (E.residual ? 2 : 0)) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}

// ---- tile selection of the fp32 kernels (and the K slice count of the bf16 one) -------------------------------------------
// Large tiles (each wave owns 2x2 / 2x1 MFMA tiles: half the LDS traffic per flop, 4 independent
// accumulator chains) when the problem still fills the chip with them; smaller tiles / split K for the skinny deep layers.
static inline void gemm_plan(int M, int N, int K, int M_hint, int& bm, int& bn, int& S, int& tps) {
    // capacity mode: M is only an upper bound; split K for the row count the caller EXPECTS (skinny deep layers would
    // otherwise be planned as if they filled the chip and run their whole K loop in a handful of workgroups)
    if (M_hint > 0 && M_hint < M) M = M_hint;
    // Measured on MI355X over the network's 37 shapes (round 1 / 2 sweeps): these GEMMs are small (<= 7 GFLOP) and latency /
    // bandwidth bound, so the 64x64 tile -- 37 KB of LDS, 4 workgroups resident per CU -- beat the register-tiled 128x128 /
    // 128x64 variants everywhere.
    auto blocks_of = [&](int m, int n) { return (long long)d3f_cdiv(M, m) * d3f_cdiv(N, n); };
    if (N <= 32) { bm = 128; bn = 32; }
    else { bm = 64; bn = 64; }
    const long long blocks = blocks_of(bm, bn);
    const int nt = d3f_cdiv(K, GM_BK);
    // Skinny problems with a long K are latency bound per k-tile (global -> LDS -> MFMA): give every CU ~6 co-resident
    // workgroups by splitting K, as long as each split keeps >= 8 k-tiles.  Up to 16 k-tiles (K <= 512) a split never paid
    // for its slab traffic and reduce launch (tools/gemm_bench.py sweep).
    S = 1;
    if (blocks < 768 && nt > 16) {
        long long want = (1536 + blocks - 1) / blocks;
        long long maxs = nt / 8;
        S = (int)(want < maxs ? want : maxs);
        if (S > 64) S = 64;
        if (S < 1) S = 1;
    }
    tps = d3f_cdiv(nt, S);
    S = d3f_cdiv(nt, tps);
}
