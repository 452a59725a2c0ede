// Small shared launchers: fill of 32-bit words, the status pack at the end of a replay, the trace marker.
// (Scans, bounding boxes and the length -> offset prefix are the fused templates of prims.h.)
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Fill of 32-bit words as a plain kernel.  Used instead of hipMemsetAsync so that a captured launch sequence consists of
// kernel nodes only (no runtime-implemented memset nodes inside the HIP graph).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fill_u32_kernel(unsigned* __restrict__ p, size_t n, unsigned v) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n4 = (((uintptr_t)p & 15) == 0) ? n / 4 : 0;
    uint4* p4 = (uint4*)p;
    const uint4 v4 = make_uint4(v, v, v, v);
    for (size_t j = i; j < n4; j += stride) p4[j] = v4;
    for (size_t j = n4 * 4 + i; j < n; j += stride) p[j] = v;
}

int d3f_fill_u32(void* p, size_t n_words, unsigned v, hipStream_t stream) {
    if (n_words == 0) return D3F_OK;
    long long blocks = d3f_cdiv((long long)(n_words / 4 + 1), 256);
    if (blocks > 2048) blocks = 2048;
    fill_u32_kernel<<<(int)blocks, 256, 0, stream>>>((unsigned*)p, n_words, v);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

// ---- trace marker ---------------------------------------------------------------------------------------------------
// A one-thread kernel whose only purpose is to show up BY NAME in a `rocprofv3 --kernel-trace`: bench.py launches it at the
// two ends of its timed region, tools/rocpd_summary.py --timed-region keeps the launches between the first two of them (the
// capture warm-ups, the calibration prologue and the untimed legs of a run stay out of the per-kernel table).
// One launch at the end of a replay: the device-resident sizes and status words of the whole launch sequence packed into ONE
// block (read back by one copy), and the sticky FLAG words (clear[clear_first + i * clear_step]; the size words beside them stay
// readable after the replay) cleared for the next replay -- instead of four copy nodes and a fill
// node per replay (r04: runtime copies and torch fills cost more kernel time than max pooling).
__global__ void __launch_bounds__(256) d3f_pack_status_kernel(int* __restrict__ dst, const int* __restrict__ a, int na,
                                                              const int* __restrict__ b, int nb, const int* __restrict__ c, int nc,
                                                              const int* __restrict__ d, int nd, int* __restrict__ clear, int nclear,
                                                              int clear_first, int clear_step) {
    for (int i = threadIdx.x; i < na; i += blockDim.x) dst[i] = a[i];
    for (int i = threadIdx.x; i < nb; i += blockDim.x) dst[na + i] = b[i];
    for (int i = threadIdx.x; i < nc; i += blockDim.x) dst[na + nb + i] = c[i];
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dst[na + nb + nc + i] = d[i];
    __syncthreads();                    // (`clear` may be one of the sources)
    for (int i = threadIdx.x; i < nclear; i += blockDim.x) clear[clear_first + i * clear_step] = 0;
}
extern "C" int d3f_pack_status(int* dst, const int* a, int na, const int* b, int nb, const int* c, int nc, const int* d, int nd,
                               int* clear, int nclear, int clear_first, int clear_step, void* stream) {
    if (!dst || na < 0 || nb < 0 || nc < 0 || nd < 0 || nclear < 0 || (na && !a) || (nb && !b) || (nc && !c) || (nd && !d) ||
        (nclear && (!clear || clear_first < 0 || clear_step < 1)))
        return D3F_ERR_ARG;
    d3f_pack_status_kernel<<<1, 256, 0, (hipStream_t)stream>>>(dst, a, na, b, nb, c, nc, d, nd, clear, nclear, clear_first, clear_step);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}

__global__ void d3f_trace_marker_kernel(int id, int* sink) {
    if (sink && id == 0x7fffffff) *sink = id;
}
extern "C" int d3f_trace_marker(int id, void* stream) {
    d3f_trace_marker_kernel<<<1, 1, 0, (hipStream_t)stream>>>(id, nullptr);
    D3F_LAUNCH_CHECK();
    return D3F_OK;
}
