// Overlap of fragment pairs (datasets/cal_overlap.py:78-126): for pair (a, b) of the elements of ONE built grid, the nearest point
// of b strictly inside the threshold for every point of a.  (included by radius_neighbors.hip; the metric of every search:
// d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA, strict d2 < r2, ties by the smaller index.)
//
// The grid is the only point input.  It is sorted element-major by cell, so the points of element a are the records
// sorted[soffs[a] .. soffs[a+1]) -- position and original index in one 16-byte load, already in a's cell order: neighbouring lanes
// are neighbouring points, fall into the same or adjacent cells of b's grid and walk the same runs of b's records.  The search
// kernels copy the geometry of up to NB_EL_LDS elements to LDS and find each query's element; here the pair names both elements,
// the same for the whole workgroup, so el[b] and the offsets are wave-uniform loads and B may be anything up to D3F_MAX_BATCH.
//
// ONE THREAD PER QUERY, workgroups (x, pair): x strides over a's points.  Most pairs of a scene do not overlap: a pair whose boxes
// (b's grown by the threshold) are disjoint ends at once, a query outside b's grown box costs six comparisons.  The others walk
// the 27-cell stencil as nine runs whose 18 bounds are fetched together.  Counts are summed per thread, per wavefront, per
// workgroup; one atomic per workgroup and pair (integer: independent of the order of arrival).
#pragma once

__global__ void __launch_bounds__(256) nb_overlap_kernel(const NbElem* __restrict__ el, const int* __restrict__ soffs,
                                                         const unsigned* __restrict__ bbox, const int* __restrict__ cell_start,
                                                         const int* __restrict__ cell_base, const float4* __restrict__ sorted, int B,
                                                         const int* __restrict__ pairs, int P, float thr, float r2,
                                                         int* __restrict__ count, int* __restrict__ nearest, int ld) {
    __shared__ int wsum[4];
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        // everything up to the query loop is the same for the whole workgroup
        const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
        if (a < 0 || a >= B || b < 0 || b >= B) {
            if (blockIdx.x == 0 && threadIdx.x == 0) count[p] = -1;      // (the fill came first; the nearest row is all -1 already)
            continue;
        }
        const int a0 = soffs[a], a1 = soffs[a + 1], b0 = soffs[b], b1 = soffs[b + 1];
        if (a1 <= a0 || b1 <= b0) continue;
        // b's box grown by the threshold (in double, then rounded outwards): outside it |q - s| > thr on one axis for every s of b,
        // and then the rounded d2 cannot be below the rounded r2 (rounding is monotone)
        float lo[3], hi[3];
        bool apart = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = __double2float_rd((double)d3f_ord2f(bbox[b * 6 + d]) - (double)thr * 1.000001);
            hi[d] = __double2float_ru((double)d3f_ord2f(bbox[b * 6 + 3 + d]) + (double)thr * 1.000001);
            apart = apart || d3f_ord2f(bbox[a * 6 + 3 + d]) < lo[d] || d3f_ord2f(bbox[a * 6 + d]) > hi[d];
        }
        if (apart) continue;
        const NbElem e = el[b];
        int* row = nearest ? nearest + (size_t)p * ld : nullptr;
        int mine = 0;
        for (int w = a0 + blockIdx.x * 256 + threadIdx.x; w < a1; w += gridDim.x * 256) {
            const float4 me = sorted[w];
            const float qx = me.x, qy = me.y, qz = me.z;
            if (qx < lo[0] || qx > hi[0] || qy < lo[1] || qy > hi[1] || qz < lo[2] || qz > hi[2]) continue;
            int cx, cy, cz;
            nb_cell_of(e, qx, qy, qz, cx, cy, cz);
            cx = min(max(cx, -2), e.dims[0] + 1);
            cy = min(max(cy, -2), e.dims[1] + 1);
            cz = min(max(cz, -2), e.dims[2] + 1);
            const int x0 = max(cx - 1, 0), x1 = min(cx + 1, e.dims[0] - 1);
            if (x0 > x1) continue;
            // the 18 bounds of the nine (y, z) rows in one round trip, then the walks
            int rlo[9], rhi[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int y = cy + (j % 3) - 1, z = cz + (j / 3) - 1;
                rlo[j] = rhi[j] = 0;
                if (y >= 0 && y < e.dims[1] && z >= 0 && z < e.dims[2]) {
                    const int rowbase = e.cbase + e.dims[0] * (y + e.dims[1] * z);
                    rlo[j] = d3f_scan_at(cell_start, cell_base, rowbase + x0);
                    rhi[j] = d3f_scan_at(cell_start, cell_base, rowbase + x1 + 1);
                }
            }
            float bd2 = 3.4e38f;
            int bidx = -1;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                for (int t = rlo[j]; t < rhi[j]; ++t) {
                    const float4 sp = sorted[t];
                    const float d2 = rc_d2(qx, qy, qz, sp.x, sp.y, sp.z);
                    const int si = __float_as_int(sp.w);
                    if (d2 < r2 && (d2 < bd2 || (d2 == bd2 && si < bidx))) { bd2 = d2; bidx = si; }
                }
            }
            if (bidx >= 0) {
                ++mine;
                const int i = __float_as_int(me.w) - a0;                // the point's own index inside a
                if (row && i >= 0 && i < ld) row[i] = bidx - b0;
            }
        }
        // per wavefront, per workgroup, then one atomic
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            if (tot) atomicAdd(&count[p], tot);
        }
        __syncthreads();
    }
}
