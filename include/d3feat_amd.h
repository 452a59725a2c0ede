/*
 * d3feat_amd -- C ABI of the MI355X-native D3Feat inference hot path (libd3feat_amd.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / HIP types in the signatures.
 * Every pointer named *_dev (and every tensor argument) is a DEVICE pointer in HBM unless stated
 * otherwise; `stream` is a hipStream_t passed as void* (NULL = default stream).  All entry points
 * are asynchronous on `stream`, allocate nothing (the caller owns outputs and the workspace) and
 * return D3F_OK or a negative D3F_ERR_* code.  Data-dependent failures that can only be detected
 * on the device are reported through a caller-provided int status[] in HBM (see each function).
 *
 * Each function cites the reference interface (paths relative to the XuyangBai/D3Feat checkout)
 * it replaces.  INTEGRATION.md shows the binding a maintainer of the reference would add.
 */
#ifndef D3FEAT_AMD_H
#define D3FEAT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3F_OK 0
#define D3F_ERR_HIP (-1)        /* a HIP runtime call / kernel launch failed */
#define D3F_ERR_WORKSPACE (-2)  /* workspace too small (see *_workspace_bytes) */
#define D3F_ERR_ARG (-3)        /* invalid argument (negative size, B out of range, bad leading dimension ...) */

/* bits of the device-side status word */
#define D3F_ST_EMPTY_ELEMENT 1   /* a batch element has zero points (UB in the reference, cloud.cpp:30,51)  */
#define D3F_ST_NEG_CELL 2        /* floor((p-origin)/dl) < 0 (the reference's (size_t) cast would be UB, :52-54) */
#define D3F_ST_KEY_RANGE 4       /* voxel key >= 2^56 */
#define D3F_ST_HIT_OVERFLOW 8    /* a query has more in-radius supports than D3F_NEIGHBOR_CAP */
#define D3F_ST_OUT_OVERFLOW 16   /* capacity mode: more output rows than the caller's buffer holds (nothing is written out of bounds) */
#define D3F_ST_KEY_WIDTH 32      /* capacity mode of the grid subsampling: (element, voxel key) needs more than the 32 bits of the
                                    stage-0 sort key (a grid of > 2^32 / B cells): empty result, the synchronous call handles it */

/* pad_value of the neighbour searches meaning "the number of supports as known on the DEVICE" (sum of s_lens_dev) --
 * what BatchOrderedNeighbors pads with (neighbors.cpp:324) when the host only knows an upper bound of Ns */
#define D3F_NB_NO_KMAX 2
#define D3F_PAD_NUM_SUPPORTS (-2147483647 - 1)

#define D3F_MAX_BATCH 255        /* batch elements per stacked call */
#define D3F_NEIGHBOR_CAP 1024    /* max in-radius supports per query that can be ordered */
#define D3F_TOPK_MAX 8192        /* most keypoints per cloud d3f_topk_records selects */
#define D3F_PAIRS_KMAX 1024      /* most rows of one keypoint block d3f_register_pairs uses */
#define D3F_REPEAT_COUNTS_MAX 16 /* most keypoint counts one d3f_repeatability_pairs / d3f_match_pairs call evaluates */
#define D3F_SCENES_MAX 256       /* most scenes one d3f_matching_summary call summarises */
#define D3F_MATCH_KMAX 8192      /* largest keypoint count of d3f_match_pairs (= D3F_TOPK_MAX, the largest block the selection makes) */
#define D3F_VALIDATION_NMAX 1024 /* most index pairs (keypoint correspondences) of one pair d3f_validation_pairs takes */
#define D3F_NUM_KP_MAX 16        /* kernel points per KPConv (reference uses 15) */

int d3f_version(void);

/* Measurement aid (no reference counterpart): launches the one-thread kernel `d3f_trace_marker_kernel` on `stream`, so that
 * a kernel trace of a run can be cut at the ends of a timed region (bench.py; tools/rocpd_summary.py --timed-region). */
int d3f_trace_marker(int id, void* stream);
/* Capacity mode (no reference counterpart: the reference's ops return their sizes to the host one by one): packs up to four device
 * int blocks (sizes, status words, lens) into dst[0 .. na+nb+nc+nd) in ONE launch, then zeroes the nclear words
 * clear[clear_first + i * clear_step] -- the sticky flag words of the searches ([kmax | flags] pairs: first 1, step 2), ready for the
 * next replay (`clear` may alias a source).  Any pointer whose count is 0 may be NULL. */
int d3f_pack_status(int* dst, const int* a, int na, const int* b, int nb, const int* c, int nc, const int* d, int nd,
                    int* clear, int nclear, int clear_first, int clear_step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident sizes ("capacity mode").  The reference's ops have data-dependent output sizes, which costs a host
 * round trip per op (5 per fragment on this path).  Every entry point below therefore also works with sizes that live
 * in HBM: the int size arguments are then UPPER BOUNDS (they size launch grids and buffers) and the real sizes are read on
 * the device -- from the lens arrays for the preprocessing ops, from the optional `*_dev` pointers (NULL = use the host
 * value) for the network ops.  A whole fragment is then a fixed launch sequence: captured once as a HIP graph, replayed
 * for any cloud up to the capacity, with one status read-back at the end.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Grid subsampling.
 * Replaces tf_custom_ops/tf_subsampling: BatchGridSubsampling (tf_batch_subsampling.cpp:8-20,
 * kernel :26-123 -> grid_subsampling/grid_subsampling.cpp:101-149) and GridSubsampling
 * (tf_subsampling.cpp:8-11 -> grid_subsampling.cpp:5-97) with B = 1; with features/classes it also
 * replaces the numeric core of cpp_wrappers/cpp_subsampling (wrapper.cpp:58-286 ->
 * grid_subsampling/grid_subsampling.cpp:5-105).
 *
 *   points   f32[N,3]  stacked clouds          lens_dev  i32[B] points per batch element (device)
 *   features f32[N,fdim] or NULL (fdim 0)      classes   i32[N,ldim] or NULL (ldim 0)
 *   sub_points f32[N,3] (capacity N rows; the first M are valid)   sub_features f32[N,fdim]  sub_classes i32[N,ldim]
 *   sub_lens_dev i32[B]  voxels per element (device copy, feeds the next pyramid level)
 *   status_host i32[B+2] (HOST memory): [0] = M (total voxels), [1] = OR of D3F_ST_* flags, [2..] = voxels per element
 * Output is bit-identical to the reference INCLUDING row order (libstdc++ unordered_map iteration order).
 * The output size is data dependent, so this entry point synchronises `stream` ONCE internally (after the voxel
 * count is known) -- the reference op likewise allocates its output after computing it (tf_batch_subsampling.cpp:96-105).
 * When a flag is raised the outputs are not computed.
 * ------------------------------------------------------------------------------------------- */
size_t d3f_grid_subsample_workspace_bytes(int N, int B, int fdim, int ldim);
/* Capacity-mode form (points only): no host synchronisation.  `points` has N_cap rows of which sum(lens_dev) are valid;
 * sub_points has M_cap rows; elem_cap bounds the voxels of any ONE batch element (0: M_cap) -- the iteration-order rounds
 * are launched for that size, so a stack of B similar clouds should pass its per-cloud capacity; elem_points_cap bounds the
 * POINTS of any one batch element (0: N_cap): when it is at most 16384 every cloud is subsampled by ONE workgroup out of LDS
 * (two launches per call instead of ~25: the coarse pyramid levels); status_dev i32[2] (DEVICE) = [M, OR of D3F_ST_* flags];
 * M > M_cap, an element above elem_cap or above elem_points_cap raises D3F_ST_OUT_OVERFLOW (empty result: status_dev[0] = 0, every
 * length 0, no row of sub_points written -- by every form alike).
 * Workspace: d3f_grid_subsample_workspace_bytes(N_cap, B, 0, 0). */
int d3f_batch_grid_subsample_async(const float* points, int N_cap, const int* lens_dev, int B, float dl,
                                   float* sub_points, int M_cap, int elem_cap, int elem_points_cap, int* sub_lens_dev,
                                   int* status_dev, void* workspace, size_t workspace_bytes, void* stream);
/* d3f_batch_grid_subsample_async with the clouds read IN PLACE: cloud b is its own device array clouds_dev[b] (f32[lens_dev[b], 3])
 * instead of rows of one stacked array -- the stage-0 call of a replayed fragment sequence takes its raw clouds where the
 * producer left them (no copy into a staging buffer: datasets/ThreeDMatch.py:186-192 hands the generator separate arrays too).
 * clouds_dev: device array of B device pointers; N_cap bounds sum(lens_dev).  Results are those of the stacked call. */
int d3f_batch_grid_subsample_async_inplace(const float* const* clouds_dev, int N_cap, const int* lens_dev, int B, float dl,
                                           float* sub_points, int M_cap, int elem_cap, int* sub_lens_dev, int* status_dev,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* The self-pair stacking of the reference's test generators (datasets/ThreeDMatch.py:190-192, demo_registration.py:72-79:
 * np.concatenate([pts, pts])) for B stacked clouds whose row counts live in HBM (lens_in_dev i32[B]): cloud b is written
 * twice in a row -- out f32[2*M_cap,3] = [c_0; c_0; c_1; c_1; ...], lens_out_dev i32[2B] = [m_0, m_0, m_1, m_1, ...],
 * total_dev i32[1] = 2 * sum m_b.  B = 1: the single self-pair; B > 1: several fragments in one stack. */
int d3f_stack_self_pair(const float* pts, int M_cap, const int* lens_in_dev, int B, float* out, int* lens_out_dev,
                        int* total_dev, void* stream);
/* The same two producers with bounding boxes handed along (see d3f_neighbor_grid_build_boxed).
 * d3f_batch_grid_subsample_async_boxed is the capacity-mode subsampling of `points` or, when clouds_dev is given (points NULL), of
 * the clouds in place.  bbox_out_dev (optional) u32[B][6] receives the boxes of the clouds it writes: the sort form accumulates
 * them with atomic min / max into words pre-initialised by d3f_geometry_reset, the one-workgroup form stores them.  bbox_in_dev
 * (optional) = finished boxes of its INPUT clouds: the sort form then skips its boxing pass.
 * d3f_stack_self_pair_boxed: bbox_in_dev u32[B][6] = finished boxes of the B input clouds; bbox_out_dev u32[2B][6] receives them,
 * one per copy (when M_cap cuts a cloud short its box is that of the whole cloud: a superset, which every consumer accepts).
 * NULL box pointers give the plain calls. */
int d3f_stack_self_pair_boxed(const float* pts, int M_cap, const int* lens_in_dev, int B, float* out, int* lens_out_dev,
                              int* total_dev, const unsigned* bbox_in_dev, unsigned* bbox_out_dev, void* stream);
int d3f_batch_grid_subsample_async_boxed(const float* points, const float* const* clouds_dev, int N_cap, const int* lens_dev,
                                         int B, float dl, float* sub_points, int M_cap, int elem_cap, int elem_points_cap,
                                         int* sub_lens_dev, int* status_dev, const unsigned* bbox_in_dev,
                                         unsigned* bbox_out_dev, void* workspace, size_t workspace_bytes, void* stream);
int d3f_batch_grid_subsample(const float* points, int N, const int* lens_dev, int B, float dl,
                             const float* features, int fdim, const int* classes, int ldim,
                             float* sub_points, float* sub_features, int* sub_classes, int* sub_lens_dev,
                             int* status_host, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Radius neighbours.
 * Replaces tf_custom_ops/tf_neighbors: BatchOrderedNeighbors (tf_batch_neighbors.cpp:8-30, kernel
 * :36-120 -> neighbors/neighbors.cpp:211-332 batch_nanoflann_neighbors / :125-208
 * batch_ordered_neighbors).  Per query: all supports of the same batch element with fp32
 * d2 = (dx*dx + dy*dy) + dz*dz < radius*radius (strict, no FMA), ordered by (d2, support index)
 * ascending -- exactly batch_ordered_neighbors, and equal to the active nanoflann path except inside
 * runs of bit-equal d2 (whose order nanoflann leaves unspecified).
 *
 *   queries f32[Nq,3], supports f32[Ns,3], q_lens_dev / s_lens_dev i32[B]
 *   out i32[Nq, ld]: columns [0,width) are written: the first min(count,width) neighbours then pad_value
 *       (pass Ns for BatchOrderedNeighbors, neighbors.cpp:324; -1 for OrderedNeighbors, neighbors.cpp:111-119)
 *   status_dev i32[2]: [0] = max neighbour count over all queries (the reference's output width Kmax),
 *                      [1] = OR of D3F_ST_* flags
 * `width` plays the role of datasets/common.py:399-406 (big_neighborhood_filter): pass the layer's
 * neighborhood limit; pass width = ld >= Kmax to get the untruncated matrix.
 * Nq / Ns are upper bounds (buffer rows): the real counts are sum(q_lens_dev) / sum(s_lens_dev), read on the device.
 * pad_value D3F_PAD_NUM_SUPPORTS pads with the device-side number of supports.
 * ------------------------------------------------------------------------------------------- */
size_t d3f_radius_neighbors_workspace_bytes(int Nq, int Ns, int B);
int d3f_batch_radius_neighbors(const float* queries, int Nq, const float* supports, int Ns,
                               const int* q_lens_dev, const int* s_lens_dev, int B, float radius,
                               int* out, int ld, int width, int pad_value, int* status_dev,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Two-step form of the same op.  datasets/common.py:1344,1367 search the SAME supports with the SAME radius twice
 * per pyramid level (conv_i and pool_i), so the cell grid is an object the caller keeps:
 *   d3f_neighbor_grid_build   supports -> cell grid (counting sort by cell) inside caller memory `grid`
 *                             (>= d3f_neighbor_grid_bytes(Ns, B) bytes, must stay untouched until the last search)
 *   d3f_neighbor_grid_search  queries against a built grid.
 *       queries_are_supports  1 when `queries` is the very array the grid was built from: queries are then visited in
 *                             cell order (L2 locality); results are identical either way
 *       cap                   in-radius supports per query that can be ordered (LDS budget; <= D3F_NEIGHBOR_CAP);
 *                             a query with more sets D3F_ST_HIT_OVERFLOW -> search again with a larger cap
 *       first_only            1: only column 0 (the nearest support, ties by index) is computed -- all that
 *                             closest_pool reads of the upsampling matrices (models/network_blocks.py:81);
 *                             columns 1..width-1 are filled with pad_value
 *       nn_hint               (first_only) > 0: the caller expects the nearest support within this distance (< radius), e.g.
 *                             sqrt(3) dl for the upsampling matrices, whose supports are the voxel barycentres of the queries:
 *                             only the cells that ball touches are visited first; a query whose nearest support is farther
 *                             is searched again over the full stencil, so the result never depends on the hint.  0: none
 *       reset_status          bit 0: status_dev is zeroed first (one extra launch); clear: the caller zeroed it (a
 *                             captured fragment zeroes the status words of all its ops with one fill).
 *                             bit 1 (D3F_NB_NO_KMAX): status_dev[0] (the largest neighbour count, which only callers that
 *                             size their output by it need) is NOT maintained -- every query otherwise reads one shared
 *                             word through L2, a same-address hot spot that serialises the whole launch
 */
size_t d3f_neighbor_grid_bytes(int Ns, int B);
/* byte offset inside a built grid of `order` i32[Ns]: the support indices sorted by cell.  Passing it as q_order /
 * row_order to the per-point kernels below makes them visit points in a spatially coherent order (neighbouring
 * workgroup rows share their gathered neighbours in L1 / L2); results do not depend on it. */
size_t d3f_neighbor_grid_order_offset(int Ns, int B);
int d3f_neighbor_grid_build(const float* supports, int Ns, const int* s_lens_dev, int B, float radius,
                            void* grid, size_t grid_bytes, void* stream);
/* d3f_neighbor_grid_build from FINISHED bounding boxes: bbox_dev u32[B][6] (ordered-uint min xyz, max xyz) of the B clouds, gathered
 * by the kernel that wrote `supports` (the *_boxed producers below and above).  Nothing reads the cloud to box it and no workgroup
 * waits for another: the geometry is derived per workgroup.  Two forms, chosen on the host from the capacities only
 * (d3f_neighbor_grid_boxed_form: 1 = small, 2 = large):
 *   small  ceil(Ns / B) <= T (4096; environment D3F_NB_SMALL_T): ONE launch, one workgroup per cloud, cell counters / scan in LDS; the
 *          cell budget of a cloud is min(d3f_neighbor_grid_build's, 8192) -- a cloud over it gets a coarser cell edge, as there
 *   large  three launches (count, scan, scatter); its cell counters and scan ticket must have been cleared by d3f_geometry_reset
 * The grid object serves every search exactly as one built by d3f_neighbor_grid_build; the order of the supports INSIDE a cell
 * (atomics) is the only freedom, and no search result depends on it.
 *   d3f_geometry_reset: ONE launch that prepares a whole chain of boxed calls -- n_boxes box rows get their initial values (the
 *   producers accumulate into them with atomic min / max), and every large-form grid of the list (HOST arrays of n_grids <=
 *   D3F_GRID_RESET_MAX grid objects with their byte sizes, Ns and B) has its counters cleared.  It must precede the producers. */
#define D3F_GRID_RESET_MAX 8
int d3f_neighbor_grid_boxed_form(int Ns, int B);
int d3f_geometry_reset(unsigned* boxes_dev, int n_boxes, const void* const* grids, const size_t* grid_bytes, const int* Ns,
                       const int* B, int n_grids, void* stream);
int d3f_neighbor_grid_build_boxed(const float* supports, int Ns, const int* s_lens_dev, int B, float radius,
                                  const unsigned* bbox_dev, void* grid, size_t grid_bytes, void* stream);
int d3f_neighbor_grid_search(const void* grid, size_t grid_bytes, int Ns, const float* queries, int Nq,
                             const int* q_lens_dev, int B, float radius, int queries_are_supports,
                             int* out, int ld, int width, int pad_value, int cap, int first_only, float nn_hint,
                             int reset_status, int* status_dev, void* stream);
/* The general form of d3f_neighbor_grid_search: the queries may bring a grid of their own.
 *   query_grid   a grid built by d3f_neighbor_grid_build over `queries` themselves (any radius; Nq rows capacity, the same B), or
 *                `grid` itself when the queries ARE the supports, or NULL.  The queries are visited in ITS cell order: neighbouring
 *                wavefronts then read the same support runs.  Results do not depend on it -- unless D3F_NB_INTERNAL is set.
 *   flags        bit 0: zero status_dev first; bit 1 (D3F_NB_NO_KMAX); bit 2 (D3F_NB_INTERNAL, needs query_grid): the INTERNAL
 *                numbering of a pipeline that keeps every level in cell-sorted order -- row j of `out` belongs to the j-th query
 *                in the query grid's cell order (not to query j), and every entry is the POSITION of that support in `grid`'s cell
 *                order (d3f_neighbor_grid_inv_offset) instead of its index.  Which supports a row holds and their order (d2, then
 *                the ORIGINAL index) are exactly those of the reference numbering: renumbering both sides back gives the
 *                matrix of d3f_neighbor_grid_search bit for bit (tests/test_gpu_internal_order.py).  pad_value is written as is.
 *   first_only with D3F_NB_NO_KMAX: column 0 by the nearest-support kernel (four lanes per query). */
#define D3F_NB_INTERNAL 4
int d3f_neighbor_grid_search_ordered(const void* grid, size_t grid_bytes, int Ns, const float* queries, int Nq,
                                     const int* q_lens_dev, int B, float radius, const void* query_grid, size_t query_grid_bytes,
                                     int* out, int ld, int width, int pad_value, int cap, int first_only, float nn_hint, int flags,
                                     int* status_dev, void* stream);
/* byte offsets inside a built grid of `inv` i32[Ns] (position of support i in cell order: the inverse of `order`) and of `xyz`
 * f32[Ns, 3] (the supports in cell order: the point array of a level kept in the internal numbering). */
size_t d3f_neighbor_grid_inv_offset(int Ns, int B);
size_t d3f_neighbor_grid_xyz_offset(int Ns, int B);



/* ---------------------------------------------------------------------------------------------
 * KPConv, phase 1: neighbour gather + kernel-point influence + weighted aggregation.
 * Replaces the first half of kernels/convolution_ops.py:161-255 (KPConv_ops :186-240, :250-252):
 *   wf[n,p,c]  = sum_k  h(|| (s[idx[n,k]] - q[n]) - KP[p] ||) * f[idx[n,k], c]
 *   inv_cnt[n] = 1 / max(#{k : row_pos[idx[n,k]]}, 1),  row_pos from d3f_row_positive(f)
 * influence: 0 constant, 1 linear  h = max(1 - sqrt(d2+1e-10)/(2*KP_extent), 0), 2 gaussian (sigma = 0.3*KP_extent);
 * aggregation: 0 sum, 1 closest.  Shadow neighbours (idx >= Ns) contribute nothing.
 *   q f32[Nq,3]  s f32[Ns,3]  idx i32[Nq,ld_idx] (K columns used)  f f32[Ns,ldf] (Cin columns used)
 *   kp_host f32[num_kp,3] (HOST pointer: 45 floats passed by value to the kernel)  wf f32[Nq, num_kp*Cin]  inv_cnt f32[Nq]
 * Phase 2 is d3f_gemm_f32(wf, K_values reshaped [num_kp*Cin, Cout]) with row_scale = inv_cnt.
 * Nq_dev / Ns_dev (device i32, may be NULL): real row counts when Nq / Ns are capacities (see "Device-resident sizes").
 * ------------------------------------------------------------------------------------------- */
/* row_pos[s] = (sum_c f[s,c] > 0): the per-support test behind the neighbour count (:250-251), evaluated once
 * per support row.  row_pos u8[Ns]. */
/* feat_bf16 (here and in the KPConv / pooling / contraction entry points below): 0 = feature tensors are f32 (the parity path);
 * 1 = BASELINE configs[4] "bf16 features": every feature tensor named f / x / out / residual holds bfloat16 values (2 bytes per
 * element, leading dimensions in elements, 8-byte aligned rows); all arithmetic stays fp32, values are rounded to nearest even
 * when stored.  Only the shipped configuration (linear influence, 'sum', <= 15 kernel points) has the bf16 forms. */
int d3f_row_positive(const void* f, int Ns, int ldf, int Cin, unsigned char* row_pos, const int* Ns_dev, int feat_bf16,
                     void* stream);
int d3f_kpconv_aggregate(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                         const void* f, int ldf, int Cin, const unsigned char* row_pos, const float* kp_host,
                         int num_kp, float KP_extent, int influence, int aggregation, float* wf, float* inv_cnt,
                         const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deformable KPConv, phase 1: the first half of kernels/convolution_ops.py:379-499 (KPConv_deform_ops), the kernel points of
 * every query moved by its own offsets:
 *   KP'[n,p]  = kp[p] + offsets[n, 3p .. 3p+2] * offset_scale
 *   mod[n,p]  = modulations ? (mod_logits ? 2 * sigmoid(modulations[n,p]) : modulations[n,p]) : 1
 *   in[n,k]   = any_p || (s[idx[n,k]] - q[n]) - KP'[n,p] ||^2 < KP_extent^2
 *   wf[n,p,c] = mod[n,p] * sum_{k : in[n,k]}  h(|| (s[idx[n,k]] - q[n]) - KP'[n,p] ||) * f[idx[n,k], c]
 * influence: 0 constant  h = (d2 < KP_extent^2), 1 linear  h = max(1 - sqrt(d2+1e-10)/KP_extent, 0)  (KP_extent, not 2*KP_extent
 * as in d3f_kpconv_aggregate), 2 gaussian (sigma = 0.3*KP_extent); aggregation: 0 sum, 1 closest (arg-min over the DEFORMED points).
 * A neighbour within KP_extent of no deformed point contributes nothing, for any influence; shadow neighbours (idx outside
 * [0, Ns)) neither.  There is no neighbour count: the reference does not normalise this operator.
 *   offsets f32[Nq, ld_off] (3*num_kp columns used)   modulations f32[Nq, ld_mod] (num_kp columns used) or NULL
 *   other operands as d3f_kpconv_aggregate; wf f32[Nq, num_kp*Cin]
 * KPConv_deformable (:258-376) passes the RAW output x f32[Nq, 4*num_kp] of its offset convolution: offsets = x, offset_scale =
 * KP_extent, modulations = x + 3*num_kp, ld_mod = ld_off, mod_logits = 1 -- the scaling and the sigmoid cost no launch of their own.
 * KPConv_deform_ops' own arguments are offset_scale = 1, mod_logits = 0.
 * Phase 2 is d3f_gemm_f32(wf, K_values reshaped [num_kp*Cin, Cout]) without row_scale.
 * fp32 feature rows only: feat_bf16 != 0 is D3F_ERR_ARG.  Ns == 0 with Nq > 0 is D3F_ERR_ARG.
 * ------------------------------------------------------------------------------------------- */
int d3f_kpconv_deform_aggregate(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                                const void* f, int ldf, int Cin, const float* offsets, int ld_off, float offset_scale,
                                const float* modulations, int ld_mod, int mod_logits, const float* kp_host, int num_kp,
                                float KP_extent, int influence, int aggregation, float* wf, const int* Nq_dev, const int* Ns_dev,
                                const int* q_order, int feat_bf16, void* stream);

/* Whole KPConv_ops (kernels/convolution_ops.py:161-255) + the fused inference epilogue for Cin = 1 -- the input
 * layer of every shipped model (`simple` block on the all-ones features, models/network_blocks.py:222-244):
 *   out[n,o] = act( (sum_p wf[n,p] * W[p,o]) / max(#{k : f[idx[n,k]] > 0}, 1) * col_scale[o] + col_shift[o] + residual[n,o] )
 * f f32[Ns,1] (ldf), W f32[num_kp, Cout] (= K_values[:,0,:]); one kernel, only `out` is written to HBM. */
int d3f_kpconv_fused_c1(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                        const float* f, int ldf, const float* kp_host, int num_kp, float KP_extent, int influence,
                        int aggregation, const float* W, int Cout, const float* col_scale, const float* col_shift,
                        const float* residual, int ldr, int leaky, float alpha, void* out, int ldo,
                        const int* Nq_dev, const int* Ns_dev, const int* q_order, int out_bf16, void* stream);

/* Whole KPConv_ops + inference epilogue for Cin = Cout = 32 (the level-0 convolutions of the shipped architecture) in one
 * launch: gather + influences + aggregation as d3f_kpconv_aggregate, then the 32 x (num_kp*32) tile of weighted features is
 * contracted with K_values on the matrix cores straight from LDS -- the wf tensor (Nq x 480 floats) never reaches HBM.
 *   W f32[num_kp*32, 32] (= K_values reshaped, contiguous);  out f32[Nq, 32] (ldo);  row_pos from d3f_row_positive(f)
 *   out = act( (wf @ W) / max(count, 1) * col_scale + col_shift + residual ) */
int d3f_kpconv_fused32(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                       const void* f, int ldf, const unsigned char* row_pos, const float* kp_host, int num_kp,
                       float KP_extent, int influence, int aggregation, const float* W, const float* col_scale,
                       const float* col_shift, const float* residual, int ldr, int leaky, float alpha, void* out, int ldo,
                       const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16, void* stream);

/* Whole KPConv_ops + epilogue in one kernel for Cin == Cout in {64, 128, 256} (levels 1 to 3 of the shipped architecture), the
 * [Nq, 15*Cin] weighted-feature tensor of kernels/convolution_ops.py:237-240 staying in LDS (tiles of 16 queries, passes of
 * 512 k-values, v_mfma_f32_16x16x4_f32).  Only the configuration of the shipped models (linear influence, 'sum'
 * aggregation, 15 kernel points): d3f_kpconv_fused_supported() says whether a call qualifies (1: use it; 2: the form
 * exists -- Cin = 256 -- but aggregation + contraction measured no slower; 0: not available); otherwise use
 * d3f_kpconv_aggregate + d3f_gemm_f32.  W_packed: K_values [15*Cin, Cout] reordered once by d3f_kpconv_pack_weights
 * (Wp[blk][g][n][j] = W[16*blk + 4*g + j][n]: the MFMA B-operand order, one 16-byte load per lane and k-block).
 * Arguments otherwise as d3f_kpconv_fused32.
 * Size limit of the one-kernel forms (d3f_kpconv_fused32 / d3f_kpconv_fused): rows are addressed with 24-bit multiplies, so
 * Nq, Ns, ld_idx, ldf < 2^24 and Nq * ld_idx, Ns * ldf < 2^31, else D3F_ERR_ARG (d3f_kpconv_aggregate + d3f_gemm_f32 have no
 * such limit: beyond it they take their generic kernel). */
int d3f_kpconv_fused_supported(int Cin, int Cout, int num_kp, int influence, int aggregation);
int d3f_kpconv_pack_weights(const float* W, int K, int N, float* W_packed, void* stream);
/* The same operator (kernels/convolution_ops.py:161-255 + epilogue) with its 15*Cin-deep contraction in the operand-split form of
 * d3f_gemm_x3 (round 5): the weighted features are written to LDS as three exact bfloat16 planes, K_values is pre-split once per
 * tensor by d3f_kpconv_pack_weights_x3 into d3f_kpconv_packed_x3_bytes(K, N) = 6 K N bytes (the B fragments of
 * v_mfma_f32_16x16x32_bf16; K % 32 == 0, N % 16 == 0), six exact products per fp32 product, fp32 accumulation: fp32 in, fp32 out,
 * 2.5 x less matrix-pipe time than v_mfma_f32_16x16x4_f32.  Arguments as d3f_kpconv_fused, W_packed = the planes. */
/* (N = 32: the fragment order of d3f_kpconv_fused32_x3, v_mfma_f32_32x32x16_bf16; any other N: d3f_kpconv_fused_x3's.) */
size_t d3f_kpconv_packed_x3_bytes(int K, int N);
int d3f_kpconv_pack_weights_x3(const float* W, int K, int N, void* W_planes, void* stream);
/* d3f_kpconv_fused32 (Cin = Cout = 32, the level-0 convolutions) with the split contraction; W_planes =
 * d3f_kpconv_pack_weights_x3(K_values [15*32, 32]).  Arguments as d3f_kpconv_fused32. */
int d3f_kpconv_fused32_x3(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                          const void* f, int ldf, const unsigned char* rowpos, const float* kp_host, int num_kp,
                          float KP_extent, int influence, int aggregation, const float* W_planes, const float* col_scale,
                          const float* col_shift, const float* residual, int ldr, int leaky, float alpha, void* out,
                          int ldo, const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16, void* stream);
int d3f_kpconv_fused_x3(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                        const void* f, int ldf, int Cin, const unsigned char* rowpos, const float* kp_host, int num_kp,
                        float KP_extent, int influence, int aggregation, const float* W_planes, int Cout,
                        const float* col_scale, const float* col_shift, const float* residual, int ldr, int leaky,
                        float alpha, void* out, int ldo, const int* Nq_dev, const int* Ns_dev, const int* q_order,
                        int feat_bf16, void* stream);
int d3f_kpconv_fused(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K,
                     const void* f, int ldf, int Cin, const unsigned char* rowpos, const float* kp_host, int num_kp,
                     float KP_extent, int influence, int aggregation, const float* W_packed, int Cout,
                     const float* col_scale, const float* col_shift, const float* residual, int ldr, int leaky,
                     float alpha, void* out, int ldo, const int* Nq_dev, const int* Ns_dev, const int* q_order,
                     int feat_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense contraction on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, fmaf-chain numerics).
 * Replaces kernels/convolution_ops.py:90-99 (unary_convolution = tf.matmul) and :243-253 (the
 * kernel-weight contraction + neighbour-count normalisation), with the inference epilogue of
 * models/network_blocks.py:149-160,185-186 fused:
 *   C[m,n] = act( (sum_k A[m,k] B[k,n]) * row_scale[m] * col_scale[n] + col_shift[n] + residual[m,n] )
 * row_scale / col_scale / col_shift / residual may be NULL (identity); act = LeakyReLU(alpha) when
 * leaky != 0.  A f32[M,K] (lda), B f32[K,N] (ldb), C f32[M,N] (ldc), residual f32[M,N] (ldr).
 * workspace is used only when the call decides to split K (skinny shapes).
 * M_dev (device i32, may be NULL): real row count when M is a capacity; M_hint (0 = none): the row count the caller
 * expects, used only to plan the K split (pass the same value to d3f_gemm_workspace_bytes).
 * ------------------------------------------------------------------------------------------- */
size_t d3f_gemm_workspace_bytes(int M, int N, int K, int M_hint);
int d3f_gemm_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                 const float* row_scale, const float* col_scale, const float* col_shift,
                 const float* residual, int ldr, int leaky, float alpha,
                 void* workspace, size_t workspace_bytes, const int* M_dev, int M_hint, void* stream);

/* Decoder step: nearest upsampling + skip concatenation + the unary block that consumes them, as ONE contraction whose
 * A operand is composed on the fly (the concatenated tensor never exists in HBM).  Replaces models/D3Feat.py:39-63
 * (closest_pool, models/network_blocks.py:69-83, then tf.concat) followed by unary_block (models/network_blocks.py:207-219):
 *   C[m, :] = act( ([ x'[idx[m,0]] | skip[m] ] @ W) * col_scale + col_shift ),   x' = x with a zero row appended
 *   x f32[N1,C1] (ldx), idx i32[M, ld_idx] (column 0 is read), skip f32[M,C2] (lds; NULL when C2 = 0), W f32[C1+C2, N] (ldb)
 *   C1 % 4 == 0 when C2 > 0.  M_dev / N1_dev / M_hint as for d3f_gemm_f32; workspace: d3f_gemm_workspace_bytes(M, N, C1+C2, M_hint).
 * idx == NULL: no gather, A = [ x[m] | skip[m] ] -- used to contract the two branches of a resnet block in one launch
 * (models/network_blocks.py:321-368: conv3 + shortcut, batch-norm scales folded into the stacked weights). */
int d3f_gemm_upsample_cat_f32(const float* x, int N1, int ldx, int C1, const int* idx, int ld_idx,
                              const float* skip, int lds, int C2, const float* W, int ldb, float* C, int ldc,
                              int M, int N, const float* col_scale, const float* col_shift, int leaky, float alpha,
                              void* workspace, size_t workspace_bytes, const int* M_dev, const int* N1_dev,
                              int M_hint, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pooling / upsampling gathers.
 *   d3f_ind_max_pool      models/network_blocks.py:51-66  out[n,c] = max_k x'[idx[n,k],c], x' = x + row of column minima
 *   d3f_closest_pool_cat  models/network_blocks.py:69-83 + models/D3Feat.py:63
 *                         out[n, 0:C1] = x'[idx[n,0]] (x' = x + zero row), out[n, C1:C1+C2] = skip[n]  (skip may be NULL, C2 0)
 *   col_min_dev: unused since round 6 (may be NULL): the column minima are taken inside the one pooling launch, by the
 *   threads of a row that has no valid neighbour and therefore takes the shadow row.
 * ------------------------------------------------------------------------------------------- */
int d3f_ind_max_pool(const void* x, int N1, int ldx, int C, const int* idx, int N2, int ld_idx, int K,
                     void* out, int ldo, float* col_min_dev, const int* N1_dev, const int* N2_dev, const int* row_order,
                     int feat_bf16, void* stream);
int d3f_closest_pool_cat(const float* x, int N1, int ldx, int C1, const int* idx, int N2, int ld_idx,
                         const float* skip, int lds, int C2, float* out, int ldo, const int* N1_dev, const int* N2_dev,
                         void* stream);

/* Stand-alone form of the GEMM epilogue (models/network_blocks.py:149-160 batch_norm in inference mode folded to
 * scale/shift, :185-186 leaky_relu, residual add):  out = act(x * col_scale + col_shift + residual). */
int d3f_affine_act(const float* x, int ldx, int M, int N, const float* col_scale, const float* col_shift,
                   const float* residual, int ldr, int leaky, float alpha, float* out, int ldo, const int* M_dev,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * D3Feat head: descriptors + detection scores.  Replaces models/D3Feat.py:65-115.
 *   x f32[N,C] (ldx)  un-normalised output of last_unary;  idx i32[N,ld_idx] level-0 neighbours (K columns)
 *   lens_dev i32[B] points per stacked cloud (B = 2 in the reference, any B >= 1 here)
 *   include_zero_dev i32[B] (device) or NULL: 1 if the cloud's row of in_batches contains the shadow index (so that
 *       the per-cloud maximum of :84-85 includes the zero row) -- datasets/common.py:453-496; NULL derives it from
 *       lens_dev on the device (shorter than the longest cloud, or all clouds equally long)
 *   stack_group: 0 = the B clouds are ONE reference stack (the rule above is applied over all of them); g > 0 = the
 *       stack is a concatenation of independent reference stacks of g consecutive clouds each (the fragment engine's
 *       batched replays: g = 2 pairs, g = 1 self-pairs computed once) and the rule is applied inside every group, so a
 *       fragment's result never depends on its stack mates.  Ignored when include_zero_dev is given.
 *   N is an upper bound: the real point count is sum(lens_dev)
 *   desc f32[N,C] = l2_normalize(x, eps 1e-10);  score f32[N]
 *   scratch_dev: >= 2*B + 2 + (N + 3) / 4 ints of device scratch (per-cloud maxima, offsets, one flag byte per row).  C <= 128.
 * ------------------------------------------------------------------------------------------- */
int d3f_detect_head(const float* x, int N, int ldx, int C, const int* idx, int ld_idx, int K,
                    const int* lens_dev, const int* include_zero_dev, int stack_group, int B, float* desc, int ldd,
                    float* score, int* scratch_dev, const int* row_order, void* stream);

/* The per-point output record of the path: out[n] = [ xyz(3) | desc(C) | score(1) ], f32, row stride ldo >= C + 4.
 * Replaces the three arrays the testers keep per fragment (utils/tester.py:215-229: points, features, scores written
 * side by side) with one contiguous block per fragment -- the unit the multi-GPU runner gathers once at the end.
 * N is an upper bound when N_dev (device int) is given. */
int d3f_pack_descriptors(const float* xyz, const float* desc, int ldd, int C, const float* score, int N, float* out,
                         int ldo, const int* N_dev, void* stream);
/* d3f_pack_descriptors with per-fragment destinations: the stack holds B clouds (lens_dev), a fragment is `group` consecutive
 * clouds; the rows of the first `keep` clouds of fragment f go to the address dst_ptrs_dev[f] (f32 rows of ldo floats, the
 * fragment's kept rows packed from row 0) when that entry is non-zero, every other row to `out` as in d3f_pack_descriptors.
 * What utils/tester.py:208-229 keeps of a stacked self-pair is its first cloud (in_batches[0]): group = 2, keep = 1 writes exactly
 * that, straight into the caller's shard buffer -- a replayed sequence needs no copy after it.
 * row_map_dev (optional, i32[N]): the inputs are in an internal row order (the cell order of the level-0 grid), record n belongs
 * at row row_map_dev[n] of the reference order -- the one place where a pipeline on the internal numbering returns to the
 * reference's row order.  dst_ptrs_dev may be NULL when only the row map is wanted. */
int d3f_pack_descriptors_to(const float* xyz, const float* desc, int ldd, int C, const float* score, int N, float* out,
                            int ldo, const int* N_dev, const int* lens_dev, int B, int group, int keep,
                            const long long* dst_ptrs_dev, const int* row_map_dev, void* stream);

/* Keypoint selection: for every kept cloud of a stack the K records with the highest detection scores, in ascending score order --
 *     sel = np.argsort(s, kind="stable")[-K:];  out = records[sel]                      (min(n, K) rows)
 * which is what the reference does on the host after every sess.run: its testers order a fragment's rows by score
 * (utils/tester.py:208-213, demo_registration.py:159-163: np.argsort(scores)) and every consumer keeps the tail
 * (geometric_registration/evaluate.py:45-50 [-num_keypts:], utils/tester.py:283-284, demo_registration.py:249,261 [-50:]).
 * Order of the keys: numpy's for float32 (-0.0 == +0.0, every NaN after +inf, all NaNs tied); ties in ascending row index, so among
 * the rows whose score equals the K-th largest the HIGHEST rows are kept.  Rows are the reference's rows of the cloud.
 * Inputs as d3f_pack_descriptors_to takes them, each with its own row stride in floats: xyz (ldx >= 3), desc (ldd >= C), score
 * (lds >= 1) -- a finished record block `rec` of row stride ld is xyz = rec, desc = rec + 3, score = rec + 3 + C, all strides ld.
 * The stack holds B clouds (lens_dev i32[B]; N bounds the stack's rows, N_dev optional as everywhere); a fragment is `group`
 * consecutive clouds and its first `keep` are kept (d3f_pack_descriptors_to's rule); row_map_dev (optional) has that function's
 * meaning: input row n is stack-global reference row row_map_dev[n], a cloud's rows stay inside its own range, and the row of a
 * record is its reference row minus the cloud's start.  n_cap: upper bound of one cloud's rows, < 2^24 (rows of a cloud beyond it
 * are not looked at); it plans the launch (workgroups per cloud, keys in LDS or through the workspace).
 * Kept cloud j (stack order, ceil(B / group) * keep of them): rows out + j * K * ldo, [xyz | desc | score] of ldo >= C + 4 floats, the
 * first count_dev[j] = min(n_j, K) rows written, the rest untouched; idx_out (optional) i32[., K] the reference row inside the
 * cloud; count_dev (optional) i32[.].  `out` must not overlap the inputs.  One launch, asynchronous on `stream`, no allocation, no
 * synchronisation; every data-dependent size is read on the device.  1 <= K <= D3F_TOPK_MAX.
 * tickets_dev (optional) i32[kept clouds], ZERO before the first call and left zero by every call: with it a long cloud is split over
 * up to 16 workgroups that hand their candidates to the last one to finish; calls that can overlap (different streams) need their own.
 * NULL: one workgroup per cloud.  workspace >= d3f_topk_workspace_bytes(N, B, n_cap, K), else D3F_ERR_WORKSPACE. */
size_t d3f_topk_workspace_bytes(int N, int B, int n_cap, int K);
int d3f_topk_records(const float* xyz, int ldx, const float* desc, int ldd, int C, const float* score, int lds, int N,
                     const int* N_dev, const int* lens_dev, int B, int group, int keep, const int* row_map_dev, int n_cap, int K,
                     float* out, int ldo, int* idx_out, int* count_dev, int* tickets_dev, void* workspace, size_t workspace_bytes,
                     void* stream);

/* LDS-DMA form of the fp32 contractions (round 4): the operator of d3f_gemm_f32 / d3f_gemm_upsample_cat_f32 with the same
 * composite A operand as d3f_gemm_bf16 below -- A f32[., C1] (rows in place when idx == NULL, else the gathered rows x'[idx[m,0]],
 * zero row for indices outside [0, N1)), optional second operand skip f32[M, C2], K = C1 + C2 -- and the same epilogue
 * (kernels/convolution_ops.py:90-99,243-253 + models/network_blocks.py:149-160,185-186 + the resnet residual add), exact fp32
 * products and sums on v_mfma_f32_32x32x2_f32.  The weights are handed over PRE-TRANSPOSED: Wt = d3f_gemm_pack_f32t(W f32[K,N])
 * -> f32 [N][Kp], Kp = K rounded up to 32, zero padded (4 * N * Kp bytes), made once per weight tensor.  Requires float4-addressable
 * operands (C1, C2, N, lda, lds, ldc, ldr multiples of 4; 16-byte aligned bases): D3F_ERR_ARG otherwise -- use d3f_gemm_f32 then.
 * workspace >= d3f_gemm_workspace_bytes(M, N, K, M_hint). */
int d3f_gemm_pack_f32t(const float* W, int ldb, int K, int N, float* Wt, void* stream);
int d3f_gemm_f32t(const float* A, int N1, int lda, int C1, const int* idx, int ld_idx, const float* skip, int lds, int C2,
                  const float* Wt, float* C, int ldc, int M, int N, const float* row_scale, const float* col_scale,
                  const float* col_shift, const float* residual, int ldr, int leaky, float alpha, void* workspace,
                  size_t workspace_bytes, const int* M_dev, const int* N1_dev, int M_hint, void* stream);

/* Operand-split form of the fp32 contractions: the operator, operands and epilogue of d3f_gemm_f32t, with every fp32 operand value
 * written EXACTLY as the sum of three bfloat16 values (8 + 8 + 8 significant bits) and every fp32 product as the six exact bf16
 * products whose sum differs from it by < 2^-23 relative, accumulated in fp32 on v_mfma_f32_32x32x16_bf16 (d3feat_amd/csrc/gemm_x3.h).
 * fp32 in, fp32 out, fp32-grade error (tests/test_gpu_gemm_x3.py measures it against float64 beside d3f_gemm_f32t's); the weights are
 * handed over PRE-SPLIT: Wx = d3f_gemm_pack_x3(W f32[K,N]), d3f_gemm_x3_packed_bytes(K, N) bytes, made once per weight tensor.
 * On top of d3f_gemm_f32t's addressing rules: K = C1 + C2 a multiple of 32 and, with a second operand, C1 a multiple of 32 too --
 * D3F_ERR_ARG otherwise (use d3f_gemm_f32t).  workspace >= d3f_gemm_x3_workspace_bytes(M, N, K, M_hint). */
size_t d3f_gemm_x3_packed_bytes(int K, int N);
int d3f_gemm_pack_x3(const float* W, int ldb, int K, int N, void* Wx, void* stream);
size_t d3f_gemm_x3_workspace_bytes(int M, int N, int K, int M_hint);
/* the workgroup shape (rows x cols: 128 x 32, 128 x 64 or 256 x 128) and K slice count d3f_gemm_x3 uses for a problem; D3F_ERR_ARG
 * for a K it does not take.  Diagnostics / tests only: the launcher decides by itself. */
int d3f_gemm_x3_plan(int M, int N, int K, int M_hint, int* rows, int* cols, int* slices);
/* 1 when d3f_gemm_x3 takes its resident-W persistent form for a problem (from 65536 expected rows on, 32, 64 or 128 columns, and the
 * whole pre-split W within the LDS of a CU), else 0.  The launcher decides with this same function. */
int d3f_gemm_x3_resident(int M, int N, int K, int M_hint);
int d3f_gemm_x3(const float* A, int N1, int lda, int C1, const int* idx, int ld_idx, const float* skip, int lds, int C2,
                const void* Wx, float* C, int ldc, int M, int N, const float* row_scale, const float* col_scale,
                const float* col_shift, const float* residual, int ldr, int leaky, float alpha, void* workspace,
                size_t workspace_bytes, const int* M_dev, const int* N1_dev, int M_hint, void* stream);
/* d3f_gemm_x3 with a GATHERED residual operand: output row m adds residual[res_idx[m * ld_res_idx]] (int32 indices, ld_res_idx >= 1)
 * instead of residual[m].  The residual tensor has res_rows rows (*res_rows_dev of them when that pointer is given); an index outside
 * [0, rows) -- the shadow index of an upsampling matrix, a negative one -- adds exact zeros.  It is the fine-level half of a decoder
 * block whose upsampled half Y = x @ W[:C1] was contracted once per coarse row: leaky(skip @ W[C1:] + shift + Y[up[m, 0]]).  Always
 * the tile form (d3f_gemm_x3_plan), whatever d3f_gemm_x3_resident answers; res_idx == NULL is d3f_gemm_x3 itself.  D3F_ERR_ARG on top
 * of d3f_gemm_x3's rules: res_idx without a residual, ld_res_idx < 1, res_rows < 0. */
int d3f_gemm_x3_gres(const float* A, int N1, int lda, int C1, const int* idx, int ld_idx, const float* skip, int lds, int C2,
                     const void* Wx, float* C, int ldc, int M, int N, const float* row_scale, const float* col_scale,
                     const float* col_shift, const float* residual, int ldr, const int* res_idx, int ld_res_idx, int res_rows,
                     const int* res_rows_dev, int leaky, float alpha, void* workspace, size_t workspace_bytes, const int* M_dev,
                     const int* N1_dev, int M_hint, void* stream);

/* d3f_gemm_x3's resident-W form with the NEXT contraction of the network chained in registers (d3feat_amd/csrc/gemm_x3.h):
 *   Y  = act((([ A[idx] | skip ] @ W) * row_scale) * col_scale + col_shift + residual)     [M, N], N = 64 or 128; stored iff C != NULL
 *   C2 = act2((Y @ W2) * col_scale2 + col_shift2)                                          [M, 32] (ldc2 >= 32, a multiple of 4)
 * One launch instead of two; Y is not written (C == NULL) or not read back (C != NULL).  Y is the fp32 value d3f_gemm_x3 stores, split
 * exactly into three bf16 planes for the second product: only the order of the second sum differs from the two-launch form.
 * Wx = d3f_gemm_pack_x3(W); W2x = d3f_gemm_pack_x3_chain(W2 f32[N, 32]), d3f_gemm_x3_packed_bytes(N, 32) bytes: the same planes with the
 * k rows of every 16-block in the order the kernel holds its finished columns.  Always the resident form, whatever M is.
 * d3f_gemm_x3_chain_ok(M, N, K, store_first, M_hint): 1 where d3f_gemm_x3 would take its resident form for the first contraction AND
 * the chained LDS image (W, W2, the output patches when the first output is stored) fits 160 KB -- where the chained launch replaces
 * two launches of the same family; else 0.  D3F_ERR_ARG on top of d3f_gemm_x3's rules: N other than 64 / 128, C2 / W2x missing or not
 * 16-byte aligned, ldc2 < 32 or not a multiple of 4, an LDS image beyond 160 KB. */
int d3f_gemm_pack_x3_chain(const float* W2, int ldb, int K, int N, void* W2x, void* stream);
int d3f_gemm_x3_chain_ok(int M, int N, int K, int store_first, int M_hint);
int d3f_gemm_x3_chain(const float* A, int N1, int lda, int C1, const int* idx, int ld_idx, const float* skip, int lds, int C2cols,
                      const void* Wx, float* C, int ldc, int M, int N, const float* row_scale, const float* col_scale,
                      const float* col_shift, const float* residual, int ldr, int leaky, float alpha, const void* W2x,
                      const float* col_scale2, const float* col_shift2, int leaky2, float alpha2, float* C2, int ldc2,
                      const int* M_dev, const int* N1_dev, void* stream);

/* bf16-operand form of the contractions (BASELINE.json configs[4]: batched inference, bf16 MFMA contraction): the operator of
 * d3f_gemm_f32 / d3f_gemm_upsample_cat_f32 -- A f32[M, C1] (rows in place when idx == NULL, else the gathered rows
 * x'[idx[m,0]], zero row for indices outside [0, N1)), optional second operand skip f32[M, C2], K = C1 + C2, same epilogue --
 * with both operands rounded to bfloat16 (nearest even) and multiplied by v_mfma_f32_32x32x16_bf16, fp32 accumulate.
 * NOT bit-compatible with the fp32 path (2^-9 relative operand rounding); separate tolerance, separate bench configuration.
 * W_packed: d3f_gemm_pack_bf16(W f32[K,N]) -> bf16 [N][Kp], Kp = K rounded up to 32 (2 * N * Kp bytes).
 * C1, C2, lda, lds multiples of 4, 16-byte aligned bases.  workspace >= d3f_gemm_bf16_workspace_bytes(M, N, K, M_hint) -- its
 * OWN sizing function: the bf16 kernel's tile and K split differ from the fp32 kernel's (round-3 header pointed at
 * d3f_gemm_workspace_bytes, which under-sizes the slabs for N <= 32). */
size_t d3f_gemm_bf16_workspace_bytes(int M, int N, int K, int M_hint);
int d3f_gemm_pack_bf16(const float* W, int ldb, int K, int N, void* W_packed, void* stream);
/* a_bf16: A, skip and residual hold bfloat16 values (bf16 feature storage, see d3f_row_positive); c_bf16: C is written as bfloat16.
 * Both 0: the operands are f32 in HBM and only rounded on their way into the multiply (the round-2 form of configs[4]). */
int d3f_gemm_bf16(const void* A, int N1, int lda, int C1, const int* idx, int ld_idx, const void* skip, int lds, int C2,
                  const void* W_packed, void* C, int ldc, int M, int N, const float* row_scale, const float* col_scale,
                  const float* col_shift, const void* residual, int ldr, int leaky, float alpha, void* workspace,
                  size_t workspace_bytes, const int* M_dev, const int* N1_dev, int M_hint, int a_bf16, int c_bf16, void* stream);

/* Stage-0 ingestion: float32 xyz [n,3] out of raw file records already on the device -- a binary PLY
 * vertex element (demo_registration.py:23, datasets/ThreeDMatch.py:348; float or double coordinates at byte offsets
 * off_x/y/z of `stride`-byte records, either byte order) or a KITTI velodyne sweep (datasets/KITTI.py:131, 277-278:
 * stride 16, offsets 0/4/8).  The output feeds d3f_batch_grid_subsample directly. */
int d3f_decode_xyz_records(const void* raw, int n, int stride, int off_x, int off_y, int off_z, int is_f64, int big_endian,
                           float* out, void* stream);

/* =============================================================================================
 * Downstream matching -- what the reference does with the descriptors after the hot path.
 * ============================================================================================= */

/* Nearest descriptor: idx[i] = argmin_j ||A_i - B_j||^2 (lowest j on ties); d2_out (optional) the minimum.
 * No match: a row i without ANY distance below FLT_MAX in the fp32 chain (d = a[c] - b[c]; d2 = fmaf(d, d, d2), c ascending) --
 * Nb == 0, a NaN in A_i, every d2 overflowing -- gets idx[i] = -1 and d2_out[i] = FLT_MAX; a row of B whose distance is NaN or
 * not below FLT_MAX is never the answer.  -1 is what d3f_mutual_matches and d3f_ransac_hypotheses read as "no match".
 * Replaces the argmin over the dense distance matrix of geometric_registration/evaluate.py:17-21 (one direction per call)
 * and the KD-tree feature lookup inside open3d.registration_ransac_based_on_feature_matching (evaluate.py:93-99).
 * A f32[Na,C] (lda), B f32[Nb,C] (ldb), C in {16, 32, 64}. */
size_t d3f_feature_nn_workspace_bytes(int Na);
int d3f_feature_nn(const float* A, int Na, int lda, const float* B, int Nb, int ldb, int C, int* idx, float* d2_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Mutually closest pairs (evaluate.py:21-26 build_correspondence): pairs (i, ab[i]) with ba[ab[i]] == i, ascending i.
 * pairs i32[<= Na, 2]; count_dev i32[1] on the device.  Entries of ab outside [0, Nb) (the -1 of d3f_feature_nn) match nothing;
 * ba may be NULL when Nb == 0.  Rows of pairs from the count on are not written. */
size_t d3f_mutual_matches_workspace_bytes(int Na);
int d3f_mutual_matches(const int* ab, int Na, const int* ba, int Nb, int* pairs, int* count_dev, void* workspace,
                       size_t workspace_bytes, void* stream);

/* RANSAC hypotheses of open3d.registration_ransac_based_on_feature_matching (demo_registration.py:184-192, evaluate.py:
 * 93-99) for iterations it0 .. it0+H-1: sample ransac_n source points (counter-based random numbers: a pure function of
 * (seed, iteration, draw) -- d3f_ransac_draw is the host copy), pair each with nn[.] (its nearest target FEATURE),
 * CorrespondenceCheckerBasedOnEdgeLength(edge_similarity; <= 0: off), rigid fit without scaling
 * (TransformationEstimationPointToPoint(False)), CorrespondenceCheckerBasedOnDistance(checker_distance; <= 0: off).
 * T_out f32[H,12] row-major [R | t]; valid_out u8[H]. */
int d3f_ransac_hypotheses(const float* src, int Ns, const float* tgt, int Nt, const int* nn, int ransac_n,
                          float edge_similarity, float checker_distance, uint64_t seed, uint64_t it0,
                          int H, float* T_out, unsigned char* valid_out, void* stream);
int d3f_ransac_draw(uint64_t seed, uint64_t iteration, int d, int n);

/* Fitness of V hypotheses (Open3D's GetRegistrationResultAndCorrespondences): for every transformed source point the
 * nearest TARGET point strictly inside `radius` (grid built over the target by d3f_neighbor_grid_build, one cloud);
 * count_dev i32[V] inliers, sumd2_dev u64[V] sum of squared distances in 2^-32 units (order independent),
 * nearest_dev i32[Ns] (optional) the correspondences under hypothesis 0. */
int d3f_neighbor_grid_score(const void* grid, size_t grid_bytes, int Nt, const float* src, int Ns, const float* T, int V,
                            float radius, int* count_dev, uint64_t* sumd2_dev, int* nearest_dev, void* stream);

/* Registration of P pairs of keypoint blocks in four launches, whatever P is (geometric_registration/evaluate.py:150-156: every
 * pair id1 < id2 of a scene's fragments): for each pair what d3f_feature_nn (both directions) + d3f_mutual_matches +
 * d3f_ransac_hypotheses + d3f_neighbor_grid_score compute through a host loop, bit for bit, with no host read-back and no
 * host-side decision between the launches -- so the call can be captured in a HIP graph.
 * kp f32[n_blocks, K, ld]: rows [xyz | C-d descriptor | score] in ascending score order (d3f_topk_records' blocks), ld >= C + 4,
 * C in {16, 32, 64}; count_dev i32[n_blocks] rows written per block; pairs_dev i32[P, 2] block indices (source, target; equal
 * indices allowed, an index outside [0, n_blocks) selects an empty block).  Pair (a, b) uses the LAST min(count, num_keypts) rows of
 * each block (evaluate.py:45-50; num_keypts <= 0: all K), Ns source and Nt target rows; Kmax = min(K, num_keypts) <=
 * D3F_PAIRS_KMAX, else D3F_ERR_ARG (larger blocks: the single-pair entry points above).
 *   mutual_count i32[P], mutual (optional) i32[P, Kmax, 2]: the mutually closest descriptor pairs (i, j) in ascending i (evaluate.py:
 *     21-26), padding -1; nearest descriptors are argmin of the fp32 chain of d3f_feature_nn, lowest index on ties.
 *   gt (optional) f32[P, 12], row-major [R | t] taking the TARGET frame into the SOURCE frame; gt_inliers i32[P] (required with gt):
 *     mutual pairs with |s_i - (R t_j + t)| < distance_threshold (evaluate.py:70-77), fp32, d3f_neighbor_grid_score's metric.
 *   RANSAC exactly as d3f_ransac_hypotheses defines iteration it = 0, 1, ... for (seed, it) on the source rows, the target rows and
 *     the source -> target nearest descriptors: the first max_validation valid iterations below max_iteration are scored as
 *     d3f_neighbor_grid_score scores them (nearest target point strictly inside max_correspondence_distance, ties to the lowest
 *     index); the winner has the largest count, then the smallest sumd2, then the smallest iteration.
 *     T_out f32[P, 12], inliers i32[P], sumd2 u64[P] (2^-32 units), best_iteration i32[P] (-1: none), nearest i32[P, Kmax] (the
 *     target row of every source row under the winner, -1 for none and for padding), validations i32[P] (hypotheses scored),
 *     iterations i32[P] (the index after the max_validation-th valid iteration, else max_iteration).
 *     Ns < ransac_n, Nt < ransac_n or max_correspondence_distance <= 0: identity, every count 0, best_iteration -1.
 * 3 <= ransac_n <= 8, 0 <= max_iteration <= 2^30, 1 <= max_validation <= 2^20; every size is checked before the first launch
 * (D3F_ERR_ARG), workspace >= d3f_register_pairs_workspace_bytes(P, K, num_keypts, max_validation), else D3F_ERR_WORKSPACE
 * (64 bytes per pair and validation).  Asynchronous on `stream`, no allocation, no synchronisation. */
size_t d3f_register_pairs_workspace_bytes(int P, int K, int num_keypts, int max_validation);
int d3f_register_pairs(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev, int P,
                       int num_keypts, float max_correspondence_distance, int ransac_n, float edge_similarity,
                       float checker_distance, int max_iteration, int max_validation, uint64_t seed, const float* gt,
                       float distance_threshold, float* T_out, int* inliers, uint64_t* sumd2, int* validations, int* iterations,
                       int* best_iteration, int* mutual_count, int* nearest, int* mutual, int* gt_inliers, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Keypoint repeatability of P pairs of keypoint blocks at n_counts keypoint counts in one launch (repeatability/
 * evaluate_3dmatch_our.py:30-41, evaluate_kitti_our.py:12-23: for each count k the last k rows of both blocks, one block moved with
 * the ground truth in float64, cdist, and the number of TARGET keypoints whose nearest source keypoint is closer than the threshold).
 * kp / count_dev / pairs_dev as d3f_register_pairs takes them, ld >= 3 (only xyz is read; rows in ascending score order); K may
 * exceed D3F_PAIRS_KMAX: only the largest requested count bounds the rows used.
 *   gt_dev f64[P, 12], row-major [R | t].  moved 0: gt takes the TARGET frame into the SOURCE frame and the target rows are moved
 *     (3DMatch, the convention of d3f_register_pairs' gt); moved 1: gt takes the source frame into the target frame and the source
 *     rows are moved (KITTI's `trans`).  In both cases the count runs over the target rows.
 *   threshold_host: ONE double on the host (a pointer, because 0.1f is not 0.1); num_keypts_host: n_counts ints on the host,
 *     strictly ascending, each in 1 .. D3F_PAIRS_KMAX, 1 <= n_counts <= D3F_REPEAT_COUNTS_MAX.  Both are read before the call
 *     returns and reach the kernel by value.
 *   repeat_dev i32[P, n_counts]: with rank 0 the last (best) row of a block, repeat[p, c] = number of target rows of rank < k_c whose
 *     nearest source row of rank < k_c is strictly closer than the threshold.  The blocks are in score order, so the row sets of the
 *     counts are nested and one walk over the sources in rank order, with a test at every count, serves all of them.  A block
 *     shorter than k_c contributes the rows it has, a pair without source rows counts 0, an index outside [0, n_blocks) selects
 *     no rows.  The reference's ratio is repeat / k_c (k_c itself, whatever the blocks hold).
 *   totals_dev (optional) i64[n_counts]: the sums of repeat over the P pairs (a second launch; integer, order independent).
 * Arithmetic in float64 with every operation rounded on its own: rows widened f32 -> f64, q_r = ((R[r,0] x + R[r,1] y) + R[r,2] z)
 * + t[r], d2 = (dx dx + dy dy) + dz dz, the test d2 < threshold * threshold (the rounded product).
 * D3F_ERR_ARG before anything touches the device: P < 0, K < 1, ld < 3, n_counts or a count out of range, counts not strictly
 * ascending, moved not 0 or 1, a NaN or non-positive threshold, a NULL pointer other than totals_dev; P == 0 is D3F_OK.
 * Asynchronous on `stream`, no workspace, no allocation, no synchronisation, no memset: capturable. */
int d3f_repeatability_pairs(const float* kp, int n_blocks, int K, int ld, const int* count_dev, const int* pairs_dev, int P,
                            const double* gt_dev, int moved, const double* threshold_host, const int* num_keypts_host,
                            int n_counts, int* repeat_dev, int64_t* totals_dev, void* stream);

/* Feature-matching recall of P pairs of keypoint blocks at n_counts keypoint counts in two launches, whatever P and the counts are
 * (geometric_registration/evaluate.py:45-50, 67-82, whose num_keypts is edited by hand to sweep 5000 / 2500 / 1000 / 500 / 250): per
 * pair and count k what d3f_register_pairs returns as mutual_count and gt_inliers for num_keypts = k, bit for bit, without its
 * RANSAC and without its limit of D3F_PAIRS_KMAX rows.  No memset, no atomics between workgroups, no read-back: capturable.
 * kp / count_dev / pairs_dev as d3f_register_pairs takes them (rows [xyz | C-d descriptor | ...] in ascending score order, an index
 * outside [0, n_blocks) selects no rows), C in {16, 32, 64}, ld >= C + 3; K may exceed every count.
 *   num_keypts_host: n_counts ints on the host, strictly ascending, each in 1 .. D3F_MATCH_KMAX, 1 <= n_counts <=
 *     D3F_REPEAT_COUNTS_MAX; read before the call returns.  Count k uses the LAST min(count, k) rows of each block.
 *   nearest descriptors: argmin of the fp32 chain of d3f_feature_nn (d = a[c] - b[c]; d2 = fmaf(d, d, d2), c ascending), the lowest
 *     row on ties, in both directions.  The blocks are in score order, so the rows of the counts are nested prefixes in rank (rank 0 =
 *     the last row) and the nearest row at count k is a running minimum of one walk in rank order: one pass over the largest count
 *     serves every count.
 *   mutual_count i32[P, n_counts]: source rows i with nn_ts[nn_st[i]] == i (evaluate.py:21-26).
 *   gt (optional) f32[P, 12], row-major [R | t] taking the TARGET frame into the SOURCE frame; gt_inliers i32[P, n_counts], NULL if
 *     and only if gt is NULL: the mutual pairs with |s_i - (R t_j + t)|^2 < distance_threshold * distance_threshold (evaluate.py:
 *     70-77), fp32, the metric of d3f_register_pairs.
 * A block shorter than a count contributes the rows it has; a pair without rows on either side counts 0.
 * workspace >= d3f_match_pairs_workspace_bytes(P, num_keypts_host, n_counts): 8 * sum of the counts bytes per pair (the nearest rank
 * of every row of every count, both directions), else D3F_ERR_WORKSPACE; the function returns 0 for arguments d3f_match_pairs refuses.
 * D3F_ERR_ARG before anything touches the device: P < 0, n_blocks or K < 1, C not 16 / 32 / 64, ld < C + 3, n_counts or a count out of
 * range, counts not strictly ascending, a NaN threshold, exactly one of gt / gt_inliers NULL, another NULL pointer with P > 0; P == 0
 * is D3F_OK without a launch.  Asynchronous on `stream`, no allocation, no synchronisation. */
size_t d3f_match_pairs_workspace_bytes(int P, const int* num_keypts_host, int n_counts);
int d3f_match_pairs(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev, int P,
                    const float* gt, float distance_threshold, const int* num_keypts_host, int n_counts, int* mutual_count,
                    int* gt_inliers, void* workspace, size_t workspace_bytes, void* stream);

/* RANSAC registration of P pairs of keypoint blocks at n_counts keypoint counts in one call (geometric_registration/evaluate.py:45-50,
 * 67-99, whose num_keypts is edited by hand to sweep 5000 / 2500 / 1000 / 500 / 250): per pair p and count k_c everything
 * d3f_register_pairs computes for num_keypts = k_c, bit for bit, without its limit of D3F_PAIRS_KMAX rows -- no kernel of this call
 * keeps a block in LDS, the nearest target POINT comes from one cell grid over all blocks.  Twelve launches whatever P and the
 * counts are, no allocation, no read-back, no host decision between the launches, no memset: capturable on one stream.
 * kp / count_dev / pairs_dev as d3f_register_pairs takes them (rows [xyz | C-d descriptor | score] in ascending score order, C in
 * {16, 32, 64}, ld >= C + 4, an index outside [0, n_blocks) selects an empty block), n_blocks <= D3F_MAX_BATCH; K may exceed every count.
 *   num_keypts_host: n_counts ints on the host, strictly ascending, each in 1 .. D3F_MATCH_KMAX, 1 <= n_counts <=
 *     D3F_REPEAT_COUNTS_MAX; read before the call returns.  Count k_c uses the LAST min(count, k_c) rows of each block, Ns source and
 *     Nt target rows, numbered from 0 inside those rows (the numbering of d3f_register_pairs at num_keypts = k_c).
 *   mutual_count, gt_inliers i32[P, n_counts]: what d3f_match_pairs writes for the same counts; gt (optional) f32[P, 12] row-major
 *     [R | t] taking the TARGET frame into the SOURCE frame, distance_threshold as there; gt_inliers is required with gt.
 *   RANSAC per (pair, count) exactly as d3f_ransac_hypotheses defines iteration it = 0, 1, ... for (seed, it) on the Ns source rows,
 *     the Nt target rows and the source -> target nearest descriptors of that count (the draws of d3f_ransac_draw run over Ns): the
 *     first max_validation valid iterations below max_iteration are scored as d3f_neighbor_grid_score scores them (nearest target
 *     row strictly inside max_correspondence_distance by (d2, row), the metric never contracted); the winner has the largest count,
 *     then the smallest sumd2, then the smallest iteration.
 *     T_out f32[P, n_counts, 12], inliers / validations / iterations / best_iteration i32[P, n_counts] (best_iteration -1: none),
 *     sumd2 u64[P, n_counts] (2^-32 units), nearest (optional) i32[P, sum of the counts]: entry off_c + i, off_c = k_0 + ... + k_{c-1},
 *     is the target row of source row i under the winner of count c, -1 for none and for padding (i >= Ns).
 *     Ns < ransac_n, Nt < ransac_n or max_correspondence_distance <= 0: identity, every count 0, best_iteration -1.
 * ONE GRID FOR EVERY COUNT: the grid holds the last min(count, k_max) rows of every block, k_max the largest count.  At count k_c the
 * rows of a block are the records with index >= min(count, k_max) - min(count, k_c); the others are skipped, and a constant shift of
 * the index keeps the (d2, index) order, so the minimum over the kept records is the row d3f_register_pairs finds.
 * D3F_ERR_ARG before anything touches the device: n_blocks > D3F_MAX_BATCH, n_counts or a count out of range, counts not strictly
 * ascending, and every size d3f_register_pairs refuses (P < 0, n_blocks or K < 1, C not 16 / 32 / 64, ld < C + 4, ransac_n outside
 * 3 .. 8, max_iteration outside 0 .. 2^30, max_validation outside 1 .. 2^20, a NaN distance, a NULL pointer other than gt, gt_inliers
 * without gt and nearest); P == 0 is D3F_OK without a launch.  workspace >= d3f_register_pairs_counts_workspace_bytes(...), else
 * D3F_ERR_WORKSPACE: 64 bytes per pair, count and validation, 12 bytes per pair and row of every count, and the stack and grid of
 * n_blocks * min(K, k_max) points; the function returns 0 for sizes the call refuses.  Asynchronous on `stream`. */
size_t d3f_register_pairs_counts_workspace_bytes(int P, int n_blocks, int K, const int* num_keypts_host, int n_counts,
                                                 int max_validation);
int d3f_register_pairs_counts(const float* kp, int n_blocks, int K, int ld, int C, const int* count_dev, const int* pairs_dev, int P,
                              const int* num_keypts_host, int n_counts, float max_correspondence_distance, int ransac_n,
                              float edge_similarity, float checker_distance, int max_iteration, int max_validation, uint64_t seed,
                              const float* gt, float distance_threshold, float* T_out, int* inliers, uint64_t* sumd2,
                              int* validations, int* iterations, int* best_iteration, int* mutual_count, int* gt_inliers,
                              int* nearest, void* workspace, size_t workspace_bytes, void* stream);

/* Overlap of P pairs of a scene's fragments in two launches, whatever P is (datasets/cal_overlap.py:78-126: for every pair the
 * nearest point of the second fragment for each point of the first, the matches closer than the voxel size, their share of the
 * first fragment): what a host loop of one d3f_neighbor_grid_build per target and one d3f_neighbor_grid_score(V = 1, identity) per
 * pair computes, bit for bit, with no host read-back and no host-side decision -- so the call can be captured in a HIP graph.
 *   grid: built by d3f_neighbor_grid_build over the N stacked points of B fragments (s_lens_dev = their lengths), all in ONE common
 *     frame, with radius >= threshold (the caller's contract, as for d3f_neighbor_grid_search).  It is the only point input: a built
 *     grid holds every fragment's points in the fragment's own cell order with their indices, and those records are the queries.
 *   pairs_dev i32[P, 2]: (source a, target b) fragment indices, read on the device; a == b and repeated pairs are allowed.
 *   count_dev i32[P], OVERWRITTEN: points of a whose nearest point of b is strictly inside the threshold; -1 for a pair with an
 *     index outside [0, B) (nothing is read for it, its nearest row is all -1).  The reference's ratio is count / len_a.
 *   nearest_dev (optional) i32[P, ld_nearest]: entry [p, i] = index INSIDE fragment b (cv2's trainIdx) of the nearest point of b to
 *     point i of a (i its index inside a, not the cell order), -1: none inside the threshold; entries from len_a on are -1; a row
 *     shorter than its source fragment receives the first ld_nearest entries only (nothing is written past it).
 * The metric of every search here: r2 = threshold * threshold in fp32, d2 = (dx*dx + dy*dy) + dz*dz with dx = q - s, every
 * operation rounded to fp32 and never contracted, a match iff d2 < r2, the nearest point the minimum by (d2, index in b).
 * D3F_ERR_ARG before anything touches the device: a negative size, B outside 1 .. D3F_MAX_BATCH, a threshold that is not positive
 * and finite, grid / pairs_dev / count_dev NULL with P > 0; a grid_bytes below d3f_neighbor_grid_bytes(N, B): D3F_ERR_WORKSPACE;
 * P == 0 is D3F_OK without a launch.  Asynchronous on `stream`, no workspace, no allocation, no synchronisation. */
int d3f_overlap_pairs(const void* grid, size_t grid_bytes, int N, int B, const int* pairs_dev, int P, float threshold,
                      int* count_dev, int* nearest_dev, int ld_nearest, void* stream);

/* Validation figures of P pairs in three launches, whatever P is (models/KPFCNN_model.py:131-186 with utils/loss.py of the reference:
 * what its model class evaluates per validation pair, and utils/trainer.py:442-452, 467-471: the means over a split).  The forward; d3f_loss_gradients adds the gradient.
 * Pair p is the stack [anchor; positive] held by rows row0_dev[p] .. row0_dev[p + 1] of three row arrays, each a base pointer and a
 * leading dimension in floats, so that column views of one block of [xyz | descriptor | score] records need no copy:
 *   desc f32[n_rows, ldd] (C = 16 / 32 / 64 columns read), score f32[n_rows, lds] (one column), points f32[n_rows, ldp] (three).
 *   row0_dev i32[P + 1], anc_dev / pos_dev i32[P, ld_idx]: n_dev[p] index pairs (ai, pi) into the pair's rows, the positive's already
 *   shifted by the anchor's length as the reference feeds them; repeated indices are allowed.  All read on the device.
 * With m = neg_margin, q = pos_margin, L = log_scale, r = safe_radius, n = n_dev[p], in fp32:
 *   D[i,j]  = sqrt(sum_c (f[ai[i],c] - f[pi[j],c])^2 + 1e-12), the sum an fmaf chain over ascending c of the differences (loss.cdist;
 *             one arithmetic for every entry: equal index pairs give equal bits);
 *   KD[i,j] = sqrt(((dx dx + dy dy) + dz dz) + 1e-12) between the points of ai[i] and ai[j], never contracted (KPFCNN_model.py:131-132);
 *   FN[i,j] = KD[i,j] < r and i != j;   fp_i = D[i,i];   cn_i = min_j (D[i,j] + 1e5 [i == j]) (FN not applied: loss.py:151);
 *   z[i,j]  = 0 if (i == j or FN[i,j] or D[i,j] >= m) else (L (m - D[i,j])) (m - D[i,j]);   lse_i = log sum_j exp z[i,j] -- a masked
 *             entry contributes exp(0), as the reference's 1e8 terms make it.
 * values f32[P, 8]: [0] circle = mean_i softplus(L (fp_i - q) + lse_i) / L (softplus with the shortcuts of d3f_detect_head),
 *   [1] contrastive = mean_i (max(fp_i - q, 0) + max(m - cn_i, 0)), [2] det = det_loss_weight * mean_i (fp_i - cn_i) ((s[ai[i]] +
 *   s[pi[i]]) + 1e-6), constant 0 for a zero weight, [3] accuracy = #{i: fp_i - cn_i <= 0} / n, [4] d_pos = mean_i fp_i,
 *   [5] d_neg = (mean over all n n entries of D [i != j and not FN]) n / (n - 1) -- NaN at n = 1, as the reference --,
 *   [6] the number of accurate rows, [7] n.  D, KD and the exponentials are fp32; the per-row terms and the means are float64
 *   in a fixed order and each figure is rounded to fp32 once.
 * A pair with n == 0 or 2 n < keypts_num (KPFCNN_model.py:172-186) gets (0, 0, 0, -1, 0, 0 | 0, n).  So does one with n outside
 * 0 .. min(ld_idx, D3F_VALIDATION_NMAX) (status_dev[p] = 2) or with an index outside its rows, or offsets outside 0 .. n_rows
 * (status_dev[p] = 1): nothing is read through such an index.  status_dev[p] = 0 otherwise.
 * sums_dev f64[6] / counts_dev i64[6]: per figure [0..5] the sum over the pairs where it is != 0 (accuracy: > 0) and their number --
 * the lists the trainer averages.
 * No memset, no atomics, no read-back, fixed summation orders (two calls give equal bits): capturable.
 * workspace >= d3f_validation_pairs_workspace_bytes(P, ld_idx): 32 bytes per pair and index of min(ld_idx, D3F_VALIDATION_NMAX)
 * rounded up to 64, else D3F_ERR_WORKSPACE; the function returns 0 for sizes the call refuses.
 * D3F_ERR_ARG before anything touches the device: P < 0, C not 16 / 32 / 64, ldd < C, lds < 1, ldp < 3, n_rows < 0, ld_idx < 1,
 * keypts_num < 0, a NaN parameter, neg_margin or log_scale not positive, log_scale * neg_margin^2 > 80 (exp would leave fp32 without
 * a running maximum), a NULL pointer (with P == 0 only sums_dev and counts_dev are needed: they are zeroed by one launch).
 * Asynchronous on `stream`, no allocation, no synchronisation. */
size_t d3f_validation_pairs_workspace_bytes(int P, int ld_idx);
int d3f_validation_pairs(const float* desc, int ldd, int C, const float* score, int lds, const float* points, int ldp, int n_rows,
                         const int* row0_dev, const int* anc_dev, const int* pos_dev, int ld_idx, const int* n_dev, int P,
                         float safe_radius, int keypts_num, float det_loss_weight, float pos_margin, float neg_margin,
                         float log_scale, float* values, int* status_dev, double* sums_dev, int64_t* counts_dev, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Loss gradients of P training pairs in five launches, whatever P is: the gradient of desc_loss + det_loss (models/KPFCNN_model.py:
 * 143-191 with utils/loss.py of the reference; the regularisation term of :188-191 depends on the weights only and is not part of it)
 * with respect to the rows of desc and score, together with the forward's values and status.  The inputs, the skip rule, the status
 * and D, KD, FN, fp, cn, z, lse are those of d3f_validation_pairs, computed by the same kernels: values / status_dev are bit-equal to
 * what that call writes.  contrastive = 0: desc_loss is the circle loss (what the model class uses); 1: the contrastive loss.
 * With n = n_dev[p], q = pos_margin, m = neg_margin, L = log_scale, w = det_loss_weight, and for row i
 *   T_i      = the columns j whose entry D[i,j] + 1e5 [i == j] is bit-equal to cn_i; share[i,j] = [j in T_i] / |T_i| (the equal split
 *              of reduce_min's gradient; index pairs drawn with replacement make such ties the rule);
 *   sab_i    = (s[ai[i]] + s[pi[i]]) + 1e-6;   live[i,j] = i != j and not FN[i,j] and D[i,j] < m;
 *   sg_i     = sigmoid(L (fp_i - q) + lse_i),
 * G = d loss / d D is the sum of
 *   circle       G[i,i] += sg_i / n;   where live: G[i,j] -= (sg_i / n) exp(z[i,j] - lse_i) (m - D[i,j])   (the factor max(0, m - D) of
 *                loss.py:176 is under stop_gradient: dz/dD = -L (m - D), and the 1 / L of :179 cancels the L)
 *   contrastive  G[i,i] += [fp_i - q >= 0] / n;   G[i,j] -= share[i,j] [m - cn_i >= 0] / n   (tf.maximum passes the gradient to its
 *                first argument on equality)
 *   det, w != 0  G[i,i] += w sab_i / n;   G[i,j] -= share[i,j] w sab_i / n   (the diagonal column too when n = 1: the two cancel)
 * and with a_i = f[ai[i]], p_j = f[pi[j]]:
 *   d a_i = sum_j (G[i,j] / D[i,j]) (a_i - p_j);   d p_j = sum_i (G[i,j] / D[i,j]) (p_j - a_i);
 *   the entry i adds w (fp_i - cn_i) / n to the score gradient of ai[i] and of pi[i].
 * grad_desc f32[n_rows, ldg] (C columns written) and grad_score f32[n_rows, ldgs] (one column): row r of a pair receives the sum over
 * the list entries that name it (tf.gather's gradient: duplicates add, a row may be named by both lists), the anchor entries in list
 * order, then the positive entries in list order.  EVERY word of the C + 1 columns of all n_rows rows is written: zeros for the rows
 * no list names, for a pair under the skip rule and for a pair whose status is not 0; the buffers need not be cleared, and may be
 * column views of a record block.  The pairs' rows must not overlap (they cannot when row0_dev is non-decreasing).
 * D, KD, the exponentials and the sums over j and i are fp32 (per wave an fmaf chain over ascending columns, the four waves of a
 * 64-entry tile added in wave order); the four numbers of a row that G is made of are float64, rounded once.  n x n is never stored.
 * No memset, no atomics, no read-back; every sum runs in an order that depends on (n, P, the lists) only: two calls give equal bits,
 * and a call of P pairs gives the bits of P calls of one pair.  Capturable.
 * workspace >= d3f_loss_gradients_workspace_bytes(P, ld_idx, C): (52 + 8 C) bytes per pair and index of min(ld_idx,
 * D3F_VALIDATION_NMAX) rounded up to 64, else D3F_ERR_WORKSPACE; the function returns 0 for sizes the call refuses.
 * D3F_ERR_ARG before anything touches the device: what d3f_validation_pairs refuses, ldg < C, ldgs < 1, contrastive not 0 / 1, a NULL
 * pointer (with P == 0 only the two outputs are needed: they are zeroed by one launch).
 * Asynchronous on `stream`, no allocation, no synchronisation. */
size_t d3f_loss_gradients_workspace_bytes(int P, int ld_idx, int C);
int d3f_loss_gradients(const float* desc, int ldd, int C, const float* score, int lds, const float* points, int ldp, int n_rows,
                       const int* row0_dev, const int* anc_dev, const int* pos_dev, int ld_idx, const int* n_dev, int P,
                       float safe_radius, int keypts_num, float det_loss_weight, float pos_margin, float neg_margin, float log_scale,
                       int contrastive, float* grad_desc, int ldg, float* grad_score, int ldgs, float* values, int* status_dev,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The transposed neighbour table: for every row, the edges that name it, in a fixed order.  The scatter of every backward through a
 * neighbour gather (the head's neighbour mean below; a KPConv's support features) becomes a gather in a defined order through it.
 *   idx i32[N, ld_idx] (K columns), lens_dev i32[B]: n = min(N, sum(lens_dev)) is read on the device, N is the capacity.
 *   Edge e = i * K + k (i < n, k < K) is VALID when 0 <= idx[i, k] < n -- the head's shadow rule: negative entries, n, anything above n.
 *   start i32[N + 1]: start[j] .. start[j + 1] is row j's segment of `edges`; every start[j] with j >= n is the number of valid edges.
 *   edges i32[N * K]: row j's segment holds the valid edges with idx[i, k] == j in ascending e (a row that names j twice appears
 *     twice); words at or beyond the number of valid edges are left alone.
 * The table IS np.argsort(keys, kind="stable") over the valid edges, integer for integer.  Built by a stable radix sort of (named row,
 * e) and one bisection per row: nine launches whatever N, K and B are, no atomic on global memory, no memset, no read-back; capturable.
 * D3F_ERR_ARG before anything touches the device: N < 0, K < 0, N * K > 2^31 - 8192 (the sort addresses whole 8192-slot tiles with
 * 32-bit positions), ld_idx < K, B < 1 or > D3F_MAX_BATCH, a NULL start or lens_dev, a NULL edges or idx with N * K > 0.
 * workspace >= d3f_neighbor_transpose_workspace_bytes(N, K) (about 16 bytes per slot of idx), else D3F_ERR_WORKSPACE; the function
 * returns 0 for sizes the call refuses. */
size_t d3f_neighbor_transpose_workspace_bytes(int N, int K);
int d3f_neighbor_transpose(const int* idx, int N, int ld_idx, int K, const int* lens_dev, int B, int* start, int* edges, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Backward of d3f_detect_head (models/D3Feat.py:65-115): from the gradients with respect to the rows of desc (gdesc f32[n, ldg], C
 * columns) and of score (gscore f32[n, ldgs], one column) -- either may be NULL and counts as zero; both may be column views of a
 * record block, as d3f_loss_gradients writes them -- to gx f32[n, ldgx], the gradient with respect to x.  x, idx, lens_dev,
 * include_zero_dev, stack_group, B and the capacity N as in d3f_detect_head, C <= 128; start / edges: the table
 * d3f_neighbor_transpose made of the same idx.  Every word of the first n rows' C columns of gx is written; rows at or beyond n are
 * left alone.
 * With the forward's quantities -- m_b, den_b = m_b + 1e-6, y = x / den_b, the valid neighbours, num_i = max(#{valid neighbours with
 * a non-zero row sum}, 1) (a constant: count_nonzero has no gradient), mean = S / num, d = y - mean, alpha = softplus(d) (with the
 * forward's shortcuts), w_i = max_c y, beta = y / (1e-6 + w_i), a = alpha beta, s_i = max_c a --
 *   1. T_i = {c : a[i,c] == s_i}, bit-equal in this kernel's arithmetic;  ga[i,c] = gscore_i / |T_i| on T_i, else 0 (the equal split of
 *      reduce_max, the rule d3f_loss_gradients uses for reduce_min);
 *   2. g_d = ga beta sigmoid(d);  g_beta = ga alpha;
 *   3. gy[i,c] = g_d[i,c] + g_beta[i,c] / (1e-6 + w_i), and on W_i = {c : y[i,c] == w_i} plus gw_i / |W_i| with
 *      gw_i = -sum_c g_beta[i,c] y[i,c] / (1e-6 + w_i)^2;
 *   4. gS[i,:] = -g_d[i,:] / num_i;  gy[j,:] += sum over row j's segment of `edges`, in ascending e, of gS[e / K, :];
 *   5. gx[i,c] = gy[i,c] / den_b;
 *   6. per cloud gden_b = -sum_{i in b, c} gy[i,c] y[i,c] / den_b, split equally among the entries that tie for m_b and added to gx
 *      there: the real entries with x == m_b, plus pads_b * C zeros when pads_b > 0 and m_b == 0 -- each shadow slot of the cloud's row
 *      of in_batches gathers a whole zero ROW of C entries.  pads_b (datasets/common.py:453-496) = longest - len_b, plus 1 when all
 *      clouds of the stack (of the stack_group) are equally long; when include_zero_dev is given its entry is read as that number
 *      (the forward keeps reading it as a flag);
 *   7. with ss = sum_c x^2 and desc = x rsqrt(ss):  gx += rsqrt(ss) (gdesc - desc (desc . gdesc)) where ss >= 1e-10, else
 *      gx += gdesc rsqrt(1e-10).
 * Summation orders: the segment sum of 4 is ONE fp32 chain per channel, started at zero, in ascending e, added to the row's own
 * terms at the end.  The sum of 6 is float64: per row, lane l of 32 adds gy y of channels l, l + 32, ... in ascending order and the 32
 * lane sums are combined by xor-butterfly over 16, 8, 4, 2, 1; per cloud, thread t of 256 adds the rows t, t + 256, ... counted from
 * the cloud's first row, in ascending order, and the 256 sums are halved (sum[t] += sum[t + o], o = 128, 64, ..., 1): a tree that
 * depends on the cloud's own length only.  The channel sums of 3 and 7 are the fp32 xor-butterfly of the forward.  No float atomic,
 * and no workgroup waits for another: two calls give equal bits, and a concatenation of independent stacks under stack_group gives
 * the bits of the stacks run alone provided neighbours stay inside their own cloud (the head's contract).
 * Six launches (the forward's two per-cloud maximum launches, then: per-row terms, segment gather, per-cloud tree, finish); all sizes
 * are read on the device; no memset, no read-back; capturable.
 * D3F_ERR_ARG before anything touches the device: what d3f_detect_head refuses, N * K > 2^31 - 8192 (no table exists beyond),
 * ldgx < C, ldg < C (gdesc given), ldgs < 1 (gscore given), a NULL x, lens_dev, start or gx, a NULL idx or edges with K > 0 (N == 0 is D3F_OK).  workspace >=
 * d3f_detect_head_backward_workspace_bytes(N, C, B): (8 C + 12) bytes per row of capacity, else D3F_ERR_WORKSPACE; the function
 * returns 0 for sizes the call refuses. */
size_t d3f_detect_head_backward_workspace_bytes(int N, int C, int B);
int d3f_detect_head_backward(const float* x, int N, int ldx, int C, const int* idx, int ld_idx, int K, const int* lens_dev,
                             const int* include_zero_dev, int stack_group, int B, const int* start, const int* edges,
                             const float* gdesc, int ldg, const float* gscore, int ldgs, float* gx, int ldgx, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The rectangular transposed table: Nq query rows name Ns support rows (a strided KPConv; d3f_neighbor_transpose is the square case
 * whose row count comes from stack lengths).  Nq_dev / Ns_dev (device i32, may be NULL): nq = min(Nq, *Nq_dev), ns = min(Ns, *Ns_dev),
 * as in the KPConv entry points; Nq and Ns are capacities.
 *   idx i32[Nq, ld_idx] (K columns).  Edge e = i * K + k (i < nq) is VALID when 0 <= idx[i, k] < ns.  Keys are 0 .. ns.
 *   start i32[Ns + 1]: row j's segment; every start[j] with j >= ns is the number of valid edges.
 *   edges i32[Nq * K]: as d3f_neighbor_transpose; words at or beyond the number of valid edges are left alone.
 * The same stable sort, the same nine launches and the same finishing kernel as d3f_neighbor_transpose.  D3F_ERR_ARG before anything
 * touches the device: Nq < 0, Ns < 0, K < 0, Nq * K > 2^31 - 8192, ld_idx < K, a NULL start, a NULL edges or idx with Nq * K > 0.
 * workspace >= d3f_neighbor_transpose_workspace_bytes(Nq, K), else D3F_ERR_WORKSPACE. */
int d3f_neighbor_transpose_qs(const int* idx, int Nq, int ld_idx, int K, const int* Nq_dev, int Ns, const int* Ns_dev, int* start,
                              int* edges, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the rigid KPConv (kernels/convolution_ops.py:161-255): from gout f32[nq, Cout] (leading dimension ldg), the gradient
 * with respect to the output of KPConv_ops, to gf f32[ns, Cin] (ldgf), the gradient with respect to the support feature rows, and
 * gW f32[num_kp * Cin, Cout], the gradient with respect to K_values.  Either output may be NULL when it is not wanted.  The gather
 * group (q .. Cin) and the kernel-point group (kp_host .. aggregation) are d3f_kpconv_aggregate's; W f32[num_kp * Cin, Cout] is
 * K_values; start / edges: the table d3f_neighbor_transpose_qs made of the same idx; Nq_dev / Ns_dev / q_order as in the forward.
 * Every influence, aggregation mode, channel count and num_kp the forward takes; queries may differ from supports (strided layers).
 * fp32 feature rows only: feat_bf16 != 0 is D3F_ERR_ARG.
 * Forward, as d3f_kpconv_aggregate documents it: h[n,k,p] is the influence of kernel point p on the pair (n, k) -- zero for shadow
 * slots (idx[n,k] outside [0, ns)), masked to the arg-min kernel point under 'closest' --
 *   wf[n,p,c] = sum_k h[n,k,p] f[idx[n,k], c]      cnt_n = max(#{k valid : row_pos[idx[n,k]]}, 1)
 *   out[n,o]  = (sum_{p,c} wf[n,p,c] W[p,c,o]) / cnt_n
 * Backward:
 *   g[n,o]     = gout[n,o] / cnt_n (the rounded product gout * inv_cnt, inv_cnt = 1 / cnt_n as the forward computes it).  The count
 *                has no gradient (tf.greater and the cast have none); the kernel points are trainable=False and the points are inputs,
 *                so h is a constant of the backward; one_hot and argmin have no gradient either.
 *   gW[p,c,o]  = sum_{n < nq} wf[n,p,c] g[n,o]
 *   gwf[n,p,c] = sum_o g[n,o] W[p,c,o]
 *   msg[e,c]   = sum_p h[n,k,p] gwf[n,p,c]   for the edge e = n K + k
 *   gf[j,c]    = sum of msg[e,c] over row j's segment of the transposed table, in ascending e
 * Summation orders: msg is ONE chain of fp32 fused multiply-adds over ascending p, started at zero.  The segment sum is ONE fp32 chain
 * per channel in ascending e, started at zero (the rule of d3f_detect_head_backward step 4).  gW is summed over slices of consecutive
 * query rows; the slice length depends on the CAPACITY Nq only -- 256 rows, doubled until at most 128 slices cover Nq -- never on
 * the device or its occupancy; inside a slice the matrix instruction (v_mfma_f32_32x32x2_f32) adds pairs of rows to one accumulator
 * in ascending row order; the slice partials are added in ascending slice order, started at zero.  gwf is d3f_gemm_f32 on g (a
 * contiguous copy, so ldg does not matter) and a transposed copy of W: fixed for given shapes.  No float atomic, no workgroup waits for another: two
 * calls give equal bits in both outputs, and a row of gf depends on its own segment only.
 * Every word of the first ns rows of gf (Cin columns) and of all of gW is written; rows that nobody names get exact zeros; gf rows at
 * or beyond ns are left alone.  gout, q and idx rows at or beyond nq are never read, s and f rows at or beyond ns neither, and no
 * index outside [0, ns) forms an address.  The table is range-checked, never trusted.
 * Launches: d3f_row_positive and d3f_kpconv_aggregate as they are (wf, inv_cnt); g; for gW the slice contraction and the kernel that
 * adds the partials; for gf the transposed copy of W, d3f_gemm_f32 (gwf overwrites wf), the message kernel (the forward's neighbour
 * loop turned round: Cin = 4 .. 1024 powers of two on the forward's lanes-per-query ladder, any other Cin one thread per (query,
 * channel)) and the segment gather.  All sizes are read on the device; no read-back, no memset, no atomic on global memory;
 * capturable.  Nq == 0 or K == 0 is D3F_OK with gf and gW written as zeros.
 * D3F_ERR_ARG before anything touches the device: a negative size, Cin or Cout < 1 or > 2^20, ld_idx < K, ldf < Cin, ldg < Cout,
 * ldgf < Cin (gf given), num_kp outside 1 .. 15, an unknown influence or aggregation, KP_extent <= 0, Nq * K > 2^31 - 8192, both
 * outputs NULL, Ns == 0 with Nq > 0, a NULL kp_host or W, a NULL start with gf given, a NULL q, s, f or gout with Nq > 0, a NULL idx
 * (or edges, gf given) with Nq * K > 0.
 * workspace >= d3f_kpconv_backward_workspace_bytes(Nq, Ns, K, Cin, Cout, num_kp): wf / gwf (Nq num_kp Cin floats), msg (Nq K Cin),
 * the gW partials (ceil(Nq / slice) num_kp Cin Cout), g (Nq Cout), inv_cnt (Nq), the row flags (Ns bytes), the transposed W and the contraction's
 * own workspace; else D3F_ERR_WORKSPACE.  The function returns 0 for sizes the call refuses. */
size_t d3f_kpconv_backward_workspace_bytes(int Nq, int Ns, int K, int Cin, int Cout, int num_kp);
int d3f_kpconv_backward(const float* q, int Nq, const float* s, int Ns, const int* idx, int ld_idx, int K, const void* f, int ldf,
                        int Cin, const float* kp_host, int num_kp, float KP_extent, int influence, int aggregation, const float* W,
                        const float* gout, int ldg, int Cout, const int* start, const int* edges, float* gf, int ldgf, float* gW,
                        const int* Nq_dev, const int* Ns_dev, const int* q_order, int feat_bf16, void* workspace,
                        size_t workspace_bytes, void* stream);

/* out f32[Ca, Cb] = A^T B over the first m = min(M, *M_dev) rows (M_dev may be NULL: m = M): A f32[m, Ca] (lda), B f32[m, Cb] (ldb).  The
 * backward of a unary convolution y = x W with respect to W is gW = x^T gy.  A second entry onto the two kernels of d3f_kpconv_backward's
 * gW, so the order is the same: slices of consecutive rows whose length depends on the CAPACITY M only (256 rows, doubled until at most
 * 128 slices cover M); inside a slice the matrix instruction (v_mfma_f32_32x32x2_f32) adds pairs of rows to one accumulator in ascending
 * row order; the slice partials are added in ascending slice order, started at zero.  On contiguous operands the bits are those of
 * d3f_kpconv_backward's gW for the same rows.  Two launches, no atomic, no read-back, capturable; every word of out is written (m == 0:
 * zeros); rows at or beyond m are never read.  D3F_ERR_ARG: a negative M, Ca or Cb < 1 or > 2^20, lda < Ca, ldb < Cb, a NULL out, a
 * NULL A or B with M > 0.  workspace >= d3f_gemm_tn_workspace_bytes(M, Ca, Cb) (the slice partials), else D3F_ERR_WORKSPACE. */
size_t d3f_gemm_tn_workspace_bytes(int M, int Ca, int Cb);
int d3f_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, int M, int Ca, int Cb, float* out, const int* M_dev,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Batch normalisation in TRAINING mode with the epilogue of a block, and its backward: tf.layers.batch_normalization(training=True) of
 * models/network_blocks.py:149-165 on a rank-2 input (the non-fused path of TF 1.x), then the residual add and leaky_relu (:185-186).
 * x f32[n, C] (ldx), n = min(M, *M_dev) (M_dev may be NULL: n = M); M is the capacity.  The statistics are taken over the n real rows of
 * the stacked batch, all clouds together.
 * Forward:
 *   mean_c = (1/n) sum_i x[i,c]
 *   var_c  = (1/n) sum_i (x[i,c] - mean_c)^2      two passes as tf.nn.moments, biased (no Bessel correction); the deviation is taken
 *                                                 from the float64 mean, so a constant column has var == 0 exactly
 *   rstd_c = 1 / sqrt(var_c + eps)                in float64, then rounded; rstd f32[C] is an output
 *   mean f32[2, C] is an output in two parts: mean[0, c] the float64 mean rounded to fp32 (the batch mean of the moving update),
 *             mean[1, c] the rounded remainder (float64 mean - mean[0, c]).  Both passes take x - mean as (x - mean[0]) - mean[1]: a
 *             column whose spread is far below its mean (mean 1e3, spread 1e-2) would otherwise carry the rounding of its mean,
 *             2^-24 |mean| rstd, as a shift of every entry of y.
 *   z      = (x - mean) rstd gamma + beta [+ residual]          fp32, every operation rounded on its own, left to right
 *   y      = z, or leaky != 0: z > 0 ? z : z alpha
 *   moving <- moving - (moving - batch) * float32(1 - momentum)  in fp32, in TF's operation order (assign_moving_average), for the
 *             mean and for the biased variance, batch = the float64 statistic rounded to fp32; 1 - momentum is taken in float64 from
 *             the float argument.  moving_mean and moving_var are both given or both NULL (no update).
 *   gamma == NULL: the form without batch norm (:162-165), z = x + beta [+ residual] with beta the offset; no statistics, one launch;
 *             mean, rstd, eps, momentum and the moving pointers are unused.
 * Backward, from gy f32[n, C] (ldg) and the STORED y (never a recomputation):
 *   g      = gy (y > 0 ? 1 : alpha) under leaky (y == 0 takes alpha, as LeakyReluGrad), gy otherwise (y is then unused, may be NULL)
 *   xhat   = (x - mean) rstd
 *   gbeta_c = sum_i g     ggamma_c = sum_i g xhat
 *   gx     = gamma rstd (g - gbeta/n - xhat ggamma/n)      gres = g (gres may be NULL)
 *   gamma == NULL: gbeta (the offset's gradient) and gx = g only; x, mean, rstd and ggamma are unused.
 * Aliases: y may be residual's buffer; gx may be gy's; gres may be gy's when gx is not.
 * THE SUMMATION ORDER IS PART OF THE DEFINITION and is a function of the capacity M, n and C only -- never of the device, the leading
 * dimensions or the alignment.  Rows are cut into slices of S = 256 rows, doubled until at most 128 slices cover M.  With
 * LQ = min(16, the power of two >= ceil(C / 4)) and R = 256 / LQ, chain r of a slice adds the slice's rows r, r + R, r + 2 R, ... in
 * ascending order from 0.0; the R chains are added by the tree  chain[r] += chain[r + s]  for r < s,  s = R/2, R/4, ... 1; the slice
 * partials are added in ascending slice order from 0.0.  All of it in float64 (the summands are the fp32 values widened; for var the
 * float64 squares of the float64 deviations; for ggamma the float64 products of the fp32 g and the fp32 xhat).  No float atomic, no
 * read-back, capturable; two calls give equal bits.
 * Kernels: lanes run across columns, four consecutive columns (a quad) per lane, LQ lanes per row, so a wavefront reads 64 / LQ rows at
 * a time (C <= 16: 16 to 64 rows; C >= 64: four runs of 256 bytes).  Quads are moved as one 16-byte access when C % 4 == 0, every leading
 * dimension in the call is a multiple of 4 and every base pointer is 16-byte aligned; as four guarded 4-byte accesses otherwise.  The
 * thread mapping, and so the order above, is the same on both paths.
 * Launches.  Forward, three: the column sums; the centred sums, whose last workgroup to finish writes mean and rstd and updates the
 * moving statistics; the elementwise pass.  (gamma == NULL: the elementwise pass alone.)  Backward, two: the two column sums per slice;
 * the elementwise pass, in which every workgroup adds the slice partials of its own columns and those of slice 0 write ggamma and gbeta.
 * Every word of the first n rows (C columns) of y / gx / gres is written and rows at or beyond n are left alone; x, y, gy and residual
 * rows at or beyond n are never read.  n == 0 writes nothing, leaves the moving statistics untouched and returns D3F_OK.
 * D3F_ERR_ARG before anything touches the device: M < 0, C < 1 or > 2^20, a leading dimension in use below C, a NULL beta / gbeta,
 * gamma with a NULL mean or rstd (or ggamma, backward) or eps <= 0, one moving pointer without the other, gres == gx, a NULL x / y /
 * gy / gx in use with M > 0.
 * workspace (8-byte aligned) >= d3f_batch_norm_workspace_bytes(M, C): a ticket and two sets of slice partials (slices x C doubles); its
 * contents before the call do not matter; else D3F_ERR_WORKSPACE. */
size_t d3f_batch_norm_workspace_bytes(int M, int C);
int d3f_batch_norm_train(const float* x, int ldx, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                         float* moving_mean, float* moving_var, const float* residual, int ldr, int leaky, float alpha, float* y, int ldy,
                         float* mean, float* rstd, const int* M_dev, void* workspace, size_t workspace_bytes, void* stream);
int d3f_batch_norm_backward(const float* x, int ldx, const float* y, int ldy, const float* gy, int ldg, int M, int C, const float* gamma,
                            const float* mean, const float* rstd, int leaky, float alpha, float* gx, int ldgx, float* ggamma,
                            float* gbeta, float* gres, int ldgr, const int* M_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of d3f_ind_max_pool (models/network_blocks.py:51-66): TF's gradient of gather -> reduce_max with the reduce_min behind the
 * shadow row, under the equal-split tie rule of d3f_detect_head_backward.  fp32 rows only: feat_bf16 != 0 is D3F_ERR_ARG.
 * x f32[n1, C] (ldx) the pooled layer's input, idx i32[n2, ld_idx] (K columns), y f32[n2, C] (ldy) the STORED forward output, gy f32[n2, C]
 * (ldg) its gradient, gx f32[n1, C] (ldgx) the result; n1 = min(N1, *N1_dev), n2 = min(N2, *N2_dev) (either pointer may be NULL), N1 and
 * N2 are capacities.  start / edges: the table d3f_neighbor_transpose_qs made of the same idx with Ns = N1.
 * Forward: x' = concat(x, colmin), colmin[c] = min_j x[j,c] (the ordered minimum: -0 below +0); a slot whose index is outside [0, n1) is a
 * SHADOW slot and gathers colmin; y[i,c] = max_k x'[idx[i,k], c].
 * Backward.  Equality is equality of VALUES (tf.equal: -0 == +0); inputs are finite.
 *   T[i,c]  = the number of the K slots of row i whose gathered value equals y[i,c]: a real index listed twice counts twice, every
 *             shadow slot counts on its own, and counts when colmin[c] == y[i,c]
 *   gs[i,c] = gy[i,c] / T[i,c]                       one fp32 division (T == 0, which a y of the forward never gives, takes gs = 0)
 *   S[c]    = sum_i (tying shadow slots of (i,c)) * gs[i,c]        the products rounded in fp32, the sum in float64
 *   M[c]    = #{j < n1 : x[j,c] == colmin[c]}
 *   gx[j,c] = sum over the edges e = i K + k of row j's segment, in ascending e, of [x[j,c] == y[i,c]] gs[i,c]
 *             + [x[j,c] == colmin[c]] float(S[c] / M[c])
 * Summation orders.  The segment sum is ONE fp32 chain per entry in ascending e, started at zero, and the shadow share is added last.
 * S: pooled rows are cut into slices of 256 rows, doubled until at most 128 slices cover the capacity N2; with LQ = min(16, the power of
 * two >= ceil(C / 4)) and R = 256 / LQ, chain r of a slice adds the rows r, r + R, ... in ascending order from 0.0, the R chains are added
 * by the tree chain[r] += chain[r + s], s = R/2 .. 1, and the slice partials in ascending slice order -- all in float64, the rule of
 * d3f_batch_norm_train.  colmin and M are integer work (ordered minima and counts): any order gives the same result.  No float atomic;
 * two calls give equal bits; a row of gx depends on its own segment and on the two column vectors only.
 * Kernels: lanes run across columns, a quad of four columns per lane; one 16-byte access per quad when C % 4 == 0, every leading dimension
 * is a multiple of 4 and x, y, gy, gx are 16-byte aligned, four guarded 4-byte accesses otherwise -- the same thread mapping and the
 * same orders on both paths.  Three launches: column minima and their counts per slice of fine rows; per pooled row T, gs and the
 * slice partials of S, whose last workgroup to finish folds colmin, M and S into the share; the segment gather.  All sizes are read on
 * the device; no memset, no read-back; capturable.
 * Every word of the first n1 rows (C columns) of gx is written; rows at or beyond n1 are left alone; a row nobody names gets exactly
 * the shadow share or zero; n2 == 0 (or K == 0) writes zeros.  x rows at or beyond n1 and idx / y / gy rows at or beyond n2 are never
 * read; no index outside [0, n1) forms an address; the table is range-checked, never trusted.  N1 == 0 is D3F_OK.
 * D3F_ERR_ARG before anything touches the device: feat_bf16 != 0, a negative size, C < 1 or > 2^20, N2 * K > 2^31 - 8192, ld_idx < K,
 * ldx / ldy / ldg / ldgx < C, a NULL x, gx or start, a NULL y or gy with N2 > 0, a NULL idx or edges with N2 * K > 0.
 * workspace >= d3f_ind_max_pool_backward_workspace_bytes(N1, N2, K, C): gs (N2 rows of ceil(C / 4) quads), the slice partials, two
 * column vectors and a ticket; its contents before the call do not matter; else D3F_ERR_WORKSPACE.  The function returns 0 for sizes
 * the call refuses. */
size_t d3f_ind_max_pool_backward_workspace_bytes(int N1, int N2, int K, int C);
int d3f_ind_max_pool_backward(const void* x, int N1, int ldx, int C, const int* idx, int N2, int ld_idx, int K, const void* y, int ldy,
                              const float* gy, int ldg, const int* start, const int* edges, float* gx, int ldgx, const int* N1_dev,
                              const int* N2_dev, int feat_bf16, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of d3f_closest_pool_cat (models/network_blocks.py:69-83 + models/D3Feat.py:63) with respect to x: from g f32[n2, >= C1]
 * (ldg), the gradient of out = [x'[idx[n,0]] | skip[n]], to gx f32[n1, C1] (ldgx):
 *   gx[j,:] = sum of g[n, 0:C1] over the fine rows n < n2 with idx[n,0] == j, in ascending n, ONE fp32 chain per entry started at zero.
 * A shadow index (outside [0, n1)) carries no gradient.  The gradient of skip is the column view g[:, C1:]: no kernel.
 * idx i32[n2, ld_idx]: the first column is read.  start / edges: the table d3f_neighbor_transpose_qs made of that ONE column (K = 1,
 * the same ld_idx, Ns = N1); an edge is used only when it is in range and idx[e, 0] == j.  n1 = min(N1, *N1_dev), n2 = min(N2, *N2_dev).
 * One launch, the thread mapping and the two access paths of d3f_ind_max_pool_backward (16 bytes when C1 % 4 == 0, ldg and ldgx are
 * multiples of 4 and g, gx are 16-byte aligned); no atomic, no memset, no read-back, capturable; two calls give equal bits.  Every word of
 * the first n1 rows (C1 columns) of gx is written, rows nobody names get zeros (n2 == 0: all), rows at or beyond n1 are left alone.
 * D3F_ERR_ARG before anything touches the device: a negative size, C1 < 1 or > 2^20, N2 > 2^31 - 8192, ldg < C1, ldgx < C1, ld_idx < 1,
 * a NULL gx or start, a NULL g, idx or edges with N2 > 0.  N1 == 0 is D3F_OK. */
int d3f_closest_pool_cat_backward(const float* g, int N2, int ldg, int C1, const int* idx, int ld_idx, int N1, const int* start,
                                  const int* edges, float* gx, int ldgx, const int* N1_dev, const int* N2_dev, void* stream);

/* The optimiser's step of EVERY variable in one call (utils/trainer.py:119-156 of the reference: tf.train.MomentumOptimizer, no
 * Nesterov, behind a per-variable tf.clip_by_norm; the gradient of the regularisation loss of KPFCNN_model.py:189-191 folded in).
 * desc: T descriptors on the DEVICE, one per variable: v f32[count] the variable, g f32[count] its gradient, a f32[count] its `Momentum`
 *   slot, and a decay flag.  A variable whose g (or v, or a) is NULL is skipped whole: v and a are left untouched, nothing goes into R.
 * chunks: the table d3f_momentum_sgd_plan made of the same counts, on the device: i32[nchunks, 2] = (variable, first element); every
 *   variable is cut into chunks of D3F_SGD_CHUNK elements, a variable's chunks are contiguous and in element order.  The kernels
 *   range-check every entry against desc; an entry that does not fit is passed over.
 * hyper: f32[4] on the DEVICE, {lr, mom, clip, wd}: read by the kernels, so a captured call follows a new learning rate.
 * Per variable, fl(.) one float32 rounding, nothing contracted into a fused multiply-add:
 *   g1 = g                      (decay == 0)        g1 = fl(g + fl(wd * v))      (decay != 0)
 *   S  = sum over the variable of (double)g1 * (double)g1,  n = (float)sqrt(S)   (a correctly rounded float64 root, rounded once more)
 *   s  = clip > 0 ? fl(clip / max(n, clip)) : 1          (n == 0 gives 1; a NaN n stays NaN)
 *   g2 = fl(g1 * s),   a' = fl(fl(mom * a) + g2),   v' = fl(v - fl(lr * a'))
 *   R  = sum over the decayed variables of 0.5 * (double)v * (double)v  of the OLD v;  *reg_loss_out = (float)((double)wd * R)
 * zero_grad != 0: every word of g inside the counts is +0 afterwards (a gradient buffer that autograd accumulates into stays in place);
 * else g is only read.  reg_loss_out may be NULL.  A non-finite gradient follows the arithmetic and stays inside its own variable.
 * Summation orders, all float64 from 0.0.  Within a chunk, thread t of 256 adds the elements of its quads t, t + 256, ... (quad q =
 * elements 4 q .. 4 q + 3 of the chunk) in ascending order; lane l of a wave takes acc += acc[l + s] for s = 32 .. 1; the four wave sums
 * are added as (w0 + w2) + (w1 + w3).  A variable's chunk partials are added in chunk order, R's over the whole table in table order.
 * A quad is one 16-byte access where v, g and a of the variable are all 16-byte aligned, four 4-byte accesses otherwise and in a
 * variable's tail: the same orders and the same bits on both paths.
 * Two launches whatever T is (partials; totals + update).  No float atomic, no memset, no read-back, capturable; two calls on equal
 * inputs give equal bits; no word beyond count of any tensor is written.  T == 0 launches nothing and returns D3F_OK.
 * D3F_ERR_ARG before anything touches the device: T or nchunks negative, a NULL hyper, a NULL desc with T > 0, a NULL chunks with T > 0
 * and nchunks > 0.  workspace >= d3f_momentum_sgd_workspace_bytes(T, nchunks): 16 bytes per chunk, every word of it written before it is
 * read; else D3F_ERR_WORKSPACE.  The size function returns 0 for negative sizes.
 * d3f_momentum_sgd_plan (host only): counts i32[T] -> the number of chunks, and the first chunks_cap of them into chunks_out when it is
 * not NULL; D3F_ERR_ARG for a negative T, count or chunks_cap, a NULL counts with T > 0, more than 2^30 chunks. */
#define D3F_SGD_CHUNK 4096
typedef struct d3f_sgd_var {
    float* v;
    float* g;
    float* a;
    int count;
    int decay;
} d3f_sgd_var;
int d3f_momentum_sgd_plan(const int* counts, int T, int* chunks_out, int chunks_cap);
size_t d3f_momentum_sgd_workspace_bytes(int T, int nchunks);
int d3f_momentum_sgd(const void* desc, int T, const int* chunks, int nchunks, const float* hyper, int zero_grad, float* reg_loss_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The KITTI test metric of P * per_pair estimated transforms in two launches (utils/tester.py:326-344 of the reference: relative
 * translation error, relative rotation error, success under both thresholds, and the sums of its three AverageMeters).
 *   T_est f32[P * per_pair, 12], row-major [R | t]; gt f32[P, 12] in the SAME direction as T_est: source -> target, the direction of
 *     KITTI's `trans` and of what d3f_register_pairs returns for the pair (anchor, positive).  NOT the target -> source convention of
 *     d3f_register_pairs' own gt argument.  Row i uses gt[i / per_pair]: per_pair is 1 for d3f_register_pairs' T_out and n_counts for
 *     d3f_register_pairs_counts' T_out.
 *   thresholds_host: TWO doubles on the host, [rte_max, rre_max in radians] (2 and pi / 180 * 5 in the reference), read before the
 *     call returns.
 * Per row, in float64, the inputs widened f32 -> f64 and every operation rounded on its own (never contracted):
 *     d_r = T[r,3] - G[r,3];  rte = sqrt((d0 d0 + d1 d1) + d2 d2);
 *     tr  = the nine products T[k,i] G[k,i] of the rotation parts in row-major order (k outer), summed left to right
 *           (= trace(R_est^T R_gt));  c = (tr - 1) / 2;  rre = acos(c);  rre_deg = (rre * 180) / pi.
 *   A NaN is kept, never clamped: c > 1 gives rre = NaN, and NaN counts as a failure (tester.py:330,335 do not clamp either).
 *   rte_dev f64[P * per_pair], rre_deg_dev f64[P * per_pair] (degrees), flags_dev i32[P * per_pair]:
 *     bit 0: rte < rte_max;  bit 1: rre is no NaN and rre < rre_max (radians);  bit 2: both.  Strict comparisons (tester.py:332-338).
 *   meters_dev (optional) f64[per_pair, 8], per column c over the rows p * per_pair + c, p = 0 .. P - 1:
 *     [0] sum of rte, [1] sum of rte * rte, [2] their number -- over the rows with bit 0 (whatever bit 1 is);
 *     [3] sum of rre_deg, [4] sum of rre_deg * rre_deg, [5] their number -- over the rows with bit 1 (whatever bit 0 is);
 *     [6] rows with bit 2, [7] P.  avg = sum / n and var = sq_sum / n - avg^2 are the reference's AverageMeter figures.
 *   THE SUMMATION ORDER IS PART OF THE DEFINITION: 256 partial sums, partial t adding the rows p = t, t + 256, t + 512, ... in ascending
 *     order from 0.0 (rows without the bit are skipped); then s = 128, 64, ... 1: partial[t] += partial[t + s] for t < s; the result
 *     is partial[0].  The squares are rounded products.  One workgroup, a second launch.
 * NEAR THE GROUND TRUTH the decision rests on the float32 rounding of the two matrices: for T_est == gt, c computed in float64
 * exceeds 1 (rre NaN, a failure) for about half of random float32-rounded rotations, where the reference's own float32 evaluation
 * exceeds 1 for about 0.25 % of them; within roughly 0.03 degrees of gt the two can differ.  RANSAC on 0.3 m voxels does not get there.
 * D3F_ERR_ARG before anything touches the device: P < 0, per_pair < 1, P * per_pair >= 2^31, a NULL pointer other than meters_dev, a
 * NaN or non-positive threshold.  P == 0 is D3F_OK (the meters, when asked for, are written as zeros by one launch).
 * Asynchronous on `stream`; no float atomics, no ticket counter, no memset, no workspace, no allocation, no synchronisation:
 * capturable. */
int d3f_pose_errors(const float* T_est, const float* gt, int P, int per_pair, const double* thresholds_host, double* rte_dev,
                    double* rre_deg_dev, int* flags_dev, double* meters_dev, void* stream);

/* np.nan_to_num of the descriptors of keypoint blocks, in place (geometric_registration_eth/evaluate_eth.py:26-27 of the reference pass
 * the descriptors through it before matching; d3f_match_pairs alone never matches a row that holds a NaN, which is not the same for a
 * row with one bad component).  kp f32[n_blocks, K, ld] on the device, rows [xyz | C descriptor floats | ...]; on the columns
 * 3 .. 3 + C - 1 of every row of every block:
 *     NaN (either sign, any payload) -> +0.0;  +inf -> FLT_MAX;  -inf -> -FLT_MAX;  every other bit pattern, -0.0 and denormals
 *     included, is left as it is (only an element that changes is written).
 * The xyz columns, the score and any further column are never read or written, whatever they hold.  One launch, one thread per
 * element, every element has one writer; a second call changes nothing.  C in {16, 32, 64}, ld >= C + 3, else D3F_ERR_ARG; so are
 * negative sizes and a NULL kp with n_blocks * K > 0.  n_blocks * K == 0 is D3F_OK.  Asynchronous on `stream`, capturable. */
int d3f_sanitize_descriptors(float* kp, int n_blocks, int K, int ld, int C, void* stream);

/* Per-scene summary of the feature-matching figures of d3f_match_pairs: what geometric_registration/evaluate.py:200-219 and
 * geometric_registration_eth/evaluate_eth.py:142-177 of the reference compute from the .rt.txt rows of a scene, for S scenes and n
 * keypoint counts at once.  mutual_count i32[P, n], gt_inliers i32[P, n] (d3f_match_pairs' outputs), gt_flag i32[P] (1 where gt.log
 * lists the pair), all on the device; scene s owns the pairs scene_start_host[s] .. scene_start_host[s + 1] - 1 (S + 1 ints on the
 * HOST, read before the call returns); inlier_ratio_host: one double on the host (0.05 in both scripts).
 * ratio_e8 i32[P, n]: per pair and count the integer m with m / 1e8 == float("%.8f" % (a / b)), a = gt_inliers, b = mutual_count --
 *   the inlier ratio as the reference reads it back from the 8 decimals of its result file -- computed in integers:
 *   m = floor((2 a 10^8 + b) / (2 b)); where a 10^8 / b is exactly a half-integer (only possible when 512 divides b) the decimal
 *   conversion rounds the double fl(a / b), not the rational: with e = fma(fl(a / b), b, -a), which is exact, e > 0 rounds up, e < 0
 *   down, e == 0 to the even integer.  a is clamped to 0 .. b.  b == 0 gives m = 0: the convention of this library's Python layer
 *   (PairMatching.ratios); the reference would divide by zero there.  A pair with gt_flag == 0 gets m = 0 (evaluate_eth.py:43-47).
 * figures i64[S, n, 4], per scene and count: [0] the pairs with gt_flag != 0; [1] the pairs, flagged or not, with
 *   fl(m / 1e8) > inlier_ratio (division and comparison in float64, evaluate_eth.py:154); [2] the sum of gt_inliers and [3] the sum
 *   of m over the pairs with gt_flag != 0.  All integers: no summation order enters.  An empty scene gives four zeros.
 * Two launches (one thread per (pair, count); one workgroup per (scene, count)), no atomics, no memset, no workspace, no allocation,
 * no synchronisation: capturable.  D3F_ERR_ARG before anything touches the device: P < 0, n outside 1 .. D3F_REPEAT_COUNTS_MAX,
 * P * n >= 2^31, S outside 0 .. D3F_SCENES_MAX, scene_start_host not ascending from 0 or scene_start_host[S] != P, a NaN
 * inlier_ratio, a NULL pointer that is needed (the device inputs and ratio_e8 when P > 0, figures when S > 0).  P == 0 is legal. */
int d3f_matching_summary(const int* mutual_count, const int* gt_inliers, const int* gt_flag, int P, int n, const int* scene_start_host,
                         int S, const double* inlier_ratio_host, int* ratio_e8, long long* figures, void* stream);

/* Registration recall of the 3DMatch benchmark (Choi et al.) for S scenes and n estimates per pair at once: what
 * geometric_registration/3dmatch/evaluate.m of the reference computes, through external/ElasticReconstruction/mrEvaluateRegistration.m,
 * from the .log file geometric_registration/evaluate.py:101-110 writes and the scene's gt.log / gt.info.  THE DEFINITION is the text
 * below (tests/recall_np.py is this text in numpy); MATLAB's own bits and the summation order of its BLAS are not reproduced.
 *   T_est, logged: logged == 0: f32[P, n, 3, 4] estimates source -> target (d3f_register_pairs' / d3f_register_pairs_counts' T), widened
 *     to float64 and INVERTED on the device, because evaluate.py:104 logs inv(transformation); logged != 0: f64[P, n, 4, 4] as the
 *     .log holds them, not inverted, the fourth row not read.
 *   gt f64[P, 4, 4]: the gt.log matrix of the pair, target -> source (the direction of d3f_register_pairs' gt; fourth row not read);
 *   info f64[P, 6, 6]: its gt.info matrix;  gt_flag i32[P]: 1 where gt.log lists the pair;  result_flag i32[P]: 1 where the pair has a
 *   result, NULL: result_flag == gt_flag (evaluate.py:60-65 logs exactly the listed pairs);  ids i32[P, 2]: the fragment numbers of the
 *   pair INSIDE ITS SCENE;  all on the device.  Scene s owns the pairs scene_start_host[s] .. scene_start_host[s + 1] - 1 (S + 1 ints
 *   on the HOST, read before the call returns); err2_host: one double on the host (0.04 = 0.2^2 in the .m file).
 * Per row (pair p, column c), with apart = ids[p][1] - ids[p][0] > 1, g = gt_flag[p] != 0, r = result_flag[p] != 0:
 *   flags i32[P, n]: bit 1 (rs_num): r and apart;  bit 3 (gt_num): g and apart, with or without a result;  bit 2 (false positive): r
 *     and apart and not g;  bit 0 (good): r and g and apart and p <= err2 -- NOT strict, and false for a NaN.
 *   error f64[P, n]: the transformation error p where r and g and apart, 0 elsewhere.  In float64, every operation rounded on its own
 *   and every sum taken left to right as written:
 *     inverse of an affine [A | t] by cofactors over the determinant (a general inverse, not A^T: a float32 rotation is orthonormal
 *     to 1e-7 only, and the log holds its true inverse):
 *       n00 = a11 a22 - a12 a21   n01 = a02 a21 - a01 a22   n02 = a01 a12 - a02 a11
 *       n10 = a12 a20 - a10 a22   n11 = a00 a22 - a02 a20   n12 = a02 a10 - a00 a12
 *       n20 = a10 a21 - a11 a20   n21 = a01 a20 - a00 a21   n22 = a00 a11 - a01 a10
 *       det = (a00 n00 + a01 n10) + a02 n20;  B[r][c] = n_rc / det;  u[r] = -((B[r][0] t0 + B[r][1] t1) + B[r][2] t2)
 *     result [R | w] = the inverse of T_est (logged == 0) or the first three rows of T_est (logged != 0);  [B | u] = the inverse of gt;
 *     E[r][c] = (B[r][0] R[0][c] + B[r][1] R[1][c]) + B[r][2] R[2][c];  E[r][3] = ((B[r][0] w0 + B[r][1] w1) + B[r][2] w2) + u[r]
 *     s = ((1 + E00) + E11) + E22;  q0 = 0.5 sqrt(s);  d = 4 q0;
 *     er = [E03, E13, E23, (E21 - E12) / d, (E02 - E20) / d, (E10 - E01) / d]
 *     v[r] = the six products info[r][c] er[c], c ascending;  p = (the six products er[r] v[r], r ascending) / info[0][0].
 *   Where s > 0 is false, p is NaN (MATLAB would go complex for s < 0: only within rounding of a 180 degree error).  A NaN anywhere
 *   gives a NaN p and a row that is not good.
 * figures i64[S, n, 5], per scene and column the rows with: [0] bit 0 (good); [1] bit 1 without bits 0 and 2 (bad); [2] bit 2
 *   (false_pos); [3] bit 3 (gt_num); [4] bit 1 (rs_num).  recall = good / gt_num, precision = good / rs_num.  All integers: no
 *   summation order enters.  An empty scene gives five zeros.  Duplicate ground-truth entries, which the .m file's mask resolves to
 *   the last one, cannot be expressed: one row per pair and estimate.  Duplicate result rows are rows.
 * Two launches whatever P is (one thread per row; one workgroup per scene), no atomics, no memset, no workspace, no allocation, no
 * synchronisation: capturable.  D3F_ERR_ARG before anything touches the device: P < 0, n outside 1 .. D3F_REPEAT_COUNTS_MAX,
 * P * n >= 2^31, S outside 0 .. D3F_SCENES_MAX, scene_start_host not ascending from 0 or scene_start_host[S] != P, err2 not positive
 * (NaN too), a NULL pointer that is needed (the host pointers; the device inputs other than result_flag, error and flags when P > 0;
 * figures when S > 0).  P == 0 is legal. */
int d3f_registration_recall(const void* T_est, int logged, const double* gt, const double* info, const int* gt_flag,
                            const int* result_flag, const int* ids, int P, int n, const int* scene_start_host, int S,
                            const double* err2_host, double* error, int* flags, long long* figures, void* stream);

/* Point-to-point ICP of B (source, target) pairs, run to convergence on the device (datasets/KITTI.py:293-297 of the reference refines
 * the KITTI ground truth with it).  THE DEFINITION is Open3D's registration_icp with TransformationEstimationPointToPoint(False) and
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration), restated here; tests/icp_np.py is this text in numpy, and
 * what the tests pin is this text, not Open3D's bits.
 *   grid: built by d3f_neighbor_grid_build over the N_tgt stacked rows of the B target clouds (s_lens_dev = their lengths) with a
 *     radius >= max_correspondence_distance.  (Any built grid gives the same result: the kernel derives the stencil from the grid's
 *     own cell edge; a radius below the distance only widens the stencil and costs time.)
 *   src f32[N_src, 3]: the stacked source rows; src_lens_dev i32[B] on the device (a length that runs past N_src is cut there, a
 *     negative one is 0).  Pair p is source cloud p against target cloud p.  init f64[B, 12] on the device: row-major [R | t] of T_0.
 *   criteria_host: THREE doubles on the host, [max_correspondence_distance r, relative_fitness, relative_rmse], read before the call returns.
 * Per pair, with Ns source rows s_i, T_0 = init and k = 0, 1, ..., everything in float64 with every operation rounded on its own:
 *   move      p_i = ((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r] for r = 0, 1, 2, (x, y, z) = s_i widened f32 -> f64, [R | t] = T_k
 *             (the convention of d3f_repeatability_pairs' moved keypoints, in float64);
 *   search    the nearest row of the pair's target cloud by d2 = (dx dx + dy dy) + dz dz, dx = p_i - x widened, among those with
 *             d2 < r r STRICTLY (r r the rounded float64 product); equal d2: the lowest target index.  n_k = the rows that have one.
 *   figures   fitness_k = n_k / Ns (0 for Ns = 0), rmse_k = sqrt(sum d2 / n_k) (0 for n_k = 0).
 *   stop      at k with T_k if k >= 1 and |fitness_k - fitness_{k-1}| < relative_fitness and |rmse_k - rmse_{k-1}| < relative_rmse:
 *             converged = 1; otherwise if k == max_iteration: converged = 0.  iterations = k, the updates applied (Open3D's loop count).
 *   update    otherwise T_{k+1} = U_k T_k, each entry ((u0 m0 + u1 m1) + u2 m2), the translation column + t_U last.  U_k = [R_U | t_U]
 *             is the rigid fit without scaling of the pairs (p_i -> its target row x_i): mp = (sum p) / n_k, mt = (sum x) / n_k,
 *             S[a][b] = (sum p_a x_b) - (sum p_a) mt[b], R_U = the rotation of Horn's quaternion method on S (the largest eigenvector
 *             of the 4 x 4 matrix N(S) by 12 cyclic Jacobi sweeps, as the RANSAC fit of d3f_ransac_hypotheses),
 *             t_U[a] = mt[a] - ((R_U[a,0] mp[0] + R_U[a,1] mp[1]) + R_U[a,2] mp[2]).  n_k = 0: U_k is the identity and T_{k+1} has T_k's bits.
 *   At most max_iteration + 1 searches run per pair.
 * THE SUMMATION ORDER IS PART OF THE DEFINITION.  The 16 sums are sum d2 | sum p (3) | sum x (3) | sum p_a x_b (a outer; rounded
 * products); a row without a correspondence adds +0.0 to each.  Chunk c of a pair = its rows 256 c .. 256 c + 255 in original
 * numbering (the last one padded with +0.0).  Inside a chunk: each group of 64 consecutive rows by the halving tree s = 32, 16, .. 1
 * (v[t] += v[t + s] for t < s), then (g0 + g1) + (g2 + g3) over the four groups.  Over the chunks of the pair: 256 partial sums,
 * partial t adding the chunks c = t, t + 256, ... in ascending order from 0.0, then s = 128, 64, .. 1: partial[t] += partial[t + s]
 * for t < s.  No floating-point atomics: nothing depends on an order of arrival.
 * Outputs, all on the device and OVERWRITTEN: T f64[B, 12] = T_k at the stop; count i32[B] = n_k, sumd2 f64[B], fitness f64[B],
 *   rmse f64[B] -- the figures of the last search, the one under the returned T; iterations i32[B]; converged i32[B]; nearest
 *   (optional) i32[N_src]: per source row the index INSIDE the pair's target cloud of its correspondence under the returned T, -1:
 *   none (rows past the sum of the lengths are not written).
 * Launches: one to initialise, then per round a search over the rows of every unfinished pair and a one-workgroup-per-pair finish
 *   (sums, stop test, fit, T_{k+1}); both return at once for a finished pair.  No persistent kernel, no grid-wide sync, no workgroup
 *   waits for another.  check_every = n > 0: after every n rounds the host reads the number of unfinished pairs (one more launch, one
 *   4-byte copy, one stream synchronisation) and stops enqueueing when it is 0.  check_every = 0: exactly max_iteration + 1 rounds
 *   are enqueued with no read-back, no allocation and no memset -- capturable in a HIP graph.  Both forms give the same bits.
 * workspace >= d3f_icp_pairs_workspace_bytes(N_src, B) (132 bytes per 256 source rows, plus the per-pair words), else
 * D3F_ERR_WORKSPACE; so is a grid_bytes below d3f_neighbor_grid_bytes(N_tgt, B).  The size function returns 0 for sizes the call refuses.
 * D3F_ERR_ARG before anything touches the device: a negative size, B outside 1 .. D3F_MAX_BATCH, max_iteration < 0, check_every < 0,
 * r not positive and finite (NaN too), a NaN criterion, a NULL pointer other than nearest (src may be NULL when N_src == 0).
 * Asynchronous on `stream` apart from the read-backs of check_every > 0; no allocation. */
size_t d3f_icp_pairs_workspace_bytes(int N_src, int B);
int d3f_icp_pairs(const void* grid, size_t grid_bytes, int N_tgt, const float* src, int N_src, const int* src_lens_dev, int B,
                  const double* init, const double* criteria_host, int max_iteration, int check_every, double* T, int* count,
                  double* sumd2, double* fitness, double* rmse, int* iterations, int* converged, int* nearest, void* workspace,
                  size_t workspace_bytes, void* stream);

/* Training pairs: the correspondences, the sample and the augmentation of P pairs in one call (what the reference's generators do per
 * pair on the host: datasets/KITTI.py:35-48, 182-206, 319-337; datasets/ThreeDMatch.py:24-45, 222-229, 266-273).  No read-back, no
 * host decision, every length read on the device: capturable.
 *   points f32[N, 3]: 2 P stacked clouds, lens_dev i32[2 P]; cloud 2 p is the anchor and cloud 2 p + 1 the positive of pair p.  A
 *   length below 0 counts as 0, one that runs past N is cut there; n = the sum.  Rows from n on are neither read nor written.
 * THE DRAWS.  Counter based and stateless: with mix = the finaliser of splitmix64 (the function under d3f_ransac_draw),
 *   key  = mix(mix(seed ^ mix(step)) ^ (pair << 8 | stream)),   draw(seed, step, pair, stream, counter) = mix(key ^ counter),
 * 64 bits; d3f_training_draw is the host copy (D3F_ERR_ARG: out NULL, pair < 0, stream outside 0 .. 255).  pair = pair0 + p: a caller
 * that splits a list of pairs over several calls passes the number of the first one, and P pairs in one call give the bits of P calls.
 * u24(r) = (r >> 40) 2^-24, a float in [0, 1); integers in [0, m) are (r >> 11) mod m.  The streams and their counters:
 *   D3F_TP_STREAM_NOISE + side     3 i + c        coordinate c of row i of the cloud (side 0: anchor, 1: positive)
 *   D3F_TP_STREAM_ROTATION + side  2 d, 2 d + 1   angle and axis of rotation d of the cloud
 *   D3F_TP_STREAM_SCALE            0              the scale of the PAIR
 *   D3F_TP_STREAM_SHIFT + side     c              coordinate c of the shift of the cloud
 *   D3F_TP_STREAM_SAMPLE           i              entry i of the sample
 * step: *step_dev, a u64 on the device, read by the first kernel; the call's last kernel stores step + 1 there, so a replayed graph
 * draws afresh every time with no host write.  use_host_step != 0: host_step is used instead (step_dev, when not NULL, still receives
 * host_step + 1).  Equal (seed, step) give equal bits.
 * THE MATCHES, radius form (grid != NULL: built by d3f_neighbor_grid_build over these points and lengths, B = 2 P, with a radius >=
 * `radius`; trans f32[P, 16]: row-major 4 x 4, source to target, three rows read).  The anchor row (x, y, z) is moved to
 *   q[r] = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], fp32, every operation rounded on its own (no FMA),
 * and every row j of the positive with d2 = (dx dx + dy dy) + dz dz < radius radius STRICTLY (dx = q - s; fp32, no FMA: the metric of
 * every search of this library) is a match (i, j).  The matches are ordered by i ascending and inside a row by (d2, j) ascending:
 * get_matching_indices' list, FLANN returning a radius result by distance (equal distances: the smaller index here; Open3D's own bits
 * are not pinned, it is not available to the tests).  M = their number (all pairs of a call together: below 2^31).  The list is never
 * stored: match number t is the candidate of rank t - start[i] of the row i with start[i] <= t < start[i + 1].
 * The sample, radius form: keypts_num DISTINCT match numbers by Floyd's algorithm -- S empty; for i = 0 .. keypts_num - 1 with
 * j = M - keypts_num + i: t = draw(SAMPLE, i) mod (j + 1); entry i = t if t is not in S, else j; S gains entry i.  (Every subset is
 * equally likely; M == keypts_num returns every match.)  anc_idx[p, i] = the match's i, pos_idx[p, i] = its j + the anchor's length:
 * indices into the pair's own rows, the convention of d3f_loss_gradients.  status_dev[p]: D3F_TP_FEW_MATCHES when M < min_matches
 * (the reference drops such a pair; its 1024 is an argument here), D3F_TP_BELOW_KEYPTS when M < keypts_num.
 * List form (grid == NULL; keypts_pairs i32[L, 2], pair_start_dev i32[P + 1]: pair p owns rows pair_start[p] .. pair_start[p + 1] of
 * the list, the reference's precomputed keypts): entry i is row draw(SAMPLE, i) mod len of the pair's list, WITH replacement, the
 * second column shifted by the anchor's length.  No search, trans and radius are not read.  D3F_TP_BELOW_KEYPTS for an empty list,
 * D3F_TP_LIST_RANGE for offsets outside 0 .. L.  The list's values are not checked (d3f_loss_gradients does).
 * A pair with a status other than 0 gets n_dev[p] = 0 and NO index is written for it (d3f_loss_gradients then skips it); otherwise
 * n_dev[p] = keypts_num.  matches_dev[p] = M (list form: the list's length).  row0_dev i32[P + 1]: the first row of every pair, and n.
 * THE ROW PASS.  params f32[2 P, 16] per cloud: [0..8] R row-major, [9] scale, [10..12] shift, [13] the first angle, [14] the first
 * axis, [15] augment_rotation.
 *   R: identity for augment_rotation 0; for 1 one draw, for 3 the product (R_0 R_1) R_2 of three draws with axes 0, 1, 2, each entry
 *      (a0 b0 + a1 b1) + a2 b2 in fp32 without FMA.  A draw: theta = ((r >> 11) 2^-53 2) pi in float64, c = (float)cos(theta),
 *      s = (float)sin(theta), axis = (r' >> 11) mod 3 for augment_rotation 1; the matrix is the reference's own (ThreeDMatch.py:24-45,
 *      as it stands): [[c, -s, -s], [s, c, -s], [s, s, c]] with column and row `axis` cleared and R[axis, axis] = 1.
 *   scale = scale_min + (scale_max - scale_min) u24, one per pair; shift[c] = -shift_range + (2 shift_range) u24, one per cloud; fp32,
 *      each operation rounded on its own.
 *   out_points row = ((p + u noise) @ R) scale + shift:  a[c] = p[c] + u24(NOISE, 3 i + c) augment_noise  (u uniform, not Gaussian: the
 *      reference's rand);  o[j] = ((a[0] R[0,j] + a[1] R[1,j]) + a[2] R[2,j]) scale + shift[j];  fp32, no FMA.  The rows of a pair with
 *      a status are augmented all the same.
 *   backup row: radius form: the moved anchor rows and the positive's rows as they are (the pair in one frame); list form: the input.
 * Launches: parameters and offsets; rows (backup, augmentation, the matches of every anchor row); radius form: the one-launch scan,
 * the sample per pair, one thread per sample entry for its (i, j); list form: the sample per pair.  Five or three, whatever P is.
 * No float atomic, no memset, fixed orders; nothing is written beyond n rows, P entries or keypts_num indices of a row.
 * workspace >= d3f_training_pairs_workspace_bytes(N, P, keypts_num) (8 bytes per row, 4 per sample entry, the offsets), else
 * D3F_ERR_WORKSPACE; so is a grid_bytes below d3f_neighbor_grid_bytes(N, 2 P).  The size function returns 0 for sizes the call refuses.
 * D3F_ERR_ARG before anything touches the device: N < 0, P < 1, 2 P > D3F_MAX_BATCH, keypts_num outside 1 .. D3F_TRAINING_KEYPTS_MAX
 * (the sample is drawn in LDS), ld_idx < keypts_num, pair0 < 0, L < 0, radius form: a radius that is not positive and finite, trans
 * NULL; list form: keypts_pairs or pair_start_dev NULL; augment_rotation not 0 / 1 / 3, a NaN parameter, step_dev NULL without
 * use_host_step, any other NULL pointer (points, out_points and backup may be NULL when N == 0).
 * Asynchronous on `stream`, no allocation, no synchronisation. */
#define D3F_TRAINING_KEYPTS_MAX 1024   /* largest keypts_num of d3f_training_pairs (= D3F_VALIDATION_NMAX, what the loss takes) */
#define D3F_TP_STREAM_NOISE 0
#define D3F_TP_STREAM_ROTATION 2
#define D3F_TP_STREAM_SCALE 4
#define D3F_TP_STREAM_SHIFT 6
#define D3F_TP_STREAM_SAMPLE 8
#define D3F_TP_FEW_MATCHES 1
#define D3F_TP_BELOW_KEYPTS 2
#define D3F_TP_LIST_RANGE 4
int d3f_training_draw(uint64_t seed, uint64_t step, int pair, int stream, uint64_t counter, uint64_t* out);
size_t d3f_training_pairs_workspace_bytes(int N, int P, int keypts_num);
int d3f_training_pairs(const void* grid, size_t grid_bytes, const float* points, int N, const int* lens_dev, int P, const float* trans,
                       const int* keypts_pairs, int L, const int* pair_start_dev, float radius, int keypts_num, int min_matches,
                       uint64_t seed, uint64_t* step_dev, int use_host_step, uint64_t host_step, int pair0, float augment_noise,
                       int augment_rotation, float scale_min, float scale_max, float shift_range, float* out_points, float* backup,
                       int* anc_idx, int* pos_idx, int ld_idx, int* n_dev, int* row0_dev, int* matches_dev, int* status_dev,
                       float* params, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D3FEAT_AMD_H */
