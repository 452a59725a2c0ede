"""Downstream matching on the MI355X: what the reference does with descriptors after the hot path.

    feature_nn(A, B)                        nearest descriptor, one direction           geometric_registration/evaluate.py:17-21
    build_correspondence(src_desc, tgt_desc) mutually closest pairs                      evaluate.py:11-27 (same name)
    ransac_feature_matching(...)            open3d.registration_ransac_based_on_feature_matching as the reference calls it
                                            (evaluate.py:93-99, demo_registration.py:184-192)
    register_keypoints(src_rec, tgt_rec)    both of them on the last num_keypts rows of two keypoint record blocks
                                            (evaluate.py:45-50,67,93-99), the records never leaving the device
    register_pairs(kp, count, pairs, ...)   register_keypoints for every pair of a scene's fragments in one call (evaluate.py:150-156):
                                            four launches, no read-back in between, capturable; scene_pairs, stack_keypoints,
                                            EVALUATE_3DMATCH go with it
    repeatability_pairs(kp, count, pairs, gt) keypoint repeatability of every pair at every keypoint count in one launch
                                            (repeatability/evaluate_3dmatch_our.py:30-41, evaluate_kitti_our.py:12-23; float64)
    match_pairs(kp, count, pairs, gt)       feature-matching recall figures (mutual matches, inliers under gt) of every pair at every
                                            keypoint count in two launches (evaluate.py:45-50,67-82), up to 8192 rows per block
    register_pairs_counts(kp, count, pairs, ...) register_pairs AND match_pairs for every pair at every keypoint count in one call
                                            (evaluate.py:45-50,67-99 swept over num_keypts), up to 8192 rows per block
    pose_errors(T, gt)                      the KITTI test metric (RTE, RRE, success, the running meters) of every estimate in two
                                            launches (utils/tester.py:326-344; float64); register_kitti_pairs(kp, count, gt, voxel)
                                            is register_pairs + pose_errors as ModelTester.test_kitti pairs them (:292-344)
    sanitize_descriptors(kp)                np.nan_to_num of the descriptor columns, in place (evaluate_eth.py:26-27)
    matching_summary(matching, gt_flag, scene_start) recall, average inliers and average inlier ratio of every scene at every count
                                            in two launches (evaluate.py:200-219, evaluate_eth.py:142-177); match_scenes(...) is
                                            sanitize_descriptors + match_pairs + matching_summary, the ETH test in one call
    registration_recall(T, gt, info, gt_flag, ids, scene_start) the registration recall of the 3DMatch benchmark (3dmatch/evaluate.m,
                                            mrEvaluateRegistration.m; float64) of every scene at every count in two launches;
                                            register_scenes(...) is sanitize_descriptors + register_pairs(_counts) + matching_summary
                                            + registration_recall: both recalls of all eight scenes in one call

Every computation is a kernel of libd3feat_amd.so (csrc/registration.hip, csrc/radius_neighbors.hip); numpy / torch only
move data and run the host loop over batches of hypotheses.  Open3D's own random stream is unspecified, so results are
deterministic functions of `seed` here and are pinned to oracle/registration_np.py (same algorithm, same random numbers).
"""
import numpy as np
import torch

from . import _lib, ops
from .utils import results


def _dev(device=None):
    return device if device is not None else torch.device("cuda", torch.cuda.current_device())


def _f32(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


# ---- plumbing of the one-call entry points (here and in overlap.py / validation.py): each rule once -----------------------------------
PAIRS_PER_CALL = 4096


def _blocks(fn, kp, count, pairs, min_ld):
    """The keypoint blocks of a call: kp f32[n_blocks, K, ld >= min_ld], count i32[n_blocks], pairs i32[P, 2], device, contiguous.
    -> kp, count, pairs, n_blocks, K, ld, P, device."""
    kp = ops._req(kp, torch.float32, "kp", 3)
    count = ops._req(count, torch.int32, "count", 1)
    pairs = ops._req(pairs, torch.int32, "pairs", 2)
    if not kp.is_contiguous() or not count.is_contiguous() or not pairs.is_contiguous() or pairs.shape[1] != 2:
        raise ValueError("%s: kp, count and pairs must be contiguous, pairs [P, 2]" % fn)
    n_blocks, K, ld = kp.shape
    if count.shape[0] != n_blocks or n_blocks < 1 or K < 1 or ld < min_ld:
        raise ValueError("%s: kp %s, count %s" % (fn, tuple(kp.shape), tuple(count.shape)))
    return kp, count, pairs, n_blocks, K, ld, pairs.shape[0], kp.device


def _counts(fn, num_keypts, kmax):
    """The keypoint counts of a sweep -> (list of ints, the ctypes array the library reads)."""
    ks = [int(k) for k in num_keypts]
    if not 1 <= len(ks) <= _lib.REPEAT_COUNTS_MAX or any(not 1 <= k <= kmax for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("%s: num_keypts %s must be 1 to %d strictly ascending counts in 1..%d" % (fn, ks, _lib.REPEAT_COUNTS_MAX, kmax))
    return ks, (_lib.C.c_int * len(ks))(*ks)


def _gt32(fn, gt, P):
    """The float32 ground truth of P pairs: device f32[P, 3, 4], contiguous."""
    gt = ops._req(gt, torch.float32, "gt", 3)
    if tuple(gt.shape) != (P, 3, 4) or not gt.is_contiguous():
        raise ValueError("%s: gt of shape %s for %d pairs" % (fn, tuple(gt.shape), P))
    return gt


def _scene_starts(fn, scene_start, P):
    """S + 1 host ints, scene s owning the pairs scene_start[s] .. scene_start[s + 1] - 1 -> (list, the ctypes array the library reads)."""
    starts = [int(v) for v in np.asarray(scene_start).reshape(-1)]
    S = len(starts) - 1
    if not 0 <= S <= _lib.SCENES_MAX or starts[0] != 0 or starts[-1] != P or any(b < a for a, b in zip(starts, starts[1:])):
        raise ValueError("%s: scene_start %s must hold 1 to %d ascending ints from 0 to P = %d" % (fn, starts, _lib.SCENES_MAX + 1, P))
    return starts, (_lib.C.c_int * (S + 1))(*starts)


def _chunks(P, per_call=None):
    """The slices of P pairs, per_call (PAIRS_PER_CALL as it is now) at a time."""
    per_call = per_call or PAIRS_PER_CALL
    for p0 in range(0, P, per_call):
        yield slice(p0, min(p0 + per_call, P))


def _ptr(t):
    """The address of a tensor; None for no tensor and for an empty one, which has no address."""
    return t.data_ptr() if t is not None and t.numel() else None


class _PairResult:
    """Base of the device-result objects.  FIELDS: the tensors _host() reads back (a None one is left out), HOST: further ones; every
    constructor sets key -- what a later call with out=self must ask for again.  device: where the first of FIELDS is."""
    FIELDS = HOST = ()
    key = None
    _cache = None
    device = property(lambda self: getattr(self, self.FIELDS[0]).device)

    def _read(self, name):
        return getattr(self, name).cpu().numpy()

    def _host(self):
        # one read-back of the whole result, kept until the next call with out=self
        if self._cache is None:
            self._cache = {k: self._read(k) for k in self.FIELDS + self.HOST if getattr(self, k) is not None}
        return self._cache


def _reuse(fn, out, cls, key, device, make):
    """The result object of a call: make() without `out`, else `out` itself if it is a `cls` made for the same key on the same device.
    Its read-back is forgotten either way."""
    if out is None:
        out = make()
    elif not isinstance(out, cls) or out.key != key or out.device != device:
        raise _another_call(fn)
    out._cache = None
    return out


def _another_call(fn):
    return ValueError("%s: out= was made for another call" % fn)


def _ransac_dict(h, at, near=None):
    """The dict ransac_feature_matching returns (plus best_iteration), from row `at` of a read-back h; near: the winner's target row of
    every source row, for correspondence_set."""
    Ns, cnt = int(h["ns"][at]), np.int64(h["inliers"][at])
    sd2 = np.float64(h["sumd2"][at]) / 4294967296.0
    M = np.eye(4)
    M[:3, :4] = h["T"][at].astype(np.float64)
    out = dict(transformation=M, fitness=float(cnt) / Ns if Ns else 0.0, inlier_rmse=float(np.sqrt(sd2 / np.maximum(cnt, 1))))
    if near is not None:
        out["correspondence_set"] = _correspondence_set(near[:Ns])
    out.update(iterations=int(h["iterations"][at]), validations=int(h["validations"][at]), best_iteration=int(h["best_iteration"][at]))
    return out


def _correspondence_set(near):
    sel = np.nonzero(near >= 0)[0]
    return np.stack([sel, near[sel]], 1).astype(np.int64)


def _gt_figures(out, h, at, k):
    """gt_inliers and inlier_ratio = gt_inliers / k (k: the mutual matches; 0.0 without one), when the call had gt."""
    if "gt_inliers" in h:
        out["gt_inliers"] = int(h["gt_inliers"][at])
        out["inlier_ratio"] = out["gt_inliers"] / k if k else 0.0
    return out


def feature_nn(A, B, return_d2=False, device=None):
    """idx[i] = argmin_j ||A_i - B_j||^2 (ties to the lowest j).  A [n,C], B [m,C], C in {16,32,64} -> int32 [n] (device)."""
    lib = _lib.load()
    dev = _dev(device)
    A, B = _f32(A, dev), _f32(B, dev)
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("feature_nn: A %s, B %s" % (tuple(A.shape), tuple(B.shape)))
    n, m, C = A.shape[0], B.shape[0], A.shape[1]
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    d2 = torch.empty((n,), dtype=torch.float32, device=dev) if return_d2 else None
    ws = ops.workspace(lib.d3f_feature_nn_workspace_bytes(n), dev)
    rc = lib.d3f_feature_nn(A.data_ptr(), n, C, B.data_ptr(), m, C, C, idx.data_ptr(), d2.data_ptr() if return_d2 else None,
                            ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "feature_nn")
    return (idx, d2) if return_d2 else idx


def build_correspondence(source_desc, target_desc, device=None):
    """evaluate.py:11-27: the mutually closest pairs in feature space -> int array [k, 2] (host), ascending source index."""
    lib = _lib.load()
    dev = _dev(device)
    A, B = _f32(source_desc, dev), _f32(target_desc, dev)
    ab, ba = feature_nn(A, B, device=dev), feature_nn(B, A, device=dev)
    n = A.shape[0]
    pairs = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = ops.workspace(lib.d3f_mutual_matches_workspace_bytes(n), dev)
    rc = lib.d3f_mutual_matches(ab.data_ptr(), n, ba.data_ptr(), B.shape[0], pairs.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                ws.numel(), ops._stream(dev))
    _lib.check(rc, "mutual_matches")
    k = int(count.item())
    return pairs[:k].cpu().numpy().astype(np.int64)


def ransac_feature_matching(source_points, target_points, source_desc, target_desc, max_correspondence_distance, ransac_n=4,
                            edge_similarity=0.9, checker_distance=None, max_iteration=100000, max_validation=100, seed=0,
                            batch=1 << 16, device=None):
    """open3d.registration_ransac_based_on_feature_matching (Open3D 0.7 semantics):
    iterate: ransac_n random source points, each paired with its nearest target FEATURE -> edge-length checker -> rigid fit ->
    distance checker; the first `max_validation` iterations that pass (in iteration order, among at most `max_iteration`) are
    scored -- fitness = share of source points with a target POINT inside max_correspondence_distance after the transform,
    rmse over those -- and the best (fitness, then rmse) wins.  Iterations run on the GPU in batches of `batch`.
    -> dict(transformation f64[4,4], fitness, inlier_rmse, correspondence_set i64[k,2], iterations, validations)."""
    lib = _lib.load()
    dev = _dev(device)
    src, tgt = _f32(source_points, dev), _f32(target_points, dev)
    Ns, Nt = src.shape[0], tgt.shape[0]
    ident = dict(transformation=np.eye(4), fitness=0.0, inlier_rmse=0.0, correspondence_set=np.zeros((0, 2), np.int64),
                 iterations=0, validations=0)
    if Ns < ransac_n or Nt < ransac_n or max_correspondence_distance <= 0:
        return ident
    nn = feature_nn(source_desc, target_desc, device=dev)
    st = ops._stream(dev)
    chosen, it0, max_validation = [], 0, int(max_validation)
    while it0 < max_iteration and sum(c.shape[0] for c in chosen) < max_validation:
        H = int(min(batch, max_iteration - it0))
        T = torch.empty((H, 12), dtype=torch.float32, device=dev)
        valid = torch.empty((H,), dtype=torch.uint8, device=dev)
        rc = lib.d3f_ransac_hypotheses(src.data_ptr(), Ns, tgt.data_ptr(), Nt, nn.data_ptr(), int(ransac_n),
                                       float(edge_similarity or 0.0), float(checker_distance or 0.0), int(seed), int(it0), H,
                                       T.data_ptr(), valid.data_ptr(), st)
        _lib.check(rc, "ransac_hypotheses")
        keep = torch.nonzero(valid, as_tuple=False).reshape(-1)        # (plumbing: index selection of the passing rows)
        if keep.numel():
            chosen.append(T.index_select(0, keep))
        it0 += H
    if not chosen:
        ident["iterations"] = it0
        return ident
    Tv = torch.cat(chosen, 0)[:max_validation].contiguous()
    V = Tv.shape[0]
    grid = ops.NeighborGrid(tgt, ops.as_lens([Nt], dev), float(max_correspondence_distance))
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    sumd2 = torch.empty((V,), dtype=torch.int64, device=dev)
    rc = lib.d3f_neighbor_grid_score(grid.mem.data_ptr(), grid.nbytes, Nt, src.data_ptr(), Ns, Tv.data_ptr(), V,
                                     float(max_correspondence_distance), count.data_ptr(), sumd2.data_ptr(), None, st)
    _lib.check(rc, "neighbor_grid_score")
    cnt = count.cpu().numpy().astype(np.int64)
    sd2 = sumd2.cpu().numpy().astype(np.float64) / 4294967296.0
    rmse = np.sqrt(sd2 / np.maximum(cnt, 1))
    # best fitness, then lowest rmse, then earliest iteration
    order = np.lexsort((np.arange(V), rmse, -cnt))
    b = int(order[0])
    Tb = Tv[b:b + 1].contiguous()
    nearest = torch.empty((Ns,), dtype=torch.int32, device=dev)
    rc = lib.d3f_neighbor_grid_score(grid.mem.data_ptr(), grid.nbytes, Nt, src.data_ptr(), Ns, Tb.data_ptr(), 1,
                                     float(max_correspondence_distance), count[:1].data_ptr(), sumd2[:1].data_ptr(),
                                     nearest.data_ptr(), st)
    _lib.check(rc, "neighbor_grid_score")
    near = nearest.cpu().numpy()
    sel = np.nonzero(near >= 0)[0]
    M = np.eye(4)
    M[:3, :4] = Tb.cpu().numpy().reshape(3, 4).astype(np.float64)
    return dict(transformation=M, fitness=float(cnt[b]) / Ns, inlier_rmse=float(rmse[b]),
                correspondence_set=np.stack([sel, near[sel]], 1).astype(np.int64), iterations=it0, validations=V)


def register_keypoints(src_records, tgt_records, num_keypts=None, device=None, **ransac_kw):
    """Registration of two fragments from their keypoint records: device f32[k, 3 + C + 1] blocks of [xyz | desc | score] rows in
    ascending score order (keypoints.topk_records, FragmentEngine.fetch(keypoints=True)).  As geometric_registration/evaluate.py
    does with the files of a pair: the last `num_keypts` rows of each (:45-50; None = all rows) -> build_correspondence (:67) and
    ransac_feature_matching (:93-99, `ransac_kw` are its arguments, max_correspondence_distance among them) -- slicing only, the
    records do not visit the host.  -> the RANSAC dict plus `correspondences` (the mutually closest pairs, i64[k, 2])."""
    dev = _dev(device)
    blocks = []
    for name, rec in (("src_records", src_records), ("tgt_records", tgt_records)):
        rec = ops._req(rec, torch.float32, name, 2)
        if rec.shape[1] < 5:
            raise ValueError("register_keypoints: %s of %d floats per row" % (name, rec.shape[1]))
        if num_keypts is not None:
            rec = rec[max(rec.shape[0] - int(num_keypts), 0):]
        blocks.append(rec)
    (s, t), w = blocks, blocks[0].shape[1]
    out = ransac_feature_matching(s[:, :3], t[:, :3], s[:, 3:w - 1], t[:, 3:w - 1], device=dev, **ransac_kw)
    out["correspondences"] = build_correspondence(s[:, 3:w - 1], t[:, 3:w - 1], device=dev)
    return out


# ---- every pair of a scene in one call (geometric_registration/evaluate.py:150-156) -------------------------------------------
# evaluate.py:93-99: the call the reference makes for every pair (compat/open3d spells it for one pair)
EVALUATE_3DMATCH = dict(max_correspondence_distance=0.05, ransac_n=3, edge_similarity=0.9, checker_distance=0.05,
                        max_iteration=50000, max_validation=1000)


def scene_pairs(n, device=None):
    """All pairs id1 < id2 of n fragments in the order of evaluate.py:154-155 -> device i32[n (n - 1) / 2, 2]."""
    iu = np.triu_indices(int(n), 1)
    return torch.from_numpy(np.stack(iu, 1).astype(np.int32).reshape(-1, 2)).to(_dev(device))


def stack_keypoints(blocks, K=None, device=None):
    """A list of [k_i, ld] keypoint record blocks (what FragmentEngine.fetch(slot, keypoints=True) returns per fragment, ascending
    score order) -> (kp f32[n, K, ld], count i32[n]) on the device; a block longer than K keeps its LAST K rows."""
    blocks = [b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)) for b in blocks]
    if not blocks or any(b.dim() != 2 or b.shape[1] != blocks[0].shape[1] for b in blocks):
        raise ValueError("stack_keypoints: blocks of shapes %s" % ([tuple(b.shape) for b in blocks],))
    dev = _dev(device) if device is not None or not blocks[0].is_cuda else blocks[0].device
    K = int(K) if K is not None else max(b.shape[0] for b in blocks)
    kp = torch.zeros((len(blocks), max(K, 1), blocks[0].shape[1]), dtype=torch.float32, device=dev)
    for f, b in enumerate(blocks):
        b = b[max(b.shape[0] - K, 0):]
        kp[f, :b.shape[0]].copy_(b, non_blocking=True)
    count = torch.tensor([min(b.shape[0], K) for b in blocks], dtype=torch.int32).to(dev)
    return kp, count


class PairRegistration(_PairResult):
    """Result of register_pairs: DEVICE tensors, one row per pair.
    T f32[P,3,4] ([R | t] of the winner, identity without one), inliers i32[P], sumd2 i64[P] (2^-32 units), validations i32[P],
    iterations i32[P], best_iteration i32[P] (-1: none), mutual_count i32[P], nearest i32[P,Kmax] (target row of every source row
    under the winner, -1: none); mutual i32[P,Kmax,2] / gt_inliers i32[P] when asked for.  Rows are numbered inside the rows a
    pair uses (the last min(count, num_keypts) of a block)."""
    FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "nearest", "mutual", "gt_inliers")
    HOST = ("ns", "nt")

    def __init__(self, P, Kmax, device, correspondences, gt):
        i32 = dict(dtype=torch.int32, device=device)
        self.P, self.Kmax = P, Kmax
        self.key = (P, Kmax, bool(correspondences), bool(gt))
        self.T = torch.empty((P, 3, 4), dtype=torch.float32, device=device)
        self.inliers, self.validations, self.iterations = (torch.empty((P,), **i32) for _ in range(3))
        self.best_iteration, self.mutual_count = torch.empty((P,), **i32), torch.empty((P,), **i32)
        self.sumd2 = torch.empty((P,), dtype=torch.int64, device=device)
        self.nearest = torch.empty((P, Kmax), **i32)
        self.mutual = torch.empty((P, Kmax, 2), **i32) if correspondences else None
        self.gt_inliers = torch.empty((P,), **i32) if gt else None
        self.ns = self.nt = None

    def host(self, p):
        """The dict register_keypoints returns for pair p (plus best_iteration, and inlier_ratio when gt was given)."""
        h = self._host()
        out = _ransac_dict(h, p, h["nearest"][p])
        k = int(h["mutual_count"][p])
        if "mutual" in h:
            out["correspondences"] = h["mutual"][p, :k].astype(np.int64)
        return _gt_figures(out, h, p, k)


def register_pairs(kp, count, pairs, max_correspondence_distance, num_keypts=None, ransac_n=4, edge_similarity=0.9,
                   checker_distance=None, max_iteration=100000, max_validation=100, seed=0, gt=None, distance_threshold=0.10,
                   correspondences=False, out=None):
    """register_keypoints for P pairs of keypoint blocks in one call: kp f32[n_blocks, K, ld] ([xyz | desc | score] rows in ascending
    score order, keypoints.topk_records / stack_keypoints), count i32[n_blocks], pairs i32[P, 2] (source, target) block indices, all on
    the device.  Four launches per PAIRS_PER_CALL pairs, no read-back and no host decision in between (capturable: pass the previous
    result as `out`); per pair bit-identical to register_keypoints(kp[a, :count[a]], kp[b, :count[b]], num_keypts, ...) -- the keywords
    are ransac_feature_matching's.  gt f32[P, 3, 4] (target -> source) adds gt_inliers (evaluate.py:70-77, distance_threshold);
    correspondences=True adds the mutually closest pairs themselves.  -> PairRegistration (device tensors; .host(p) for a dict)."""
    lib = _lib.load()
    kp, count, pairs, n_blocks, K, ld, P, dev = _blocks("register_pairs", kp, count, pairs, 0)
    C = ld - 4
    Kmax = min(K, int(num_keypts)) if num_keypts is not None else K
    if Kmax < 1:
        raise ValueError("register_pairs: kp %s, count %s, num_keypts %s" % (tuple(kp.shape), tuple(count.shape), num_keypts))
    if Kmax > _lib.PAIRS_KMAX or C not in (16, 32, 64) or not 3 <= int(ransac_n) <= 8:
        raise ValueError("register_pairs takes up to %d rows per block, descriptors of 16, 32 or 64 floats and ransac_n in 3..8 (got %d "
                         "rows, %d floats, ransac_n %s): use register_keypoints for one pair of larger blocks"
                         % (_lib.PAIRS_KMAX, Kmax, C, ransac_n))
    if gt is not None:
        gt = _gt32("register_pairs", gt, P)
    out = _reuse("register_pairs", out, PairRegistration, (P, Kmax, bool(correspondences), gt is not None), dev,
                 lambda: PairRegistration(P, Kmax, dev, correspondences, gt is not None))
    # rows each pair uses (plumbing for host(): fitness = inliers / Ns)
    used = count.clamp(0, Kmax)
    out.ns, out.nt = used[pairs[:, 0].long()], used[pairs[:, 1].long()]
    st = ops._stream(dev)
    nk, mv = int(num_keypts) if num_keypts is not None else 0, int(max_validation)
    for s in _chunks(P):
        n = s.stop - s.start
        ws = ops.workspace(lib.d3f_register_pairs_workspace_bytes(n, K, nk, mv), dev)
        rc = lib.d3f_register_pairs(
            kp.data_ptr(), n_blocks, K, ld, C, count.data_ptr(), pairs[s].data_ptr(), n, nk, float(max_correspondence_distance),
            int(ransac_n), float(edge_similarity or 0.0), float(checker_distance or 0.0), int(max_iteration), mv, int(seed),
            gt[s].data_ptr() if gt is not None else None, float(distance_threshold), out.T[s].data_ptr(), out.inliers[s].data_ptr(),
            out.sumd2[s].data_ptr(), out.validations[s].data_ptr(), out.iterations[s].data_ptr(), out.best_iteration[s].data_ptr(),
            out.mutual_count[s].data_ptr(), out.nearest[s].data_ptr(), out.mutual[s].data_ptr() if correspondences else None,
            out.gt_inliers[s].data_ptr() if gt is not None else None, ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "register_pairs")
    return out


# ---- keypoint repeatability of every pair at every count in one call (repeatability/evaluate_*_our.py) -----------------------------
REPEATABILITY_COUNTS = (4, 8, 16, 32, 64, 128, 256, 512)                       # num_list of both scripts
REPEATABILITY_3DMATCH = dict(distance_threshold=0.1, moved="target")           # evaluate_3dmatch_our.py:36-40
REPEATABILITY_KITTI = dict(distance_threshold=0.5, moved="source")             # evaluate_kitti_our.py:18-22,43


class PairRepeatability(_PairResult):
    """Result of repeatability_pairs: DEVICE tensors repeat i32[P, n] (target keypoints with a source keypoint inside the threshold,
    per pair and count) and totals i64[n] (their sums over the pairs); num_keypts is the tuple of the n counts."""
    FIELDS = ("repeat", "totals")

    def __init__(self, P, num_keypts, device):
        self.P, self.num_keypts = P, tuple(num_keypts)
        self.key = (P, self.num_keypts)
        n, chunks = len(self.num_keypts), max(-(-P // PAIRS_PER_CALL), 1)
        self.repeat = torch.empty((P, n), dtype=torch.int32, device=device)
        self.totals = torch.zeros((n,), dtype=torch.int64, device=device)
        # more than PAIRS_PER_CALL pairs: the totals of every call, added up in row order (integers)
        self.chunk_totals = torch.empty((chunks, n), dtype=torch.int64, device=device) if chunks > 1 else None

    def ratios(self):
        """f64[P, n]: repeat / num_keypts, the figure the reference appends per pair (the count itself, whatever the blocks hold)."""
        return self._host()["repeat"].astype(np.float64) / np.asarray(self.num_keypts, np.float64)

    def scene(self):
        """f64[n]: the average of the ratios over the P pairs, as totals / (num_keypts * P)."""
        k = np.asarray(self.num_keypts, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._host()["totals"].astype(np.float64) / (k * self.P)


def _gt_f64(gt, P, device):
    """[P,3,4] or [P,4,4], float32 or float64, tensor or numpy -> f64[P,3,4] contiguous on the device (as it is when it is that already)."""
    if not isinstance(gt, torch.Tensor):
        gt = torch.from_numpy(np.ascontiguousarray(gt))
    if gt.dtype not in (torch.float32, torch.float64) or gt.dim() != 3 or gt.shape[0] != P or tuple(gt.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError("repeatability_pairs: gt %s of shape %s for %d pairs" % (gt.dtype, tuple(gt.shape), P))
    return gt[:, :3].to(device=device, dtype=torch.float64).contiguous()


def repeatability_pairs(kp, count, pairs, gt, num_keypts=REPEATABILITY_COUNTS, distance_threshold=0.1, moved="target", out=None):
    """Keypoint repeatability of P pairs of keypoint blocks at every count of `num_keypts` in one call (repeatability/
    evaluate_3dmatch_our.py:30-41, evaluate_kitti_our.py:12-23): kp f32[n_blocks, K, ld >= 3] (rows [xyz | ...] in ascending score
    order: keypoints.topk_records / stack_keypoints), count i32[n_blocks], pairs i32[P, 2] (source, target) block indices, all on the
    device.  For each count k the last k rows of both blocks are taken, one block is moved with gt in float64 -- moved="target": gt
    takes the target frame into the source frame (3DMatch, as register_pairs' gt); moved="source": gt takes the source into the
    target frame (KITTI's trans) -- and the TARGET keypoints with a source keypoint strictly closer than distance_threshold are
    counted.  The counts are nested prefixes in score rank, so one pass over the sources serves all of them: two launches per
    PAIRS_PER_CALL pairs, no read-back and no host decision (capturable: pass the previous result as `out`, and gt as a device
    f64[P,3,4] tensor so that it is read in place).  num_keypts: strictly ascending, 1 .. 1024, at most 16 of them.
    -> PairRepeatability (device tensors; .ratios() / .scene() for the reference's figures)."""
    lib = _lib.load()
    kp, count, pairs, n_blocks, K, ld, P, dev = _blocks("repeatability_pairs", kp, count, pairs, 3)
    ks, c_ks = _counts("repeatability_pairs", num_keypts, _lib.PAIRS_KMAX)
    if moved not in ("target", "source"):
        raise ValueError("repeatability_pairs: moved=%r (\"target\" or \"source\")" % (moved,))
    thr = float(distance_threshold)
    if not thr > 0.0:
        raise ValueError("repeatability_pairs: distance_threshold %r" % (distance_threshold,))
    gt = _gt_f64(gt, P, dev)
    out = _reuse("repeatability_pairs", out, PairRepeatability, (P, tuple(ks)), dev, lambda: PairRepeatability(P, ks, dev))
    st = ops._stream(dev)
    c_thr, n = _lib.C.c_double(thr), len(ks)
    for i, s in enumerate(_chunks(P)):
        totals = out.totals if out.chunk_totals is None else out.chunk_totals[i]
        rc = lib.d3f_repeatability_pairs(kp.data_ptr(), n_blocks, K, ld, count.data_ptr(), pairs[s].data_ptr(), s.stop - s.start,
                                         gt[s].data_ptr(), 1 if moved == "source" else 0, _lib.C.addressof(c_thr),
                                         _lib.C.addressof(c_ks), n, out.repeat[s].data_ptr(), totals.data_ptr(), st)
        _lib.check(rc, "repeatability_pairs")
    if out.chunk_totals is not None:
        torch.sum(out.chunk_totals, 0, out=out.totals)          # (plumbing: int64 rows of the calls)
    return out


# ---- feature-matching recall of every pair at every count in one call (geometric_registration/evaluate.py:45-50,67-82) -------------
MATCHING_COUNTS = (250, 500, 1000, 2500, 5000)                                 # the sweep of evaluate.py:46's num_keypts


class PairMatching(_PairResult):
    """Result of match_pairs: DEVICE tensors mutual_count i32[P, n] (mutually nearest descriptor pairs, per pair and count) and
    gt_inliers i32[P, n] (those inside the distance threshold under gt; None without gt); num_keypts is the tuple of the n counts."""
    FIELDS = ("mutual_count", "gt_inliers")

    def __init__(self, P, num_keypts, device, gt):
        self.P, self.num_keypts = P, tuple(num_keypts)
        self.key = (P, self.num_keypts, bool(gt))
        n = len(self.num_keypts)
        self.mutual_count = torch.empty((P, n), dtype=torch.int32, device=device)
        self.gt_inliers = torch.empty((P, n), dtype=torch.int32, device=device) if gt else None

    def ratios(self):
        """f64[P, n]: gt_inliers / mutual_count (evaluate.py:81), 0.0 for a pair without a mutual match (as PairRegistration.host)."""
        h = self._host()
        if "gt_inliers" not in h:
            raise ValueError("PairMatching.ratios: match_pairs was called without gt")
        m = h["mutual_count"].astype(np.float64)
        return np.where(m > 0, h["gt_inliers"] / np.maximum(m, 1.0), 0.0)

    def rows(self, c, gt_flag):
        """The rows [num_inliers, inlier_ratio, gt_flag] of count num_keypts[c] as evaluate.py:203-204 reads them back from the result
        files (the ratio at the 8 decimals of the file), one per pair: the input of results.feature_matching_recall /
        matching_table.  gt_flag: P ints, 1 where gt.log lists the pair; the other pairs get zeros (evaluate.py:60-64)."""
        flag = np.asarray(gt_flag)
        if flag.ndim != 1 or flag.shape[0] != self.P or flag.dtype.kind not in "iub":
            raise ValueError("PairMatching.rows: gt_flag of %d ints, one per pair" % self.P)
        flag = (flag != 0).astype(np.int64)
        inl, ratio = self._host()["gt_inliers"][:, c], self.ratios()[:, c]
        return [[int(n) if g else 0, float("%.8f" % r) if g else 0.0, int(g)] for n, r, g in zip(inl, ratio, flag)]


def match_pairs(kp, count, pairs, gt=None, num_keypts=MATCHING_COUNTS, distance_threshold=0.10, out=None):
    """The feature-matching figures of P pairs of keypoint blocks at every count of `num_keypts` in one call (geometric_registration/
    evaluate.py:45-50, 67-82, whose num_keypts = 250 is edited by hand for the sweep): kp f32[n_blocks, K, ld] ([xyz | desc | score]
    rows in ascending score order: keypoints.topk_records / stack_keypoints), count i32[n_blocks], pairs i32[P, 2] (source, target)
    block indices, all on the device.  For each count k the last min(count, k) rows of both blocks: mutual_count = the mutually nearest
    descriptor pairs (build_correspondence), gt_inliers = those with |s - gt t| < distance_threshold, gt f32[P, 3, 4] (target ->
    source) -- for k <= 1024 bit for bit what register_pairs(..., num_keypts=k, gt=gt) returns under these names, without its RANSAC
    and for blocks of up to 8192 rows.  The counts are nested prefixes in score rank, so one pass over the largest count serves all of
    them: two launches per PAIRS_PER_CALL pairs, no read-back and no host decision (capturable: pass the previous result as `out`).
    num_keypts: strictly ascending, 1 .. 8192, at most 16 of them.  -> PairMatching (device tensors; .ratios() / .rows())."""
    lib = _lib.load()
    kp, count, pairs, n_blocks, K, ld, P, dev = _blocks("match_pairs", kp, count, pairs, 0)
    C = ld - 4
    if C not in (16, 32, 64):
        raise ValueError("match_pairs: kp %s (descriptors of 16, 32 or 64 floats), count %s" % (tuple(kp.shape), tuple(count.shape)))
    ks, c_ks = _counts("match_pairs", num_keypts, _lib.MATCH_KMAX)
    thr = float(distance_threshold)
    if thr != thr:
        raise ValueError("match_pairs: distance_threshold %r" % (distance_threshold,))
    if gt is not None:
        gt = _gt32("match_pairs", gt, P)
    out = _reuse("match_pairs", out, PairMatching, (P, tuple(ks), gt is not None), dev, lambda: PairMatching(P, ks, dev, gt is not None))
    st, n = ops._stream(dev), len(ks)
    for s in _chunks(P):
        ws = ops.workspace(lib.d3f_match_pairs_workspace_bytes(s.stop - s.start, _lib.C.addressof(c_ks), n), dev)
        rc = lib.d3f_match_pairs(kp.data_ptr(), n_blocks, K, ld, C, count.data_ptr(), pairs[s].data_ptr(), s.stop - s.start,
                                 gt[s].data_ptr() if gt is not None else None, thr, _lib.C.addressof(c_ks), n,
                                 out.mutual_count[s].data_ptr(), out.gt_inliers[s].data_ptr() if gt is not None else None,
                                 ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "match_pairs")
    return out


# ---- RANSAC registration of every pair at every count in one call (geometric_registration/evaluate.py:45-50,67-99) -----------------
class PairRegistrationCounts(_PairResult):
    """Result of register_pairs_counts: DEVICE tensors, one row per pair and count (num_keypts is the tuple of the n counts).
    T f32[P,n,3,4] ([R | t] of the winner, identity without one), inliers / validations / iterations / best_iteration (-1: none) /
    mutual_count i32[P,n], sumd2 i64[P,n] (2^-32 units), gt_inliers i32[P,n] when gt was given, nearest i32[P, sum of the counts] when
    asked for: entries offsets[c] .. offsets[c] + num_keypts[c] - 1 are the target rows of the source rows under the winner of count c
    (-1: none).  Rows are numbered inside the rows a pair uses at that count (the last min(count, num_keypts[c]) of a block)."""
    FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers", "nearest")
    HOST = ("ns", "nt")

    def __init__(self, P, num_keypts, device, gt, nearest):
        i32 = dict(dtype=torch.int32, device=device)
        self.P, self.num_keypts = P, tuple(num_keypts)
        self.key = (P, self.num_keypts, bool(gt), bool(nearest))
        n = len(self.num_keypts)
        self.offsets = tuple(int(x) for x in np.concatenate([[0], np.cumsum(self.num_keypts)[:-1]]))
        self.T = torch.empty((P, n, 3, 4), dtype=torch.float32, device=device)
        self.inliers, self.validations, self.iterations = (torch.empty((P, n), **i32) for _ in range(3))
        self.best_iteration, self.mutual_count = torch.empty((P, n), **i32), torch.empty((P, n), **i32)
        self.sumd2 = torch.empty((P, n), dtype=torch.int64, device=device)
        self.gt_inliers = torch.empty((P, n), **i32) if gt else None
        self.nearest = torch.empty((P, sum(self.num_keypts)), **i32) if nearest else None
        self.ns = self.nt = None

    def at(self, c):
        """The device tensors of count num_keypts[c], shaped as PairRegistration's: a dict name -> tensor ([P, ...] views)."""
        k, o = self.num_keypts[c], self.offsets[c]
        out = {f: getattr(self, f)[:, c] for f in self.FIELDS[:-1] if getattr(self, f) is not None}
        if self.nearest is not None:
            out["nearest"] = self.nearest[:, o:o + k]
        return out

    def host(self, p, c):
        """The dict PairRegistration.host(p) returns, for pair p at count num_keypts[c] (`correspondences` needs register_pairs;
        `correspondence_set` needs nearest=True)."""
        h = self._host()
        out = _ransac_dict(h, (p, c))
        out["mutual_count"] = int(h["mutual_count"][p, c])
        if "nearest" in h:
            out["correspondence_set"] = _correspondence_set(h["nearest"][p, self.offsets[c]:self.offsets[c] + int(h["ns"][p, c])])
        return _gt_figures(out, h, (p, c), out["mutual_count"])


def register_pairs_counts(kp, count, pairs, max_correspondence_distance, num_keypts=MATCHING_COUNTS, ransac_n=4, edge_similarity=0.9,
                          checker_distance=None, max_iteration=100000, max_validation=100, seed=0, gt=None, distance_threshold=0.10,
                          nearest=False, out=None):
    """register_keypoints for P pairs of keypoint blocks at every count of `num_keypts` in one call (geometric_registration/evaluate.py:
    45-50, 67-99, whose num_keypts = 250 is edited by hand for the sweep): kp f32[n_blocks, K, ld] ([xyz | desc | score] rows in
    ascending score order, keypoints.topk_records / stack_keypoints; at most 255 blocks), count i32[n_blocks], pairs i32[P, 2] (source,
    target) block indices, all on the device.  Count k uses the last min(count, k) rows of both blocks; per pair and count the result
    is bit-identical to register_keypoints(kp[a, :count[a]], kp[b, :count[b]], num_keypts=k, ...) -- the keywords are
    ransac_feature_matching's -- and, for k <= 1024, to register_pairs(num_keypts=k); mutual_count / gt_inliers are match_pairs'.  No
    block is kept in LDS (blocks of up to 8192 rows), the nearest target point of every hypothesis comes from ONE cell grid over all
    blocks.  Twelve launches per entry-point call, PAIRS_PER_CALL (pair, count) results each, no read-back and no host decision in
    between (capturable: pass the previous result as `out`).  gt f32[P, 3, 4] (target -> source) adds gt_inliers; nearest=True adds
    the winner's correspondences.  num_keypts: strictly ascending, 1 .. 8192, at most 16 of them.
    -> PairRegistrationCounts (device tensors; .host(p, c) for a dict, .at(c) for the tensors of one count)."""
    lib = _lib.load()
    kp, count, pairs, n_blocks, K, ld, P, dev = _blocks("register_pairs_counts", kp, count, pairs, 0)
    C = ld - 4
    if n_blocks > _lib.MAX_BATCH or C not in (16, 32, 64) or not 3 <= int(ransac_n) <= 8:
        raise ValueError("register_pairs_counts takes 1 to %d blocks, descriptors of 16, 32 or 64 floats and ransac_n in 3..8 (got kp %s, "
                         "count %s, ransac_n %s)" % (_lib.MAX_BATCH, tuple(kp.shape), tuple(count.shape), ransac_n))
    ks, c_ks = _counts("register_pairs_counts", num_keypts, _lib.MATCH_KMAX)
    if gt is not None:
        gt = _gt32("register_pairs_counts", gt, P)
    out = _reuse("register_pairs_counts", out, PairRegistrationCounts, (P, tuple(ks), gt is not None, bool(nearest)), dev,
                 lambda: PairRegistrationCounts(P, ks, dev, gt is not None, nearest))
    # rows each pair uses at each count (plumbing for host(): fitness = inliers / Ns)
    used = torch.stack([count.clamp(0, min(K, k)) for k in ks], 1)                  # (device only: nothing to copy under capture)
    valid = (pairs >= 0) & (pairs < n_blocks)
    rows = used[pairs.clamp(0, n_blocks - 1).long()] * valid[:, :, None]           # [P, 2, n]
    out.ns, out.nt = rows[:, 0], rows[:, 1]
    st = ops._stream(dev)
    n, mv = len(ks), int(max_validation)
    for s in _chunks(P, max(PAIRS_PER_CALL // n, 1)):
        m = s.stop - s.start
        ws = ops.workspace(lib.d3f_register_pairs_counts_workspace_bytes(m, n_blocks, K, _lib.C.addressof(c_ks), n, mv), dev)
        rc = lib.d3f_register_pairs_counts(
            kp.data_ptr(), n_blocks, K, ld, C, count.data_ptr(), pairs[s].data_ptr(), m, _lib.C.addressof(c_ks), n,
            float(max_correspondence_distance), int(ransac_n), float(edge_similarity or 0.0), float(checker_distance or 0.0),
            int(max_iteration), mv, int(seed), gt[s].data_ptr() if gt is not None else None, float(distance_threshold),
            out.T[s].data_ptr(), out.inliers[s].data_ptr(), out.sumd2[s].data_ptr(), out.validations[s].data_ptr(),
            out.iterations[s].data_ptr(), out.best_iteration[s].data_ptr(), out.mutual_count[s].data_ptr(),
            out.gt_inliers[s].data_ptr() if gt is not None else None, out.nearest[s].data_ptr() if nearest else None,
            ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "register_pairs_counts")
    return out


# ---- the KITTI test metric of every pair in one call (utils/tester.py:235-360) ------------------------------------------------------
KITTI_SUCCESS = dict(rte_threshold=2.0, rre_threshold=np.pi / 180 * 5)         # tester.py:332-338


def EVALUATE_KITTI(voxel_size):
    """tester.py:305-314: the RANSAC call the reference makes for every KITTI test pair, as register_pairs' keywords."""
    v = float(voxel_size) * 1.0
    return dict(max_correspondence_distance=v, ransac_n=4, edge_similarity=0.9, checker_distance=v, max_iteration=50000,
                max_validation=1000)


def frame_pairs(n_pairs, device=None):
    """(2i, 2i + 1) for i < n_pairs, the block order of FragmentEngine(two_clouds=True, keypoints=K) -> device i32[n_pairs, 2]."""
    a = np.arange(2 * int(n_pairs), dtype=np.int32).reshape(-1, 2)
    return torch.from_numpy(a).to(_dev(device))


class PairPoseErrors(_PairResult):
    """Result of pose_errors: DEVICE tensors rte f64[P, n] (metres), rre_deg f64[P, n] (degrees, NaN kept), flags i32[P, n] (bit 0:
    rte under its threshold, bit 1: rre under its threshold and no NaN, bit 2: both = success) and sums f64[n, 8] (per column the
    sums of d3f_pose_errors' meters: rte sum / square sum / number, the same of rre_deg, successes, P); n is 1 for a [P, 3, 4] input
    (the tensors are then [P]).  .meters(c) turns the sums into the reference's AverageMeter figures."""
    FIELDS = ("rte", "rre_deg", "flags", "sums")

    def __init__(self, P, per_pair, flat, device):
        self.P, self.per_pair, self.flat = P, per_pair, flat
        self.key = (P, per_pair, flat)
        shape = (P,) if flat else (P, per_pair)
        self.rte = torch.empty(shape, dtype=torch.float64, device=device)
        self.rre_deg = torch.empty(shape, dtype=torch.float64, device=device)
        self.flags = torch.empty(shape, dtype=torch.int32, device=device)
        self.sums = torch.empty((per_pair, 8), dtype=torch.float64, device=device)

    def _read(self, name):
        a = super()._read(name)
        return a if name == "sums" else a.reshape(self.P, self.per_pair)

    def host(self):
        """One read-back of the whole result, kept until the next pose_errors(out=self): dict of numpy arrays rte, rre_deg, flags
        ([P, n], a column per count) and sums [n, 8]."""
        return self._host()

    def meters(self, c=0):
        """{"rte" | "rre" | "success": dict(sum, count, avg, var)} of column c: the AverageMeters of tester.py:252 after the last pair
        (var is NaN for a meter that never updated: the reference has no such attribute then)."""
        return results.kitti_meters_from_sums(self.host()["sums"][c])

    def failed(self, ids, c=0):
        """[(id, rte, rre_deg)] of the pairs without success in column c, in pair order: the 'Failed with' lines of tester.py:342."""
        h = self.host()
        if len(ids) != self.P:
            raise ValueError("PairPoseErrors.failed: %d ids for %d pairs" % (len(ids), self.P))
        return [(ids[p], float(h["rte"][p, c]), float(h["rre_deg"][p, c])) for p in range(self.P) if not h["flags"][p, c] & 4]

    def running(self, every=10, c=0):
        """[(i, meters after the first i pairs)] for i = every, 2 every, ...: the figures of the periodic line (tester.py:346-352),
        computed on the host from the per-pair arrays in pair order."""
        h = self.host()
        return [(i, results.kitti_meters(h["rte"][:i, c], h["rre_deg"][:i, c], h["flags"][:i, c]))
                for i in range(int(every), self.P + 1, int(every))]


def pose_errors(T, gt, rte_threshold=KITTI_SUCCESS["rte_threshold"], rre_threshold=KITTI_SUCCESS["rre_threshold"], out=None):
    """The KITTI test metric (tester.py:326-344) of estimated transforms in one call: T f32[P, 3, 4] (PairRegistration.T) or
    f32[P, n, 3, 4] (PairRegistrationCounts.T), gt f32[P, 3, 4] in the SAME direction as T -- source -> target, KITTI's `trans` and what
    register_pairs returns for (anchor, positive); NOT the target -> source gt register_pairs itself takes -- both on the device.
    rte = |t - t_gt|, rre = arccos((trace(R^T R_gt) - 1) / 2) in float64 (NaN kept and counted as a failure), thresholds in metres and
    radians, strict.  Two launches whatever P is, no read-back (capturable: pass the previous result as `out`).
    -> PairPoseErrors (device tensors; .host(), .meters(), .failed(ids), .running())."""
    lib = _lib.load()
    T = ops._req(T, torch.float32, "T")
    if T.dim() not in (3, 4) or tuple(T.shape[-2:]) != (3, 4) or not T.is_contiguous():
        raise ValueError("pose_errors: T of shape %s (contiguous [P, 3, 4] or [P, n, 3, 4])" % (tuple(T.shape),))
    dev, P, flat = T.device, T.shape[0], T.dim() == 3
    n = 1 if flat else T.shape[1]
    gt = ops._req(gt, torch.float32, "gt", 3)
    if tuple(gt.shape) != (P, 3, 4) or not gt.is_contiguous() or n < 1:
        raise ValueError("pose_errors: gt of shape %s for T %s" % (tuple(gt.shape), tuple(T.shape)))
    thr = (float(rte_threshold), float(rre_threshold))
    if not (thr[0] > 0.0 and thr[1] > 0.0):
        raise ValueError("pose_errors: thresholds %r, %r" % (rte_threshold, rre_threshold))
    out = _reuse("pose_errors", out, PairPoseErrors, (P, n, flat), dev, lambda: PairPoseErrors(P, n, flat, dev))
    if P == 0:
        out.sums.zero_()                                         # (plumbing: the meters of no pairs; an empty tensor has no address)
        return out
    c_thr = (_lib.C.c_double * 2)(*thr)
    # one call whatever P is: the summation order of the meters is part of their definition
    rc = lib.d3f_pose_errors(T.data_ptr(), gt.data_ptr(), P, n, _lib.C.addressof(c_thr), out.rte.data_ptr(), out.rre_deg.data_ptr(),
                             out.flags.data_ptr(), out.sums.data_ptr(), ops._stream(dev))
    _lib.check(rc, "pose_errors")
    return out


class KittiRegistration:
    """Result of register_kitti_pairs: `registration` (PairRegistration of register_pairs(frame_pairs, **EVALUATE_KITTI)) and `errors`
    (PairPoseErrors of its T against gt), both device tensors."""

    def __init__(self, registration, errors, pairs):
        self.registration, self.errors, self.pairs = registration, errors, pairs
        self.T = registration.T


def register_kitti_pairs(kp, count, gt, voxel_size, seed=0, out=None):
    """The registration and the metric of ModelTester.test_kitti (tester.py:292-344) for every pair in one call: kp f32[2 P, K, ld] /
    count i32[2 P] the keypoint blocks of FragmentEngine(two_clouds=True, keypoints=K) -- blocks 2i and 2i + 1 are anchor and positive
    of pair i --, gt f32[P, 3, 4] KITTI's `trans` (source -> target).  register_pairs(frame_pairs(P), **EVALUATE_KITTI(voxel_size))
    and then pose_errors on its T with KITTI_SUCCESS, no read-back in between (capturable: pass the previous result as `out`); T is
    bit-equal to register_pairs' own.  gt is NOT handed to register_pairs, whose gt runs target -> source.  -> KittiRegistration."""
    kp = ops._req(kp, torch.float32, "kp", 3)
    if kp.shape[0] % 2:
        raise ValueError("register_kitti_pairs: %d keypoint blocks, not two per pair" % kp.shape[0])
    P = kp.shape[0] // 2
    if out is not None and not isinstance(out, KittiRegistration):
        raise _another_call("register_kitti_pairs")
    pairs = out.pairs if out is not None else frame_pairs(P, kp.device)
    reg = register_pairs(kp, count, pairs, seed=seed, out=out.registration if out is not None else None, **EVALUATE_KITTI(voxel_size))
    err = pose_errors(reg.T, gt, out=out.errors if out is not None else None, **KITTI_SUCCESS)
    return out if out is not None else KittiRegistration(reg, err, pairs)


# ---- the ETH test: every scene's matching recall in one call (geometric_registration_eth/evaluate_eth.py) -----------------------------
EVALUATE_ETH = dict(num_keypts=(250,), distance_threshold=0.10, inlier_ratio=0.05)     # evaluate_eth.py:29,123-124


def sanitize_descriptors(kp):
    """np.nan_to_num on the descriptor columns of kp f32[n_blocks, K, 4 + C] (device, contiguous, C in 16 / 32 / 64), IN PLACE
    (evaluate_eth.py:26-27): NaN -> +0.0, +inf -> FLT_MAX, -inf -> -FLT_MAX, every other bit pattern kept.  The xyz and score columns
    are not touched.  One launch; a second call changes nothing.  -> kp."""
    lib = _lib.load()
    kp = ops._req(kp, torch.float32, "kp", 3)
    n_blocks, K, ld = kp.shape
    if not kp.is_contiguous() or ld - 4 not in (16, 32, 64):
        raise ValueError("sanitize_descriptors: kp %s (contiguous, descriptors of 16, 32 or 64 floats)" % (tuple(kp.shape),))
    if n_blocks * K:
        _lib.check(lib.d3f_sanitize_descriptors(kp.data_ptr(), n_blocks, K, ld, ld - 4, ops._stream(kp.device)), "sanitize_descriptors")
    return kp


class SceneMatching(_PairResult):
    """Result of matching_summary: DEVICE tensors ratio_e8 i32[P, n] (per pair and count the inlier ratio at the 8 decimals of the
    reference's result file, times 1e8; 0 for a pair gt.log does not list) and figures i64[S, n, 4] (per scene and count: ground-truth
    pairs, pairs above inlier_ratio, sum of gt_inliers and sum of ratio_e8 over the ground-truth pairs).  .scenes(), .overall() and
    .rows(c) share one read-back."""
    FIELDS = ("ratio_e8", "figures", "gt_inliers", "gt_flag")

    def __init__(self, P, n, scene_start, inlier_ratio, device):
        self.P, self.n, self.scene_start, self.inlier_ratio = P, n, tuple(int(v) for v in scene_start), float(inlier_ratio)
        self.key = (P, n, self.scene_start, self.inlier_ratio)
        self.S = len(self.scene_start) - 1
        self.ratio_e8 = torch.empty((P, n), dtype=torch.int32, device=device)
        self.figures = torch.empty((self.S, n, 4), dtype=torch.int64, device=device)
        self.gt_inliers = self.gt_flag = None                   # the inputs of the call, kept for the read-back

    def _read(self, name):
        a = super()._read(name)
        return a.reshape(self.P, self.n) if name == "gt_inliers" else a

    def host(self):
        """One read-back of the whole result, kept until the next matching_summary(out=self): dict of numpy arrays ratio_e8 [P, n],
        figures [S, n, 4], gt_inliers [P, n] and gt_flag [P]."""
        return self._host()

    def scenes(self):
        """[scene][count] -> dict(correct, gt, recall, ave_num_inliers, ave_inlier_ratio): the keys and conventions of
        results.feature_matching_recall (the averages divide the sums over the ground-truth pairs by `correct`; 0.0 where the
        reference would divide by zero).  correct, gt and the inlier sum are the integers of `figures`.  The reference adds the
        ratios as float64 in numpy's order, which an integer sum cannot give back bit for bit, so ave_inlier_ratio is np.sum over the
        read-back ratio_e8 / 1e8 column of the scene -- the reference's own expression on the same numbers; figures[..., 3] / 1e8 is
        the same sum without a rounding error."""
        h = self.host()
        out = []
        for s in range(self.S):
            sl, per_count = slice(self.scene_start[s], self.scene_start[s + 1]), []
            flag = h["gt_flag"][sl] != 0
            for c in range(self.n):
                gt, correct, inl = (int(v) for v in h["figures"][s, c, :3])
                ratio = h["ratio_e8"][sl, c] / 1e8
                div = lambda a: float(a / correct) if correct else 0.0
                per_count.append(dict(correct=correct, gt=gt, recall=float(correct / gt) * 100 if gt else 0.0,
                                      ave_num_inliers=div(np.float64(inl)),
                                      ave_inlier_ratio=div(np.sum(np.where(flag, ratio, np.zeros(ratio.shape[0]))))))
            out.append(per_count)
        return out

    def overall(self, c=0):
        """The closing figures of evaluate_eth.py:168-177 at count c: dict(recall_list, matching_recall = all correct / all
        ground-truth pairs in percent, average_recall, average_inliers, average_inliers_ratio = the means over the scenes)."""
        sc = [per_count[c] for per_count in self.scenes()]
        pred, gt = sum(r["correct"] for r in sc), sum(r["gt"] for r in sc)
        mean = lambda key: sum(r[key] for r in sc) / len(sc) if sc else 0.0
        return dict(recall_list=[r["recall"] for r in sc], matching_recall=pred / gt * 100 if gt else 0.0,
                    average_recall=mean("recall"), average_inliers=mean("ave_num_inliers"), average_inliers_ratio=mean("ave_inlier_ratio"))

    def rows(self, c=0):
        """The rows [num_inliers, inlier_ratio, gt_flag] of count c as evaluate_eth.py:150-151 reads them back, one per pair."""
        h = self.host()
        return [[int(i) if g else 0, float(m / 1e8), int(g != 0)] for i, m, g in zip(h["gt_inliers"][:, c], h["ratio_e8"][:, c], h["gt_flag"])]


def matching_summary(mutual_count, gt_inliers=None, gt_flag=None, scene_start=None, inlier_ratio=0.05, out=None):
    """The per-scene summary of evaluate.py:200-219 / evaluate_eth.py:142-177 on the device: mutual_count / gt_inliers i32[P, n]
    (match_pairs' tensors; or a PairMatching in place of the two: matching_summary(matching, gt_flag, scene_start)), gt_flag i32[P]
    device (1 where gt.log lists the pair), scene_start: S + 1 ascending host ints from 0 to P, scene s owning the pairs
    scene_start[s] .. scene_start[s + 1] - 1 (S <= 256).  Per pair and count the ratio gt_inliers / mutual_count rounded to the 8
    decimals of the reference's result file, as an integer (0 without a mutual match: PairMatching.ratios' convention; the reference
    would divide by zero); per scene and count four integer sums.  Two launches, no read-back (capturable: pass the previous result
    as `out`).  -> SceneMatching (device tensors; .scenes(), .overall(), .rows(c))."""
    lib = _lib.load()
    if isinstance(mutual_count, PairMatching):
        if scene_start is None:
            gt_inliers, gt_flag, scene_start = None, gt_inliers, gt_flag
        elif gt_inliers is not None:
            raise ValueError("matching_summary: a PairMatching brings its own gt_inliers")
        matching = mutual_count
        if matching.gt_inliers is None:
            raise ValueError("matching_summary: match_pairs was called without gt")
        mutual_count, gt_inliers = matching.mutual_count, matching.gt_inliers
    mutual_count = ops._req(mutual_count, torch.int32, "mutual_count")
    gt_inliers = ops._req(gt_inliers, torch.int32, "gt_inliers")
    gt_flag = ops._req(gt_flag, torch.int32, "gt_flag", 1)
    if mutual_count.dim() == 1:
        mutual_count, gt_inliers = mutual_count.reshape(-1, 1), gt_inliers.reshape(-1, 1)
    P, n = mutual_count.shape[0], mutual_count.shape[1] if mutual_count.dim() == 2 else 0
    if (mutual_count.dim() != 2 or mutual_count.shape != gt_inliers.shape or gt_flag.shape[0] != P or not 1 <= n <= _lib.REPEAT_COUNTS_MAX
            or not (mutual_count.is_contiguous() and gt_inliers.is_contiguous() and gt_flag.is_contiguous())):
        raise ValueError("matching_summary: mutual_count %s, gt_inliers %s, gt_flag %s (contiguous [P, n], [P, n], [P])"
                         % (tuple(mutual_count.shape), tuple(gt_inliers.shape), tuple(gt_flag.shape)))
    starts, c_starts = _scene_starts("matching_summary", scene_start, P)
    ratio = float(inlier_ratio)
    if ratio != ratio:
        raise ValueError("matching_summary: inlier_ratio %r" % (inlier_ratio,))
    dev = mutual_count.device
    out = _reuse("matching_summary", out, SceneMatching, (P, n, tuple(starts), ratio), dev, lambda: SceneMatching(P, n, starts, ratio, dev))
    out.gt_inliers, out.gt_flag = gt_inliers, gt_flag
    c_ratio = _lib.C.c_double(ratio)
    rc = lib.d3f_matching_summary(_ptr(mutual_count), _ptr(gt_inliers), _ptr(gt_flag), P, n, _lib.C.addressof(c_starts), out.S,
                                  _lib.C.addressof(c_ratio), _ptr(out.ratio_e8), _ptr(out.figures), ops._stream(dev))
    _lib.check(rc, "matching_summary")
    return out


class SceneMatches:
    """Result of match_scenes: `matching` (PairMatching of match_pairs) and `summary` (SceneMatching of matching_summary), both device
    tensors."""

    def __init__(self, matching, summary):
        self.matching, self.summary = matching, summary


def match_scenes(kp, count, pairs, gt, gt_flag, scene_start, num_keypts=EVALUATE_ETH["num_keypts"],
                 distance_threshold=EVALUATE_ETH["distance_threshold"], inlier_ratio=EVALUATE_ETH["inlier_ratio"], nan_to_num=True, out=None):
    """geometric_registration_eth/evaluate_eth.py for every pair of every scene in one call: kp f32[n_blocks, K, 4 + C] / count the
    keypoint blocks of ALL scenes (stack_keypoints), pairs i32[P, 2] global block indices with the scenes contiguous, gt f32[P, 3, 4]
    target -> source, gt_flag i32[P], scene_start as matching_summary takes it (datasets.eth.benchmark makes the four).
    sanitize_descriptors(kp) -- IN PLACE, skipped with nan_to_num=False --, match_pairs and matching_summary, no read-back in between
    (capturable: pass the previous result as `out`).  -> SceneMatches (.matching, .summary)."""
    if out is not None and not isinstance(out, SceneMatches):
        raise _another_call("match_scenes")
    if nan_to_num:
        sanitize_descriptors(kp)
    m = match_pairs(kp, count, pairs, gt, num_keypts=num_keypts, distance_threshold=distance_threshold,
                    out=out.matching if out is not None else None)
    s = matching_summary(m, gt_flag, scene_start, inlier_ratio=inlier_ratio, out=out.summary if out is not None else None)
    return out if out is not None else SceneMatches(m, s)


# ---- the 3DMatch registration benchmark: registration recall of every scene in one call (geometric_registration/3dmatch/evaluate.m) ---
RECALL_3DMATCH = dict(err2=0.04)                                               # mrEvaluateRegistration.m:2-4 (0.2 ^ 2)
RECALL_GOOD, RECALL_RESULT, RECALL_FALSE_POS, RECALL_GT = 1, 2, 4, 8           # the bits of SceneRecall.flags
RECALL_FIGURES = ("good", "bad", "false_pos", "gt_num", "rs_num")


def _round_half_away(x):
    """MATLAB's round for x >= 0 (evaluate.m:45)."""
    f = int(np.floor(x))
    return f + (1 if x - f >= 0.5 else 0)


class SceneRecall(_PairResult):
    """Result of registration_recall: DEVICE tensors error f64[P, n] (the transformation error p of mrComputeTransformationError where
    the pair has a result and a ground truth and is not consecutive, 0 elsewhere; NaN kept), flags i32[P, n] (bit 0: good, bit 1:
    counted in rs_num, bit 2: false positive, bit 3: counted in gt_num) and figures i64[S, n, 5] (per scene and count: good, bad,
    false_pos, gt_num, rs_num); n is 1 for a [P, 3, 4] / [P, 4, 4] input (error and flags are then [P]).  .host(), .scenes(),
    .overall(c) and .failed(c) share one read-back."""
    FIELDS = ("error", "flags", "figures", "ids")

    def __init__(self, P, n, flat, scene_start, err2, logged, device):
        self.P, self.n, self.flat, self.scene_start = P, n, flat, tuple(int(v) for v in scene_start)
        self.err2, self.logged, self.S = float(err2), bool(logged), len(self.scene_start) - 1
        self.key = (P, n, flat, self.scene_start, self.err2, self.logged)
        shape = (P,) if flat else (P, n)
        self.error = torch.empty(shape, dtype=torch.float64, device=device)
        self.flags = torch.empty(shape, dtype=torch.int32, device=device)
        self.figures = torch.empty((self.S, n, 5), dtype=torch.int64, device=device)
        self.ids = None                                         # an input of the call, kept for the read-back

    def _read(self, name):
        a = super()._read(name)
        return a if name == "figures" else a.reshape(self.P, 2 if name == "ids" else self.n)

    def host(self):
        """One read-back of the whole result, kept until the next registration_recall(out=self): dict of numpy arrays error [P, n],
        flags [P, n], figures [S, n, 5] and ids [P, 2]."""
        return self._host()

    def scenes(self):
        """[scene][count] -> dict(good, bad, false_pos, gt_num, rs_num, recall, precision): the integers of `figures`, recall = good /
        gt_num and precision = good / rs_num as FRACTIONS (mrEvaluateRegistration.m:38-39), 0.0 where MATLAB would divide by zero."""
        fig = self.host()["figures"]
        out = []
        for s in range(self.S):
            per_count = []
            for c in range(self.n):
                r = {k: int(v) for k, v in zip(RECALL_FIGURES, fig[s, c])}
                r["recall"] = r["good"] / r["gt_num"] if r["gt_num"] else 0.0
                r["precision"] = r["good"] / r["rs_num"] if r["rs_num"] else 0.0
                per_count.append(r)
            out.append(per_count)
        return out

    def overall(self, c=0):
        """The closing figures of evaluate.m:41-48 at count c: dict(recall_list, mean_recall, mean_precision = the means over the scenes,
        total_tp = the sum of round(gt_num * recall), total_gt, true_recall = total_tp / total_gt)."""
        sc = [per_count[c] for per_count in self.scenes()]
        mean = lambda key: sum(r[key] for r in sc) / len(sc) if sc else 0.0
        tp, gt = sum(_round_half_away(r["gt_num"] * r["recall"]) for r in sc), sum(r["gt_num"] for r in sc)
        return dict(recall_list=[r["recall"] for r in sc], mean_recall=mean("recall"), mean_precision=mean("precision"), total_tp=tp,
                    total_gt=gt, true_recall=tp / gt if gt else 0.0)

    def failed(self, c=0):
        """[(scene, id1, id2, p)] of the bad rows of count c, in pair order: a result for a listed, non-consecutive pair whose error is
        above err2 (or NaN)."""
        h = self.host()
        out = []
        for s in range(self.S):
            for p in range(self.scene_start[s], self.scene_start[s + 1]):
                if h["flags"][p, c] & (RECALL_GOOD | RECALL_RESULT | RECALL_FALSE_POS) == RECALL_RESULT:
                    out.append((s, int(h["ids"][p, 0]), int(h["ids"][p, 1]), float(h["error"][p, c])))
        return out


def registration_recall(T, gt, info, gt_flag, ids, scene_start, err2=RECALL_3DMATCH["err2"], result_flag=None, logged=False, out=None):
    """The registration recall of the 3DMatch benchmark (geometric_registration/3dmatch/evaluate.m with mrEvaluateRegistration.m) for
    every scene in one call.  T: f32[P, 3, 4] / f32[P, n, 3, 4] estimates source -> target, or the PairRegistration /
    PairRegistrationCounts that holds them -- widened to float64 and inverted on the device, as evaluate.py:104 logs the inverse --, or
    with logged=True f64[P, 4, 4] / f64[P, n, 4, 4] matrices as a .log file holds them (results.read_result_log), not inverted.
    gt f64[P, 4, 4] the gt.log matrix (target -> source, register_pairs' direction), info f64[P, 6, 6] the gt.info matrix, gt_flag
    i32[P] (1 where gt.log lists the pair), result_flag i32[P] (1 where the pair has a result; None: gt_flag, what evaluate.py logs),
    ids i32[P, 2] the fragment numbers of the pair inside its scene -- all on the device (datasets.threedmatch.benchmark makes them);
    scene_start as matching_summary takes it.  Per row the error p = er' info er / info[0][0] of gt^-1 * result in float64 (NaN kept, a
    bad row) and four flags, per scene and count five integer sums.  Two launches whatever P is, no read-back (capturable: pass the
    previous result as `out`).  -> SceneRecall (device tensors; .host(), .scenes(), .overall(c), .failed(c))."""
    lib = _lib.load()
    if isinstance(T, (PairRegistration, PairRegistrationCounts)):
        T = T.T
    T = ops._req(T, torch.float64 if logged else torch.float32, "T")
    tail = (4, 4) if logged else (3, 4)
    if T.dim() not in (3, 4) or tuple(T.shape[-2:]) != tail or not T.is_contiguous():
        raise ValueError("registration_recall: T of shape %s (contiguous [P, %d, 4] or [P, n, %d, 4])" % (tuple(T.shape), tail[0], tail[0]))
    dev, P, flat = T.device, T.shape[0], T.dim() == 3
    n = 1 if flat else T.shape[1]
    gt = ops._req(gt, torch.float64, "gt", 3)
    info = ops._req(info, torch.float64, "info", 3)
    gt_flag = ops._req(gt_flag, torch.int32, "gt_flag", 1)
    ids = ops._req(ids, torch.int32, "ids", 2)
    if result_flag is not None:
        result_flag = ops._req(result_flag, torch.int32, "result_flag", 1)
    if (tuple(gt.shape) != (P, 4, 4) or tuple(info.shape) != (P, 6, 6) or gt_flag.shape[0] != P or tuple(ids.shape) != (P, 2)
            or (result_flag is not None and result_flag.shape[0] != P) or not 1 <= n <= _lib.REPEAT_COUNTS_MAX
            or not all(t.is_contiguous() for t in (gt, info, gt_flag, ids) + ((result_flag,) if result_flag is not None else ()))):
        raise ValueError("registration_recall: gt %s, info %s, gt_flag %s, ids %s for T %s (contiguous [P, 4, 4], [P, 6, 6], [P], [P, 2])"
                         % (tuple(gt.shape), tuple(info.shape), tuple(gt_flag.shape), tuple(ids.shape), tuple(T.shape)))
    starts, c_starts = _scene_starts("registration_recall", scene_start, P)
    e2 = float(err2)
    if not e2 > 0.0:
        raise ValueError("registration_recall: err2 %r" % (err2,))
    out = _reuse("registration_recall", out, SceneRecall, (P, n, flat, tuple(starts), e2, bool(logged)), dev,
                 lambda: SceneRecall(P, n, flat, starts, e2, logged, dev))
    out.ids = ids
    c_err2 = _lib.C.c_double(e2)
    rc = lib.d3f_registration_recall(_ptr(T), 1 if logged else 0, _ptr(gt), _ptr(info), _ptr(gt_flag), _ptr(result_flag), _ptr(ids), P, n,
                                     _lib.C.addressof(c_starts), out.S, _lib.C.addressof(c_err2), _ptr(out.error), _ptr(out.flags),
                                     _ptr(out.figures), ops._stream(dev))
    _lib.check(rc, "registration_recall")
    return out


class SceneRegistration:
    """Result of register_scenes: `registration` (PairRegistration of register_pairs, or PairRegistrationCounts of
    register_pairs_counts for a tuple of counts), `matching` (SceneMatching of matching_summary on its mutual_count / gt_inliers) and
    `recall` (SceneRecall of registration_recall on its T), all device tensors; gt32 is the float32 ground truth RANSAC was given."""

    def __init__(self, registration, matching, recall, gt32):
        self.registration, self.matching, self.recall, self.gt32 = registration, matching, recall, gt32
        self.T = registration.T


def register_scenes(kp, count, pairs, gt, info, gt_flag, ids, scene_start, num_keypts=250, seed=0,
                    distance_threshold=0.10, inlier_ratio=0.05, err2=RECALL_3DMATCH["err2"], nan_to_num=True, out=None):
    """The 3DMatch benchmark for every pair of every scene in one call: geometric_registration/evaluate.py (np.nan_to_num of the
    descriptors, :43-44; the mutual matches and their inliers under gt, :67-82; RANSAC, :93-99) and 3dmatch/evaluate.m (registration
    recall).  kp f32[n_blocks, K, 4 + C] / count the keypoint blocks of ALL scenes (stack_keypoints), pairs i32[P, 2] global block
    indices with the scenes contiguous, gt f64[P, 4, 4] (target -> source), info f64[P, 6, 6], gt_flag i32[P], ids i32[P, 2] and
    scene_start as registration_recall takes them (datasets.threedmatch.benchmark makes the six).  sanitize_descriptors(kp) -- IN
    PLACE, skipped with nan_to_num=False --, then register_pairs(num_keypts, gt rounded to float32, **EVALUATE_3DMATCH) for one count or
    register_pairs_counts for a tuple of counts, matching_summary on its mutual_count / gt_inliers and registration_recall on its T; no
    read-back in between (capturable: pass the previous result as `out`).  T and the matching figures are bit-equal to the
    stand-alone calls.  -> SceneRegistration (.registration, .matching, .recall): both recalls of every scene at every count."""
    if out is not None and not isinstance(out, SceneRegistration):
        raise _another_call("register_scenes")
    gt = ops._req(gt, torch.float64, "gt", 3)
    if tuple(gt.shape[1:]) != (4, 4):
        raise ValueError("register_scenes: gt of shape %s ([P, 4, 4])" % (tuple(gt.shape),))
    many = isinstance(num_keypts, (tuple, list))
    if out is not None and isinstance(out.registration, PairRegistrationCounts) != many:
        raise _another_call("register_scenes")
    if nan_to_num:
        sanitize_descriptors(kp)
    if out is not None:
        gt32 = out.gt32.copy_(gt[:, :3])                         # (plumbing: the rounding of the ground truth, in place under capture)
    else:
        gt32 = gt[:, :3].to(torch.float32).contiguous()
    kw = dict(seed=seed, gt=gt32, distance_threshold=distance_threshold, out=out.registration if out is not None else None, **EVALUATE_3DMATCH)
    if many:
        reg = register_pairs_counts(kp, count, pairs, num_keypts=tuple(num_keypts), **kw)
    else:
        reg = register_pairs(kp, count, pairs, num_keypts=int(num_keypts), **kw)
    m = matching_summary(reg.mutual_count, reg.gt_inliers, gt_flag, scene_start, inlier_ratio=inlier_ratio,
                         out=out.matching if out is not None else None)
    r = registration_recall(reg.T, gt, info, gt_flag, ids, scene_start, err2=err2, out=out.recall if out is not None else None)
    return out if out is not None else SceneRegistration(reg, m, r, gt32)
