"""Which fragments of a scene overlap, and where: the data preparation of datasets/cal_overlap.py:78-126 on the MI355X.

    stack_fragments(clouds, poses)          the posed fragments of a scene as one stack in the common frame (cal_overlap.py:53-59,108-109)
    overlap_pairs(points, lens, pairs, thr) for every pair (a, b): the points of a whose nearest point of b is closer than thr -- their
                                            number (the overlap ratio is count / len(a), :116) and, when asked for, the index pairs
                                            themselves (keypts_pairs, :122); two launches per PAIRS_PER_CALL pairs, capturable
    PairOverlap                             the device tensors of a call; .ratios() / .selected() / .matches(p) for the reference's figures

The reference runs cv2.BFMatcher over every pair: a brute-force 30 k x 30 k search each.  Here ONE cell grid over the whole stack
(ops.NeighborGrid: every fragment its own element) serves all pairs, and its cell-sorted records are the queries as well
(d3f_overlap_pairs, csrc/nb_overlap.h).  numpy / torch only move data.
"""
import numpy as np
import torch

from . import _lib, ops
from . import registration

OVERLAP_3DMATCH = dict(threshold=0.025, min_ratio=0.30)       # cal_overlap.py:112,121,138: the voxel size, and the pairs kept


def stack_fragments(clouds, poses=None, device=None):
    """A list of [n_i, 3] clouds (numpy or tensors) -> (points f32[N, 3], lens i32[n]) on the device.  poses: one 4 x 4 matrix per
    cloud taking the fragment into the world; each cloud becomes R x + t in float64 and is then cast to float32, as the reference
    transforms the downsampled cloud (cal_overlap.py:57-58) and casts it (:108-109)."""
    if poses is not None and len(poses) != len(clouds):
        raise ValueError("stack_fragments: %d clouds, %d poses" % (len(clouds), len(poses)))
    out = []
    for f, c in enumerate(clouds):
        c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        c = c.reshape(-1, 3)
        if poses is not None:
            M = np.asarray(poses[f], np.float64)
            c = c.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        out.append(c.astype(np.float32))
    dev = registration._dev(device)
    pts = np.concatenate(out, 0) if out else np.zeros((0, 3), np.float32)
    return torch.from_numpy(np.ascontiguousarray(pts)).to(dev), ops.as_lens([len(c) for c in out], dev)


class PairOverlap(registration._PairResult):
    """Result of overlap_pairs: DEVICE tensors, one row per pair.  count i32[P] (points of the source with a target point strictly
    inside the threshold; -1: a fragment index outside the stack), src_len i32[P] (points of the source), nearest i32[P, ld] when
    asked for (per source point the index inside the target of its nearest point, -1: none; -1 from src_len on)."""
    FIELDS = ("count", "src_len", "nearest")

    def __init__(self, P, ld, device):
        self.P, self.ld = P, ld
        self.key = (P, ld is not None)
        self.count = torch.empty((P,), dtype=torch.int32, device=device)
        self.src_len = torch.empty((P,), dtype=torch.int32, device=device)
        self.nearest = torch.empty((P, ld), dtype=torch.int32, device=device) if ld is not None else None
        self.grid = None

    def ratios(self):
        """f64[P]: count / src_len, the overlap ratio of cal_overlap.py:116; 0 for an empty source."""
        h = self._host()
        n = h["src_len"].astype(np.float64)
        return np.where(n > 0, h["count"].astype(np.float64) / np.maximum(n, 1.0), 0.0)

    def selected(self, min_ratio=OVERLAP_3DMATCH["min_ratio"]):
        """Rows whose ratio is strictly above min_ratio (cal_overlap.py:121) -> i64 row numbers, ascending."""
        return np.nonzero(self.ratios() > float(min_ratio))[0]

    def matches(self, p):
        """i32[M, 2]: the [queryIdx, trainIdx] rows of pair p in ascending query index -- what keypts_pairs holds (cal_overlap.py:
        82-85,122).  Needs nearest=True."""
        h = self._host()
        if "nearest" not in h:
            raise ValueError("PairOverlap.matches: the call was made without nearest=True")
        near = h["nearest"][p, :max(int(h["src_len"][p]), 0)]
        sel = np.nonzero(near >= 0)[0]
        return np.stack([sel, near[sel]], 1).astype(np.int32)


def overlap_pairs(points, lens, pairs=None, threshold=OVERLAP_3DMATCH["threshold"], nearest=False, grid=None, out=None):
    """Overlap of P pairs of fragments in one call: points f32[N, 3], the fragments stacked in one common frame (stack_fragments),
    lens i32[n] their lengths, pairs i32[P, 2] (source, target) fragment indices (default: registration.scene_pairs(n), every pair
    a < b), all on the device.  For each pair the points of the source whose nearest target point is strictly closer than `threshold`
    are counted (fp32, the metric of every search of this library, ties to the lowest target index).  One cell grid over the stack is
    built (ops.NeighborGrid(points, lens, threshold): five launches) unless `grid` is one built over these points with a radius >=
    threshold; then two launches per PAIRS_PER_CALL pairs, no read-back and no host decision (capturable: pass the previous result
    as `out`).  nearest=True also keeps, per pair, the matched target index of every source point in an i32[P, max(lens)] tensor:
    pass only the pairs whose matches are wanted (the selected ones of a first call), not all of a scene.
    -> PairOverlap (device tensors; .ratios() / .selected() / .matches(p) for the reference's figures)."""
    lib = _lib.load()
    n = int(lens.numel()) if isinstance(lens, torch.Tensor) else len(lens)
    if not 1 <= n <= _lib.MAX_BATCH:
        raise ValueError("overlap_pairs: %d fragments; one stack holds 1 to %d (D3F_MAX_BATCH)" % (n, _lib.MAX_BATCH))
    thr = float(threshold)
    if not (thr > 0.0 and np.isfinite(thr)):
        raise ValueError("overlap_pairs: threshold %r" % (threshold,))
    if grid is not None and not grid.radius >= thr:
        raise ValueError("overlap_pairs: the grid was built for radius %g, below the threshold %g" % (grid.radius, thr))
    points = ops._req(points, torch.float32, "points", 2)
    dev = points.device
    if points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError("overlap_pairs: points must be contiguous [N, 3] (got %s)" % (tuple(points.shape),))
    lens = ops.as_lens(lens, dev)
    if pairs is None:
        pairs = registration.scene_pairs(n, device=dev)
    pairs = ops._req(pairs, torch.int32, "pairs", 2)
    if pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise ValueError("overlap_pairs: pairs must be contiguous [P, 2]")
    N, P = points.shape[0], pairs.shape[0]
    if grid is None:
        grid = ops.NeighborGrid(points, lens, thr)
    elif grid.Ns != N or grid.B != n or grid.supports.data_ptr() != points.data_ptr():
        raise ValueError("overlap_pairs: the grid was not built over these points")
    out = registration._reuse("overlap_pairs", out, PairOverlap, (P, bool(nearest)), dev,
                              lambda: PairOverlap(P, max(max(ops.host_lens(lens)), 1) if nearest else None, dev))
    if nearest and getattr(lens, "host_lens", None) is not None and max(lens.host_lens) > out.ld:
        # (lengths known on the host only: a device-only lens tensor is not read back here, the kernel then keeps to the row)
        raise ValueError("overlap_pairs: out= holds %d matches per pair, the longest fragment %d points" % (out.ld, max(lens.host_lens)))
    out.grid = grid                                            # (a captured call keeps reading this grid's memory)
    # length of every pair's source (plumbing for ratios(); a fragment index outside the stack: 0)
    a = pairs[:, 0].long()
    torch.mul(lens[a.clamp(0, n - 1)], ((a >= 0) & (a < n)).to(torch.int32), out=out.src_len)
    st = ops._stream(dev)
    for s in registration._chunks(P):
        rc = lib.d3f_overlap_pairs(grid.mem.data_ptr(), grid.nbytes, N, n, pairs[s].data_ptr(), s.stop - s.start, thr,
                                   out.count[s].data_ptr(), out.nearest[s].data_ptr() if nearest else None,
                                   out.ld if nearest else 0, st)
        _lib.check(rc, "overlap_pairs")
    return out
