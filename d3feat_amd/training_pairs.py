"""What a training step consumes, made on the MI355X: the correspondences, the sample and the augmentation of every pair in one call.

    training_pairs(points, lens, trans=..., radius=..., keypts_num=...)          the KITTI form: every positive point strictly inside
                                            `radius` of a moved anchor point is a match (datasets/KITTI.py:35-48); keypts_num distinct
                                            ones are drawn (:186) -- without the list ever being stored
    training_pairs(points, lens, keypts_pairs=..., pair_start=...)               the 3DMatch form: keypts_num rows of the pair's
                                            precomputed list with replacement (datasets/ThreeDMatch.py:222-229)
    both: noise, rotation, scale and shift of every row (KITTI.py:192-206, ThreeDMatch.py:266-273), backup_points, and the index lists
    in the convention validation.loss_gradients documents
    training_flat_inputs(dataset, config, result, p)                             one pair's flat_inputs for KernelPointFCNN.run

The definition -- the counter-based draws and their streams, the order of the matches, Floyd's algorithm, the fp32 arithmetic of the
row pass -- is in include/d3feat_amd.h (d3f_training_pairs); tests/training_pairs_np.py is the same text in numpy.  The stack holds
2 P clouds: cloud 2 p the anchor, cloud 2 p + 1 the positive (the convention of registration.register_kitti_pairs).  numpy / torch
only move data.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from . import registration

# training_KITTI.py:125-132 / training_3DMatch.py:125-131 of the reference
AUGMENT_KITTI = dict(augment_noise=0.01, augment_rotation=1, augment_scale_min=0.8, augment_scale_max=1.2, augment_shift_range=2.0)
AUGMENT_3DMATCH = dict(augment_noise=0.005, augment_rotation=1, augment_scale_min=1.0, augment_scale_max=1.0, augment_shift_range=0.0)
# datasets/KITTI.py:72 (matching_search_voxel_size = first_subsampling_dl * 1.5), :186, :324
MATCHING_KITTI = dict(radius=1.5 * 0.30, keypts_num=1024, min_matches=1024)

STREAM_NOISE, STREAM_ROTATION, STREAM_SCALE, STREAM_SHIFT, STREAM_SAMPLE = 0, 2, 4, 6, 8
FEW_MATCHES, BELOW_KEYPTS, LIST_RANGE = 1, 2, 4
PAIRS_PER_CALL = _lib.MAX_BATCH // 2


def training_draw(seed, step, pair, stream, counter):
    """The 64-bit draw of (seed, step, pair, stream, counter): the host copy of what the kernels use (d3f_training_draw)."""
    out = ctypes.c_uint64()
    _lib.check(_lib.load().d3f_training_draw(int(seed), int(step), int(pair), int(stream), int(counter), ctypes.byref(out)), "training_draw")
    return int(out.value)


class TrainingPairs(registration._PairResult):
    """Result of training_pairs: DEVICE tensors.  points f32[N, 3] (the augmented rows), backup f32[N, 3] (the pair in one frame, not
    augmented), anc_idx / pos_idx i32[P, keypts_num] (indices into the pair's own rows, the positive's shifted by the anchor's length;
    only the first n[p] of a row are written), n i32[P], row0 i32[P + 1], matches i32[P] (M; the list's length in the 3DMatch form),
    status i32[P] (FEW_MATCHES | BELOW_KEYPTS | LIST_RANGE: such a pair has n = 0), params f32[2 P, 16] (per cloud: R, scale, shift,
    first angle, first axis, rotation mode), step u64[1] (the step the NEXT call draws with), lens i32[2 P], trans."""
    FIELDS = ("n", "row0", "matches", "status", "anc_idx", "pos_idx", "params")

    def __init__(self, N, P, keypts_num, device, points=None):
        self.key = (N, P, keypts_num)
        self.N, self.P, self.keypts_num = N, P, keypts_num
        self.points = points if points is not None else torch.empty((N, 3), dtype=torch.float32, device=device)
        self.backup = torch.empty((N, 3), dtype=torch.float32, device=device)
        self.anc_idx = torch.empty((P, keypts_num), dtype=torch.int32, device=device)
        self.pos_idx = torch.empty((P, keypts_num), dtype=torch.int32, device=device)
        self.n = torch.empty((P,), dtype=torch.int32, device=device)
        self.row0 = torch.empty((P + 1,), dtype=torch.int32, device=device)
        self.matches = torch.empty((P,), dtype=torch.int32, device=device)
        self.status = torch.empty((P,), dtype=torch.int32, device=device)
        self.params = torch.empty((2 * P, 16), dtype=torch.float32, device=device)
        self.step = torch.zeros((1,), dtype=torch.int64, device=device)       # (the bits of a u64)
        self.lens = self.trans = self.grid = None
        self._ws = []

    def host(self):
        """The small tensors on the host (one read-back, kept until the next call with out=self)."""
        return self._host()


def _augment(augment):
    a = dict(AUGMENT_KITTI if augment is None else augment)
    try:
        return (float(a["augment_noise"]), int(a["augment_rotation"]), float(a["augment_scale_min"]), float(a["augment_scale_max"]),
                float(a["augment_shift_range"]))
    except KeyError as e:
        raise ValueError("training_pairs: augment lacks %s" % e)


def training_pairs(points, lens, trans=None, keypts_pairs=None, pair_start=None, radius=MATCHING_KITTI["radius"],
                   keypts_num=MATCHING_KITTI["keypts_num"], min_matches=1024, seed=0, step=None, augment=AUGMENT_KITTI, grid=None, out=None,
                   first_pair=0):
    """points f32[N, 3] (device, contiguous): 2 P stacked clouds, lens their lengths (cloud 2 p the anchor, 2 p + 1 the positive).
    KITTI form: trans f32[P, 4, 4] (device; source to target) and `radius`; one cell grid over the stack is built unless `grid` is one
    built over these points with a radius >= `radius`.  3DMatch form: keypts_pairs i32[L, 2] and pair_start i32[P + 1] (device).
    keypts_num (at most 1024) indices per pair; a pair with fewer than min_matches (or keypts_num) matches is flagged in .status and
    gets n = 0.  augment: AUGMENT_KITTI / AUGMENT_3DMATCH or a dict of the same keys (augment_rotation 0, 1 or 3).
    seed, step: every draw is a pure function of (seed, step, first_pair + p, stream, counter).  step=None: the device counter .step of
    `out` (0 for a new result), which the call advances by one -- a captured call draws afresh on every replay; an int overrides it.
    out: the previous result of the same sizes (its tensors are written again; needed for capture); out.points may have been made by
    the caller (TrainingPairs(N, P, keypts_num, device, points=buffer)) so that the augmented rows land where an engine reads them.
    More than 127 pairs are run in chunks (the lengths, and without step= the device counter, are then read on the host); otherwise
    there is no read-back.  -> TrainingPairs."""
    lib = _lib.load()
    points = ops._req(points, torch.float32, "points", 2)
    dev = points.device
    if points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError("training_pairs: points must be contiguous [N, 3] (got %s)" % (tuple(points.shape),))
    lens = ops.as_lens(lens, dev)
    N, B = int(points.shape[0]), int(lens.numel())
    if B < 2 or B % 2:
        raise ValueError("training_pairs: %d clouds; a stack holds the anchor and the positive of every pair" % B)
    P, k = B // 2, int(keypts_num)
    if not 1 <= k <= _lib.TRAINING_KEYPTS_MAX:
        raise ValueError("training_pairs: keypts_num %d outside 1 .. %d" % (k, _lib.TRAINING_KEYPTS_MAX))
    by_radius = keypts_pairs is None
    if by_radius:
        if trans is None or pair_start is not None:
            raise ValueError("training_pairs: pass trans (the radius form) or keypts_pairs and pair_start (the list form)")
        r = float(radius)
        if not (r > 0.0 and np.isfinite(r)):
            raise ValueError("training_pairs: radius %r" % (radius,))
        trans = ops._req(trans, torch.float32, "trans", 3)
        if tuple(trans.shape) != (P, 4, 4) or not trans.is_contiguous():
            raise ValueError("training_pairs: trans of shape %s for %d pairs" % (tuple(trans.shape), P))
        if grid is not None and (not grid.radius >= r or grid.Ns != N or grid.B != B or grid.supports.data_ptr() != points.data_ptr()):
            raise ValueError("training_pairs: the grid was not built over these points with a radius >= %g" % r)
        L = 0
    else:
        if pair_start is None or trans is not None or grid is not None:
            raise ValueError("training_pairs: the list form takes keypts_pairs and pair_start, no trans and no grid")
        keypts_pairs = ops._req(keypts_pairs, torch.int32, "keypts_pairs", 2)
        pair_start = ops._req(pair_start, torch.int32, "pair_start", 1)
        if keypts_pairs.shape[1] != 2 or not keypts_pairs.is_contiguous() or not pair_start.is_contiguous() or pair_start.numel() != P + 1:
            raise ValueError("training_pairs: keypts_pairs must be contiguous [L, 2], pair_start hold %d offsets" % (P + 1))
        r, L = 0.0, int(keypts_pairs.shape[0])
    noise, rotation, smin, smax, shift = _augment(augment)
    if rotation not in (0, 1, 3):
        raise ValueError("training_pairs: augment_rotation %d is none of 0, 1, 3" % rotation)
    out = registration._reuse("training_pairs", out, TrainingPairs, (N, P, k), dev, lambda: TrainingPairs(N, P, k, dev))
    if out.points.data_ptr() == points.data_ptr() and N:
        raise ValueError("training_pairs: the augmented rows cannot overwrite the input")
    out.lens, out.trans = lens, trans
    if P <= PAIRS_PER_CALL:
        chunks = [(0, P, 0, N)]
    else:
        offs = np.concatenate([[0], np.cumsum(np.maximum(np.asarray(ops.host_lens(lens), np.int64), 0))])
        chunks = [(a, min(a + PAIRS_PER_CALL, P)) for a in range(0, P, PAIRS_PER_CALL)]
        chunks = [(a, b, int(min(offs[2 * a], N)), int(min(offs[2 * b], N))) for a, b in chunks]
        if grid is not None:
            raise ValueError("training_pairs: %d pairs run in chunks, each with a grid of its own" % P)
    if len(out._ws) != len(chunks):
        out._ws = [None] * len(chunks)
    out.grid = []
    st = ops._stream(dev)
    use_host = step is not None
    step0 = int(step) if use_host else 0
    if not use_host and len(chunks) > 1:
        # every chunk draws with the same step: the device counter is read once, the last chunk stores its successor
        use_host, step0 = True, int(out.step.item()) & 0xFFFFFFFFFFFFFFFF
    for c, (a, b, r0, r1) in enumerate(chunks):
        n_rows, Pc = r1 - r0, b - a
        last = c == len(chunks) - 1
        rows = points[r0:r1]
        g = None
        if by_radius:
            g = grid if grid is not None else ops.NeighborGrid(rows, lens[2 * a:2 * b], r)
            out.grid.append(g)                                       # (a captured call keeps reading this grid's memory)
        wsb = lib.d3f_training_pairs_workspace_bytes(n_rows, Pc, k)
        if out._ws[c] is None or out._ws[c].numel() < wsb:
            out._ws[c] = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        # (an empty list has no address; the entry point wants one and reads nothing through it: every pair is then flagged)
        rc = lib.d3f_training_pairs(g.mem.data_ptr() if g is not None else None, g.nbytes if g is not None else 0,
                                    registration._ptr(rows), n_rows, lens[2 * a:2 * b].data_ptr(), Pc,
                                    trans[a:b].data_ptr() if by_radius else None,
                                    None if by_radius else (registration._ptr(keypts_pairs) or out.anc_idx.data_ptr()), L,
                                    None if by_radius else pair_start[a:b + 1].data_ptr(), r, k, int(min_matches), int(seed),
                                    out.step.data_ptr() if last else None, 1 if use_host else 0, step0, int(first_pair) + a,
                                    noise, rotation, smin, smax, shift, registration._ptr(out.points[r0:r1]),
                                    registration._ptr(out.backup[r0:r1]), out.anc_idx[a:b].data_ptr(), out.pos_idx[a:b].data_ptr(), k,
                                    out.n[a:b].data_ptr(), out.row0[a:b + 1].data_ptr(), out.matches[a:b].data_ptr(),
                                    out.status[a:b].data_ptr(), out.params[2 * a:2 * b].data_ptr(), out._ws[c].data_ptr(), wsb, st)
        _lib.check(rc, "training_pairs")
        if r0:
            out.row0[a:b + 1] += r0                                  # (a chunk numbers its rows from its own first one)
    out._inputs = (points, lens, trans, keypts_pairs, pair_start)    # (a captured call keeps reading these)
    return out


def training_flat_inputs(dataset, config, pairs_result, p, ids=None):
    """The flat_inputs of pair p for KernelPointFCNN.run, through dataset.tf_descriptor_input on the device tensors of a training_pairs
    result: the pyramid over the pair's augmented rows, then [stack_lengths, anc_keypts, pos_keypts, ids, backup_points] and -- radius
    form -- trans (datasets/KITTI.py:245-254).  The pair's lengths and n are read on the host (the pyramid's shapes depend on them)."""
    r = pairs_result
    lens = [max(int(x), 0) for x in ops.host_lens(r.lens)[2 * p:2 * p + 2]]
    h = r.host()
    a0, n = int(h["row0"][p]), int(h["n"][p])
    rows = r.points[a0:a0 + lens[0] + lens[1]]
    dev = rows.device
    stack_lengths = ops.as_lens(lens, dev)
    ones = torch.ones((rows.shape[0], 1), dtype=torch.float32, device=dev)
    li = dataset.tf_descriptor_input(config, rows, ones, stack_lengths, dataset.tf_get_batch_inds(stack_lengths))
    ids = list(ids) if ids is not None else ["pair_%d_anc" % p, "pair_%d_pos" % p]
    flat = li + [stack_lengths, r.anc_idx[p, :n], r.pos_idx[p, :n], ids, r.backup[a0:a0 + lens[0] + lens[1]]]
    if r.trans is not None:
        flat.append(r.trans[p])
    return flat
