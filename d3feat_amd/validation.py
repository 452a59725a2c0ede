"""Validation figures of a split on the MI355X: what the reference's model class evaluates per validation pair (models/
KPFCNN_model.py:131-186 with utils/loss.py -- desc_loss, det_loss, accuracy, ave_d_pos, ave_d_neg) and what utils/trainer.py:417-498
makes of them.  Forward only: no gradient, no regularisation loss.

    validation_pairs(features, scores, points, anc_idx, pos_idx, n, row0)   P pairs in one call (three launches, capturable)
    validation_records(records, lens, anc_idx, pos_idx, n)                 the same on packed [xyz | desc | score] records
    PairValidation                                                         the device tensors of a call; .means() / .line()
    VALIDATION_3DMATCH / VALIDATION_KITTI                                  safe_radius, keypts_num, det_loss_weight of training_*.py

The reference materialises all n x n x C descriptor differences (cdist) twice per pair; d3f_validation_pairs (csrc/rp_validation.h)
keeps four numbers per anchor row instead.  numpy / torch only move data here.
"""
import numpy as np
import torch

from . import _lib, ops
from .registration import _PairResult, _reuse

VALIDATION_3DMATCH = dict(safe_radius=0.1, keypts_num=256, det_loss_weight=1.0)      # training_3DMatch.py
VALIDATION_KITTI = dict(safe_radius=1.0, keypts_num=1024, det_loss_weight=1.0)       # training_KITTI.py
POS_MARGIN, NEG_MARGIN, LOG_SCALE = 0.1, 1.4, 25.0                                   # KPFCNN_model.py:159-160, loss.py:157
FIGURES = ("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg")            # columns 0..5 of PairValidation.values
SKIP = (0.0, 0.0, -1.0, 0.0, 0.0)                                                    # KPFCNN_model.py:179-184


class PairValidation(_PairResult):
    """Result of validation_pairs: DEVICE tensors.  values f32[P, 8] (circle, contrastive, det, accuracy, d_pos, d_neg, accurate rows,
    n), status i32[P] (0; _lib.VP_INDEX_RANGE: an index outside the pair's rows; _lib.VP_COUNT_RANGE: n outside 0 .. the list length /
    1024 -- both give the skip tuple), sums f64[6] / counts i64[6]: per figure the sum over the pairs where it is != 0 (accuracy: > 0)
    and how many those are.  loss: which descriptor loss is THE desc_loss of means() / line(): 'circle_loss' (what the model class
    uses, KPFCNN_model.py:157) or 'desc_loss' (the contrastive entry of LOSS_CHOICES)."""
    FIELDS = ("values", "status", "sums", "counts")

    def __init__(self, P, device, loss="circle_loss"):
        if loss not in ("circle_loss", "desc_loss"):
            raise ValueError("PairValidation: loss %r is neither 'circle_loss' nor 'desc_loss'" % (loss,))
        self.P, self.loss = P, loss
        self.key = (P,)
        self.values = torch.empty((P, 8), dtype=torch.float32, device=device)
        self.status = torch.empty((P,), dtype=torch.int32, device=device)
        self.sums = torch.empty((6,), dtype=torch.float64, device=device)
        self.counts = torch.empty((6,), dtype=torch.int64, device=device)

    def figures(self, p=0):
        """(desc_loss, det_loss, accuracy, ave_d_pos, ave_d_neg) of pair p as device scalars: the model's five outputs."""
        v = self.values[p]
        return v[0 if self.loss == "circle_loss" else 1], v[2], v[3], v[4], v[5]

    def means(self):
        """The five means of utils/trainer.py:467-471 as python floats (desc_loss, det_loss, accuracy, d_pos, d_neg): each over the
        pairs where the figure is != 0 (accuracy: > 0); NaN for an empty list, as np.mean([]) gives.  One read-back."""
        return split_means(self.sums.cpu().numpy(), self.counts.cpu().numpy(), self.loss)

    def line(self, dataset, epoch):
        """The line utils/trainer.py:479 prints after a validation."""
        return format_line(dataset, epoch, self.means())


def split_means(sums, counts, loss="circle_loss"):
    """sums f64[6], counts i64[6] in the order of FIGURES -> the trainer's five means."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = sums / counts
    keep = [0 if loss == "circle_loss" else 1, 2, 3, 4, 5]
    return tuple(float(m[k]) for k in keep)


def format_line(dataset, epoch, means):
    return '{:s} Epoch {:3d}: desc_loss = {:.3f} det_loss = {:.3f} accuracy = {:.2f}%  d_pos = {:.3f} d_neg = {:.3f}'.format(
        dataset, epoch, means[0], means[1], means[2] * 100, means[3], means[4])


def _column_view(t, name, cols=None):
    """2-D float32 device tensor whose rows are `ld` floats apart and whose columns are adjacent -> (tensor, ld).  A column view of a
    record block is taken as it is; anything else is made contiguous."""
    t = ops._req(t, torch.float32, name)
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError("%s must be [N, %s] (got %s)" % (name, cols if cols is not None else "C", tuple(t.shape)))
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _check_shapes(features, scores, points, anc_idx, pos_idx, n):
    for name, t in (("features", features), ("scores", scores), ("points", points), ("anc_idx", anc_idx), ("pos_idx", pos_idx)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor on a GPU (got %s)" % (name, type(t)))
    if features.dim() != 2 or features.shape[1] not in (16, 32, 64):
        raise ValueError("validation_pairs: features of shape %s; [N, 16], [N, 32] or [N, 64] are implemented" % (tuple(features.shape),))
    N = features.shape[0]
    if scores.dim() not in (1, 2) or scores.shape[0] != N or (scores.dim() == 2 and scores.shape[1] != 1):
        raise ValueError("validation_pairs: %d feature rows, scores of shape %s" % (N, tuple(scores.shape)))
    if points.dim() != 2 or tuple(points.shape) != (N, 3):
        raise ValueError("validation_pairs: %d feature rows, points of shape %s" % (N, tuple(points.shape)))
    if anc_idx.dim() not in (1, 2) or anc_idx.shape != pos_idx.shape:
        raise ValueError("validation_pairs: index lists of shapes %s and %s" % (tuple(anc_idx.shape), tuple(pos_idx.shape)))
    ld = int(anc_idx.shape[-1])
    if n is not None and not isinstance(n, torch.Tensor):
        for x in np.asarray(n).reshape(-1):
            if not 0 <= int(x) <= min(ld, _lib.VALIDATION_NMAX):
                raise ValueError("validation_pairs: a pair of %d index pairs; the lists hold %d and one pair takes at most %d"
                                 % (int(x), ld, _lib.VALIDATION_NMAX))
    elif n is None and ld > _lib.VALIDATION_NMAX:
        raise ValueError("validation_pairs: lists of %d index pairs; one pair takes at most %d" % (ld, _lib.VALIDATION_NMAX))


def validation_pairs(features, scores, points, anc_idx, pos_idx, n=None, row0=None, safe_radius=VALIDATION_3DMATCH["safe_radius"],
                     keypts_num=VALIDATION_3DMATCH["keypts_num"], det_loss_weight=VALIDATION_3DMATCH["det_loss_weight"],
                     pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN, log_scale=LOG_SCALE, loss="circle_loss", out=None):
    """The validation figures of P pairs in one call, all inputs on the device:
      features f32[N, C] (C = 16 / 32 / 64), scores f32[N] or [N, 1], points f32[N, 3]: the stacks [anchor; positive] of all pairs one
        after the other; separate arrays or column views of one record block (no copy is made of a view with adjacent columns);
      anc_idx / pos_idx i32[P, ld] (or [ld] for one pair): the index pairs of every pair into ITS rows, the positive's already shifted
        by the anchor's length (datasets/ThreeDMatch.py:222-229); n i32[P] how many of them count (an int, or None = ld, for all);
      row0 i32[P + 1]: pair p holds rows row0[p] .. row0[p + 1] (None: one pair, all rows).
    safe_radius / keypts_num / det_loss_weight: the config entries (VALIDATION_3DMATCH, VALIDATION_KITTI); the margins and the log
    scale default to the reference's.  Three launches whatever P is, no read-back: capturable (pass the previous result as `out`).
    -> PairValidation."""
    _check_shapes(features, scores, points, anc_idx, pos_idx, n)           # (before the device is asked for: plain argument errors)
    lib = _lib.load()
    features, ldd = _column_view(features, "features")
    dev = features.device
    N, C = int(features.shape[0]), int(features.shape[1])
    if C not in (16, 32, 64):
        raise ValueError("validation_pairs: %d descriptor columns; 16, 32 or 64 are implemented" % C)
    scores, lds = _column_view(scores, "scores", 1)
    points, ldp = _column_view(points, "points", 3)
    if scores.shape[0] != N or points.shape[0] != N:
        raise ValueError("validation_pairs: %d feature rows, %d scores, %d points" % (N, scores.shape[0], points.shape[0]))
    anc_idx = ops._req(anc_idx, torch.int32, "anc_idx")
    pos_idx = ops._req(pos_idx, torch.int32, "pos_idx")
    if anc_idx.dim() == 1:
        anc_idx = anc_idx[None]
    if pos_idx.dim() == 1:
        pos_idx = pos_idx[None]
    if anc_idx.dim() != 2 or anc_idx.shape != pos_idx.shape:
        raise ValueError("validation_pairs: index lists of shapes %s and %s" % (tuple(anc_idx.shape), tuple(pos_idx.shape)))
    anc_idx, pos_idx = anc_idx.contiguous(), pos_idx.contiguous()
    P, ld = int(anc_idx.shape[0]), int(anc_idx.shape[1])
    if isinstance(n, torch.Tensor):
        n = ops._req(n, torch.int32, "n").reshape(-1).contiguous()
        host_n = getattr(n, "host_lens", None)
    else:
        host_n = [ld if n is None else int(n)] * P if np.ndim(n) == 0 else [int(x) for x in n]
        n = torch.as_tensor(np.asarray(host_n, np.int32), device=dev)
    if n.numel() != P:
        raise ValueError("validation_pairs: %d pairs, %d counts" % (P, n.numel()))
    if host_n is not None and P and (max(host_n) > min(ld, _lib.VALIDATION_NMAX) or min(host_n) < 0):
        raise ValueError("validation_pairs: a pair of %d index pairs; the lists hold %d and one pair takes at most %d"
                         % (max(host_n) if max(host_n) > 0 else min(host_n), ld, _lib.VALIDATION_NMAX))
    if row0 is None:
        if P != 1:
            raise ValueError("validation_pairs: %d pairs need row0" % P)
        row0 = torch.as_tensor(np.asarray([0, N], np.int32), device=dev)
    else:
        row0 = row0 if isinstance(row0, torch.Tensor) else torch.as_tensor(np.asarray(row0, np.int32))
        row0 = row0.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if row0.numel() != P + 1:
            raise ValueError("validation_pairs: row0 holds %d offsets for %d pairs (P + 1 are needed)" % (row0.numel(), P))
    if ld < 1:                                                   # no index pairs at all: n = 0 for every pair, the skip tuple
        anc_idx = pos_idx = torch.zeros((P, 1), dtype=torch.int32, device=dev)
    out = _reuse("validation_pairs", out, PairValidation, (P,), dev, lambda: PairValidation(P, dev, loss))
    out.loss = loss
    ldi = max(ld, 1)
    ws = ops.workspace(lib.d3f_validation_pairs_workspace_bytes(P, ldi), dev)
    rc = lib.d3f_validation_pairs(features.data_ptr(), ldd, C, scores.data_ptr(), lds, points.data_ptr(), ldp, N, row0.data_ptr(),
                                  anc_idx.data_ptr(), pos_idx.data_ptr(), ldi, n.data_ptr(), P, float(safe_radius), int(keypts_num),
                                  float(det_loss_weight), float(pos_margin), float(neg_margin), float(log_scale),
                                  out.values.data_ptr(), out.status.data_ptr(), out.sums.data_ptr(), out.counts.data_ptr(),
                                  ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "validation_pairs")
    out._inputs = (features, scores, points, anc_idx, pos_idx, n, row0, ws)          # (a captured call keeps reading these)
    return out


def validation_records(records, lens, anc_idx, pos_idx, n=None, descriptor_dim=None, **kw):
    """validation_pairs on the packed records FragmentEngine.fetch(packed=True) returns: records f32[N, 3 + C + 1] of [xyz | desc |
    score] rows, the stacks of the P pairs one after the other (one fetch, or several concatenated); lens: the lengths of their 2 P
    clouds (anchor, positive, anchor, ...) -- a list or a device tensor.  The three inputs are column views of `records`."""
    records = ops._req(records, torch.float32, "records", 2)
    if not records.is_contiguous():
        raise ValueError("validation_records: the record block must be contiguous")
    C = int(descriptor_dim) if descriptor_dim is not None else int(records.shape[1]) - 4
    if records.shape[1] < C + 4:
        raise ValueError("validation_records: %d columns hold no [xyz | %d-d desc | score] record" % (records.shape[1], C))
    dev = records.device
    lens = ops.as_lens(lens, dev)
    if lens.numel() % 2:
        raise ValueError("validation_records: %d clouds do not make pairs" % lens.numel())
    host = getattr(lens, "host_lens", None)
    if host is not None:
        row0 = torch.as_tensor(np.concatenate([[0], np.cumsum(np.asarray(host, np.int64).reshape(-1, 2).sum(1))]).astype(np.int32), device=dev)
    else:
        row0 = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), lens.view(-1, 2).sum(1).cumsum(0).to(torch.int32)])
    return validation_pairs(records[:, 3:3 + C], records[:, 3 + C:4 + C], records[:, :3], anc_idx, pos_idx, n, row0, **kw)
