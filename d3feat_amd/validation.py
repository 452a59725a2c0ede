"""Validation figures of a split on the MI355X: what the reference's model class evaluates per validation pair (models/
KPFCNN_model.py:131-186 with utils/loss.py -- desc_loss, det_loss, accuracy, ave_d_pos, ave_d_neg) and what utils/trainer.py:417-498
makes of them -- and the first stage of a backward pass: the gradient of desc_loss + det_loss with respect to the rows of
out_features and out_scores.  No regularisation loss; the backward of the head, of the network and the optimiser are not here.

    validation_pairs(features, scores, points, anc_idx, pos_idx, n, row0)   P pairs in one call (three launches, capturable)
    validation_records(records, lens, anc_idx, pos_idx, n)                 the same on packed [xyz | desc | score] records
    PairValidation                                                         the device tensors of a call; .means() / .line()
    loss_gradients(features, scores, points, anc_idx, pos_idx, n, row0)     loss and gradients of P pairs (five launches, capturable)
    loss_gradients_records(records, lens, anc_idx, pos_idx, n)             the same on packed records, in and out
    PairGradients                                                          .features, .scores, .values, .status; .figures(p)
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


def _check_shapes(features, scores, points, anc_idx, pos_idx, n, fn="validation_pairs"):
    for name, t in (("features", features), ("scores", scores), ("points", points), ("anc_idx", anc_idx), ("pos_idx", pos_idx)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor on a GPU (got %s)" % (name, type(t)))
    if features.dim() != 2 or features.shape[1] not in (16, 32, 64):
        raise ValueError("%s: features of shape %s; [N, 16], [N, 32] or [N, 64] are implemented" % (fn, tuple(features.shape)))
    N = features.shape[0]
    if scores.dim() not in (1, 2) or scores.shape[0] != N or (scores.dim() == 2 and scores.shape[1] != 1):
        raise ValueError("%s: %d feature rows, scores of shape %s" % (fn, N, tuple(scores.shape)))
    if points.dim() != 2 or tuple(points.shape) != (N, 3):
        raise ValueError("%s: %d feature rows, points of shape %s" % (fn, N, tuple(points.shape)))
    if anc_idx.dim() not in (1, 2) or anc_idx.shape != pos_idx.shape:
        raise ValueError("%s: index lists of shapes %s and %s" % (fn, tuple(anc_idx.shape), tuple(pos_idx.shape)))
    ld = int(anc_idx.shape[-1])
    if n is not None and not isinstance(n, torch.Tensor):
        for x in np.asarray(n).reshape(-1):
            if not 0 <= int(x) <= min(ld, _lib.VALIDATION_NMAX):
                raise ValueError("%s: a pair of %d index pairs; the lists hold %d and one pair takes at most %d"
                                 % (fn, int(x), ld, _lib.VALIDATION_NMAX))
    elif n is None and ld > _lib.VALIDATION_NMAX:
        raise ValueError("%s: lists of %d index pairs; one pair takes at most %d" % (fn, ld, _lib.VALIDATION_NMAX))


def _pair_arguments(fn, features, scores, points, anc_idx, pos_idx, n, row0):
    """The argument checks and conversions of validation_pairs and loss_gradients -> (lib, dev, N, C, P, ldi, features, ldd, scores,
    lds, points, ldp, anc_idx, pos_idx, n, row0), the tensors as the entry points take them."""
    _check_shapes(features, scores, points, anc_idx, pos_idx, n, fn)       # (before the device is asked for: plain argument errors)
    lib = _lib.load()
    features, ldd = _column_view(features, "features")
    dev = features.device
    N, C = int(features.shape[0]), int(features.shape[1])
    if C not in (16, 32, 64):
        raise ValueError("%s: %d descriptor columns; 16, 32 or 64 are implemented" % (fn, C))
    scores, lds = _column_view(scores, "scores", 1)
    points, ldp = _column_view(points, "points", 3)
    if scores.shape[0] != N or points.shape[0] != N:
        raise ValueError("%s: %d feature rows, %d scores, %d points" % (fn, N, scores.shape[0], points.shape[0]))
    anc_idx = ops._req(anc_idx, torch.int32, "anc_idx")
    pos_idx = ops._req(pos_idx, torch.int32, "pos_idx")
    if anc_idx.dim() == 1:
        anc_idx = anc_idx[None]
    if pos_idx.dim() == 1:
        pos_idx = pos_idx[None]
    if anc_idx.dim() != 2 or anc_idx.shape != pos_idx.shape:
        raise ValueError("%s: index lists of shapes %s and %s" % (fn, tuple(anc_idx.shape), tuple(pos_idx.shape)))
    anc_idx, pos_idx = anc_idx.contiguous(), pos_idx.contiguous()
    P, ld = int(anc_idx.shape[0]), int(anc_idx.shape[1])
    if isinstance(n, torch.Tensor):
        n = ops._req(n, torch.int32, "n").reshape(-1).contiguous()
        host_n = getattr(n, "host_lens", None)
    else:
        host_n = [ld if n is None else int(n)] * P if np.ndim(n) == 0 else [int(x) for x in n]
        n = torch.as_tensor(np.asarray(host_n, np.int32), device=dev)
    if n.numel() != P:
        raise ValueError("%s: %d pairs, %d counts" % (fn, P, n.numel()))
    if host_n is not None and P and (max(host_n) > min(ld, _lib.VALIDATION_NMAX) or min(host_n) < 0):
        raise ValueError("%s: a pair of %d index pairs; the lists hold %d and one pair takes at most %d"
                         % (fn, max(host_n) if max(host_n) > 0 else min(host_n), ld, _lib.VALIDATION_NMAX))
    if row0 is None:
        if P != 1:
            raise ValueError("%s: %d pairs need row0" % (fn, P))
        row0 = torch.as_tensor(np.asarray([0, N], np.int32), device=dev)
    else:
        row0 = row0 if isinstance(row0, torch.Tensor) else torch.as_tensor(np.asarray(row0, np.int32))
        row0 = row0.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if row0.numel() != P + 1:
            raise ValueError("%s: row0 holds %d offsets for %d pairs (P + 1 are needed)" % (fn, row0.numel(), P))
    if ld < 1:                                                   # no index pairs at all: n = 0 for every pair, the skip tuple
        anc_idx = pos_idx = torch.zeros((P, 1), dtype=torch.int32, device=dev)
    return lib, dev, N, C, P, max(ld, 1), features, ldd, scores, lds, points, ldp, anc_idx, pos_idx, n, row0


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
    (lib, dev, N, C, P, ldi, features, ldd, scores, lds, points, ldp, anc_idx, pos_idx, n,
     row0) = _pair_arguments("validation_pairs", features, scores, points, anc_idx, pos_idx, n, row0)
    out = _reuse("validation_pairs", out, PairValidation, (P,), dev, lambda: PairValidation(P, dev, loss))
    out.loss = loss
    ws = ops.workspace(lib.d3f_validation_pairs_workspace_bytes(P, ldi), dev)
    rc = lib.d3f_validation_pairs(features.data_ptr(), ldd, C, scores.data_ptr(), lds, points.data_ptr(), ldp, N, row0.data_ptr(),
                                  anc_idx.data_ptr(), pos_idx.data_ptr(), ldi, n.data_ptr(), P, float(safe_radius), int(keypts_num),
                                  float(det_loss_weight), float(pos_margin), float(neg_margin), float(log_scale),
                                  out.values.data_ptr(), out.status.data_ptr(), out.sums.data_ptr(), out.counts.data_ptr(),
                                  ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "validation_pairs")
    out._inputs = (features, scores, points, anc_idx, pos_idx, n, row0, ws)          # (a captured call keeps reading these)
    return out


def _record_columns(fn, records, lens, descriptor_dim):
    """records f32[N, 3 + C + 1], the lengths of the 2 P clouds -> (C, row0 i32[P + 1] on the device)."""
    if not records.is_contiguous():
        raise ValueError("%s: the record block must be contiguous" % fn)
    C = int(descriptor_dim) if descriptor_dim is not None else int(records.shape[1]) - 4
    if records.shape[1] < C + 4:
        raise ValueError("%s: %d columns hold no [xyz | %d-d desc | score] record" % (fn, records.shape[1], C))
    dev = records.device
    lens = ops.as_lens(lens, dev)
    if lens.numel() % 2:
        raise ValueError("%s: %d clouds do not make pairs" % (fn, lens.numel()))
    host = getattr(lens, "host_lens", None)
    if host is not None:
        row0 = torch.as_tensor(np.concatenate([[0], np.cumsum(np.asarray(host, np.int64).reshape(-1, 2).sum(1))]).astype(np.int32), device=dev)
    else:
        row0 = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), lens.view(-1, 2).sum(1).cumsum(0).to(torch.int32)])
    return C, row0


def validation_records(records, lens, anc_idx, pos_idx, n=None, descriptor_dim=None, **kw):
    """validation_pairs on the packed records FragmentEngine.fetch(packed=True) returns: records f32[N, 3 + C + 1] of [xyz | desc |
    score] rows, the stacks of the P pairs one after the other (one fetch, or several concatenated); lens: the lengths of their 2 P
    clouds (anchor, positive, anchor, ...) -- a list or a device tensor.  The three inputs are column views of `records`."""
    records = ops._req(records, torch.float32, "records", 2)
    C, row0 = _record_columns("validation_records", records, lens, descriptor_dim)
    return validation_pairs(records[:, 3:3 + C], records[:, 3 + C:4 + C], records[:, :3], anc_idx, pos_idx, n, row0, **kw)


class PairGradients(_PairResult):
    """Result of loss_gradients: DEVICE tensors.  features f32[N, C] and scores f32[N]: the gradient of desc_loss + det_loss of every
    pair with respect to the rows of the call's features and scores (zeros for the rows no list names, for a pair under the skip rule
    and for a pair whose status is not 0); values f32[P, 8] and status i32[P]: what validation_pairs returns for the same input, bit
    for bit.  loss: which descriptor loss was differentiated ('circle_loss' or 'desc_loss') and is THE desc_loss of figures().
    features / scores may be views the caller handed in (column views of a record-shaped block)."""
    FIELDS = ("features", "scores", "values", "status")

    def __init__(self, P, N, C, device, loss="circle_loss", features=None, scores=None):
        if loss not in ("circle_loss", "desc_loss"):
            raise ValueError("PairGradients: loss %r is neither 'circle_loss' nor 'desc_loss'" % (loss,))
        self.P, self.loss = P, loss
        self.key = (P, N, C)
        self.features = torch.empty((N, C), dtype=torch.float32, device=device) if features is None else features
        self.scores = torch.empty((N,), dtype=torch.float32, device=device) if scores is None else scores
        if tuple(self.features.shape) != (N, C) or self.features.dtype != torch.float32 or (C > 1 and N > 0 and self.features.stride(1) != 1):
            raise ValueError("PairGradients: features must be f32[%d, %d] with adjacent columns" % (N, C))
        if self.scores.dim() == 2 and self.scores.shape[1] == 1:
            self.scores = self.scores[:, 0]
        if tuple(self.scores.shape) != (N,) or self.scores.dtype != torch.float32 or self.scores.device != self.features.device:
            raise ValueError("PairGradients: scores must be f32[%d] on the device of features" % N)
        self.values = torch.empty((P, 8), dtype=torch.float32, device=device)
        self.status = torch.empty((P,), dtype=torch.int32, device=device)

    def figures(self, p=0):
        """(desc_loss, det_loss, accuracy, ave_d_pos, ave_d_neg) of pair p as device scalars, as PairValidation.figures."""
        v = self.values[p]
        return v[0 if self.loss == "circle_loss" else 1], v[2], v[3], v[4], v[5]


def _ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]) if t.dim() == 2 else 1, 1)


def loss_gradients(features, scores, points, anc_idx, pos_idx, n=None, row0=None, safe_radius=VALIDATION_3DMATCH["safe_radius"],
                   keypts_num=VALIDATION_3DMATCH["keypts_num"], det_loss_weight=VALIDATION_3DMATCH["det_loss_weight"],
                   pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN, log_scale=LOG_SCALE, loss="circle_loss", out=None):
    """The gradient of desc_loss + det_loss (models/KPFCNN_model.py:143-191; the regularisation term is not part of it) of P pairs with
    respect to the rows of `features` and `scores`, and the forward's figures, in one call: the arguments of validation_pairs, the
    same checks.  loss: 'circle_loss' (what the model class trains with) or 'desc_loss' (the contrastive loss).  The definition, the
    tie rule (equal split among bit-equal minima) and the summation order are in include/d3feat_amd.h (d3f_loss_gradients).  Five
    launches whatever P is, no read-back, every word of both gradients written: capturable (pass the previous result as `out`; a
    PairGradients made by hand may hold column views of a record-shaped block).  -> PairGradients."""
    if loss not in ("circle_loss", "desc_loss"):
        raise ValueError("loss_gradients: loss %r is neither 'circle_loss' nor 'desc_loss'" % (loss,))
    (lib, dev, N, C, P, ldi, features, ldd, scores, lds, points, ldp, anc_idx, pos_idx, n,
     row0) = _pair_arguments("loss_gradients", features, scores, points, anc_idx, pos_idx, n, row0)
    out = _reuse("loss_gradients", out, PairGradients, (P, N, C), dev, lambda: PairGradients(P, N, C, dev, loss))
    out.loss = loss
    ws = ops.workspace(lib.d3f_loss_gradients_workspace_bytes(P, ldi, C), dev)
    rc = lib.d3f_loss_gradients(features.data_ptr(), ldd, C, scores.data_ptr(), lds, points.data_ptr(), ldp, N, row0.data_ptr(),
                                anc_idx.data_ptr(), pos_idx.data_ptr(), ldi, n.data_ptr(), P, float(safe_radius), int(keypts_num),
                                float(det_loss_weight), float(pos_margin), float(neg_margin), float(log_scale),
                                1 if loss == "desc_loss" else 0, out.features.data_ptr(), max(_ld(out.features), C),
                                out.scores.data_ptr(), _ld(out.scores), out.values.data_ptr(), out.status.data_ptr(),
                                ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "loss_gradients")
    out._inputs = (features, scores, points, anc_idx, pos_idx, n, row0, ws)          # (a captured call keeps reading these)
    return out


def loss_gradients_records(records, lens, anc_idx, pos_idx, n=None, descriptor_dim=None, out_records=None, **kw):
    """loss_gradients on packed [xyz | desc | score] records, as validation_records.  out_records f32[N, 3 + C + 1] (contiguous): the
    gradients are written into its descriptor and score columns (the xyz columns are left as they are); None: separate tensors."""
    records = ops._req(records, torch.float32, "records", 2)
    C, row0 = _record_columns("loss_gradients_records", records, lens, descriptor_dim)
    if out_records is not None and kw.get("out") is None:
        out_records = ops._req(out_records, torch.float32, "out_records", 2)
        if out_records.shape != records.shape or not out_records.is_contiguous():
            raise ValueError("loss_gradients_records: out_records must be a contiguous block of the records' shape")
        P = int(row0.numel()) - 1
        kw["out"] = PairGradients(P, int(records.shape[0]), C, records.device, kw.get("loss", "circle_loss"),
                                  features=out_records[:, 3:3 + C], scores=out_records[:, 3 + C])
    return loss_gradients(records[:, 3:3 + C], records[:, 3 + C:4 + C], records[:, :3], anc_idx, pos_idx, n, row0, **kw)
