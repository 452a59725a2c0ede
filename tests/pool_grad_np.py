"""The backward of the two gathers at a level boundary, restated in float64 numpy (the definition of include/d3feat_amd.h:
d3f_ind_max_pool_backward, d3f_closest_pool_cat_backward), line-by-line torch restatements of the reference's forward for autograd
(models/network_blocks.py:51-66, :69-83 + models/D3Feat.py:63), and the tie cases both test files share.

Equality is equality of values, so the restatement is exact about ties whatever the dtype of its inputs: float32 inputs are widened, the
comparisons are unchanged by that, and only the sums are float64."""
import numpy as np
import torch


# ---- float64 numpy ------------------------------------------------------------------------------------------------------------
def max_pool_forward(x, inds):
    """ind_max_pool in the dtype of x: x' = concat(x, column minima), y = max_k x'[inds]; an index outside [0, N1) names the shadow row."""
    x = np.asarray(x)
    N1 = x.shape[0]
    xs = np.concatenate([x, x.min(0, keepdims=True)], 0)
    idx = np.where((inds >= 0) & (inds < N1), inds, N1)
    return xs[idx].max(1)


def max_pool_backward(x, inds, y, g, parts=False):
    """gx f64[N1, C] from the stored y and its gradient g (T, gs, S, M as the header names them)."""
    x, y, g = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(g, np.float64)
    (N1, C), (N2, K) = x.shape, inds.shape
    colmin = x.min(0) if N1 else np.zeros(C)
    xs = np.concatenate([x, colmin[None]], 0)
    idx = np.where((inds >= 0) & (inds < N1), inds, N1).astype(np.int64)
    tie = xs[idx] == y[:, None, :]                                   # [N2, K, C]
    T = tie.sum(1)
    gs = np.where(T > 0, g / np.maximum(T, 1), 0.0)
    acc = np.zeros((N1 + 1, C))
    np.add.at(acc, idx.reshape(-1), (tie * gs[:, None, :]).reshape(-1, C))     # (unbuffered: ascending e)
    S = acc[N1]
    holds = x == colmin
    M = holds.sum(0)
    gx = acc[:N1] + holds * (S / np.maximum(M, 1))
    if parts:
        return dict(gx=gx, T=T, gs=gs, S=S, M=M, colmin=colmin, shadow_ties=(tie & (idx == N1)[:, :, None]).sum(1))
    return gx


def upsample_cat_forward(x, inds, skip=None):
    x = np.asarray(x)
    N1 = x.shape[0]
    xs = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)
    first = inds[:, 0]
    up = xs[np.where((first >= 0) & (first < N1), first, N1)]
    return up if skip is None else np.concatenate([up, skip], 1)


def upsample_cat_backward(g, inds, N1, C1):
    """(gx f64[N1, C1], gskip = g[:, C1:])"""
    g = np.asarray(g, np.float64)
    first = inds[:, 0]
    idx = np.where((first >= 0) & (first < N1), first, N1).astype(np.int64)
    acc = np.zeros((N1 + 1, C1))
    np.add.at(acc, idx, g[:, :C1])
    return acc[:N1], g[:, C1:]


def transpose_np(inds, N1):
    """(start i32[N1 + 1], edges) of the rectangular table: the stable sort of the valid edges by the row they name."""
    flat = np.asarray(inds).reshape(-1)
    valid = np.nonzero((flat >= 0) & (flat < N1))[0]
    order = valid[np.argsort(flat[valid], kind="stable")]
    start = np.searchsorted(flat[order], np.arange(N1 + 1), side="left").astype(np.int32)
    return start, order.astype(np.int32)


def longest_segment(inds, N1):
    start, _ = transpose_np(inds, N1)
    return int(np.diff(start).max()) if N1 else 0


# ---- torch restatements for autograd ------------------------------------------------------------------------------------------
def torch_ind_max_pool(x, inds):
    """models/network_blocks.py:51-66, line by line.  amin / amax: their gradients split ties evenly (checked by the host test)."""
    N1 = x.shape[0]
    x = torch.cat([x, torch.amin(x, dim=0, keepdim=True)], dim=0)
    idx = torch.as_tensor(np.where((inds >= 0) & (inds < N1), inds, N1).astype(np.int64))
    pool_features = x[idx]
    return torch.amax(pool_features, dim=1)


def torch_closest_pool_cat(x, inds, skip=None):
    """models/network_blocks.py:69-83 and the concatenation of models/D3Feat.py:63."""
    N1 = x.shape[0]
    x = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=x.dtype)], dim=0)
    first = inds[:, 0]
    pool_features = x[torch.as_tensor(np.where((first >= 0) & (first < N1), first, N1).astype(np.int64))]
    return pool_features if skip is None else torch.cat([pool_features, skip], dim=1)


# ---- the shared cases ---------------------------------------------------------------------------------------------------------
def sliced_pool_case(seed, N1, N2, K, C, S=256, zero_column=None, dtype=np.float32):
    """pool_case for more than one slice of S rows on either side (the device folds per-slice partials): quantised values, and in EVERY
    slice of pooled rows, at its first rows p0, p0 + 1, p0 + 2 (a trailing slice shorter than 3 rows: as many as fit) --
      p0             no valid neighbour (all K slots shadow: y = colmin, T = K per column, so the slice's shadow share is not zero)
      p0 + 1         its only valid neighbour is fine row N1 - 2, the strict argmin of column 0 -- a row of the LAST slice of fine rows,
                     so the minimum of column 0 is held there only -- beside K - 1 shadow slots
      p0 + 2         names fine row 7 twice (K > 2)
    column 1's minimum is held by one fine row of each of the first three slices (M = 3, or fewer slices: fewer); fine row 3 is named
    in slot 0 by every sixth pooled row from row 5 on (at most 90 of them: the longest segment), fine rows 4 and S + 4 by none (both
    hold a zero of zero_column).
    zero_column: that column holds non-negative multiples of 1/8 whose zeros are +0 in the first slice of fine rows and -0 beyond."""
    rng = np.random.default_rng(seed)
    assert N1 >= 2 * S and N2 >= 8 and K >= 3
    x = rng.integers(-16, 17, (N1, C)) / 8.0
    inds = rng.integers(0, N1, (N2, K))
    inds[rng.random((N2, K)) < 0.2] = N1
    inds[rng.random((N2, K)) < 0.03] = N1 + 3
    inds[rng.random((N2, K)) < 0.03] = -1
    inds[(inds == 4) | (inds == 3) | (inds == S + 4)] = 8
    inds[5:5 + 6 * 90:6, 0] = 3
    for p0 in range(0, N2, S):
        inds[p0, :] = N1
        if p0 + 1 < N2:
            inds[p0 + 1, :] = N1
            inds[p0 + 1, 0] = N1 - 2
        if p0 + 2 < N2:
            inds[p0 + 2, 1:3] = 7
    x[N1 - 2, 0] = x[:, 0].min() - 0.5
    if C > 1:
        x[[r for r in (2, S + 6, 2 * S + 9) if r < N1 - 2], 1] = x[:, 1].min() - 0.25
    if zero_column is not None:
        col = rng.integers(0, 17, N1) / 8.0
        col[[1, 4, S - 1, S, S + 4, N1 - 1]] = 0.0
        col[S:][col[S:] == 0] = -0.0
        x[:, zero_column] = col
    g = rng.normal(size=(N2, C))
    return x.astype(dtype), inds.astype(np.int32), g.astype(dtype)


def pool_case(seed, N1, N2, K, C, quantised=True, ties=True, dtype=np.float32, slice_rows=None, zero_column=None):
    """x [N1, C], inds i32[N2, K] with shadow entries (N1 and beyond, and negative), g [N2, C].  quantised: multiples of 1/8 in [-2, 2]
    (many ties).  slice_rows / zero_column: sliced_pool_case above instead.  ties (N1 >= 12, N2 >= 8): the planted rows --
      pooled row 0   no valid neighbour (all K slots shadow: y = colmin, T = K per column)
      pooled row 1   its only valid neighbour is fine row 5, which is made the strict argmin of column 0, beside shadow slots when K > 1
                     (column 0 ties between the real slot and the K - 1 shadow slots)
      column 1       its minimum is held by the fine rows 2, 6 and 9 (M = 3)
      pooled row 2   names fine row 7 twice when K > 1
      fine row 3     named by every pooled row but rows 0 and 1 (slot 0); fine row 4 named by none."""
    if slice_rows is not None:
        return sliced_pool_case(seed, N1, N2, K, C, slice_rows, zero_column, dtype)
    rng = np.random.default_rng(seed)
    if quantised:
        x = rng.integers(-16, 17, (N1, C)) / 8.0
    else:
        x = rng.permutation(N1 * C).reshape(N1, C) / float(N1 * C) + rng.uniform(0, 0.1 / (N1 * C), (N1, C))
    inds = rng.integers(0, N1, (N2, K))
    inds[rng.random((N2, K)) < 0.2] = N1                                        # shadow entries
    inds[rng.random((N2, K)) < 0.03] = N1 + 3
    inds[rng.random((N2, K)) < 0.03] = -1
    if ties and N1 >= 12 and N2 >= 8:
        inds[inds == 4] = 8
        inds[2:, 0] = 3
        inds[0, :] = N1
        inds[1, :] = N1
        inds[1, 0] = 5
        x[5, 0] = x[:, 0].min() - 0.5
        if C > 1:
            x[[2, 6, 9], 1] = x[:, 1].min() - 0.25
        if K > 1:
            inds[2, 1] = 7
            if K > 2:
                inds[2, 2] = 7
    g = rng.normal(size=(N2, C))
    return x.astype(dtype), inds.astype(np.int32), g.astype(dtype)


def upsample_case(seed, N1, N2, K, C1, C2, dtype=np.float32):
    """inds i32[N2, K] whose first column names coarse rows, with shadow entries; coarse row 1 is named by every fine row from 10 on,
    coarse row 2 by none; g [N2, C1 + C2]."""
    rng = np.random.default_rng(seed)
    inds = rng.integers(0, N1, (N2, K))
    inds[inds == 2] = 0
    inds[10:, 0] = 1
    inds[rng.random(N2) < 0.1, 0] = N1
    inds[3, 0], inds[4, 0] = N1 + 2, -1
    inds[5:10, 0] = [0, 3, 3, 0, min(N1 - 1, 7)]
    g = rng.normal(size=(N2, C1 + C2))
    return inds.astype(np.int32), g.astype(dtype)
