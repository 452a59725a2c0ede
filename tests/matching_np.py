"""float64 numpy restatement of d3f_match_pairs (include/d3feat_amd.h), done the slow way of geometric_registration/evaluate.py:45-50,
67-82: per count -- slice the last k rows of both blocks, ALL squared descriptor distances, argmin in both directions, the mutual pairs,
the target points moved with gt, the distances against the threshold.  The nested-prefix walk of the kernel is deliberately not used
here: it is what the comparison tests.

numpy has no fused multiply-add, so this module does NOT claim the kernel's bits.  It is to be used only on inputs whose margins were
asserted first (margins()): every row's best and second-best float64 distance further apart than 8 x the largest difference between
the float64 distances and the fp32 forms, and every mutual pair's point distance further from the threshold than 8 x the largest
fp32 / float64 difference -- then the argmin, hence every count, is the same in either arithmetic.  A helper module (no tests in it)."""
import numpy as np


def tail(block, k):
    block = np.asarray(block)
    return block[max(len(block) - int(k), 0):]


def _blocks_of(blocks, pair):
    empty = np.zeros((0, np.asarray(blocks[0]).shape[1]), np.float32)
    return tuple(np.asarray(blocks[i]) if 0 <= i < len(blocks) else empty for i in pair)


def d2_f64(s_desc, t_desc):
    """f64[n, m]: sum_c (s_i[c] - t_j[c])^2 of the f32 descriptors widened to float64."""
    s, t = np.asarray(s_desc, np.float64), np.asarray(t_desc, np.float64)
    if len(s) == 0:
        return np.zeros((0, len(t)))
    return np.stack([((row[None, :] - t) ** 2).sum(1) for row in s])            # differences first: no cancellation of norms


def d2_f32_chain(s_desc, t_desc):
    """f32[n, m]: the chain of the kernels, d = s[c] - t[c] (fp32), d2 = fma(d, d, d2), c ascending -- the product exact in float64, the
    sum rounded to float64 and then to fp32 (a double rounding: equal to the fused result except in rare halfway cases)."""
    s, t = np.asarray(s_desc, np.float32), np.asarray(t_desc, np.float32)
    acc = np.zeros((len(s), len(t)), np.float32)
    for c in range(s.shape[1]):
        d = (s[:, None, c] - t[None, :, c]).astype(np.float64)
        acc = (d * d + acc.astype(np.float64)).astype(np.float32)
    return acc


def d2_reference(s_desc, t_desc):
    """f32[n, m]: the square of the reference's distance, 2 - 2 s.t in float32 (evaluate.py:17, unit descriptors)."""
    s, t = np.asarray(s_desc, np.float32), np.asarray(t_desc, np.float32)
    return np.float32(2) - np.float32(2) * (s @ t.T)


def _gap(D):
    """smallest (second best - best) over the rows and over the columns of a distance matrix; inf with fewer than two candidates"""
    g = np.inf
    for M in (D, D.T):
        if M.shape[0] and M.shape[1] >= 2:
            two = np.partition(M, 1, axis=1)[:, :2]
            g = min(g, float((two[:, 1] - two[:, 0]).min()))
    return g


def move(M, xyz):
    M = np.asarray(M, np.float64)
    return np.asarray(xyz, np.float64) @ M[:3, :3].T + M[:3, 3]


def move_f32(M, xyz):
    """R x + t in float32 (rounded at every step; the kernel fuses, the difference is what margins() measures against float64)"""
    M, p = np.asarray(M, np.float32), np.asarray(xyz, np.float32)
    return np.stack([M[r, 0] * p[:, 0] + (M[r, 1] * p[:, 1] + (M[r, 2] * p[:, 2] + M[r, 3])) for r in range(3)], 1)


def mutual_pairs(s_desc, t_desc):
    """i64[k, 2]: the pairs (i, argmin_j D[i, j]) with argmin_i D[i, j] == i, ascending i, lowest index on ties (float64)."""
    D = d2_f64(s_desc, t_desc)
    if D.shape[0] == 0 or D.shape[1] == 0:
        return np.zeros((0, 2), np.int64)
    st, ts = D.argmin(1), D.argmin(0)
    i = np.nonzero(ts[st] == np.arange(len(st)))[0]
    return np.stack([i, st[i]], 1).astype(np.int64)


def match_counts(blocks, pairs, gts, num_keypts, threshold, C=32):
    """(mutual_count, gt_inliers) i64[P, n]; blocks f32[k, 3 + C + ...] in ascending score order, gts [P, 3 or 4, 4] target -> source
    (None: no inliers).  A pair index outside the blocks selects no rows."""
    mc = np.zeros((len(pairs), len(num_keypts)), np.int64)
    gi = np.zeros_like(mc)
    for p, pair in enumerate(pairs):
        S, T = _blocks_of(blocks, pair)
        for c, k in enumerate(num_keypts):
            s, t = tail(S, k), tail(T, k)
            m = mutual_pairs(s[:, 3:3 + C], t[:, 3:3 + C])
            mc[p, c] = len(m)
            if gts is not None and len(m):
                d = np.sqrt(((s[m[:, 0], :3].astype(np.float64) - move(gts[p], t[m[:, 1], :3])) ** 2).sum(1))
                gi[p, c] = int(np.sum(d < threshold))
    return mc, gi


def margins(blocks, pairs, gts, num_keypts, threshold, C=32, reference_form=False):
    """dict(err, gap, point_err, band): err = largest |float64 d2 - fp32 chain d2| (and - the reference's 2 - 2 s.t form with
    reference_form=True) over every descriptor pair of the largest count; gap = smallest best / second-best difference of any row, at
    any count, in either direction; point_err = largest |float64 - fp32| point distance of a mutual pair, band = smallest |float64
    point distance - threshold| (inf without gts or mutual pairs)."""
    err = perr = 0.0
    gap = band = np.inf
    for p, pair in enumerate(pairs):
        S, T = _blocks_of(blocks, pair)
        kmax = max(num_keypts)
        s, t = tail(S, kmax)[:, 3:3 + C], tail(T, kmax)[:, 3:3 + C]
        if len(s) == 0 or len(t) == 0:
            continue
        D = d2_f64(s, t)
        err = max(err, float(np.abs(D - d2_f32_chain(s, t)).max()))
        if reference_form:
            err = max(err, float(np.abs(D - d2_reference(s, t)).max()))
        for k in num_keypts:
            Dk = D[max(len(s) - int(k), 0):, max(len(t) - int(k), 0):]         # the tails of the tails
            gap = min(gap, _gap(Dk))
            if gts is not None:
                sk, tk = tail(S, k), tail(T, k)
                st, ts = Dk.argmin(1), Dk.argmin(0)
                i = np.nonzero(ts[st] == np.arange(len(st)))[0]
                if len(i):
                    d64 = np.sqrt(((sk[i, :3].astype(np.float64) - move(gts[p], tk[st[i], :3])) ** 2).sum(1))
                    q = move_f32(gts[p], tk[st[i], :3])
                    d32 = np.sqrt(((sk[i, :3] - q) ** 2).sum(1, dtype=np.float32))
                    perr = max(perr, float(np.abs(d64 - d32).max()))
                    band = min(band, float(np.abs(d64 - threshold).min()))
    return dict(err=err, gap=gap, point_err=perr, band=band)


def margins_ok(m, factor=8.0):
    return m["gap"] >= factor * m["err"] and m["band"] >= factor * m["point_err"]
