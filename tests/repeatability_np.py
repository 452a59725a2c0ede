"""float64 numpy restatement of d3f_repeatability_pairs (include/d3feat_amd.h) with exactly its operation order, done the slow way of
repeatability/evaluate_3dmatch_our.py:30-41 / evaluate_kitti_our.py:12-23: per count -- slice the last k rows of both blocks, move
one of them, ALL distances, the column minimum.  The nested-prefix walk of the kernel is deliberately not used here: it is what the
comparison tests.  A helper module (no tests in it)."""
import numpy as np


def move(M, xyz):
    """q_r = ((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r], every operation rounded on its own.  M f64[3 or 4, 4], xyz f64[n,3]."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], 1)


def min_d2(src, tgt, gt, k, moved="target"):
    """Column minima d2[j] = min_i |s_i - t_j|^2 over the last k rows of both blocks (f32 [n, >= 3] in ascending score order), inf
    without a source row."""
    s = np.asarray(src)[:, :3][max(len(src) - k, 0):].astype(np.float64)
    t = np.asarray(tgt)[:, :3][max(len(tgt) - k, 0):].astype(np.float64)
    M = np.asarray(gt, np.float64)
    if moved == "target":
        t = move(M, t)
    elif moved == "source":
        s = move(M, s)
    else:
        raise ValueError(moved)
    if len(s) == 0:
        return np.full(len(t), np.inf)
    dx, dy, dz = (s[:, None, c] - t[None, :, c] for c in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    return d2.min(axis=0)


def repeat_counts(blocks, pairs, gts, num_keypts, threshold, moved="target"):
    """i64[P, n]: target keypoints with a source keypoint strictly inside the threshold, d2 < threshold * threshold.  A pair index
    outside the blocks selects no rows."""
    thr2 = np.float64(threshold) * np.float64(threshold)
    empty = np.zeros((0, 3), np.float32)
    out = np.zeros((len(pairs), len(num_keypts)), np.int64)
    for p, (a, b) in enumerate(pairs):
        src = blocks[a] if 0 <= a < len(blocks) else empty
        tgt = blocks[b] if 0 <= b < len(blocks) else empty
        for c, k in enumerate(num_keypts):
            out[p, c] = int(np.sum(min_d2(src, tgt, gts[p], int(k), moved) < thr2))
    return out


def band(blocks, pairs, gts, num_keypts, threshold, moved="target"):
    """Smallest | sqrt(column minimum) - threshold | over every (pair, count, target row)."""
    best = np.inf
    for p, (a, b) in enumerate(pairs):
        for k in num_keypts:
            d = np.sqrt(min_d2(blocks[a], blocks[b], gts[p], int(k), moved))
            d = d[np.isfinite(d)]
            if len(d):
                best = min(best, float(np.abs(d - threshold).min()))
    return best
