"""numpy restatement of d3f_overlap_pairs (include/d3feat_amd.h) for the tests: chunked brute force, no grid.

The metric, every operation rounded to fp32 and none contracted (numpy's float32 ufuncs round each result):
    r2 = thr * thr;  d2 = (dx*dx + dy*dy) + dz*dz with dx = q - s;  match iff d2 < r2;  nearest = minimum by (d2, index).
Also the two float64 margins under which an fp32 search and a float64 one cannot disagree (tools/make_golden_overlap.py)."""
import numpy as np

CHUNK = 512
BAND = 2.0 ** -18


def nearest_rows(src, tgt, thr):
    """-> i32[len(src)]: index in tgt of the nearest point strictly inside thr (lowest index among equal d2), -1: none."""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    out = np.full((len(src),), -1, np.int32)
    if not len(src) or not len(tgt):
        return out
    r2 = np.float32(thr) * np.float32(thr)
    for i0 in range(0, len(src), CHUNK):
        q = src[i0:i0 + CHUNK]
        dx, dy, dz = (q[:, None, d] - tgt[None, :, d] for d in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        j = np.argmin(d2, axis=1)                                 # the first minimum: the lowest index
        hit = d2[np.arange(len(q)), j] < r2
        out[i0:i0 + CHUNK] = np.where(hit, j, -1)
    return out


def overlap(clouds, pairs, thr, ld=None):
    """-> (count i32[P], nearest i32[P, ld]) as the entry point defines them; ld defaults to the longest cloud."""
    n = len(clouds)
    ld = max([len(c) for c in clouds] + [1]) if ld is None else ld
    count, near = np.zeros((len(pairs),), np.int32), np.full((len(pairs), ld), -1, np.int32)
    for p, (a, b) in enumerate(pairs):
        if not (0 <= a < n and 0 <= b < n):
            count[p] = -1
            continue
        row = nearest_rows(clouds[a], clouds[b], thr)
        count[p] = int((row >= 0).sum())
        near[p, :min(len(row), ld)] = row[:ld]
    return count, near


def margins(src, tgt, thr):
    """float64 distances of the float32 points -> (threshold margin, runner-up margin): the minimum over the queries of
    |d2 / r2 - 1| for the nearest point, and of (d2_second - d2_first) / d2_second over the queries whose nearest d2 < 1.5 r2."""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    r2 = float(thr) * float(thr)
    m_thr, m_run = np.inf, np.inf
    if not len(src) or not len(tgt):
        return m_thr, m_run
    for i0 in range(0, len(src), CHUNK):
        q = src[i0:i0 + CHUNK]
        dx, dy, dz = (q[:, None, d] - tgt[None, :, d] for d in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        rows = np.arange(len(q))
        j = np.argmin(d2, axis=1)
        first = d2[rows, j].copy()
        if d2.shape[1] > 1:
            d2[rows, j] = np.inf
            second = d2.min(axis=1)
            near = first < 1.5 * r2
            if near.any():
                m_run = min(m_run, float(((second[near] - first[near]) / second[near]).min()))
        m_thr = min(m_thr, float(np.abs(first / r2 - 1.0).min()))
    return m_thr, m_run


def split(points, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [points[offs[i]:offs[i + 1]] for i in range(len(lens))]
