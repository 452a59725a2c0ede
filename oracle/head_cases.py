"""TEST INFRASTRUCTURE ONLY.  Seeded inputs for the detection-head tests (tests/test_gpu_pool_head.py on the GPU,
tests/test_oracle_network.py on the CPU): features and a level-0 neighbour matrix of a stack of clouds, built so that
the one discontinuity of the head -- "does this neighbour row count", sum_c y != 0 (models/D3Feat.py:94-96) -- is never
decided by rounding: a row's sum is exactly zero in every precision, or far from zero."""
import numpy as np

SHADOWS = (0, 3, -1, -9, 1 << 30)     # added to n (the first two) or taken as they are: == N, > N, negative, huge


def head_case(seed, C, K, lens, shadow=0.2, negative=(), scale=None, specials=True):
    """-> (x f32[n, C], nb i32[n, K]), n = sum(lens).
    Every cloud: N(0, 2) features (clouds listed in `negative`: every entry <= -0.05; scale: {cloud: factor}); ordinary rows are
    pushed away from a zero sum (|sum| >= 0.45 max|x| of the cloud).  specials (clouds of >= 6 rows that are not `negative`):
      row 0  all zeros;  row 1  [t, -t, 0, ...] (sum exactly 0, C >= 2);  row 2  [3e-6, -3e-6, 0, ...] (squared norm 1.8e-11: the
      descriptor clamp);  row 3's first neighbours ARE rows 0, 1, 2 (present, not counted);  row 4 has only shadow slots.
    Neighbours: uniform inside the point's OWN cloud (the per-cloud searches never cross clouds); a fraction `shadow` of the slots
    holds a shadow value: n, n + 3, -1, -9 or 2^30."""
    rng = np.random.default_rng(seed)
    lens = [int(l) for l in lens]
    n = sum(lens)
    x = rng.normal(0.0, 2.0, (n, C)).astype(np.float32)
    nb = np.zeros((n, K), np.int32)
    a = 0
    for b, l in enumerate(lens):
        if l == 0:
            continue
        xs = x[a:a + l]
        if b in negative:
            xs[:] = -np.abs(xs) - np.float32(0.05)
        if scale and b in scale:
            xs *= np.float32(scale[b])
        amax = np.abs(xs).max()
        s = xs.astype(np.float64).sum(1)
        bad = np.abs(s) < 0.05 * amax
        xs[bad, 0] += (np.where(s[bad] >= 0, 0.5, -0.5) * amax).astype(np.float32)
        sp = specials and l >= 6 and b not in negative
        if sp:
            xs[0:3] = 0
            if C >= 2:
                t = np.float32(0.75) * amax
                xs[1, 0], xs[1, 1] = t, -t
                xs[2, 0], xs[2, 1] = np.float32(3e-6), np.float32(-3e-6)
        ids = rng.integers(a, a + l, (l, K))
        sh = rng.random((l, K)) < shadow
        pick = rng.integers(0, len(SHADOWS), (l, K))
        vals = np.asarray([n + SHADOWS[0], n + SHADOWS[1], SHADOWS[2], SHADOWS[3], SHADOWS[4]], np.int64)[pick]
        ids = np.where(sh, vals, ids)
        if sp:
            ids[3, :min(K, 3)] = a + np.arange(min(K, 3))
            ids[4, :] = n
        nb[a:a + l] = ids.astype(np.int32)
        a += l
    return x, nb


def neighbours_stay_in_cloud(nb, lens):
    """The head kernels' stated contract: every real neighbour index of a point lies inside the point's own cloud."""
    n, a = int(sum(lens)), 0
    for l in lens:
        r = nb[a:a + int(l)].astype(np.int64)
        real = (r >= 0) & (r < n)
        if not np.all(~real | ((r >= a) & (r < a + int(l)))):
            return False
        a += int(l)
    return True


def in_batches(lens, include_zero):
    """A two-(or more-)cloud in_batches matrix (datasets/common.py:453-496) that realises a given include-zero vector: a cloud's
    row holds the shadow index n iff its flag is set; other padding repeats the cloud's own first row (changes no maximum)."""
    lens = [int(l) for l in lens]
    n, w = sum(lens), max(lens) + 1
    rows, a = [], 0
    for l, z in zip(lens, include_zero):
        assert l > 0
        rows.append(np.concatenate([np.arange(a, a + l), np.full(w - l, n if z else a)]).astype(np.int64))
        a += l
    return np.stack(rows, 0)
