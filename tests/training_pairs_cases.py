"""The fixtures of the training-pair tests (host and GPU): clouds on which fp32 and float64 must agree about every match.

Points lie on a lattice of spacing 1/4 with a jitter of -2 .. 2 sixty-fourths per coordinate, transforms are quarter turns about z with
translations in sixty-fourths, the radius is 20/64: every coordinate, difference, square and sum is a small multiple of 2^-12, exact in
fp32, so d2 < r2 has one answer in any precision, and equal distances inside a row (and d2 == r2 exactly, which is NOT a match) are
frequent.  tests/golden/training_pairs.npz adds one pair under a general rotation whose seed tools/make_golden_training_pairs.py searched
so that no decision is closer than 1e-4 relative.
"""
import numpy as np

H = 0.25
RADIUS = 20.0 / 64.0
f32 = np.float32


def quarter_turn(turns, t64):
    """4 x 4 float32: `turns` quarter turns about z, translation t64 / 64."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][turns % 4]
    T = np.eye(4, dtype=f32)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = np.asarray(t64, f32) / f32(64)
    return T


def inverse(T):
    """The exact inverse of a quarter_turn."""
    Ti = np.eye(4, dtype=f32)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def lattice(rng, n, dims=(12, 10, 3)):
    """n distinct lattice nodes of a dims box with jitter, float32 [n, 3], in random order."""
    total = dims[0] * dims[1] * dims[2]
    pick = rng.choice(total, size=n, replace=False)
    ijk = np.stack(np.unravel_index(pick, dims), 1).astype(np.float64)
    jit = rng.integers(-2, 3, size=(n, 3)) / 64.0
    return (ijk * H + jit).astype(f32)


def pair(rng, n_anchor, n_positive, turns=1, t64=(64, -32, 16), dims=(12, 10, 3)):
    """(anchor in its own frame, positive, T): the anchor is a lattice cloud of the positive's frame taken back through T."""
    T = quarter_turn(turns, t64)
    Ti = inverse(T)
    a = lattice(rng, n_anchor, dims)
    anchor = (a @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)                  # exact: entries 0 / +-1, translations in 64ths
    return anchor, lattice(rng, n_positive, dims), T


def stack(pairs):
    """[(anchor, positive, T)] -> points f32[N, 3], lens i32[2 P], trans f32[P, 4, 4]."""
    clouds = [c for a, b, _ in pairs for c in (a, b)]
    pts = np.concatenate([c.reshape(-1, 3) for c in clouds]).astype(f32)
    return np.ascontiguousarray(pts), np.asarray([len(c) for c in clouds], np.int32), np.stack([T for _, _, T in pairs]).astype(f32)


def three_pairs():
    """Clouds of 300 - 700 points and one anchor of 1100: past one workgroup and one scan tile."""
    rng = np.random.default_rng(11)
    return [pair(rng, 1100, 700, 1, (64, -32, 16), dims=(24, 20, 3)), pair(rng, 300, 420, 3, (0, 128, -64), dims=(14, 12, 3)),
            pair(rng, 650, 520, 2, (-192, 64, 0), dims=(16, 14, 3))]


def small_pair(seed=5, n_anchor=40, n_positive=36):
    rng = np.random.default_rng(seed)
    return pair(rng, n_anchor, n_positive, 1, (32, 0, -16), dims=(5, 4, 2))


def ends_pair():
    """The first and the last anchor row have no match (far outside the positive's grown box); so has a row in the middle."""
    rng = np.random.default_rng(17)
    a, b, T = pair(rng, 60, 50, 1, (0, 0, 0), dims=(5, 4, 3))
    far = inverse(T)
    for i, d in ((0, (40.0, 0, 0)), (len(a) - 1, (0, -37.5, 3.0)), (30, (0, 0, 25.0))):
        q = np.asarray(d, f32) + f32(0.5)
        a[i] = q @ far[:3, :3].T + far[:3, 3]
    return a, b, T


def cluster_pair():
    """75 positives inside the radius of ONE anchor point (past any register-resident cap), next to an ordinary lattice."""
    rng = np.random.default_rng(23)
    a, b, T = pair(rng, 30, 40, 0, (0, 0, 0), dims=(5, 4, 3))
    g = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3)
    centre = np.asarray([3.0, 3.0, 2.5], f32)                            # a node away from the lattice box
    cluster = (centre + g.astype(f32) / f32(64)).astype(f32)
    b = np.concatenate([b[:20], cluster[rng.permutation(len(cluster))], b[20:]]).astype(f32)
    a = np.concatenate([a[:10], centre[None], a[10:]]).astype(f32)
    return a, b, T


def apart_pair():
    """The whole anchor lies outside the positive's grown box: M = 0."""
    rng = np.random.default_rng(29)
    a, b, T = pair(rng, 35, 33, 0, (0, 0, 0), dims=(4, 4, 3))
    return (a + f32(100.0)).astype(f32), b, T


def many_pairs(P=127):
    rng = np.random.default_rng(31)
    return [pair(rng, int(rng.integers(18, 40)), int(rng.integers(18, 40)), int(rng.integers(0, 4)),
                 tuple(int(v) for v in rng.integers(-64, 65, 3)), dims=(4, 4, 3)) for _ in range(P)]


def keypts_lists(lengths, rows, seed=37):
    """The 3DMatch form's input: lists of the given lengths over pairs of `rows` = [(len anchor, len positive)] -> (i32[L, 2], i32[P + 1])."""
    rng = np.random.default_rng(seed)
    out, start = [], [0]
    for n, (la, lb) in zip(lengths, rows):
        out.append(np.stack([rng.integers(0, la, n), rng.integers(0, lb, n)], 1))
        start.append(start[-1] + n)
    return np.concatenate(out).astype(np.int32), np.asarray(start, np.int32)


def margins(anchor, positive, T, radius):
    """The smallest relative distance of a fp32 d2 to r2, and between two unequal d2 of one row's matches (1.0: none)."""
    import training_pairs_np as tp
    d2 = tp.d2_f32(tp.move(T, anchor), np.asarray(positive, f32)).astype(np.float64)
    r2 = float(f32(radius) * f32(radius))
    edge = np.abs(d2 - r2).min() / r2 if d2.size else 1.0
    row = 1.0
    for i in range(d2.shape[0]):
        v = np.sort(d2[i][d2[i] < r2])
        if len(v) > 1:
            gap = np.diff(v)
            rel = gap[gap > 0] / v[1:][gap > 0]
            if rel.size:
                row = min(row, rel.min())
    return float(edge), float(row)
