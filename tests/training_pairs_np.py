"""d3f_training_pairs restated in plain numpy (include/d3feat_amd.h is the definition; this is the same text).

    draw / key / u24        the counter-based draws (64-bit integer arithmetic, vectorised over the counter)
    matches                 brute force in float64: every (i, j) with |T a_i - b_j|^2 < r^2, ordered by i and inside a row by (d2, j);
                            d2 is the fp32 metric of the header evaluated in float32 numpy (no FMA there), so the order is the device's
    floyd / with_replacement  the sampling procedures, integer for integer (floyd is the serial algorithm with a Python set)
    cloud_params / augment  the parameters of a cloud and the row pass in float32 numpy, operation by operation in the header's order
    training_pairs          one call: the dict of what the device returns

Open3D is not available to the tests: the order of get_matching_indices' list inside runs of equal distance, and its voxel grid, stay
unpinned (the header says so).  The reference's rotate() pins R and the points @ R convention (tests/golden/training_pairs.npz).
"""
import numpy as np

STREAM_NOISE, STREAM_ROTATION, STREAM_SCALE, STREAM_SHIFT, STREAM_SAMPLE = 0, 2, 4, 6, 8
FEW_MATCHES, BELOW_KEYPTS, LIST_RANGE = 1, 2, 4
AUGMENT_KITTI = dict(augment_noise=0.01, augment_rotation=1, augment_scale_min=0.8, augment_scale_max=1.2, augment_shift_range=2.0)
AUGMENT_3DMATCH = dict(augment_noise=0.005, augment_rotation=1, augment_scale_min=1.0, augment_scale_max=1.0, augment_shift_range=0.0)
f32 = np.float32
_U = np.uint64


def mix(x):
    """The finaliser of splitmix64 on uint64 (scalars or arrays), wrapping."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, _U) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def key(seed, step, pair, stream):
    a = mix(_U(seed & 0xFFFFFFFFFFFFFFFF) ^ mix(_U(step & 0xFFFFFFFFFFFFFFFF)))
    return mix(a ^ _U((int(pair) << 8) | int(stream)))


def draw(seed, step, pair, stream, counter):
    """uint64 (an array for an array of counters)."""
    return mix(key(seed, step, pair, stream) ^ np.asarray(counter, _U))


def u24(r):
    return (np.asarray(r, _U) >> _U(40)).astype(f32) * f32(2.0 ** -24)


def below(r, m):
    """(r >> 11) mod m as Python ints / int64 arrays."""
    return ((np.asarray(r, _U) >> _U(11)) % np.asarray(m, _U)).astype(np.int64)


# ---- the matches ------------------------------------------------------------------------------------------------------------------
def move(T, a):
    """((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in float32, every operation rounded on its own."""
    T, a = np.asarray(T, f32), np.asarray(a, f32).reshape(-1, 3)
    return np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] for r in range(3)], 1).astype(f32)


def d2_f32(q, b):
    """[len(q), len(b)] of the header's metric in float32."""
    d = q[:, None, :].astype(f32) - b[None, :, :].astype(f32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def matches(anchor, positive, T, radius):
    """-> i64[M, 2] (i, j) in the list's order, and start i64[len(anchor) + 1]."""
    q = move(T, anchor)
    b = np.asarray(positive, f32).reshape(-1, 3)
    if len(q) == 0 or len(b) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(len(q) + 1, np.int64)
    d2 = d2_f32(q, b)
    r2 = f32(radius) * f32(radius)
    rows, start = [], [0]
    for i in range(len(q)):
        j = np.nonzero(d2[i] < r2)[0]
        j = j[np.lexsort((j, d2[i, j]))]
        rows.append(np.stack([np.full(len(j), i, np.int64), j.astype(np.int64)], 1))
        start.append(start[-1] + len(j))
    return np.concatenate(rows), np.asarray(start, np.int64)


def matches_f64(anchor, positive, T, radius):
    """The set of matches by a float64 brute force on the float64 transform (what a reader would write): a set of (i, j)."""
    T = np.asarray(T, np.float64)
    q = np.asarray(anchor, np.float64).reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]
    b = np.asarray(positive, np.float64).reshape(-1, 3)
    d2 = ((q[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    i, j = np.nonzero(d2 < float(radius) ** 2)
    return set(zip(i.tolist(), j.tolist()))


# ---- the sample -------------------------------------------------------------------------------------------------------------------
def floyd(seed, step, pair, M, k):
    """k distinct match numbers of [0, M), in the order they are drawn (Floyd's algorithm, the header's text)."""
    r = draw(seed, step, pair, STREAM_SAMPLE, np.arange(k))
    S, out = set(), []
    for i in range(k):
        j = M - k + i
        t = int(below(r[i], j + 1))
        v = j if t in S else t
        S.add(v)
        out.append(v)
    return np.asarray(out, np.int64)


def with_replacement(seed, step, pair, length, k):
    return below(draw(seed, step, pair, STREAM_SAMPLE, np.arange(k)), length)


# ---- parameters and the row pass --------------------------------------------------------------------------------------------------
def rotation_draw(c, s, axis):
    """The reference's matrix (datasets/ThreeDMatch.py:24-45) from float32 c, s."""
    R = np.array([[c, -s, -s], [s, c, -s], [s, s, c]], dtype=f32)
    R[:, axis] = 0
    R[axis, :] = 0
    R[axis, axis] = 1
    return R


def mat3(a, b):
    """(a0 b0 + a1 b1) + a2 b2 per entry in float32."""
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)], dtype=f32)


def rotation_draws(seed, step, pair, side, mode):
    """[(theta float64, axis)] of the cloud's rotation draws."""
    out = []
    for d in range(mode):
        r = draw(seed, step, pair, STREAM_ROTATION + side, 2 * d)
        theta = (float(int(r) >> 11) * 2.0 ** -53 * 2.0) * np.pi
        axis = int(below(draw(seed, step, pair, STREAM_ROTATION + side, 2 * d + 1), 3)) if mode == 1 else d
        out.append((theta, axis))
    return out


def cloud_params(seed, step, pair, side, augment):
    """f32[16]: R (9), scale, shift (3), first angle, first axis, rotation mode."""
    mode = int(augment["augment_rotation"])
    R = np.eye(3, dtype=f32)
    theta0 = axis0 = f32(0)
    for d, (theta, axis) in enumerate(rotation_draws(seed, step, pair, side, mode)):
        Rd = rotation_draw(f32(np.cos(theta)), f32(np.sin(theta)), axis)
        if d == 0:
            R, theta0, axis0 = Rd, f32(theta), f32(axis)
        else:
            R = mat3(R, Rd)
    smin, smax, rng = f32(augment["augment_scale_min"]), f32(augment["augment_scale_max"]), f32(augment["augment_shift_range"])
    scale = smin + (smax - smin) * u24(draw(seed, step, pair, STREAM_SCALE, 0))
    shift = -rng + (f32(2) * rng) * u24(draw(seed, step, pair, STREAM_SHIFT + side, np.arange(3)))
    return np.concatenate([R.reshape(9), [scale], shift, [theta0, axis0, f32(mode)]]).astype(f32)


def augment_rows(seed, step, pair, side, noise, params, rows):
    """out = ((p + u noise) @ R) scale + shift in float32, the header's order, from the given f32[16] parameters."""
    rows = np.asarray(rows, f32).reshape(-1, 3)
    n = len(rows)
    u = u24(draw(seed, step, pair, STREAM_NOISE + side, np.arange(3 * n))).reshape(n, 3)
    a = (rows + u * f32(noise)).astype(f32)
    R, scale, shift = params[:9].reshape(3, 3), params[9], params[10:13]
    out = np.empty((n, 3), f32)
    for j in range(3):
        o = (a[:, 0] * R[0, j] + a[:, 1] * R[1, j]) + a[:, 2] * R[2, j]
        out[:, j] = o * scale + shift[j]
    return out


def training_pairs(points, lens, trans=None, keypts_pairs=None, pair_start=None, radius=0.45, keypts_num=1024, min_matches=1024, seed=0,
                   step=0, augment=AUGMENT_KITTI, first_pair=0, params=None):
    """The whole call on the host -> dict(points, backup, anc_idx, pos_idx (-1: not written), n, row0, matches, status, params, lists).
    params: use these f32[2 P, 16] in the row pass instead of the restatement's own (the device's, for the bit-for-bit row test)."""
    points = np.asarray(points, f32).reshape(-1, 3)
    N = len(points)
    off = [0]
    for l in np.asarray(lens).reshape(-1):
        off.append(off[-1] + min(max(int(l), 0), N - off[-1]))
    P, k = (len(off) - 1) // 2, int(keypts_num)
    out = dict(points=points.copy(), backup=points.copy(), anc_idx=np.full((P, k), -1, np.int32), pos_idx=np.full((P, k), -1, np.int32),
               n=np.zeros(P, np.int32), row0=np.asarray(off[::2], np.int32), matches=np.zeros(P, np.int32), status=np.zeros(P, np.int32),
               params=np.zeros((2 * P, 16), f32), lists=[])
    for p in range(P):
        pair = first_pair + p
        a0, a1, b1 = off[2 * p], off[2 * p + 1], off[2 * p + 2]
        for side, (r0, r1) in enumerate(((a0, a1), (a1, b1))):
            out["params"][2 * p + side] = cloud_params(seed, step, pair, side, augment)
            use = out["params"][2 * p + side] if params is None else np.asarray(params, f32)[2 * p + side]
            out["points"][r0:r1] = augment_rows(seed, step, pair, side, augment["augment_noise"], use, points[r0:r1])
        if keypts_pairs is None:
            out["backup"][a0:a1] = move(trans[p], points[a0:a1])
            lst, _ = matches(points[a0:a1], points[a1:b1], trans[p], radius)
            M = len(lst)
            st = (FEW_MATCHES if M < min_matches else 0) | (BELOW_KEYPTS if M < k else 0)
            sel = floyd(seed, step, pair, M, k) if not st else None
        else:
            s0, s1 = int(pair_start[p]), int(pair_start[p + 1])
            M = s1 - s0
            if s0 < 0 or M < 0 or s1 > len(keypts_pairs):
                st, M = LIST_RANGE, 0
            else:
                st = BELOW_KEYPTS if M < 1 else 0
            lst = np.asarray(keypts_pairs, np.int64).reshape(-1, 2)[s0:s0 + M]
            sel = with_replacement(seed, step, pair, M, k) if not st else None
        out["lists"].append(lst)
        out["matches"][p], out["status"][p] = M, st
        if not st:
            out["n"][p] = k
            out["anc_idx"][p] = lst[sel, 0]
            out["pos_idx"][p] = lst[sel, 1] + (a1 - a0)
    return out
