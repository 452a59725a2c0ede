"""TEST INFRASTRUCTURE ONLY.  Seeded inputs and float64 / integer expectations for the branch tests of the four single-pair
registration entry points (tests/test_gpu_registration_branches.py on the GPU, tests/test_registration_cases.py on the CPU):
d3f_feature_nn, d3f_mutual_matches, d3f_ransac_hypotheses (csrc/registration.hip) and d3f_neighbor_grid_score
(csrc/radius_neighbors.hip).  numpy only; the RANSAC expectations come from oracle/registration_np.py, the descriptor distances from
a function the caller hands in (tests/matching_np.d2_f64).  Every builder states what its case means to exercise; the CPU test checks
those statements, every margin and every cap from these expectations alone.

  nn_*      d3f_feature_nn: nn_launch mirrors the launch arithmetic of the entry point (row blocks, column splits, rows per split) only
            to say WHICH tile shapes a case runs, never what the result is
  mm_*      d3f_mutual_matches: crafted ab / ba arrays, the expected pairs in three lines of numpy
  rs_*      d3f_ransac_hypotheses: per hypothesis the oracle's result, the stage at which it ended and the conditioning of Horn's matrix
  sc_*      d3f_neighbor_grid_score: lattice inputs whose fp32 arithmetic is exact (integer expectation) and room-surface inputs whose
            every decision is further from its threshold than 8 x the fp32 error (float64 brute force)"""
import numpy as np

from oracle import registration_np as onp

FLT_MAX = np.float32(3.402823466e38)
SENT_I = np.int32(-77777)                 # pre-filled integer outputs
SENT_F = np.float32(-7.25e9)              # pre-filled float outputs
PAD = 9                                   # rows every output buffer is longer than its documented extent


def f32(x):
    """the value a C float argument receives, as a Python float"""
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def unit(rng, n, c):
    x = rng.standard_normal((n, c)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---- d3f_feature_nn --------------------------------------------------------------------------------------------------------------
NN_WIDTHS = (16, 32, 64)
# (Na, Nb): one row and column; one short of / exactly / one past a 256-row block and a 128-row tile; three row blocks with nine
# ragged column splits; one tile per split with a last tile of 32 and of 33 rows; no columns; no rows
NN_SHAPES = [(1, 1), (255, 127), (256, 128), (257, 129), (700, 1025), (3, 20000), (3, 20001), (300, 0), (0, 5)]
NN_TILE = 128
# what nn_launch must say about the shapes: (row blocks, column splits, rows per split, rows of the last split)
NN_INTENT = {(1, 1): (1, 1, 1, 1), (255, 127): (1, 1, 127, 127), (256, 128): (1, 1, 128, 128), (257, 129): (2, 2, 65, 64),
             (700, 1025): (3, 9, 114, 113), (3, 20000): (1, 157, 128, 32), (3, 20001): (1, 157, 128, 33)}


def nn_launch(Na, Nb):
    """(row blocks bx, column splits by, rows per split, [(j0, j1) of every split]) as d3f_feature_nn launches Na x Nb (Na, Nb > 0)"""
    bx = cdiv(Na, 256)
    by = max(min(cdiv(1024, bx), cdiv(Nb, NN_TILE)), 1)
    per = cdiv(Nb, by)
    return bx, by, per, [(y * per, min(Nb, y * per + per)) for y in range(by)]


def nn_data(C, Na, Nb, scale=1.0):
    """random unit descriptors A f32[Na, C], B f32[Nb, C] (times `scale`, rounded to fp32), seeded by the shape"""
    rng = np.random.default_rng(1000003 * C + 1009 * Na + Nb)
    s = np.float32(scale)
    return unit(rng, Na, C) * s, unit(rng, Nb, C) * s


def nn_tie_data(C):
    """every descriptor of B twice, 300 rows apart (5 column splits of 120 rows: the copies lie in different splits, the atomicMin key
    decides), and rows 1, 3, .., 59 copies of rows 0, 2, .., 58 (neighbours in one tile: the strict comparison of the walk decides);
    A = the first 300 rows in a random order -> (A, B, the expected index: the FIRST of the two or four bit-equal rows, d2 = 0)"""
    rng = np.random.default_rng(77 + C)
    B = unit(rng, 600, C)
    B[1:60:2] = B[0:60:2]
    B[300:] = B[:300]
    perm = rng.permutation(300)
    want = np.where((perm < 60) & (perm % 2 == 1), perm - 1, perm)
    return B[perm].copy(), B, want.astype(np.int64)


NN_NOFINITE_ROWS = {5: "nan", 130: "huge", 258: "nan", 259: "huge"}      # rows of A without a finite distance (two row blocks)
NN_NOFINITE_NAN_COLUMN = 17                                              # a row of B that is all NaN: never the answer


def nn_nofinite_data(C):
    """260 x 300 unit descriptors; rows NN_NOFINITE_ROWS of A are all NaN / all 3e19 (every d2 overflows fp32: C * 9e38 > FLT_MAX),
    row 17 of B is all NaN"""
    A, B = nn_data(C, 260, 300)
    for r, kind in NN_NOFINITE_ROWS.items():
        A[r] = np.nan if kind == "nan" else np.float32(3e19)
    B[NN_NOFINITE_NAN_COLUMN] = np.nan
    return A, B


def records(X, C):
    """record rows [xyz | descriptor | score] f32[n + 1, C + 4] with NaN in every float that is not a descriptor (reading one would
    show), one spare row; the descriptors start 12 bytes into the buffer and are C + 4 floats apart"""
    rec = np.full((len(X) + 1, C + 4), np.nan, np.float32)
    rec[:len(X), 3:3 + C] = X
    return rec


def nn_bound(C, d2):
    """the tolerance of the fp32 chain on a squared distance: C fmaf steps over non-negative terms and one rounding per difference"""
    return (C + 4) * 2.0 ** -24 * d2


def nn_reference(A, B, C, d2_f64):
    """float64 expectation of A against B: dict(D f64[Na, Nb] (NaN columns -> inf), idx, d2 (the argmin and minimum, lowest index on
    exact ties), idx2, d2_2 (second best; -1 / inf with one column), sure (bool: the float64 gap exceeds twice the bound at the
    minimum, so the fp32 argmin is the float64 one), sliver (rows whose gap lies between that and the sum of both bounds))"""
    with np.errstate(invalid="ignore", over="ignore"):
        D = d2_f64(A, B) if len(B) else np.zeros((len(A), 0))
    D = np.where(np.isnan(D), np.inf, D)
    n = len(A)
    if D.shape[1] == 0:
        return dict(D=D, idx=np.full(n, -1, np.int64), d2=np.full(n, np.inf), idx2=np.full(n, -1, np.int64), d2_2=np.full(n, np.inf),
                    sure=np.ones(n, bool), sliver=np.zeros(n, bool))
    idx = D.argmin(1)
    d2 = D[np.arange(n), idx]
    if D.shape[1] > 1:
        E = D.copy()
        E[np.arange(n), idx] = np.inf
        idx2 = E.argmin(1)
        d2_2 = E[np.arange(n), idx2]
    else:
        idx2, d2_2 = np.full(n, -1, np.int64), np.full(n, np.inf)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(d2), d2_2 - d2, np.inf)
        sure = gap > 2.0 * nn_bound(C, d2)
        sliver = sure & ~(gap > nn_bound(C, d2) + nn_bound(C, np.where(np.isfinite(d2_2), d2_2, 0.0)))
    return dict(D=D, idx=idx, d2=d2, idx2=idx2, d2_2=d2_2, sure=sure, sliver=sliver)


# ---- d3f_mutual_matches ----------------------------------------------------------------------------------------------------------
MM_NA = (0, 1, 1023, 1024, 1025, 3077)    # both sides of the 1024-entry scan tile; 3077 = three tiles and five entries
MM_FILLS = ("all", "none", "half", "invalid")


def mm_nb(Na):
    return sorted({0, 7, Na, 2 * Na})


def _mm_break(rng, ab, ba, cols):
    """make ba[c] point at a row that does not point back, for every c of cols"""
    Na = len(ab)
    for c in cols:
        if Na == 1:
            ba[c] = -1 if ab[0] == c else 0
            continue
        r = int(rng.integers(0, Na))
        while ab[r] == c:
            r = int(rng.integers(0, Na))
        ba[c] = r


def mm_case(Na, Nb, fill):
    """(ab i32[Na], ba i32[Nb]).  all: min(Na, Nb) rows get a column of their own that points back (a permutation and its inverse when
    Nb == Na), further rows share columns, further columns point anywhere -> min(Na, Nb) mutual pairs; none: every used column points
    at a row that does not point back (a derangement when Nb == Na); half: `all` with a random half of its pairs broken; invalid:
    `half` with a tenth of ab set to -1 and a tenth to values >= Nb (Nb itself, Nb + 3, INT_MAX).  Nb == 0: ab in -1 .. 5, all of it
    outside the columns."""
    rng = np.random.default_rng(7 + 31 * Na + 1000003 * Nb + MM_FILLS.index(fill))
    if Nb == 0:
        return rng.integers(-1, 6, Na).astype(np.int32), np.zeros(0, np.int32)
    m = min(Na, Nb)
    rows, cols = rng.permutation(Na), rng.permutation(Nb)[:m]
    ab = rng.integers(0, Nb, Na).astype(np.int64)
    if Na > Nb:
        ab[rows[m:]] = cols[rng.integers(0, m, Na - m)]
    ab[rows[:m]] = cols
    ba = rng.integers(0, max(Na, 1), Nb).astype(np.int64)
    ba[cols] = rows[:m]
    if fill == "none":
        _mm_break(rng, ab, ba, np.unique(ab))
    elif fill in ("half", "invalid"):
        _mm_break(rng, ab, ba, cols[rng.random(m) < 0.5])
    if fill == "invalid":
        u = rng.random(Na)
        ab[u < 0.1] = -1
        big = (u >= 0.1) & (u < 0.2)
        ab[big] = np.asarray([Nb, Nb + 3, 2 ** 31 - 1])[rng.integers(0, 3, int(big.sum()))]
    return ab.astype(np.int32), ba.astype(np.int32)


def mm_expected(ab, ba, Nb):
    """i64[k, 2]: the pairs (i, ab[i]) with ba[ab[i]] == i, ascending i"""
    i = np.arange(len(ab))
    ok = (ab >= 0) & (ab < Nb)
    ok[ok] = ba[ab[ok]] == i[ok]
    return np.stack([i[ok], ab[ok].astype(np.int64)], 1)


# ---- d3f_ransac_hypotheses -------------------------------------------------------------------------------------------------------
RS_H = 1999                                                   # not a multiple of 256
RS_SEEDS = ((12345, 0), ((1 << 63) + 11, (1 << 32) + 5))      # (seed, it0): the second pair needs all 64 bits of both
RS_CHECKERS = ((0.0, 0.0), (0.9, 0.0), (0.0, 0.05), (0.9, 0.05))
RS_RELGAP = 1e-3
REPEAT, NO_MATCH, EDGE, DISTANCE, OK = range(5)               # index into onp.STAGES


def pair(seed, n=400, outliers=0.3, noise=0.003):
    """the _pair construction of tests/test_gpu_registration.py: target keypoints on a room surface, source = the same points moved by
    a known rigid motion (+ noise) and shuffled, a share of the descriptors replaced by unrelated ones"""
    from d3feat_amd.utils.synthetic import room_fragment
    rng = np.random.default_rng(seed)
    tgt = room_fragment(seed, n_raw=20000, edge=2.0)[rng.permutation(20000)[:n]].astype(np.float32)
    ang = rng.uniform(-0.6, 0.6, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-0.5, 0.5, 3)
    src = ((tgt.astype(np.float64) - t) @ R + rng.normal(scale=noise, size=tgt.shape)).astype(np.float32)
    perm = rng.permutation(n)
    src = src[perm]
    d_t = unit(rng, n, 32)
    d_s = d_t[perm] + 0.05 * rng.standard_normal((n, 32)).astype(np.float32)
    bad = rng.random(n) < outliers
    d_s[bad] = unit(rng, int(bad.sum()), 32)
    d_s /= np.linalg.norm(d_s, axis=1, keepdims=True)
    return src, tgt, d_s.astype(np.float32), d_t, R, t


_RS_DATA = {}


def rs_data(kind):
    """(src f32[Ns, 3], tgt f32[Nt, 3], nn i32[Ns]).  full: pair(3, n=300), nn from the oracle (not injective: unrelated descriptors
    land on targets that have a match already); badnn: the same with a tenth of nn set to -1 and a tenth to Nt; five: the first
    five source points (ransac_n = 4: four draws of five are distinct once in five; ransac_n = 8: never)"""
    if kind not in _RS_DATA:
        src, tgt, ds, dt, _, _ = pair(3, n=300)
        nn = onp.feature_nn(ds, dt)[0].astype(np.int32)
        if kind == "badnn":
            u = np.random.default_rng(41).random(300)
            nn[u < 0.1] = -1
            nn[(u >= 0.1) & (u < 0.2)] = 300
        if kind == "five":
            src, nn = src[:5].copy(), nn[:5].copy()
        for a in (src, tgt, nn):
            a.setflags(write=False)
        _RS_DATA[kind] = (src, tgt, nn)
    return _RS_DATA[kind]


class RansacCase:
    def __init__(self, data, n, checkers, which_seed, all_repeat=False):
        self.data, self.n, self.all_repeat = data, n, all_repeat
        self.edge_similarity, self.checker_distance = f32(checkers[0]), f32(checkers[1])      # what the C floats hold
        self.seed, self.it0 = RS_SEEDS[which_seed]
        self.name = "%s-n%d-e%g-d%g-s%d" % (data, n, checkers[0], checkers[1], which_seed)


def _rs_cases():
    cs = []
    for a, n in enumerate((3, 4, 5, 8)):
        for b, ck in enumerate(RS_CHECKERS):
            cs.append(RansacCase("full", n, ck, (a + b) % 2))
    cs += [RansacCase("badnn", 3, RS_CHECKERS[3], 1), RansacCase("badnn", 4, RS_CHECKERS[0], 0), RansacCase("badnn", 5, RS_CHECKERS[1], 1),
           RansacCase("badnn", 8, RS_CHECKERS[2], 0),
           RansacCase("five", 4, RS_CHECKERS[0], 0), RansacCase("five", 4, RS_CHECKERS[0], 1),
           RansacCase("five", 8, RS_CHECKERS[0], 1, all_repeat=True)]
    return {c.name: c for c in cs}


RS_CASES = _rs_cases()


def horn_matrix(S):
    """Horn 1987's symmetric 4 x 4 matrix of the cross-covariance S[a][b] = sum s~_a t~_b: its largest eigenvector is the quaternion of
    the rotation that maximises tr(R S)"""
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def horn_rotation(S):
    """the rotation of horn_matrix(S)'s largest eigenvector by numpy.linalg.eigh (an independent route to kabsch's SVD)"""
    w, x, y, z = np.linalg.eigh(horn_matrix(S))[1][:, -1]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


_RS_REF = {}


def rs_reference(case):
    """per hypothesis h = 0 .. RS_H - 1 (iteration it0 + h) of a case: dict(stage i64[H] (REPEAT .. OK), T f64[H, 12] (the oracle's
    [R | t] where the fit was reached, else the identity), S f64[H, 3, 3], ms, mt f64[H, 3] (the sample means), scale f64[H]
    (|s~|_F |t~|_F), relgap f64[H] ((l1 - l2) / scale of Horn's matrix; inf where the fit was not reached), edge f64[H] (smallest edge
    ratio, NaN where not computed), dist f64[H] (largest aligned distance, NaN where not computed), dup_t bool[H] (the fit was reached
    with two equal target points in the sample))"""
    if case.name in _RS_REF:
        return _RS_REF[case.name]
    src, tgt, nn = rs_data(case.data)
    H = RS_H
    ident = np.eye(3, 4).reshape(12)
    out = dict(stage=np.zeros(H, np.int64), T=np.tile(ident, (H, 1)), S=np.zeros((H, 3, 3)), ms=np.zeros((H, 3)), mt=np.zeros((H, 3)),
               scale=np.zeros(H), relgap=np.full(H, np.inf), edge=np.full(H, np.nan), dist=np.full(H, np.nan), dup_t=np.zeros(H, bool))
    for h in range(H):
        tr = onp.hypothesis_trace(src, tgt, nn, case.n, case.edge_similarity, case.checker_distance, case.seed, case.it0 + h)
        out["stage"][h] = onp.STAGES.index(tr["stage"])
        if tr["edge"] is not None:
            out["edge"][h] = tr["edge"]
        if tr["R"] is None:
            continue
        s, t = tr["s"], tr["t"]
        out["dup_t"][h] = len(set(tr["ti"])) < case.n
        ms, mt = s.mean(0), t.mean(0)
        sc, tc = s - ms, t - mt
        S = sc.T @ tc
        lam = np.linalg.eigvalsh(horn_matrix(S))
        scale = np.linalg.norm(sc) * np.linalg.norm(tc)
        out["T"][h] = np.concatenate([tr["R"], tr["tr"][:, None]], 1).reshape(12)
        out["S"][h], out["ms"][h], out["mt"][h], out["scale"][h] = S, ms, mt, scale
        out["relgap"][h] = (lam[3] - lam[2]) / scale if scale > 0 else 0.0
        if tr["dist"] is not None:
            out["dist"][h] = tr["dist"]
    for v in out.values():
        v.setflags(write=False)
    _RS_REF[case.name] = out
    return out


# ---- d3f_neighbor_grid_score -----------------------------------------------------------------------------------------------------
SC_UNIT = 2.0 ** -6                       # lattice step of the exact case
SC_R_INT = 10                             # its radius in lattice steps: 6^2 + 8^2 = 10^2 puts a lattice point exactly on the sphere


def _signed_perm(axes, signs):
    P = np.zeros((3, 3), np.int64)
    for r in range(3):
        P[r, axes[r]] = signs[r]
    return P


def sc_exact():
    """Everything a multiple of 2^-6: sources and targets in [0, 4), transforms = signed axis permutations and lattice translations,
    radius 10 steps.  Every product, sum and square of the kernel is then exact in fp32 (integers below 2^24 in units of 2^-12), so
    count, nearest and sumd2 have ONE right answer, given by sc_exact_expected in integers.
    Hypothesis 0 is not the identity; under it are planted (the moved source point q, its targets):
      three ties      q + (3,0,0) / q - (3,0,0);  q - (0,0,5) / q + (0,0,5);  q + (2,2,1) / q + (-1,2,2) -- equal distances, the lower
                      index named first: on the high x side in the first tie, on the low z side in the second (a walk in ascending
                      cell order meets it last in one and first in the other); the lower index must win
      on the sphere   q + (6,8,0) and q + (10,0,0): distance exactly the radius, nothing nearer -> no inlier
      one step inside q + (9,0,0) -> an inlier
    -> dict(src, tgt f32[., 3], T f32[V, 12], radius, src_i, tgt_i (lattice integers), P i64[V, 3, 3], tau i64[V, 3], planted =
    {name: source row})"""
    rng = np.random.default_rng(2024)
    P0, tau0 = _signed_perm((1, 2, 0), (-1, 1, 1)), np.array([255 + 3, -5, 2])
    hyps = [(P0, tau0), (np.eye(3, dtype=np.int64), np.zeros(3, np.int64)), (np.eye(3, dtype=np.int64), np.array([1, 0, 0])),
            (_signed_perm((2, 1, 0), (1, -1, -1)), np.array([-4, 255 + 6, 255])), (P0, tau0 + np.array([0, 12, 0]))]
    S = rng.integers(0, 256, (300, 3))
    moved0 = S @ P0.T + tau0
    off0 = rng.integers(-7, 8, (200, 3))
    off0[:10] = 0
    tg = [np.clip(moved0[:200] + off0, 0, 255),                                   # near the moved sources of hypothesis 0 (ten ON them)
          np.clip(S[100:250] + rng.integers(-7, 8, (150, 3)), 0, 255),            # near the sources themselves (identity, lattice step)
          rng.integers(0, 256, (100, 3))]
    tg = np.concatenate(tg)
    q = np.array([[40, 40, 40], [120, 40, 200], [200, 200, 40], [40, 200, 120], [200, 40, 120], [120, 120, 120]])
    names = ("tie_x", "tie_z", "tie_skew", "sphere_68", "sphere_10", "inside")
    keep = (np.abs(tg[:, None, :] - q[None, :, :]).max(2) > 25).all(1)            # nothing else near a planted point
    tg = tg[keep]
    first = [q[0] + (3, 0, 0), q[1] - (0, 0, 5), q[2] + (2, 2, 1)]                  # in index order: 0, 1, 2, then 3, 4, 5 after 40 others
    second = [q[0] - (3, 0, 0), q[1] + (0, 0, 5), q[2] + (-1, 2, 2)]
    single = [q[3] + (6, 8, 0), q[4] + (10, 0, 0), q[5] + (9, 0, 0)]
    tg = np.concatenate([np.asarray(first), tg[:40], np.asarray(second), tg[40:], np.asarray(single)])
    qs = (q - tau0) @ P0                                                          # P0^-1 = P0^T for a signed permutation
    assert (qs >= 0).all() and (qs < 256).all() and (tg >= 0).all() and (tg < 256).all()
    planted = {nm: len(S) + k for k, nm in enumerate(names)}
    S = np.concatenate([S, qs])
    T = np.stack([np.concatenate([P.astype(np.float64), (tau * SC_UNIT)[:, None]], 1).reshape(12) for P, tau in hyps]).astype(np.float32)
    return dict(src=(S * SC_UNIT).astype(np.float32), tgt=(tg * SC_UNIT).astype(np.float32), T=T, radius=SC_R_INT * SC_UNIT,
                src_i=S, tgt_i=tg, P=np.stack([h[0] for h in hyps]), tau=np.stack([h[1] for h in hyps]), planted=planted)


def sc_exact_expected(c):
    """integer restatement: (count i64[V], sumd2 in 2^-32 units (Python ints), nearest i64[Ns] of hypothesis 0, D i64[V, Ns, Nt])"""
    moved = np.einsum("vrc,ic->vir", c["P"], c["src_i"]) + c["tau"][:, None, :]
    D = ((moved[:, :, None, :] - c["tgt_i"][None, None, :, :]) ** 2).sum(-1)
    best, j = D.min(2), D.argmin(2)                                               # argmin: the lowest index among equals
    inl = best < SC_R_INT ** 2                                                    # strictly inside
    count = inl.sum(1)
    sumd2 = [int(best[v][inl[v]].sum()) << 20 for v in range(len(D))]             # (2^-6)^2 = 2^-12 -> 2^-32 units
    return count, sumd2, np.where(inl[0], j[0], -1), D


SC_NT, SC_NS, SC_V = (1, 50, 3000), (0, 1, 257, 1000), (1, 2, 37)
SC_RADIUS = f32(0.05)
SC_FACTOR = 8.0
_SC = {}


def _rot(ang):
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def sc_brute(src, tgt, T, radius):
    """float64 brute force of every (hypothesis, source point) against every target, and the fp32 form of the two nearest distances.
    -> dict(b1, b2 f64[V, Ns] (nearest and second nearest d2; inf without), j1 i64[V, Ns], err_rows f64[V, Ns] = |float64 - fp32| of
    the nearest / second nearest d2 where below 4 r^2 (further ones decide nothing; the larger of the two), err = its maximum,
    r2 = (fp32(r) * fp32(r), r * r))"""
    V, Ns, Nt = len(T), len(src), len(tgt)
    t64, s64 = tgt.astype(np.float64), src.astype(np.float64)
    b1, b2, j1 = np.full((V, Ns), np.inf), np.full((V, Ns), np.inf), np.zeros((V, Ns), np.int64)
    r = float(radius)
    err_rows = np.zeros((V, Ns))
    rows = np.arange(Ns)
    for v in range(V):
        M = T[v].reshape(3, 4)
        if Ns == 0:
            continue
        p = s64 @ M[:, :3].astype(np.float64).T + M[:, 3].astype(np.float64)
        D = (p[:, None, 0] - t64[None, :, 0]) ** 2
        D += (p[:, None, 1] - t64[None, :, 1]) ** 2
        D += (p[:, None, 2] - t64[None, :, 2]) ** 2
        j1[v] = D.argmin(1)
        b1[v] = D[rows, j1[v]]
        cols = [j1[v]]
        if Nt > 1:
            D[rows, j1[v]] = np.inf
            j2 = D.argmin(1)
            b2[v] = D[rows, j2]
            cols.append(j2)
        # fp32, every step rounded (the kernel fuses the transform: the difference is part of what err measures)
        q = np.stack([M[a, 0] * src[:, 0] + (M[a, 1] * src[:, 1] + (M[a, 2] * src[:, 2] + M[a, 3])) for a in range(3)], 1)
        for k, jj in enumerate(cols):
            d = q - tgt[jj]
            d32 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ref = b1[v] if k == 0 else b2[v]
            near = ref < 4 * r * r
            err_rows[v][near] = np.maximum(err_rows[v][near], np.abs(ref[near] - d32[near].astype(np.float64)))
    return dict(b1=b1, b2=b2, j1=j1, err_rows=err_rows, err=float(err_rows.max(initial=0.0)),
                r2=(float(np.float32(radius) * np.float32(radius)), r * r))


def sc_brute_rows(br, keep):
    """sc_brute of the source rows `keep` alone, from the result for a superset (every row is computed on its own)"""
    out = {k: br[k][:, keep] for k in ("b1", "b2", "j1", "err_rows")}
    out["err"], out["r2"] = float(out["err_rows"].max(initial=0.0)), br["r2"]
    return out


def sc_margins(br, factor=SC_FACTOR):
    """bool[V, Ns]: the nearest d2 is further than factor x err from the squared radius (in both of its forms) and, where it is an
    inlier, further than that from the second nearest"""
    band = np.minimum(np.abs(br["b1"] - br["r2"][0]), np.abs(br["b1"] - br["r2"][1]))
    tol = factor * br["err"]
    return (band > tol) & ((br["b1"] >= min(br["r2"])) | (br["b2"] - br["b1"] > tol))


def sc_random(Nt, Ns, V):
    """Targets: Nt points of a room surface (edge 2).  Sources: targets moved back by a known motion plus noise of 0 .. 1.6 radii, so
    about five in eight are inliers under the true motion, many with several targets inside the radius.  Hypotheses (fp32 [R | t]):
    the true motion perturbed by up to 0.004 rad / 0.004 per axis; from V = 2 on, hypothesis 1 moves the whole source past the far x
    side of the grid by 64 radii and more (clamp to cell dims + 1: no inlier); V = 37 adds the same on -y and +z and three
    hypotheses (4, 5, 6) that FLATTEN the source onto the plane half a radius below the grid's lower x, y, z side in turn (a
    3 x 4 matrix with a zero row: every moved point in cell -1 of that axis, the targets of cell 0 still reachable).
    Source candidates that would decide within 8 x err of a threshold under ANY of the hypotheses are left out (sc_margins), so the
    float64 brute force fixes count and nearest exactly.
    -> dict(src, tgt, T f32, radius, brute = sc_brute of these arrays, special = {name: hypothesis index}, lo = the targets' minimum)"""
    key = (Nt, Ns, V)
    if key in _SC:
        return _SC[key]
    from d3feat_amd.utils.synthetic import room_fragment
    rng = np.random.default_rng(90001 + 7 * Nt + 1013 * Ns + V)
    r = SC_RADIUS
    tgt = room_fragment(11, n_raw=20000, edge=2.0)[rng.permutation(20000)[:Nt]].astype(np.float32)
    R, t = _rot(rng.uniform(-0.6, 0.6, 3)), rng.uniform(-0.5, 0.5, 3)
    ncand = Ns + Ns // 4 + 8 if Ns else 0
    k = rng.integers(0, Nt, ncand)
    noise = rng.standard_normal((ncand, 3))
    noise *= (rng.uniform(0, 1.6 * r, ncand) / np.linalg.norm(noise, axis=1))[:, None]
    src = ((tgt[k].astype(np.float64) - t) @ R + noise).astype(np.float32)
    T = np.zeros((V, 3, 4))
    for v in range(V):
        T[v, :, :3], T[v, :, 3] = R @ _rot(rng.uniform(-0.004, 0.004, 3)), t + rng.uniform(-0.004, 0.004, 3)
    special = {}
    lo, hi = tgt.astype(np.float64).min(0), tgt.astype(np.float64).max(0)
    ext = float(np.abs(src).max(initial=0.0)) * 2 + float((hi - lo).max())
    if V >= 2:
        for v, (axis, sign) in ((1, (0, 1)), (2, (1, -1)), (3, (2, 1))):
            if v < V and (v == 1 or V == 37):
                T[v, axis, 3] += sign * (ext + 64 * r)
                special["far_%s" % "xyz"[axis]] = v
    if V == 37:
        for v, axis in ((4, 0), (5, 1), (6, 2)):
            T[v, axis, :3], T[v, axis, 3] = 0.0, lo[axis] - 0.5 * r
            special["flat_%s" % "xyz"[axis]] = v
    T = T.reshape(V, 12).astype(np.float32)
    br = sc_brute(src, tgt, T, r)
    good = np.nonzero(sc_margins(br, SC_FACTOR * 1.01).all(0))[0] if Ns else np.zeros(0, np.int64)
    assert len(good) >= Ns, (key, len(good))
    good = good[:Ns]
    src = np.ascontiguousarray(src[good])
    br = sc_brute_rows(br, good)
    out = dict(src=src, tgt=tgt, T=T, radius=r, brute=br, special=special, lo=lo)
    _SC[key] = out
    return out


def sc_eps_p(src, T):
    """f64[V]: 4 * 2^-24 * max over points and rows of (|R| |s| + |t|) per hypothesis: the bound of the three-fmaf transform"""
    if len(src) == 0:
        return np.zeros(len(T))
    M = np.abs(T.astype(np.float64)).reshape(-1, 3, 4)
    return 4 * 2.0 ** -24 * (np.einsum("vrc,ic->vir", M[:, :, :3], np.abs(src.astype(np.float64))) + M[:, None, :, 3]).max((1, 2))


def sc_sumd2_tol(count, radius, eps_p):
    r = float(radius)
    return count * (2 * r * eps_p + 4 * 2.0 ** -24 * r * r + 2.0 ** -32)
