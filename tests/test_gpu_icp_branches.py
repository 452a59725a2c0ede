"""d3f_icp_pairs (csrc/nb_icp.h) and icp.icp_pairs where tests/test_gpu_icp.py does not reach: the size of the KITTI workload, grids
whose cells are not the radius, calls of more than 255 pairs, and fits away from the easy case.  The reference of every case is the
float64 restatement (tests/icp_np.py), run here or recorded in tests/golden/icp_sweep.npz (tools/make_golden_icp.py --sweep).  Each
case is the smallest shape that still takes its branch, and asserts that it does (chunk counts, icp_cases.cell_edge):

  1. more than 256 chunks per pair: sources of 65 537 rows (257 chunks, the smallest at which a thread of icp_finish_kernel adds a
     second chunk before the tree), 0 rows and 66 000 rows (258) in one call -- d3f_find_elem on the chunk offsets 0 / 257 / 257 / 515;
     and, because a total of 59 000 terms hides in its rounding where a chunk was added, five pairs in which only six chunks hold
     matched rows, one of them made by hand so that the header's order differs in the last bits from three wrong ones;
  2. two pairs at sweep size to convergence: 65 984 source rows against 20 000 targets over 160 m, the smallest pair of clouds that
     makes nb_prep double the cell edge three times (h = 8 r, dozens of targets per cell): the lb2 pruning decides which rows of cells
     are read; check_every 8 = 0, the batch = each pair alone;
  3. any built grid gives the same bits: grids built at 1, 3, 8 and 64 radii, and at r / 2 and r / 4 (K = 2 and 4, 32^3 cells: the
     finest a 500-row cloud can have within the 65 536-cell budget);
  4. a sprawling target: two outliers stretch the box until nearly every target shares one cell of at least 32 radii, with sources
     around the outliers, at exactly d2 == r r from one, and far outside;
  5. 300 pairs (255 + 45): the chunking of icp.icp_pairs -- row offsets, output slices, one grid per chunk -- against the restatement
     and against the two chunks run directly;
  6. lengths that exist only on the device: a negative one counts as 0, one past the stack is cut;
  7. non-finite rows: a target cloud with an inf and a NaN row gets the one-cell grid (inv_h = 0), non-finite source rows match nothing,
     and a finite pair in the same call is untouched;
  8. fits away from the easy case: planar correspondences (rank-2 S), a radius far larger than the cloud (every row matched,
     max_iteration exhausted), an init about 170 degrees from the identity, two correspondences (the rotation under-determined).

"The exact part" is count, iterations, converged, nearest and fitness; in a single search (max_iteration = 0) device and restatement
evaluate the same rounded expression, so sumd2 and rmse are bit-equal too and T keeps the init's bits.  Where the loop runs, the fit is
the one step whose bits differ (Jacobi against LAPACK): the margins of the restatement's run are asserted FIRST (>= 1e-9: a last-bit
difference in T cannot flip a correspondence or the stop test), then T is compared within max(64 x |T_eigh - T_svd|, 1e-12), the rule
of tests/test_gpu_icp.py, and rmse / sumd2 within what that tolerance can move them (_allowance).
"""
import os

import numpy as np
import pytest
import torch

import icp_cases
import icp_np
from conftest import GOLDEN
from icp_cases import OUT, R, cell_edge, host, rigid, rows, run_direct, run_pairs

pytestmark = pytest.mark.gpu

MARGIN = 1e-9       # the cap of tools/make_golden_icp.py
KITTI = dict(max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6, relative_rmse=1e-6)


def _gr(r):
    from d3feat_amd import icp
    return icp.grid_radius(r)


def _restate(pair, **kw):
    with np.errstate(invalid="ignore", over="ignore"):
        return icp_np.icp(pair[0], pair[1], pair[2], **kw)


def _restate_svd(pair, **kw):
    """The second run, with the other fit: only its T, iterations and nearest are used, so above 10 000 rows the k-d tree searches
    where scipy is installed (the same indices as the brute-force search wherever the margins hold; seconds less)."""
    nearest = icp_np.nearest_brute
    if len(pair[0]) > 10000:
        try:
            import scipy.spatial  # noqa: F401
            nearest = icp_np.nearest_ckdtree
        except ImportError:
            pass
    return _restate(pair, fit="svd", nearest=nearest, **kw)


def _back(M, pts):
    """the rows x with M x = pts: (pts - t) R, float64"""
    return (np.asarray(pts, np.float64) - M[:3, 3]) @ M[:3, :3]


def _check_exact_part(h, p, off, want):
    assert h["count"][p] == want.count and h["iterations"][p] == want.iterations and h["converged"][p] == want.converged, p
    assert np.array_equal(h["nearest"][off[p]:off[p + 1]], want.nearest), p
    assert h["fitness"][p] == want.fitness, p


def _check_single_search(h, p, off, pair, w):
    _check_exact_part(h, p, off, w)
    assert h["sumd2"][p] == w.sumd2 and h["rmse"][p] == w.rmse, p                    # bit-equal: the sums are in the header's order
    assert h["iterations"][p] == 0 and h["converged"][p] == 0
    init = np.eye(4) if pair[2] is None else np.asarray(pair[2], np.float64)
    assert np.array_equal(h["T"][p].reshape(3, 4), init[:3]), p                      # untouched: the init's bits


def _allowance(tol, pair, count, r):
    """What a T within tol of the restatement's can do (the derivation of test_gpu_icp._check_gold, per case): a source row moves by at
    most tol (|x| + |y| + |z| + 1) <= tol (3 max|coordinate| + 1) =: disp; rmse is a 2-norm over the rows divided by sqrt(count), so it
    moves by at most disp; each d <= r, so each d2 moves by at most 2 r disp and sum d2 by count times that."""
    src = np.asarray(pair[0], np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        m = float(np.max(np.abs(src[np.isfinite(src).all(axis=1)]), initial=0.0))
    disp = tol * (3.0 * m + 1.0)
    return disp, count * 2.0 * r * disp


def _check_within(h, p, what, T, rmse, sumd2, tol, pair, count, r):
    err = float(np.max(np.abs(h["T"][p].reshape(3, 4) - T[:3])))
    d_rmse, d_sum = _allowance(tol, pair, count, r)
    print("%s: T max difference %.3e (allowed %.3e), rmse %.3e (%.3e), sumd2 %.3e (%.3e)"
          % (what, err, tol, abs(h["rmse"][p] - rmse), d_rmse, abs(h["sumd2"][p] - sumd2), d_sum))
    assert err <= tol, what
    assert abs(h["rmse"][p] - rmse) <= d_rmse and abs(h["sumd2"][p] - sumd2) <= d_sum, what


def _margins(w):
    return min(w.margin_nn, w.margin_r, w.margin_stop)


def _check_loop(h, p, off, pair, what, margin_r=None, **kw):
    """the restatement with both fits; margins first; the exact part; T, rmse, sumd2 within tolerance -> the eigh run"""
    w, v = _restate(pair, fit="eigh", **kw), _restate_svd(pair, **kw)
    m = min(w.margin_nn, w.margin_r if margin_r is None else margin_r, w.margin_stop)
    print("%s: iterations %d converged %d count %d margin %.3e" % (what, w.iterations, w.converged, w.count, m))
    assert m >= MARGIN, what
    assert v.iterations == w.iterations and np.array_equal(v.nearest, w.nearest), what     # the two fits walk the same rounds
    tol = max(64.0 * float(np.max(np.abs(w.T - v.T))), 1e-12)
    _check_exact_part(h, p, off, w)
    _check_within(h, p, what, w.T, w.rmse, w.sumd2, tol, pair, w.count, kw["max_correspondence_distance"])
    return w


def _same_bits(a, b, what=""):
    for k in OUT:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _pair_of(h, p, off):
    return {k: (h[k][off[p]:off[p + 1]] if k == "nearest" else h[k][p:p + 1]) for k in OUT}


# ---- 1. more than 256 chunks per pair ------------------------------------------------------------------------------------------------------
def _order_sensitive_pairs(device):
    """With 59 000 matched rows the sum d2 is a thousand times a chunk's, and a chunk added to the wrong partial changes the rounding
    far below the last bit of the total: the bits would be the same nine times out of ten.  Here only the chunks 0, 1, 254, 255,
    256 and 257 hold matched rows, so the total is
        ((c0 + c256) + c254) + ((c1 + c257) + c255)
    of six terms of comparable size.  Pair 0 is made by hand: one matched row per chunk, at offsets of powers of two from a target at
    the origin under the identity, so every d2 is exact and the header's order differs IN THE LAST BITS from the chunks 256 / 257
    landing in other partials, swapped, or added after the tree (asserted below).  Pairs 1 to 4 are random ones of the same shape."""
    f32 = np.float32
    offs = {0: (-29, -28, -29), 1: (-28, None, -32), 254: (-29, -32, -29), 255: (None, -6, -6), 256: (None, -31, -30), 257: (-31, None, -32)}
    tgt = np.array([[9, 9, 9], [-9, 9, 9], [0, 0, 0], [9, -9, 9], [9, 9, -9]], f32)
    src = np.full((66000, 3), 4.0, f32)
    for c, e in offs.items():
        src[256 * c] = [0.0 if k is None else 2.0 ** k for k in e]
    d2 = {c: float((src[256 * c].astype(np.float64) ** 2) @ np.ones(3)) for c in offs}
    for c, e in offs.items():
        assert d2[c] == sum(0.0 if k is None else 4.0 ** k for k in e)               # exact: at most three bits each
    right = ((d2[0] + d2[256]) + d2[254]) + ((d2[1] + d2[257]) + d2[255])
    wrong = [(d2[0] + (d2[254] + d2[257])) + (d2[1] + (d2[255] + d2[256])),           # 256 -> partial 255, 257 -> partial 254
             (((d2[0] + d2[254]) + (d2[1] + d2[255])) + d2[256]) + d2[257],           # the second round added after the tree
             ((d2[0] + d2[257]) + d2[254]) + ((d2[1] + d2[256]) + d2[255])]           # 256 and 257 swapped
    assert all(w != right for w in wrong)
    pairs = [(src, tgt, None)]
    rng = np.random.default_rng(257)
    few = rng.uniform(0, 2, (60, 3)).astype(f32)
    M = rigid(2.0, (1, 2, 3), (0.03, -0.02, 0.01))
    for ns in (65793, 65850, 65900, 66000):
        s = few[rng.integers(0, 60, ns)].astype(np.float64) + rng.normal(0, 0.03, (ns, 3))
        far = np.ones(ns, bool)
        for c in offs:
            far[256 * c: 256 * (c + 1)] = False
        s[far] += 5.0
        pairs.append((_back(M, s).astype(f32), few, M))
    assert all((len(p[0]) + 255) // 256 == 258 for p in pairs)
    off = rows(pairs)
    kw = dict(max_correspondence_distance=0.2, max_iteration=0)
    h = host(run_pairs(device, pairs, check_every=0, **kw))
    for p, pair in enumerate(pairs):
        w = _restate(pair, **kw)
        matched = np.unique(np.nonzero(w.nearest >= 0)[0] // 256)
        assert set(matched) == set(offs) and np.all(np.nonzero(w.nearest >= 0)[0] // 256 < 258), p
        _check_single_search(h, p, off, pair, w)
    assert h["sumd2"][0] == right and h["count"][0] == 6


def test_more_than_256_chunks(device):
    rng = np.random.default_rng(65537)
    tgt = rng.uniform(0, 2, (600, 3)).astype(np.float32)
    M = rigid(2.0, (1, 2, 3), (0.03, -0.02, 0.01))
    pairs = []
    for ns in (65537, 0, 66000):
        s = tgt[rng.integers(0, 600, ns)].astype(np.float64) + rng.normal(0, 0.03, (ns, 3))
        s[rng.random(ns) < 0.1] += 5.0                                               # 10 % of the rows: no correspondence
        pairs.append((_back(M, s).astype(np.float32), tgt, M))
    off = rows(pairs)
    chunks = [(len(p[0]) + 255) // 256 for p in pairs]
    assert chunks == [257, 0, 258] and list(np.cumsum([0] + chunks)) == [0, 257, 257, 515]
    kw = dict(max_correspondence_distance=0.2, max_iteration=0)
    h = host(run_pairs(device, pairs, check_every=0, **kw))
    for p, pair in enumerate(pairs):
        w = _restate(pair, **kw)
        assert (w.count == 0) if p == 1 else (0.85 * len(pair[0]) < w.count < 0.95 * len(pair[0]))
        _check_single_search(h, p, off, pair, w)
    _order_sensitive_pairs(device)
    # the loop from the identity: the sources start 2 degrees and a few centimetres off
    pairs = [(s, t, None) for s, t, _ in pairs]
    kw = dict(KITTI, max_iteration=3)
    h = host(run_pairs(device, pairs, **kw))
    for p, pair in enumerate(pairs):
        w = _check_loop(h, p, off, pair, "%d rows" % len(pair[0]), **kw)
        assert (w.iterations, w.converged) == ((1, 1) if p == 1 else (3, 0))


# ---- 2. sweep size, cells of eight radii ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    return np.load(os.path.join(GOLDEN, "icp_sweep.npz"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "icp.npz"))


def _check_sweep(h, p, off, sweep, pair):
    assert h["iterations"][p] == int(sweep["iterations"][p]) and h["converged"][p] == int(sweep["converged"][p]) == 1
    assert np.array_equal(h["nearest"][off[p]:off[p + 1]], sweep["nearest"][p])
    assert h["count"][p] == int(sweep["count"][p]) and h["fitness"][p] == float(sweep["fitness"][p])
    tol = max(64.0 * float(sweep["fit_difference"][p]), 1e-12)
    _check_within(h, p, "sweep pair %d" % p, sweep["T"][p], float(sweep["rmse"][p]), float(sweep["sumd2"][p]), tol, pair,
                  int(sweep["count"][p]), 0.2)


def test_sweep_pairs_to_convergence(device, sweep):
    pairs = icp_cases.sweep_pairs()
    assert [icp_cases.pair_sha256(p) for p in pairs] == [str(x) for x in sweep["sha256"]]                # the inputs the fixture was made of
    assert [(len(p[0]) + 255) // 256 for p in pairs] == [258, 258]
    gr = _gr(0.2)
    assert np.array_equal(cell_edge([p[1] for p in pairs], gr), [8 * gr * (1 + 2.0 ** -20)] * 2)
    assert np.all(sweep["margins"] >= MARGIN)
    off = rows(pairs)
    every8 = host(run_pairs(device, pairs, check_every=8, **KITTI))
    for p in (0, 1):
        _check_sweep(every8, p, off, sweep, pairs[p])
    _same_bits(host(run_pairs(device, pairs, check_every=0, **KITTI)), every8, "check_every 0")
    for p in (0, 1):
        assert np.array_equal(cell_edge([pairs[p][1]], gr), [8 * gr * (1 + 2.0 ** -20)])
        _same_bits(host(run_pairs(device, [pairs[p]], **KITTI)), _pair_of(every8, p, off), "pair %d alone" % p)


# ---- 3. any built grid ----------------------------------------------------------------------------------------------------------------------
def test_any_built_grid_gives_the_same_bits(device, gold):
    # (a) the single-search cases of test_gpu_icp.py on coarser grids
    pairs = icp_cases.single_pass_pairs()
    off = rows(pairs)
    kw = dict(max_correspondence_distance=R, max_iteration=0)
    gr = _gr(R)
    assert gr == R
    base = run_direct(device, pairs, gr, check_every=0, **kw)
    for p, pair in enumerate(pairs):
        _check_single_search(base, p, off, pair, _restate(pair, **kw))
    for f in (1, 3, 8, 64):
        assert np.array_equal(cell_edge([p[1] for p in pairs], f * gr), [f * gr * (1 + 2.0 ** -20)] * 5), f       # no doubling: f radii
        _same_bits(run_direct(device, pairs, f * gr, check_every=0, **kw), base, "single search, %d radii" % f)
    # (b) the golden pair to convergence
    pair = (gold["src"], gold["tgt"], None)
    gr = _gr(0.2)
    base = run_direct(device, [pair], gr, **KITTI)
    assert np.all(gold["margins"] >= MARGIN)
    assert base["iterations"][0] == int(gold["iterations"]) and base["converged"][0] == int(gold["converged"])
    assert np.array_equal(base["nearest"], gold["nearest"]) and base["count"][0] == int(gold["count"])
    assert base["fitness"][0] == float(gold["fitness"])
    _check_within(base, 0, "golden pair", gold["T"], float(gold["rmse"]), float(gold["sumd2"]),
                  max(64.0 * float(gold["fit_difference"]), 1e-12), pair, int(gold["count"]), 0.2)
    for f in (1, 3, 8):
        edge = cell_edge([pair[1]], np.float32(f * gr))
        assert edge[0] >= f * gr, f
        _same_bits(run_direct(device, [pair], float(np.float32(f * gr)), **KITTI), base, "golden pair, %d radii" % f)
    # (c) cells finer than the radius: K = ceil(r / h ..) = 2 and 4 cells each way
    rng = np.random.default_rng(31)
    tgt = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    src = rng.uniform(0, 1, (400, 3)).astype(np.float32)
    pair = (src, tgt, rigid(1.0, (3, 1, 2), (0.01, -0.02, 0.015)))
    assert np.array_equal(cell_edge([tgt], R), [R * (1 + 2.0 ** -20)])
    for kw in (dict(max_correspondence_distance=R, max_iteration=0), dict(KITTI, max_correspondence_distance=R, max_iteration=3)):
        base = run_direct(device, [pair], R, **kw)
        if kw["max_iteration"] == 0:
            w = _restate(pair, **kw)
            assert 100 < w.count < 400
            _check_single_search(base, 0, [0, 400], pair, w)
        else:
            w = _check_loop(base, 0, [0, 400], pair, "compact pair", **kw)
            assert w.iterations == 3
        for div in (2, 4):
            edge = cell_edge([tgt], R / div)[0]
            assert edge == (R / div) * (1 + 2.0 ** -20) and edge < R and np.ceil(R / edge) == div        # no doubling: 16^3 / 32^3 cells
            _same_bits(run_direct(device, [pair], R / div, **kw), base, "r / %d, max_iteration %d" % (div, kw["max_iteration"]))


# ---- 4. a sprawling target --------------------------------------------------------------------------------------------------------------------
def test_sprawling_target(device):
    rng = np.random.default_rng(41)
    out_a, out_b = np.array([500.0, -400.0, 30.0]), np.array([-300.0, 600.0, -20.0])
    tgt = np.concatenate([rng.uniform(0, 2, (598, 3)), [out_a, out_b]]).astype(np.float32)
    near = np.concatenate([out_a + rng.uniform(-1, 1, (2, 3)) * R / (2 * np.sqrt(3)), out_b + rng.uniform(-1, 1, (2, 3)) * R / (2 * np.sqrt(3))])
    src = np.concatenate([tgt[rng.integers(0, 598, 690)].astype(np.float64) + rng.normal(0, 0.03, (690, 3)),     # jittered copies
                          near,                                                                                  # [690..693] within r / 2 of an outlier
                          [out_a + [R, 0, 0]],                                                                   # [694] d2 == r r exactly
                          [[40, 1, 1], [1, -55, 1], [1, 1, 70], [-1e4, 1e4, 0], [900, -900, 90]]]).astype(np.float32)   # far outside the box
    assert src.shape == (700, 3) and tgt.shape == (600, 3)
    assert cell_edge([tgt], _gr(R))[0] >= 32 * R                                    # nearly every target is in one cell
    kw = dict(max_correspondence_distance=R, max_iteration=0)
    pair = (src, tgt, None)
    w = _restate(pair, **kw)
    assert list(w.nearest[690:695]) == [598, 598, 599, 599, -1] and w.margin_r == 0.0 and np.all(w.nearest[695:] == -1)
    assert 400 < w.count <= 694
    _check_single_search(host(run_pairs(device, [pair], check_every=0, **kw)), 0, [0, 700], pair, w)
    # the loop from a small init (under the identity row 694 sits at a margin of 0 on purpose, which no loop can be compared at)
    pair = (src, tgt, rigid(0.002, (1, 2, 3), (0.004, -0.003, 0.002)))
    kw = dict(KITTI, max_correspondence_distance=R, max_iteration=3)
    w = _check_loop(host(run_pairs(device, [pair], **kw)), 0, [0, 700], pair, "sprawling target", **kw)
    assert w.nearest[690] == 598 and w.nearest[692] == 599


# ---- 5. more than 255 pairs ---------------------------------------------------------------------------------------------------------------------
def test_more_than_255_pairs(device):
    rng = np.random.default_rng(300)
    pairs = []
    for _ in range(300):
        nt, ns = int(rng.integers(5, 51)), int(rng.integers(0, 41))
        tgt = rng.uniform(0, 1, (nt, 3)).astype(np.float32)
        M = rigid(rng.uniform(0, 4), rng.normal(size=3), rng.normal(0, 0.02, 3))
        s = tgt[rng.integers(0, nt, ns)].astype(np.float64) + rng.normal(0, 0.01, (ns, 3))
        pairs.append((_back(M, s).astype(np.float32), tgt, None))
    kw = dict(KITTI, max_iteration=30)
    off = rows(pairs)
    res = run_pairs(device, pairs, check_every=8, **kw)
    h = host(res)
    compared, worst = 0, 0.0
    for p, pair in enumerate(pairs):
        w, v = _restate(pair, fit="eigh", **kw), _restate(pair, fit="svd", **kw)
        if _margins(w) < MARGIN or v.iterations != w.iterations or not np.array_equal(v.nearest, w.nearest):
            continue
        compared += 1
        _check_exact_part(h, p, off, w)
        tol = max(64.0 * float(np.max(np.abs(w.T - v.T))), 1e-12)
        err = float(np.max(np.abs(h["T"][p].reshape(3, 4) - w.T[:3])))
        worst = max(worst, err / tol)
        assert err <= tol, p
        d_rmse, d_sum = _allowance(tol, pair, w.count, 0.2)
        assert abs(h["rmse"][p] - w.rmse) <= d_rmse and abs(h["sumd2"][p] - w.sumd2) <= d_sum, p
        if p in (0, 254, 255, 299):
            i = np.nonzero(w.nearest >= 0)[0]
            assert np.array_equal(res.correspondences(p), np.stack([i, w.nearest[i]], axis=1).astype(np.int32)), p
    print("%d of 300 pairs compared, the largest T difference is %.3f of its allowance" % (compared, worst))
    assert compared >= 297
    assert sum(1 for p in pairs if len(p[0]) == 0) >= 1
    # the call = its two chunks run directly
    gr = _gr(0.2)
    for a, b in ((0, 255), (255, 300)):
        d = run_direct(device, pairs[a:b], gr, check_every=8, **kw)
        _same_bits(d, {k: (h[k][off[a]:off[b]] if k == "nearest" else h[k][a:b]) for k in OUT}, "pairs %d:%d" % (a, b))
    _same_bits(host(run_pairs(device, pairs, check_every=0, **kw)), h, "check_every 0")


# ---- 6. lengths that exist only on the device ---------------------------------------------------------------------------------------------------
def test_lengths_that_exist_only_on_the_device(device):
    from d3feat_amd import icp
    rng = np.random.default_rng(61)
    tgts = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in (120, 150, 400)]
    M = rigid(1.5, (2, -1, 1), (0.01, 0.02, -0.01))
    src = _back(M, np.concatenate([tgts[1][:10], tgts[2][:290]]).astype(np.float64) + rng.normal(0, 0.01, (300, 3))).astype(np.float32)
    cut = [(src[0:0], tgts[0], M), (src[0:10], tgts[1], M), (src[10:300], tgts[2], M)]        # what the lengths -3, 10, 1000 mean
    off = rows(cut)
    init = np.stack([M] * 3)
    for kw in (dict(max_correspondence_distance=R, max_iteration=0), dict(KITTI, max_correspondence_distance=R, max_iteration=3)):
        lens = torch.tensor([-3, 10, 1000], dtype=torch.int32, device=device)
        assert not hasattr(lens, "host_lens")
        res = icp.icp_pairs(torch.from_numpy(src).to(device), lens, torch.from_numpy(np.concatenate(tgts)).to(device),
                            [len(t) for t in tgts], init=init, **kw)
        h = host(res)
        assert h["nearest"].shape == (300,)
        for p, pair in enumerate(cut):
            if kw["max_iteration"] == 0:
                _check_single_search(h, p, off, pair, _restate(pair, **kw))
            else:
                _check_loop(h, p, off, pair, "length %d" % [-3, 10, 1000][p], **kw)
        assert h["count"][0] == 0 and h["count"][1] == 10 and 250 < h["count"][2] <= 290
        assert np.array_equal(res.correspondences(1)[:, 0], np.arange(10))
        # the same lengths straight into the C entry point: B = 3, N_src = 300
        _same_bits(run_direct(device, [(src, tgts[0], M), (src[:0], tgts[1], M), (src[:0], tgts[2], M)], _gr(R), src_lens=[-3, 10, 1000],
                              **kw), h, "run_direct")


# ---- 7. non-finite rows ---------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows(device):
    rng = np.random.default_rng(71)
    inf, nan = np.inf, np.nan
    good = rng.uniform(0, 1, (300, 3))
    tgt0 = np.concatenate([good, [[inf, 0, 0], [nan, nan, nan]]]).astype(np.float32)
    stand_in = tgt0.copy()
    stand_in[300:] = 1e6                                # the indices stay; np.argmin would otherwise pick the NaN
    M = rigid(1.0, (1, -2, 2), (0.01, -0.01, 0.02))
    src0 = np.concatenate([_back(M, good[rng.integers(0, 300, 257)] + rng.normal(0, 0.02, (257, 3))),
                           [[nan, 0, 0], [inf, 0, 0], [-inf, 1, 1]]]).astype(np.float32)
    tgt1 = rng.uniform(0, 1, (250, 3)).astype(np.float32)
    pair1 = (_back(M, tgt1[:200].astype(np.float64) + rng.normal(0, 0.02, (200, 3))).astype(np.float32), tgt1, M)
    pairs = [(src0, tgt0, M), pair1]
    off = rows(pairs)
    edges = cell_edge([tgt0, tgt1], _gr(R))
    assert edges[0] == np.inf and edges[1] == R * (1 + 2.0 ** -20)                   # pair 0: the one-cell grid, inv_h = 0
    for kw in (dict(max_correspondence_distance=R, max_iteration=0), dict(KITTI, max_correspondence_distance=R, max_iteration=3)):
        h = host(run_pairs(device, pairs, **kw))
        want0 = (src0, stand_in, M)
        if kw["max_iteration"] == 0:
            w = _restate(want0, **kw)
            _check_single_search(h, 0, off, want0, w)
        else:
            # the three non-finite rows come last and add +0.0 to every sum: the finite rows alone walk the same transforms, and give
            # the margin to the radius that the NaN rows hide in the full run
            fin = _restate((src0[:257], stand_in, M), **kw)
            w = _check_loop(h, 0, off, want0, "non-finite rows", margin_r=fin.margin_r, **kw)
            assert np.array_equal(fin.T, w.T) and fin.iterations == w.iterations and np.isfinite(fin.margin_r)
            assert np.all(np.isfinite(h["T"][0]))
        assert 200 < w.count <= 257 and np.all(w.nearest[257:] == -1) and np.all(w.nearest < 300)
        _same_bits(host(run_pairs(device, [pair1], **kw)), _pair_of(h, 1, off), "the finite pair alone")
        assert h["count"][1] > 150


# ---- 8. fits away from the easy case ----------------------------------------------------------------------------------------------------------------
def test_fits_away_from_the_easy_case(device):
    rng = np.random.default_rng(29)
    # planar: every correspondence on z = 0.5, S has rank 2
    flat = np.concatenate([rng.uniform(0, 1, (300, 2)), np.full((300, 1), 0.5)], axis=1).astype(np.float32)
    c = flat[:200].astype(np.float64).mean(axis=0)
    tilt = rigid(3.0, (1, 1, 0), (0, 0, 0))
    moved = (flat[:200].astype(np.float64) - c) @ tilt[:3, :3].T + c + [0.01, -0.015, 0.005]
    pair = (moved.astype(np.float32), flat, None)
    kw = dict(KITTI, max_correspondence_distance=R)
    w = _check_loop(host(run_pairs(device, [pair], **kw)), 0, [0, 200], pair, "planar", **kw)
    assert w.converged == 1 and w.count == 200 and np.all(flat[:, 2] == 0.5)
    # a radius far larger than the cloud, 170 degrees away: every row matched in every round, max_iteration exhausted
    cloud = rng.uniform(0, 1, (400, 3)).astype(np.float32)
    G = rigid(170.0, (1, 2, 3), (0.3, -0.2, 0.1))
    turned = (cloud[:300].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    pair = (turned, cloud, None)
    kw = dict(KITTI, max_correspondence_distance=1e3, max_iteration=30)
    assert cell_edge([cloud], _gr(1e3))[0] >= 1e3                                   # the default grid: one cell
    w = _check_loop(host(run_pairs(device, [pair], **kw)), 0, [0, 300], pair, "huge radius", **kw)
    assert w.count == 300 and w.fitness == 1.0 and (w.iterations, w.converged) == (30, 0)
    # the same clouds from an init that undoes the 170 degrees but for 2: the first update is small, the init is not
    init = rigid(2.0, (2, -1, 1), (0.01, 0.01, -0.01)) @ np.linalg.inv(G)
    pair = (turned, cloud, init)
    kw = dict(KITTI, max_correspondence_distance=R)
    w = _check_loop(host(run_pairs(device, [pair], **kw)), 0, [0, 300], pair, "170 degree init", **kw)
    assert w.converged == 1 and w.count == 300 and np.array_equal(w.nearest, np.arange(300))
    assert np.trace(init[:3, :3]) < -0.9                                            # about 170 degrees from the identity
    # two correspondences: the rotation about the line through them is not determined, so no T is compared
    src = np.array([[0.2, 0.3, 0.4], [0.7, 0.5, 0.6], [0.4, 5.0, 0.5]], np.float32)
    tgt = np.array([[0.24, 0.33, 0.38], [0.77, 0.49, 0.63], [50.0, 0.0, 0.0]], np.float32)
    pair = (src, tgt, None)
    kw = dict(KITTI, max_correspondence_distance=R)
    w, v = _restate(pair, fit="eigh", **kw), _restate(pair, fit="svd", **kw)
    print("two correspondences: iterations %d, eigh and SVD differ by %.3e" % (w.iterations, np.max(np.abs(w.T - v.T))))
    assert _margins(w) >= MARGIN and list(w.nearest) == [0, 1, -1] and w.converged == 1
    assert (v.count, v.iterations, v.converged) == (w.count, w.iterations, w.converged) and np.array_equal(v.nearest, w.nearest)
    h = host(run_pairs(device, [pair], **kw))
    _check_exact_part(h, 0, [0, 3], w)
    T = h["T"][0].reshape(3, 4)
    assert np.all(np.isfinite(T))
    assert np.max(np.abs(T[:, :3] @ T[:, :3].T - np.eye(3))) <= 1e-12 and abs(np.linalg.det(T[:, :3]) - 1.0) <= 1e-12
    cs, ct = src[:2].astype(np.float64).mean(axis=0), tgt[:2].astype(np.float64).mean(axis=0)
    assert np.max(np.abs(T[:, :3] @ cs + T[:, 3] - ct)) <= 1e-12
