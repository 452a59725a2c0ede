"""ICP refinement without a GPU: the float64 restatement (tests/icp_np.py) on its own (the summation order spelled out at 3 and at 258
chunks, the k-d tree search and its margins against the brute-force one), the margins of tests/golden/icp.npz and of
tests/golden/icp_sweep.npz (tools/make_golden_icp.py) and the inputs the latter is regenerated from, d3f_icp_pairs' argument checks, the cache files of d3feat_amd/datasets/kitti.py with the device call
replaced by the restatement, and the compat entry point's refusals."""
import ctypes
import os

import numpy as np
import pytest

import icp_cases
import icp_np
from conftest import GOLDEN, ROOT
from d3feat_amd.datasets import kitti

MARGIN = 1e-9       # the cap of tools/make_golden_icp.py


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "icp.npz"))


def _rigid(deg, axis, shift):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = shift
    return T


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_recovers_a_known_motion_on_an_exact_copy():
    """Target = the moved source, row for row: from an init one step away ICP ends at fitness 1 and rmse 0 (to rounding), on the motion."""
    rng = np.random.default_rng(3)
    src = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    G = _rigid(2.0, (0.2, 1.0, -0.4), (0.02, -0.03, 0.01))
    tgt = (src.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    for fit in ("eigh", "svd"):
        r = icp_np.icp(src, tgt, None, max_correspondence_distance=0.2, max_iteration=50, fit=fit)
        assert r.converged == 1 and r.count == 300 and r.fitness == 1.0
        assert r.rmse < 1e-6                                             # the float32 rounding of the target rows, nothing else
        assert np.max(np.abs(r.T - G)) < 1e-6, fit
        assert np.array_equal(r.nearest, np.arange(300))


def test_ckdtree_agrees_with_the_brute_force_search():
    pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    src, tgt = rng.uniform(0, 1, (400, 3)).astype(np.float32), rng.uniform(0, 1, (500, 3)).astype(np.float32)
    p = icp_np.move(_rigid(3.0, (1, 1, 0), (0.01, 0.0, 0.02))[:3], src)
    a, b = icp_np.nearest_brute(p, tgt, 0.08), icp_np.nearest_ckdtree(p, tgt, 0.08)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert 0 < (a[0] >= 0).sum() < 400                                   # some rows have a correspondence and some have none
    ra = icp_np.icp(src, tgt, None, max_correspondence_distance=0.08, max_iteration=5)
    rb = icp_np.icp(src, tgt, None, max_correspondence_distance=0.08, max_iteration=5, nearest=icp_np.nearest_ckdtree)
    assert np.array_equal(ra.T, rb.T) and ra.iterations == rb.iterations and np.array_equal(ra.nearest, rb.nearest)


def test_no_correspondence_gives_the_identity_update_and_converges_at_one():
    src = np.zeros((5, 3), np.float32)
    tgt = np.full((7, 3), 10.0, np.float32)
    T0 = _rigid(10.0, (0, 0, 1), (0.5, 0.0, 0.0))
    r = icp_np.icp(src, tgt, T0, max_correspondence_distance=0.2, max_iteration=200)
    assert r.count == 0 and r.fitness == 0.0 and r.rmse == 0.0 and r.iterations == 1 and r.converged == 1
    assert np.array_equal(r.T, T0) and np.all(r.nearest == -1)
    e = icp_np.icp(np.zeros((0, 3), np.float32), tgt, None)               # an empty source: the same path
    assert e.count == 0 and e.fitness == 0.0 and e.iterations == 1 and e.converged == 1
    z = icp_np.icp(src, tgt, T0, max_iteration=0)                          # max_iteration = 0: one search, no update
    assert z.iterations == 0 and z.converged == 0 and np.array_equal(z.T, T0)


def test_strict_radius_and_lowest_index():
    tgt = np.array([[0.25, 0, 0], [0, 0.125, 0], [0, -0.125, 0], [0.125, 0, 0]], np.float32)
    idx, d2, _, _ = icp_np.nearest_brute(np.zeros((1, 3)), tgt, 0.125)
    assert idx[0] == -1                                                   # d2 == r r exactly: excluded
    idx, d2, gap, _ = icp_np.nearest_brute(np.zeros((1, 3)), tgt, 0.2)
    assert idx[0] == 1 and d2[0] == 0.015625 and gap == 0.0               # three at equal d2: the lowest index


def test_summation_order_is_the_headers():
    """The chunk tree and the tree over chunks against math.fsum: the same value to rounding, and the order spelled out for 600 rows."""
    import math
    rng = np.random.default_rng(11)
    p, tgt = rng.normal(size=(600, 3)), rng.normal(size=(600, 3)).astype(np.float32)
    idx = np.arange(600)
    idx[::7] = -1
    d2 = np.where(idx >= 0, rng.random(600), 0.0)
    sm, n = icp_np.sums(p, tgt, idx, d2)
    assert n == int((idx >= 0).sum())
    assert abs(sm[0] - math.fsum(d2)) <= 1e-12 * math.fsum(d2)
    v = np.zeros(768)
    v[:600] = d2
    chunks = []
    for c in range(3):
        g = []
        for w in range(4):
            x = v[256 * c + 64 * w: 256 * c + 64 * w + 64].copy()
            for s in (32, 16, 8, 4, 2, 1):
                x[:s] = x[:s] + x[s:2 * s]
            g.append(x[0])
        chunks.append((g[0] + g[1]) + (g[2] + g[3]))
    assert sm[0] == ((0.0 + chunks[0]) + (0.0 + chunks[2])) + (0.0 + chunks[1])     # partials 0, 1, 2; tree: s = 2 adds [0] += [2], s = 1 [0] += [1]


def test_summation_order_at_258_chunks_restated_literally():
    """66 000 rows are 258 chunks: partial 0 adds chunks 0 and 256, partial 1 adds 1 and 257, every other partial one chunk.  The
    header's order in plain loops -- over the chunks, their four groups of 64 rows and the steps of the two trees -- against
    icp_np.sums, all 16 sums bit for bit (the restatement's own acc[c % 256] is otherwise only checked at 3 chunks)."""
    rng = np.random.default_rng(258)
    n = 66000
    p, tgt = rng.normal(size=(n, 3)) * [40.0, 40.0, 3.0], (rng.normal(size=(500, 3)) * [40.0, 40.0, 3.0]).astype(np.float32)
    idx = rng.integers(0, 500, n)
    idx[rng.random(n) < 0.1] = -1                                          # about 10 % of the rows have no correspondence
    d2 = np.where(idx >= 0, rng.random(n) * 0.04, 0.0)
    sm, cnt = icp_np.sums(p, tgt, idx, d2)
    assert cnt == int((idx >= 0).sum()) and 0.88 * n < cnt < 0.92 * n
    nc = (n + 255) // 256
    assert nc == 258
    x = tgt.astype(np.float64)
    v = np.zeros((nc * 256, 16))                                           # the last chunk padded with +0.0
    for i in range(n):
        if idx[i] >= 0:
            t = x[idx[i]]
            v[i] = [d2[i], p[i, 0], p[i, 1], p[i, 2], t[0], t[1], t[2], p[i, 0] * t[0], p[i, 0] * t[1], p[i, 0] * t[2],
                    p[i, 1] * t[0], p[i, 1] * t[1], p[i, 1] * t[2], p[i, 2] * t[0], p[i, 2] * t[1], p[i, 2] * t[2]]
    part = []
    for c in range(nc):
        g = []
        for w in range(4):
            lanes = v[256 * c + 64 * w: 256 * c + 64 * w + 64].copy()      # [64 rows, 16 sums]
            s_ = 32
            while s_ > 0:
                for t in range(s_):
                    lanes[t] = lanes[t] + lanes[t + s_]
                s_ //= 2
            g.append(lanes[0])
        part.append((g[0] + g[1]) + (g[2] + g[3]))
    red = []
    for t in range(256):                                                   # thread t: chunks t, t + 256, ... ascending, from 0.0
        acc = np.zeros(16)
        for c in range(t, nc, 256):
            acc = acc + part[c]
        red.append(acc)
    assert sum(1 for t in range(256) if len(range(t, nc, 256)) == 2) == 2
    s_ = 128
    while s_ > 0:
        for t in range(s_):
            red[t] = red[t] + red[t + s_]
        s_ //= 2
    assert np.array_equal(red[0], sm)
    assert np.all(sm[[0, 7, 11, 15]] != 0.0) and abs(sm[0] - d2.sum()) <= 1e-12 * d2.sum()


def test_ckdtree_margins_are_the_brute_force_ones():
    """600 rows against 300 targets: the same indices and d2, the same margin_nn, and a margin_r that is no smaller than the brute
    one (the nearest target's |d2 - r r| against every couple's)."""
    pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(600)
    src, tgt = rng.uniform(0, 1, (600, 3)).astype(np.float32), rng.uniform(0, 1, (300, 3)).astype(np.float32)
    p = icp_np.move(_rigid(2.0, (1, 2, 3), (0.01, -0.02, 0.01))[:3], src)
    a, b = icp_np.nearest_brute(p, tgt, 0.1), icp_np.nearest_ckdtree(p, tgt, 0.1)
    assert 0 < (a[0] >= 0).sum() < 600
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.isfinite(a[2]) and a[2] > 0.0 and b[2] == a[2]
    assert np.isfinite(b[3]) and b[3] >= a[3] > 0.0
    # the nearest target's margin itself, from the brute-force matrix of every couple
    D = icp_np._d2(p, tgt.astype(np.float64))
    assert b[3] == np.min(np.abs(D.min(axis=1) - 0.1 * 0.1))
    # equal d2: the lower index, whichever the tree proposes first; a single target: no second one, margin_nn stays inf
    two = np.array([[0.0, 0.125, 0.0], [0.0, -0.125, 0.0]], np.float32)
    for t in (two, two[::-1].copy()):
        idx, d2, gap, _ = icp_np.nearest_ckdtree(np.zeros((1, 3)), t, 0.2)
        assert idx[0] == 0 and d2[0] == 0.015625 and gap == 0.0
    idx, d2, gap, gap_r = icp_np.nearest_ckdtree(np.zeros((1, 3)), two[:1], 0.2)
    assert idx[0] == 0 and gap == np.inf and gap_r == abs(0.015625 - 0.2 * 0.2)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    return np.load(os.path.join(GOLDEN, "icp_sweep.npz"))


@pytest.fixture(scope="module")
def sweep_pairs():
    return icp_cases.sweep_pairs()


def test_sweep_fixture_margins_meet_the_cap(sweep):
    assert sweep["margins"].shape == (2, 3) and np.all(sweep["margins"] >= MARGIN)
    assert np.all(sweep["fit_difference"] >= 0.0) and np.all(sweep["fit_difference"] < 1e-12)
    assert sweep["nearest"].shape == (2, 65984) and sweep["nearest"].dtype == np.int32 and sweep["T"].shape == (2, 4, 4)
    assert np.all(sweep["converged"] == 1) and np.all(sweep["iterations"] >= 2) and np.all(sweep["iterations"] <= 200)
    assert np.array_equal(sweep["count"], (sweep["nearest"] >= 0).sum(axis=1)) and np.all(sweep["count"] > 50000)
    assert os.path.getsize(os.path.join(GOLDEN, "icp_sweep.npz")) < 1000000
    for k, v in icp_cases.SWEEP.items():
        assert float(sweep["recipe_" + k]) == float(v), k


def test_sweep_fixture_inputs_are_the_regenerated_ones(sweep, sweep_pairs):
    assert [len(p[0]) for p in sweep_pairs] == list(sweep["src_rows"]) == [65984, 65984]                # 258 chunks each
    assert [len(p[1]) for p in sweep_pairs] == list(sweep["tgt_rows"]) == [20000, 20000]
    assert [icp_cases.pair_sha256(p) for p in sweep_pairs] == [str(x) for x in sweep["sha256"]]
    # the regime the fixture is there for: cells of eight radii, in the batch of two and for a pair alone
    from d3feat_amd import icp
    gr = icp.grid_radius(0.2)
    assert np.array_equal(icp_cases.cell_edge([p[1] for p in sweep_pairs], gr), [8 * gr * (1 + 2.0 ** -20)] * 2)
    assert np.array_equal(icp_cases.cell_edge([sweep_pairs[1][1]], gr), [8 * gr * (1 + 2.0 ** -20)])


def test_sweep_fixture_is_the_restatement(sweep, sweep_pairs):
    """Pair 0 recomputed (eight rounds of 66 k rows through the k-d tree: about a second)."""
    pytest.importorskip("scipy.spatial")
    src, tgt, init = sweep_pairs[0]
    r = icp_np.icp(src, tgt, init, nearest=icp_np.nearest_ckdtree, **{k[3:]: float(sweep[k]) for k in sweep.files if k.startswith("kw_")})
    assert np.array_equal(r.T, sweep["T"][0]) and np.array_equal(r.nearest, sweep["nearest"][0])
    assert (r.count, r.iterations, r.converged) == (int(sweep["count"][0]), int(sweep["iterations"][0]), int(sweep["converged"][0]))
    assert (r.sumd2, r.fitness, r.rmse) == (float(sweep["sumd2"][0]), float(sweep["fitness"][0]), float(sweep["rmse"][0]))
    assert np.array_equal([r.margin_nn, r.margin_r, r.margin_stop], sweep["margins"][0])


def test_cell_edge_is_the_budget_arithmetic():
    """icp_cases.cell_edge on cases worked out by hand: 65 536 cells at least, an equal share per element, the edge doubled until the
    cloud fits."""
    cube = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    h = 0.125 * (1 + 2.0 ** -20)
    assert np.array_equal(icp_cases.cell_edge([cube], 0.125), [h])                                      # 8^3 cells
    assert np.array_equal(icp_cases.cell_edge([cube], 0.125 / 4), [h / 4])                              # 32^3 <= 65 536
    assert np.array_equal(icp_cases.cell_edge([cube], 0.125 / 8), [h / 4])                              # 64^3 does not fit: doubled once
    assert np.array_equal(icp_cases.cell_edge([cube, cube[:1], cube[:0]], 0.125 / 4), [h / 2, h / 4, 1.0])   # a third of the budget each
    bad = np.array([[0, 0, 0], [np.inf, 0, 0]], np.float32)
    assert np.array_equal(icp_cases.cell_edge([cube, bad], 0.125), [h, np.inf])                         # never fits: the one-cell grid


def test_fixture_margins_meet_the_cap(gold):
    for tag in ("", "it3_"):
        assert gold[tag + "margins"].shape == (3,) and np.all(gold[tag + "margins"] >= MARGIN), tag
        assert 0.0 <= float(gold[tag + "fit_difference"]) < 1e-12
    assert gold["src"].shape == (2000, 3) and gold["src"].dtype == np.float32 and gold["tgt"].shape == (1400, 3)
    assert int(gold["converged"]) == 1 and 1 <= int(gold["iterations"]) <= 200
    assert int(gold["it3_converged"]) == 0 and int(gold["it3_iterations"]) == 3


def test_fixture_is_the_restatement(gold):
    """max_iteration = 3 on the golden pair, restated again here (the whole loop is tools/make_golden_icp.py's)."""
    r = icp_np.icp(gold["src"], gold["tgt"], None, max_correspondence_distance=0.2, max_iteration=3)
    assert np.array_equal(r.T, gold["it3_T"]) and r.count == int(gold["it3_count"]) and np.array_equal(r.nearest, gold["it3_nearest"])
    assert r.sumd2 == float(gold["it3_sumd2"]) and r.rmse == float(gold["it3_rmse"])


# ---- argument checks: no launch ------------------------------------------------------------------------------------------------------------
def test_icp_pairs_refuses_bad_arguments_without_a_gpu():
    from d3feat_amd import _lib
    lib = _lib.load()
    assert "d3f_icp_pairs" in _lib.SIGNATURES and "d3f_icp_pairs_workspace_bytes" in _lib.SIGNATURES
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    keep = {}
    crit = lambda r=0.2, f=1e-6, m=1e-6: ctypes.addressof(keep.setdefault((r, f, m), (ctypes.c_double * 3)(r, f, m)))
    gb, wb = lib.d3f_neighbor_grid_bytes(100, 2), lib.d3f_icp_pairs_workspace_bytes(100, 2)
    assert wb >= 3 * 16 * 8 and lib.d3f_icp_pairs_workspace_bytes(-1, 2) == 0 and lib.d3f_icp_pairs_workspace_bytes(10, 0) == 0
    assert lib.d3f_icp_pairs_workspace_bytes(10, 256) == 0

    def call(grid=p, gbytes=gb, Nt=100, src=p, Ns=100, lens=p, B=2, init=p, c=None, it=200, every=0, T=p, count=p, sumd2=p, fitness=p,
             rmse=p, iterations=p, converged=p, nearest=None, ws=p, wsb=wb):
        return lib.d3f_icp_pairs(grid, gbytes, Nt, src, Ns, lens, B, init, crit() if c is None else c, it, every, T, count, sumd2, fitness,
                                 rmse, iterations, converged, nearest, ws, wsb, None)
    for r in (0.0, -0.2, float("nan"), float("inf")):
        assert call(c=crit(r=r)) == -3, r
    assert call(c=crit(f=float("nan"))) == -3 and call(c=crit(m=float("nan"))) == -3
    assert call(Nt=-1) == -3 and call(Ns=-1) == -3 and call(B=0) == -3 and call(B=256) == -3
    assert call(it=-1) == -3 and call(every=-1) == -3
    for name in ("grid", "src", "lens", "init", "T", "count", "sumd2", "fitness", "rmse", "iterations", "converged"):
        assert call(**{name: None}) == -3, name
    assert lib.d3f_icp_pairs(p, gb, 100, p, 100, p, 2, p, None, 200, 0, p, p, p, p, p, p, p, None, p, wb, None) == -3      # criteria
    assert call(wsb=wb - 1) == -2 and call(ws=None) == -2 and call(gbytes=gb - 1024 - 1) == -2


# ---- the cache files -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tree(tmp_path):
    """Two sweeps of sequence 8 and their poses: frame 1 is frame 0 seen from 0.05 m further on (camera z = velodyne x)."""
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-2, 2, (400, 2)), rng.normal(0, 0.01, (400, 1))], 1)
    pts = np.concatenate([pts, pts[:, [2, 0, 1]] + [2.0, 0, 1.0]]).astype(np.float32)
    velo = tmp_path / "sequences" / "08" / "velodyne"
    velo.mkdir(parents=True)
    (tmp_path / "poses").mkdir()
    moved = pts.copy()
    moved[:, 0] -= np.float32(0.08)                     # what the sensor sees after moving 0.08 m along x, the odometry says 0.05
    for t, a in ((0, pts), (1, moved)):
        np.concatenate([a, np.zeros((len(a), 1), np.float32)], 1).astype(np.float32).tofile(str(velo / ("%06d.bin" % t)))
    poses = np.tile(np.eye(4)[:3].reshape(1, 12), (2, 1))
    poses[1, 11] = 0.05                                  # camera z
    np.savetxt(str(tmp_path / "poses" / "08.txt"), poses)
    return str(tmp_path)


def test_cache_files_hold_what_the_reference_writes(tree, monkeypatch):
    from d3feat_amd import icp
    calls = []

    def restated(src, src_lens, tgt, tgt_lens, init=None, check_every=8, **kw):
        calls.append((list(src_lens), kw))
        return icp_np.icp_pairs(src, src_lens, tgt, tgt_lens, init=init, **kw)
    monkeypatch.setattr(icp, "icp_pairs", restated)
    icp_dir = os.path.join(tree, "icp")
    with pytest.raises(FileNotFoundError, match="8_0_1.npy"):               # the default still raises, and writes nothing
        kitti.pair_transform(tree, 8, 0, 1)
    assert not os.path.exists(icp_dir) and not calls
    assert kitti.refine_pairs(tree, [(8, 0, 1), (8, 0, 1)]) == 1
    assert os.listdir(icp_dir) == ["8_0_1.npy"] and calls[0][1] == icp.ICP_KITTI and calls[0][0] == [800]
    M2 = np.load(os.path.join(icp_dir, "8_0_1.npy"))
    # the reference's own steps (KITTI.py:288-303) in numpy: ICP from the identity on the sweep pre-moved by M, the file = M @ T_icp
    M = kitti.odometry_transform(tree, 8, 0, 1)
    xyz0, xyz1 = kitti.read_pair(tree, 8, 0, 1)
    want = icp_np.icp(xyz0, xyz1, M, **icp.ICP_KITTI)
    assert M2.shape == (4, 4) and M2.dtype == np.float64
    assert np.array_equal(M2, M @ (want.T @ np.linalg.inv(M)))
    assert abs(M2[0, 3] + 0.08) < 1e-3 and abs(M[0, 3] + 0.05) < 1e-4       # refined: the 0.08 m the points moved, not the odometry's 0.05
    # an existing cache file wins: nothing is computed, nothing is rewritten
    marker = np.arange(16.0).reshape(4, 4)
    np.save(os.path.join(icp_dir, "8_0_1.npy"), marker)
    assert kitti.refine_pairs(tree, [(8, 0, 1)]) == 0 and len(calls) == 1
    assert np.array_equal(kitti.pair_transform(tree, 8, 0, 1, refine=True), marker) and len(calls) == 1
    # pair_transform(refine=True) computes and caches a missing file, under icp_dir when one is given
    other = os.path.join(tree, "elsewhere")
    got = kitti.pair_transform(tree, 8, 0, 1, icp_dir=other, refine=True)
    assert len(calls) == 2 and np.array_equal(got, M2) and os.listdir(other) == ["8_0_1.npy"]
    assert np.array_equal(kitti.pair_transform(tree, 8, 0, 1, icp_dir=other), M2)


# ---- compat --------------------------------------------------------------------------------------------------------------------------------
def test_compat_registration_icp(monkeypatch):
    with icp_np.compat_open3d(ROOT) as open3d:
        _compat_registration_icp(open3d, monkeypatch)


def _compat_registration_icp(open3d, monkeypatch):
    from d3feat_amd import icp
    monkeypatch.setattr(icp, "icp_pairs", lambda *a, check_every=8, **kw: icp_np.icp_pairs(*a, **kw))
    rng = np.random.default_rng(4)
    a, b = open3d.geometry.PointCloud(), open3d.geometry.PointCloud()
    a.points = open3d.utility.Vector3dVector(rng.uniform(0, 1, (200, 3)))
    b.points = open3d.utility.Vector3dVector(np.asarray(a.points) + [0.01, 0.0, -0.01])
    reg = open3d.registration
    res = reg.registration_icp(a, b, 0.2, np.eye(4), reg.TransformationEstimationPointToPoint(), reg.ICPConvergenceCriteria(max_iteration=30))
    assert isinstance(res, open3d.RegistrationResult) and res.transformation.shape == (4, 4) and res.fitness == 1.0
    assert np.max(np.abs(res.transformation[:3, 3] - [0.01, 0.0, -0.01])) < 1e-6 and np.asarray(res.correspondence_set).shape == (200, 2)
    with pytest.raises(NotImplementedError, match="with_scaling"):
        reg.registration_icp(a, b, 0.2, np.eye(4), reg.TransformationEstimationPointToPoint(True))
    with pytest.raises(NotImplementedError, match="PointToPoint"):
        reg.registration_icp(a, b, 0.2, np.eye(4), object())


# ---- the tool and the host-side length check -----------------------------------------------------------------------------------------------
def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_kitti_icp_tool_fills_the_cache_and_goes_on_to_the_test(tree, monkeypatch, capsys):
    """tools/kitti_icp.py: every test pair without a cache file gets one (the restatement stands in for the device call); with --weights
    tools/kitti_test.py's main runs afterwards in the same process, with the same tree and every option the tool does not know."""
    import sys
    import types
    from d3feat_amd import icp
    tool = _load_tool("kitti_icp")
    monkeypatch.setattr(icp, "icp_pairs", lambda *a, check_every=8, **kw: icp_np.icp_pairs(*a, **kw))
    monkeypatch.setattr(kitti, "test_pairs", lambda root, seqs: [(8, 0, 1)] if list(seqs) == [8] else [])
    assert tool.main(["--root", tree, "--sequences", "8"]) == 1
    assert os.listdir(os.path.join(tree, "icp")) == ["8_0_1.npy"] and "1 test pairs, 1 cache files written" in capsys.readouterr().out
    M2 = np.load(os.path.join(tree, "icp", "8_0_1.npy"))
    assert abs(M2[0, 3] + 0.08) < 1e-3
    seen = []
    monkeypatch.setattr(tool, "kitti_test_module", lambda: types.SimpleNamespace(main=lambda: seen.append(list(sys.argv[1:]))))
    before = list(sys.argv)
    other = os.path.join(tree, "cache2")
    assert tool.main(["--root", tree, "--sequences", "8", "--icp-dir", other, "--weights", "W", "--out", "X", "--slots", "2"]) == 1
    assert seen == [["--root", tree, "--weights", "W", "--sequences", "8", "--icp-dir", other, "--out", "X", "--slots", "2"]]
    assert sys.argv == before and np.array_equal(np.load(os.path.join(other, "8_0_1.npy")), M2)
    assert tool.main(["--root", tree, "--sequences", "8", "--weights", "W"]) == 0 and len(seen) == 2      # the cache wins, the test still runs
    with pytest.raises(SystemExit):                                                                        # an option of the test without --weights
        tool.main(["--root", tree, "--sequences", "8", "--out", "X"])
    assert callable(_load_tool("kitti_icp").kitti_test_module().main)                                      # the real module loads and has a main


def test_icp_pairs_checks_host_lengths_before_the_device():
    from d3feat_amd import icp
    pts = np.zeros((10, 3), np.float32)
    for sl, tl in (([4, 5], [5, 5]), ([5, 5], [5, 6]), ([11, -1], [5, 5])):
        with pytest.raises(ValueError, match="do not add up"):
            icp.icp_pairs(pts, sl, pts, tl)
