"""The 3DMatch registration recall on the GPU (d3f_registration_recall, registration.registration_recall / register_scenes):

  1. the fixture of the reference's own gt.log / gt.info (tests/golden/recall.npz): `error` bit for bit, flags and figures equal to the
     numpy restatement of the header (tests/recall_np.py, (a)), for float32 estimates inverted on the device and for float64 matrices
     as a .log holds them;
  2. the comparison is not strict: an error of exactly err2 is good, err2 one float64 lower makes it bad;
  3. s <= 0 (a half turn), a NaN in T, a NaN in info and info[0][0] = 0 are bad rows, and the rows around them keep their bits;
  4. shapes: P = 0, S = 0, an empty scene between two others, scenes of 1 / 257 / 513 pairs, n = 1 flat and n = 3, result_flag None
     against explicit, false positives, duplicate result rows, S = SCENES_MAX;
  5. out= reuse, two runs and a replay from a captured HIP graph, bit-equal to the eager call;
  6. register_scenes on two small scenes whose descriptors carry a NaN and an inf, for one count and for two: T, mutual_count and
     gt_inliers bit-equal to register_pairs / register_pairs_counts alone on sanitised blocks, the matching figures equal to
     matching_summary's, the recall figures equal to the restatement on the read-back T."""
import os

import numpy as np
import pytest
import torch

import recall_np as rnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SCENE = "sun3d-hotel_umd-maryland_hotel3"


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits_equal(got, want):
    """float64 arrays: the same bits where `want` is a number, NaN where it is NaN (the payload of a NaN is not part of the definition)"""
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _run(device, T, gt, info, gt_flag, ids, scene_start, result_flag=None, **kw):
    from d3feat_amd import registration as reg
    return reg.registration_recall(_dev(T, device), _dev(gt, device), _dev(info, device), _dev(gt_flag, device), _dev(ids, device), scene_start,
                                   result_flag=None if result_flag is None else _dev(result_flag, device), **kw)


def _check(res, want):
    h = res.host()
    assert _bits_equal(h["error"], want["error"]), "error"
    assert np.array_equal(h["flags"], want["flags"]) and np.array_equal(h["figures"], want["figures"])
    assert res.scenes() == rnp.summary(want["figures"])


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    from d3feat_amd.datasets import threedmatch
    g = np.load(os.path.join(GOLDEN, "recall.npz"))
    bm = threedmatch.benchmark(None, [37], scenes=[SCENE], gt_logs=[os.path.join(GOLDEN, "gt_log_hotel3.log")],
                               gt_infos=[os.path.join(GOLDEN, "gt_info_hotel3.info")])
    return g, bm


@pytest.mark.parametrize("logged", [False, True])
def test_fixture_bit_for_bit(device, fixture, logged):
    g, bm = fixture
    T = g["logged"] if logged else g["T"]
    args = (bm.gt, bm.info, bm.gt_flag, bm.ids, bm.scene_start)
    res = _run(device, T, *args, result_flag=g["result_flag"], logged=logged)
    want = rnp.device(T, *args, result_flag=g["result_flag"], logged=logged)
    assert np.array_equal(want["error"].view(np.uint64), g["p_a_logged" if logged else "p_a"].view(np.uint64))
    _check(res, want)
    assert res.error.shape == (666, 2) and res.error.dtype == torch.float64 and res.flags.dtype == torch.int32 and res.figures.shape == (1, 2, 5)
    # the .m files line by line, within the tolerance the fixture measured
    pb = g["p_b_logged" if logged else "p_b"]
    assert np.all(np.abs(res.host()["error"] - pb) <= float(g["tol"]) * np.abs(pb))
    assert np.array_equal(res.host()["figures"], g["figures"])
    bad = res.failed(0)
    assert len(bad) == int(g["figures"][0, 0, 1]) and all(p > 0.04 for _, _, _, p in bad) and all(b - a > 1 for _, a, b, _ in bad)
    # a single column, flat
    one = _run(device, np.ascontiguousarray(T[:, 1]), *args, result_flag=g["result_flag"], logged=logged)
    assert one.error.shape == (666,) and torch.equal(one.error, res.error[:, 1]) and torch.equal(one.flags, res.flags[:, 1])
    assert torch.equal(one.figures[:, 0], res.figures[:, 1])


# ---- 2. the boundary -------------------------------------------------------------------------------------------------------------------------
def test_error_of_exactly_err2_is_good(device):
    T = np.zeros((3, 3, 4), np.float32)
    T[:, :, :3], T[:, 0, 3] = np.eye(3), -0.25                                                   # the inverse is a translation by exactly 0.25
    gt, info = np.tile(np.eye(4), (3, 1, 1)), np.tile(7.0 * np.eye(6), (3, 1, 1))
    flag, ids = np.ones(3, np.int32), np.array([[0, 2], [1, 3], [4, 9]], np.int32)
    below = float(np.nextafter(0.0625, 0.0))
    for err2, good in ((0.0625, 3), (below, 0), (float(np.nextafter(0.0625, 1.0)), 3)):
        res = _run(device, T, gt, info, flag, ids, [0, 3], err2=err2)
        h = res.host()
        assert h["error"][:, 0].tolist() == [0.0625] * 3 and h["figures"][0, 0].tolist() == [good, 3 - good, 0, 3, 3], err2
        assert h["flags"][:, 0].tolist() == [11 if good else 10] * 3
        _check(res, rnp.device(T, gt, info, flag, ids, [0, 3], err2=err2))
    # the same through the .log form
    L = np.tile(np.eye(4), (3, 1, 1))
    L[:, 0, 3] = 0.25
    assert _run(device, L, gt, info, flag, ids, [0, 3], err2=0.0625, logged=True).host()["figures"][0, 0, 0] == 3
    assert _run(device, L, gt, info, flag, ids, [0, 3], err2=below, logged=True).host()["figures"][0, 0, 0] == 0


# ---- 3. NaN ----------------------------------------------------------------------------------------------------------------------------------
def _case(seed, P, n, logged=False):
    """random rows: gt a rigid motion, info symmetric positive definite, estimates = gt moved by errors around the threshold"""
    rng = np.random.default_rng(seed)

    def rigid(k, scale=1.0):
        q = rng.normal(size=(k, 4))
        q[:, 1:] *= scale
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        M = np.tile(np.eye(4), (k, 1, 1))
        M[:, :3, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                                 2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(k, 3, 3)
        M[:, :3, 3] = rng.normal(size=(k, 3)) * scale
        return M
    gt = rigid(P)
    A = rng.normal(size=(P, 6, 6))
    info = A @ A.transpose(0, 2, 1) * 100 + 5000 * np.eye(6)
    L = gt[:, None] @ rigid(P * n, 0.08).reshape(P, n, 4, 4)
    T = np.linalg.inv(L)[:, :, :3].astype(np.float32) if P * n else np.zeros((P, n, 3, 4), np.float32)
    flag = (rng.random(P) < 0.7).astype(np.int32)
    res = (rng.random(P) < 0.8).astype(np.int32)
    a = rng.integers(0, 30, P)
    ids = np.stack([a, a + rng.choice([1, 2, 3, 17], P)], 1).astype(np.int32)
    return (np.ascontiguousarray(L) if logged else T), gt, info, flag, ids, res


def test_nan_rows_are_bad_and_disturb_nothing(device):
    P = 300
    L, gt, info, flag, ids, _ = _case(5, P, 2, logged=True)
    flag[:], ids[:] = 1, [0, 2]
    gt[7] = gt[8] = np.eye(4)                                                                    # their inverse is exact: E is the estimate itself
    clean = rnp.device(L, gt, info, flag, ids, [0, 100, P], logged=True)
    assert np.isfinite(clean["error"]).all() and 0 < clean["figures"][0, 0, 0] < 100
    half, under = np.diag([-1.0, -1.0, 1.0, 1.0]), np.diag([-1.0, -1.0, 0.9999999999999999, 1.0])    # s = 0 and s = -1.1e-16
    rows = [7, 8, 120, 121, 256, 299]
    L[7, 0], L[8, 1] = gt[7] @ half, gt[8] @ under
    L[120, 1, 1, 2] = np.nan
    info[121, 4, 5] = np.nan
    info[256, 0, 0] = 0.0
    L[299, 0, 0, 3] = np.nan
    want = rnp.device(L, gt, info, flag, ids, [0, 100, P], logged=True)
    assert np.isnan(want["error"][7, 0]) and np.isnan(want["error"][8, 1]) and np.isnan(want["error"][120, 1]) and np.isnan(want["error"][121]).all()
    assert np.isinf(want["error"][256]).all() and np.isnan(want["error"][299, 0])
    assert np.isnan(want["error"]).sum() == 6 and (want["flags"][~np.isfinite(want["error"])] == 10).all()
    keep = np.ones((P, 2), bool)
    keep[rows] = False
    assert np.array_equal(want["error"][keep], clean["error"][keep])
    res = _run(device, L, gt, info, flag, ids, [0, 100, P], logged=True)
    _check(res, want)
    assert {(s, c) for c in (0, 1) for s, _, _, p in res.failed(c) if not np.isfinite(p)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # a NaN in a float32 estimate that is inverted on the device
    T, gt, info, flag, ids, _ = _case(6, 40, 1)
    flag[:], ids[:] = 1, [3, 9]
    T[11, 0, 2, 1], T[12, 0, 0, 3] = np.nan, np.inf
    want = rnp.device(T, gt, info, flag, ids, [0, 40])
    assert np.isnan(want["error"][[11, 12], 0]).all() and np.isfinite(np.delete(want["error"], [11, 12])).all()
    _check(_run(device, T, gt, info, flag, ids, [0, 40]), want)


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------------------------
STARTS = [0, 3, 3, 4, 261, 774]                                                                   # 3, none, 1, 257 and 513 pairs


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("logged", [False, True])
def test_scene_shapes(device, n, logged):
    P = STARTS[-1]
    T, gt, info, flag, ids, res_flag = _case(100 * n + logged, P, n, logged)
    ids[600], T[600], gt[600], info[600] = ids[599], T[599], gt[599], info[599]                   # the same pair twice: two result rows
    flag[600] = flag[599] = res_flag[600] = res_flag[599] = 1
    ids[599, 1] = ids[600, 1] = ids[599, 0] + 2
    for rf in (None, res_flag, flag.copy()):
        want = rnp.device(T, gt, info, flag, ids, STARTS, result_flag=rf, logged=logged)
        res = _run(device, T, gt, info, flag, ids, STARTS, result_flag=rf, logged=logged)
        _check(res, want)
        assert want["figures"][1].sum() == 0 and want["figures"][4, :, 0].min() > 20 and want["figures"][4, :, 1].min() > 20
        assert (want["figures"][:, :, 2] > 0).any() == (rf is res_flag)                             # false positives need an explicit result_flag
        assert want["flags"][600].tolist() == want["flags"][599].tolist() and (want["flags"][600] & 2).all()
    assert torch.equal(_run(device, T, gt, info, flag, ids, STARTS, logged=logged).flags,
                       _run(device, T, gt, info, flag, ids, STARTS, result_flag=flag.copy(), logged=logged).flags)
    if n == 1:                                                                                    # flat
        Tf = np.ascontiguousarray(T[:, 0])
        res = _run(device, Tf, gt, info, flag, ids, STARTS, result_flag=res_flag, logged=logged)
        assert res.error.shape == (P,) and res.flags.shape == (P,) and res.figures.shape == (5, 1, 5)
        _check(res, rnp.device(T, gt, info, flag, ids, STARTS, result_flag=res_flag, logged=logged))


def test_empty_and_most_scenes(device):
    from d3feat_amd import _lib, registration as reg
    for logged in (False, True):
        T, gt, info, flag, ids, _ = _case(1, 0, 2, logged)
        res = _run(device, T, gt, info, flag, ids, [0], logged=logged)                            # P = 0, S = 0
        assert res.error.shape == (0, 2) and res.figures.shape == (0, 2, 5) and res.scenes() == [] and res.overall()["total_gt"] == 0
        res = _run(device, T, gt, info, flag, ids, [0, 0, 0], logged=logged)                      # P = 0, two empty scenes
        assert res.figures.cpu().numpy().tolist() == [[[0] * 5] * 2] * 2 and res.failed() == []
    T, gt, info, flag, ids, _ = _case(2, 9, 1)
    starts = [0] * 200 + [4] * 56 + [9]
    assert len(starts) == _lib.SCENES_MAX + 1
    res = _run(device, T, gt, info, flag, ids, starts)
    _check(res, rnp.device(T, gt, info, flag, ids, starts))
    assert res.figures.shape == (256, 1, 5) and res.figures[:199].sum().item() == 0 and res.figures[200:255].sum().item() == 0
    d = lambda a: _dev(a, device)
    for bad in ([0] * 257 + [9], [0, 5, 4, 9], [0, 8], [1, 9]):
        with pytest.raises(ValueError):
            _run(device, T, gt, info, flag, ids, bad)
    with pytest.raises(ValueError):
        _run(device, T, gt, info, flag, ids, [0, 9], err2=0.0)
    with pytest.raises(ValueError):
        _run(device, T, gt, info, flag[:8], ids, [0, 9])
    with pytest.raises(ValueError):
        _run(device, T, gt[:, :3], info, flag, ids, [0, 9])
    with pytest.raises(TypeError):
        _run(device, T.astype(np.float64), gt, info, flag, ids, [0, 9])
    with pytest.raises(ValueError):
        reg.registration_recall(d(T), d(gt), d(info), d(flag), d(ids), [0, 9], out=_run(device, T, gt, info, flag, ids, [0, 4, 9]))


# ---- 5. reuse --------------------------------------------------------------------------------------------------------------------------------
def _same(x, want):
    return (_bits_equal(x.error.cpu().numpy(), want["error"]) and np.array_equal(x.flags.cpu().numpy().reshape(want["flags"].shape), want["flags"])
            and np.array_equal(x.figures.cpu().numpy(), want["figures"]))


@pytest.mark.parametrize("logged", [False, True])
def test_out_reuse_two_runs_and_graph_replay(device, logged):
    from d3feat_amd import registration as reg
    starts = [0, 257, 300]
    A, B = _case(41 + logged, 300, 2, logged), _case(43 + logged, 300, 2, logged)
    want_a = rnp.device(*A[:5], starts, result_flag=A[5], logged=logged)
    want_b = rnp.device(*B[:5], starts, result_flag=B[5], logged=logged)
    assert not np.array_equal(want_a["flags"], want_b["flags"])
    t = [_dev(a, device) for a in A]
    call = lambda out=None: reg.registration_recall(t[0], t[1], t[2], t[3], t[4], starts, result_flag=t[5], logged=logged, out=out)
    first, second = call(), call()
    assert _same(first, want_a) and torch.equal(first.error.view(torch.int64), second.error.view(torch.int64))
    assert torch.equal(first.flags, second.flags) and torch.equal(first.figures, second.figures)
    res = first
    assert res.host() is res.host()
    for x, b in zip(t, B):
        x.copy_(_dev(b, device))
    assert call(out=res) is res and _same(res, want_b) and res.scenes() == rnp.summary(want_b["figures"])     # the cache was dropped
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        call(out=res)                                                                             # eager warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        call(out=res)
    for x, a in zip(t, A):
        x.copy_(_dev(a, device))
    res.error.fill_(-7.0)
    res.flags.fill_(-7)
    res.figures.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same(res, want_a)
    for x, b in zip(t, B):
        x.copy_(_dev(b, device))
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same(res, want_b)


# ---- 6. register_scenes ----------------------------------------------------------------------------------------------------------------------
def _two_scenes(seed, device):
    """two scenes of 5 and 6 blocks of 64 keypoints (synthetic.scene), every other pair listed, a NaN and an inf in the descriptors"""
    from d3feat_amd.datasets import threedmatch
    from d3feat_amd.utils.synthetic import scene
    rng = np.random.default_rng(seed)
    blocks, logs, infos = [], [], []
    for k, n in enumerate((5, 6)):
        b, poses = scene(seed + k, n_frag=n, K=64)
        blocks += b
        keys = [(i, j) for i in range(n) for j in range(i + 1, n) if (i + j + k) % 2 or j - i == 2]
        logs.append({"%d_%d" % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i, j in keys})
        A = rng.normal(size=(len(keys), 6, 6))
        infos.append({"%d_%d" % ij: a @ a.T * 50 + 5000 * np.eye(6) for ij, a in zip(keys, A)})
    kp = np.stack(blocks)
    kp[1, 5, 7], kp[4, 60, 3:35], kp[6, 40, 20], kp[9, 63, 34] = np.nan, np.nan, np.inf, -np.inf
    bm = threedmatch.benchmark(None, [5, 6], gt_logs=logs, gt_infos=infos)
    assert bm.scene_start.tolist() == [0, 10, 25] and 0 < bm.gt_flag.sum() < 25
    return kp, bm


@pytest.mark.parametrize("num_keypts", [64, (32, 64)])
def test_register_scenes_equals_the_stand_alone_calls(device, num_keypts):
    from d3feat_amd import registration as reg
    kp, bm = _two_scenes(17, device)
    count = torch.full((11,), 64, dtype=torch.int32, device=device)
    d = lambda a: _dev(a, device)
    pairs, gt, info, flag, ids = d(bm.pairs), d(bm.gt), d(bm.info), d(bm.gt_flag), d(bm.ids)
    kp_dev = d(kp)
    out = reg.register_scenes(kp_dev, count, pairs, gt, info, flag, ids, bm.scene_start, num_keypts=num_keypts, seed=3)
    assert not torch.isnan(kp_dev[:, :, 3:35]).any() and not torch.isinf(kp_dev[:, :, 3:35]).any()       # sanitised in place
    clean = reg.sanitize_descriptors(d(kp))
    gt32 = d(bm.gt[:, :3].astype(np.float32))
    if isinstance(num_keypts, tuple):
        alone = reg.register_pairs_counts(clean, count, pairs, num_keypts=num_keypts, seed=3, gt=gt32, **reg.EVALUATE_3DMATCH)
        assert isinstance(out.registration, reg.PairRegistrationCounts) and out.T.shape == (25, 2, 3, 4)
    else:
        alone = reg.register_pairs(clean, count, pairs, num_keypts=num_keypts, seed=3, gt=gt32, **reg.EVALUATE_3DMATCH)
        assert isinstance(out.registration, reg.PairRegistration) and out.T.shape == (25, 3, 4) and out.recall.error.shape == (25,)
    for name in ("T", "mutual_count", "gt_inliers", "inliers", "best_iteration"):
        assert torch.equal(getattr(out.registration, name), getattr(alone, name)), name
    summary = reg.matching_summary(alone.mutual_count, alone.gt_inliers, flag, bm.scene_start)
    assert torch.equal(out.matching.figures, summary.figures) and torch.equal(out.matching.ratio_e8, summary.ratio_e8)
    assert out.matching.scenes() == summary.scenes()
    T = out.T.cpu().numpy()
    want = rnp.device(T, bm.gt, bm.info, bm.gt_flag, bm.ids, bm.scene_start)
    _check(out.recall, want)
    b = rnp.matlab(T, bm.gt, bm.info, bm.gt_flag, bm.ids, bm.scene_start)
    assert np.array_equal(b["figures"], want["figures"])
    fig = want["figures"]
    assert fig[:, -1, 3].tolist() == [int(((bm.gt_flag != 0) & (bm.ids[:, 1] - bm.ids[:, 0] > 1))[a:z].sum()) for a, z in ((0, 10), (10, 25))]
    assert fig[:, -1, 3].min() > 0 and (fig[:, :, 0] + fig[:, :, 1] == fig[:, :, 4]).all()       # every result is good or bad: no false positive here
    # a second call into the same result
    again = reg.register_scenes(d(kp), count, pairs, gt, info, flag, ids, bm.scene_start, num_keypts=num_keypts, seed=3, out=out)
    assert again is out and torch.equal(out.T, alone.T)
    _check(out.recall, want)
    with pytest.raises(ValueError):
        reg.register_scenes(d(kp), count, pairs, gt, info, flag, ids, bm.scene_start, num_keypts=(64,) if num_keypts == 64 else 64, out=out)
