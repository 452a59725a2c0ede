"""The 3DMatch registration recall (d3f_registration_recall, registration.registration_recall / register_scenes, datasets.threedmatch,
results.read_gt_info / read_result_log / registration_recall_lines), the part that needs no GPU: the two restatements of
tests/recall_np.py against each other on the fixture of the reference's own gt.log / gt.info (tests/golden/recall.npz,
tools/make_golden_recall.py), the readers, the printed lines, the closing arithmetic, the pair list and the argument checks of the
entry point."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import recall_np as rnp
from conftest import GOLDEN, ROOT

SCENE = "sun3d-hotel_umd-maryland_hotel3"
LOG, INFO = os.path.join(GOLDEN, "gt_log_hotel3.log"), os.path.join(GOLDEN, "gt_info_hotel3.info")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "recall.npz"))


@pytest.fixture(scope="module")
def bench():
    from d3feat_amd.datasets import threedmatch
    return threedmatch.benchmark(None, [37], scenes=[SCENE], gt_logs=[LOG], gt_infos=[INFO])


def _args(bm):
    return bm.gt, bm.info, bm.gt_flag, bm.ids, bm.scene_start


# ---- the fixture and the two restatements ----------------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_describes(golden, bench):
    g, bm = golden, bench
    assert str(g["scene"]) == SCENE and int(g["fragments"]) == 37 and float(g["err2"]) == 0.04 and float(g["margin"]) == 1e-6
    assert g["T"].shape == (666, 2, 3, 4) and g["T"].dtype == np.float32 and g["logged"].shape == (666, 2, 4, 4) and g["logged"].dtype == np.float64
    assert os.path.getsize(INFO) < 40000 and os.path.getsize(os.path.join(GOLDEN, "recall.npz")) < 1 << 20
    apart, listed, res = bm.ids[:, 1] - bm.ids[:, 0] > 1, bm.gt_flag != 0, g["result_flag"] != 0
    assert (listed & ~apart).sum() > 0 and (res & ~listed & apart).sum() == 5 and (listed & apart & ~res).sum() == 3    # consecutive, absent, no result
    assert (res & ~listed & ~apart).sum() == 1
    took = listed & apart & res
    p = g["p_a"][took]
    assert p.min() < 0.01 * 0.04 and p.max() > 10 * 0.04 and ((p > 0.03) & (p < 0.04)).any() and ((p > 0.04) & (p < 0.05)).any()    # the ladder
    for k in ("p_a", "p_b", "p_a_logged", "p_b_logged"):
        assert (np.abs(g[k][took] - 0.04) > 1e-6 * 0.04).all() and (g[k][~took] == 0).all(), k
    assert int(g["dropped"]) <= 0.05 * int(g["draws"])
    assert 0 < float(g["rel_diff"]) < 1e-10 and float(g["tol"]) == 4 * float(g["rel_diff"])
    man = json.load(open(os.path.join(GOLDEN, "recall_manifest.json")))
    assert man["rel_diff_a_b"] == float(g["rel_diff"]) and man["tol"] == float(g["tol"]) and man["dropped"] == int(g["dropped"])
    assert set(man["files"]) == {"recall.npz", "gt_info_hotel3.info"}
    for f, want in man["files"].items():
        assert hashlib.sha256(open(os.path.join(GOLDEN, f), "rb").read()).hexdigest() == want, f


@pytest.mark.parametrize("logged", [False, True])
def test_device_definition_against_the_m_files_on_the_fixture(golden, bench, logged):
    g, bm = golden, bench
    T = g["logged"] if logged else g["T"]
    kw = dict(err2=float(g["err2"]), result_flag=g["result_flag"], logged=logged)
    a, b = rnp.device(T, *_args(bm), **kw), rnp.matlab(T, *_args(bm), **kw)
    sfx = "_logged" if logged else ""
    assert np.array_equal(a["error"].view(np.uint64), g["p_a" + sfx].view(np.uint64))          # element-wise IEEE operations: the same bits anywhere
    assert np.array_equal(a["flags"], g["flags"]) and np.array_equal(a["figures"], g["figures"])
    assert np.array_equal(b["flags"], a["flags"]) and np.array_equal(b["figures"], a["figures"])
    tol = float(g["tol"])
    assert np.all(np.abs(a["error"] - b["error"]) <= tol * np.abs(b["error"]))
    assert np.all(np.abs(b["error"] - g["p_b" + sfx]) <= tol * np.abs(g["p_b" + sfx]))         # a LAPACK of another build


def test_both_input_forms_agree_on_the_fixture(golden):
    g = golden
    assert np.array_equal(g["p_a"] == 0, g["p_a_logged"] == 0)
    nz = g["p_a"] != 0
    assert np.all(np.abs(g["p_a"][nz] - g["p_a_logged"][nz]) <= float(g["tol"]) * g["p_a"][nz])


def test_ground_truth_as_result_gives_recall_one(bench):
    bm = bench
    for fn in (rnp.device, rnp.matlab):
        r = fn(bm.gt.copy(), *_args(bm), logged=True)
        assert r["error"].shape == (666, 1) and np.all(np.abs(r["error"]) < 1e-12)
        good, bad, fpos, gtn, rsn = r["figures"][0, 0].tolist()
        assert (good, bad, fpos) == (gtn, 0, 0) and rsn == gtn and rnp.summary(r["figures"])[0][0]["recall"] == 1.0


def test_consecutive_pairs_count_nowhere(bench):
    bm = bench
    apart, listed = bm.ids[:, 1] - bm.ids[:, 0] > 1, bm.gt_flag != 0
    assert (listed & ~apart).sum() == 28 and (listed & apart).sum() == 26
    r = rnp.device(bm.gt.copy(), *_args(bm), logged=True)
    assert r["figures"][0, 0, 3] == 26 and r["figures"][0, 0, 4] == 26
    assert (r["flags"][~apart] == 0).all() and (r["flags"][listed & apart] == 11).all() and (r["flags"][~listed] == 0).all()
    # every pair with a result: the unlisted non-consecutive ones are false positives, the consecutive ones still nothing
    r = rnp.device(bm.gt.copy(), *_args(bm), logged=True, result_flag=np.ones(666, np.int32))
    assert r["figures"][0, 0].tolist() == [26, 0, int((~listed & apart).sum()), 26, int(apart.sum())]
    assert (r["flags"][~apart] == 0).all() and (r["flags"][~listed & apart] == 6).all()


# ---- the readers ---------------------------------------------------------------------------------------------------------------------------
def test_read_gt_info_against_loadtxt(tmp_path):
    from d3feat_amd.utils import results
    info = results.read_gt_info(INFO)
    lines = open(INFO).read().splitlines()
    heads = [l.split() for l in lines[0::7]]
    mats = np.loadtxt([l for i, l in enumerate(lines) if i % 7]).reshape(-1, 6, 6)
    assert len(info) == len(heads) == len(mats) == 54 and all(h[2] == "37" for h in heads)
    for h, M in zip(heads, mats):
        got = info["%d_%d" % (int(h[0]), int(h[1]))]
        assert got.dtype == np.float64 and got.shape == (6, 6) and np.array_equal(got, M)
    assert set(info) == set(results.read_gt_log(LOG))
    assert all(np.array_equal(M, M.T) and M[0, 0] in (5000.0, 4330.0) for M in info.values())    # the sampled points of the pair
    dup = tmp_path / "dup.info"
    dup.write_text("\n".join(lines[:7] + lines[7:14] + lines[:7]) + "\n")
    with pytest.raises(ValueError):
        results.read_gt_info(str(dup))
    short = tmp_path / "short.info"
    short.write_text("\n".join(lines[:6]) + "\n")
    with pytest.raises(ValueError):
        results.read_gt_info(str(short))


def test_read_result_log_round_trips_write_registration_log(tmp_path, golden):
    from d3feat_amd.utils import results
    g = golden
    pairs = [(0, 2), (1, 5), (0, 2), (3, 30)]                                                     # a pair twice: kept twice
    T = np.tile(np.eye(4), (4, 1, 1))
    T[:, :3] = g["T"][[5, 70, 9, 100], 0].astype(np.float64)
    path = str(tmp_path / "D3Feat_.log")
    results.write_registration_log(path, pairs, T)
    rows = results.read_result_log(path)
    assert [(a, b) for a, b, _ in rows] == pairs
    for (_, _, M), t in zip(rows, T):
        assert M.dtype == np.float64 and np.array_equal(M, np.linalg.inv(t))                     # repr of a double reads back exactly
    assert len(results.read_gt_log(path)) == 3                                                    # the dict reader keeps the last one
    assert [(a, b) for a, b, _ in results.read_result_log(LOG)][:3] == [(0, 1), (0, 12), (2, 3)]


# ---- SceneRecall, the closing arithmetic and the lines ---------------------------------------------------------------------------------------
def _recall(figures, scene_start=None, flags=None, error=None, ids=None):
    """a SceneRecall as registration_recall leaves it, on host tensors"""
    import torch
    from d3feat_amd import registration as reg
    fig = np.asarray(figures, np.int64)
    S, n = fig.shape[:2]
    P = 0 if flags is None else len(flags)
    s = reg.SceneRecall(P, n, False, scene_start if scene_start is not None else [0] * (S + 1), 0.04, False, torch.device("cpu"))
    s.figures.copy_(torch.from_numpy(fig))
    if P:
        s.flags.copy_(torch.from_numpy(np.asarray(flags, np.int32).reshape(P, n)))
        s.error.copy_(torch.from_numpy(np.asarray(error, np.float64).reshape(P, n)))
    s.ids = torch.from_numpy(np.asarray(ids if ids is not None else np.zeros((P, 2)), np.int32).reshape(P, 2))
    return s


def test_scenes_and_overall_arithmetic():
    from d3feat_amd import registration as reg
    assert reg.RECALL_3DMATCH == dict(err2=0.04)
    #          good bad fpos gt rs
    fig = [[[3, 1, 2, 7, 6]], [[0, 0, 0, 0, 0]], [[5, 0, 0, 5, 5]], [[1, 2, 0, 3, 3]]]
    s = _recall(fig)
    sc = [per[0] for per in s.scenes()]
    assert sc[0] == dict(good=3, bad=1, false_pos=2, gt_num=7, rs_num=6, recall=3 / 7, precision=0.5)
    assert sc[1]["recall"] == 0.0 and sc[1]["precision"] == 0.0                                  # MATLAB: 0 / 0
    assert [r[0] for r in rnp.summary(np.asarray(fig))] == sc
    o = s.overall()
    assert o["recall_list"] == [3 / 7, 0.0, 1.0, 1 / 3]
    assert o["mean_recall"] == (3 / 7 + 0.0 + 1.0 + 1 / 3) / 4 and o["mean_precision"] == (0.5 + 0.0 + 1.0 + 1 / 3) / 4
    assert (o["total_tp"], o["total_gt"]) == (9, 15) and o["true_recall"] == 9 / 15           # tp = round(7 * (3 / 7)) + 0 + 5 + round(3 * (1 / 3))
    assert _recall(np.zeros((0, 1, 5))).overall() == dict(recall_list=[], mean_recall=0.0, mean_precision=0.0, total_tp=0, total_gt=0,
                                                         true_recall=0.0)
    assert [reg._round_half_away(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.9999999999999996)] == [0, 0, 1, 2, 3, 3]
    # every good <= gt_num <= 2000: round(gt_num * (good / gt_num)) gives good back
    assert all(reg._round_half_away(n * (k / n)) == k for n in range(1, 400) for k in range(n + 1))


def test_failed_rows():
    flags = [[11, 10], [0, 0], [10, 11], [6, 6], [8, 8], [10, 10]]
    error = [[0.01, 0.3], [0, 0], [np.nan, 0.02], [0, 0], [0, 0], [0.05, 0.041]]
    ids = [[0, 2], [0, 1], [1, 3], [0, 2], [0, 3], [1, 3]]
    s = _recall(np.zeros((2, 2, 5)), [0, 3, 6], flags, error, ids)
    f0, f1 = s.failed(0), s.failed(1)
    assert [r[:3] for r in f0] == [(0, 1, 3), (1, 1, 3)] and np.isnan(f0[0][3]) and f0[1][3] == 0.05
    assert f1 == [(0, 0, 2, 0.3), (1, 1, 3, 0.041)]
    h = s.host()
    assert h is s.host() and h["flags"].shape == (6, 2) and h["ids"].shape == (6, 2)


def test_printed_lines():
    from d3feat_amd.utils import results
    fig = [[[3, 1, 2, 7, 6], [7, 0, 0, 7, 7]], [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], [[5, 0, 0, 5, 5], [1, 4, 0, 5, 5]], [[1, 2, 0, 3, 3], [2, 1, 0, 3, 4]]]
    s = _recall(fig)
    assert results.registration_recall_lines("abcd", s) == [
        "recall : 0.42857 ( 3 / 7 )", "recall : 0 ( 0 / 0 )", "recall : 1 ( 5 / 5 )", "recall : 0.33333 ( 1 / 3 )",
        "Mean registration recall: 0.440476 precision: 0.458333", "True average recall: 0.600000 (9/15)"]
    assert results.registration_recall_lines("abcd", s, 1) == [
        "recall : 1 ( 7 / 7 )", "recall : 0 ( 0 / 0 )", "recall : 0.2 ( 1 / 5 )", "recall : 0.66667 ( 2 / 3 )",
        "Mean registration recall: 0.466667 precision: 0.425000", "True average recall: 0.666667 (10/15)"]
    assert results._num2str(0.5) == "0.5" and results._num2str(0.90476190476) == "0.90476" and results._num2str(37) == "37"
    with pytest.raises(ValueError):
        results.registration_recall_lines("abc", s)


# ---- datasets.threedmatch ------------------------------------------------------------------------------------------------------------------
def _log_text(entries, width, n):
    return "".join("%d\t %d\t %d\n" % (a, b, n) + "".join("\t".join(repr(float(v)) for v in row) + "\t\n" for row in M) for a, b, M in entries)


def test_benchmark_on_a_toy_tree(tmp_path):
    from d3feat_amd.datasets import threedmatch as tdm
    assert len(tdm.SCENES) == 8 and tdm.SCENES[0] == "7-scenes-redkitchen" and tdm.SCENES[5] == SCENE
    assert tdm.SCENES[7] == "sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika"
    rng = np.random.default_rng(3)
    A, B = np.eye(4), np.eye(4)
    A[:3, 3], B[:3, :3], B[:3, 3] = [1.5, -2.0, 0.25], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0.1, 0.2, 0.3]
    IA, IB = (rng.normal(size=(6, 6)) for _ in range(2))
    scenes = ("first", "second")
    entries = ([(0, 1, A, IA), (0, 3, B, IB), (2, 3, A, IB)], [(0, 2, B, IA)])
    for sc, ent in zip(scenes, entries):
        d = tmp_path / (sc + "-evaluation")
        d.mkdir()
        (d / "gt.log").write_text(_log_text([(a, b, M) for a, b, M, _ in ent], 4, 4))
        (d / "gt.info").write_text(_log_text([(a, b, I) for a, b, _, I in ent], 6, 4))
    bm = tdm.benchmark(str(tmp_path), [4, 3], scenes=scenes)
    assert [a.dtype for a in bm] == [np.int32, np.int32, np.float64, np.float64, np.int32, np.int64]
    assert bm.pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [4, 5], [4, 6], [5, 6]]            # global block numbers
    assert bm.ids.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [0, 1], [0, 2], [1, 2]]              # numbers inside the scene
    assert bm.gt_flag.tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0] and bm.scene_start.tolist() == [0, 6, 9]
    assert np.array_equal(bm.gt[0], A) and np.array_equal(bm.gt[2], B) and np.array_equal(bm.gt[5], A) and np.array_equal(bm.gt[7], B)
    assert np.array_equal(bm.info[0], IA) and np.array_equal(bm.info[2], IB) and np.array_equal(bm.info[5], IB) and np.array_equal(bm.info[7], IA)
    assert np.array_equal(bm.gt[1], np.eye(4)) and np.array_equal(bm.info[1], np.eye(6)) and bm.gt.shape == (9, 4, 4) and bm.info.shape == (9, 6, 6)
    # dicts, None, an empty scene, a scene of one fragment
    b2 = tdm.benchmark(None, [0, 1, 3], scenes=None, gt_logs=[None, None, {"0_2": A}], gt_infos=[None, None, {"0_2": IA}])
    assert b2.pairs.tolist() == [[1, 2], [1, 3], [2, 3]] and b2.ids.tolist() == [[0, 1], [0, 2], [1, 2]] and b2.gt_flag.tolist() == [0, 1, 0]
    assert b2.scene_start.tolist() == [0, 0, 0, 3]
    b0 = tdm.benchmark(None, [])
    assert b0.pairs.shape == (0, 2) and b0.gt.shape == (0, 4, 4) and b0.info.shape == (0, 6, 6) and b0.scene_start.tolist() == [0]
    with pytest.raises(ValueError):                                                              # a pair in one file only
        tdm.benchmark(None, [3], gt_logs=[{"0_2": A}], gt_infos=[{}])
    with pytest.raises(ValueError):                                                              # a fragment the scene does not have
        tdm.benchmark(None, [2], gt_logs=[{"0_2": A}], gt_infos=[{"0_2": IA}])
    with pytest.raises(ValueError):
        tdm.benchmark(str(tmp_path), [4], scenes=scenes)
    d = tmp_path / "first-evaluation"
    (d / "gt.log").write_text(_log_text([(0, 1, A), (0, 1, B)], 4, 4))                              # a pair listed twice
    (d / "gt.info").write_text(_log_text([(0, 1, IA)], 6, 4))
    with pytest.raises(ValueError):
        tdm.benchmark(str(tmp_path), [4, 3], scenes=scenes)


def test_python_validation_has_no_cpu_path():
    import torch
    from d3feat_amd import _lib, registration as reg
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.registration_recall(z(2, 3, 4, dt=torch.float32), z(2, 4, 4), z(2, 6, 6), z(2, dt=torch.int32), z(2, 2, dt=torch.int32), [0, 2])
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.register_scenes(z(2, 4, 36, dt=torch.float32), z(2, dt=torch.int32), z(1, 2, dt=torch.int32), z(1, 4, 4), z(1, 6, 6),
                            z(1, dt=torch.int32), z(1, 2, dt=torch.int32), [0, 1])


# ---- the entry point refuses bad arguments before anything touches the device ----------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from d3feat_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    e2 = ctypes.c_double(0.04)

    def recall(P=4, n=1, starts=(0, 4), S=None, e=e2, dev=p, fig=p, logged=0, **null):
        c = (ctypes.c_int * len(starts))(*starts)
        a = dict(T=dev, gt=dev, info=dev, gt_flag=dev, result_flag=dev, ids=dev, error=dev, flags=dev)
        a.update(null)
        return lib.d3f_registration_recall(a["T"], logged, a["gt"], a["info"], a["gt_flag"], a["result_flag"], a["ids"], P, n,
                                           ctypes.addressof(c) if starts is not None else None, len(starts) - 1 if S is None else S,
                                           ctypes.addressof(e) if e is not None else None, a["error"], a["flags"], fig, None)
    assert recall(starts=(0, 3, 2, 4)) == -3 and recall(starts=(0, 3)) == -3 and recall(starts=(1, 4)) == -3 and recall(starts=(0, 5)) == -3
    assert recall(starts=tuple([0] * 257 + [4])) == -3                                            # S = 257
    assert recall(P=-1) == -3 and recall(n=0) == -3 and recall(n=-1) == -3 and recall(n=17) == -3 and recall(S=-1) == -3
    assert recall(e=None) == -3 and recall(e=ctypes.c_double(0.0)) == -3 and recall(e=ctypes.c_double(-0.04)) == -3
    assert recall(e=ctypes.c_double(float("nan"))) == -3
    for name in ("T", "gt", "info", "gt_flag", "ids", "error", "flags"):
        assert recall(**{name: None}) == -3, name
        assert recall(logged=1, **{name: None}) == -3, name
    assert recall(fig=None) == -3
    assert recall(P=1 << 28, n=16, starts=(0, 1 << 28)) == -3                                     # P * n >= 2^31
    assert recall(P=0, starts=(0,), dev=None, fig=None) == 0                                       # nothing to do: D3F_OK, no launch
    hdr = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    assert "int d3f_registration_recall(const void* T_est, int logged" in hdr
