"""The ETH test (d3f_sanitize_descriptors / d3f_matching_summary, registration.match_scenes, datasets.eth, results.eth_lines, the drop-in
datasets.ETH and compat_run --skip-breakpoints), the part that needs no GPU: the fixture of the reference's own script
(tests/golden/eth.npz, tools/make_golden_eth.py) against the float64 restatement (tests/eth_np.py), the integer rounding rule against
Python's formatting, the host side of the new Python, the argument checks of the two entry points, and -- where the reference checkout
is present -- that every name its test_eth.py and datasets/ETH.py touch exists in compat/."""
import ast
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import eth_np as enp
from conftest import GOLDEN, ROOT

REF = "/root/reference"
COMPAT = os.path.join(ROOT, "compat")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "eth.npz"))


@pytest.fixture(scope="module")
def parsed(golden, tmp_path_factory):
    """blocks, pairs, gts (float64, as the script parsed them), flag, scene_start of the fixture"""
    from d3feat_amd.utils.results import read_gt_log
    g, d = golden, tmp_path_factory.mktemp("eth_gt")
    blocks = [g["kp"][f, :n] for f, n in enumerate(g["count"])]
    gts = []
    for s, text in enumerate(g["gt_logs"].tolist()):
        (d / ("gt%d.log" % s)).write_text(text)
        log, n = read_gt_log(str(d / ("gt%d.log" % s))), int(g["scene_blocks"][s])
        gts += [log.get("%d_%d" % (a, b), np.eye(4)) for a in range(n) for b in range(a + 1, n)]
    return blocks, g["pairs"], gts, g["gt_flag"], g["scene_start"]


# ---- the fixture and the restatement ----------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_describes(golden):
    g = golden
    assert os.path.getsize(os.path.join(GOLDEN, "eth.npz")) <= os.path.getsize(os.path.join(GOLDEN, "matching.npz"))
    assert tuple(g["kp"].shape) == (9, 280, 36) and g["count"].tolist() == [280] * 8 + [180] and int(g["num_keypts"]) == 250
    assert g["scene_blocks"].tolist() == [5, 4, 5, 4] and g["scene_start"].tolist() == [0, 10, 16, 26, 32]
    assert 0 < g["gt_flag"].sum() < len(g["gt_flag"]) == 32                                   # gt.log lists only some pairs
    assert len(str(g["sha256_evaluate_eth"])) == 64 and float(g["factor"]) == 8.0
    desc = g["kp"][:, :, 3:35]
    nan_rows = np.argwhere(np.isnan(desc).any(2))
    whole = [(b, r) for b, r in nan_rows if np.isnan(desc[b, r]).all()]
    part = [(b, r) for b, r in nan_rows if not np.isnan(desc[b, r]).all()]
    first = lambda b: int(g["count"][b]) - min(int(g["count"][b]), 250)
    assert len(whole) == 1 and len(part) >= 3 and all(r >= first(b) for b, r in part)           # the partly bad rows are evaluated
    assert all(r < first(b) for b, r in whole + [tuple(x) for x in np.argwhere(np.isinf(desc).any(2))])
    assert (desc == np.inf).sum() == 1 and (desc == -np.inf).sum() == 1
    bits = desc.view(np.uint32)[np.isnan(desc)]
    assert (bits >> 31).any() and not (bits >> 31).all() and (bits & 0x3fffff).any()            # both signs, a payload
    assert not np.isnan(g["kp"][:, :, :3]).any() and not np.isnan(g["kp"][:, :, 35]).any()
    assert 0 < float(g["err"]) < 1e-5 and float(g["gap"]) >= 8 * float(g["err"]) and float(g["zero_slack"]) >= 8 * float(g["err"])
    assert 0 < float(g["point_err"]) < 1e-5 and float(g["band"]) >= 8 * float(g["point_err"])


def test_restatement_reproduces_the_rows_and_lines_of_the_script(golden, parsed):
    g = golden
    blocks, pairs, gts, flag, scene_start = parsed
    m = enp.margins(blocks, pairs, gts, flag, 250, float(g["threshold"]))
    assert enp.margins_ok(m, float(g["factor"]))
    assert np.isclose(m["err"], float(g["err"]), rtol=0.05) and np.isclose(m["gap"], float(g["gap"]), rtol=1e-6)
    assert np.isclose(m["band"], float(g["band"]), rtol=1e-6)
    mc, gi = enp.pair_counts(blocks, pairs, gts, flag, (250,), float(g["threshold"]))
    assert (mc[flag != 0] > 0).all()                                                            # no listed pair without a mutual match
    rows = enp.rows(mc[:, 0], gi[:, 0], flag)
    assert rows == [[int(a), float(b), int(c)] for a, b, c in g["rows"]]
    assert enp.lines(rows, scene_start, float(g["inlier_ratio"])) == g["lines"].tolist()
    assert np.array_equal(enp.ratio_e8(gi[:, 0], mc[:, 0])[flag != 0], np.rint(g["rows"][flag != 0, 1] * 1e8).astype(np.int64))


def test_integer_rounding_rule_equals_python_formatting():
    a, b = enp.rounding_cases()
    assert len(a) == sum(range(1, 601)) + sum(v + 1 for v in enp.LARGE_B)
    want, got = enp.ratio_e8_python(a, b), enp.ratio_e8(a, b)
    assert np.array_equal(got, want)
    ties = (b > 0) & ((2 * a.astype(np.int64) * 10 ** 8) % np.maximum(2 * b.astype(np.int64), 1) == b)
    assert ties.sum() == 5120 and (b[ties] % 512 == 0).all()
    inexact = np.array([(int(x) / int(y)).as_integer_ratio()[1] * int(x) != (int(x) / int(y)).as_integer_ratio()[0] * int(y)
                        for x, y in zip(a[ties], b[ties])])
    assert inexact.sum() == 3072
    assert (got[b == 0] == 0).all() and got[(a == b) & (b > 0)].tolist() == [10 ** 8] * 607


# ---- datasets.eth -----------------------------------------------------------------------------------------------------------------------
def test_scene_names_config_and_scan_order(tmp_path):
    from d3feat_amd.datasets import eth
    from d3feat_amd.utils.config import threedmatch_config
    assert eth.SCENES == ('gazebo_summer', 'gazebo_winter', 'wood_autmn', 'wood_summer')
    cfg = threedmatch_config()
    assert (cfg.first_subsampling_dl, cfg.KP_extent, cfg.dataset) == (0.03, 1.0, '3DMatch')
    assert eth.apply_config(cfg) is cfg and (cfg.first_subsampling_dl, cfg.KP_extent, cfg.dataset) == (0.05, 2, 'ETH')
    d = tmp_path / "wood_autmn"
    d.mkdir()
    for name in ("Hokuyo_10.ply", "Hokuyo_9.ply", "Hokuyo_0.ply", "Hokuyo_2.ply", "gt.log", "Hokuyo_1.txt"):
        (d / name).write_text("")
    got = [os.path.basename(p) for p in eth.scene_scans(str(tmp_path), "wood_autmn")]
    assert got == ["Hokuyo_0.ply", "Hokuyo_2.ply", "Hokuyo_9.ply", "Hokuyo_10.ply"]


def _log_text(entries):
    return "".join("%d\t %d\t 4\n" % (a, b) + "".join("\t".join(repr(float(v)) for v in row) + "\n" for row in M) for a, b, M in entries)


def test_benchmark_pairs_flags_and_scene_starts(tmp_path):
    from d3feat_amd.datasets import eth
    A, B = np.eye(4), np.eye(4)
    A[:3, 3], B[:3, :3], B[:3, 3] = [1.5, -2.0, 0.25], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0.1, 0.2, 0.3]
    logs = []
    for s, entries in enumerate(([(0, 2, A), (1, 2, B)], [], [(0, 1, B)])):
        (tmp_path / ("gt%d.log" % s)).write_text(_log_text(entries))
        logs.append(str(tmp_path / ("gt%d.log" % s)))
    pairs, gt, flag, start = eth.benchmark([3, 2, 2], logs)
    assert pairs.dtype == np.int32 and gt.dtype == np.float32 and flag.dtype == np.int32
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 2], [3, 4], [5, 6]] and start.tolist() == [0, 3, 4, 5]
    assert flag.tolist() == [0, 1, 1, 0, 1]                                                     # the second scene lists no pair
    eye = np.eye(4, dtype=np.float32)[:3]
    assert np.array_equal(gt[0], eye) and np.array_equal(gt[3], eye)
    assert np.array_equal(gt[1], A[:3].astype(np.float32)) and np.array_equal(gt[2], B[:3].astype(np.float32)) and np.array_equal(gt[4], gt[2])
    # a dict, None, a scene without scans, a scene of one scan
    p2, g2, f2, s2 = eth.benchmark([0, 1, 3], [None, None, {"0_2": A}])
    assert p2.tolist() == [[1, 2], [1, 3], [2, 3]] and f2.tolist() == [0, 1, 0] and s2.tolist() == [0, 0, 0, 3] and p2.shape == (3, 2)
    assert eth.benchmark([], None)[0].shape == (0, 2) and eth.benchmark([], None)[3].tolist() == [0]
    with pytest.raises(ValueError):
        eth.benchmark([3, 2], [None])
    # from a data root: the scans are counted on disk, gt.log is read from the scene's folder
    for s, (scene, n) in enumerate(zip(eth.SCENES, (3, 2, 2, 1))):
        (tmp_path / "ETH" / scene).mkdir(parents=True)
        for k in range(n):
            (tmp_path / "ETH" / scene / ("Hokuyo_%d.ply" % k)).write_text("")
        (tmp_path / "ETH" / scene / "gt.log").write_text(open(logs[s]).read() if s < 3 else "")
    p3, g3, f3, s3 = eth.benchmark(str(tmp_path / "ETH"))
    assert p3.tolist() == pairs.tolist() and f3.tolist() == flag.tolist() and s3.tolist() == [0, 3, 4, 5, 5] and np.array_equal(g3, gt)


# ---- SceneMatching and the lines -----------------------------------------------------------------------------------------------------------
def _summary(rows, scene_start, inlier_ratio=0.05):
    """a SceneMatching as matching_summary leaves it, on host tensors, from rows [num_inliers, ratio, flag] of one count"""
    import torch
    from d3feat_amd import registration as reg
    r = np.array(rows, np.float64).reshape(-1, 3)
    s = reg.SceneMatching(len(r), 1, scene_start, inlier_ratio, torch.device("cpu"))
    fig, _ = enp.scene_figures(rows, scene_start, inlier_ratio)
    s.ratio_e8.copy_(torch.from_numpy(np.rint(r[:, 1] * 1e8).astype(np.int32).reshape(-1, 1)))
    s.figures.copy_(torch.from_numpy(fig.reshape(-1, 1, 4)))
    s.gt_inliers, s.gt_flag = torch.from_numpy(r[:, 0].astype(np.int32).reshape(-1, 1)), torch.from_numpy(r[:, 2].astype(np.int32))
    return s


def test_eth_lines_equal_the_lines_of_the_script(golden):
    from d3feat_amd.datasets import eth
    from d3feat_amd.utils import results
    g = golden
    rows = [[int(a), float(b), int(c)] for a, b, c in g["rows"]]
    s = _summary(rows, g["scene_start"], float(g["inlier_ratio"]))
    assert results.eth_lines(eth.SCENES, s) == g["lines"].tolist()
    assert s.rows(0) == rows and all(type(a) is int and type(b) is float and type(c) is int for a, b, c in s.rows())
    o = s.overall()
    assert g["lines"].tolist()[-4] == "Avergae Matching Recall: %s%%" % o["matching_recall"] and len(o["recall_list"]) == 4
    with pytest.raises(ValueError):
        results.eth_lines(eth.SCENES[:3], s)


def test_scene_matching_conventions():
    from d3feat_amd import registration as reg
    from d3feat_amd.utils.results import feature_matching_recall
    assert reg.EVALUATE_ETH == dict(num_keypts=(250,), distance_threshold=0.10, inlier_ratio=0.05)
    rows = [[3, 0.1, 1], [0, 0.0, 0], [9, 0.04, 1], [1, 0.05000001, 1], [0, 0.0, 1], [7, 0.5, 1]]
    s = _summary(rows, [0, 3, 3, 5, 6])
    sc = [per[0] for per in s.scenes()]
    for k, sl in enumerate((slice(0, 3), slice(3, 3), slice(3, 5), slice(5, 6))):
        assert sc[k] == feature_matching_recall(rows[sl]), k                                     # the same keys and conventions
    assert sc[1] == dict(correct=0, gt=0, recall=0.0, ave_num_inliers=0.0, ave_inlier_ratio=0.0)  # an empty scene
    assert sc[0]["correct"] == 1 and sc[0]["gt"] == 2 and sc[0]["ave_num_inliers"] == 12.0         # the averages divide by `correct`
    assert s.overall()["matching_recall"] == 3 / 5 * 100


def test_python_validation_has_no_cpu_path():
    import torch
    from d3feat_amd import _lib, registration as reg
    z = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.matching_summary(z, z, torch.zeros(2, dtype=torch.int32), [0, 2])
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.sanitize_descriptors(torch.zeros(1, 4, 36))


# ---- the two entry points refuse bad arguments before anything touches the device ------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from d3feat_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    ratio = ctypes.c_double(0.05)

    def summary(P=4, n=1, starts=(0, 4), S=None, r=ratio, dev=p, fig=p):
        c = (ctypes.c_int * len(starts))(*starts)
        return lib.d3f_matching_summary(dev, dev, dev, P, n, ctypes.addressof(c), len(starts) - 1 if S is None else S,
                                        ctypes.addressof(r) if r is not None else None, dev, fig, None)
    assert summary(starts=(0, 3, 2, 4)) == -3 and summary(starts=(0, 3)) == -3 and summary(starts=(1, 4)) == -3
    assert summary(starts=tuple([0] * 257 + [4])) == -3                                           # S = 257
    assert summary(P=-1) == -3 and summary(n=0) == -3 and summary(n=17) == -3 and summary(r=None) == -3
    assert summary(r=ctypes.c_double(float("nan"))) == -3 and summary(dev=None) == -3 and summary(fig=None) == -3
    assert summary(P=0, starts=(0,), dev=None, fig=None) == 0                                      # nothing to do: D3F_OK, no launch
    assert _lib.SCENES_MAX == 256 and "#define D3F_SCENES_MAX 256" in open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    san = lambda n_blocks=2, K=5, ld=36, C=32, kp=p: lib.d3f_sanitize_descriptors(kp, n_blocks, K, ld, C, None)
    assert san(C=48, ld=52) == -3 and san(C=8, ld=12) == -3 and san(ld=34) == -3 and san(n_blocks=-1) == -3 and san(K=-1) == -3
    assert san(kp=None) == -3 and san(n_blocks=0, kp=None) == 0 and san(K=0, kp=None) == 0


# ---- compat_run --skip-breakpoints -----------------------------------------------------------------------------------------------------
def _compat_run(script, cwd, *flags):
    return subprocess.run([sys.executable, "-m", "d3feat_amd.compat_run", str(script), "--cwd", str(cwd)] + list(flags), capture_output=True,
                          text=True, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT), stdin=subprocess.DEVNULL, timeout=300)


def test_skip_breakpoints(tmp_path):
    plain, stops = tmp_path / "plain.py", tmp_path / "stops.py"
    plain.write_text("import sys\nprint('pdb' in sys.modules and sys.modules['pdb'].__file__)\nprint('done', sys.argv[1:])\n")
    stops.write_text("import pdb\nprint('before')\npdb.set_trace()\nprint('after', pdb.__name__, 'compat' in pdb.__file__)\n")
    runs = [_compat_run(plain, tmp_path, *f) for f in ((), ("--skip-breakpoints",), ("--keep-breakpoints",))]
    assert all(r.returncode == 0 for r in runs), [r.stderr[-2000:] for r in runs]
    assert runs[0].stdout == runs[1].stdout == runs[2].stdout and "done []" in runs[0].stdout       # a script without pdb: untouched
    assert "skipped" not in runs[0].stdout
    for flags in ((), ("--skip-breakpoints",)):                                                   # stdin is no terminal: on by default
        r = _compat_run(stops, tmp_path, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert out[:3] == ["before", "[compat_run] pdb.set_trace() skipped (--skip-breakpoints)", "after pdb False"], r.stdout
    r = _compat_run(stops, tmp_path, "--keep-breakpoints")                                         # the real pdb reads EOF and quits
    assert "(Pdb)" in r.stdout and "after pdb" not in r.stdout and "skipped" not in r.stdout
    assert not os.path.exists(os.path.join(COMPAT, "pdb.py")) and not os.path.exists(os.path.join(COMPAT, "pdb"))


# ---- the names the reference's test_eth.py and datasets/ETH.py touch ------------------------------------------------------------------------
def _top_level_names(path):
    out = set()
    for n in ast.parse(open(path).read()).body:
        if isinstance(n, (ast.ClassDef, ast.FunctionDef)):
            out.add(n.name)
        elif isinstance(n, ast.Assign):
            out |= {t.id for t in n.targets if isinstance(t, ast.Name)}
        elif isinstance(n, (ast.Import, ast.ImportFrom)):
            out |= {(a.asname or a.name).split(".")[0] for a in n.names}
    return out


def _class(path, name):
    return next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.ClassDef) and n.name == name)


def _self_attributes(cls):
    return {t.attr for n in ast.walk(cls) if isinstance(n, ast.Assign) for t in n.targets
            if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self"}


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "test_eth.py")), reason="reference checkout not present")
def test_compat_covers_what_test_eth_and_the_eth_dataset_touch():
    from test_compat_scripts import _chains, _import_compat, _resolves
    script = os.path.join(REF, "test_eth.py")
    # every `from <module> import <name>` of the script resolves to a compat file that defines the name
    imports = [(n.module, a.name) for n in ast.walk(ast.parse(open(script).read())) if isinstance(n, ast.ImportFrom) for a in n.names]
    assert ("datasets.ETH", "ETHDataset") in imports and len(imports) == 4
    for module, name in imports:
        path = os.path.join(COMPAT, *module.split(".")) + ".py"
        assert os.path.isfile(path), path
        assert name in _top_level_names(path), (module, name)
    # the methods and attributes the script uses on its objects
    tree = ast.parse(open(script).read())
    used = {(n.value.id, n.attr) for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)}
    assert {("dataset", "init_test_input_pipeline"), ("dataset", "flat_inputs"), ("tester", "generate_descriptor"), ("pdb", "set_trace")} <= used
    common = open(os.path.join(ROOT, "d3feat_amd", "datasets", "common.py")).read()
    assert "def init_test_input_pipeline" in common and "self.flat_inputs" in common
    tester = _class(os.path.join(COMPAT, "utils", "tester.py"), "ModelTester")
    assert "generate_descriptor" in {n.name for n in tester.body if isinstance(n, ast.FunctionDef)}
    cfg_names = {a for v, a in used if v == "config"}
    assert cfg_names == {"load", "first_subsampling_dl", "dataset", "KP_extent"}
    from d3feat_amd.utils.config import Config
    assert all(hasattr(Config, a) for a in cfg_names)
    # the public surface of the reference's dataset class: methods, the attributes its constructor sets, its signature
    ref_cls, our_cls = _class(os.path.join(REF, "datasets", "ETH.py"), "ETHDataset"), _class(os.path.join(COMPAT, "datasets", "ETH.py"), "ETHDataset")
    methods = lambda c: {n.name: [a.arg for a in n.args.args] for n in c.body if isinstance(n, ast.FunctionDef)}
    assert methods(ref_cls) == methods(our_cls)
    init = lambda c: next(n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    assert [ast.literal_eval(d) for d in init(ref_cls).args.defaults] == [ast.literal_eval(d) for d in init(our_cls).args.defaults]
    assert _self_attributes(ref_cls) <= _self_attributes(our_cls)
    assert [b.id for b in ref_cls.bases] == [b.id for b in our_cls.bases] == ["Dataset"]
    # the tensorflow / open3d symbols of the dataset file
    tf, o3d = _import_compat("tensorflow"), _import_compat("open3d")
    chains = _chains(os.path.join(REF, "datasets", "ETH.py"), {"tf", "open3d"})
    assert ("open3d", "voxel_down_sample") in chains and ("tf", "string") in chains
    missing = sorted((r, c) for r, c in chains if not _resolves(tf if r == "tf" else o3d, c))
    assert missing == [], missing
