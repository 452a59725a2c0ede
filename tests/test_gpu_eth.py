"""The ETH test on the GPU (d3f_sanitize_descriptors, d3f_matching_summary, registration.match_scenes, the drop-in datasets.ETH):

  1. sanitize_descriptors against np.nan_to_num bit for bit at C = 16 / 32 / 64, with NaN of both signs and a payload, +-inf, -0.0 and
     a denormal planted in every column class; the xyz and score columns keep their bits; a second call changes nothing;
  2. ratio_e8 against Python's own "%.8f" formatting for every 0 <= a <= b, b <= 599 and eight b with exact ties;
  3. figures against the restatement (tests/eth_np.py), integer for integer, for P = 0 / 1 / 257 / 600 with empty scenes first, in the
     middle and last and a scene of 257 pairs, n = 1 and 3, mixed flags; the refused arguments;
  4. match_scenes on the fixture of the reference's own script (tests/golden/eth.npz): every row and line; without nan_to_num a listed
     pair's mutual_count differs;
  5. match_scenes captured in a HIP graph with out=, replayed on a second benchmark: bit-equal to the eager call;
  6. tests/compat_caller_eth.py (the calls of the reference's test_eth.py, its pdb.set_trace() included) through compat_run on two
     scenes of three synthetic scans with seeded random weights: the files it writes, through tools/eth_scene.py's function, give the
     rows of tools/eth_test.py's function on the same scans.  Agreement between paths, not matching quality: the weights are random."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eth_np as enp
from conftest import GOLDEN, ROOT, write_tf_bundle

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- 1. sanitise ---------------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x7fc00000, 0xffc00000, 0x7f800123, 0xffffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff],
                   np.uint32).view(np.float32)               # NaN +, NaN -, payloads, +inf, -inf, -0.0, denormals of both signs


@pytest.mark.parametrize("C", [16, 32, 64])
def test_sanitize_equals_nan_to_num_bit_for_bit(device, C):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(C)
    kp = rng.standard_normal((3, 5, 4 + C)).astype(np.float32)
    flat = kp.reshape(-1, 4 + C)
    for r in range(len(flat)):                                # every row: specials in xyz, in the score, at both ends of the descriptor
        for c in (r % 3, 3, 3 + C - 1, 3 + (5 * r) % C, 3 + C):
            flat[r, c] = SPECIAL[(r + c) % len(SPECIAL)]
    flat[4, 3:3 + C] = SPECIAL[1]                             # a whole row of NaN
    for c in range(4 + C):                                    # every special in every column
        flat[5 + c % 9, c] = SPECIAL[c % len(SPECIAL)]
    want = kp.copy()
    want[:, :, 3:3 + C] = np.nan_to_num(kp[:, :, 3:3 + C])
    assert np.isnan(want[:, :, :3]).any() and np.isnan(want[:, :, 3 + C]).any() and np.isfinite(want[:, :, 3:3 + C]).all()
    t = _dev(kp, device)
    assert reg.sanitize_descriptors(t) is t
    got = t.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, :, :3].view(np.uint32), kp[:, :, :3].view(np.uint32))
    assert np.array_equal(got[:, :, 3 + C].view(np.uint32), kp[:, :, 3 + C].view(np.uint32))
    reg.sanitize_descriptors(t)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        reg.sanitize_descriptors(torch.zeros((2, 3, 4 + 48), device=device))
    assert reg.sanitize_descriptors(torch.zeros((0, 3, 4 + C), device=device)).shape[0] == 0


# ---- 2. the rounding of the result file ----------------------------------------------------------------------------------------------------
def test_ratio_e8_equals_python_formatting(device):
    from d3feat_amd import registration as reg
    a, b = enp.rounding_cases()
    want = enp.ratio_e8_python(a, b)
    s = reg.matching_summary(_dev(b, device), _dev(a, device), torch.ones(len(a), dtype=torch.int32, device=device), [0, len(a)])
    got = s.ratio_e8.cpu().numpy()
    assert got.shape == (len(a), 1) and np.array_equal(got[:, 0], want)
    assert (got[b == 0, 0] == 0).all() and (b == 0).sum() == 1
    fig = s.figures.cpu().numpy()
    assert fig.shape == (1, 1, 4) and fig[0, 0].tolist() == [len(a), int((want / 1e8 > 0.05).sum()), int(a.sum()), int(want.sum())]


# ---- 3. the scene sums ---------------------------------------------------------------------------------------------------------------------
SCENE_LISTS = {0: [[0], [0, 0, 0]], 1: [[0, 1], [0, 0, 1, 1]], 257: [[0, 257], [0, 0, 100, 100, 257, 257]],
               600: [[0, 0, 257, 257, 514, 600, 600], [0, 600], [0, 1, 2, 600]]}


@pytest.mark.parametrize("P", [0, 1, 257, 600])
@pytest.mark.parametrize("n", [1, 3])
def test_scene_figures_equal_the_restatement(device, P, n):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(1000 * n + P)
    mc = rng.choice([0, 1, 7, 64, 250, 512, 1024], size=(P, n)).astype(np.int32)
    gi = (rng.random((P, n)) ** 3 * (mc + 1)).astype(np.int32).clip(0, mc)
    flag = (rng.random(P) < 0.6).astype(np.int32)
    for starts in SCENE_LISTS[P]:
        s = reg.matching_summary(_dev(mc, device), _dev(gi, device), _dev(flag, device), starts, inlier_ratio=0.05)
        e8, fig = s.ratio_e8.cpu().numpy(), s.figures.cpu().numpy()
        assert e8.shape == (P, n) and fig.shape == (len(starts) - 1, n, 4) and fig.dtype == np.int64
        for c in range(n):
            rows = enp.rows(mc[:, c], gi[:, c], flag)
            want, fsum = enp.scene_figures(rows, starts, 0.05)
            assert np.array_equal(e8[:, c], np.where(flag != 0, enp.ratio_e8(gi[:, c], mc[:, c]), 0))
            assert np.array_equal(fig[:, c], want), (starts, c)
            # the float sum of the reference against the exact integer sum: any order of N non-negative terms is within (N + 1) u of it
            for k in range(len(starts) - 1):
                N, exact = int(want[k, 0]), fig[k, c, 3] / 1e8
                assert abs(exact - fsum[k]) <= (N + 1) * 2.0 ** -53 * exact
            assert s.rows(c) == rows
            assert [per[c] for per in s.scenes()] == [_recall(rows[a:b]) for a, b in zip(starts, starts[1:])]
        if P == 600 and len(starts) == 7:
            assert fig[0].sum() == 0 and fig[2].sum() == 0 and fig[5].sum() == 0 and fig[1, 0, 0] > 100       # empty first, middle, last


def _recall(rows):
    from d3feat_amd.utils.results import feature_matching_recall
    return feature_matching_recall(rows) if rows else dict(correct=0, gt=0, recall=0.0, ave_num_inliers=0.0, ave_inlier_ratio=0.0)


def test_refused_arguments(device):
    from d3feat_amd import registration as reg
    mc = torch.ones((4, 1), dtype=torch.int32, device=device)
    flag = torch.ones(4, dtype=torch.int32, device=device)
    for starts in ([0, 3, 2, 4], [0, 3], [0, 5], [1, 4], [0] * 257 + [4]):                     # descending, scene_start[S] != P, S = 257
        with pytest.raises(ValueError):
            reg.matching_summary(mc, mc, flag, starts)
    with pytest.raises(ValueError):
        reg.matching_summary(mc, mc, flag[:3], [0, 4])
    with pytest.raises(ValueError):
        reg.matching_summary(mc, mc, flag, [0, 4], inlier_ratio=float("nan"))
    ok = reg.matching_summary(mc, mc, flag, [0] * 256 + [4])                                      # S = 256 is accepted
    assert ok.figures.shape == (256, 1, 4) and ok.figures[:255].sum().item() == 0 and ok.figures[255, 0].tolist() == [4, 4, 4, 4 * 10 ** 8]
    with pytest.raises(ValueError):
        reg.matching_summary(mc, mc, flag, [0, 4], out=reg.matching_summary(mc, mc, flag, [0, 2, 4]))


# ---- 4. the fixture of the reference's script ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "eth.npz"))


def _gt_of_fixture(g, tmp):
    from d3feat_amd.utils.results import read_gt_log
    gts = []
    for s, text in enumerate(g["gt_logs"].tolist()):
        (tmp / ("gt%d.log" % s)).write_text(text)
        log, n = read_gt_log(str(tmp / ("gt%d.log" % s))), int(g["scene_blocks"][s])
        gts += [log.get("%d_%d" % (a, b), np.eye(4))[:3] for a in range(n) for b in range(a + 1, n)]
    return np.asarray(gts, np.float64).astype(np.float32)


def test_match_scenes_on_the_fixture_of_the_reference(device, golden, tmp_path):
    from d3feat_amd import registration as reg
    from d3feat_amd.datasets import eth
    from d3feat_amd.utils import results
    g = golden
    gt = _gt_of_fixture(g, tmp_path)
    args = lambda: (_dev(g["kp"], device), _dev(g["count"], device), _dev(g["pairs"], device), _dev(gt, device), _dev(g["gt_flag"], device),
                    g["scene_start"])
    out = reg.match_scenes(*args(), **reg.EVALUATE_ETH)
    assert out.summary.rows(0) == [[int(a), float(b), int(c)] for a, b, c in g["rows"]]
    assert results.eth_lines(eth.SCENES, out.summary) == g["lines"].tolist()
    raw = reg.match_scenes(*args(), nan_to_num=False, **reg.EVALUATE_ETH)
    listed = g["gt_flag"] != 0
    a, b = out.matching.mutual_count.cpu().numpy()[listed], raw.matching.mutual_count.cpu().numpy()[listed]
    assert (a != b).any(), "the planted rows do not matter"


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------------
def _benchmark(seed, device):
    """two scenes of 4 and 3 blocks of 96 rows (scene(seed)), every other pair listed, NaN planted -> the arguments of match_scenes"""
    from d3feat_amd.datasets import eth
    from d3feat_amd.utils.synthetic import scene
    blocks, logs = [], []
    for k, n in enumerate((4, 3)):
        b, poses = scene(seed + k, n_frag=n, K=96)
        blocks += b
        logs.append({"%d_%d" % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i in range(n) for j in range(i + 1, n) if (i + j + k) % 2})
    kp = np.stack(blocks)
    kp[1, 5, 7], kp[4, 90, 3:35], kp[6, 40, 20] = np.nan, np.nan, np.inf
    pairs, gt, flag, start = eth.benchmark([4, 3], logs)
    return _dev(kp, device), torch.full((7,), 96, dtype=torch.int32, device=device), _dev(pairs, device), _dev(gt, device), _dev(flag, device), start


def _same(x, y):
    return all(torch.equal(a, b) for a, b in ((x.matching.mutual_count, y.matching.mutual_count), (x.matching.gt_inliers, y.matching.gt_inliers),
                                              (x.summary.ratio_e8, y.summary.ratio_e8), (x.summary.figures, y.summary.figures)))


def test_match_scenes_captured_and_replayed(device):
    from d3feat_amd import ops
    from d3feat_amd import registration as reg
    A, B = _benchmark(21, device), _benchmark(31, device)
    assert A[5].tolist() == B[5].tolist() and torch.equal(A[2], B[2])
    kw = dict(num_keypts=(50, 96), distance_threshold=0.10, inlier_ratio=0.05)
    eager_a = reg.match_scenes(A[0].clone(), *A[1:], **kw)
    eager_b = reg.match_scenes(B[0].clone(), *B[1:], **kw)
    assert not _same(eager_a, eager_b) and eager_a.matching.mutual_count.min().item() > 0
    kp, gt, flag = A[0].clone(), A[3].clone(), A[4].clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            res = reg.match_scenes(kp, A[1], A[2], gt, flag, A[5], **kw)                          # eager warm-up on this stream (scratch)
        stream.synchronize()
        kp.copy_(A[0])
        with torch.cuda.graph(graph, stream=stream):
            reg.match_scenes(kp, A[1], A[2], gt, flag, A[5], out=res, **kw)
    keep = pw.kept
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same(res, eager_a) and not torch.isnan(kp[:, :, 3:35]).any()
    kp.copy_(B[0])
    gt.copy_(B[3])
    flag.copy_(B[4])
    for t in (res.matching.mutual_count, res.matching.gt_inliers, res.summary.ratio_e8, res.summary.figures):
        t.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res.summary._cache = None
    assert _same(res, eager_b) and not _same(res, eager_a)
    assert res.summary.rows(1) == eager_b.summary.rows(1)
    del keep


# ---- 6. the drop-in caller -----------------------------------------------------------------------------------------------------------------
def _eth_checkout(tmp_path, seed=9):
    """A working directory shaped like the reference checkout for test_eth.py: data/ETH with two of the four scenes, three scans each
    (numbered 0, 1, 2; every scan a few thousand points after the 0.0625 m grid: a 2.5 m room in three translated frames), a gt.log per scene
    that lists two of the three pairs, and a results/Log_* folder whose parameters.txt says dataset = ETH with a REAL checkpoint bundle
    of seeded random weights."""
    from d3feat_amd.datasets import eth
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    from d3feat_amd.utils.ply import write_ply
    from d3feat_amd.utils.synthetic import room_fragment
    rng = np.random.default_rng(seed)
    root = tmp_path / "checkout_eth"
    scenes = (eth.SCENES[0], eth.SCENES[2])
    for k, sc in enumerate(scenes):
        (root / "data" / "ETH" / sc).mkdir(parents=True)
        world = room_fragment(seed + k, n_raw=60000, edge=2.5).astype(np.float64)
        text = []
        poses = []
        for i in range(3):
            # the scans differ by a translation of whole coarsest-level voxels and by which 90 % of the points they hold: a network with
            # random weights knows nothing of rotations, and the test needs pairs that do match
            M = np.eye(4)
            M[:3, 3] = 4.0 * rng.integers(-2, 3, 3)
            poses.append(M)
            keep = rng.random(len(world)) < 0.9
            pts = (world[keep] - M[:3, 3]).astype(np.float32)
            assert write_ply(str(root / "data" / "ETH" / sc / ("Hokuyo_%d.ply" % i)), [pts], ["x", "y", "z"])
        for a, b in ((0, 1), (1, 2)):
            T = np.linalg.inv(poses[a]) @ poses[b]
            text.append("%d\t %d\t 3\n" % (a, b) + "".join("\t".join(repr(float(v)) for v in row) + "\n" for row in T))
        (root / "data" / "ETH" / sc / "gt.log").write_text("".join(text))
    snaps = root / "results" / "Log_ethtest00" / "snapshots"
    snaps.mkdir(parents=True)
    params = open(os.path.join(GOLDEN, "parameters_3dmatch.txt")).read().replace("dataset = 3DMatch", "dataset = ETH")
    assert "dataset = ETH" in params
    (root / "results" / "Log_ethtest00" / "parameters.txt").write_text(params)
    W = build_variables(threedmatch_config(), seed=seed, randomize_bn=True).values
    write_tf_bundle(str(snaps / "snap-54"), {"KernelPointNetwork/" + k: v for k, v in W.items()}, crc=False)
    (snaps / "snap-54.meta").write_bytes(b"")
    (root / "geometric_registration").mkdir()
    return root, scenes, W


@pytest.mark.timeout(900)
def test_eth_caller_through_compat(device, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eth_scene
    import eth_test
    from d3feat_amd.datasets import eth
    from d3feat_amd.utils.config import Config
    root, scenes, W = _eth_checkout(tmp_path)
    r = subprocess.run([sys.executable, "-m", "d3feat_amd.compat_run", os.path.join(ROOT, "tests", "compat_caller_eth.py"), "--cwd", str(root)],
                       capture_output=True, text=True, cwd=str(root), env=dict(os.environ, PYTHONPATH=ROOT), stdin=subprocess.DEVNULL,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pdb.set_trace() skipped" in r.stdout and "Model restored from results/Log_ethtest00/snapshots/snap-54" in r.stdout
    info = np.load(root / "eth_caller.npz")
    assert info["ids"].tolist() == ["%s/Hokuyo_%d.ply" % (s, i) for s in scenes for i in range(3)]
    desc_root = root / "geometric_registration" / ("D3Feat_%s" % str(info["experiment"]))
    files = sorted(str(p.relative_to(desc_root)) for p in desc_root.rglob("*.npy"))
    assert len(files) == 18 and "descriptors/%s/cloud_bin_2.D3Feat.npy" % scenes[1] in files, files
    logs = [str(root / "data" / "ETH" / s / "gt.log") for s in scenes]
    blocks, per_scene = eth_scene.load_blocks(str(desc_root), scenes, 250)
    assert per_scene == [3, 3] and all(b.shape == (250, 36) for b in blocks)
    from_files = eth_scene.evaluate(blocks, per_scene, logs, device=device)
    # the engine path on the same scans
    cfg = Config()
    cfg.load(str(root / "results" / "Log_ethtest00"))
    eth.apply_config(cfg)
    scans = [[eth.read_scan(p) for p in eth.scene_scans(str(root / "data" / "ETH"), s)] for s in scenes]
    assert all(2000 < len(s) < 20000 for sc in scans for s in sc), [len(s) for sc in scans for s in sc]
    engine, eblocks, eng = eth_test.run(scans, logs, cfg, W, device=device, limits=info["limits"])
    assert eng.fallbacks == 0
    assert from_files.summary.scene_start == engine.summary.scene_start == (0, 3, 6)
    print("rows from the files ", from_files.summary.rows(0))
    print("rows of the engine  ", engine.summary.rows(0))
    print("mutual from the files", from_files.matching.mutual_count[:, 0].tolist(), " engine", engine.matching.mutual_count[:, 0].tolist())
    assert from_files.summary.rows(0) == engine.summary.rows(0)
    assert max(r[0] for r in engine.summary.rows(0)) > 25                                         # pairs that do match: the rows say something
    assert [r[2] for r in engine.summary.rows(0)] == [1, 0, 1, 1, 0, 1]
