"""The KITTI test on the GPU (d3f_pose_errors, registration.pose_errors / register_kitti_pairs, the drop-in ModelTester.test_kitti):

  1. pose_errors against the float64 numpy restatement (tests/kitti_np.py) at sizes on both sides of the 256-row workgroup and of the
     256 partial sums, one and three estimates per pair, with planted rows: rte bit-equal, flags equal, rre_deg within the library
     arccos allowance, the meters bit-equal to the restatement's tree sums over the device's own per-row values;
  2. the device against what the reference's own Python computed (tests/golden/kitti.npz), the assertions of test_kitti_host.py;
  3. register_kitti_pairs captured in a HIP graph, replayed, the keypoints rewritten in place, replayed again: equal to the eager
     call bit for bit, T equal to register_pairs', per pair equal to register_keypoints + the restatement;
  4. [P, n, 3, 4] estimates of register_pairs_counts equal n single-count calls;
  5. tests/compat_caller_kitti.py (the calls of the reference's test_kitti.py) end to end on a two-pair KITTI tree with seeded random
     weights: files, lines, figures equal to register_kitti_pairs on the same keypoint blocks, the second call reads the files.
     Agreement between paths, not registration quality: the weights are random."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kitti_np
from conftest import GOLDEN, ROOT, write_tf_bundle

pytestmark = pytest.mark.gpu

THR = (2.0, np.pi / 180 * 5)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _row(R, t):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)]).astype(np.float32).reshape(12)


def _equal_with_c_above_one(rng):
    """A float32-rounded rigid transform M with c(M, M) > 1 in float64 (about every second one)."""
    while True:
        M = _row(_rot(rng.normal(size=3), rng.uniform(5, 60)), rng.normal(size=3) * 4)
        if kitti_np.rows(M[None], M[None])["c"][0] > 1.0:
            return M


def _cases(P, per_pair, seed):
    """-> (T f32[P * per_pair, 12], gt f32[P, 12], {name: row}): random estimates on both sides of both thresholds; from 8 pairs on
    the first rows of column 0 are planted; with per_pair = 3 no row of the last column succeeds."""
    rng = np.random.default_rng(seed)
    gt = np.stack([_row(_rot(rng.normal(size=3), rng.uniform(0, 40)), rng.normal(size=3) * [8, 2, 0.3]) for _ in range(P)])
    T = np.empty((P, per_pair, 12), np.float32)
    for p in range(P):
        Rg, tg = gt[p].reshape(3, 4)[:, :3].astype(np.float64), gt[p].reshape(3, 4)[:, 3].astype(np.float64)
        for c in range(per_pair):
            far_r, far_t = rng.random() < 0.3, rng.random() < 0.3 or c == 2
            d = rng.normal(size=3)
            T[p, c] = _row(_rot(rng.normal(size=3), rng.uniform(6, 90) if far_r else rng.uniform(0.1, 4)) @ Rg,
                           tg + d / np.linalg.norm(d) * (rng.uniform(2.2, 9) if far_t else rng.uniform(0.01, 1.8)))
    planted = {}
    if P >= 8:
        I, Q = np.eye(3), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
        plant = [("rte_equals_2", _row(I, [3, 1, 0]), _row(I, [1, 1, 0])), ("rte_1_5", _row(I, [2.5, 1, 0]), _row(I, [1, 1, 0])),
                 ("half_turn", _row(Q @ np.diag([1.0, -1, -1]), [0, 0, 0]), _row(Q, [0, 0.5, 0]))]
        M = _equal_with_c_above_one(rng)
        plant.append(("equal", M, M))
        nan, inf = T[4, 0].copy(), T[5, 0].copy()
        nan[5], inf[3] = np.nan, np.inf
        plant += [("nan", nan, gt[4]), ("inf", inf, gt[5])]
        for p, (name, t, g) in enumerate(plant):
            T[p, 0], gt[p], planted[name] = t, g, p * per_pair
    return T.reshape(-1, 12), gt, planted


def _device_call(device, T, gt, per_pair):
    from d3feat_amd import registration as reg
    Td = torch.from_numpy(T.reshape((-1, 3, 4) if per_pair == 1 else (-1, per_pair, 3, 4))).to(device)
    res = reg.pose_errors(Td, torch.from_numpy(gt.reshape(-1, 3, 4)).to(device), *THR)
    assert res.rte.dtype == res.rre_deg.dtype == res.sums.dtype == torch.float64 and res.flags.dtype == torch.int32 and res.rte.is_cuda
    assert tuple(res.rte.shape) == ((len(gt),) if per_pair == 1 else (len(gt), per_pair)) and tuple(res.sums.shape) == (per_pair, 8)
    return res


def _rre_bound_deg(want):
    """Per row: 4 ulp of the library arccos plus 4 ulp of c carried through arccos (|d arccos / dc| = 1 / sqrt(1 - c^2)), in degrees,
    plus the two roundings of the conversion.  c = +-1 exactly: arccos is exact there (0 and the rounded pi), so only the conversion."""
    c, rre = want["c"], want["rre"]
    with np.errstate(invalid="ignore", divide="ignore"):
        rad = 4 * np.spacing(np.abs(rre)) + np.where(np.abs(c) == 1.0, 0.0, 4 * np.spacing(np.abs(c)) / np.sqrt(1.0 - c * c))
        return rad * 180.0 / np.pi + 2 * np.spacing(np.abs(want["rre_deg"]))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,per_pair", [(1, 1), (255, 1), (256, 1), (257, 1), (600, 1), (70, 3)])
def test_pose_errors_equal_the_restatement(device, P, per_pair):
    T, gt, planted = _cases(P, per_pair, seed=P + per_pair)
    want = kitti_np.pose_errors(T, gt, per_pair, *THR)
    res = _device_call(device, T, gt, per_pair)
    h = res.host()
    rte, deg, fl = h["rte"].reshape(-1), h["rre_deg"].reshape(-1), h["flags"].reshape(-1)
    assert np.array_equal(rte.view(np.uint64), want["rte"].view(np.uint64))
    assert np.array_equal(fl, want["flags"])
    assert np.array_equal(np.isnan(deg), np.isnan(want["rre_deg"]))                 # c > 1 / c < -1 / a NaN input: the same rows
    ok = ~np.isnan(deg)
    excess = np.abs(deg[ok] - want["rre_deg"][ok]) - _rre_bound_deg(want)[ok]
    print("P %d x %d: largest |rre_deg - restatement| %.3e deg, largest excess over the per-row bound %.3e"
          % (P, per_pair, np.max(np.abs(deg[ok] - want["rre_deg"][ok]), initial=0.0), np.max(excess, initial=-np.inf)))
    assert np.all(excess <= 0.0)
    # the meters: the documented tree over the DEVICE's per-row values, bit for bit
    sums = kitti_np.meters(rte, deg, fl, per_pair)
    assert np.array_equal(h["sums"].view(np.uint64), sums.view(np.uint64)), (h["sums"], sums)
    assert np.all(h["sums"][:, 7] == P)
    if P > 1:
        assert 0 < h["sums"][0, 6] < min(h["sums"][0, 2], h["sums"][0, 5]) < P      # both kinds of failure among the random rows
    if planted:
        r = planted
        assert rte[r["rte_equals_2"]] == 2.0 and not fl[r["rte_equals_2"]] & 1 and fl[r["rte_equals_2"]] & 2     # strict
        assert rte[r["rte_1_5"]] == 1.5 and fl[r["rte_1_5"]] == 7 and deg[r["rte_1_5"]] == 0.0
        assert want["c"][r["half_turn"]] == -1.0 and deg[r["half_turn"]] == 180.0 and fl[r["half_turn"]] == 1
        assert want["c"][r["equal"]] > 1.0 and np.isnan(deg[r["equal"]]) and rte[r["equal"]] == 0.0 and fl[r["equal"]] == 1
        assert np.isnan(deg[r["nan"]]) and not fl[r["nan"]] & 6
        assert np.isinf(rte[r["inf"]]) and not fl[r["inf"]] & 5
    if per_pair == 3:                                                              # a column without a success, and without an rte update
        m = res.meters(2)
        assert m["success"]["sum"] == 0.0 and m["success"]["count"] == P and m["rte"]["count"] == 0
        assert m["rte"]["avg"] == 0 and np.isnan(m["rte"]["var"]) and m["rre"]["count"] > 0
        assert res.meters(0)["success"]["sum"] > 0


def test_no_pairs_and_refused_arguments(device):
    from d3feat_amd import registration as reg
    res = reg.pose_errors(torch.zeros((0, 3, 4), device=device), torch.zeros((0, 3, 4), device=device))
    assert res.host()["sums"].tolist() == [[0.0] * 8] and res.meters()["success"]["count"] == 0
    T = torch.zeros((2, 3, 4), device=device)
    with pytest.raises(ValueError):
        reg.pose_errors(T, torch.zeros((3, 3, 4), device=device))
    with pytest.raises(ValueError):
        reg.pose_errors(T, T, rte_threshold=float("nan"))
    with pytest.raises(ValueError):
        reg.pose_errors(T, T, out=reg.pose_errors(torch.zeros((3, 3, 4), device=device), torch.zeros((3, 3, 4), device=device)))


# ---- 2. the reference's own figures ----------------------------------------------------------------------------------------------------
def test_fixture_of_the_reference(device):
    from d3feat_amd import registration as reg
    g = np.load(os.path.join(GOLDEN, "kitti.npz"))
    T = torch.from_numpy(np.ascontiguousarray(g["T"][:, :3])).to(device)
    gt = torch.from_numpy(np.ascontiguousarray(g["gt"][:, :3])).to(device)
    res = reg.pose_errors(T, gt, **reg.KITTI_SUCCESS)
    h = res.host()
    kitti_np.check_against_golden(g, h["rte"][:, 0], h["rre_deg"][:, 0], h["flags"][:, 0], h["sums"][0])
    ids = [str(s) for s in g["anc_ids"]]
    assert [i for i, _, _ in res.failed(ids)] == [str(s) for s in g["failed_ids"]]
    run = res.running(every=10)
    assert [i for i, _ in run] == [10, 20, 30]
    periodic = [kitti_np.split_line(str(l))[1] for l in g["lines"] if ": Feat time" in str(l)]
    for (i, m), nums in zip(run, periodic):
        assert nums[0] == i and m["success"]["sum"] == nums[7] and m["success"]["count"] == nums[8]
        assert abs(m["rte"]["avg"] - nums[5]) <= g["tol_avg_rte"] and abs(m["rre"]["avg"] - nums[6]) <= g["tol_avg_rre"]


# ---- 3. one call, captured -------------------------------------------------------------------------------------------------------------
def _kitti_blocks(seed):
    """3 pairs of K = 64, C = 32 keypoint blocks with planted motions -> (kp f32[6, 64, 36], gt f32[3, 3, 4] source -> target)"""
    from d3feat_amd.utils.synthetic import keypoint_pairs
    return keypoint_pairs(seed, n_pairs=3, K=64, C=32)


def _same(a, b):
    ra, rb = a.registration, b.registration
    for k in ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "nearest"):
        x, y = getattr(ra, k), getattr(rb, k)
        if not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y):
            return False
    return all(torch.equal(getattr(a.errors, k).view(torch.int64) if getattr(a.errors, k).dtype == torch.float64 else getattr(a.errors, k),
                           getattr(b.errors, k).view(torch.int64) if getattr(b.errors, k).dtype == torch.float64 else getattr(b.errors, k))
               for k in ("rte", "rre_deg", "flags", "sums"))


def test_register_kitti_pairs_captured_and_replayed(device):
    from d3feat_amd import ops
    from d3feat_amd import registration as reg
    VOXEL, SEED = 0.3, 5
    (kpa, gta), (kpb, gtb) = _kitti_blocks(1), _kitti_blocks(2)
    kpa, gta, kpb, gtb = (torch.from_numpy(x).to(device) for x in (kpa, gta, kpb, gtb))
    count = torch.full((6,), 64, dtype=torch.int32, device=device)
    eager_a = reg.register_kitti_pairs(kpa, count, gta, VOXEL, seed=SEED)
    eager_b = reg.register_kitti_pairs(kpb, count, gtb, VOXEL, seed=SEED)
    assert not _same(eager_a, eager_b)
    # T is register_pairs' own; per pair the figures are register_keypoints + the restatement
    plain = reg.register_pairs(kpa, count, reg.frame_pairs(3, device), seed=SEED, **reg.EVALUATE_KITTI(VOXEL))
    assert torch.equal(eager_a.T.view(torch.int32), plain.T.view(torch.int32))
    assert reg.frame_pairs(3, device).tolist() == [[0, 1], [2, 3], [4, 5]]
    h = eager_a.errors.host()
    for p in range(3):
        one = reg.register_keypoints(kpa[2 * p], kpa[2 * p + 1], seed=SEED, **reg.EVALUATE_KITTI(VOXEL))
        T1 = one["transformation"][:3].astype(np.float32)
        assert np.array_equal(T1, eager_a.T[p].cpu().numpy())
        w = kitti_np.pose_errors(T1.reshape(1, 12), gta[p].cpu().numpy().reshape(1, 12))
        assert h["rte"][p, 0] == w["rte"][0] and h["flags"][p, 0] == w["flags"][0]
        assert abs(h["rre_deg"][p, 0] - w["rre_deg"][0]) <= _rre_bound_deg(w)[0]
    assert (h["flags"][:, 0] == 7).all(), h                                      # the planted motions are found: 64 rows, 80 % inliers
    kp, gt = kpa.clone(), gta.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            res = reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED)          # eager warm-up on this stream (scratch)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED, out=res)
    keep = pw.kept
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same(res, eager_a)
    kp.copy_(kpb)
    gt.copy_(gtb)
    for t in (res.T, res.errors.rte, res.errors.rre_deg, res.errors.flags, res.errors.sums):
        t.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res.errors._cache = None
    assert _same(res, eager_b) and not _same(res, eager_a)
    assert res.errors.meters()["success"]["count"] == 3
    del keep


# ---- 4. several estimates per pair -----------------------------------------------------------------------------------------------------
def test_estimates_of_every_count_equal_single_count_calls(device):
    from d3feat_amd import registration as reg
    kp, gt = _kitti_blocks(3)
    kp, gt = torch.from_numpy(kp).to(device), torch.from_numpy(gt).to(device)
    count = torch.full((6,), 64, dtype=torch.int32, device=device)
    rc = reg.register_pairs_counts(kp, count, reg.frame_pairs(3, device), num_keypts=(16, 64), seed=1, **reg.EVALUATE_KITTI(0.3))
    both = reg.pose_errors(rc.T, gt)
    assert tuple(both.rte.shape) == (3, 2)
    for c in range(2):
        one = reg.pose_errors(rc.T[:, c].contiguous(), gt)
        for k in ("rte", "rre_deg"):
            assert torch.equal(getattr(both, k)[:, c].view(torch.int64), getattr(one, k).view(torch.int64)), (k, c)
        assert torch.equal(both.flags[:, c], one.flags) and torch.equal(both.sums[c].view(torch.int64), one.sums[0].view(torch.int64))
    assert not torch.equal(both.rte[:, 0], both.rte[:, 1])


# ---- 5. the drop-in caller -------------------------------------------------------------------------------------------------------------
def _kitti_checkout(tmp_path, seed=7):
    """A working directory shaped like the reference checkout for test_kitti.py: data/kitti with sequence 08 of 25 frames moving 1 m
    per frame -- the pairs (8, 0, 10) and (8, 11, 21) --, zero-byte sweeps for the frames no pair uses, the ground truth as icp cache
    files, the reference's KITTI parameters.txt and a REAL checkpoint bundle of seeded random weights."""
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import kitti_config
    from d3feat_amd.utils.synthetic import lidar_sweep
    rng = np.random.default_rng(seed)
    root = tmp_path / "checkout_kitti"
    velo = root / "data" / "kitti" / "sequences" / "08" / "velodyne"
    for d in (velo, root / "data" / "kitti" / "poses", root / "data" / "kitti" / "icp", root / "data" / "kitti" / "config"):
        d.mkdir(parents=True)
    (root / "data" / "kitti" / "config" / "test_kitti.txt").write_text("08\n")
    poses = np.tile(np.eye(4)[:3].reshape(1, 12), (25, 1))
    poses[:, 11] = np.arange(25)                                                   # camera z is forward
    np.savetxt(root / "data" / "kitti" / "poses" / "08.txt", poses, fmt="%.6e")
    pairs, sweeps, gts = [(8, 0, 10), (8, 11, 21)], {}, []
    for k, (_, t0, t1) in enumerate(pairs):
        a = lidar_sweep(seed + k, n_raw=20000).astype(np.float64)
        R, t = _rot([0.02, 0.01, 1], 3.0 + 4 * k), np.array([9.5, 0.4 * k, 0.05])
        b = a @ R.T + t + rng.normal(scale=0.01, size=a.shape)
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, t
        np.save(root / "data" / "kitti" / "icp" / ("8_%d_%d.npy" % (t0, t1)), M)
        gts.append(M)
        sweeps[t0], sweeps[t1] = a, b
    for t in range(25):
        with open(velo / ("%06d.bin" % t), "wb") as f:
            if t in sweeps:
                f.write(np.concatenate([sweeps[t], np.zeros((len(sweeps[t]), 1))], 1).astype(np.float32).tobytes())
    snaps = root / "results_kitti" / "Log_kitti" / "snapshots"
    snaps.mkdir(parents=True)
    (root / "results_kitti" / "Log_kitti" / "parameters.txt").write_text(open(os.path.join(GOLDEN, "parameters_kitti.txt")).read())
    W = build_variables(kitti_config(), seed=seed, randomize_bn=True).values
    write_tf_bundle(str(snaps / "snap-61"), {"KernelPointNetwork/" + k: v for k, v in W.items()}, crc=False)
    (snaps / "snap-61.meta").write_bytes(b"")
    return root, pairs, np.array(gts)


@pytest.mark.timeout(900)
def test_kitti_caller_through_compat(device, tmp_path):
    from d3feat_amd import registration as reg
    root, pairs, gts = _kitti_checkout(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "d3feat_amd.compat_run", os.path.join(ROOT, "tests", "compat_caller_kitti.py"), "--cwd",
                        str(root)], capture_output=True, text=True, cwd=str(root), env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Num_test 2" in r.stdout and "Model restored from results_kitti/Log_kitti/snapshots/snap-61" in r.stdout
    first, second = r.stdout.split("---- call 1 ----")[1].split("---- call 2 ----")
    d1, d2 = (np.load(root / ("kitti_caller_%d.npz" % k)) for k in (1, 2))
    out_dir = root / "geometric_registration_kitti" / ("D3Feat_%s-pred250" % str(d1["experiment"]))
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == ["8@0-10.npz", "8@11-21.npz"], files
    # the files: the reference's keys, the transform of the call, the 250 best rows of both clouds in ascending score order
    assert d1["kp"].shape == (4, 250, 36) and d1["count"].tolist() == [250] * 4
    assert np.array_equal(d1["gt"], gts[:, :3].astype(np.float32))
    for p, name in enumerate(files):
        z = np.load(out_dir / name)
        assert sorted(z.files) == ["anc_pts", "anc_scores", "pos_pts", "pos_scores", "trans"]
        assert z["trans"].shape == (4, 4) and z["trans"].dtype == np.float32 and np.array_equal(z["trans"][:3], d1["T"][p])
        assert np.array_equal(z["anc_pts"], d1["kp"][2 * p, :, :3]) and np.array_equal(z["pos_pts"], d1["kp"][2 * p + 1, :, :3])
        assert np.array_equal(z["anc_scores"], d1["kp"][2 * p, :, -1:]) and np.all(np.diff(z["pos_scores"][:, 0]) >= 0)
    # the figures: register_kitti_pairs on the same keypoint blocks, bit for bit
    want = reg.register_kitti_pairs(torch.from_numpy(d1["kp"]).to(device), torch.from_numpy(d1["count"]).to(device),
                                    torch.from_numpy(d1["gt"]).to(device), float(d1["voxel_size"]))
    h = want.errors.host()
    assert np.array_equal(want.T.cpu().numpy(), d1["T"])
    for k in ("rte", "rre_deg", "flags", "sums"):
        assert np.array_equal(h[k], d1[k], equal_nan=True), k
    # the lines: the reference's skeleton, the figures of the call
    def log_lines(text):
        return [l[15:] for l in text.splitlines() if "Failed with" in l or l[15:].startswith("Total loss")]
    lines = log_lines(first)
    assert kitti_np.split_line(lines[-1])[0] == "Total loss: #, RTE: #, var: #, RRE: #, var: #, Success: # / # (# %)"
    n_failed = int((d1["flags"][:, 0] & 4 == 0).sum())
    assert len(lines) == n_failed + 1
    for l in lines[:-1]:
        sk, nums, ident = kitti_np.split_line(l)
        p = ["8@0", "8@11"].index(ident)
        assert sk == "Failed with RTE: #, RRE: #" and nums[0] == d1["rte"][p, 0]
        assert nums[1] == d1["rre_deg"][p, 0] or (np.isnan(nums[1]) and np.isnan(d1["rre_deg"][p, 0]))
    assert kitti_np.split_line(lines[-1])[1][5:7] == [float(2 - n_failed), 2.0]
    # the second call read the files instead of registering: the same figures from the stored transforms
    assert first.count("Read from") == 0 and second.count("Read from") == 2
    assert log_lines(second) == lines
    for k in ("T", "rte", "rre_deg", "flags", "sums"):
        assert np.array_equal(d1[k], d2[k], equal_nan=True), k
