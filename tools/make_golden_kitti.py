#!/usr/bin/env python3
"""tests/golden/kitti.npz: what the REFERENCE'S OWN PYTHON computes for the KITTI test (build machine only).

utils/tester.py and datasets/KITTI.py are loaded UNMODIFIED from the reference tree by path.  They import tensorflow and open3d (not
installed here) and the dataset base class; this script provides stub modules of its own for those (a PointCloud that holds points
and applies R x + t, a voxel_down_sample that returns its input, a registration_icp that returns the identity) and then runs

    ModelTester.test_kitti              unbound, on a fake self / model / dataset: sess.run hands out prepared arrays, the per-pair
                                        .npz files are written beforehand, so the method reads T_ransac from them (tester.py:299-302)
                                        and calls no Open3D; its log is captured                          -> rte / rre / meters / lines
    KITTIDataset.prepare_kitti_ply      on a seeded synthetic tree (contiguous frames, varying speed, a stretch where nothing within
                                        100 frames is 10 m away, a sequence 8 that yields (8, 15, 58))    -> the pair list
    KITTIDataset.__getitem__('test', i) for a few pairs: without a cache file (M of :288-289, ICP = identity) and with one
                                                                                                           -> the transforms

NumPy here is 2.x: a Python float plus a float32 scalar stays float32, so the reference's AverageMeters accumulate in float32
(recorded as `meter_dtype`).  NumPy >= 2.2 also raises for `empty array in list`, which :105 evaluates whenever no frame is far enough;
the NumPy the reference was written for gave False (with a DeprecationWarning).  The module-level name `sorted` of the loaded KITTI
module is pointed at a version that returns a list with that older behaviour, and the name `time` of the loaded tester module at a
clock that stands still (the "Feat time" / "Reg time" figures are then 0.0 and the fixture regenerates byte for byte); nothing else
of the files is touched.

Margins: the float64 definition of include/d3feat_amd.h (tests/kitti_np.py) is evaluated on the same inputs.  The largest
|float32 - float64| difference of rte, of rre_deg and of every printed figure is recorded; the generator refuses to write unless
every non-NaN case lies at least 16 x that difference from its threshold, and stores the differences x 4 as the tolerances of the tests.
Every case takes part in every comparison.  Only arrays and log lines the reference computed go into the fixture (plus the inputs and
the sha256 of the two files); none of its text does.
"""
import contextlib
import hashlib
import importlib.util
import io
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import kitti_np
from d3feat_amd.utils import results

REF = "/root/reference"
SEED = 7
OUT = os.path.join(ROOT, "tests", "golden", "kitti.npz")
EXPERIMENT = "golden"
VOXEL = 0.3


# ---- stubs ---------------------------------------------------------------------------------------------------------------------------
class _List(list):
    def __contains__(self, x):
        if isinstance(x, np.ndarray) and x.size == 0:
            return False
        return list.__contains__(self, x)


def stub_modules():
    o3d = types.ModuleType("open3d")

    class PointCloud:
        points = colors = None

        def transform(self, T):
            T = np.asarray(T, np.float64)
            self.points = np.asarray(self.points, np.float64) @ T[:3, :3].T + T[:3, 3]
            return self

    class Feature:
        data = None

        def resize(self, dim, n):
            pass

    def must_not_run(*a, **k):
        raise AssertionError("the per-pair file must be read instead of running RANSAC")

    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud, KDTreeFlann=None)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64))
    o3d.registration = types.SimpleNamespace(
        Feature=Feature, registration_ransac_based_on_feature_matching=must_not_run,
        registration_icp=lambda *a, **k: types.SimpleNamespace(transformation=np.eye(4)),
        TransformationEstimationPointToPoint=lambda *a, **k: None, ICPConvergenceCriteria=lambda *a, **k: None)
    o3d.voxel_down_sample = lambda pcd, voxel_size: pcd
    tf = types.ModuleType("tensorflow")
    ds, common, tdm = types.ModuleType("datasets"), types.ModuleType("datasets.common"), types.ModuleType("datasets.ThreeDMatch")
    common.Dataset = type("Dataset", (), {"__init__": lambda self, name: None})
    tdm.rotate = lambda pts, num_axis=1: pts
    sys.modules.update({"open3d": o3d, "tensorflow": tf, "datasets": ds, "datasets.common": common, "datasets.ThreeDMatch": tdm})


def load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def mat(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M.astype(np.float32)


def pose_cases(rng):
    """-> (T f32[n,4,4], gt f32[n,4,4], kind[n]): est = gt moved by (angle, distance) of the kind's range."""
    kinds = ["ok"] * 22 + ["rte"] * 5 + ["rre"] * 5 + ["both"] * 5
    rng.shuffle(kinds)
    T, G, K = [], [], []
    for kind in kinds:
        Rg = rot(rng.normal(size=3), rng.uniform(0, 30))
        tg = rng.normal(size=3) * [8.0, 2.0, 0.3]
        ang = rng.uniform(0.2, 3.5) if kind in ("ok", "rte") else rng.uniform(7.0, 60.0)
        dist = rng.uniform(0.05, 1.6) if kind in ("ok", "rre") else rng.uniform(2.5, 6.0)
        d = rng.normal(size=3)
        T.append(mat(rot(rng.normal(size=3), ang) @ Rg, tg + d / np.linalg.norm(d) * dist))
        G.append(mat(Rg, tg))
        K.append(kind)
    # a rotation by exactly 180 degrees: signed permutation matrices, so c = -1 in every precision
    Rg = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    T.insert(13, mat(Rg @ np.diag([1.0, -1.0, -1.0]), [1.0, 0.5, 0.0])); G.insert(13, mat(Rg, [1.0, 0.25, 0.0])); K.insert(13, "half_turn")
    # est == gt with the argument of arccos above 1 in float32 (the reference) AND in float64 (the device): NaN, a failure
    while True:
        M = mat(rot(rng.normal(size=3), rng.uniform(5, 40)), rng.normal(size=3) * 5)
        R32 = M[:3, :3]
        c32 = (np.trace(R32.transpose() @ R32) - 1) / 2
        c64 = kitti_np.rows(M[:3].reshape(1, 12), M[:3].reshape(1, 12))["c"][0]
        if c32 > 1 and c64 > 1:
            break
    T.insert(29, M.copy()); G.insert(29, M.copy()); K.insert(29, "equal_nan")
    return np.stack(T), np.stack(G), K


def drive_poses(rng, drive):
    """Camera poses of a synthetic sequence as the rounded text of poses/<drive>.txt holds them -> (text, f64[n, 12])."""
    if drive == 8:
        # (8, 0, 14): 15 * 0.7 > 10 >= 14 * 0.7; then (8, 15, 58): 44 * 0.23 > 10 >= 43 * 0.23
        step = [0.7] * 15 + [0.23] * 44 + list(rng.uniform(0.2, 1.3, 90)) + [0.001] * 130 + list(rng.uniform(0.3, 1.1, 60))
    else:
        step = list(rng.uniform(0.15, 0.5, 40)) + list(rng.uniform(0.8, 1.4, 70)) + [0.0] * 3 + list(rng.uniform(0.3, 0.9, 40))
    s = np.concatenate([[0.0], np.cumsum(step)])
    yaw = np.cumsum(rng.normal(0, 0.2, len(s)))
    rows = []
    for si, y in zip(s, yaw):
        M = np.hstack([rot([0, 1, 0], y), np.array([[0.02 * si], [0.0], [si]])])     # camera frame: forward is z
        rows.append(M.reshape(-1))
    text = "\n".join(" ".join("%.6e" % v for v in r) for r in rows) + "\n"
    return text, np.genfromtxt(io.StringIO(text)).reshape(-1, 12)


def sweep(rng, n=6):
    return np.concatenate([rng.normal(size=(n, 3)) * 10, rng.uniform(size=(n, 1))], 1).astype(np.float32)


def write_tree(root, poses_text, frames, sweeps):
    """sequences/<drive>/velodyne/<frame>.bin for every frame (zero bytes unless in `sweeps`) and poses/<drive>.txt"""
    os.makedirs(os.path.join(root, "poses"))
    for drive, text in poses_text.items():
        with open(os.path.join(root, "poses", "%02d.txt" % drive), "w") as f:
            f.write(text)
        d = os.path.join(root, "sequences", "%02d" % drive, "velodyne")
        os.makedirs(d)
        for t in range(frames[drive]):
            with open(os.path.join(d, "%06d.bin" % t), "wb") as f:
                if (drive, t) in sweeps:
                    f.write(sweeps[(drive, t)].tobytes())


# ---- the three runs ------------------------------------------------------------------------------------------------------------------
def run_test_kitti(tester, T, G, ids):
    n = len(T)
    state = {"i": 0}
    pts = np.arange(24, dtype=np.float32).reshape(8, 3)

    class Sess:
        def run(self, ops, feed=None):
            if not isinstance(ops, list):
                return None
            i = state["i"]
            state["i"] += 1
            inputs = {"stack_lengths": np.array([4, 4], np.int32), "points": [pts], "trans": G[i]}
            a, p = ids[i]
            return [inputs, np.zeros((8, 32), np.float32), np.linspace(0, 1, 8, dtype=np.float32).reshape(8, 1), a.encode(), p.encode(),
                    np.float32(0)]

    fake = types.SimpleNamespace(sess=Sess(), experiment_str=EXPERIMENT)
    model = types.SimpleNamespace(anchor_inputs=0, out_features=1, out_scores=2, anc_id=3, pos_id=4, accuracy=5, dropout_prob="dropout")
    dataset = types.SimpleNamespace(test_init_op=None, num_test=n, voxel_size=VOXEL)
    d = "geometric_registration_kitti/D3Feat_%s-pred250" % EXPERIMENT
    for (a, p), M in zip(ids, T):
        results.save_kitti_pair(d, a, p, M, pts[:4], pts[4:], pts[:4, :1], pts[4:, :1])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tester.ModelTester.test_kitti(fake, model, dataset)
    assert state["i"] == n
    lines = [l[15:] for l in buf.getvalue().splitlines() if not l.startswith("Read from")]      # '%m/%d %H:%M:%S ' is 15 characters
    return lines


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s: the reference tree is needed" % REF)
    stub_modules()
    kitti = load("datasets/KITTI.py", "datasets.KITTI")
    kitti.sorted = lambda it: _List(sorted(it))
    tester = load("utils/tester.py", "utils_tester_reference")
    tester.time = types.SimpleNamespace(time=lambda: 0.0)              # the two timers print 0.0: the fixture regenerates byte for byte
    rng = np.random.default_rng(SEED)
    here = os.getcwd()

    # -- pose errors ------------------------------------------------------------------------------------------------------------------
    T, G, kinds = pose_cases(rng)
    n = len(T)
    ids = [("%d@%d" % (8 + i % 3, 11 * i), "%d@%d" % (8 + i % 3, 11 * i + 9)) for i in range(n)]
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            lines = run_test_kitti(tester, T, G, ids)
        finally:
            os.chdir(here)
    fail = [l for l in lines if "Failed with" in l]
    periodic = [l for l in lines if " / %d: Feat time" % n in l]
    final = [l for l in lines if l.startswith("Total loss")]
    assert len(fail) + len(periodic) + len(final) == len(lines) and len(final) == 1 and len(periodic) == n // 10, lines
    # the reference's per-pair figures, as it evaluates them (float32 in, float32 out)
    rte32 = np.array([np.linalg.norm(a[:3, 3] - g[:3, 3]) for a, g in zip(T, G)])
    with np.errstate(invalid="ignore"):
        rre32 = np.array([np.arccos((np.trace(a[:3, :3].transpose() @ g[:3, :3]) - 1) / 2) for a, g in zip(T, G)])
    assert rte32.dtype == np.float32 and rre32.dtype == np.float32
    deg32 = rre32 * 180 / np.pi
    ok32 = (rte32 < 2) & ~np.isnan(rre32) & (rre32 < np.pi / 180 * 5)
    failed_ids = [kitti_np.split_line(l)[2] for l in fail]
    assert failed_ids == [ids[i][0] for i in range(n) if not ok32[i]], "the captured log and the per-pair figures disagree"

    # -- the float64 definition on the same inputs, the margins -----------------------------------------------------------------------
    r64 = kitti_np.pose_errors(T[:, :3].reshape(n, 12), G[:, :3].reshape(n, 12))
    assert np.isnan(r64["rre"][kinds.index("equal_nan")]) and np.isnan(rre32[kinds.index("equal_nan")])
    assert np.array_equal(np.isnan(r64["rre"]), np.isnan(rre32)), "NaN in one precision only"
    flags32 = (rte32 < 2).astype(np.int32) | ((~np.isnan(rre32) & (rre32 < np.pi / 180 * 5)).astype(np.int32) << 1) | (ok32.astype(np.int32) << 2)
    assert np.array_equal(flags32, r64["flags"]), "a flag differs between the precisions"
    d_rte = float(np.max(np.abs(rte32.astype(np.float64) - r64["rte"])))
    d_rre = float(np.nanmax(np.abs(deg32.astype(np.float64) - r64["rre_deg"])))
    lines64 = results.kitti_lines([a for a, _ in ids], r64["rte"], r64["rre_deg"], r64["flags"],
                                  final=results.kitti_meters_from_sums(r64["meters"][0]))
    assert len(lines64) == len(lines)
    diffs = {}
    for a, b in zip(lines, lines64):
        (ska, na, _), (skb, nb, _) = kitti_np.split_line(a), kitti_np.split_line(b)
        assert ska == skb and len(na) == len(nb), (a, b)
        for name, x, y in zip(kitti_np.figure_names(a), na, nb):
            if name is None:
                continue
            if np.isnan(x) or np.isnan(y):
                assert np.isnan(x) and np.isnan(y), (a, b)
                continue
            diffs[name] = max(diffs.get(name, 0.0), abs(x - y))
    for name in ("count", "success"):
        assert diffs.pop(name) == 0.0
    margin_rte = float(np.min(np.abs(r64["rte"] - 2.0)))
    margin_rre = float(np.nanmin(np.abs(r64["rre_deg"] - 5.0)))
    print("largest |float32 - float64|: rte %.3e, rre_deg %.3e, printed %s" % (d_rte, d_rre, {k: "%.3e" % v for k, v in diffs.items()}))
    print("closest case to a threshold: rte %.3e m, rre %.3e deg" % (margin_rte, margin_rre))
    if not (margin_rte >= 16 * d_rte and margin_rre >= 16 * d_rre):
        raise SystemExit("a case lies within 16 x the precision difference of its threshold: change SEED")

    # -- pair list and transforms ------------------------------------------------------------------------------------------------------
    poses_text, poses = {}, {}
    for drive in (8, 9):
        poses_text[drive], poses[drive] = drive_poses(rng, drive)
    frames = {d: len(p) for d, p in poses.items()}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "kitti")
        cfg = os.path.join(tmp, "test_kitti.txt")
        with open(cfg, "w") as f:
            f.write("08\n09\n")
        write_tree(root, poses_text, frames, {})
        ds = object.__new__(kitti.KITTIDataset)
        ds.root, ds.icp_path, ds.voxel_size = root, os.path.join(tmp, "icp"), VOXEL
        ds.DATA_FILES = {"test": cfg}
        ds.files, ds.anc_points = {"test": []}, {"test": []}
        with contextlib.redirect_stdout(io.StringIO()):
            ds.prepare_kitti_ply("test")
        pairs = np.array(ds.files["test"], np.int32)
        assert ds.num_test == len(pairs) and (8, 15, 58) not in ds.files["test"]
        # transforms: three pairs without a cache file (M of :288-289), one with
        os.makedirs(ds.icp_path)
        picks = [0, len(pairs) // 2, len(pairs) - 1, 3]
        cached = mat(rot(rng.normal(size=3), 12.0), rng.normal(size=3) * 4).astype(np.float64)
        d, t0, t1 = (int(v) for v in pairs[picks[3]])
        np.save(os.path.join(ds.icp_path, "%d_%d_%d.npy" % (d, t0, t1)), cached)
        trans = []
        for i in picks:
            d, t0, t1 = (int(v) for v in pairs[i])
            for t in (t0, t1):
                with open(ds._get_velodyne_fn(d, t), "wb") as f:
                    f.write(sweep(rng).tobytes())
            trans.append(np.asarray(ds.__getitem__("test", i)[5], np.float64))
        assert np.array_equal(trans[3], cached)
    print("%d pairs (%d of sequence 8); transforms of pairs %s" % (len(pairs), int((pairs[:, 0] == 8).sum()), picks))

    sha = lambda rel: hashlib.sha256(open(os.path.join(REF, rel), "rb").read()).hexdigest()
    tol = {"tol_" + k: np.float64(4 * v) for k, v in diffs.items()}
    np.savez_compressed(
        OUT, T=T, gt=G, kinds=np.array(kinds), anc_ids=np.array([a for a, _ in ids]), pos_ids=np.array([p for _, p in ids]),
        rte=rte32, rre_deg=deg32, flags=flags32, failed_ids=np.array(failed_ids), lines=np.array(lines),
        meter_dtype=np.array("float32"), numpy_version=np.array(np.__version__),
        tol_rte=np.float64(4 * d_rte), tol_rre_deg=np.float64(4 * d_rre), **tol,
        poses_08=poses[8], poses_09=poses[9], pairs=pairs, trans_pairs=np.array(picks, np.int32), trans=np.array(trans),
        trans_cached=np.array([False, False, False, True]),
        sha256_tester=np.array(sha("utils/tester.py")), sha256_KITTI=np.array(sha("datasets/KITTI.py")))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
