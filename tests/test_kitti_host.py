"""The KITTI test without a GPU: d3f_pose_errors' argument checks, the float64 restatement (tests/kitti_np.py) and the host helpers
against tests/golden/kitti.npz -- what the reference's own ModelTester.test_kitti / KITTIDataset computed (tools/make_golden_kitti.py)
-- and the host side of the test split (d3feat_amd/datasets/kitti.py)."""
import ctypes
import os

import numpy as np
import pytest

import kitti_np
from conftest import GOLDEN, ROOT
from d3feat_amd.datasets import kitti
from d3feat_amd.utils import results

REF = "/root/reference"
COMPAT = os.path.join(ROOT, "compat")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "kitti.npz"))


@pytest.fixture(scope="module")
def restated(gold):
    n = len(gold["T"])
    return kitti_np.pose_errors(gold["T"][:, :3].reshape(n, 12), gold["gt"][:, :3].reshape(n, 12))


# ---- argument checks: no launch --------------------------------------------------------------------------------------------------------
def test_pose_errors_refuses_bad_arguments_without_a_gpu():
    from d3feat_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    thr = lambda a, b: ctypes.addressof(keep.setdefault((a, b), (ctypes.c_double * 2)(a, b)))
    keep = {}
    good = thr(2.0, np.pi / 180 * 5)
    call = lambda T=p, gt=p, P=4, per=1, t=good, rte=p, rre=p, fl=p, m=None: lib.d3f_pose_errors(T, gt, P, per, t, rte, rre, fl, m, None)
    assert call(P=-1) == -3 and call(per=0) == -3 and call(per=-2) == -3
    assert call(P=1 << 20, per=1 << 12) == -3                                     # P * per_pair does not fit an int
    for name in ("T", "gt", "t", "rte", "rre", "fl"):
        assert call(**{name: None}) == -3, name
    for a, b in ((float("nan"), 0.1), (2.0, float("nan")), (0.0, 0.1), (2.0, 0.0), (-1.0, 0.1), (2.0, -0.1)):
        assert call(t=thr(a, b)) == -3, (a, b)
    assert call(P=0) == 0                                                         # nothing to launch without the meters
    assert call(P=0, T=None) == -3                                                # a NULL pointer is refused whatever P is


# ---- the restatement against the reference's own figures -------------------------------------------------------------------------------
def test_fixture_is_the_references_and_covers_the_cases(gold):
    assert str(gold["meter_dtype"]) == "float32"
    kinds = list(gold["kinds"])
    assert len(kinds) == 39 and {"ok", "rte", "rre", "both", "half_turn", "equal_nan"} <= set(kinds)
    fl = gold["flags"]
    assert set(fl[[k == "rte" for k in kinds]]) == {2} and set(fl[[k == "rre" for k in kinds]]) == {1}
    assert set(fl[[k == "both" for k in kinds]]) == {0} and set(fl[[k == "ok" for k in kinds]]) == {7}
    assert np.isnan(gold["rre_deg"][kinds.index("equal_nan")]) and gold["rre_deg"][kinds.index("half_turn")] == 180.0
    if os.path.isdir(REF):
        import hashlib
        for key, rel in (("sha256_tester", "utils/tester.py"), ("sha256_KITTI", "datasets/KITTI.py")):
            assert str(gold[key]) == hashlib.sha256(open(os.path.join(REF, rel), "rb").read()).hexdigest(), rel


def test_restatement_equals_the_reference(gold, restated):
    lines = kitti_np.check_against_golden(gold, restated["rte"], restated["rre_deg"], restated["flags"], restated["meters"][0])
    assert lines[-1].startswith("Total loss: 0.0, RTE: ") and "b'9@11' Failed with RTE: " in lines[0]


def test_meters_of_the_restatement(gold, restated):
    """The tree-ordered sums against plain sequential ones, and the AverageMeter figures derived from them."""
    m = results.kitti_meters_from_sums(restated["meters"][0])
    seq = results.kitti_meters(restated["rte"], restated["rre_deg"], restated["flags"])
    for k in ("rte", "rre", "success"):
        assert m[k]["count"] == seq[k]["count"]
        for f in ("sum", "avg", "var"):
            assert abs(m[k][f] - seq[k][f]) <= 1e-12 * max(1.0, abs(seq[k][f])), (k, f)
    fl = restated["flags"]
    assert m["rte"]["count"] == int((fl & 1 != 0).sum()) and m["rre"]["count"] == int((fl & 2 != 0).sum())
    assert m["success"]["sum"] == float((fl & 4 != 0).sum()) and m["success"]["count"] == len(fl)
    # a meter that never updated: avg 0 as after reset(), no variance
    none = results.kitti_meters_from_sums(kitti_np.pose_errors(np.zeros((3, 12), np.float32), np.ones((3, 12), np.float32))["meters"][0])
    assert none["rre"]["count"] == 0 and none["rre"]["avg"] == 0 and np.isnan(none["rre"]["var"]) and none["success"]["avg"] == 0.0


def test_tree_sum_is_the_documented_order():
    rng = np.random.default_rng(0)
    v, mask = rng.normal(size=600) * 1e3, rng.uniform(size=600) < 0.7
    part = [0.0] * 256
    for t in range(256):
        for p in range(t, 600, 256):
            if mask[p]:
                part[t] = part[t] + float(v[p])
    s = 128
    while s:
        for t in range(s):
            part[t] = part[t] + part[t + s]
        s //= 2
    assert kitti_np.tree_sum(v, mask) == part[0]
    assert kitti_np.tree_sum(v[:1], mask[:1] | True) == v[0] and kitti_np.tree_sum(v[:0], mask[:0]) == 0.0


def test_save_kitti_pair_writes_the_references_file(tmp_path):
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    T = np.arange(12, dtype=np.float64).reshape(3, 4)
    path = results.save_kitti_pair(str(tmp_path / "out"), b"8@15", "8@58", T, pts, pts + 1, pts[:, :1], pts[:, 1:2])
    assert os.path.basename(path) == "8@15-58.npz" and os.path.exists(path)
    z = np.load(path)
    assert sorted(z.files) == ["anc_pts", "anc_scores", "pos_pts", "pos_scores", "trans"]
    assert z["trans"].dtype == np.float32 and z["trans"].shape == (4, 4) and np.array_equal(z["trans"][3], [0, 0, 0, 1])
    assert np.array_equal(z["trans"][:3], T.astype(np.float32)) and np.array_equal(z["pos_pts"], pts + 1)


# ---- the host side of the split --------------------------------------------------------------------------------------------------------
def write_tree(root, gold, sweeps=()):
    """The synthetic tree of the fixture: poses/<drive>.txt and a zero-byte sweep per frame (a few floats for those in `sweeps`)."""
    os.makedirs(os.path.join(root, "poses"))
    for drive in (8, 9):
        poses = gold["poses_%02d" % drive]
        with open(os.path.join(root, "poses", "%02d.txt" % drive), "w") as f:
            f.write("\n".join(" ".join("%.6e" % v for v in r) for r in poses) + "\n")
        d = os.path.join(root, "sequences", "%02d" % drive, "velodyne")
        os.makedirs(d)
        for t in range(len(poses)):
            with open(os.path.join(d, "%06d.bin" % t), "wb") as f:
                if (drive, t) in sweeps:
                    f.write(np.arange(8, dtype=np.float32).tobytes())


@pytest.fixture(scope="module")
def tree(gold, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti") / "kitti")
    write_tree(root, gold, sweeps={(8, 0), (8, 14)})
    return root


def test_pair_list_equals_the_references(gold, tree):
    pairs = kitti.test_pairs(tree, (8, 9))
    assert pairs == [tuple(int(v) for v in r) for r in gold["pairs"]]
    assert (8, 0, 14) in pairs and (8, 15, 58) not in pairs and {d for d, _, _ in pairs} == {8, 9}
    # the `curr_time += 1` branch was taken: a pair of sequence 8 starts later than the frame after its predecessor's end
    s8 = [p for p in pairs if p[0] == 8]
    assert any(b[1] > a[2] + 1 for a, b in zip(s8, s8[1:]) if a[2] != 14)
    # data without the wrong pair: nothing to remove, no error (the reference's list.remove would raise)
    assert kitti.test_pairs(tree, (9,)) == [p for p in pairs if p[0] == 9]


def test_pair_list_refuses_gaps(gold, tree, tmp_path):
    import shutil
    root = str(tmp_path / "gap")
    shutil.copytree(tree, root)
    os.remove(kitti.velodyne_file(root, 9, 20))
    with pytest.raises(ValueError, match="000020"):
        kitti.test_pairs(root, (9,))
    with pytest.raises(FileNotFoundError):
        kitti.test_pairs(root, (10,))


def test_pair_transform(gold, tree, tmp_path):
    pairs, icp = gold["pairs"], str(tmp_path / "icp")
    os.makedirs(icp)
    for i, want, cached in zip(gold["trans_pairs"], gold["trans"], gold["trans_cached"]):
        d, t0, t1 = (int(v) for v in pairs[i])
        if cached:
            np.save(os.path.join(icp, "%d_%d_%d.npy" % (d, t0, t1)), want)
            assert np.array_equal(kitti.pair_transform(tree, d, t0, t1, icp_dir=icp), want)
            assert np.array_equal(kitti.pair_transform(tree, d, t0, t1, icp_dir=icp, odometry_gt=True), want)   # the cache wins
        else:
            with pytest.raises(FileNotFoundError, match="%d_%d_%d.npy" % (d, t0, t1)):
                kitti.pair_transform(tree, d, t0, t1, icp_dir=icp)
            got = kitti.pair_transform(tree, d, t0, t1, icp_dir=icp, odometry_gt=True)
            # the same float64 products as the reference's :288-289, in the same order
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), i
            assert not os.listdir(icp) or all(not f.startswith("%d_%d_%d" % (d, t0, t1)) for f in os.listdir(icp))
    assert list(gold["trans_cached"]) == [False, False, False, True]


def test_read_pair(tree):
    a, b = kitti.read_pair(tree, 8, 0, 14)
    assert a.shape == b.shape == (2, 3) and a.dtype == np.float32 and np.array_equal(a, [[0, 1, 2], [4, 5, 6]])


def test_constants_of_the_references_call():
    from d3feat_amd import registration as reg
    assert reg.EVALUATE_KITTI(0.3) == dict(max_correspondence_distance=0.3, ransac_n=4, edge_similarity=0.9, checker_distance=0.3,
                                           max_iteration=50000, max_validation=1000)
    assert reg.KITTI_SUCCESS == dict(rte_threshold=2.0, rre_threshold=np.pi / 180 * 5)


# ---- compat coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present")
def test_compat_modules_cover_what_the_kitti_callers_touch():
    from test_compat_scripts import _chains, _import_compat, _resolves
    tf, o3d = _import_compat("tensorflow"), _import_compat("open3d")
    used = set()
    used |= _chains(os.path.join(REF, "test_kitti.py"), {"tf", "open3d"})
    used |= _chains(os.path.join(REF, "utils", "tester.py"), {"tf", "open3d"}, only_functions={"__init__", "test_kitti"})
    used |= _chains(os.path.join(REF, "datasets", "KITTI.py"), {"tf", "open3d"},
                    only_functions={"make_open3d_point_cloud", "make_open3d_feature", "get_tf_mapping", "__getitem__"})
    missing = sorted((r, c) for r, c in used if not _resolves(tf if r == "tf" else o3d, c))
    assert missing == [], missing
    assert ("open3d", "registration.registration_ransac_based_on_feature_matching") in used
    assert ("open3d", "registration.RANSACConvergenceCriteria") in used
    for rel in ("datasets/KITTI.py", "utils/tester.py"):
        assert os.path.isfile(os.path.join(COMPAT, rel)), rel
    assert "def test_kitti" in open(os.path.join(COMPAT, "utils", "tester.py")).read()
