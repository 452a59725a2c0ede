#!/usr/bin/env python3
"""tests/golden/repeatability.npz: what the REFERENCE'S OWN PYTHON computes for keypoint repeatability (build machine only).

repeatability/evaluate_3dmatch_our.py and repeatability/evaluate_kitti_our.py are imported UNMODIFIED from the reference tree.  They
import open3d (not installed here) for one thing only -- PointCloud().transform(gt) on the keypoints -- and datasets.KITTI for the
file list of the test split; this script provides stub modules of its own for both (a PointCloud whose transform is R x + t in
float64) and then runs

    evaluate_kitti_our.deal_with_one_pair       on every pair of a seeded scene at every count      (source moved, 0.5 m)
    evaluate_3dmatch_our.deal_with_one_scene    on a temporary directory tree laid out as the script expects: placeholder
                                                cloud_bin_*.ply files, keypoints/<scene>/*.npy, gt_result/<scene>-evaluation/gt.log
                                                (target moved, 0.1 m); once with the scene's gt.log, once per pair with a
                                                gt.log of that pair alone, which returns the pair's own ratio

Scene: utils.synthetic.scene(SEED, n_frag=6, K=512), block CUT_BLOCK cut to its best 300 rows; gt.log lists only some of the pairs.
Only arrays the reference computed go into the fixture (plus the inputs and the sha256 of the two scripts); none of its text does.

The fixture's counts are to be reproduced EXACTLY by float64 code with another rounding order, so the generator refuses to write it
unless every column minimum of every (pair, count) keeps at least BAND = 1e-6 from the threshold (a transform in another operation
order moves a distance by ~1e-15).  If that fails, change SEED -- not BAND.
"""
import hashlib
import importlib.util
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MPLBACKEND", "Agg")
import numpy as np

import repeatability_np as rnp
from d3feat_amd.utils.synthetic import scene

REF = "/root/reference"
SEED, N_FRAG, K, CUT_BLOCK, CUT_ROWS = 3, 6, 512, 2, 300
COUNTS = (4, 8, 16, 32, 64, 128, 256, 512)
UNLISTED = ((0, 3), (1, 4), (2, 5), (0, 5))          # pairs gt.log does not list
BAND = 1e-6
SCENE = "synthetic-room"
OUT = os.path.join(ROOT, "tests", "golden", "repeatability.npz")


def stub_modules():
    o3d = types.ModuleType("open3d")

    class PointCloud:
        points = None

        def transform(self, T):
            T = np.asarray(T, np.float64)
            self.points = np.asarray(self.points, np.float64) @ T[:3, :3].T + T[:3, 3]
            return self

    o3d.PointCloud = PointCloud
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64))
    o3d.VerbosityLevel = types.SimpleNamespace(Error=0)
    o3d.set_verbosity_level = lambda level: None
    ds, kitti = types.ModuleType("datasets"), types.ModuleType("datasets.KITTI")
    kitti.KITTIDataset = type("KITTIDataset", (), {})
    ds.KITTI = kitti
    sys.modules.update({"open3d": o3d, "datasets": ds, "datasets.KITTI": kitti})


def load(rel):
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3], os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gt_log_text(pairs, mats):
    lines = []
    for (a, b), M in zip(pairs, mats):
        lines.append("%d\t %d\t %d\n" % (a, b, N_FRAG))
        lines += ["\t ".join(repr(float(v)) for v in row) + "\t \n" for row in M]
    return "".join(lines)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s: the reference tree is needed" % REF)
    stub_modules()
    sys.path.insert(0, REF)                              # evaluate_3dmatch_our imports geometric_registration.utils
    kitti, tdm = load("repeatability/evaluate_kitti_our.py"), load("repeatability/evaluate_3dmatch_our.py")
    blocks, poses = scene(SEED, n_frag=N_FRAG, K=K)
    xyz = [np.ascontiguousarray(b[:, :3]) for b in blocks]
    xyz[CUT_BLOCK] = xyz[CUT_BLOCK][-CUT_ROWS:]
    pairs = [(a, b) for a in range(N_FRAG) for b in range(a + 1, N_FRAG)]
    listed = np.array([p not in UNLISTED for p in pairs])
    gt_ts = [np.linalg.inv(poses[a]) @ poses[b] for a, b in pairs]          # target -> source (3DMatch gt.log)
    for M in gt_ts:
        M[3] = [0, 0, 0, 1]
    gt_st = [np.linalg.inv(M) for M in gt_ts]                                 # source -> target (KITTI trans)
    for M in gt_st:
        M[3] = [0, 0, 0, 1]
    log_text = gt_log_text([p for p, l in zip(pairs, listed) if l], [M for M, l in zip(gt_ts, listed) if l])

    # KITTI convention: the function of the script on every pair
    r_kitti = np.array([[kitti.deal_with_one_pair(xyz[a][-k:], xyz[b][-k:], gt_st[i], k, threshold=0.5) for k in COUNTS]
                        for i, (a, b) in enumerate(pairs)], np.float64)
    s_kitti = np.array([np.mean(r_kitti[listed, c]) for c in range(len(COUNTS))])      # evaluate_kitti_our.py:44

    # 3DMatch convention: the script's scene function on the directory tree it reads
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        frag = os.path.join(tmp, "data", "3DMatch", "fragments", SCENE)
        kdir = os.path.join(tmp, "geometric_registration", "D3Feat_golden", "keypoints", SCENE)
        gdir = os.path.join(tmp, "geometric_registration", "gt_result", SCENE + "-evaluation")
        work = os.path.join(tmp, "repeatability")
        for d in (frag, kdir, gdir, work):
            os.makedirs(d)
        for f, x in enumerate(xyz):
            open(os.path.join(frag, "cloud_bin_%d.ply" % f), "w").close()
            np.save(os.path.join(kdir, "cloud_bin_%d.npy" % f), x)
        os.chdir(work)
        try:
            def run(text):
                with open(os.path.join(gdir, "gt.log"), "w") as f:
                    f.write(text)
                return [tdm.deal_with_one_scene(SCENE, "D3Feat", "golden", k) for k in COUNTS]
            s_3dm = np.array(run(log_text), np.float64)
            r_3dm = np.array([run(gt_log_text([p], [M])) for p, M in zip(pairs, gt_ts)], np.float64)
        finally:
            os.chdir(here)

    # the band, and the counts of the float64 restatement, for the fixture's own scene
    ipairs = np.array(pairs, np.int32)
    for name, gts, thr, moved, ratios in (("3dmatch", gt_ts, 0.1, "target", r_3dm), ("kitti", gt_st, 0.5, "source", r_kitti)):
        gap = rnp.band(xyz, pairs, gts, COUNTS, thr, moved)
        print("%-8s closest column minimum to the threshold: %.3e; mean ratio per count %s"
              % (name, gap, np.round(ratios.mean(0), 4).tolist()))
        if not gap >= BAND:
            raise SystemExit("%s: a column minimum lies %.3e from the threshold (< %g): change SEED" % (name, gap, BAND))
        counts = np.rint(ratios * np.asarray(COUNTS)).astype(np.int64)
        assert np.array_equal(counts, rnp.repeat_counts(xyz, pairs, gts, COUNTS, thr, moved)), name
    kp = np.zeros((N_FRAG, K, 3), np.float32)
    for f, x in enumerate(xyz):
        kp[f, :len(x)] = x
    sha = lambda rel: hashlib.sha256(open(os.path.join(REF, rel), "rb").read()).hexdigest()
    np.savez_compressed(OUT, kp=kp, count=np.array([len(x) for x in xyz], np.int32), pairs=ipairs, listed=listed,
                        num_keypts=np.array(COUNTS, np.int32), gt_target_to_source=np.array(gt_ts), gt_source_to_target=np.array(gt_st),
                        gt_log=np.array(log_text), ratios_3dmatch=r_3dm, scene_3dmatch=s_3dm, ratios_kitti=r_kitti, scene_kitti=s_kitti,
                        threshold_3dmatch=np.float64(0.1), threshold_kitti=np.float64(0.5),
                        sha256_evaluate_3dmatch_our=np.array(sha("repeatability/evaluate_3dmatch_our.py")),
                        sha256_evaluate_kitti_our=np.array(sha("repeatability/evaluate_kitti_our.py")))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
