#!/usr/bin/env python3
"""tests/golden/matching.npz: what the REFERENCE'S OWN PYTHON computes for feature matching (build machine only).

geometric_registration/evaluate.py is imported UNMODIFIED from the reference tree.  It imports open3d and cv2 (not installed here);
this script provides stub modules of its own: a PointCloud whose transform is R x + t in float64, and placeholders for the RANSAC call
that the fixture does not use.  Then, for every pair of a seeded scene and every count k,

    evaluate.build_correspondence      on the descriptors of the last k rows of both blocks    -> the mutual pairs
    the inlier lines evaluate.py:70-77  on those pairs, through the stub PointCloud               -> the inlier count

evaluate.py:46 fixes num_keypts = 250 inside register2Fragments, which its users edit by hand; the function itself is therefore run
for the count 250 only (its file readers handed the arrays, the RANSAC a placeholder) and must return the same inlier count and ratio
as the lines above.

Scene: utils.synthetic.scene(SEED, n_frag=3, K=1536); the largest count is beyond what d3f_register_pairs accepts and one block is
shorter than it.  Only arrays the reference computed go into the fixture (plus the inputs, the measured margins and the sha256 of the
script); none of its text does.

The reference computes sqrt(2 - 2 s.t) in float32 and moves points in float64; the kernels compute a fused fp32 chain.  Equal results
need margins, and they are measured (tests/matching_np.py: margins): err = the largest difference between the float64 squared
descriptor distances and either fp32 form.  The generator refuses to write the fixture unless
    every row's best and second-best float64 distance, at every count and in both directions, differ by at least FACTOR x err
        (a swap needs two errors to add; 8 leaves a factor 4),
    no mutual pair's float64 point distance lies within FACTOR x the largest fp32 / float64 difference of the threshold,
    the reference's distance matrix holds no NaN.
If that fails, change SEED -- not FACTOR.
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

import matching_np as mnp
from d3feat_amd.utils.synthetic import scene

REF = "/root/reference"
SEED, N_FRAG, K = 4, 3, 1536
COUNTS = (250, 1000, 1536)
THRESHOLD, FACTOR = 0.10, 8.0
OUT = os.path.join(ROOT, "tests", "golden", "matching.npz")


def stub_modules():
    o3d = types.ModuleType("open3d")

    class PointCloud:
        points = None

        def transform(self, T):
            T = np.asarray(T, np.float64)
            self.points = np.asarray(self.points, np.float64) @ T[:3, :3].T + T[:3, 3]
            return self

    thing = lambda *a, **k: types.SimpleNamespace()
    o3d.PointCloud = PointCloud
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64))
    o3d.registration = types.SimpleNamespace(Feature=thing)
    o3d.registration_ransac_based_on_feature_matching = lambda *a, **k: types.SimpleNamespace(transformation=np.eye(4))
    for name in ("TransformationEstimationPointToPoint", "CorrespondenceCheckerBasedOnEdgeLength", "CorrespondenceCheckerBasedOnDistance",
                 "RANSACConvergenceCriteria"):
        setattr(o3d, name, thing)
    sys.modules.update({"open3d": o3d, "cv2": types.ModuleType("cv2")})
    return o3d


def load(rel):
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3], os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s: the reference tree is needed" % REF)
    o3d = stub_modules()
    sys.path.insert(0, REF)                              # evaluate.py imports geometric_registration.utils
    ev = load("geometric_registration/evaluate.py")
    blocks, poses = scene(SEED, n_frag=N_FRAG, K=K)
    pairs = [(a, b) for a in range(N_FRAG) for b in range(a + 1, N_FRAG)]
    gts = []
    for a, b in pairs:                                   # target -> source (gt.log)
        M = np.linalg.inv(poses[a]) @ poses[b]
        M[3] = [0, 0, 0, 1]
        gts.append(M)

    m = mnp.margins(blocks, pairs, gts, COUNTS, THRESHOLD, reference_form=True)
    print("err %.3e  smallest best/second-best gap %.3e (%.1f x err)   point err %.3e  band %.3e (%.1f x)"
          % (m["err"], m["gap"], m["gap"] / m["err"], m["point_err"], m["band"], m["band"] / max(m["point_err"], 1e-300)))
    if not mnp.margins_ok(m, FACTOR):
        raise SystemExit("margins below %g x: change SEED" % FACTOR)

    mutual, offsets = [], [0]
    mutual_count = np.zeros((len(pairs), len(COUNTS)), np.int32)
    gt_inliers = np.zeros_like(mutual_count)
    for p, (a, b) in enumerate(pairs):
        for c, k in enumerate(COUNTS):
            s, t = blocks[a][-k:], blocks[b][-k:]
            with np.errstate(invalid="raise"):          # a negative 2 - 2 s.t would be a NaN of the reference
                corr = ev.build_correspondence(s[:, 3:35], t[:, 3:35])
            # evaluate.py:70-77 with the names of the reference
            frag1 = s[:, :3][corr[:, 0]]
            frag2_pc = o3d.PointCloud()
            frag2_pc.points = o3d.utility.Vector3dVector(t[:, :3][corr[:, 1]])
            frag2_pc.transform(gts[p])
            distance = np.sqrt(np.sum(np.power(frag1 - np.asarray(frag2_pc.points), 2), axis=1))
            if np.isnan(distance).any():
                raise SystemExit("NaN in the reference's result: change SEED")
            mutual.append(corr.astype(np.int32).reshape(-1, 2))
            offsets.append(offsets[-1] + len(corr))
            mutual_count[p, c], gt_inliers[p, c] = len(corr), np.sum(distance < THRESHOLD)
            assert np.array_equal(corr, mnp.mutual_pairs(s[:, 3:35], t[:, 3:35])), (p, k)
    mc, gi = mnp.match_counts(blocks, pairs, gts, COUNTS, THRESHOLD)
    assert np.array_equal(mc, mutual_count) and np.array_equal(gi, gt_inliers)

    # the function of the reference itself, at the count it hard-codes
    assert COUNTS[0] == 250
    by_name = {"cloud_bin_%d" % f: b for f, b in enumerate(blocks)}
    ev.get_keypts = lambda path, name: by_name[name][:, :3]
    ev.get_desc = lambda path, name, desc_name: by_name[name][:, 3:35]
    ev.timestr = "golden"
    with tempfile.TemporaryDirectory() as tmp:
        for p, (a, b) in enumerate(pairs):
            with contextlib.redirect_stdout(io.StringIO()):
                n, ratio, flag = ev.register2Fragments(a, b, "", "", tmp, tmp, {"%d_%d" % (a, b): gts[p]}, "D3Feat", 0.05, THRESHOLD)
            assert (int(n), flag) == (int(gt_inliers[p, 0]), 1) and ratio == gt_inliers[p, 0] / mutual_count[p, 0], (a, b)

    kp = np.zeros((N_FRAG, K, blocks[0].shape[1]), np.float32)
    for f, b in enumerate(blocks):
        kp[f, :len(b)] = b
    sha = hashlib.sha256(open(os.path.join(REF, "geometric_registration/evaluate.py"), "rb").read()).hexdigest()
    np.savez_compressed(OUT, kp=kp, count=np.array([len(b) for b in blocks], np.int32), pairs=np.array(pairs, np.int32),
                        num_keypts=np.array(COUNTS, np.int32), gt_target_to_source=np.array(gts), threshold=np.float64(THRESHOLD),
                        mutual=np.concatenate(mutual), mutual_offsets=np.array(offsets, np.int64), mutual_count=mutual_count,
                        gt_inliers=gt_inliers, err=np.float64(m["err"]), gap=np.float64(m["gap"]), point_err=np.float64(m["point_err"]),
                        band=np.float64(m["band"]), factor=np.float64(FACTOR), sha256_evaluate=np.array(sha))
    print("counts of the blocks %s; mutual %s; inliers %s" % ([len(b) for b in blocks], mutual_count.tolist(), gt_inliers.tolist()))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
