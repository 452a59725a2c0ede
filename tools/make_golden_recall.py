#!/usr/bin/env python3
"""tests/golden/recall.npz and tests/golden/gt_info_hotel3.info: the fixture of the 3DMatch registration recall (build machine only).

gt_info_hotel3.info is the reference's own gt.info of sun3d-hotel_umd-maryland_hotel3 (data; its gt.log is tests/golden/
gt_log_hotel3.log already), copied byte for byte.  On that scene -- all 666 pairs of its 37 fragments, datasets.threedmatch.benchmark --
the generator builds two seeded estimates per pair: for a pair gt.log lists, the ground truth composed with a perturbation whose error
sqrt(p) runs over LADDER, well inside to well outside the benchmark's 0.2, in a random direction of the six-dimensional error vector
(translation, rotation, or both); for the others a random rigid motion.  The estimate is the inverse of that matrix rounded to
float32, source -> target, as RANSAC returns it.  Consecutive pairs are among the listed ones; a few pairs gt.log does not list get a
result (false positives) and a few listed pairs get none (result_flag).

Both restatements of tests/recall_np.py are evaluated, on the float32 estimates and on the float64 matrices a .log file would hold
(np.linalg.inv of the estimates, what results.write_registration_log writes): (a) the device definition, (b) the .m files line by
line.  The generator writes the file only if every recorded p differs from err2 by more than 1e-6 relative under both, so that no flag
depends on the inversion method; a draw that does not is dropped and drawn again, and more than 5 % dropped draws is an error.  The
largest relative difference between (a) and (b) is recorded; the tests compare against (b) with 4 x that difference (the rule of
kitti.npz).  The figure also goes into tests/golden/recall_manifest.json, with the sha256 of the two fixture files and of the .m files.
"""
import hashlib
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import recall_np as rnp
from d3feat_amd.datasets import threedmatch

REF = "/root/reference"
SCENE = "sun3d-hotel_umd-maryland_hotel3"
FRAGMENTS = 37
SEED = 11
N = 2
ERR2 = 0.04
MARGIN = 1e-6
LADDER = (0.01, 0.05, 0.1, 0.15, 0.19, 0.199, 0.201, 0.21, 0.25, 0.4, 1.0, 2.5)
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG, INFO, OUT, MANIFEST = (os.path.join(GOLDEN, f) for f in ("gt_log_hotel3.log", "gt_info_hotel3.info", "recall.npz", "recall_manifest.json"))
M_FILES = ("geometric_registration/3dmatch/evaluate.m", "geometric_registration/3dmatch/external/ElasticReconstruction/mrEvaluateRegistration.m",
           "geometric_registration/3dmatch/external/ElasticReconstruction/mrLoadInfo.m",
           "geometric_registration/3dmatch/external/ElasticReconstruction/mrLoadLog.m")


def quat_matrix(v):
    """vector part v of a unit quaternion with a non-negative scalar part -> rotation matrix"""
    x, y, z = v
    w = np.sqrt(max(1.0 - float(v @ v), 0.0))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def perturbation(rng, info, level):
    """A rigid D whose error vector er has er' info er / info[0][0] = level ^ 2, up to the rounding of the construction."""
    kind = rng.integers(3)
    er = rng.normal(size=6) * (np.array([1, 1, 1, 0, 0, 0]) if kind == 0 else np.array([0, 0, 0, 1, 1, 1]) if kind == 1 else np.ones(6))
    er *= level / np.sqrt(er @ info @ er / info[0, 0])
    if er[3:] @ er[3:] > 0.81:                                    # a rotation beyond 128 degrees: shrink it, the level goes with it
        er[3:] *= 0.9 / np.linalg.norm(er[3:])
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = quat_matrix(er[3:]), er[:3]
    return D


def random_rigid(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = quat_matrix(q[1:] * np.sign(q[0])), rng.normal(size=3)
    return M


def estimate(logged):
    """the .log matrix -> the float32 [3, 4] estimate source -> target whose inverse it is"""
    return np.linalg.inv(logged)[:3].astype(np.float32)


def evaluate(T, bm, result_flag):
    """-> (a, b, a_logged, b_logged, logged): both restatements on both input forms"""
    M = np.tile(np.eye(4), T.shape[:2] + (1, 1))
    M[:, :, :3] = T.astype(np.float64)
    logged = np.linalg.inv(M)
    args = (bm.gt, bm.info, bm.gt_flag, bm.ids, bm.scene_start)
    kw = dict(err2=ERR2, result_flag=result_flag)
    return (rnp.device(T, *args, **kw), rnp.matlab(T, *args, **kw), rnp.device(logged, *args, logged=True, **kw),
            rnp.matlab(logged, *args, logged=True, **kw), logged)


def main():
    src = os.path.join(REF, "geometric_registration", "gt_result", SCENE + "-evaluation")
    if not os.path.isdir(src):
        raise SystemExit("%s: the reference tree is needed" % src)
    assert open(os.path.join(src, "gt.log"), "rb").read() == open(LOG, "rb").read(), "gt_log_hotel3.log is not the reference's gt.log"
    shutil.copyfile(os.path.join(src, "gt.info"), INFO)
    bm = threedmatch.benchmark(None, [FRAGMENTS], scenes=[SCENE], gt_logs=[LOG], gt_infos=[INFO])
    P = len(bm.pairs)
    rng = np.random.default_rng(SEED)
    apart = bm.ids[:, 1] - bm.ids[:, 0] > 1
    listed = bm.gt_flag != 0
    assert (listed & ~apart).sum() >= 10 and (listed & apart).sum() >= 10, "the scene must list consecutive and non-consecutive pairs"
    result_flag = bm.gt_flag.copy()
    false_pos = rng.choice(np.nonzero(~listed & apart)[0], 5, replace=False)
    no_result = rng.choice(np.nonzero(listed & apart)[0], 3, replace=False)
    result_flag[false_pos], result_flag[no_result] = 1, 0
    result_flag[np.nonzero(~listed & ~apart)[0][:1]] = 1           # a consecutive pair gt.log does not list, with a result: counts nowhere

    T = np.zeros((P, N, 3, 4), np.float32)
    level = np.zeros((P, N))
    draws = dropped = 0
    k = 0
    for p in range(P):
        for c in range(N):
            if not listed[p]:
                T[p, c] = estimate(random_rigid(rng))
                continue
            while True:
                draws += 1
                lv = LADDER[k % len(LADDER)]
                T[p, c] = estimate(bm.gt[p] @ perturbation(rng, bm.info[p], lv))
                one = type(bm)(bm.pairs[p:p + 1], bm.ids[p:p + 1], bm.gt[p:p + 1], bm.info[p:p + 1], bm.gt_flag[p:p + 1], np.array([0, 1]))
                ev = evaluate(T[p:p + 1, c:c + 1], one, np.ones(1, np.int32))[:4]
                ps = np.array([e["error"][0, 0] for e in ev])
                if not apart[p] or (np.isfinite(ps).all() and (np.abs(ps - ERR2) > MARGIN * ERR2).all()):
                    break
                dropped += 1
            level[p, c] = lv
            k += 1
    if dropped > 0.05 * draws:
        raise SystemExit("%d of %d draws dropped: change SEED" % (dropped, draws))

    a, b, al, bl, logged = evaluate(T, bm, result_flag)
    took = (listed & apart & (result_flag != 0))[:, None] & np.ones((1, N), bool)
    for x, y in ((a, b), (al, bl), (a, al)):
        assert np.array_equal(x["flags"], y["flags"]) and np.array_equal(x["figures"], y["figures"]), "a flag depends on the inversion method"
    for e in (a, b, al, bl):
        assert np.isfinite(e["error"]).all() and (np.abs(e["error"][took] - ERR2) > MARGIN * ERR2).all() and (e["error"][~took] == 0).all()
    rel = lambda x, y: float(np.max(np.abs(x["error"][took] - y["error"][took]) / np.abs(y["error"][took])))
    rel_diff = max(rel(a, b), rel(al, bl))
    good, bad, fpos, gtn, rsn = a["figures"][0, 0].tolist()
    print("%d pairs, %d listed (%d consecutive), %d evaluated per column; column 0: good %d bad %d false_pos %d gt_num %d rs_num %d"
          % (P, listed.sum(), (listed & ~apart).sum(), took[:, 0].sum(), good, bad, fpos, gtn, rsn))
    print("draws %d, dropped %d; largest relative |(a) - (b)| %.3e; closest p to err2: %.3e relative"
          % (draws, dropped, rel_diff, float(np.min(np.abs(a["error"][took] - ERR2)) / ERR2)))
    assert 0 < good < gtn and bad > 0 and fpos == 5 and gtn == (listed & apart).sum() and rsn == gtn - 3 + 5

    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()
    np.savez_compressed(
        OUT, scene=np.array(SCENE), fragments=np.int32(FRAGMENTS), seed=np.int32(SEED), err2=np.float64(ERR2), margin=np.float64(MARGIN),
        T=T, logged=logged, level=level, result_flag=result_flag, p_a=a["error"], p_b=b["error"], p_a_logged=al["error"],
        p_b_logged=bl["error"], flags=a["flags"], figures=a["figures"], rel_diff=np.float64(rel_diff), tol=np.float64(4 * rel_diff),
        draws=np.int32(draws), dropped=np.int32(dropped), numpy_version=np.array(np.__version__),
        sha256_gt_info=np.array(sha(INFO)), sha256_m_files=np.array([sha(os.path.join(REF, f)) for f in M_FILES]))
    # a manifest of its own: tests/golden/MANIFEST.json belongs to the geometry and network generators
    man = dict(generated_by="tools/make_golden_recall.py", files={os.path.basename(f): sha(f) for f in (OUT, INFO)}, seed=SEED, draws=draws,
               dropped=dropped, rel_diff_a_b=rel_diff, tol=4 * rel_diff, err2=ERR2, margin=MARGIN,
               reference_sources={f: sha(os.path.join(REF, f)) for f in M_FILES})
    with open(MANIFEST, "w") as f:
        json.dump(man, f, indent=1)
    print("wrote %s (%d bytes), %s (%d bytes) and %s" % (OUT, os.path.getsize(OUT), INFO, os.path.getsize(INFO), MANIFEST))


if __name__ == "__main__":
    main()
