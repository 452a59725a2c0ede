"""Writes tests/golden/training_pairs.npz: data only, a few kB.

1. The reference's own rotate() (datasets/ThreeDMatch.py:24-45), imported UNMODIFIED from /root/reference with the numpy stand-in for
   TensorFlow (oracle/tf_eager) and an empty module named open3d on the path, run with np.random.rand / np.random.randint patched to
   return the definition's draws (tests/training_pairs_np.rotation_draws).  Recorded: the input points, the draws, the results for
   num_axis 1 and 3.  It pins R and the `points @ R` convention of the restatement.
2. One pair under a GENERAL rotation, whose seed is searched so that, in the fp32 metric, NO d2 lies within 1e-4 relative of r2 and no
   two unequal d2 of one row's matches lie within 1e-4 relative of each other: fp32, float64 and a KD-tree then agree about every
   match and every order.  The condition is checked here, on the CPU, and recorded.

    python tools/make_golden_training_pairs.py          # needs /root/reference
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "training_pairs.npz")
sys.path[:0] = [os.path.join(ROOT, "tests")]
import training_pairs_cases as tc  # noqa: E402
import training_pairs_np as tp  # noqa: E402

ROTATE_CASES = [(3, 0, 0, 0, 1), (3, 0, 0, 1, 1), (9, 4, 2, 0, 1), (9, 4, 2, 1, 3), (1, 7, 5, 0, 3), (12, 1, 9, 1, 1)]   # seed, step, pair, side, mode


def reference_rotate():
    sys.path[:0] = [os.path.join(ROOT, "oracle", "tf_eager"), REF]
    for name in ("open3d", "cpp_wrappers", "cpp_wrappers.cpp_subsampling", "cpp_wrappers.cpp_subsampling.grid_subsampling"):
        sys.modules[name] = types.ModuleType(name)
    for name in ("datasets", "kernels", "models", "utils"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, name)]
        sys.modules[name] = m
    from datasets.ThreeDMatch import rotate
    return rotate


def run_rotate(rotate, points, draws, mode):
    """rotate() with rand() answering theta / (2 pi)'s draw u and randint(3) answering the axis, in the order it asks."""
    us = [u for u, _ in draws]
    axes = [a for _, a in draws]
    rand, randint = np.random.rand, np.random.randint
    np.random.rand = lambda *a: us.pop(0)
    np.random.randint = lambda *a, **k: axes.pop(0)
    try:
        return rotate(points.copy(), num_axis=mode)
    finally:
        np.random.rand, np.random.randint = rand, randint


def general_pair():
    """-> (seed, anchor, positive, T, edge margin, row margin): the first seed that leaves no excluded row."""
    radius = 0.45
    for seed in range(10000):
        rng = np.random.default_rng(1000 + seed)
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = q.astype(np.float32)
        T[:3, 3] = rng.uniform(-3, 3, 3).astype(np.float32)
        positive = (rng.random((260, 3)) * [3.0, 2.5, 0.8]).astype(np.float32)
        a = (rng.random((240, 3)) * [3.0, 2.5, 0.8])
        anchor = ((a - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)).astype(np.float32)
        edge, row = tc.margins(anchor, positive, T, radius)
        if edge > 1e-4 and row > 1e-4:
            return seed, anchor, positive, T, edge, row, radius
    raise SystemExit("no seed leaves every decision a margin of 1e-4")


def main():
    out = {}
    try:
        rotate = reference_rotate()
        out["rotate_source"] = np.asarray("datasets/ThreeDMatch.py:24-45 of the reference, unmodified, under oracle/tf_eager")
    except Exception as e:  # noqa: BLE001
        raise SystemExit("datasets/ThreeDMatch.py does not import here (%s: %s)" % (type(e).__name__, e))
    rng = np.random.default_rng(41)
    pts = (rng.random((24, 3)) * 4 - 2).astype(np.float32)
    out["rotate_points"] = pts
    out["rotate_cases"] = np.asarray(ROTATE_CASES, np.int64)
    for c, (seed, step, pair, side, mode) in enumerate(ROTATE_CASES):
        draws = tp.rotation_draws(seed, step, pair, side, mode)
        # rotate() computes theta = rand() * 2 * pi itself: hand it u
        us = [(float(int(tp.draw(seed, step, pair, tp.STREAM_ROTATION + side, 2 * d)) >> 11) * 2.0 ** -53, a) for d, (_, a) in enumerate(draws)]
        res = run_rotate(rotate, pts, us, mode)
        out["rotate_u_%d" % c] = np.asarray([u for u, _ in us], np.float64)
        out["rotate_axis_%d" % c] = np.asarray([a for _, a in us], np.int64)
        out["rotate_result_%d" % c] = np.asarray(res)
    seed, anchor, positive, T, edge, row, radius = general_pair()
    out.update(general_seed=np.asarray(seed), general_anchor=anchor, general_positive=positive, general_trans=T,
               general_radius=np.asarray(radius, np.float64), general_margins=np.asarray([edge, row]), general_excluded_rows=np.asarray(0))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes): rotate() on %d cases, general pair seed %d, margins %.2e / %.2e" %
          (OUT, os.path.getsize(OUT), len(ROTATE_CASES), seed, edge, row))


if __name__ == "__main__":
    main()
