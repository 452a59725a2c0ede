#!/usr/bin/env python
"""Writes tests/golden/icp.npz: the seeded golden pair of the ICP tests, what the float64 restatement (tests/icp_np.py) makes of it,
the margins of that run, and the largest difference of the transform between the two fit formulations (eigh of Horn's matrix, as
rg_horn states it, against SVD-Kabsch).

    python tools/make_golden_icp.py [--seed 7]

The golden pair: 2000 source rows on three noisy planes; the target is a permuted copy thinned by 30 %, rotated by about one degree
and shifted by 0.08 m.  A case whose margin (nearest against second-nearest d2, any d2 against r r, the stop test against its
thresholds) is below 1e-9 is REFUSED: above it a last-bit difference in T -- Jacobi on the device, LAPACK here -- cannot flip a
correspondence or the stop test, so both walk the same sequence of rounds.  Open3D is not involved: what the fixture pins is the
definition of include/d3feat_amd.h.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_np  # noqa: E402

MARGIN = 1e-9
KW = dict(max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6, relative_rmse=1e-6)


def golden_pair(seed):
    rng = np.random.default_rng(seed)
    n = 2000
    uv = rng.uniform(0.0, 2.0, (n, 2))
    noise = rng.normal(0.0, 0.01, n)
    plane = np.arange(n) % 3
    pts = np.empty((n, 3))
    pts[plane == 0] = np.stack([uv[:, 0], uv[:, 1], noise], 1)[plane == 0]
    pts[plane == 1] = np.stack([noise, uv[:, 0], uv[:, 1]], 1)[plane == 1]
    pts[plane == 2] = np.stack([uv[:, 0], noise, uv[:, 1]], 1)[plane == 2]
    src = (pts + np.array([3.0, -2.0, 1.0])).astype(np.float32)
    keep = rng.permutation(n)[: int(0.7 * n)]
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(1.0)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    c = src.astype(np.float64).mean(0)
    shift = 0.08 * np.array([0.6, 0.64, -0.48])
    tgt = ((src[keep].astype(np.float64) - c) @ R.T + c + shift).astype(np.float32)
    return src, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "icp.npz"))
    args = ap.parse_args()
    src, tgt = golden_pair(args.seed)
    out = dict(src=src, tgt=tgt, seed=np.int64(args.seed), **{"kw_" + k: np.float64(v) for k, v in KW.items()})
    for tag, kw in (("", KW), ("it3_", dict(KW, max_iteration=3))):
        a = icp_np.icp(src, tgt, None, fit="eigh", **kw)
        b = icp_np.icp(src, tgt, None, fit="svd", **kw)
        margins = np.array([a.margin_nn, a.margin_r, a.margin_stop])
        if not np.all(margins >= MARGIN) or a.iterations != b.iterations or not np.array_equal(a.nearest, b.nearest):
            raise SystemExit("refused: margins %s below %g, or the two fits walk different sequences -- try another --seed" % (margins, MARGIN))
        print("%scase: iterations %d converged %d count %d fitness %.6f rmse %.3e margins %s fit difference %.3e"
              % (tag, a.iterations, a.converged, a.count, a.fitness, a.rmse, margins, np.max(np.abs(a.T - b.T))))
        out.update({tag + "T": a.T, tag + "count": np.int64(a.count), tag + "sumd2": np.float64(a.sumd2), tag + "fitness": np.float64(a.fitness),
                    tag + "rmse": np.float64(a.rmse), tag + "iterations": np.int64(a.iterations), tag + "converged": np.int64(a.converged),
                    tag + "nearest": a.nearest.astype(np.int32), tag + "margins": margins,
                    tag + "fit_difference": np.float64(np.max(np.abs(a.T - b.T)))})
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
