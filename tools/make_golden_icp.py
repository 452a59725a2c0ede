#!/usr/bin/env python
"""Writes tests/golden/icp.npz: the seeded golden pair of the ICP tests, what the float64 restatement (tests/icp_np.py) makes of it,
the margins of that run, and the largest difference of the transform between the two fit formulations (eigh of Horn's matrix, as
rg_horn states it, against SVD-Kabsch).

    python tools/make_golden_icp.py [--seed 7]
    python tools/make_golden_icp.py --sweep          (needs scipy)

The golden pair: 2000 source rows on three noisy planes; the target is a permuted copy thinned by 30 %, rotated by about one degree
and shifted by 0.08 m.  A case whose margin (nearest against second-nearest d2, any d2 against r r, the stop test against its
thresholds) is below 1e-9 is REFUSED: above it a last-bit difference in T -- Jacobi on the device, LAPACK here -- cannot flip a
correspondence or the stop test, so both walk the same sequence of rounds.  Open3D is not involved: what the fixture pins is the
definition of include/d3feat_amd.h.

--sweep writes tests/golden/icp_sweep.npz instead: two pairs at sweep size (tests/icp_cases.py sweep_pairs: tools/icp_bench.py's
recipe at 66 000 points, 258 chunks of source rows, the target thinned to 20 000 rows over 160 x 160 x 9.6 m, so that the grid's cells
come out at eight radii) run to convergence by the restatement with scipy's k-d tree as the nearest search.  The clouds are NOT stored:
the fixture holds the recipe's parameters and a SHA-256 per pair of the bytes of src, tgt and init, which the tests check against the
inputs they regenerate; then per pair T, count, sumd2, fitness, rmse, iterations, converged, nearest, the three margins and the
difference between the two fit formulations.  The same refusals apply.  The archive is written with fixed member dates, so that the
same inputs give the same file byte for byte.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases  # noqa: E402
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


def save_npz_reproducibly(path, arrays):
    """numpy.savez_compressed with every member dated 1980-01-01: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def sweep(out_path):
    pairs = icp_cases.sweep_pairs()
    kw = dict(KW, nearest=icp_np.nearest_ckdtree)
    runs = []
    for p, (src, tgt, init) in enumerate(pairs):
        a = icp_np.icp(src, tgt, init, fit="eigh", **kw)
        b = icp_np.icp(src, tgt, init, fit="svd", **kw)              # a prerequisite: the fit difference, and the same sequence of rounds
        margins = np.array([a.margin_nn, a.margin_r, a.margin_stop])
        if not np.all(margins >= MARGIN) or a.iterations != b.iterations or not np.array_equal(a.nearest, b.nearest):
            raise SystemExit("refused: pair %d, margins %s below %g, or the two fits walk different sequences" % (p, margins, MARGIN))
        a.margins, a.fit_difference = margins, float(np.max(np.abs(a.T - b.T)))
        print("pair %d: rows %d / %d iterations %d converged %d count %d fitness %.6f rmse %.3e margins %s fit difference %.3e"
              % (p, len(src), len(tgt), a.iterations, a.converged, a.count, a.fitness, a.rmse, margins, a.fit_difference))
        runs.append(a)
    out = {"recipe_" + k: np.float64(v) if isinstance(v, float) else np.int64(v) for k, v in icp_cases.SWEEP.items()}
    out.update({"kw_" + k: np.float64(v) for k, v in KW.items()})
    out["sha256"] = np.array([icp_cases.pair_sha256(p) for p in pairs])
    out["src_rows"] = np.array([len(p[0]) for p in pairs], np.int64)
    out["tgt_rows"] = np.array([len(p[1]) for p in pairs], np.int64)
    out["T"] = np.stack([r.T for r in runs])
    for k, dt in (("count", np.int64), ("sumd2", np.float64), ("fitness", np.float64), ("rmse", np.float64), ("iterations", np.int64),
                  ("converged", np.int64), ("fit_difference", np.float64)):
        out[k] = np.array([getattr(r, k) for r in runs], dt)
    out["margins"] = np.stack([r.margins for r in runs])
    out["nearest"] = np.stack([r.nearest.astype(np.int32) for r in runs])
    save_npz_reproducibly(out_path, out)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sweep", action="store_true", help="write tests/golden/icp_sweep.npz, the two pairs at sweep size")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.sweep:
        return sweep(args.out or os.path.join(ROOT, "tests", "golden", "icp_sweep.npz"))
    args.out = args.out or os.path.join(ROOT, "tests", "golden", "icp.npz")
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
