#!/usr/bin/env python3
"""What does the ICP refinement of KITTI-sized pairs cost in one device call?  (One process, one GPU; not bench.py.)

Workload: 16 synthetic pairs of 120 k-point sweeps (utils.synthetic.lidar_sweep; the target is the sweep moved rigidly, jittered by
1 cm and permuted; the init is off by about 0.1 m and 0.3 degrees, as an odometry pose is), with icp.ICP_KITTI.  The two forms of the
call are alternated inside the same run, nine windows each, wall clock around call + synchronise, the clouds already on the device:

  (a) check_every = 8: the host looks every 8 rounds whether every pair has stopped;
  (b) check_every = 0: max_iteration + 1 rounds enqueued, no read-back.

Before any timing the two are compared bit for bit.  When scipy imports, the float64 restatement (tests/icp_np.py) with
scipy.spatial.cKDTree as the nearest search runs on two of the pairs: its results are compared (integers equal, T within 1e-9) and its
time per pair is recorded next to the device's.  No time is a pass / fail condition.

    python tools/icp_bench.py [--out profiles/icp_bench.json] [--pairs 16] [--points 120000] [--windows 9]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from d3feat_amd import icp
from d3feat_amd.utils.synthetic import lidar_sweep


def rigid(rng, deg, shift):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    d = rng.normal(size=3)
    T[:3, 3] = shift * d / np.linalg.norm(d)
    return T


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(float(t.min()) * 1e3, 3), "max_ms": round(float(t.max()) * 1e3, 3),
            "ms_per_pair_median": round(float(np.median(t)) * 1e3 / pairs, 3), "windows_ms": [round(float(x) * 1e3, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--host-pairs", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    srcs, tgts, inits = [], [], []
    for p in range(a.pairs):
        s = lidar_sweep(100 + p, n_raw=a.points)
        G = rigid(rng, 2.0, 10.0)                                        # the pair's true motion: 10 m on, as the test split's pairs
        t = (s.astype(np.float64) @ G[:3, :3].T + G[:3, 3] + rng.normal(scale=0.01, size=s.shape)).astype(np.float32)
        srcs.append(s)
        tgts.append(t[rng.permutation(len(t))])
        inits.append(rigid(rng, 0.3, 0.1) @ G)
    sl, tl = [len(s) for s in srcs], [len(t) for t in tgts]
    src, tgt = torch.from_numpy(np.concatenate(srcs)).to(dev), torch.from_numpy(np.concatenate(tgts)).to(dev)
    init = torch.from_numpy(np.stack(inits)[:, :3].reshape(-1, 12).copy()).to(dev)
    sl_d, tl_d = torch.tensor(sl, dtype=torch.int32, device=dev), torch.tensor(tl, dtype=torch.int32, device=dev)
    sl_d.host_lens, tl_d.host_lens = sl, tl

    def call(every):
        r = icp.icp_pairs(src, sl_d, tgt, tl_d, init=init, check_every=every, **icp.ICP_KITTI)
        torch.cuda.synchronize(dev)
        return r

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    r8, r0 = call(8), call(0)
    same = all(torch.equal(r8.dev[k], r0.dev[k]) for k in r8.dev)
    times = {"check_every_8": [], "check_every_0": []}
    for w in range(a.windows):
        times["check_every_8"].append(wall(lambda: call(8)))
        times["check_every_0"].append(wall(lambda: call(0)))
        print("window %d: check_every 8 %.1f ms, 0 %.1f ms" % (w, *(times[k][-1] * 1e3 for k in times)), file=sys.stderr, flush=True)
    out = {"pairs": a.pairs, "points_per_sweep": a.points, "parameters": dict(icp.ICP_KITTI), "windows": a.windows,
           "timing": "the two forms alternated, %d windows each; wall clock around call + synchronise, grid build included, clouds on the "
                     "device" % a.windows,
           "forms_equal": bool(same), "iterations": r8.iterations.tolist(), "converged": r8.converged.astype(int).tolist(),
           "fitness": [round(float(x), 6) for x in r8.fitness], "inlier_rmse": [round(float(x), 6) for x in r8.inlier_rmse]}
    for k, t in times.items():
        out[k] = stats(t, a.pairs)
    try:
        import scipy.spatial  # noqa: F401
        import icp_np
    except ImportError:
        out["host"] = "scipy is not installed: the cKDTree restatement was not run"
    else:
        host_t, agree = [], True
        T_dev = r8.transformation
        for p in range(min(a.host_pairs, a.pairs)):
            t0 = time.perf_counter()
            h = icp_np.icp(srcs[p], tgts[p], inits[p], nearest=icp_np.nearest_ckdtree, **icp.ICP_KITTI)
            host_t.append(time.perf_counter() - t0)
            agree = agree and h.iterations == int(r8.iterations[p]) and h.count == int(r8.count[p]) and \
                float(np.max(np.abs(h.T - T_dev[p]))) <= 1e-9
        out["host"] = {"what": "tests/icp_np.py with scipy.spatial.cKDTree, one core, %d pairs" % len(host_t),
                       "s_per_pair": [round(x, 3) for x in host_t], "agrees_with_device": bool(agree)}
        out["host_over_device_per_pair"] = round(float(np.median(host_t)) / (float(np.median(times["check_every_8"])) / a.pairs), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if not same:
        raise SystemExit("the two check_every forms differ")


if __name__ == "__main__":
    main()
