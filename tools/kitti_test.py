#!/usr/bin/env python3
"""The KITTI test of the reference (test_kitti.py -> utils/tester.py:235-360) on the engine path of an MI355X:

    python tools/kitti_test.py --root data/kitti --weights results_kitti/Log_xxx [--odometry-gt] [--out DIR] [--sequences 8,9,10]

Every test pair (datasets/kitti.test_pairs) goes through FragmentEngine(two_clouds=True, keypoints=250) with several pairs in flight;
the 250 best records of both sweeps stay on the device.  After the last pair ONE registration.register_kitti_pairs call registers and
scores all of them, and the reference's log lines are printed (results.kitti_lines).  --out DIR additionally writes the reference's
per-pair files (results.save_kitti_pair).
Ground truth: <root>/icp/<drive>_<t0>_<t1>.npy, the reference's ICP-refined cache.  ICP is not built here: a pair without its file
stops the run, unless --odometry-gt selects the unrefined odometry transform for such pairs (the figures then differ from the paper's).
--weights: a training folder (parameters.txt if present, the highest snapshots/snap-N) or a checkpoint prefix.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3feat_amd import registration as reg  # noqa: E402
from d3feat_amd.datasets import kitti  # noqa: E402
from d3feat_amd.datasets.common import FragmentDataset  # noqa: E402
from d3feat_amd.engine import FragmentEngine  # noqa: E402
from d3feat_amd.utils import results  # noqa: E402
from d3feat_amd.utils.config import Config, kitti_config  # noqa: E402
from d3feat_amd.utils.tf_checkpoint import load_checkpoint  # noqa: E402

NUM_KEYPTS = 250                                  # tester.py:243


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="data/kitti")
    ap.add_argument("--weights", required=True)
    ap.add_argument("--sequences", default=",".join(str(s) for s in kitti.TEST_SEQUENCES))
    ap.add_argument("--icp-dir", default=None, help="default: <root>/icp")
    ap.add_argument("--odometry-gt", action="store_true", help="pairs without an icp file use the unrefined odometry transform")
    ap.add_argument("--out", default=None, help="write the reference's <anc>-<pos>.npz files here")
    ap.add_argument("--limits", default=None, help="neighbourhood limits per layer; default: calibrated on the first pairs")
    ap.add_argument("--slots", type=int, default=3, help="pairs in flight")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, prefix = kitti_config(), args.weights
    if os.path.isdir(args.weights):
        if os.path.exists(os.path.join(args.weights, "parameters.txt")):
            cfg = Config()
            cfg.load(args.weights)
        snaps = glob.glob(os.path.join(args.weights, "snapshots", "snap-*.index"))
        if not snaps:
            raise SystemExit("%s holds no snapshots/snap-N" % args.weights)
        prefix = max(snaps, key=lambda p: int(p[:-len(".index")].rsplit("-", 1)[1]))[:-len(".index")]
    weights = load_checkpoint(prefix)
    voxel = float(cfg.first_subsampling_dl)
    pairs = kitti.test_pairs(args.root, [int(s) for s in args.sequences.split(",")])
    if not pairs:
        raise SystemExit("no test pair under %s" % args.root)
    # every ground truth before any GPU work: a missing file stops the run here
    gt = np.stack([kitti.pair_transform(args.root, d, t0, t1, icp_dir=args.icp_dir, odometry_gt=args.odometry_gt)[:3] for d, t0, t1 in pairs])
    print("Num_test", len(pairs))
    if args.limits:
        limits = np.asarray([int(v) for v in args.limits.split(",")], np.int32)
    else:
        from d3feat_amd import tf_custom_ops as tfo
        sub = [tfo.grid_subsampling(torch.from_numpy(kitti.read_pair(args.root, *p)[0]).to(dev), voxel).cpu().numpy() for p in pairs[:8]]
        ds = FragmentDataset(sub)
        ds.init_test_input_pipeline(cfg)
        limits = ds.neighborhood_limits
    eng = FragmentEngine(cfg, weights, limits, raw_cap=300000, n0_cap=80000, level_ratio=0.6, slots=args.slots, device=dev,
                         two_clouds=True, keypoints=NUM_KEYPTS)
    P = len(pairs)
    kp = torch.zeros((2 * P, NUM_KEYPTS, 36), dtype=torch.float32, device=dev)
    count = torch.zeros((2 * P,), dtype=torch.int32, device=dev)
    counts_host = np.zeros(2 * P, np.int32)

    def collect(p):
        a, b = eng.fetch(p % args.slots, keypoints=True)
        for c, blk in enumerate((a, b)):
            kp[2 * p + c, :blk.shape[0]].copy_(blk)
            counts_host[2 * p + c] = blk.shape[0]

    t0 = time.time()
    for p, (d, ta, tb) in enumerate(pairs):
        if p >= args.slots:
            collect(p - args.slots)
        a, b = kitti.read_pair(args.root, d, ta, tb)
        eng.submit(p % args.slots, (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    for p in range(max(P - args.slots, 0), P):
        collect(p)
    count.copy_(torch.from_numpy(counts_host))
    torch.cuda.synchronize(dev)
    feat_time = (time.time() - t0) / P
    t0 = time.time()
    out = reg.register_kitti_pairs(kp, count, torch.from_numpy(gt.astype(np.float32)).to(dev), voxel, seed=args.seed)
    h = out.errors.host()
    reg_time = (time.time() - t0) / P
    ids = [("%d@%d" % (d, ta), "%d@%d" % (d, tb)) for d, ta, tb in pairs]
    if args.out:
        T, rec = out.T.cpu().numpy(), kp.cpu().numpy()
        for p, (a, b) in enumerate(ids):
            s, t = rec[2 * p, :counts_host[2 * p]], rec[2 * p + 1, :counts_host[2 * p + 1]]
            results.save_kitti_pair(args.out, a, b, T[p], s[:, :3], t[:, :3], s[:, -1:], t[:, -1:])
    for line in results.kitti_lines([a for a, _ in ids], h["rte"][:, 0], h["rre_deg"][:, 0], h["flags"][:, 0], feat_times=[feat_time] * P,
                                    reg_times=[reg_time] * P, final=out.errors.meters()):
        print(line)
    print("%d pairs, %d took the eager path" % (P, eng.fallbacks))


if __name__ == "__main__":
    main()
