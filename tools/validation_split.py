#!/usr/bin/env python3
"""The validation figures of a split on an MI355X: what utils/trainer.py:417-498 of the reference prints after an epoch, for a
checkpoint trained elsewhere.

    python tools/validation_split.py --points 3DMatch_val_0.030_points.pkl --keypts 3DMatch_val_0.030_keypts.pkl
                                     --weights results/Log_xxx [--kitti] [--epoch N] [--seed S] [--limits a,b,c,d,e]

The split is read the way datasets/ThreeDMatch.py:101-136 reads it ({id: cloud} and {'anc@pos': correspondences [m, 2]}), and pairs
are drawn the way its generator draws them (:188-229): per anchor the first positive or a random one, clouds outside 2000 .. 80000
points skipped, keypts_num correspondences sampled with replacement, the positive's indices shifted by the anchor's length.  The
clouds are already at first_subsampling_dl, so every pair goes through FragmentEngine(two_clouds=True, stage0=False) as it is and
the packed records of all pairs are evaluated by validation_records in one call per 64 pairs.  The generator's augmentations
(noise, rotation) are random and not applied; --seed fixes the draws.
--weights: a training folder (parameters.txt if present, the highest snapshots/snap-N) or a checkpoint prefix.
"""
import argparse
import glob
import os
import pickle
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3feat_amd.datasets.common import FragmentDataset  # noqa: E402
from d3feat_amd.engine import FragmentEngine  # noqa: E402
from d3feat_amd.utils.config import Config, kitti_config, threedmatch_config  # noqa: E402
from d3feat_amd.utils.tf_checkpoint import load_checkpoint  # noqa: E402
from d3feat_amd.validation import VALIDATION_3DMATCH, VALIDATION_KITTI, format_line, split_means, validation_records  # noqa: E402

CHUNK = 64


def draw_pairs(points, keypts, keypts_num):
    """datasets/ThreeDMatch.py:122-129, 188-229 -> [(anchor cloud, positive cloud, anc_keypts, pos_keypts)]."""
    anc_to_pos = {}
    for idpair in keypts.keys():
        anc, pos = idpair.split("@")[0], idpair.split("@")[1]
        anc_to_pos.setdefault(anc, []).append(pos)
    out = []
    for p_i in np.random.permutation(len(anc_to_pos)):
        anc_id = list(anc_to_pos.keys())[p_i]
        pos_id = anc_to_pos[anc_id][0] if random.random() > 0.5 else random.choice(anc_to_pos[anc_id])
        a = np.ascontiguousarray(points[anc_id], dtype=np.float32)
        b = np.ascontiguousarray(points[pos_id], dtype=np.float32)
        if a.shape[0] > 80000 or b.shape[0] > 80000 or a.shape[0] < 2000 or b.shape[0] < 2000:
            continue
        corr = np.asarray(keypts["%s@%s" % (anc_id, pos_id)])
        sel = np.random.choice(len(corr), keypts_num, replace=True)
        out.append((a, b, corr[sel, 0].astype(np.int32), (corr[sel, 1] + len(a)).astype(np.int32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", required=True)
    ap.add_argument("--keypts", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--kitti", action="store_true")
    ap.add_argument("--epoch", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keypts-num", type=int, default=None, help="default: the data set's (256 / 1024)")
    ap.add_argument("--limits", default=None, help="neighbourhood limits per layer; default: calibrated on the split")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = kitti_config() if args.kitti else threedmatch_config()
    prefix = args.weights
    if os.path.isdir(args.weights):
        if os.path.exists(os.path.join(args.weights, "parameters.txt")):
            cfg = Config()
            cfg.load(args.weights)
        snaps = glob.glob(os.path.join(args.weights, "snapshots", "snap-*.index"))
        if not snaps:
            raise SystemExit("%s holds no snapshots/snap-N" % args.weights)
        prefix = max(snaps, key=lambda p: int(p[:-len(".index")].rsplit("-", 1)[1]))[:-len(".index")]
    weights = load_checkpoint(prefix)
    par = dict(VALIDATION_KITTI if args.kitti else VALIDATION_3DMATCH)
    if args.keypts_num is not None:
        par["keypts_num"] = args.keypts_num
    np.random.seed(args.seed)
    random.seed(args.seed)
    with open(args.points, "rb") as f:
        points = pickle.load(f)
    with open(args.keypts, "rb") as f:
        keypts = pickle.load(f)
    pairs = draw_pairs(points, keypts, par["keypts_num"])
    if not pairs:
        raise SystemExit("no pair of the split passes the generator's size rule (2000 .. 80000 points)")
    if args.limits:
        limits = np.asarray([int(v) for v in args.limits.split(",")], np.int32)
    else:
        ds = FragmentDataset([p[0] for p in pairs[:16]])
        ds.init_test_input_pipeline(cfg)
        limits = ds.neighborhood_limits
    cap = int(max(len(a) + len(b) for a, b, _, _ in pairs) * 1.05) + 1024
    eng = FragmentEngine(cfg, weights, limits, n0_cap=cap, slots=1, device=dev, two_clouds=True, stage0=False)
    sums, counts = np.zeros(6), np.zeros(6, np.int64)
    for c0 in range(0, len(pairs), CHUNK):
        chunk = pairs[c0:c0 + CHUNK]
        recs, lens = [], []
        for a, b, _, _ in chunk:
            eng.submit(0, (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
            recs.append(eng.fetch(0, packed=True).clone())
            lens += [len(a), len(b)]
        anc = torch.from_numpy(np.stack([p[2] for p in chunk])).to(dev)
        pos = torch.from_numpy(np.stack([p[3] for p in chunk])).to(dev)
        out = validation_records(torch.cat(recs), lens, anc, pos, **par)
        if out.status.any().item():
            raise SystemExit("a correspondence index lies outside its pair's clouds")
        sums += out.sums.cpu().numpy()
        counts += out.counts.cpu().numpy()
    print("%d pairs, %d took the eager path" % (len(pairs), eng.fallbacks))
    print(format_line(cfg.dataset, args.epoch, split_means(sums, counts)))


if __name__ == "__main__":
    main()
