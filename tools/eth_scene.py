#!/usr/bin/env python3
"""The evaluation half of the ETH test on the GPU: what geometric_registration_eth/evaluate_eth.py computes pair by pair and scene by
scene on the host, from the descriptor files a generate_descriptor run already wrote, in ONE registration.match_scenes call.

    python tools/eth_scene.py --desc-root geometric_registration/D3Feat_xxx-pred --root data/ETH [--counts 250] [--desc-name D3Feat]

Reads `<desc-root>/keypoints/<scene>/cloud_bin_<k>.npy` and `<desc-root>/descriptors/<scene>/cloud_bin_<k>.<desc-name>.npy` (rows in
ascending score order) of the scenes present under --root and `<root>/<scene>/gt.log`; the descriptors go to the device as they are
(NaN and all: np.nan_to_num is the first launch of the call).  Prints the lines of evaluate_eth.py:158-177 for the first count and one
JSON line.  A scene's fragments are cloud_bin_0 .. cloud_bin_<n - 1>: the scans in the order of datasets.eth.scene_scans.
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def load_blocks(desc_root, scenes, num_keypts, desc_name="D3Feat"):
    """-> (blocks, blocks per scene): f32[k, 3 + C + 1] record blocks, the last num_keypts rows of every file, the descriptors
    untouched; the score column carries the row number (ascending as the scores are)."""
    blocks, per_scene = [], []
    for scene in scenes:
        kdir, ddir = os.path.join(desc_root, "keypoints", scene), os.path.join(desc_root, "descriptors", scene)
        ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"cloud_bin_(\d+)\.npy", f) for f in os.listdir(kdir)) if m)
        if not ids or ids != list(range(len(ids))):
            raise SystemExit("%s: fragments %s are not cloud_bin_0 .. cloud_bin_%d" % (kdir, ids[:5], len(ids) - 1))
        for k in ids:
            xyz = np.load(os.path.join(kdir, "cloud_bin_%d.npy" % k))[-num_keypts:]
            desc = np.load(os.path.join(ddir, "cloud_bin_%d.%s.npy" % (k, desc_name)))[-num_keypts:]
            blocks.append(np.concatenate([xyz, desc, np.arange(len(xyz), dtype=np.float32)[:, None]], 1).astype(np.float32))
        per_scene.append(len(ids))
    return blocks, per_scene


def evaluate(blocks, per_scene, gt_logs, counts=(250,), distance_threshold=0.10, inlier_ratio=0.05, device=None):
    """blocks: host or device record blocks of all scenes, per_scene: how many belong to each scene, gt_logs: per scene a path, a dict
    or None -> registration.SceneMatches of ONE match_scenes call."""
    import torch
    from d3feat_amd import registration as reg
    from d3feat_amd.datasets import eth
    dev = device if device is not None else torch.device("cuda", 0)
    kp, count = reg.stack_keypoints(blocks, max(counts), device=dev)
    pairs, gt, flag, scene_start = eth.benchmark(per_scene, gt_logs)
    return reg.match_scenes(kp, count, torch.from_numpy(pairs).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(flag).to(dev),
                            scene_start, num_keypts=counts, distance_threshold=distance_threshold, inlier_ratio=inlier_ratio)


def report(scenes, counts, out):
    from d3feat_amd.utils import results
    print("\n".join(results.eth_lines(scenes, out.summary)))
    per = out.summary.scenes()
    print(json.dumps(dict(scenes=list(scenes), pairs=out.summary.P, num_keypts=list(counts),
                          recall=[[r["recall"] for r in s] for s in per], correct=[[r["correct"] for r in s] for s in per],
                          gt=[[r["gt"] for r in s] for s in per], overall=[out.summary.overall(c) for c in range(len(counts))])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--desc-root", required=True)
    ap.add_argument("--root", default="data/ETH")
    ap.add_argument("--counts", default="250", help="comma-separated keypoint counts, ascending")
    ap.add_argument("--desc-name", default="D3Feat")
    ap.add_argument("--inlier-ratio", type=float, default=0.05)
    ap.add_argument("--distance-threshold", type=float, default=0.10)
    a = ap.parse_args()
    from d3feat_amd.datasets import eth
    counts = tuple(int(c) for c in a.counts.split(","))
    scenes = [s for s in eth.SCENES if os.path.isdir(os.path.join(a.desc_root, "keypoints", s))]
    if not scenes:
        raise SystemExit("%s/keypoints holds none of the ETH scenes" % a.desc_root)
    blocks, per_scene = load_blocks(a.desc_root, scenes, max(counts), a.desc_name)
    out = evaluate(blocks, per_scene, [os.path.join(a.root, s, "gt.log") for s in scenes], counts, a.distance_threshold, a.inlier_ratio)
    report(scenes, counts, out)


if __name__ == "__main__":
    main()
