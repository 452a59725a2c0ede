#!/usr/bin/env python3
"""The ETH generalisation test of the reference (test_eth.py + geometric_registration_eth/evaluate_eth.py) on the engine path of an
MI355X: a 3DMatch-trained model on the four outdoor scenes at first_subsampling_dl = 0.05 and KP_extent = 2, feature-matching recall
at 250 keypoints.

    python tools/eth_test.py --root data/ETH --weights results/Log_xxx [--counts 250,...] [--out DIR]

Every scan (datasets.eth.scene_scans, voxelised at 0.0625 m by datasets.eth.read_scan) goes through FragmentEngine(stage0=False,
keypoints=max count) stacked with itself, as the reference's generator feeds it; the best records stay on the device.  After the last
scan ONE registration.match_scenes call sanitises the descriptors, matches every pair of every scene and summarises the scenes; the
lines of evaluate_eth.py:158-177 are printed (results.eth_lines).  --out DIR additionally writes the reference's keypoint / descriptor
/ score files (results.save_3dmatch_keypoints).  The engine's capacities are sized from the scans themselves.
--weights: a training folder (parameters.txt if present, the highest snapshots/snap-N) or a checkpoint prefix.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3feat_amd import _lib, registration as reg  # noqa: E402
from d3feat_amd.datasets import eth  # noqa: E402
from d3feat_amd.datasets.common import FragmentDataset  # noqa: E402
from d3feat_amd.engine import FragmentEngine  # noqa: E402
from d3feat_amd.utils import results  # noqa: E402
from d3feat_amd.utils.config import Config, threedmatch_config  # noqa: E402
from d3feat_amd.utils.tf_checkpoint import load_checkpoint  # noqa: E402


def load_model(path):
    """-> (config with datasets.eth.apply_config applied, weights)"""
    cfg, prefix = threedmatch_config(), path
    if os.path.isdir(path):
        if os.path.exists(os.path.join(path, "parameters.txt")):
            cfg = Config()
            cfg.load(path)
        snaps = glob.glob(os.path.join(path, "snapshots", "snap-*.index"))
        if not snaps:
            raise SystemExit("%s holds no snapshots/snap-N" % path)
        prefix = max(snaps, key=lambda p: int(p[:-len(".index")].rsplit("-", 1)[1]))[:-len(".index")]
    return eth.apply_config(cfg), load_checkpoint(prefix)


def extract(scans, cfg, weights, num_keypts, device, slots=2, limits=None):
    """scans: f32[n, 3] host arrays already at 0.0625 m -> (list of device f32[min(n, num_keypts), 36] record blocks in ascending score
    order, the engine).  The neighbourhood limits are calibrated on the scans (init_test_input_pipeline) unless given."""
    if limits is None:
        ds = FragmentDataset(scans)
        ds.init_test_input_pipeline(cfg)
        limits = ds.neighborhood_limits
    n0 = max(len(s) for s in scans)
    eng = FragmentEngine(cfg, weights, limits, n0_cap=(int(n0 * 1.05) + 1023) // 1024 * 1024, level_ratio=0.6,
                         slots=min(slots, len(scans)), device=device, stage0=False, keypoints=num_keypts)
    # KP_extent = 2 doubles every search radius: up to eight times the supports of a 3DMatch query, more than the fast ordering budget
    # holds.  The engine raises the budget by itself after two replays overflowed (two scans through the eager path); the test knows
    # from the start, so every slot is captured again with the full budget at its first submit.
    eng.neighbor_cap = eng._eager_ds._neighbor_cap = _lib.NEIGHBOR_CAP
    S, blocks, pending = len(eng.slots), [None] * len(scans), {}
    for i, scan in enumerate(scans):
        k = i % S
        if k in pending:
            blocks[pending.pop(k)] = eng.fetch(k, keypoints=True).clone()
        eng.submit(k, torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32)).to(device))
        pending[k] = i
    for k, i in pending.items():
        blocks[i] = eng.fetch(k, keypoints=True).clone()
    return blocks, eng


def run(scans_per_scene, gt_logs, cfg, weights, counts=reg.EVALUATE_ETH["num_keypts"], device=None, limits=None):
    """scans_per_scene: per scene the list of its scans (0.0625 m, in scene_scans order); gt_logs: per scene a path, a dict or None.
    -> (registration.SceneMatches, the record blocks of all scans, the engine)"""
    from eth_scene import evaluate
    dev = device if device is not None else torch.device("cuda", 0)
    scans = [s for scene in scans_per_scene for s in scene]
    blocks, eng = extract(scans, cfg, weights, max(counts), dev, limits=limits)
    return evaluate(blocks, [len(s) for s in scans_per_scene], gt_logs, counts, device=dev), blocks, eng


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default="data/ETH")
    ap.add_argument("--weights", required=True)
    ap.add_argument("--counts", default="250", help="comma-separated keypoint counts, ascending")
    ap.add_argument("--out", default=None, help="write the reference's keypoints / descriptors / scores files here")
    a = ap.parse_args()
    from eth_scene import report
    counts = tuple(int(c) for c in a.counts.split(","))
    cfg, weights = load_model(a.weights)
    scenes = [s for s in eth.SCENES if os.path.isdir(os.path.join(a.root, s))]
    if not scenes:
        raise SystemExit("%s holds none of the ETH scenes %s" % (a.root, list(eth.SCENES)))
    paths = [eth.scene_scans(a.root, s) for s in scenes]
    scans = [[eth.read_scan(p) for p in ps] for ps in paths]
    print("Num_test", sum(len(s) for s in scans))
    out, blocks, eng = run(scans, [os.path.join(a.root, s, "gt.log") for s in scenes], cfg, weights, counts)
    if a.out:
        i = 0
        for s, ps in zip(scenes, paths):
            for k in range(len(ps)):                                   # evaluate_eth.py names the fragments by position
                results.save_3dmatch_keypoints(a.out, "%s/cloud_bin_%d.ply" % (s, k), blocks[i].cpu().numpy())
                i += 1
    report(scenes, counts, out)
    print("%d scans, %d took the eager path" % (sum(len(s) for s in scans), eng.fallbacks))


if __name__ == "__main__":
    main()
