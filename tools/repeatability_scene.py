#!/usr/bin/env python3
"""Keypoint repeatability of one scene on the GPU, as repeatability/evaluate_3dmatch_our.py computes it pair by pair and count by count
on the host (or, with --kitti, with the convention of repeatability/evaluate_kitti_our.py).

Reads the `keypoints/<scene>/cloud_bin_<k>.npy` files that utils.results.save_3dmatch_keypoints / save_3dmatch_results wrote under
--root (rows in ascending score order), keeps the pairs id1 < id2 that --gt lists (evaluate_3dmatch_our.py:28-29), makes ONE
registration.repeatability_pairs call for all of them at all --counts, prints the lines the reference prints and one JSON line.

    python tools/repeatability_scene.py --root RESULTS --scene sun3d-hotel_umd-maryland_hotel3 --gt gt.log

Default: gt.log takes the target frame into the source frame, the target keypoints are moved, 0.1 m (registration.REPEATABILITY_3DMATCH).
--kitti: the matrices take the source frame into the target frame, the source keypoints are moved, 0.5 m (REPEATABILITY_KITTI).
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def load_scene(root, scene, num_keypts):
    """-> list of f32[k, 4] blocks [xyz | row number], fragment k = cloud_bin_<k> (the row number stands for the score: ascending)."""
    kdir = os.path.join(root, "keypoints", scene)
    ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"cloud_bin_(\d+)\.npy", f) for f in os.listdir(kdir)) if m)
    if ids != list(range(len(ids))) or not ids:
        raise SystemExit("%s: fragments %s are not cloud_bin_0 .. cloud_bin_%d" % (kdir, ids[:5], len(ids) - 1))
    blocks = []
    for k in ids:
        xyz = np.load(os.path.join(kdir, "cloud_bin_%d.npy" % k))[-num_keypts:]
        blocks.append(np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32)[:, None]], 1).astype(np.float32))
    return blocks


def listed_pairs(gt_log, n_frag):
    """The pairs id1 < id2 < n_frag that gt.log lists, in the order of evaluate_3dmatch_our.py:23-29 -> (pairs, f64[P,4,4])."""
    pairs = [(a, b) for a in range(n_frag) for b in range(a + 1, n_frag) if "%d_%d" % (a, b) in gt_log]
    gt = np.stack([gt_log["%d_%d" % p] for p in pairs]) if pairs else np.zeros((0, 4, 4))
    return pairs, gt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--gt", required=True, help="the scene's gt.log (geometric_registration/gt_result/<scene>-evaluation/gt.log)")
    ap.add_argument("--counts", default=None, help="comma-separated keypoint counts, ascending (default: 4,8,...,512)")
    ap.add_argument("--kitti", action="store_true", help="source -> target matrices, the source moved, 0.5 m")
    a = ap.parse_args()
    import torch
    from d3feat_amd import registration as reg
    from d3feat_amd.utils import results
    counts = tuple(int(c) for c in a.counts.split(",")) if a.counts else reg.REPEATABILITY_COUNTS
    dev = torch.device("cuda", 0)
    blocks = load_scene(a.root, a.scene, max(counts))
    pairs, gt = listed_pairs(results.read_gt_log(a.gt), len(blocks))
    if not pairs:
        raise SystemExit("%s lists no pair of the %d fragments" % (a.gt, len(blocks)))
    kp, count = reg.stack_keypoints(blocks, max(counts), device=dev)
    kw = reg.REPEATABILITY_KITTI if a.kitti else reg.REPEATABILITY_3DMATCH
    res = reg.repeatability_pairs(kp, count, torch.tensor(pairs, dtype=torch.int32, device=dev), gt, num_keypts=counts, **kw)
    lines, table = results.repeatability_table(counts, res.scene())
    print("\n".join(lines))
    print(json.dumps(dict(scene=a.scene, fragments=len(blocks), pairs=len(pairs), num_keypts=list(counts),
                          repeatability=[table[k] for k in counts], **kw)))


if __name__ == "__main__":
    main()
