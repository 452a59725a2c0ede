#!/usr/bin/env python3
"""Feature-matching recall of one 3DMatch scene on the GPU at several keypoint counts, as geometric_registration/evaluate.py computes it
pair by pair on the host for the ONE count its line 46 names (its users edit that line to sweep 5000 / 2500 / 1000 / 500 / 250).

Reads the `keypoints/<scene>/cloud_bin_<k>.npy` and `descriptors/<scene>/cloud_bin_<k>.D3Feat.npy` files that
utils.results.save_3dmatch_keypoints / save_3dmatch_results wrote under --root (rows in ascending score order), makes ONE
registration.match_pairs call for all pairs id1 < id2 at all --counts (no RANSAC: tools/register_scene.py does the registration),
and prints the lines of evaluate.py:211-216 per count and one JSON line.  A pair that --gt does not list has gt_flag 0 and zeros, as
evaluate.py:60-64 treats it.

    python tools/matching_scene.py --root RESULTS --scene sun3d-hotel_umd-maryland_hotel3 --gt gt.log
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def gt_of_pairs(gt_log, host_pairs):
    """-> (gt_flag i64[P], f32[P, 3, 4] target -> source: the matrices of gt.log, the identity for a pair it does not list)."""
    flag = np.array([1 if "%d_%d" % p in gt_log else 0 for p in host_pairs], np.int64)
    gt = np.tile(np.eye(4)[:3], (len(host_pairs), 1, 1))
    for i, p in enumerate(host_pairs):
        if flag[i]:
            gt[i] = gt_log["%d_%d" % p][:3]
    return flag, gt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--gt", required=True, help="the scene's gt.log (geometric_registration/gt_result/<scene>-evaluation/gt.log)")
    ap.add_argument("--counts", default=None, help="comma-separated keypoint counts, ascending (default: 250,500,1000,2500,5000)")
    ap.add_argument("--desc-name", default="D3Feat")
    ap.add_argument("--inlier-ratio", type=float, default=0.05)
    ap.add_argument("--distance-threshold", type=float, default=0.10)
    a = ap.parse_args()
    import torch
    from d3feat_amd import registration as reg
    from d3feat_amd.utils import results
    from register_scene import load_scene
    counts = tuple(int(c) for c in a.counts.split(",")) if a.counts else reg.MATCHING_COUNTS
    dev = torch.device("cuda", 0)
    blocks = load_scene(a.root, a.scene, a.desc_name, max(counts))
    kp, count = reg.stack_keypoints(blocks, max(counts), device=dev)
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    flag, gt = gt_of_pairs(results.read_gt_log(a.gt), host_pairs)
    res = reg.match_pairs(kp, count, pairs, gt=torch.from_numpy(gt).to(dev), num_keypts=counts, distance_threshold=a.distance_threshold)
    lines, table = results.matching_table(counts, [res.rows(c, flag) for c in range(len(counts))], a.inlier_ratio)
    print("\n".join(lines))
    print(json.dumps(dict(scene=a.scene, fragments=len(blocks), pairs=len(host_pairs), num_keypts=list(counts),
                          recall=[table[k]["recall"] for k in counts], correct=[table[k]["correct"] for k in counts],
                          gt=[table[k]["gt"] for k in counts], ave_num_inliers=[table[k]["ave_num_inliers"] for k in counts],
                          ave_inlier_ratio=[table[k]["ave_inlier_ratio"] for k in counts])))


if __name__ == "__main__":
    main()
