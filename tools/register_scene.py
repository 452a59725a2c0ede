#!/usr/bin/env python3
"""Register every fragment pair of one 3DMatch scene on the GPU, as geometric_registration/evaluate.py does pair by pair on the host.

Reads the `keypoints/<scene>/cloud_bin_<k>.npy` and `descriptors/<scene>/cloud_bin_<k>.D3Feat.npy` files that
utils.results.save_3dmatch_keypoints / save_3dmatch_results wrote under --root (rows in ascending score order), takes the last
--num-keypts rows of every fragment (evaluate.py:45-50), registers all pairs id1 < id2 with ONE registration.register_pairs call at
registration.EVALUATE_3DMATCH (evaluate.py:93-99) and writes, under --out:

    <desc_name>.log                               the .log blocks of evaluate.py:101-110 (inverse transforms), pairs of gt.log only
    cloud_bin_<s>_cloud_bin_<t>.rt.txt            num_inliers, inlier_ratio, gt_flag of every pair (evaluate.py:113-115)

and prints the recall line of evaluate.py:200-219.  Without --gt no pair has a ground truth (gt_flag 0 everywhere, as evaluate.py:
60-65 treats a pair that gt.log does not list) and every pair goes into the .log.

--counts 250,500,1000,2500,5000 runs the sweep of evaluate.py:46 instead (ascending counts, up to 8192): ONE
registration.register_pairs_counts call for all pairs at all counts, the same files per count under --out/num_keypts_<k>/ and one
recall line per count (with its num_keypts).

--info gt.info (with --gt) adds, before each of those lines, the line of external/ElasticReconstruction/mrEvaluateRegistration.m:40 for
the scene: the registration recall of geometric_registration/3dmatch/evaluate.m, from registration.registration_recall on the
transforms while they are still on the device.  Without the flag the output is unchanged.

    python tools/register_scene.py --root RESULTS --scene sun3d-hotel_umd-maryland_hotel3 --gt gt.log --out OUT
    python tools/register_scene.py --root RESULTS --scene sun3d-hotel_umd-maryland_hotel3 --gt gt.log --out OUT --counts 250,500,1000,2500,5000
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from d3feat_amd import registration as reg
from d3feat_amd.utils import results


def load_scene(root, scene, desc_name, num_keypts):
    """-> list of f32[k, 3 + C + 1] record blocks, fragment k = cloud_bin_<k> (the score column is not stored with the keypoints:
    it carries the row number, which is ascending as the scores are)."""
    kdir, ddir = os.path.join(root, "keypoints", scene), os.path.join(root, "descriptors", scene)
    ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"cloud_bin_(\d+)\.npy", f) for f in os.listdir(kdir)) if m)
    if ids != list(range(len(ids))) or not ids:
        raise SystemExit("%s: fragments %s are not cloud_bin_0 .. cloud_bin_%d" % (kdir, ids[:5], len(ids) - 1))
    blocks = []
    for k in ids:
        xyz = np.load(os.path.join(kdir, "cloud_bin_%d.npy" % k))[-num_keypts:]
        desc = np.nan_to_num(np.load(os.path.join(ddir, "cloud_bin_%d.%s.npy" % (k, desc_name))))[-num_keypts:]   # evaluate.py:43-44
        blocks.append(np.concatenate([xyz, desc, np.arange(len(xyz), dtype=np.float32)[:, None]], 1).astype(np.float32))
    return blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--gt", default=None, help="the scene's gt.log (geometric_registration/gt_result/<scene>-evaluation/gt.log)")
    ap.add_argument("--info", default=None, help="the scene's gt.info: adds the registration recall line of mrEvaluateRegistration.m")
    ap.add_argument("--num-keypts", type=int, default=250)
    ap.add_argument("--counts", default=None, help="comma-separated ascending keypoint counts: all of them in one call, files per count")
    ap.add_argument("--desc-name", default="D3Feat")
    ap.add_argument("--inlier-ratio", type=float, default=0.05)
    ap.add_argument("--distance-threshold", type=float, default=0.10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    counts = [int(k) for k in a.counts.split(",")] if a.counts else None
    rows_kept = max(counts) if counts else a.num_keypts
    blocks = load_scene(a.root, a.scene, a.desc_name, rows_kept)
    kp, count = reg.stack_keypoints(blocks, rows_kept, device=dev)
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    gt_log = results.read_gt_log(a.gt) if a.gt else {}
    flag = np.array([1 if "%d_%d" % p in gt_log else 0 for p in host_pairs])
    gt = np.tile(np.eye(4)[:3], (len(host_pairs), 1, 1))
    for i, p in enumerate(host_pairs):
        if flag[i]:
            gt[i] = gt_log["%d_%d" % p][:3]
    recall = None
    if a.info:
        if not a.gt:
            raise SystemExit("--info needs --gt")
        info_log = results.read_gt_info(a.info)
        if set(info_log) != set(gt_log):
            raise SystemExit("%s and %s list different pairs" % (a.gt, a.info))
        gt64, info = np.tile(np.eye(4), (len(host_pairs), 1, 1)), np.tile(np.eye(6), (len(host_pairs), 1, 1))
        for i, p in enumerate(host_pairs):
            if flag[i]:
                gt64[i], info[i] = gt_log["%d_%d" % p], info_log["%d_%d" % p]
        gt64, info, dflag = torch.from_numpy(gt64).to(dev), torch.from_numpy(info).to(dev), torch.from_numpy(flag.astype(np.int32)).to(dev)
        # one scene: the block indices of `pairs` are the fragment numbers
        recall = lambda res: reg.registration_recall(res, gt64, info, dflag, pairs, [0, len(host_pairs)], **reg.RECALL_3DMATCH)
    gt = torch.from_numpy(gt.astype(np.float32)).to(dev)

    def write(out_dir, mutual, inl, T34, extra, recall_line=None):
        T = np.tile(np.eye(4), (len(host_pairs), 1, 1))
        T[:, :3] = T34.astype(np.float64)
        # pairs that gt.log does not list: num_inliers = inlier_ratio = gt_flag = 0 and no .log block (evaluate.py:60-65)
        num_inliers = np.where(flag == 1, inl, 0)
        ratio = np.where((flag == 1) & (mutual > 0), inl / np.maximum(mutual, 1), 0.0)
        os.makedirs(out_dir, exist_ok=True)
        logged = [i for i in range(len(host_pairs)) if flag[i] or not a.gt]
        results.write_registration_log(os.path.join(out_dir, "%s.log" % a.desc_name), [host_pairs[i] for i in logged], [T[i] for i in logged])
        rows = results.write_pair_results(out_dir, host_pairs, num_inliers, ratio, flag)
        rec = results.feature_matching_recall(rows, a.inlier_ratio)
        if recall_line is not None:
            print(recall_line)
        print(json.dumps(dict(scene=a.scene, fragments=len(blocks), pairs=len(host_pairs), **extra, **rec)))

    if counts is None:
        res = reg.register_pairs(kp, count, pairs, num_keypts=a.num_keypts, seed=a.seed, gt=gt, distance_threshold=a.distance_threshold,
                                 **reg.EVALUATE_3DMATCH)
        write(a.out, res.mutual_count.cpu().numpy(), res.gt_inliers.cpu().numpy(), res.T.cpu().numpy(), {},
              results.registration_recall_lines([a.scene], recall(res))[0] if recall else None)
        return
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, seed=a.seed, gt=gt, distance_threshold=a.distance_threshold,
                                    **reg.EVALUATE_3DMATCH)
    mutual, inl, T = res.mutual_count.cpu().numpy(), res.gt_inliers.cpu().numpy(), res.T.cpu().numpy()
    rec = recall(res) if recall else None
    for c, k in enumerate(counts):
        write(os.path.join(a.out, "num_keypts_%d" % k), mutual[:, c], inl[:, c], T[:, c], {"num_keypts": k},
              results.registration_recall_lines([a.scene], rec, c)[0] if rec else None)


if __name__ == "__main__":
    main()
