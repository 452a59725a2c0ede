#!/usr/bin/env python3
"""The 3DMatch benchmark on the GPU: geometric_registration/evaluate.py (feature-matching recall, RANSAC, the .log files) and
geometric_registration/3dmatch/evaluate.m (registration recall) for all scenes and every keypoint count in ONE
registration.register_scenes call.

    python tools/evaluate_3dmatch.py --root geometric_registration/D3Feat_xxx --gt-root geometric_registration/gt_result [--counts 250,500,1000] [--out OUT]

Reads `<root>/keypoints/<scene>/cloud_bin_<k>.npy` and `<root>/descriptors/<scene>/cloud_bin_<k>.<desc-name>.npy` (rows in ascending
score order, as utils.results.save_3dmatch_results / save_3dmatch_keypoints write them) of the test scenes present under --root, and
`<gt-root>/<scene>-evaluation/gt.log` / `gt.info`.  The descriptors go to the device as they are: np.nan_to_num (evaluate.py:43-44) is
the first launch of the call.  With --out it writes, per count k (in OUT itself for a single count, in OUT/num_keypts_<k> for several):

    log_result/<scene>-evaluation/<name>.log                           the blocks of evaluate.py:101-110, pairs of gt.log only
    pred_result/<scene>/cloud_bin_<s>_cloud_bin_<t>.rt.txt             num_inliers, inlier_ratio, gt_flag of every pair (:113-115)

and prints, per count, the lines of evaluate.py:211-216 per scene and the lines of mrEvaluateRegistration.m:40 / evaluate.m:47-48, then
one JSON line.  tools/registration_recall.py --log-root OUT/log_result evaluates the written files to the same figures.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from eth_scene import load_blocks


def run(root, gt_root, scenes, counts, desc_name="D3Feat", seed=0, device=None):
    """-> (registration.SceneRegistration of ONE register_scenes call, datasets.threedmatch.Benchmark, fragments per scene)"""
    import torch
    from d3feat_amd import registration as reg
    from d3feat_amd.datasets import threedmatch
    dev = device if device is not None else torch.device("cuda", 0)
    blocks, per_scene = load_blocks(root, scenes, max(counts), desc_name)
    bm = threedmatch.benchmark(gt_root, per_scene, scenes=scenes)
    kp, count = reg.stack_keypoints(blocks, max(counts), device=dev)
    d = lambda a: torch.from_numpy(a).to(dev)
    out = reg.register_scenes(kp, count, d(bm.pairs), d(bm.gt), d(bm.info), d(bm.gt_flag), d(bm.ids), bm.scene_start,
                              num_keypts=counts[0] if len(counts) == 1 else tuple(counts), seed=seed)
    return out, bm, per_scene


def write(out_dir, scenes, counts, out, bm, name="D3Feat_"):
    """the .log and .rt.txt files of every scene and count under out_dir"""
    from d3feat_amd.utils import results
    P, n = len(bm.pairs), len(counts)
    T = np.tile(np.eye(4), (P, n, 1, 1))
    T[:, :, :3] = out.T.cpu().numpy().reshape(P, n, 3, 4).astype(np.float64)
    for c, k in enumerate(counts):
        base = out_dir if n == 1 else os.path.join(out_dir, "num_keypts_%d" % k)
        rows = out.matching.rows(c)
        for s, scene in enumerate(scenes):
            sl = range(int(bm.scene_start[s]), int(bm.scene_start[s + 1]))
            log_dir = os.path.join(base, "log_result", scene + "-evaluation")
            os.makedirs(log_dir, exist_ok=True)
            listed = [p for p in sl if bm.gt_flag[p]]
            path = os.path.join(log_dir, name + ".log")
            if os.path.exists(path):
                os.remove(path)                                   # write_registration_log appends
            results.write_registration_log(path, [tuple(bm.ids[p]) for p in listed], [T[p, c] for p in listed])
            results.write_pair_results(os.path.join(base, "pred_result", scene), [tuple(bm.ids[p]) for p in sl], [rows[p][0] for p in sl],
                                       [rows[p][1] for p in sl], [rows[p][2] for p in sl])


def report(scenes, counts, out, bm):
    from d3feat_amd.utils import results
    per_count = [out.matching.rows(c) for c in range(len(counts))]
    for s, scene in enumerate(scenes):
        a, z = int(bm.scene_start[s]), int(bm.scene_start[s + 1])
        print(scene)
        print("\n".join(results.matching_table(counts, [rows[a:z] for rows in per_count], out.matching.inlier_ratio)[0]))
    for c, k in enumerate(counts):
        print("num_keypts = %d" % k)
        print("\n".join(results.registration_recall_lines(scenes, out.recall, c)))
    print(json.dumps(dict(scenes=list(scenes), pairs=len(bm.pairs), num_keypts=list(counts),
                          matching=[[dict(r) for r in per] for per in out.matching.scenes()],
                          registration=[[dict(r) for r in per] for per in out.recall.scenes()],
                          overall=[out.recall.overall(c) for c in range(len(counts))])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--gt-root", required=True)
    ap.add_argument("--counts", default="250", help="comma-separated keypoint counts, ascending (one count: up to 1024)")
    ap.add_argument("--desc-name", default="D3Feat")
    ap.add_argument("--name", default="D3Feat_", help="the result files are <name>.log (descriptorName of evaluate.m)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from d3feat_amd.datasets import threedmatch
    counts = [int(c) for c in a.counts.split(",")]
    scenes = [s for s in threedmatch.SCENES if os.path.isdir(os.path.join(a.root, "keypoints", s))]
    if not scenes:
        raise SystemExit("%s/keypoints holds none of the 3DMatch test scenes" % a.root)
    out, bm, _ = run(a.root, a.gt_root, scenes, counts, a.desc_name, a.seed)
    if a.out:
        write(a.out, scenes, counts, out, bm, a.name)
    report(scenes, counts, out, bm)


if __name__ == "__main__":
    main()
