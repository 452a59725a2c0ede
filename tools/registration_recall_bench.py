#!/usr/bin/env python3
"""What does the registration recall of the 3DMatch benchmark cost behind the RANSAC call, on the device against on the host?  (One
process, one GPU; not bench.py.)

Workload: eight synthetic scenes with the fragment counts of the eight 3DMatch test scenes (60 / 60 / 60 / 55 / 57 / 37 / 66 / 38
keypoint blocks of 250 rows with 32-d descriptors, utils.synthetic.scene, one seed per scene), all 11 905 pairs, every third pair left
out of the ground truth, a synthetic information matrix per listed pair, a few NaN planted in the descriptors; 250 keypoints,
registration.EVALUATE_3DMATCH.  Variants are alternated inside the same run, nine windows each:

  (a) one registration.register_scenes call (sanitise, RANSAC, matching summary, registration recall), a device synchronise and the
      read-back of the two summaries (wall clock);
  (b) the way to the same figures before it: sanitize_descriptors, registration.register_pairs, matching_summary, a synchronise, the
      read-back of T and the numpy restatement of the recall (tests/recall_np.py, the device definition) on the host.

Before any timing the figures of (a) are compared with those of (b): T, the matching figures, `error` bit for bit, flags and the five
sums per scene -- equal, no tolerance (a difference is reported and fails the run).  No time is a pass / fail condition.

    python tools/registration_recall_bench.py [--out profiles/registration_recall_bench.json]
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

import recall_np as rnp
from d3feat_amd import registration as reg
from d3feat_amd.datasets import threedmatch
from d3feat_amd.utils.synthetic import scene

K, WINDOWS, SCENE_BLOCKS = 250, 9, (60, 60, 60, 55, 57, 37, 66, 38)


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_recall_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    raw_blocks, logs, infos = [], [], []
    for s, n in enumerate(SCENE_BLOCKS):
        blocks, poses = scene(60 + s, n_frag=n, K=K)
        raw_blocks += blocks
        keys = [(i, j) for i in range(n) for j in range(i + 1, n) if (i + j) % 3]
        logs.append({"%d_%d" % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i, j in keys})
        A = rng.normal(size=(len(keys), 6, 6))
        infos.append({"%d_%d" % ij: m @ m.T * 50 + 5000 * np.eye(6) for ij, m in zip(keys, A)})
    for b in raw_blocks:                                          # a NaN component in three rows of every block
        b[rng.integers(0, len(b), 3), 3 + rng.integers(0, 32, 3)] = np.nan
    bm = threedmatch.benchmark(None, SCENE_BLOCKS, gt_logs=logs, gt_infos=infos)
    P, starts = len(bm.pairs), [int(v) for v in bm.scene_start]
    assert P == 11905
    kp0, count = reg.stack_keypoints(raw_blocks, K, device=dev)
    kp = kp0.clone()
    d = lambda x: torch.from_numpy(x).to(dev)
    pairs, gt, info, flag, ids = d(bm.pairs), d(bm.gt), d(bm.info), d(bm.gt_flag), d(bm.ids)
    gt32 = d(bm.gt[:, :3].astype(np.float32))
    res = reg.register_scenes(kp, count, pairs, gt, info, flag, ids, starts, num_keypts=K)
    kp.copy_(kp0)
    alone = reg.register_pairs(reg.sanitize_descriptors(kp), count, pairs, num_keypts=K, gt=gt32, **reg.EVALUATE_3DMATCH)
    alone_summary = reg.matching_summary(alone.mutual_count, alone.gt_inliers, flag, starts)
    torch.cuda.synchronize(dev)

    def call():
        kp.copy_(kp0)                                             # the descriptors as they arrive: the sanitising launch has work
        reg.register_scenes(kp, count, pairs, gt, info, flag, ids, starts, num_keypts=K, out=res)
        torch.cuda.synchronize(dev)
        res.matching._cache = None
        return res.matching.scenes(), res.recall.scenes()

    def host():
        kp.copy_(kp0)
        reg.register_pairs(reg.sanitize_descriptors(kp), count, pairs, num_keypts=K, gt=gt32, out=alone, **reg.EVALUATE_3DMATCH)
        reg.matching_summary(alone.mutual_count, alone.gt_inliers, flag, starts, out=alone_summary)
        torch.cuda.synchronize(dev)
        alone_summary._cache = None
        want = rnp.device(alone.T.cpu().numpy(), bm.gt, bm.info, bm.gt_flag, bm.ids, starts)
        return alone_summary.scenes(), rnp.summary(want["figures"]), want

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    got_matching, got_recall = call()
    want_matching, want_recall, want = host()
    h = res.recall.host()
    nan = np.isnan(want["error"][:, 0])
    equal = dict(T=bool(torch.equal(res.T, alone.T)), matching=got_matching == want_matching, recall=got_recall == want_recall,
                 flags=bool(np.array_equal(h["flags"], want["flags"])),
                 error_bits=bool(np.array_equal(np.isnan(h["error"][:, 0]), nan)
                                 and np.array_equal(h["error"][~nan, 0].view(np.uint64), want["error"][~nan, 0].view(np.uint64))))
    times = {"register_scenes": [], "register_pairs_then_host": []}
    for _ in range(WINDOWS):
        times["register_scenes"].append(wall(call))
        times["register_pairs_then_host"].append(wall(host))
    out = {"scenes": list(SCENE_BLOCKS), "pairs": P, "listed_pairs": int(bm.gt_flag.sum()), "K": K, "windows": WINDOWS, "err2": reg.RECALL_3DMATCH["err2"],
           "timing": "variants alternated, %d windows each; wall clock around the calls, a device synchronise and the read-back of the "
                     "summaries (register_scenes) or of T plus the numpy restatement of the recall (register_pairs_then_host)" % WINDOWS,
           "baseline": "register_pairs_then_host: sanitize_descriptors, register_pairs, matching_summary, T.cpu(), tests/recall_np.device",
           "equal_to_host": equal, "overall": res.recall.overall(0), "figures": res.recall.figures.cpu().numpy()[:, 0].tolist()}
    for k, t in times.items():
        out[k] = stats(t, P)
    out["host_over_register_scenes"] = round(float(np.median(times["register_pairs_then_host"]) / np.median(times["register_scenes"])), 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if not all(equal.values()):
        raise SystemExit("figures differ from the host restatement: %s" % equal)


if __name__ == "__main__":
    main()
