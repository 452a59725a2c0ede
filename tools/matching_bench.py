#!/usr/bin/env python3
"""What does the feature-matching sweep of a scene cost in one device call, against the only way the tree offered before it?  (One
process, one GPU; not bench.py.)

Workload: utils.synthetic.scene(3, n_frag=32, K=5000) -- 32 keypoint blocks of up to 5000 rows with 32-d descriptors, all 496 pairs --
at the five counts of registration.MATCHING_COUNTS, distance threshold 0.10.  Variants are alternated inside the same run, nine
windows each:

  (a) one registration.match_pairs call, then a device synchronise (wall clock);
  (b) the same call captured in a HIP graph, HIP events around a replay;
  (c) the loop over counts and pairs of registration.build_correspondence on the tails (two d3f_feature_nn + d3f_mutual_matches and a
      read-back each) plus the inlier test of evaluate.py:70-77 in torch on the device: register_pairs stops at 1024 rows and runs a
      RANSAC, so before this entry point the loop was the only way to these figures.  It is the baseline.

Before any timing the counts of (a) and (b) are compared with those of (c): equal, no tolerance (the torch inlier test is fp32 without
the kernel's fused multiply-adds: a differing count is reported, not hidden, and fails the run).

    python tools/matching_bench.py [--out profiles/matching_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/matching_bench.py --profile-call      (one call only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from d3feat_amd import registration as reg
from d3feat_amd.utils.synthetic import scene

K = 5000
WINDOWS = 9
THRESHOLD = 0.10


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def pair_loop(dev_blocks, host_pairs, gt, counts, thr):
    """-> (mutual_count, gt_inliers) i64[P, n] through build_correspondence per pair and count"""
    mc = np.zeros((len(host_pairs), len(counts)), np.int64)
    gi = torch.zeros((len(host_pairs), len(counts)), dtype=torch.int64, device=gt.device)
    for c, k in enumerate(counts):
        for p, (a, b) in enumerate(host_pairs):
            s, t = dev_blocks[a][-k:], dev_blocks[b][-k:]
            corr = reg.build_correspondence(s[:, 3:35], t[:, 3:35])
            mc[p, c] = len(corr)
            if len(corr):
                idx = torch.from_numpy(corr).to(gt.device)
                moved = t[idx[:, 1], :3] @ gt[p, :, :3].T + gt[p, :, 3]
                gi[p, c] = torch.sum(torch.sum((s[idx[:, 0], :3] - moved) ** 2, 1) < thr * thr)
    return mc, gi.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "matching_bench.json"))
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--profile-call", action="store_true", help="one match_pairs call and nothing else (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    blocks, poses = scene(3, n_frag=a.fragments, K=K)
    kp, count = reg.stack_keypoints(blocks, K, device=dev)
    dev_blocks = [kp[f, :len(b)] for f, b in enumerate(blocks)]
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    P, counts = len(host_pairs), reg.MATCHING_COUNTS
    gt = torch.from_numpy(np.array([(np.linalg.inv(poses[i]) @ poses[j])[:3] for i, j in host_pairs], np.float32)).to(dev)
    res = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=THRESHOLD)
    torch.cuda.synchronize(dev)
    if a.profile_call:
        print(json.dumps({"pairs": P, "mutual": res.mutual_count.sum(0).cpu().tolist(), "inliers": res.gt_inliers.sum(0).cpu().tolist()}))
        return

    def call():
        reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=THRESHOLD, out=res)
        torch.cuda.synchronize(dev)

    def loop():
        out = pair_loop(dev_blocks, host_pairs, gt, counts, THRESHOLD)
        torch.cuda.synchronize(dev)
        return out

    want_m, want_g = loop()
    call()
    got_m, got_g = res.mutual_count.cpu().numpy(), res.gt_inliers.cpu().numpy()
    differing = np.argwhere((got_m != want_m) | (got_g != want_g))

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gres = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=THRESHOLD)
    with torch.cuda.stream(stream):
        reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=THRESHOLD, out=gres)      # warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=THRESHOLD, out=gres)

    def replay():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            graph.replay()
            e1.record()
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    gres.mutual_count.fill_(-1)
    gres.gt_inliers.fill_(-1)
    replay()
    graph_equal = bool(torch.equal(gres.mutual_count, res.mutual_count) and torch.equal(gres.gt_inliers, res.gt_inliers))
    times = {"device_call": [], "device_call_graph": [], "pair_loop": []}
    for _ in range(WINDOWS):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["pair_loop"].append(wall(loop))
    ns = np.asarray([len(b) for b in blocks])
    out = {"fragments": len(blocks), "pairs": P, "K": K, "rows_per_block": [int(ns.min()), int(ns.max())], "num_keypts": list(counts),
           "distance_threshold": THRESHOLD, "windows": WINDOWS,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, pair_loop), HIP events around "
                     "the graph replay" % WINDOWS,
           "baseline": "pair_loop: registration.build_correspondence per pair and count plus the inlier test in torch; before this entry "
                       "point the only way to these figures above 1024 rows",
           "counts_equal_to_pair_loop": differing.size == 0, "differing_pair_count": differing[:20].tolist(),
           "graph_replay_equal_to_eager": graph_equal, "mutual_per_count": got_m.sum(0).tolist(), "inliers_per_count": got_g.sum(0).tolist(),
           "workspace_bytes": int(reg._lib.load().d3f_match_pairs_workspace_bytes(P, (reg._lib.C.c_int * len(counts))(*counts), len(counts))),
           "distance_evaluations_device": int(2 * sum(min(ns[i], counts[-1]) * min(ns[j], counts[-1]) for i, j in host_pairs)),
           "distance_evaluations_loop": int(2 * sum(min(ns[i], k) * min(ns[j], k) for i, j in host_pairs for k in counts))}
    for k, t in times.items():
        out[k] = stats(t, P)
    h = np.median(times["pair_loop"])
    out["loop_over_device_call"] = round(float(h / np.median(times["device_call"])), 1)
    out["loop_over_device_call_graph"] = round(float(h / np.median(times["device_call_graph"])), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if differing.size or not graph_equal:
        raise SystemExit("counts differ from the pair loop")


if __name__ == "__main__":
    main()
