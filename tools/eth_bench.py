#!/usr/bin/env python3
"""What does the evaluation half of the ETH test cost in one device call, against the host loop the tree offered before it?  (One
process, one GPU; not bench.py.)

Workload: four synthetic scenes of 32 / 31 / 32 / 37 keypoint blocks of 250 rows with 32-d descriptors (utils.synthetic.scene, one
seed per scene; the block counts of the ETH scenes), all 2123 pairs, every third pair left out of the ground truth, a few NaN planted
in the descriptors; 250 keypoints, distance threshold 0.10, inlier ratio 0.05.  Variants are alternated inside the same run, nine
windows each:

  (a) one registration.match_scenes call (sanitise, match, summarise), then a device synchronise (wall clock);
  (b) the same call captured in a HIP graph, HIP events around a replay;
  (c) the host loop: np.nan_to_num on the host, registration.build_correspondence per pair (two d3f_feature_nn + d3f_mutual_matches
      and a read-back each), the inlier test of evaluate_eth.py:52-59 in torch on the device, then results.feature_matching_recall per
      scene on the rows.  Before match_scenes this loop was the way to these figures.  It is the baseline.

Before any timing the rows of (a) and (b) are compared with those of (c): equal, no tolerance (a difference is reported and fails the
run).  No time is a pass / fail condition.

    python tools/eth_bench.py [--out profiles/eth_bench.json]
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
from d3feat_amd.datasets import eth
from d3feat_amd.utils import results
from d3feat_amd.utils.synthetic import scene

K, WINDOWS, SCENE_BLOCKS = 250, 9, (32, 31, 32, 37)


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def host_loop(raw_blocks, host_pairs, gt, flag, scene_start, dev, thr, ratio):
    """-> (rows, per-scene figures) the slow way"""
    blocks = []
    for b in raw_blocks:
        b = b.copy()
        b[:, 3:35] = np.nan_to_num(b[:, 3:35])
        blocks.append(torch.from_numpy(b).to(dev))
    rows = []
    for p, (a, b) in enumerate(host_pairs):
        if not flag[p]:
            rows.append([0, 0.0, 0])
            continue
        s, t = blocks[a][-K:], blocks[b][-K:]
        corr = reg.build_correspondence(s[:, 3:35], t[:, 3:35])
        n = 0
        if len(corr):
            idx = torch.from_numpy(corr).to(dev)
            moved = t[idx[:, 1], :3] @ gt[p, :, :3].T + gt[p, :, 3]
            n = int(torch.sum(torch.sum((s[idx[:, 0], :3] - moved) ** 2, 1) < thr * thr))
        rows.append([n, float("%.8f" % (n / len(corr))) if len(corr) else 0.0, 1])
    return rows, [results.feature_matching_recall(rows[a:b], ratio) for a, b in zip(scene_start, scene_start[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eth_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    kw = reg.EVALUATE_ETH
    raw_blocks, logs = [], []
    for s, n in enumerate(SCENE_BLOCKS):
        blocks, poses = scene(40 + s, n_frag=n, K=K)
        raw_blocks += blocks
        logs.append({"%d_%d" % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i in range(n) for j in range(i + 1, n) if (i + j) % 3})
    rng = np.random.default_rng(0)
    for b in raw_blocks:                                          # a NaN component in three rows of every block
        b[rng.integers(0, len(b), 3), 3 + rng.integers(0, 32, 3)] = np.nan
    pairs, gt, flag, scene_start = eth.benchmark(SCENE_BLOCKS, logs)
    P = len(pairs)
    assert P == 2123
    host_pairs, starts = [tuple(p) for p in pairs.tolist()], [int(v) for v in scene_start]
    kp0, count = reg.stack_keypoints(raw_blocks, K, device=dev)
    kp = kp0.clone()
    d_pairs, d_gt, d_flag = (torch.from_numpy(x).to(dev) for x in (pairs, gt, flag))
    res = reg.match_scenes(kp, count, d_pairs, d_gt, d_flag, starts, **kw)
    torch.cuda.synchronize(dev)

    def call():
        kp.copy_(kp0)                                             # the descriptors as they arrive: the sanitising launch has work
        reg.match_scenes(kp, count, d_pairs, d_gt, d_flag, starts, out=res, **kw)
        torch.cuda.synchronize(dev)
        res.summary._cache = None
        return res.summary.scenes()

    def loop():
        out = host_loop(raw_blocks, host_pairs, d_gt, flag, starts, dev, kw["distance_threshold"], kw["inlier_ratio"])
        torch.cuda.synchronize(dev)
        return out

    want_rows, want_scenes = loop()
    got_scenes = call()
    got_rows = res.summary.rows(0)
    differing = [p for p in range(P) if got_rows[p] != want_rows[p]]
    scenes_equal = [per[0] for per in got_scenes] == want_scenes

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gkp = kp0.clone()
    with torch.cuda.stream(stream):
        gres = reg.match_scenes(gkp, count, d_pairs, d_gt, d_flag, starts, **kw)                  # warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        reg.match_scenes(gkp, count, d_pairs, d_gt, d_flag, starts, out=gres, **kw)

    def replay():
        gkp.copy_(kp0)
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

    gres.summary.figures.fill_(-1)
    gres.summary.ratio_e8.fill_(-1)
    replay()
    graph_equal = bool(torch.equal(gres.summary.figures, res.summary.figures) and torch.equal(gres.summary.ratio_e8, res.summary.ratio_e8))
    times = {"device_call": [], "device_call_graph": [], "host_loop": []}
    for _ in range(WINDOWS):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["host_loop"].append(wall(loop))
    out = {"scenes": list(SCENE_BLOCKS), "pairs": P, "listed_pairs": int(flag.sum()), "K": K, "num_keypts": list(kw["num_keypts"]),
           "distance_threshold": kw["distance_threshold"], "inlier_ratio": kw["inlier_ratio"], "windows": WINDOWS,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise + the read-back of the summary "
                     "(device_call), around the whole loop (host_loop), HIP events around the graph replay" % WINDOWS,
           "baseline": "host_loop: np.nan_to_num, registration.build_correspondence per listed pair, the inlier test in torch, "
                       "results.feature_matching_recall per scene",
           "rows_equal_to_host_loop": not differing, "differing_pairs": differing[:20], "scenes_equal_to_host_loop": scenes_equal,
           "graph_replay_equal_to_eager": graph_equal, "figures": res.summary.figures.cpu().numpy()[:, 0].tolist()}
    for k, t in times.items():
        out[k] = stats(t, P)
    h = np.median(times["host_loop"])
    out["loop_over_device_call"] = round(float(h / np.median(times["device_call"])), 1)
    out["loop_over_device_call_graph"] = round(float(h / np.median(times["device_call_graph"])), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if differing or not graph_equal or not scenes_equal:
        raise SystemExit("rows differ from the host loop")


if __name__ == "__main__":
    main()
