#!/usr/bin/env python3
"""What does keypoint repeatability cost on the device, against the host loop of the reference's recipe?  (One process, one GPU; not
bench.py.)

Workload: utils.synthetic.scene(3, n_frag=32, K=512) -- 32 keypoint blocks of 512 rows, all 496 pairs -- at the eight counts of
registration.REPEATABILITY_COUNTS with registration.REPEATABILITY_3DMATCH.  Variants are alternated inside the same run, nine
windows each:

  (a) one registration.repeatability_pairs call, then a device synchronise (wall clock);
  (b) the same call captured in a HIP graph, HIP events around a replay;
  (c) the host loop of repeatability/evaluate_3dmatch_our.py:30-41 on arrays in memory: per count and pair, slice the last k rows, move
      the target in float64, scipy cdist, distance.min(axis=0) < 0.1 -- eight cdist passes per pair.  Before this feature it was the
      only way to the figure, so it is the baseline.

Before any timing the counts of (a) and (b) are compared with those of (c): equal, no tolerance (a scene whose column minima keep
away from the threshold is not asserted here, so a differing count is reported, with its distance from the threshold, not hidden).

    python tools/repeatability_bench.py [--out profiles/repeatability_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/repeatability_bench.py --profile-call      (one call only)
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

K = 512
WINDOWS = 9


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def host_loop(blocks, host_pairs, gts, counts, thr):
    from scipy.spatial.distance import cdist
    out = np.zeros((len(host_pairs), len(counts)), np.int64)
    for c, k in enumerate(counts):
        for p, (a, b) in enumerate(host_pairs):
            src, tgt = blocks[a][-k:, :3], blocks[b][-k:, :3]
            tgt = tgt.astype(np.float64) @ gts[p][:3, :3].T + gts[p][:3, 3]
            out[p, c] = np.sum(cdist(src, tgt, metric="euclidean").min(axis=0) < thr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "repeatability_bench.json"))
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--profile-call", action="store_true", help="one repeatability_pairs call and nothing else (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    blocks, poses = scene(3, n_frag=a.fragments, K=K)
    kp, count = reg.stack_keypoints(blocks, K, device=dev)
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    P, counts, kw = len(host_pairs), reg.REPEATABILITY_COUNTS, reg.REPEATABILITY_3DMATCH
    gts = np.array([np.linalg.inv(poses[i]) @ poses[j] for i, j in host_pairs])
    gt = torch.from_numpy(np.ascontiguousarray(gts[:, :3])).to(dev)
    res = reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, **kw)
    torch.cuda.synchronize(dev)
    if a.profile_call:
        print(json.dumps({"pairs": P, "totals": res.totals.cpu().tolist()}))
        return

    def call():
        reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, out=res, **kw)
        torch.cuda.synchronize(dev)

    want = host_loop(blocks, host_pairs, gts, counts, kw["distance_threshold"])
    call()
    got = res.repeat.cpu().numpy()
    differing = np.argwhere(got != want)

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gres = reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, **kw)
    with torch.cuda.stream(stream):
        reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, out=gres, **kw)      # warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, out=gres, **kw)

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

    gres.repeat.fill_(-1)
    replay()
    graph_equal = bool(torch.equal(gres.repeat, res.repeat) and torch.equal(gres.totals, res.totals))
    times = {"device_call": [], "device_call_graph": [], "host_loop": []}
    for _ in range(WINDOWS):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["host_loop"].append(wall(lambda: host_loop(blocks, host_pairs, gts, counts, kw["distance_threshold"])))
    ns = np.minimum(np.asarray([len(b) for b in blocks]), K)
    out = {"fragments": len(blocks), "pairs": P, "K": K, "num_keypts": list(counts), "parameters": dict(kw), "windows": WINDOWS,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, host_loop), HIP events around "
                     "the graph replay" % WINDOWS,
           "baseline": "host_loop: before this entry point the figure could only be computed this way",
           "counts_equal_to_host_loop": differing.size == 0, "differing_pair_count": differing[:20].tolist(),
           "graph_replay_equal_to_eager": graph_equal, "scene": [float(v) for v in res.scene()],
           "distance_evaluations_device": int(sum(ns[i] * ns[j] for i, j in host_pairs)),
           "distance_evaluations_host": int(sum(min(ns[i], k) * min(ns[j], k) for i, j in host_pairs for k in counts))}
    for k, t in times.items():
        out[k] = stats(t, P)
    h = np.median(times["host_loop"])
    out["host_over_device_call"] = round(float(h / np.median(times["device_call"])), 1)
    out["host_over_device_call_graph"] = round(float(h / np.median(times["device_call_graph"])), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "parameters"}))
    if differing.size or not graph_equal:
        raise SystemExit("counts differ from the host loop")


if __name__ == "__main__":
    main()
