#!/usr/bin/env python3
"""What does registering every pair of a scene in one call save?  (One process, one GPU; not bench.py.)

Workload: utils.synthetic.scene(3, n_frag=32) -- 32 keypoint blocks of K = 250 rows, all 496 pairs -- at registration.EVALUATE_3DMATCH
(the call of geometric_registration/evaluate.py:93-99), seed 5.  Variants are alternated inside the same run, nine windows each:

  (a) the single-pair path: a Python loop of registration.register_keypoints over the 496 pairs, then a device synchronise;
  (b) one registration.register_pairs call, then a device synchronise (wall clock, as (a));
      and the same call captured in a HIP graph, HIP events around a replay.

Before any timing the 496 results of (b) are compared with those of (a): transformation bits, fitness, rmse, validations and both
correspondence lists equal, no tolerance.  Reported: median, minimum and maximum of the windows in pairs/s, the ratio of the medians,
whether (b)'s median window is shorter than the FASTEST window of (a), and the distance evaluations the scoring kernel performs
(sum over the pairs of validations x Ns x Nt) for the per-kernel times of a kernel trace:

    python tools/registration_bench.py [--out profiles/register_pairs_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/registration_bench.py --profile-call      (one register_pairs call only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from d3feat_amd import ops
from d3feat_amd import registration as reg
from d3feat_amd.utils.synthetic import scene

K = 250
WINDOWS = 9
SEED = 5


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(float(t.min()) * 1e3, 3), "max_ms": round(float(t.max()) * 1e3, 3),
            "pairs_per_s": {"median": round(pairs / float(np.median(t)), 1), "min": round(pairs / float(t.max()), 1),
                            "max": round(pairs / float(t.min()), 1)},
            "windows_ms": [round(float(x) * 1e3, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "register_pairs_bench.json"))
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--profile-call", action="store_true", help="one register_pairs call and nothing else (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    blocks, _ = scene(3, n_frag=a.fragments, K=K)
    kp, count = reg.stack_keypoints(blocks, K, device=dev)
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = pairs.cpu().tolist()
    P = len(host_pairs)
    kw = dict(reg.EVALUATE_3DMATCH, seed=SEED)
    if a.profile_call:
        res = reg.register_pairs(kp, count, pairs, correspondences=True, **kw)
        torch.cuda.synchronize(dev)
        print(json.dumps({"pairs": P, "validations": int(res.validations.sum().item())}))
        return

    def single():
        out = [reg.register_keypoints(kp[i], kp[j], num_keypts=K, device=dev, **kw) for i, j in host_pairs]
        torch.cuda.synchronize(dev)
        return out

    res = reg.register_pairs(kp, count, pairs, correspondences=True, **kw)

    def batched():
        reg.register_pairs(kp, count, pairs, correspondences=True, out=res, **kw)
        torch.cuda.synchronize(dev)

    # the results first: all pairs, no tolerance
    want = single()
    batched()
    mismatches = []
    for p, w in enumerate(want):
        g = res.host(p)
        same = (np.array_equal(g["transformation"].view(np.uint64), w["transformation"].view(np.uint64)) and g["fitness"] == w["fitness"]
                and g["inlier_rmse"] == w["inlier_rmse"] and g["validations"] == w["validations"]
                and np.array_equal(g["correspondence_set"], w["correspondence_set"]) and np.array_equal(g["correspondences"], w["correspondences"]))
        if not same:
            mismatches.append(host_pairs[p])
    validations = res.validations.cpu().numpy().astype(np.int64)
    ns = res.ns.cpu().numpy().astype(np.int64)
    nt = res.nt.cpu().numpy().astype(np.int64)

    # the captured form
    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gres = reg.register_pairs(kp, count, pairs, correspondences=True, **kw)
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            reg.register_pairs(kp, count, pairs, correspondences=True, out=gres, **kw)      # warm-up on this stream (scratch)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            reg.register_pairs(kp, count, pairs, correspondences=True, out=gres, **kw)
    keep = pw.kept

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

    replay()
    graph_equal = all(torch.equal(getattr(gres, k), getattr(res, k)) for k in ("T", "inliers", "sumd2", "validations", "iterations",
                                                                              "best_iteration", "mutual_count", "nearest", "mutual"))
    times = {"single_pair_loop": [], "register_pairs": [], "register_pairs_graph": []}
    for _ in range(WINDOWS):
        times["single_pair_loop"].append(wall(single))
        times["register_pairs"].append(wall(batched))
        times["register_pairs_graph"].append(replay())
    out = {"fragments": len(blocks), "pairs": P, "K": K, "parameters": dict(kw), "windows": WINDOWS,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise, HIP events around the graph replay" % WINDOWS,
           "results_equal_to_single_pair_path": not mismatches, "mismatching_pairs": mismatches[:20],
           "graph_replay_equal_to_eager": bool(graph_equal)}
    for k, t in times.items():
        out[k] = stats(t, P)
    a_t, b_t = np.asarray(times["single_pair_loop"]), np.asarray(times["register_pairs"])
    out["ratio_of_medians"] = round(float(np.median(a_t) / np.median(b_t)), 2)
    out["graph_ratio_of_medians"] = round(float(np.median(a_t) / np.median(times["register_pairs_graph"])), 2)
    out["median_below_fastest_single_pair_window"] = bool(np.median(b_t) < a_t.min())
    out["validations"] = {"sum": int(validations.sum()), "min": int(validations.min()), "max": int(validations.max())}
    out["score_distance_evaluations"] = int((validations * ns * nt).sum())
    out["hypothesis_iterations"] = int(res.iterations.sum().item())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "parameters"}))
    del keep
    if mismatches or not graph_equal:
        raise SystemExit("results differ from the single-pair path")


if __name__ == "__main__":
    main()
