#!/usr/bin/env python3
"""What does the registration sweep of a scene cost in one device call, against the only way the tree offered before it?  (One
process, one GPU; not bench.py.)

Workload: utils.synthetic.scene(3, n_frag=32, K=5000) -- 32 keypoint blocks of up to 5000 rows with 32-d descriptors, all 496 pairs --
at the five counts of registration.MATCHING_COUNTS with registration.EVALUATE_3DMATCH.  Variants are alternated inside the same run,
nine windows each:

  (a) one registration.register_pairs_counts call, then a device synchronise (wall clock);
  (b) the same call captured in a HIP graph, HIP events around a replay;
  (c) the loop over counts and pairs of registration.register_keypoints (a grid, several launches and several read-backs per
      iteration): above 1024 rows the only way to these figures before this entry point.  It is the baseline.

Before any timing the results of (a) and (b) are compared with those of (c): equal, no tolerance, or the run fails.  A second part
records the new call at the single count 250 against registration.register_pairs on the same input (the blocks' last 250 rows), the
case the older call was built for.

    python tools/register_counts_bench.py [--out profiles/register_counts_bench.json] [--fragments 32] [--windows 9]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/register_counts_bench.py --profile-call      (one call only)
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

K = 5000
SEED = 5
FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count")


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "register_counts_bench.json"))
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--profile-call", action="store_true", help="one register_pairs_counts call and nothing else (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    blocks, _ = scene(3, n_frag=a.fragments, K=K)
    kp, count = reg.stack_keypoints(blocks, K, device=dev)
    dev_blocks = [kp[f, :len(b)] for f, b in enumerate(blocks)]
    pairs = reg.scene_pairs(len(blocks), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    P, counts = len(host_pairs), reg.MATCHING_COUNTS
    kw = dict(reg.EVALUATE_3DMATCH, seed=SEED)
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, nearest=True, **kw)
    torch.cuda.synchronize(dev)
    if a.profile_call:
        print(json.dumps({"pairs": P, "validations": res.validations.sum(0).cpu().tolist()}))
        return

    def call():
        reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, nearest=True, out=res, **kw)
        torch.cuda.synchronize(dev)

    def loop():
        out = [[reg.register_keypoints(dev_blocks[i], dev_blocks[j], num_keypts=k, device=dev, **kw) for k in counts] for i, j in host_pairs]
        torch.cuda.synchronize(dev)
        return out

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def graph_of(fn):
        """fn(out) -> result; captured on a stream of its own -> (result, replay() in seconds, what keeps the workspace alive)"""
        stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
        gres = fn(None)
        with ops.private_workspace() as pw:
            with torch.cuda.stream(stream):
                fn(gres)                                                               # warm-up on this stream (scratch)
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                fn(gres)

        def replay():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                graph.replay()
                e1.record()
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        return gres, replay, (graph, pw.kept)

    # the results first: all pairs, all counts, no tolerance
    want = loop()
    call()
    print("results of the loop and of the call are in", file=sys.stderr, flush=True)
    mismatches = []
    for p, row in enumerate(want):
        for c, w in enumerate(row):
            g = res.host(p, c)
            same = (np.array_equal(g["transformation"].view(np.uint64), w["transformation"].view(np.uint64)) and g["fitness"] == w["fitness"]
                    and g["inlier_rmse"] == w["inlier_rmse"] and g["validations"] == w["validations"]
                    and np.array_equal(g["correspondence_set"], w["correspondence_set"]) and g["mutual_count"] == len(w["correspondences"]))
            if not same:
                mismatches.append([host_pairs[p][0], host_pairs[p][1], counts[c]])
    gres, replay, keep = graph_of(lambda out: reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, nearest=True, out=out, **kw))
    for f in FIELDS + ("nearest",):
        getattr(gres, f).fill_(-7)
    replay()
    graph_equal = all(torch.equal(getattr(gres, f), getattr(res, f)) for f in FIELDS + ("nearest",))
    times = {"device_call": [], "device_call_graph": [], "pair_loop": []}
    for w in range(a.windows):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["pair_loop"].append(wall(loop))
        print("window %d: call %.1f ms, graph %.1f ms, loop %.1f ms" % (w, *(times[k][-1] * 1e3 for k in times)), file=sys.stderr, flush=True)
    validations = res.validations.cpu().numpy().astype(np.int64)
    ns, nt = res.ns.cpu().numpy().astype(np.int64), res.nt.cpu().numpy().astype(np.int64)
    rows = np.asarray([len(b) for b in blocks])
    c_ks = (reg._lib.C.c_int * len(counts))(*counts)
    per_call = min(P, max(reg.PAIRS_PER_CALL // len(counts), 1))
    out = {"fragments": len(blocks), "pairs": P, "K": K, "rows_per_block": [int(rows.min()), int(rows.max())], "num_keypts": list(counts),
           "parameters": dict(kw), "windows": a.windows,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, pair_loop), HIP events around "
                     "the graph replay" % a.windows,
           "baseline": "pair_loop: registration.register_keypoints per pair and count; above 1024 rows the only way to these figures before "
                       "this entry point",
           "results_equal_to_pair_loop": not mismatches, "mismatching_pair_count": mismatches[:20],
           "graph_replay_equal_to_eager": bool(graph_equal),
           "validations_per_count": validations.sum(0).tolist(), "iterations_per_count": res.iterations.sum(0).cpu().tolist(),
           "scored_source_rows_per_count": (validations * ns).sum(0).tolist(),
           "workspace_bytes_per_entry_point_call": int(reg._lib.load().d3f_register_pairs_counts_workspace_bytes(
               per_call, len(blocks), K, reg._lib.C.addressof(c_ks), len(counts), kw["max_validation"]))}
    for k, t in times.items():
        out[k] = stats(t, P)
    h = np.median(times["pair_loop"])
    out["loop_over_device_call"] = round(float(h / np.median(times["device_call"])), 2)
    out["loop_over_device_call_graph"] = round(float(h / np.median(times["device_call_graph"])), 2)

    # the single count 250: the new call (one grid over all blocks, no block in LDS) against register_pairs (both blocks in LDS)
    k250 = counts[0]
    old = reg.register_pairs(kp, count, pairs, num_keypts=k250, **kw)
    new = reg.register_pairs_counts(kp, count, pairs, num_keypts=(k250,), nearest=True, **kw)

    def call_old():
        reg.register_pairs(kp, count, pairs, num_keypts=k250, out=old, **kw)
        torch.cuda.synchronize(dev)

    def call_new():
        reg.register_pairs_counts(kp, count, pairs, num_keypts=(k250,), nearest=True, out=new, **kw)
        torch.cuda.synchronize(dev)

    call_old()
    call_new()
    at = new.at(0)
    single = {"num_keypts": k250, "register_pairs_counts": [], "register_pairs": [],
              "results_equal": all(torch.equal(at[f].contiguous(), getattr(old, f)) for f in FIELDS + ("nearest",))}
    for _ in range(a.windows):
        single["register_pairs_counts"].append(wall(call_new))
        single["register_pairs"].append(wall(call_old))
    for k in ("register_pairs_counts", "register_pairs"):
        single[k] = stats(single[k], P)
    single["register_pairs_counts_over_register_pairs"] = round(single["register_pairs_counts"]["median_ms"] / single["register_pairs"]["median_ms"], 2)
    out["single_count"] = single
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    del keep
    if mismatches or not graph_equal or not single["results_equal"]:
        raise SystemExit("results differ")


if __name__ == "__main__":
    main()
