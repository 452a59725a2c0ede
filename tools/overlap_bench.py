#!/usr/bin/env python3
"""What does the overlap of every fragment pair of a scene cost in one device call, against the loop that was the only way before?
(One process, one GPU; not bench.py.)

Workload: utils.synthetic.overlap_scene(SEED, n_frag=32, n_raw=...) -- 32 slabs of one room of about 30 k points each, generated from
the seed where the tool runs -- all 496 pairs a < b at overlap.OVERLAP_3DMATCH's threshold, 0.025.
Variants are alternated inside the same run, nine windows each, device synchronisation around each:

  (a) one overlap.overlap_pairs call over the 496 pairs, grid build included: eager (wall clock), and replayed from a HIP graph (HIP
      events around the replay);
  (b) the parent's means: one single-cloud ops.NeighborGrid per target fragment, then one d3f_neighbor_grid_score(V = 1, identity)
      per pair -- three launches per pair, and every matched point an atomic add to one word (parent_loop below; wall clock).

Before any timing the counts of (a) and (b) are compared: equal, no tolerance.  Medians, ranges and the ratio go to
profiles/overlap_bench.json; (a) counts as faster when the ranges of the nine windows do not overlap.

    python tools/overlap_bench.py [--out profiles/overlap_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/overlap_bench.py --profile-call      (one call only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SEED, N_FRAG, N_RAW = 0, 32, 106000
THR = 0.025
WINDOWS = 9


def parent_loop(clouds, pairs, thr, count=None, nearest=None):
    """The overlap of `pairs` with the entry points that existed before d3f_overlap_pairs: clouds = list of device f32[n, 3] tensors
    (one frame), pairs = list of (a, b).  One ops.NeighborGrid per target that occurs, one d3f_neighbor_grid_score with the identity
    per pair.  -> (count i32[P], nearest i32[P, ld] or None) device tensors; nearest (an i32[P, ld] tensor filled with -1) is
    filled when given.  A pair with an empty fragment counts 0."""
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    dev = clouds[0].device
    st = ops._stream(dev)
    P = len(pairs)
    if count is None:
        count = torch.zeros((P,), dtype=torch.int32, device=dev)
    sumd2 = torch.empty((max(P, 1),), dtype=torch.int64, device=dev)
    ident = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=torch.float32, device=dev)
    grids = {b: ops.NeighborGrid(clouds[b], ops.as_lens([clouds[b].shape[0]], dev), thr) for b in sorted({b for _, b in pairs})
             if clouds[b].shape[0]}
    for p, (a, b) in enumerate(pairs):
        src = clouds[a]
        if not src.shape[0] or b not in grids:
            count[p:p + 1].zero_()
            continue
        g = grids[b]
        row = None
        if nearest is not None:
            row = torch.empty((src.shape[0],), dtype=torch.int32, device=dev)
        rc = lib.d3f_neighbor_grid_score(g.mem.data_ptr(), g.nbytes, g.Ns, src.data_ptr(), src.shape[0], ident.data_ptr(), 1, float(thr),
                                         count[p:p + 1].data_ptr(), sumd2[p:p + 1].data_ptr(), row.data_ptr() if row is not None else None, st)
        _lib.check(rc, "neighbor_grid_score")
        if row is not None:
            nearest[p, :src.shape[0]] = row
    return count, nearest


def stats(times):
    t = np.asarray(times, np.float64) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
            "windows_ms": [round(float(x), 4) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "overlap_bench.json"))
    ap.add_argument("--fragments", type=int, default=N_FRAG)
    ap.add_argument("--raw", type=int, default=N_RAW)
    ap.add_argument("--profile-call", action="store_true", help="one overlap_pairs call and nothing else (for a kernel trace)")
    a = ap.parse_args()
    from d3feat_amd import overlap, registration
    from d3feat_amd.utils.synthetic import overlap_scene
    dev = torch.device("cuda", 0)
    host = overlap_scene(SEED, n_frag=a.fragments, n_raw=a.raw, thr=THR)
    points, lens = overlap.stack_fragments(host, device=dev)
    pairs = registration.scene_pairs(len(host), device=dev)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    P = len(host_pairs)
    res = overlap.overlap_pairs(points, lens, pairs, THR)
    torch.cuda.synchronize(dev)
    if a.profile_call:
        print(json.dumps({"pairs": P, "matched": int(res.count.sum().item())}))
        return
    clouds = list(torch.split(points, [len(c) for c in host]))
    clouds = [c.contiguous() for c in clouds]
    base_count = torch.zeros((P,), dtype=torch.int32, device=dev)

    def call():
        overlap.overlap_pairs(points, lens, pairs, THR, out=res)
        torch.cuda.synchronize(dev)

    def loop():
        parent_loop(clouds, host_pairs, THR, count=base_count)
        torch.cuda.synchronize(dev)

    call()
    loop()
    got, want = res.count.cpu().numpy(), base_count.cpu().numpy()
    differing = np.argwhere(got != want).reshape(-1)

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gres = overlap.overlap_pairs(points, lens, pairs, THR)
    with torch.cuda.stream(stream):
        overlap.overlap_pairs(points, lens, pairs, THR, out=gres)                 # warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        overlap.overlap_pairs(points, lens, pairs, THR, out=gres)

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

    gres.count.fill_(-7)
    replay()
    graph_equal = bool(torch.equal(gres.count, res.count))
    times = {"device_call": [], "device_call_graph": [], "parent_loop": []}
    for _ in range(WINDOWS):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["parent_loop"].append(wall(loop))
    ratios = res.ratios()
    out = {"fragments": len(host), "points_per_fragment": [int(len(c)) for c in host], "pairs": P, "threshold": THR, "windows": WINDOWS,
           "kernel_form": "one thread per query, in the source's cell order",
           "timing": "variants alternated, %d windows each, grid builds included on both sides; wall clock around call + synchronise "
                     "(device_call, parent_loop), HIP events around the graph replay" % WINDOWS,
           "baseline": "parent_loop: one single-cloud grid per target, one d3f_neighbor_grid_score(V = 1, identity) per pair",
           "counts_equal_to_parent_loop": differing.size == 0, "differing_pairs": differing[:20].tolist(),
           "graph_replay_equal_to_eager": graph_equal, "matched_points": int(got.sum()),
           "pairs_above_0.30": int((ratios > 0.30).sum()), "pairs_without_overlap": int((got == 0).sum())}
    for k, t in times.items():
        out[k] = stats(t)
    b = np.median(times["parent_loop"])
    out["parent_over_device_call"] = round(float(b / np.median(times["device_call"])), 2)
    out["parent_over_device_call_graph"] = round(float(b / np.median(times["device_call_graph"])), 2)
    out["ranges_disjoint"] = bool(max(times["device_call"]) < min(times["parent_loop"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if differing.size or not graph_equal:
        raise SystemExit("counts differ from the parent loop")


if __name__ == "__main__":
    main()
