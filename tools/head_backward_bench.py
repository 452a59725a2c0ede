#!/usr/bin/env python3
"""What do the transposed neighbour table and the backward of the detection head cost, against torch autograd of the restated head,
which materialises the [N, K, C] gather?  (One process, one GPU; not bench.py.  No time is a pass / fail condition.)

Workload: a two-cloud stack of synthetic room fragments of about 30 k points each after 0.03 subsampling, C = 32, the level-0
neighbour matrix of the engine (radius 0.075, K = 42 columns), random features and seeds.  Variants are alternated inside the same
run, nine windows each:

  (a) ops.neighbor_transpose (wall clock around call + synchronise);
  (b) ops.detect_head_backward with the table given: eager (wall clock), and replayed from a HIP graph (HIP events around the replay);
  (c) float32 torch autograd of tests/head_grad_np.torch_head on the same device, forward and backward (wall clock).

Before any timing the gradients of (b) and (c) are compared per row, relative to the largest entry: two float32 evaluations in
different summation orders.  The gradient follows the argmax of a row's score channels, so among 60 k random rows a few may have their
two best channels within an fp32 rounding of each other and be resolved differently; the rows beyond 1e-4 are counted and reported
(the run fails above 1 % of the rows, or if the rest disagree).  A replayed capture must be bit-equal to the eager call.
Medians and ranges go to profiles/head_backward_bench.json.

    python tools/head_backward_bench.py [--out profiles/head_backward_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/head_backward_bench.py --profile-call      (one call of each only)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from validation_bench import WINDOWS, stats

C, K = 32, 42


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_backward_bench.json"))
    ap.add_argument("--profile-call", action="store_true", help="one table build and one backward and nothing else")
    a = ap.parse_args()
    import head_grad_np as hg
    from d3feat_amd import _lib, ops
    from d3feat_amd import tf_custom_ops as tfo
    from d3feat_amd.utils.synthetic import room_fragment
    dev = torch.device("cuda", 0)
    subs = [tfo.grid_subsampling(torch.from_numpy(room_fragment(s, 300000, 1.68)).to(dev), 0.03) for s in range(2)]
    pts = torch.cat(subs, 0)
    host_lens = [int(s.shape[0]) for s in subs]
    lens = ops.as_lens(host_lens, dev)
    nb = ops.NeighborGrid(pts, lens, 0.075).search(pts, lens, K)[0].contiguous()
    N = int(pts.shape[0])
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((N, C), generator=g).to(dev)
    gd, gs = torch.randn((N, C), generator=g).to(dev), torch.randn((N,), generator=g).to(dev)
    table = ops.neighbor_transpose(nb, lens)
    out = torch.empty((N, C), device=dev)
    ops.detect_head_backward(x, nb, lens, None, gd, gs, transpose=table, out=out)
    torch.cuda.synchronize(dev)
    report = {"windows": WINDOWS, "rows": N, "lens": host_lens, "C": C, "K": int(nb.shape[1]),
              "valid_edges": int(table[0][-1]),
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise (transpose, backward, autograd), HIP "
                        "events around the graph replay" % WINDOWS,
              "baseline": "float32 torch autograd of tests/head_grad_np.torch_head on the same device: gathers [N, K, C]",
              "workspace_bytes": {"transpose": int(_lib.load().d3f_neighbor_transpose_workspace_bytes(N, int(nb.shape[1]))),
                                  "backward": int(_lib.load().d3f_detect_head_backward_workspace_bytes(N, C, 2))}}
    if a.profile_call:
        print(json.dumps(report))
        return
    pads = hg.pad_counts(host_lens)
    nbl = nb.long()

    def autograd():
        xt = x.detach().clone().requires_grad_(True)
        desc, score = hg.torch_head(xt, nbl, host_lens, pads)
        ((desc * gd).sum() + (score.reshape(-1) * gs).sum()).backward()
        torch.cuda.synchronize(dev)
        return xt.grad
    want = autograd()
    per_row = (out - want).abs().max(1).values / want.abs().max()
    flipped = int((per_row > 1e-4).sum())
    rel = float(per_row[per_row <= 1e-4].max())
    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    gout = torch.empty((N, C), device=dev)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            ops.detect_head_backward(x, nb, lens, None, gd, gs, transpose=table, out=gout)          # warm-up on this stream
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                ops.detect_head_backward(x, nb, lens, None, gd, gs, transpose=table, out=gout)

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
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0
    gout.fill_(-7.0)
    replay()
    graph_equal = bool(torch.equal(gout.view(torch.int32), out.view(torch.int32)))
    times = {"transpose": [], "backward": [], "backward_graph": [], "autograd": []}
    for _ in range(WINDOWS):
        times["transpose"].append(wall(lambda: ops.neighbor_transpose(nb, lens)))
        times["backward"].append(wall(lambda: ops.detect_head_backward(x, nb, lens, None, gd, gs, transpose=table, out=out)))
        times["backward_graph"].append(replay())
        times["autograd"].append(wall(autograd))
    report.update({"largest_row_difference_to_autograd_over_largest_entry_rows_within_1e-4": rel,
                   "rows_whose_near_tie_the_two_float32_evaluations_resolve_differently": flipped,
                   "graph_replay_equal_to_eager": graph_equal,
                   "bytes_autograd_gathers": (N + 1) * int(nb.shape[1]) * C * 4})
    for k, t in times.items():
        report[k] = stats(t)
    b = np.median(times["autograd"])
    report["autograd_over_backward"] = round(float(b / np.median(times["backward"])), 2)
    report["autograd_over_backward_graph"] = round(float(b / np.median(times["backward_graph"])), 2)
    del pw
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    if not graph_equal or flipped > N // 100:
        raise SystemExit("the device call and autograd disagree")


if __name__ == "__main__":
    main()
