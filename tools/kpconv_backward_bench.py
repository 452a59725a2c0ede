#!/usr/bin/env python3
"""What does the backward of the rigid KPConv cost, against torch autograd of the restated operator, which materialises the
[Nq, K, num_kp] influences and the [Nq, K, Cin] gather?  (One process, one GPU; not bench.py.  No time is a pass / fail condition.)

Workloads, Cin = Cout = 32, 15 kernel points, linear influence, 'sum':
  level0   the two-fragment level-0 stack of tools/head_backward_bench.py (about 30 k points per cloud after 0.03 subsampling, radius
           0.075, K = 42 columns): the queries are the supports;
  strided  the same supports, queries = the clouds subsampled again at 0.06 (a strided layer: Nq != Ns).
The features are |N(0, 1)|: every row sum is positive by a wide margin, so the neighbour count is not decided by rounding in either
evaluation.  Variants are alternated inside the same run, nine windows each:

  (a) ops.neighbor_transpose_supports (wall clock around call + synchronise);
  (b) ops.kpconv_backward with the table given: eager (wall clock), and replayed from a HIP graph (HIP events around the replay);
  (c) float32 torch autograd of tests/kpconv_grad_np.torch_kpconv on the same device, forward and backward (wall clock).

Before any timing the gradients of (b) and (c) are compared relative to the largest entry (two float32 evaluations in different
summation orders: the run fails above 1e-4), and a replayed capture must be bit-equal to the eager call.
Medians and ranges go to profiles/kpconv_backward_bench.json.

    python tools/kpconv_backward_bench.py [--out profiles/kpconv_backward_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/kpconv_backward_bench.py --profile-call      (one call of each only)
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

C, K, NUM_KP, EXTENT = 32, 42, 15, 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kpconv_backward_bench.json"))
    ap.add_argument("--profile-call", action="store_true", help="one table build and one backward per workload and nothing else")
    a = ap.parse_args()
    import kpconv_grad_np as kg
    from d3feat_amd import _lib, ops
    from d3feat_amd import tf_custom_ops as tfo
    from d3feat_amd.utils.synthetic import room_fragment
    from oracle import kpconv_cases as kc
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    subs = [tfo.grid_subsampling(torch.from_numpy(room_fragment(s, 300000, 1.68)).to(dev), 0.03) for s in range(2)]
    pts = torch.cat(subs, 0)
    host_lens = [int(s.shape[0]) for s in subs]
    lens = ops.as_lens(host_lens, dev)
    grid = ops.NeighborGrid(pts, lens, 0.075)
    coarse = [tfo.grid_subsampling(s, 0.06) for s in subs]
    qpts = torch.cat(coarse, 0)
    q_lens = ops.as_lens([int(s.shape[0]) for s in coarse], dev)
    KP = kc.kernel_points(0, NUM_KP)
    g = torch.Generator(device="cpu").manual_seed(0)
    Ns = int(pts.shape[0])
    f = torch.randn((Ns, C), generator=g).abs().to(dev)
    W = torch.from_numpy(kc.weights(0, NUM_KP, C, C)).to(dev)
    KPt = torch.from_numpy(KP).to(dev)
    report = {"windows": WINDOWS, "Cin": C, "Cout": C, "num_kp": NUM_KP, "lens": host_lens,
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise (transpose, backward, autograd), HIP "
                        "events around the graph replay" % WINDOWS,
              "baseline": "float32 torch autograd of tests/kpconv_grad_np.torch_kpconv on the same device: materialises [Nq, K, num_kp, 3] "
                          "differences and the [Nq, K, Cin] gather"}
    failed = False
    for name, q, ql in (("level0", pts, lens), ("strided", qpts, q_lens)):
        nb = grid.search(q, ql, K)[0].contiguous()
        Nq = int(q.shape[0])
        gout = torch.randn((Nq, C), generator=g).to(dev)
        table = ops.neighbor_transpose_supports(nb, Ns)
        gf, gW = torch.empty((Ns, C), device=dev), torch.empty((NUM_KP, C, C), device=dev)

        def backward(of=gf, ow=gW):
            return ops.kpconv_backward(q, pts, nb, f, KP, W, gout, EXTENT, transpose=table, out_features=of, out_weights=ow)
        backward()
        torch.cuda.synchronize(dev)
        r = {"queries": Nq, "supports": Ns, "K": int(nb.shape[1]), "valid_edges": int(table[0][-1]),
             "workspace_bytes": {"transpose": int(lib.d3f_neighbor_transpose_workspace_bytes(Nq, int(nb.shape[1]))),
                                 "backward": int(lib.d3f_kpconv_backward_workspace_bytes(Nq, Ns, int(nb.shape[1]), C, C, NUM_KP))},
             "bytes_autograd_gathers": Nq * int(nb.shape[1]) * C * 4}
        report[name] = r
        if a.profile_call:
            continue
        nbl = torch.where((nb < 0) | (nb >= Ns), torch.full_like(nb, Ns), nb).long()

        def autograd():
            ft, Wt = f.detach().clone().requires_grad_(True), W.detach().clone().requires_grad_(True)
            out = kg.torch_kpconv(q, pts, nbl, ft, KPt, Wt, EXTENT, "linear", "sum")
            (out * gout).sum().backward()
            torch.cuda.synchronize(dev)
            return ft.grad, Wt.grad
        want_f, want_w = autograd()
        r["gf_difference_to_autograd_over_largest_entry"] = float((gf - want_f).abs().max() / want_f.abs().max())
        r["gW_difference_to_autograd_over_largest_entry"] = float((gW - want_w).abs().max() / want_w.abs().max())
        stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
        cf, cw = torch.empty_like(gf), torch.empty_like(gW)
        with torch.cuda.stream(stream):
            with ops.private_workspace() as pw:
                backward(cf, cw)                                                   # warm-up on this stream
                stream.synchronize()
                with torch.cuda.graph(graph, stream=stream):
                    backward(cf, cw)

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
        cf.fill_(-7.0)
        cw.fill_(-7.0)
        replay()
        r["graph_replay_equal_to_eager"] = bool(torch.equal(cf.view(torch.int32), gf.view(torch.int32)) and
                                                torch.equal(cw.view(torch.int32), gW.view(torch.int32)))
        times = {"transpose": [], "backward": [], "backward_graph": [], "autograd": []}
        for _ in range(WINDOWS):
            times["transpose"].append(wall(lambda: ops.neighbor_transpose_supports(nb, Ns)))
            times["backward"].append(wall(backward))
            times["backward_graph"].append(replay())
            times["autograd"].append(wall(autograd))
        for k, t in times.items():
            r[k] = stats(t)
        b = np.median(times["autograd"])
        r["autograd_over_backward"] = round(float(b / np.median(times["backward"])), 2)
        r["autograd_over_backward_graph"] = round(float(b / np.median(times["backward_graph"])), 2)
        failed = failed or not r["graph_replay_equal_to_eager"] or r["gf_difference_to_autograd_over_largest_entry"] > 1e-4 or \
            r["gW_difference_to_autograd_over_largest_entry"] > 1e-4
        del pw, graph
    if a.profile_call:
        print(json.dumps(report))
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    if failed:
        raise SystemExit("the device call and autograd disagree")


if __name__ == "__main__":
    main()
