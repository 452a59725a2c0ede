#!/usr/bin/env python3
"""What do the loss and its gradients of every training pair cost in one device call, against torch autograd over the materialised
distance matrices?  (One process, one GPU; not bench.py.  No time is a pass / fail condition.)

Workloads: those of tools/validation_bench.py (its make()): 500 pairs of n = 256 correspondences (3DMatch: keypts_num 256, safe radius
0.1) and 100 pairs of n = 1024 (KITTI: 1024, 1.0), C = 32, stacks of 2 x 2048 rows per pair.  Variants are alternated inside the same
run, nine windows each:

  (a) one validation.loss_gradients call over all pairs: eager (wall clock around call + synchronise), and replayed from a HIP graph
      (HIP events around the replay);
  (b) autograd_loop below: per pair the torch restatement of utils/loss.py (tests/loss_grad_np.torch_loss: the [n, n, C] differences
      of loss.cdist for descriptors and points, masks, logsumexp, softplus, means) in float32 on the same device and its backward
      pass, the gradients accumulated into two [N, C] / [N] tensors (wall clock).

Before any timing the gradients of (a) and (b) are compared: the largest absolute difference relative to the largest entry -- two
float32 evaluations in different summation orders; the run fails above 1e-4 -- for the scores, and for the features without the det
term; with the det term (whose gradient follows the argmin of cn) per pair, the pairs beyond 1e-4 counted: a near-tie of two closest
negatives inside an fp32 rounding may be resolved differently by the two.  A replayed capture must be bit-equal to the eager call.
Medians and ranges go to profiles/loss_gradients_bench.json.

    python tools/loss_gradients_bench.py [--out profiles/loss_gradients_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/loss_gradients_bench.py --profile-call      (one call per workload only)
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

from validation_bench import C, ROWS, WINDOWS, WORKLOADS, make, stats


def autograd_loop(f, s, x, anc, pos, row0, safe_radius, keypts_num, det_loss_weight):
    """-> (d loss / d f [N, C], d loss / d s [N]) of the sum over the pairs of desc_loss + det_loss, one pair at a time."""
    import loss_grad_np as lg
    f = f.detach().clone().requires_grad_(True)
    s = s.detach().clone().requires_grad_(True)
    for p in range(anc.shape[0]):
        lo, hi = int(row0[p]), int(row0[p + 1])
        val = lg.torch_loss(f[lo:hi], s[lo:hi], x[lo:hi], anc[p].long(), pos[p].long(), safe_radius, keypts_num, det_loss_weight)
        if val is not None:
            val.backward()
    return f.grad, s.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_gradients_bench.json"))
    ap.add_argument("--profile-call", action="store_true", help="one loss_gradients call per workload and nothing else")
    a = ap.parse_args()
    from d3feat_amd import ops, validation
    dev = torch.device("cuda", 0)
    report = {"windows": WINDOWS, "descriptor_dim": C, "rows_per_pair": 2 * ROWS,
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, autograd_loop), HIP "
                        "events around the graph replay" % WINDOWS,
              "baseline": "autograd_loop: per pair the torch restatement of utils/loss.py over the materialised n x n x C differences, "
                          "forward and backward, float32 torch ops on the same device"}
    failed = False
    for name, P, n, par, cube in WORKLOADS:
        f, s, x, anc, pos, nd, row0 = make(1, P, n, cube, dev)
        res = validation.loss_gradients(f, s, x, anc, pos, nd, row0, **par)
        torch.cuda.synchronize(dev)
        if a.profile_call:
            report[name] = {"pairs": P, "n": n, "largest_feature_gradient": float(res.features.abs().max())}
            continue
        host_row0 = row0.cpu().tolist()

        def call():
            validation.loss_gradients(f, s, x, anc, pos, nd, row0, out=res, **par)
            torch.cuda.synchronize(dev)

        def loop():
            r = autograd_loop(f, s, x, anc, pos, host_row0, **par)
            torch.cuda.synchronize(dev)
            return r
        bf, bs = loop()
        # the scores' gradient w (fp - cn) / n is continuous in cn and is compared as it is.  The features' is not: the det term sends
        # w sab / n to the argmin column of cn, and among ~1e5 random rows a few have their two closest negatives within an fp32
        # rounding of each other, where two float32 evaluations may pick different columns.  So the features are compared (1) without
        # the det term (smooth: every pair must agree), (2) with it, per pair: the pairs beyond the bar are counted and reported
        rel_s = float((res.scores - bs).abs().max() / bs.abs().max())
        par0 = dict(par, det_loss_weight=0.0)
        bf0, _ = autograd_loop(f, s, x, anc, pos, host_row0, **par0)
        rel_f = float((validation.loss_gradients(f, s, x, anc, pos, nd, row0, **par0).features - bf0).abs().max() / bf0.abs().max())
        per_pair = (res.features - bf).abs().view(P, -1).max(1).values / bf.abs().max()
        flipped = int((per_pair > 1e-4).sum())
        rel_f_det = float(per_pair[per_pair <= 1e-4].max()) if flipped < P else float("nan")
        stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
        gres = validation.PairGradients(P, int(f.shape[0]), C, dev)
        with torch.cuda.stream(stream):
            with ops.private_workspace() as pw:
                validation.loss_gradients(f, s, x, anc, pos, nd, row0, out=gres, **par)          # warm-up on this stream
                stream.synchronize()
                with torch.cuda.graph(graph, stream=stream):
                    validation.loss_gradients(f, s, x, anc, pos, nd, row0, out=gres, **par)

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
        gres.features.fill_(-7.0)
        replay()
        graph_equal = bool(torch.equal(gres.features.view(torch.int32), res.features.view(torch.int32))
                           and torch.equal(gres.scores.view(torch.int32), res.scores.view(torch.int32))
                           and torch.equal(gres.values.view(torch.int32), res.values.view(torch.int32)))
        times = {"device_call": [], "device_call_graph": [], "autograd_loop": []}
        for _ in range(WINDOWS):
            times["device_call"].append(wall(call))
            times["device_call_graph"].append(replay())
            times["autograd_loop"].append(wall(loop))
        w = {"pairs": P, "n": n, "parameters": par,
             "largest_difference_to_autograd_over_largest_entry": {"features_without_det_term": rel_f, "scores": rel_s,
                                                                   "features_with_det_term_pairs_within_1e-4": rel_f_det},
             "pairs_whose_near_tie_of_cn_the_two_float32_evaluations_resolve_differently": flipped,
             "graph_replay_equal_to_eager": graph_equal, "workspace_bytes": int(validation._lib.load().d3f_loss_gradients_workspace_bytes(P, n, C)),
             "bytes_the_loop_materialises_per_pair": int(n) * int(n) * (C + 3) * 4}
        for k, t in times.items():
            w[k] = stats(t)
        b = np.median(times["autograd_loop"])
        w["autograd_loop_over_device_call"] = round(float(b / np.median(times["device_call"])), 2)
        w["autograd_loop_over_device_call_graph"] = round(float(b / np.median(times["device_call_graph"])), 2)
        w["ranges_disjoint"] = bool(max(times["device_call"]) < min(times["autograd_loop"]))
        report[name] = w
        failed = failed or not graph_equal or max(rel_f, rel_s) > 1e-4 or flipped > P // 20
        del pw
    if not a.profile_call:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))
    if failed:
        raise SystemExit("the device call and autograd disagree")


if __name__ == "__main__":
    main()
