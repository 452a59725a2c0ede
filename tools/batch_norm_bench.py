#!/usr/bin/env python3
"""What do batch norm in training mode, its backward and the unary convolution's backward cost at the level-0 size, against
torch.nn.functional.batch_norm(training=True) + leaky_relu under torch autograd on the same device?  (One process, one GPU; not
bench.py.  No time is a pass / fail condition.)

Shape: the level-0 stack of the other backward benches (two fragments, 59,104 rows) at C = 64 and 128, LeakyReLU on, no residual.
Variants are alternated inside the same run, nine windows each: eager (wall clock around call + synchronise) and replayed from a HIP
graph (HIP events around the replay).  Before any timing the gradients of the device calls and of autograd are compared relative to
the largest entry (two float32 evaluations in different summation orders, under the device's own LeakyReLU mask: the run fails above
1e-4), and a replayed capture must be bit-equal to the eager call.  Each pass also reports the bytes it must move divided by its replayed time:
  forward         x read twice (the two passes of the moments are one launch each, then the elementwise pass reads it a third time:
                  counted as 3 N C reads) and y written: 16 N C bytes;
  backward        x, y and gy read by the sums and again by the elementwise pass, gx written: 28 N C bytes;
  unary_backward  gy read twice and x once, gx written: 4 N (2 Cout + 2 Cin) bytes.
Medians and ranges go to profiles/batch_norm_bench.json.

    python tools/batch_norm_bench.py [--out profiles/batch_norm_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from validation_bench import WINDOWS, stats

N = 59104
ALPHA, EPS, MOMENTUM = 0.2, 1e-6, 0.99


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_norm_bench.json"))
    a = ap.parse_args()
    from d3feat_amd import _lib, ops
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    report = {"windows": WINDOWS, "rows": N,
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise (eager, autograd), HIP events around "
                        "the graph replay" % WINDOWS,
              "baseline": "float32 torch.nn.functional.batch_norm(training=True) + leaky_relu and a matmul under torch autograd on the "
                          "same device"}
    failed = False

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def rel(got, want):
        return float((got - want).abs().max() / want.abs().max())

    for C in (64, 128):
        x = (torch.randn((N, C), generator=g) * 1.5 + 0.3).to(dev)
        gy = torch.randn((N, C), generator=g).to(dev)
        gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
        W = (torch.randn((C, C), generator=g) / np.sqrt(C)).to(dev)
        mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        keep = {}

        def forward(out=y):
            keep["fw"] = ops.batch_norm_train(x, gamma, beta, EPS, None, True, ALPHA, mm, mv, MOMENTUM, out=out)

        def backward(out=gx, yy=y):
            keep["bw"] = ops.batch_norm_backward(x, yy, gy, gamma, keep["fw"][1], keep["fw"][2], True, ALPHA, out=out)

        def unary():
            keep["un"] = ops.unary_backward(x, W, gy)
        forward(); backward(); unary()
        torch.cuda.synchronize(dev)

        def autograd_bn(mask=None):
            xt, gt, bt = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
            z = torch.nn.functional.batch_norm(xt, None, None, gt, bt, True, 1 - MOMENTUM, EPS)
            out = torch.nn.functional.leaky_relu(z, ALPHA) if mask is None else z * mask
            (out * gy).sum().backward()
            torch.cuda.synchronize(dev)
            return out.detach(), xt.grad, gt.grad, bt.grad

        def autograd_unary():
            xt, Wt = x.detach().clone().requires_grad_(True), W.detach().clone().requires_grad_(True)
            ((xt @ Wt) * gy).sum().backward()
            torch.cuda.synchronize(dev)
            return xt.grad, Wt.grad
        # the gradients are compared under the device's own LeakyReLU mask: among millions of entries a pre-activation within a rounding
        # of zero takes the other branch in the other evaluation, and one such entry moves gbeta by most of its gradient
        own = autograd_bn()[0]
        mask = torch.where(y > 0, 1.0, ALPHA)
        wy, wgx, wgg, wgb = autograd_bn(mask)
        wux, wuw = autograd_unary()
        r = {"C": C, "workspace_bytes": {"batch_norm": int(lib.d3f_batch_norm_workspace_bytes(N, C)),
                                         "gemm_tn": int(lib.d3f_gemm_tn_workspace_bytes(N, C, C))},
             "entries_on_the_other_side_of_zero_in_autograd": int(((own > 0) != (y > 0)).sum()),
             "difference_to_autograd_over_largest_entry": {
                 "y": rel(y, wy), "gx": rel(gx, wgx), "ggamma": rel(keep["bw"][1], wgg), "gbeta": rel(keep["bw"][2], wgb),
                 "unary_gx": rel(keep["un"][0], wux), "unary_gW": rel(keep["un"][1], wuw)}}
        report["C%d" % C] = r
        failed = failed or max(r["difference_to_autograd_over_largest_entry"].values()) > 1e-4
        stream = torch.cuda.Stream(device=dev)
        cy, cgx = torch.empty_like(y), torch.empty_like(gx)
        graphs, pws = {}, []
        eager = dict(y=y.clone(), gx=gx.clone())
        with torch.cuda.stream(stream):
            for name, fn in (("forward", lambda: forward(cy)), ("backward", lambda: backward(cgx, cy)), ("unary_backward", unary)):
                with ops.private_workspace() as pw:
                    fn()
                    stream.synchronize()
                    graphs[name] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[name], stream=stream):
                        fn()
                pws.append(pw)

        def replay(name):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                graphs[name].replay()
                e1.record()
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        cy.fill_(-7.0); cgx.fill_(-7.0)
        replay("forward"); replay("backward")
        r["graph_replay_equal_to_eager"] = bool(torch.equal(cy.view(torch.int32), eager["y"].view(torch.int32)) and
                                                torch.equal(cgx.view(torch.int32), eager["gx"].view(torch.int32)))
        failed = failed or not r["graph_replay_equal_to_eager"]
        times = {k: [] for k in ("forward", "forward_graph", "backward", "backward_graph", "unary_backward", "unary_backward_graph",
                                 "autograd_batch_norm", "autograd_unary")}
        for _ in range(WINDOWS):
            times["forward"].append(wall(forward))
            times["forward_graph"].append(replay("forward"))
            times["backward"].append(wall(backward))
            times["backward_graph"].append(replay("backward"))
            times["unary_backward"].append(wall(unary))
            times["unary_backward_graph"].append(replay("unary_backward"))
            times["autograd_batch_norm"].append(wall(autograd_bn))
            times["autograd_unary"].append(wall(autograd_unary))
        for k, t in times.items():
            r[k] = stats(t)
        must = {"forward": 16 * N * C, "backward": 28 * N * C, "unary_backward": 4 * N * 4 * C}
        r["bytes"] = must
        r["GB_per_s_replayed"] = {k: round(must[k] / float(np.median(times[k + "_graph"])) * 1e-9, 1) for k in must}
        r["autograd_batch_norm_over_forward_plus_backward_graph"] = round(float(
            np.median(times["autograd_batch_norm"]) / (np.median(times["forward_graph"]) + np.median(times["backward_graph"]))), 2)
        r["autograd_unary_over_unary_backward_graph"] = round(float(np.median(times["autograd_unary"]) /
                                                                    np.median(times["unary_backward_graph"])), 2)
        del graphs, pws
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    if failed:
        raise SystemExit("the device calls and autograd disagree")


if __name__ == "__main__":
    main()
