#!/usr/bin/env python3
"""What do the backward of the max pooling and of the nearest upsampling cost, and what does one whole training step cost?  (One process,
one GPU; not bench.py.  No time is a pass / fail condition.)

Workload: a stack of two clouds of about 30 k points each (one fragment after 0.03 subsampling, stacked with itself as the test
generator does), the shipped 3DMatch architecture, the pyramid of the dataset pipeline; keypts_num index pairs drawn between the two clouds.  Variants are alternated inside the same run, nine windows each, wall clock around
call + synchronise:

  operators  at the first level boundary (the level-0 features pooled to level 1, 128 columns; the level-1 features upsampled to level
             0, 128 + 64 columns of gradient): ops.ind_max_pool_backward / ops.closest_pool_cat_backward with the table given --
             eager; replayed from a HIP graph (the replay compared bit for bit with the eager call before timing); float32 torch
             autograd of the gather statement on the device (the gradients compared before timing, the deviation recorded);
  step       model.run() at dropout_prob = 0.5 (forward + loss), model.backward(), MomentumSGD.step(), each timed separately --
             against the same step with torch autograd standing in for the two new operators only.

Medians and ranges go to profiles/training_step_bench.json.

    python tools/training_step_bench.py [--out profiles/training_step_bench.json]
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

LIMITS = np.asarray([37, 35, 36, 38, 38], np.int32)


def torch_max_pool(x, inds):
    """models/network_blocks.py:51-66 on the device."""
    n = x.shape[0]
    xs = torch.cat([x, torch.amin(x, dim=0, keepdim=True)], 0)
    idx = torch.where((inds < 0) | (inds >= n), torch.full_like(inds, n), inds).long()
    return torch.amax(xs[idx], dim=1)


def torch_upsample_cat(x, inds, skip=None):
    """models/network_blocks.py:69-83 + the concatenation on the device."""
    n = x.shape[0]
    xs = torch.cat([x, torch.zeros_like(x[:1])], 0)
    first = inds[:, 0]
    up = xs[torch.where((first < 0) | (first >= n), torch.full_like(first, n), first).long()]
    return up if skip is None else torch.cat([up, skip], 1)


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def capture(fn, dev):
    from d3feat_amd import ops
    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            fn()
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                fn()
    stream.synchronize()

    def replay():
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
    return replay, (graph, pw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training_step_bench.json"))
    a = ap.parse_args()
    from d3feat_amd import ops
    from d3feat_amd import tf_custom_ops as tfo
    from d3feat_amd.datasets.common import FragmentDataset
    from d3feat_amd.kernels import autograd as ag
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.training import MomentumSGD
    from d3feat_amd.utils.config import threedmatch_config
    from d3feat_amd.utils.synthetic import room_fragment
    dev = torch.device("cuda", 0)
    cfg = threedmatch_config()
    cfg.det_loss_weight = 1.0
    sub = tfo.grid_subsampling(torch.from_numpy(room_fragment(0, 300000, 1.68)).to(dev), 0.03).cpu().numpy()
    ds = FragmentDataset([sub], fast=True)                                        # (the fragment stacked with itself: two clouds)
    ds.neighborhood_limits = LIMITS
    gen, _, _ = ds.get_batch_gen("test", cfg)
    batch = list(next(iter(gen())))
    flat = ds.get_tf_mapping(cfg)(*ds._to_device(batch))
    L = cfg.num_layers
    n0 = int(flat[0].shape[0])
    # the index pairs run between the two halves of the stack
    rng = np.random.default_rng(0)
    half = n0 // 2
    flat = list(flat)
    flat[4 * L + 5] = torch.from_numpy(rng.integers(0, half, cfg.keypts_num).astype(np.int32)).to(dev)
    flat[4 * L + 6] = torch.from_numpy((half + rng.integers(0, n0 - half, cfg.keypts_num)).astype(np.int32)).to(dev)
    report = {"windows": WINDOWS, "rows_per_level": [int(p.shape[0]) for p in flat[:L]],
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise" % WINDOWS}
    g = torch.Generator(device="cpu").manual_seed(0)
    # ---- the two operators at the first level boundary -----------------------------------------------------------------------------
    pools, ups = flat[2 * L], flat[3 * L]
    n1 = int(flat[1].shape[0])
    x = torch.randn((n0, 128), generator=g).to(dev)
    gy = torch.randn((n1, 128), generator=g).to(dev)
    y = ops.ind_max_pool(x, pools)
    table = ops.neighbor_transpose_supports(pools, n0)
    gx = torch.empty_like(x)

    def pool_bwd(out=gx):
        return ops.ind_max_pool_backward(x, pools, y, gy, transpose=table, out=out)

    def pool_autograd():
        xt = x.detach().clone().requires_grad_(True)
        (torch_max_pool(xt, pools) * gy).sum().backward()
        return xt.grad
    xc = torch.randn((n1, 128), generator=g).to(dev)
    gout = torch.randn((n0, 192), generator=g).to(dev)
    utable = ops.neighbor_transpose_supports(ups[:, :1], n1)
    gu = torch.empty_like(xc)

    def up_bwd(out=gu):
        return ops.closest_pool_cat_backward(gout, ups, n1, 128, transpose=utable, out=out)

    def up_autograd():
        xt = xc.detach().clone().requires_grad_(True)
        (torch_upsample_cat(xt, ups) * gout[:, :128]).sum().backward()
        return xt.grad
    for name, fn, auto, out in (("ind_max_pool_backward", pool_bwd, pool_autograd, gx), ("closest_pool_cat_backward", up_bwd, up_autograd, gu)):
        fn()
        want = auto()
        r = {"difference_to_autograd_over_largest_entry": float((out - want).abs().max() / want.abs().max())}
        held = torch.empty_like(out)
        replay, keep = capture(lambda: fn(held), dev)
        held.fill_(-7.0)
        replay()
        r["graph_replay_equal_to_eager"] = bool(torch.equal(held.view(torch.int32), out.view(torch.int32)))
        times = {"eager": [], "graph": [], "autograd": []}
        for _ in range(WINDOWS):
            times["eager"].append(wall(fn, dev))
            times["graph"].append(wall(replay, dev))
            times["autograd"].append(wall(auto, dev))
        r.update({k: stats(t) for k, t in times.items()})
        report[name] = r
        del keep
    # ---- one whole step ------------------------------------------------------------------------------------------------------------
    W = build_variables(cfg, seed=42, randomize_bn=True).values

    def stand_in(on):
        nb.ind_max_pool_trainable = torch_max_pool if on else ag.ind_max_pool_trainable
        nb.closest_pool_cat_trainable = torch_upsample_cat if on else ag.closest_pool_cat_trainable
    models = {}
    for variant in ("device", "torch_stand_in"):
        m = KernelPointFCNN(iter(()), cfg, weights=dict(W), device=dev)
        m.dropout_prob = 0.5
        models[variant] = (m, MomentumSGD(m.variables, 0.1, 0.98, 100.0))
    times = {v: {"forward": [], "backward": [], "optimiser": []} for v in models}
    try:
        for w in range(WINDOWS + 1):                                              # (window 0 warms up and is dropped)
            for variant, (m, opt) in models.items():
                stand_in(variant == "torch_stand_in")
                t = (wall(lambda: m.run(flat), dev), wall(m.backward, dev), wall(opt.step, dev))
                if w:
                    for k, v in zip(("forward", "backward", "optimiser"), t):
                        times[variant][k].append(v)
    finally:
        stand_in(False)
    report["step"] = {v: {k: stats(t) for k, t in d.items()} for v, d in times.items()}
    report["step"]["loss_after_windows"] = {v: float(m.loss) for v, (m, _) in models.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: (vv["median_ms"] if isinstance(vv, dict) and "median_ms" in vv else vv)
                                                             for kk, vv in v.items()}) for k, v in report.items() if k != "step"}))
    print(json.dumps({v: {k: s["median_ms"] for k, s in d.items()} for v, d in report["step"].items() if v != "loss_after_windows"}))


if __name__ == "__main__":
    main()
