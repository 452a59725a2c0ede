#!/usr/bin/env python3
"""What does the optimiser's step cost: training.MomentumSGD (torch operations, five or six small kernels per variable) against
training.DeviceMomentumSGD (one call of two launches)?  (One process, one GPU; not bench.py.  The one requirement: the device call is
faster than MomentumSGD.step() in the same run.)

Workload: the variables of the shipped 3DMatch architecture (threedmatch_config, batch-norm statistics randomised), every trainable one
with a gradient of N(0, 0.01) entries, a tenth of them scaled past the clip norm.  Legs, alternated inside the same run, nine windows
each after one dropped warm-up window, wall clock around call + synchronise:

  torch          MomentumSGD.step()
  device         DeviceMomentumSGD.step(), eager
  device_graph   the same step replayed from a captured graph
  device_folded  the same with weights_decay folded in (the variables whose name contains `weights` decayed, the regularisation loss
                 written)
  device_zeroing the same with persistent gradient buffers, zeroed by the step

Before timing, one step of the two classes from the same state is compared: every variable within optimizer_np.bounds plus one rounding
of lr a' (torch's add_ is one fused multiply-add); the largest fraction of the bound is recorded.  Also recorded: the parameter count,
the bytes the definition must move (20 per parameter: g, v, a read, a, v written; 24 with zeroing; the re-read of g and v for the update
is not counted) and the TB/s that makes at each leg's median.

    python tools/optimizer_bench.py [--out profiles/optimizer_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from training_step_bench import capture, wall
from validation_bench import WINDOWS, stats

LR, MOM, CLIP = 0.1, 0.98, 100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    a = ap.parse_args()
    import optimizer_np as onp
    from d3feat_amd.models.variables import VariableStore, build_variables
    from d3feat_amd.training import DeviceMomentumSGD, MomentumSGD
    from d3feat_amd.utils.config import threedmatch_config
    dev = torch.device("cuda", 0)
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    names = [k for k in W if not k.endswith(("kernel_points", "moving_mean", "moving_variance"))]
    rng = np.random.default_rng(0)
    G = {}
    for i, k in enumerate(names):
        g = rng.standard_normal(W[k].shape).astype(np.float32) * np.float32(0.01)
        if i % 10 == 0:
            g *= np.float32(2 * CLIP / max(float(np.sqrt((g.astype(np.float64) ** 2).sum())), 1e-30))
        G[k] = g

    def fresh(grads=True):
        store = VariableStore(values={k: W[k].copy() for k in names}, device=dev, create=False)
        for k in names:
            p = store.parameter(k)
            if grads:
                p.grad = torch.from_numpy(G[k]).to(dev)
        return store
    count = int(sum(W[k].size for k in names))
    report = {"windows": WINDOWS, "variables": len(names), "parameters": count, "largest_variable": int(max(W[k].size for k in names)),
              "bytes_per_step": 20 * count, "bytes_per_step_with_zeroing": 24 * count,
              "timing": "legs alternated, %d windows each after one dropped; wall clock around call + synchronise" % WINDOWS}
    # ---- the two classes from the same state ---------------------------------------------------------------------------------------
    sa, sb = fresh(), fresh()
    MomentumSGD(sa, LR, MOM, CLIP).step()
    DeviceMomentumSGD(sb, LR, MOM, CLIP).step()
    hyper = (LR, MOM, CLIP, 0.0)
    case = onp.step32({k: W[k] for k in names}, G, {k: np.zeros_like(W[k]) for k in names}, hyper)
    worst, clipped, beyond = 0.0, 0, []
    for k, (ba, bv) in onp.bounds(case, hyper).items():
        d = np.abs(sa.parameter(k).detach().cpu().numpy().astype(np.float64) - sb.parameter(k).detach().cpu().numpy())
        bound = bv + onp.U * np.abs(case[3][k]["step"])
        worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
        clipped += int(case[3][k]["clipped"])
        if not (d <= bound).all():
            beyond.append(k)
    report["difference_to_torch_class_over_bound"] = worst
    report["variables_beyond_bound"] = beyond
    report["variables_clipped"] = clipped
    del sa, sb
    # ---- the legs ------------------------------------------------------------------------------------------------------------------
    stores = {"torch": fresh(), "device": fresh(), "device_folded": fresh(), "device_zeroing": fresh()}
    opts = {"torch": MomentumSGD(stores["torch"], LR, MOM, CLIP), "device": DeviceMomentumSGD(stores["device"], LR, MOM, CLIP),
            "device_folded": DeviceMomentumSGD(stores["device_folded"], LR, MOM, CLIP, weights_decay=cfg.weights_decay),
            "device_zeroing": DeviceMomentumSGD(stores["device_zeroing"], LR, MOM, CLIP, persistent_grads=True)}
    legs = {k: o.step for k, o in opts.items()}
    for fn in legs.values():
        fn()
    replay, keep = capture(opts["device"].step, dev)
    legs["device_graph"] = replay
    times = {k: [] for k in legs}
    for w in range(WINDOWS + 1):
        for k, fn in legs.items():
            t = wall(fn, dev)
            if w:
                times[k].append(t)
    report["legs"] = {k: stats(t) for k, t in times.items()}
    for k, s in report["legs"].items():
        s["TB_per_s"] = round((24 if k == "device_zeroing" else 20) * count / (s["median_ms"] * 1e-3) / 1e12, 3)
    report["device_faster_than_torch"] = bool(report["legs"]["device"]["median_ms"] < report["legs"]["torch"]["median_ms"])
    del keep
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k != "legs"}))
    print(json.dumps({k: (s["median_ms"], s["min_ms"], s["max_ms"], s["TB_per_s"]) for k, s in report["legs"].items()}))
    if beyond:                                                        # (the measurement is kept; the run fails)
        raise SystemExit("optimizer_bench: %d variables differ from MomentumSGD by more than their bound: %s" % (len(beyond), beyond[:5]))
    if not report["device_faster_than_torch"]:
        raise SystemExit("optimizer_bench: the device call is not faster than MomentumSGD.step()")


if __name__ == "__main__":
    main()
