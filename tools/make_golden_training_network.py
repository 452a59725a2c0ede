#!/usr/bin/env python
"""Writes tests/golden/training_network.npz for the shared case of tests/training_network_np.py (the whole training-mode network and one
resnetb_strided block, with batch norm and without):

  seed/<bn|off>                 the weight seed: the first from 0 on at which every discrete decision of the float64 evaluation -- the
                                LeakyReLU pre-activations, the row sums entering each KPConv, the gap between the largest and the
                                second-largest distinct value of every max-pooled entry, the margins of the detection head
                                (head_grad_np.margins' quantities) and of the loss (loss_grad_np.margins) -- has a margin of at least 100 times the
                                deviation of that quantity between the float32 and the float64 CPU evaluation
  margin/<bn|off>/<quantity>    the margin, and  deviation/<bn|off>/<quantity>  the float32-against-float64 deviation of it
  err32/<case>/<tensor>         per compared tensor the largest deviation of float32 torch-CPU autograd of the composition from float64,
                                <case> = net/<bn|off> (desc, score, the four losses, grad/<variable>, moving/<variable>) or
                                strided/<bn|off>/<widen|same> (out, gfeat, grad/..., moving/...)

The seeds found must be the WEIGHT_SEEDS of tests/training_network_np.py (the tool stops otherwise).  No GPU, no reference code.

    python tools/make_golden_training_network.py [--out tests/golden/training_network.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import training_network_np as tn  # noqa: E402

FACTOR = 100.0
TAG = {True: "bn", False: "off"}


def margin_table(use_bn):
    """-> {quantity: (margin, float32 deviation)} of the whole network at the module's current seed."""
    r, r32 = tn.run(use_bn), tn.run(use_bn, "float32")
    return {k: (r["margins"][k], tn.margin_deviation(r["margins"][k], r32["margins"][k])) for k in r["margins"]}


def holds(table):
    return all(m > 0 and m >= FACTOR * d for m, d in table.values())


def deviations(want, got):
    out = {}
    for k, v in want.items():
        if k in ("grads", "moving"):
            for name, w in v.items():
                out["%s/%s" % (k[:-1] if k == "grads" else k, name)] = float(np.abs(np.asarray(got[k][name]) - w).max())
        elif k != "margins":
            out[k] = float(np.abs(np.asarray(got[k]) - np.asarray(v)).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "training_network.npz"))
    ap.add_argument("--tries", type=int, default=400)
    args = ap.parse_args()
    out = {}
    for use_bn in (True, False):
        for seed in range(args.tries):
            tn.WEIGHT_SEEDS[use_bn] = seed
            tn.variables.cache_clear()
            tn.run.cache_clear()
            table = margin_table(use_bn)
            if holds(table):
                break
        else:
            raise SystemExit("no seed below %d passes at first_features_dim = %d" % (args.tries, tn.FDIM))
        print("%s: seed %d, smallest margin / deviation %.1f" % (TAG[use_bn], seed, min(m / max(d, 1e-300) for m, d in table.values())))
        out["seed/" + TAG[use_bn]] = np.int64(seed)
        for k, (m, d) in table.items():
            out["margin/%s/%s" % (TAG[use_bn], k)] = m
            out["deviation/%s/%s" % (TAG[use_bn], k)] = d
        for k, v in deviations(tn.run(use_bn), tn.run(use_bn, "float32")).items():
            out["err32/net/%s/%s" % (TAG[use_bn], k)] = v
        for widen in (True, False):
            for k, v in deviations(tn.strided(use_bn, widen), tn.strided(use_bn, widen, "float32")).items():
                out["err32/strided/%s/%s/%s" % (TAG[use_bn], "widen" if widen else "same", k)] = v
    found = {b: int(out["seed/" + TAG[b]]) for b in (True, False)}
    import importlib
    fresh = importlib.reload(tn).WEIGHT_SEEDS
    if found != fresh:
        raise SystemExit("tests/training_network_np.py holds WEIGHT_SEEDS = %r, the search gives %r: edit the module" % (fresh, found))
    np.savez(args.out, **out)
    print("wrote %s (%d entries, %d bytes)" % (args.out, len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
