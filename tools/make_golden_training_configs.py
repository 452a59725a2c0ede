#!/usr/bin/env python
"""Writes tests/golden/training_configs.npz for the cases of tests/training_network_np.CASES (the training-mode network at other
configuration values, and the default configuration over three optimiser steps):

  seed/<case>                        the weight seed: the first from 0 on at which every discrete decision of the float64 evaluation
                                     (the quantities of tools/make_golden_training_network.py, and under 'closest' the relative gap
                                     between the two smallest squared distances to the kernel points, per KPConv, after the near-tie
                                     slots are replaced) has a margin of at least 100 times the deviation of that quantity between
                                     the float32 and the float64 CPU evaluation -- for a step case at every one of its steps
  rate/<case>                        the learning rate: for a step case the first of 0.01 and 0.001 at which such a seed exists
  margin/<case>/<step>/<quantity>    the margin, and  deviation/<case>/<step>/<quantity>  the float32-against-float64 deviation of it
                                     (training_network_np.margin_table: the larger of the float32 evaluations of that step)
  replaced/<case>/<matrix>/replaced  and  .../valid: the replaced and the valid slots of every matrix a KPConv reads ('closest' cases)
  err32/<case>/<step>/<tensor>       the largest deviation of the float32 torch-CPU trajectory from the float64 one: desc, score, the
                                     four losses, grad/<variable>, moving/<variable>, accum/<variable>, param/<variable>

<step> is 0 for the cases of one step, 0 .. 2 for the step cases.  The file holds the names and the float64 values as two arrays
(training_network_np.load_golden gives the dict).  The seeds and rates found must be the ones
tests/training_network_np.py holds (the tool stops otherwise).  No GPU, no reference code.

    python tools/make_golden_training_configs.py [--out tests/golden/training_configs.npz]
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
RATES = (0.01, 0.001)


def holds(table):
    return all(m > 0 and m >= FACTOR * d for m, d in table.values())


def steps_of(case):
    """-> [(float64 step, float32 step, margin table)] where every step keeps the rule on the table that is recorded, or None."""
    r, r32 = tn.run(case), tn.run(case, "float32")
    if not holds({k: (m, tn.margin_deviation(m, r32["margins"][k])) for k, m in r["margins"].items()}):
        return None                                    # (the forward alone: most seeds leave here, before any trajectory is run)
    out = []
    for step in tn.steps_of(case):
        table = tn.margin_table(case, step)
        if not holds(table):
            return None
        out.append((tn.trajectory(case)[step], tn.trajectory(case, "float32")[step], table))
    return out


def deviations(want, got):
    out = {}
    for k in ("desc", "score", "desc_loss", "det_loss", "regularization_loss", "loss"):
        out[k] = float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max())
    for group, tag in (("grads", "grad"), ("moving", "moving"), ("accum", "accum"), ("param", "param")):
        for name, w in want[group].items():
            out["%s/%s" % (tag, name)] = float(np.abs(np.asarray(got[group][name]) - w).max())
    return out


def search(case, tries):
    for rate in (RATES if case in tn.STEP_RATES else (tn.LEARNING_RATE,)):
        if case in tn.STEP_RATES:
            tn.STEP_RATES[case] = rate
        for seed in range(tries):
            tn.SEEDS[case] = seed
            tn.clear()
            pairs = steps_of(case)
            if pairs is not None:
                return seed, rate, pairs
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "training_configs.npz"))
    ap.add_argument("--tries", type=int, default=1500)
    ap.add_argument("--cases", nargs="*", default=list(tn.CASES))
    args = ap.parse_args()
    out, found = {}, {}
    for case in args.cases:
        hit = search(case, args.tries)
        if hit is None:
            raise SystemExit("%s: no seed below %d passes: drop the case and say so in the module" % (case, args.tries))
        seed, rate, pairs = hit
        found[case] = (seed, rate)
        out["seed/" + case], out["rate/" + case] = np.int64(seed), np.float64(rate)
        worst = np.inf
        for step, (a, b, table) in enumerate(pairs):
            for k, (m, d) in table.items():
                out["margin/%s/%d/%s" % (case, step, k)] = m
                out["deviation/%s/%d/%s" % (case, step, k)] = d
                worst = min(worst, m / max(d, 1e-300))
            for k, v in deviations(a, b).items():
                out["err32/%s/%d/%s" % (case, step, k)] = v
        for k, v in tn.geometry(case)["replaced"].items():
            out["replaced/%s/%s/replaced" % (case, k)], out["replaced/%s/%s/valid" % (case, k)] = v
        print("%s: seed %d, learning rate %g, smallest margin / deviation %.1f, replaced %s" %
              (case, seed, rate, worst, {k: v for k, v in tn.geometry(case)["replaced"].items() if v[0]}), flush=True)
    import importlib
    fresh = importlib.reload(tn)
    held = {c: (fresh.SEEDS[c], fresh.learning_rate(c)) for c in args.cases}
    if found != held:
        raise SystemExit("tests/training_network_np.py holds %r, the search gives %r: edit the module" % (held, found))
    if args.cases == list(fresh.CASES):
        # five thousand scalars: one array of names and one of float64 values (an archive member each would cost 1.8 MB of headers)
        np.savez_compressed(args.out, names=np.asarray(list(out)), values=np.asarray([float(v) for v in out.values()], np.float64))
        print("wrote %s (%d entries, %d bytes)" % (args.out, len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
