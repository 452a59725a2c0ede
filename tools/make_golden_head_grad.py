#!/usr/bin/env python
"""Writes tests/golden/head_grad.npz: the case grid of tests/head_grad_np.py (GRID) for the backward of the detection head --

  names, seeds           the cases and the seeds head_grad_np.grid_case found (the first from the nominal seed on that keeps margins())
  margin_names, margins  the margins of every case
  err32, largest         per case and evaluation ((gdesc, 0), (0, gscore), both): the largest deviation of float32 torch-CPU autograd
                         of the restated head (head_grad_np.torch_head) from float64 autograd, and the largest float64 entry, over the
                         rows compared absolutely (head_grad_np.deviations: without the clamp rows, without the all-non-positive
                         padded cloud)
  err32_clamp, largest_clamp   the same over the clamp rows, per evaluation (they dominate both paths)
  err32_rel              the largest per-entry RELATIVE deviation over the all-non-positive padded cloud (NaN: the case has none)
  gx_<name>_<evaluation> the float64 gradients of head_grad_np.gradients for the cases of head_grad_np.STORED

No GPU, no reference code: numpy and torch on the CPU.

    python tools/make_golden_head_grad.py [--out tests/golden/head_grad.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import head_grad_np as hg  # noqa: E402

MARGIN_NAMES = ("a", "y", "cloud", "ss")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "head_grad.npz"))
    args = ap.parse_args()
    names = list(hg.GRID)
    out = dict(names=np.asarray(names), margin_names=np.asarray(MARGIN_NAMES), evaluations=np.asarray(hg.EVALS))
    seeds, margins = [], []
    err32, largest = np.zeros((len(names), 3)), np.zeros((len(names), 3))
    err32_clamp, largest_clamp = np.zeros((len(names), 3)), np.zeros((len(names), 3))
    err32_rel = np.full((len(names), 3), np.nan)
    for at, name in enumerate(names):
        c = hg.grid_case(name)
        seeds.append(c["seed"])
        margins.append([min(c["margins"][k], 1e300) for k in MARGIN_NAMES])
        neg = hg.NEGATIVE_ROWS.get(name)
        for e, ev in enumerate(hg.EVALS):
            gd, gs = hg.seeds_of(c, ev)
            res = hg.gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])
            t64 = hg.torch_gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])
            t32 = hg.torch_gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"], dtype="float32")
            assert np.abs(res["gx"] - t64).max() <= 1e-12 * np.abs(t64).max(), (name, ev)
            d = hg.deviations(t32, t64, ev, res["clamp"], neg)
            err32[at, e], largest[at, e] = d["main"]
            if "clamp" in d:
                err32_clamp[at, e], largest_clamp[at, e] = d["clamp"]
            if neg is not None:
                assert d["rel_zero_ok"], (name, ev)
                err32_rel[at, e] = d["rel"]
            if name in hg.STORED:
                out["gx_%s_%s" % (name, ev)] = res["gx"]
            print("%-8s %-5s seed %5d  largest %.3e  err32 %.2e of it%s%s" % (
                name, ev, c["seed"], largest[at, e], err32[at, e] / max(largest[at, e], 1e-300),
                "  clamp rows %.2e of %.3e" % (err32_clamp[at, e] / largest_clamp[at, e], largest_clamp[at, e]) if "clamp" in d else "",
                "  relative %.2e" % err32_rel[at, e] if neg is not None else ""))
    out.update(seeds=np.asarray(seeds, np.int64), margins=np.asarray(margins), err32=err32, largest=largest, err32_clamp=err32_clamp,
               largest_clamp=largest_clamp, err32_rel=err32_rel)
    np.savez_compressed(args.out, **out)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
