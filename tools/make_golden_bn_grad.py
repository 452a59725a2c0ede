#!/usr/bin/env python
"""Writes tests/golden/bn_grad.npz: the case grid of tests/bn_grad_np.py (GRID) for batch normalisation in training mode and its
backward --

  keys                     the case names
  "block/<block>/<bn|off>/<output>"   err32 of the whole blocks of tests/training_blocks_np.py in training mode: the output, the
                           gradient of sum(out R) with respect to the input features (gfeat) and to every variable (its full name)
  "<case>/<output>"        err32 of the output (y, gx, ggamma, gbeta, gres; those the case has): the largest deviation of float32
                           torch-CPU autograd of the restated layer (bn_grad_np.torch_block) from float64 autograd -- one figure per
                           COLUMN for y, gx and gres (the device tests compare those per column), one figure otherwise

No GPU, no reference code: numpy and torch on the CPU.

    python tools/make_golden_bn_grad.py [--out tests/golden/bn_grad.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn_grad_np as bg  # noqa: E402
import training_blocks_np as tb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bn_grad.npz"))
    args = ap.parse_args()
    store = dict(keys=np.asarray(list(bg.GRID)))
    for name in bg.GRID:
        c = bg.grid_case(name)
        fw, bw = bg.grid_reference(name)
        want = dict(bw, y=fw["y"])
        t64, t32 = bg.torch_gradients(c), bg.torch_gradients(c, dtype="float32")
        scales = bg.term_scales(c, fw, bw)
        line = []
        for out in bg.OUTPUTS:
            if t64[out] is None:
                continue
            big = np.abs(t64[out]).max()
            assert np.abs(want[out] - t64[out]).max() <= 1e-12 * max(big, scales[out]), (name, out)
            err = np.abs(t32[out] - t64[out])
            store["%s/%s" % (name, out)] = err.max(0) if out in bg.PER_COLUMN else err.max()
            line.append("%s %.1e" % (out, err.max() / big) if big > 0 else "%s (all zero)" % out)
        print("%-14s err32 / largest: %s" % (name, "  ".join(line)))
    for name in tb.BLOCKS:
        for use_bn in (True, False):
            t64, t32 = tb.torch_reference(name, use_bn), tb.torch_reference(name, use_bn, dtype="float32")
            pairs = [("out", t32["out"], t64["out"]), ("gfeat", t32["gfeat"], t64["gfeat"])] + [(k, t32["grads"][k], t64["grads"][k]) for k in t64["grads"]]
            for label, a, b in pairs:
                store["block/%s/%s/%s" % (name, "bn" if use_bn else "off", label)] = np.abs(a - b).max()
            print("%-18s %-3s err32 / largest: %s" % (name, "bn" if use_bn else "off", "  ".join(
                "%s %.1e" % (label.split("/", 2)[-1], np.abs(a - b).max() / np.abs(b).max()) for label, a, b in pairs)))
    np.savez_compressed(args.out, **store)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
