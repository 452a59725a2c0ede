#!/usr/bin/env python
"""Writes tests/golden/kpconv_grad.npz: the case grid of tests/kpconv_grad_np.py (GRID) for the backward of the rigid KPConv --

  keys            "<case>/<influence>/<aggregation>" for every case and each of its modes
  outputs         ("gf", "gW")
  err32, largest  per key and output: the largest deviation of float32 torch-CPU autograd of the restated operator
                  (kpconv_grad_np.torch_kpconv) from float64 autograd, and the largest float64 entry

No GPU, no reference code: numpy and torch on the CPU.

    python tools/make_golden_kpconv_grad.py [--out tests/golden/kpconv_grad.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kpconv_grad_np as kg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kpconv_grad.npz"))
    args = ap.parse_args()
    keys, err32, largest = [], [], []
    for name in kg.GRID:
        c = kg.grid_case(name)
        W, gout = kg.grid_operands(name)
        for influence, aggregation in kg.modes_of(name):
            res = kg.grid_gradients(name, influence, aggregation)
            t64 = kg.torch_gradients(c, W, gout, influence, aggregation)
            t32 = kg.torch_gradients(c, W, gout, influence, aggregation, dtype="float32")
            for got, want in zip((res["gf"], res["gW"]), t64):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, influence, aggregation)
            keys.append("%s/%s/%s" % (name, influence, aggregation))
            err32.append([np.abs(a - b).max() for a, b in zip(t32, t64)])
            largest.append([np.abs(b).max() for b in t64])
            print("%-28s gf largest %.3e err32 %.2e of it   gW largest %.3e err32 %.2e of it" % (
                keys[-1], largest[-1][0], err32[-1][0] / largest[-1][0], largest[-1][1], err32[-1][1] / largest[-1][1]))
    np.savez_compressed(args.out, keys=np.asarray(keys), outputs=np.asarray(["gf", "gW"]), err32=np.asarray(err32),
                        largest=np.asarray(largest))
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
