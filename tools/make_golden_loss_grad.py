#!/usr/bin/env python3
"""tests/golden/loss_grad.npz: the yardsticks of the loss-gradient tests (tests/test_loss_grad_host.py, tests/test_gpu_loss_grad.py).

The reference cannot emit these numbers: its gradients come from TensorFlow's autodiff, TensorFlow is not installed here and the numpy
stand-in oracle/tf_eager has no gradients.  What is recorded instead, per case of the size grid of the GPU test (C in 16 / 32 / 64, n
in 1, 2, 63, 64, 65, 256, 1024, both descriptor losses, det_loss_weight 0 and 1; the inputs are validation_np.make_case of the
recorded seed, found by loss_grad_np.clean_case):

    err32       the largest absolute difference, features and scores, between the FLOAT32 torch-CPU autograd evaluation of the restated
                loss (loss_grad_np.torch_gradients: utils/loss.py line by line) and the float64 definition loss_grad_np.gradients --
                "float32 run the plain way", the yardstick the device's error is held against (four times it);
    largest     the largest absolute gradient entry, features and scores (float64);
    margins     the five margins of loss_grad_np.margins;
    seed        the seed clean_case settled on.

and for a few small cases the float64 gradients themselves (features, scores), so that a change of loss_grad_np shows.  Only arrays go
into the fixture.  No part of the reference is read.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import loss_grad_np as lg

OUT = os.path.join(ROOT, "tests", "golden", "loss_grad.npz")
GRID_C, GRID_N = (16, 32, 64), (1, 2, 63, 64, 65, 256, 1024)
LOSSES, WEIGHTS = ("circle_loss", "desc_loss"), (0.0, 1.0)
SAFE_RADIUS, KEYPTS_NUM = 0.1, 2
KEPT = ((32, 2), (32, 65), (16, 64))          # (C, n) whose float64 gradients are stored whole
MARGINS = ("fp_cn", "kd", "argmin", "hinge_pos", "hinge_neg")


def grid_case(C, n):
    """The case of the size grid: a 0.4 m cube (the safe radius masks a few percent), noise 1.6 (about half of the rows accurate)."""
    return lg.clean_case(100 * C + n, n, C, SAFE_RADIUS, cube=0.4, noise=1.6)


def main():
    keys, err32, largest, margins, seeds, kept = [], [], [], [], [], {}
    for C in GRID_C:
        for n in GRID_N:
            t = time.time()
            case, DKD, mg = grid_case(C, n)
            f, s, x, ai, pi = case
            seed = next(100 * C + n + 1000 * k for k in range(40)
                        if np.array_equal(lg.vnp.make_case(100 * C + n + 1000 * k, n, C, cube=0.4, noise=1.6)[0], f))
            for loss in LOSSES:
                for w in WEIGHTS:
                    want = lg.gradients(f, s, x, ai, pi, SAFE_RADIUS, KEYPTS_NUM, w, loss=loss, DKD=DKD)
                    gf, gs = lg.torch_gradients(f, s, x, ai, pi, SAFE_RADIUS, KEYPTS_NUM, w, loss=loss, dtype="float32")
                    keys.append((C, n, LOSSES.index(loss), int(w)))
                    err32.append((np.abs(gf - want["features"]).max(), np.abs(gs - want["scores"]).max()))
                    largest.append((np.abs(want["features"]).max(), np.abs(want["scores"]).max()))
                    margins.append([mg[k] for k in MARGINS])
                    seeds.append(seed)
                    if (C, n) in KEPT:
                        tag = "C%d_n%d_%s_w%d" % (C, n, loss, int(w))
                        kept["features_" + tag], kept["scores_" + tag] = want["features"], want["scores"]
            print("C=%2d n=%4d seed %6d  float32 torch - float64: features %.2e scores %.2e  (largest %.2e %.2e)  %.1f s" % (
                C, n, seed, max(e[0] for e in err32[-4:]), max(e[1] for e in err32[-4:]), max(g[0] for g in largest[-4:]),
                max(g[1] for g in largest[-4:]), time.time() - t), flush=True)
    np.savez_compressed(OUT, keys=np.asarray(keys, np.int32), err32=np.asarray(err32, np.float64), largest=np.asarray(largest, np.float64),
                        margins=np.asarray(margins, np.float64), seeds=np.asarray(seeds, np.int64), margin_names=np.asarray(MARGINS),
                        safe_radius=np.float32(SAFE_RADIUS), keypts_num=np.int32(KEYPTS_NUM), **kept)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
