#!/usr/bin/env python3
"""The decoder's unary blocks launch by launch: the one-launch form (ops.gemm_upsample_cat over [ x'[up[m, 0]] | skip[m] ]) against
the split form (ops.gemm_upsample_split: Y = x @ W1 over the coarse rows, then skip @ W2 + Y[up[m, 0]] over the fine ones), in one
process, alternated, HIP-event timed.  Shapes: the decoder of the default run (F = 12 fragments per replay,
profiles/r06_v37_bench_default_detail.json roofline.contraction_launches).  Level 0 runs on the resident-W form and is not taken
in split form by the model (ops._split_ok); its pair is timed here all the same, with the predicate overridden.
    python tools/decoder_split_bench.py [rounds [reps]]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3feat_amd import ops  # noqa: E402

# (level, fine rows M, coarse rows n1, C1, C2, N)
LEVELS = [(3, 10860, 2370, 2048, 1024, 512), (2, 43590, 10860, 512, 512, 256), (1, 174966, 43590, 256, 256, 128),
          (0, 704868, 174966, 128, 128, 64)]


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3   # us


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    print("%d rounds of %d calls per form, alternated; us per call: median (min .. max)" % (rounds, reps))
    print("level      M     n1    C1    C2    N   fused                      split (both launches)      coarse   fine   split/fused")
    for level, M, n1, C1, C2, N in LEVELS:
        x = torch.randn(n1, C1, device=dev)
        skip = torch.randn(M, C2, device=dev)
        # a fine row's nearest coarse row, in the spatially coherent order both levels are stored in, with some scatter
        near = (np.arange(M, dtype=np.int64) * n1 // M + rng.integers(-40, 41, M)).clip(0, n1)
        idx = torch.from_numpy(np.stack([near, near, near], 1).astype(np.int32)).to(dev)
        W = torch.randn(C1 + C2, N, device=dev) / (C1 + C2) ** 0.5
        W1, W2 = W[:C1].contiguous(), W[C1:].contiguous()
        scale, shift = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev)
        u = ops.UpsampleCat(x, idx, skip)
        forced = not ops.upsample_split_ok(u, N)
        ok = ops.upsample_split_ok
        fused = lambda: ops.gemm_upsample_cat(u, W, col_scale=scale, col_shift=shift, leaky=True)       # noqa: E731
        split = lambda: ops.gemm_upsample_split(u, W1, W2, col_shift=shift, leaky=True)                 # noqa: E731
        coarse = lambda: ops.gemm(x, W1)                                                                # noqa: E731
        if forced:
            ops.upsample_split_ok = lambda u_, n_: True
        try:
            for f in (fused, split, coarse):
                for _ in range(3):
                    f()
            tf, ts, tc = [], [], []
            for _ in range(rounds):
                tf.append(_time(fused, reps))
                ts.append(_time(split, reps))
                tc.append(_time(coarse, reps))
        finally:
            ops.upsample_split_ok = ok
        mf, ms, mc = statistics.median(tf), statistics.median(ts), statistics.median(tc)
        print("%5d %6d %6d %5d %5d %4d   %7.1f (%6.1f .. %6.1f)   %7.1f (%6.1f .. %6.1f)   %6.1f %6.1f   %.3f%s"
              % (level, M, n1, C1, C2, N, mf, min(tf), max(tf), ms, min(ts), max(ts), mc, ms - mc, ms / mf,
                 "   (predicate overridden: not taken by the model)" if forced else ""), flush=True)
    # the last unary block (704868 x 64 -> 32) is not a decoder contraction over an upsampled operand: no split form
    A, B = torch.randn(704868, 64, device=dev), torch.randn(64, 32, device=dev)
    last = lambda: ops.gemm(A, B)                                                                       # noqa: E731
    for _ in range(3):
        last()
    tl = [_time(last, reps) for _ in range(rounds)]
    print("last unary 704868 x 64 -> 32 (unchanged): %.1f (%.1f .. %.1f)" % (statistics.median(tl), min(tl), max(tl)))


if __name__ == "__main__":
    main()
