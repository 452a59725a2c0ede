#!/usr/bin/env python3
"""The two chained pairs of level 0 launch by launch (ops.gemm_chain against the two launches it replaces), HIP-event timed:
(a) decoder [up(L1) 128 | skip 128] -> 64 (BN, LeakyReLU) -> 32, first output not stored; (b) encoder [x 32 | f 64] -> 128 (shift,
LeakyReLU), stored, -> 32 (BN, LeakyReLU).  Rows of level 0 at F = 12 and F = 7 fragments per replay.  Per variant the median (min,
max) of seven alternated windows of ten calls, and the first launch alone beside them.
    python tools/gemm_chain_bench.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3feat_amd import ops

dev = torch.device("cuda", 0)
g = torch.Generator(device="cpu").manual_seed(1)
def rnd(*s): return torch.randn(*s, generator=g).to(dev)

def window(fn, reps=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3

res = {}
for F, M in ((12, 704868), (7, 412762)):
    M1 = M // 4
    # (a) decoder: [up(L1) 128 | skip 128] -> 64 (BN, leaky) -> 32
    x, skip = rnd(M1, 128), rnd(M, 128)
    idx = torch.randint(0, M1, (M, 3), dtype=torch.int32).to(dev); idx[:, 0] = (torch.arange(M) // 4).clamp(max=M1 - 1).to(torch.int32).to(dev)
    W, W2 = rnd(256, 64) / 16, rnd(64, 32) / 8
    s1, t1 = rnd(64) * 0.1 + 1, rnd(64) * 0.1
    u = ops.UpsampleCat(x, idx, skip)
    def two_a():
        y = ops.gemm_upsample_cat(u, W, col_scale=s1, col_shift=t1, leaky=True)
        return ops.gemm(y, W2)
    def first_a(): return ops.gemm_upsample_cat(u, W, col_scale=s1, col_shift=t1, leaky=True)
    def chain_a(): return ops.gemm_chain(x, W, W2, idx=idx, skip=skip, store_first=False, col_scale=s1, col_shift=t1, leaky=True)[1]
    # (b) encoder: [x 32 | f 64] -> 128 (shift, leaky), stored, -> 32 (BN, leaky)
    a1, a2 = rnd(M, 32), rnd(M, 64)
    Wb, Wb2 = rnd(96, 128) / 10, rnd(128, 32) / 11
    tb, s2, t2 = rnd(128) * 0.1, rnd(32) * 0.1 + 1, rnd(32) * 0.1
    def two_b():
        y = ops.gemm_cat2(a1, a2, Wb, col_shift=tb, leaky=True)
        return ops.gemm(y, Wb2, col_scale=s2, col_shift=t2, leaky=True)
    def first_b(): return ops.gemm_cat2(a1, a2, Wb, col_shift=tb, leaky=True)
    def chain_b(): return ops.gemm_chain(a1, Wb, Wb2, skip=a2, store_first=True, col_shift=tb, leaky=True, col_scale2=s2, col_shift2=t2, leaky2=True)[1]
    d = (chain_a() - two_a()).abs().max().item(), (chain_b() - two_b()).abs().max().item()
    out = {"max_abs_diff_chain_vs_two": d}
    fns = dict(a_two=two_a, a_first_alone=first_a, a_chain=chain_a, b_two=two_b, b_first_alone=first_b, b_chain=chain_b)
    for k, fn in fns.items(): window(fn, 3)
    t = {k: [] for k in fns}
    for w in range(7):
        for k, fn in fns.items(): t[k].append(window(fn))
    for k in fns:
        v = sorted(t[k]); out[k] = {"median_us": round(v[3], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
    res["F=%d M=%d" % (F, M)] = out
    del x, skip, idx, a1, a2
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res, indent=1))
