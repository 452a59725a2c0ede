#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of every KPConv aggregation entry point on the synthetic cases of the branch tests
(oracle/kpconv_cases.py, tests/deformable_cases.py): {entry point: {instantiation: {case: digest}}}, one line per instantiation.
Two builds of the library that run the same arithmetic write the same file:

    D3FEAT_AMD_LIB=/path/to/other/libd3feat_amd.so python tools/kpconv_bits.py other.json
    python tools/kpconv_bits.py this.json            (separate processes: the variable is read at import)

Entry points: kpconv_aggregate (fp32, bf16 feature rows, the scalar kernel), kpconv_fused32 and kpconv_fused in both contraction
forms (fp32 MFMA / _x3) with fp32 and bf16 feature rows, kpconv_deform_aggregate (with and without modulations, the scalar kernel).
Cases as the tests visit them: every (Nq, K) of the generators but K = 0 (no neighbour loop runs) with the configurations of the
instantiation in turn; the last case with every configuration, and again with a q_order permutation in capacity mode (`+oc`:
Nq_dev / Ns_dev; only the rows below Nq_dev are hashed, the others are never written)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from d3feat_amd import _lib, ops  # noqa: E402
from oracle import kpconv_cases as kc  # noqa: E402
import deformable_cases as dc  # noqa: E402

FAST = ("linear", "sum", 15)
NONFAST = (("gaussian", "sum", 13), ("linear", "closest", 15), ("constant", "sum", 4))
NONFAST_DEFORM = NONFAST + (("gaussian", "closest", 15), ("constant", "closest", 13), ("linear", "sum", 4))
LQS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
dev = torch.device("cuda", 0)
out = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def record(entry, inst, case, fn, c, bf16=False, special=False):
    """fn(q, s, idx, f) -> tensor(s).  special: the capacity rows stay, Nq_dev / Ns_dev name the counts, q_order is a permutation."""
    nq, ns = (len(c.q), len(c.s)) if special else (c.Nq, c.Ns)
    q, s, idx, f = _t(c.q[:nq]), _t(c.s[:ns]), _t(c.idx[:nq]), _t(c.f[:ns])
    if bf16:
        f = f.to(torch.bfloat16)
    if special:
        q.n_dev = torch.tensor([c.Nq], dtype=torch.int32, device=dev)
        s.n_dev = torch.tensor([c.Ns], dtype=torch.int32, device=dev)
        q.order = _t(np.random.default_rng(c.Nq + idx.shape[1]).permutation(c.Nq).astype(np.int32))
    r = fn(q, s, idx, f)
    h = hashlib.sha256()
    for t in (r if isinstance(r, tuple) else (r,)):
        t = t[:c.Nq]
        h.update((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().cpu().numpy().tobytes())
    out.setdefault(entry, {}).setdefault(inst, {})[case + ("+oc" if special else "")] = h.hexdigest()


def visits(shapes, cfgs):
    """-> (Nq, K, cfg, special) in the tests' order: the configurations in turn, the last shape with all of them, plain and special."""
    shapes = [(nq, k) for nq, k in shapes if k > 0]
    for j, (Nq, K) in enumerate(shapes[:-1]):
        yield Nq, K, cfgs[j % len(cfgs)], False
    for cfg in cfgs:
        for special in (False, True):
            yield shapes[-1] + (cfg, special)


def name(Nq, K, cfg, *more):
    return "-".join(["%dx%d" % (Nq, K), cfg[0][:3], cfg[1][:3], str(cfg[2])] + [m for m in more if m])


def aggregate():
    for LQ in LQS:
        for inst, cfgs, bf16 in (("kpconv_agg_vec4<%d,true>" % LQ, (FAST,), False), ("kpconv_agg_vec4<%d,false>" % LQ, NONFAST, False),
                                 ("kpconv_agg_vec4<%d,true,bf16>" % LQ, (FAST,), True)):
            if bf16 and LQ not in (64, 128):
                continue
            for Nq, K, cfg, special in visits(kc.shapes_of("agg_vec4", 4 * LQ), cfgs):
                c = kc.shape_case("agg_vec4", 4 * LQ, Nq, K, num_kp=cfg[2], bf16=bf16)
                record("aggregate", inst, name(Nq, K, cfg), lambda q, s, idx, f: ops.kpconv_aggregate(q, s, idx, f, c.KP, kc.EXTENT, cfg[0], cfg[1]),
                       c, bf16, special)
    for Cin in (6, 1):
        for j, cfg in enumerate((FAST,) + NONFAST):
            Nq, K = kc.shapes_of("agg_scalar", Cin)[j % 2]
            c = kc.shape_case("agg_scalar", Cin, Nq, K, num_kp=cfg[2])
            record("aggregate", "kpconv_agg_scalar", name(Nq, K, cfg, "Cin%d" % Cin),
                   lambda q, s, idx, f: ops.kpconv_aggregate(q, s, idx, f, c.KP, kc.EXTENT, cfg[0], cfg[1]), c)


def fused(kernel, Cin, cfgs, bf16, inst):
    fn = ops.kpconv_fused32 if kernel == "fused32" else ops.kpconv_fused
    keep = ops.KP_X3
    try:
        for x3 in (False, True):
            ops.KP_X3 = x3
            for Nq, K, cfg, special in visits(kc.shapes_of(kernel, Cin), cfgs):
                c = kc.shape_case(kernel, Cin, Nq, K, num_kp=cfg[2], bf16=bf16)
                W = _t(kc.weights(Cin + K, cfg[2], Cin, Cin))
                record(kernel + ("_x3" if x3 else ""), inst, name(Nq, K, cfg),
                       lambda q, s, idx, f: fn(q, s, idx, f, c.KP, W, kc.EXTENT, cfg[0], cfg[1], leaky=True), c, bf16, special)
    finally:
        ops.KP_X3 = keep


def deform():
    def call(c, cfg, modulated):
        raw = c.raw[:, :(4 if modulated else 3) * cfg[2]]
        return lambda q, s, idx, f: ops.kpconv_deform_aggregate(q, s, idx, f, c.KP, _t(raw[:q.shape[0]]), dc.EXTENT, cfg[0], cfg[1], raw=True)
    for i, LQ in enumerate(LQS):
        for inst, cfgs in (("kpconv_deform_agg_vec4<%d,true>" % LQ, (FAST,)),
                           ("kpconv_deform_agg_vec4<%d,false>" % LQ, tuple(NONFAST_DEFORM[(i + k) % 6] for k in (0, 2, 4)))):
            last = dc.shapes(LQ)[-1]
            for j, (Nq, K, cfg, special) in enumerate(visits(dc.shapes(LQ), cfgs)):
                c = dc.shape_case("agg_vec4", 4 * LQ, Nq, K, num_kp=cfg[2])
                for modulated in ((False, True) if (Nq, K) == last else (j % 2 == 0,)):
                    record("deform_aggregate", inst, name(Nq, K, cfg, "mod" if modulated else ""), call(c, cfg, modulated), c, special=special)
    for j, cfg in enumerate((FAST,) + NONFAST_DEFORM):
        Nq, K = ((37, 9), (3, 5))[j % 2]
        c = dc.shape_case("agg_scalar", 6, Nq, K, num_kp=cfg[2])
        record("deform_aggregate", "kpconv_deform_agg_scalar", name(Nq, K, cfg, "mod" if j % 2 else ""), call(c, cfg, j % 2 == 1), c)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "kpconv_bits.json"
    aggregate()
    fused("fused32", 32, (FAST,), False, "kpconv_fused32_kernel<true,4,float>")
    fused("fused32", 32, NONFAST, False, "kpconv_fused32_kernel<false,8,float>")
    fused("fused32", 32, (FAST,), True, "kpconv_fused32_kernel<true,4,bf16>")
    for LQ in (16, 32, 64):
        for bf16 in (False, True):
            fused("fused", 4 * LQ, (FAST,), bf16, "kpconv_fused_kernel<%d,4,%s>" % (LQ, "bf16" if bf16 else "float"))
    deform()
    torch.cuda.synchronize()
    with open(path, "w") as fh:          # (nothing about the library: equal builds write equal files)
        fh.write("{\n" + ",\n".join(' %s: {\n%s\n }' % (json.dumps(e), ",\n".join("  %s: %s" % (json.dumps(i), json.dumps(d)) for i, d in v.items()))
                                    for e, v in out.items()) + "\n}\n")
    n = sum(len(d) for v in out.values() for d in v.values())
    print("%d digests of %d instantiations -> %s (%s)" % (n, sum(len(v) for v in out.values()), path, _lib.LIB_PATH))


if __name__ == "__main__":
    main()
