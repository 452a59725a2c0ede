"""Every instantiation of d3f_kpconv_deform_aggregate (csrc/kpconv_deform.hip) through the C ABI against the float64 mask form of
kernels/convolution_ops.py:379-490 (tests/deformable_np.kpconv_deform_f64) on synthetic inputs (tests/deformable_cases.py), in the
conventions of tests/test_gpu_kpconv_branches.py.

The launcher chooses a kernel by channel count, alignment, leading dimension and kernel-point configuration:
    vec = Cin % 4 == 0 && ldf % 4 == 0 && (f & 15) == 0 && (wf & 15) == 0 && kp_fits_u24;   fast = 15 points && linear && sum
    vec && Cin == 4 LQ -> kpconv_deform_agg_vec4<LQ, fast>, LQ in {1, 2, 4, 8, 16, 32, 64, 128, 256};   else kpconv_deform_agg_scalar
Shapes: Nq in {1, TQ - 1, 3 TQ + 5} (TQ = min(256 / LQ, 64) queries per workgroup), K in {1, LQ - 1, LQ + 1, 2 LQ + 3} around the
neighbour chunk, Cin in {4, 32, 64, 128, 256, 512, 1024} and (LQ = 2, 4: their own thread counts) {8, 16}; Cin = 6 and misaligned
views for the scalar form; 15, 13 and 4 kernel points.  Argument variants: capacity mode (Nq_dev / Ns_dev), q_order, strided ldf,
ld_idx > K, ld_off > 4 num_kp.  Padding columns of every strided view and capacity rows hold NaN, padding columns of the index matrix
0x3fffffff, outputs are pre-filled with a sentinel: a kernel that reads or writes outside its operands poisons its result.
Not covered: kp_fits_u24 false (an index stride of 2^24 needs a 128 MB allocation; the predicate and the kernel it selects are
the ones test_aggregate_scalar runs).

Bar for wf (derived, not measured; deformable_np.wf_bound, u = 2^-24, e = KP_extent, m = the query's largest |offset|, D = d / e)
----------------------------------------------------------------------------------------------------------------------------------
It is the bound of tests/test_gpu_kpconv_branches.py with the extra roundings of this kernel:
  * the deformed point kp' = kp + raw * e costs a product and an add: |delta kp'_i| <= u (|off_i| + |kp'_i|); with r = s - q and
    d_i = r_i - kp'_i one rounding each, |delta d| <= u (|r| + |d| + |off| + |kp'|).  Where h > 0: |d| < e (not 2 e: the division is by
    e, which doubles every D term of an absolute error), |kp'| <= 1.5 e + m takes the place of 1.5 e, |r| <= |d| + |kp'|:
    <= u (5 e + 3 m) = (5 + 3 m / e) u in D   (rigid: 2.75 u);
  * d2 (<= 6 roundings): 3 u in D;  v_sqrt, 1 ulp: 2 u;  1 / e rounded once: u;  h = fma(-sqrt, 1 / e, 1) or product + subtraction: 2 u.
    'linear'   |delta h| <= (13 + 3 m / e) u = (6.5 + 1.5 m / e) 2^-23
    'gaussian' |delta h| <= (8.05 + 3.05 m / e) 2^-23   (deformable_np: the inputs' part (7.6 + 6.1 m / e) u, the roundings' 8.5 u)
    'constant' h in {0, 1} is decided by the inputs' margins (deformable_cases condition 1): no error;
  * n FMAs of accumulation over the n neighbours in range (a dropped or shadow slot adds an exact 0): n / 2 * 2^-23 sum_k h_k |f_k|;
  * where a modulation multiplies: one more rounding, and the kernel's own 2 / (1 + expf(-x)) -- expf at 1 ulp, an add, a division:
    <= 5 u relative -- together 3 * 2^-23 mod sum_k h_k |f_k| (0.5 * 2^-23 when the modulations are passed as they are).
  |wf - wf64| <= 2^-23 mod (c_h sum_{k in range} |f_k| + n / 2 sum_k h_k |f_k|) + 3 * 2^-23 mod sum_k h_k |f_k|
Each test prints the largest error / bound it saw and asserts <= 1.

Instantiation -> test (19)
  kpconv_deform_agg_vec4<LQ, true>, <LQ, false>, LQ = 1 .. 256   (18)      test_deform_aggregate_vec4[LQ-FAST], [LQ-general]
  kpconv_deform_agg_scalar   (1)      test_deform_aggregate_scalar[Cin6 / Cin32-ldf33 / Cin32-base+4B]

Measured on an MI355X (the largest ratio over the cases of each kernel; printed by every test, never used as a bar)
  wf error / bound      deform_agg_vec4<LQ, true>, LQ = 1 .. 256:    0.17 0.21 0.14 0.16 0.15 0.13 0.13 0.13 0.11
                        deform_agg_vec4<LQ, false>:                 0.47 0.18 0.52 0.15 0.53 0.14 0.29 0.14 0.23
                        deform_agg_scalar: 0.36 (Cin 6), 0.36 (ldf 33), 0.36 (base + 4 B)
No defect was found.  Cost: the 23 cases take 2 s of GPU suite time (the slowest 0.3 s); nothing allocates more than a few MB.
"""
import math

import numpy as np
import pytest
import torch

import deformable_cases as dc
import deformable_np as dn
from conftest import bits

pytestmark = pytest.mark.gpu

S = -124.0                        # sentinel of pre-filled outputs
OK, ERR_ARG = 0, -3               # D3F_OK, D3F_ERR_ARG (include/d3feat_amd.h)
FAST = ("linear", "sum", 15)      # kp_fast_config: num_kp == 15 && influence == linear && aggregation == sum
NONFAST = (("gaussian", "sum", 13), ("linear", "closest", 15), ("constant", "sum", 4), ("gaussian", "closest", 15),
           ("constant", "closest", 13), ("linear", "sum", 4))
_INF = {"constant": 0, "linear": 1, "gaussian": 2}
_AGG = {"sum": 0, "closest": 1}
NAMES = ("q Nq s Ns idx ld_idx K f ldf Cin off ld_off off_scale mod ld_mod logits kp num_kp extent influence aggregation wf "
         "nq_dev ns_dev order bf16 stream").split()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(v, dev):
    return torch.tensor([int(v)], dtype=torch.int32, device=dev)


def _view(a, dev, ld=None, off=0, fill=np.nan):
    """a [n, C] on the device: contiguous, or (ld given) the column slice [off, off + C) of an [n, ld] matrix filled with `fill`."""
    n, C = a.shape
    if ld is None:
        return _t(a, dev)
    big = np.full((n, ld), fill, a.dtype)
    big[:, off:off + C] = a
    return _t(big, dev)[:, off:off + C]


def _call(a):
    from d3feat_amd import _lib
    vals = []
    for n in NAMES:
        v = a.get(n)
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        elif isinstance(v, np.ndarray):
            v = v.ctypes.data
        vals.append(v)
    return _lib.load().d3f_kpconv_deform_aggregate(*vals)


def _operands(dev, c, cfg, modulated, strided=False, cap=False, order=False, scaled=False):
    """The named C ABI arguments of a case, tensors kept alive in the dict.  cap: the tensors keep their capacity rows and Nq_dev /
    Ns_dev name the effective counts; strided: ld_idx = K + 3 (padding 0x3fffffff), ldf = Cin + 16 and ld_off = D + 5 (padding NaN);
    order: a random permutation as q_order; scaled: offsets in the units of the points and the modulations themselves (float32
    values computed here) instead of the raw output of the offset convolution."""
    from oracle import kpconv_cases as kc
    nq, ns = (len(c.q), len(c.s)) if cap else (c.Nq, c.Ns)
    K, Cin, P = c.idx.shape[1], c.f.shape[1], cfg[2]
    a = dict(Nq=nq, Ns=ns, K=K, Cin=Cin, kp=np.ascontiguousarray(c.KP, np.float32), num_kp=P, extent=dc.EXTENT, influence=_INF[cfg[0]],
             aggregation=_AGG[cfg[1]], bf16=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    a["q"], a["s"] = _t(c.q[:nq], dev), _t(c.s[:ns], dev)
    a["idx"] = _view(c.idx[:nq], dev, K + 3, 2, fill=kc.GARBAGE) if strided else _t(c.idx[:nq], dev)
    a["ld_idx"] = K + 3 if strided else K
    a["f"] = _view(c.f[:ns], dev, Cin + 16 if strided else None, 8)
    a["ldf"] = Cin + 16 if strided else Cin
    D = (4 if modulated else 3) * P
    raw = c.raw[:nq, :D]
    if scaled:
        off = (raw[:, :3 * P] * np.float32(dc.EXTENT)).astype(np.float32)
        a["off"], a["ld_off"], a["off_scale"] = _t(off, dev), 3 * P, 1.0
        if modulated:
            with np.errstate(invalid="ignore"):
                mod = (2.0 / (1.0 + np.exp(-raw[:, 3 * P:].astype(np.float64)))).astype(np.float32)
            a["mod"], a["ld_mod"], a["logits"] = _t(mod, dev), P, 0
            a["_mod_host"] = mod
        a["_off_host"] = off
    else:
        a["off"] = _view(raw, dev, D + 5 if strided else None, 3)
        a["ld_off"], a["off_scale"] = (D + 5 if strided else D), dc.EXTENT
        if modulated:
            a["mod"], a["ld_mod"], a["logits"] = a["off"][:, 3 * P:], a["ld_off"], 1
    a.setdefault("mod", None), a.setdefault("ld_mod", 0), a.setdefault("logits", 0)
    if cap:
        a["nq_dev"], a["ns_dev"] = _i32(c.Nq, dev), _i32(c.Ns, dev)
    if order:
        a["order"] = _t(np.random.default_rng(K + nq).permutation(c.Nq).astype(np.int32), dev)
    return a


def _run(dev, c, cfg, modulated, **kw):
    """-> wf as numpy through the C ABI (sentinel-filled output; rows beyond Nq_dev must keep the sentinel)."""
    a = _operands(dev, c, cfg, modulated, **kw)
    a["wf"] = torch.full((a["Nq"], cfg[2] * c.f.shape[1]), S, dtype=torch.float32, device=dev)
    assert _call(a) == OK
    wf = a["wf"].cpu().numpy()
    assert np.all(wf[c.Nq:] == S)
    return wf, a


def _check(wf, c, cfg, modulated, a=None):
    """wf [>= Nq, P * Cin] against kpconv_deform_f64 -> the largest error / bound (module docstring)."""
    inf, mode, P = cfg
    Nq, Cin = c.Nq, c.f.shape[1]
    scaled = a is not None and "_off_host" in a
    key = (cfg, modulated, scaled)
    memo = c.setdefault("_ref", {})
    if key not in memo:
        if scaled:
            off = a["_off_host"][:Nq].astype(np.float64).reshape(Nq, P, 3)
            mod = a["_mod_host"][:Nq].astype(np.float64) if modulated else None
        else:
            off, mod = dn.deformed_from_raw(c.raw[:Nq], P, dc.EXTENT, modulated)
        args = (c.q, c.s, c.idx, c.f, c.KP, off, mod)
        want = dn.kpconv_deform_f64(*args, None, dc.EXTENT, inf, mode, Nq=Nq, Ns=c.Ns)
        memo[key] = want["wf"], dn.wf_bound(*args, dc.EXTENT, inf, mode, Nq, c.Ns, logits=not scaled)
    want, bound = memo[key]
    assert np.isfinite(wf[:Nq]).all()
    err = np.abs(wf[:Nq].astype(np.float64).reshape(Nq, P, Cin) - want)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _report(name, ratio):
    print("%s: largest error / bound %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound %.3f > 1" % (name, ratio)


def _all(dev, kernel, Cin, cfgs, shapes):
    """Every (Nq, K) of `shapes` with the configurations of `cfgs` in turn, with and without modulations in turn, odd cases on strided
    views; the last (largest) case with every configuration: plain, with q_order (bit-equal), in capacity mode on strided views with
    q_order, and with pre-scaled offsets / given modulations -> largest ratio."""
    worst = 0.0
    for j, (Nq, K) in enumerate(shapes):
        cfg = cfgs[j % len(cfgs)]
        c = dc.shape_case(kernel, Cin, Nq, K, num_kp=cfg[2], self_queries=j % 3 == 2)
        n_in, n_out = dc.in_range_counts(c)
        assert n_in > 0 and n_out > 0 and dc.range_decided(c)              # the test's own inputs
        wf, _ = _run(dev, c, cfg, j % 2 == 0, strided=j % 2 == 1)
        worst = max(worst, _check(wf, c, cfg, j % 2 == 0))
        if j == len(shapes) - 1:
            for i, cfg in enumerate(cfgs):
                if cfg[2] != c.KP.shape[0]:
                    c = dc.shape_case(kernel, Cin, Nq, K, num_kp=cfg[2])
                    assert dc.range_decided(c) and min(dc.in_range_counts(c)) > 0
                for modulated in (True, False):
                    wf, _ = _run(dev, c, cfg, modulated)
                    worst = max(worst, _check(wf, c, cfg, modulated))
                    wo, _ = _run(dev, c, cfg, modulated, order=True)
                    assert np.array_equal(bits(wo), bits(wf))
                wc, _ = _run(dev, c, cfg, True, strided=True, cap=True, order=True)
                worst = max(worst, _check(wc, c, cfg, True))
                ws, a = _run(dev, c, cfg, i % 2 == 0, scaled=True)
                worst = max(worst, _check(ws, c, cfg, i % 2 == 0, a))
    return worst


@pytest.mark.parametrize("fast", [True, False], ids=["FAST", "general"])
@pytest.mark.parametrize("LQ", [1, 2, 4, 8, 16, 32, 64, 128, 256])
def test_deform_aggregate_vec4(device, LQ, fast):
    """`vec && Cin == 4 LQ` -> kpconv_deform_agg_vec4<LQ, fast>.  The general form runs three of the five other influence x
    aggregation modes (with 13 / 15 / 4 kernel points) in turn, rotating with LQ so that every mode meets several LQ, and all three
    on the largest case."""
    i = int(math.log2(LQ))
    cfgs = (FAST,) if fast else tuple(NONFAST[(i + k) % 6] for k in (0, 2, 4))
    _report("kpconv_deform_agg_vec4<%d, %s>" % (LQ, "true" if fast else "false"), _all(device, "agg_vec4", 4 * LQ, cfgs, dc.shapes(LQ)))


@pytest.mark.parametrize("Cin,ld,off", [pytest.param(6, None, 0, id="Cin6"), pytest.param(32, 33, 0, id="Cin32-ldf33"),
                                        pytest.param(32, 36, 1, id="Cin32-base+4B")])
def test_deform_aggregate_scalar(device, Cin, ld, off):
    """kpconv_deform_agg_scalar by each of its reasons but the address range: `Cin % 4 != 0`, `ldf % 4 != 0`, `(f & 15) != 0` (a view
    that starts one float into a row).  All six influence x aggregation modes, with and without modulations."""
    from oracle import kpconv_cases as kc
    worst = 0.0
    for j, (inf, mode) in enumerate(kc.MODES):
        cfg = (inf, mode, (15, 13, 4)[j % 3])
        Nq, K = ((37, 9), (3, 5))[j % 2]
        c = dc.shape_case("agg_scalar", Cin, Nq, K, num_kp=cfg[2])
        assert dc.range_decided(c) and min(dc.in_range_counts(c)) > 0
        for modulated in (j % 2 == 0, j % 2 == 1):
            a = _operands(device, c, cfg, modulated, cap=ld is None)
            if ld is not None:
                a["f"], a["ldf"] = _view(c.f[:c.Ns], device, ld, off), ld
                assert off == 0 or a["f"].data_ptr() % 16 == 4
            a["wf"] = torch.full((a["Nq"], cfg[2] * Cin), S, dtype=torch.float32, device=device)
            assert _call(a) == OK
            wf = a["wf"].cpu().numpy()
            assert np.all(wf[c.Nq:] == S)
            worst = max(worst, _check(wf, c, cfg, modulated))
    _report("kpconv_deform_agg_scalar (Cin %d ldf %s)" % (Cin, ld), worst)


def test_deform_aggregate_argument_errors(device):
    """feat_bf16 = 1 is D3F_ERR_ARG (fp32 feature rows only) and leaves the output untouched, as every other refused argument does."""
    c = dc.shape_case("errors", 16, 9, 5)
    a = _operands(device, c, FAST, True)
    a["wf"] = torch.full((9, 15 * 16), S, dtype=torch.float32, device=device)
    bad = [dict(bf16=1), dict(ld_idx=4), dict(ldf=12), dict(Cin=0), dict(num_kp=0), dict(num_kp=16), dict(extent=0.0),
           dict(extent=float("nan")), dict(influence=3), dict(aggregation=2), dict(K=-1), dict(q=None), dict(off=None), dict(wf=None),
           dict(ld_off=44), dict(ld_mod=14), dict(logits=2), dict(off_scale=float("nan")), dict(Ns=0)]
    for b in bad:
        assert _call(dict(a, **b)) == ERR_ARG, b
    assert torch.all(a["wf"] == S)
    none = {k: None for k in ("q", "s", "idx", "f", "off", "mod", "kp", "wf")}
    assert _call(dict(a, Nq=0, **none)) == OK        # Nq == 0: nothing to do, NULL pointers
    assert _call(a) == OK
    assert not torch.any(a["wf"] == S)


def test_python_layer_refuses_bfloat16_features(device):
    from d3feat_amd import ops
    c = dc.shape_case("errors", 16, 9, 5)
    q, s, idx = _t(c.q[:9], device), _t(c.s[:c.Ns], device), _t(c.idx[:9], device)
    with pytest.raises(TypeError, match="float32 feature rows only"):
        ops.kpconv_deform_aggregate(q, s, idx, _t(c.f[:c.Ns], device).to(torch.bfloat16), c.KP, _t(c.raw[:9], device), dc.EXTENT, raw=True)
