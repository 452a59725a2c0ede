"""Every dispatch branch of csrc/kpconv.hip -- the row flags, the aggregation kernels, the fused Cin = Cout = 32 / 64 / 128 / 256
kernels in both contraction forms and the Cin = 1 kernels, 52 instantiations -- against a plain float64 evaluation of
kernels/convolution_ops.py:161-255 (oracle/network_np.kpconv_f64) on synthetic inputs (oracle/kpconv_cases.py).

The launchers choose a kernel by channel count, alignment, leading dimension, address range, kernel-point configuration, feature
dtype and the X3 switch; each test names the instantiation it is meant to execute and quotes the launcher's condition its shapes
follow from.  Shapes: Nq in {1, TQ - 1, 3 TQ + 5} (TQ = queries per workgroup), K around each kernel's neighbour chunk, K = 0 through
the C ABI (torch reports a NULL address for a tensor without elements and the launchers reject a NULL index matrix).  Padding
columns of every strided feature / residual view and capacity rows hold NaN, padding columns of the index matrix 0x3fffffff, outputs
of capacity-mode calls are pre-filled with a sentinel: a kernel that reads or writes outside its operands poisons its result.

Bars
----
Row flags (d3f_row_positive): exact, the sign of math.fsum(row).

Weighted features wf[n, p, c] = sum_k h_k f_k (fp32, and fp32 from bfloat16 features: the reference is evaluated on the exact
bfloat16 values): a bound derived from the kernels' own sequence, u = 2^-24 the unit roundoff, e = KP_extent, D = d / 2e:
  * r = s - q, then d_i = r_i - KP_i: one rounding each, |delta d_i| <= u (|r_i| + |d_i|), i.e. u (|r| + |d|) in d = |d_i|; a pair
    with h > 0 has |d| < 2e and |r| <= |d| + |KP| <= 3.5e (|KP| <= 1.5e): <= 2.75 u in D;
  * d2: a product and two FMAs + the 1e-10 add (4 roundings; the general form: three products, three adds, 6 roundings), all terms
    positive: <= 6 u relative in d2, 3 u in D;  v_sqrt, 1 ulp = 2 u: 2 u in D;  1 / 2e rounded once: u in D;
  * h = fma(-sqrt, 1 / 2e, 1): one rounding of a value <= 1 (the general form: a product and a subtraction): <= 2 u; the clamp at 0
    does not increase a difference.  |delta h| <= (2.75 + 3 + 2 + 1 + 2) u = 10.75 u <= 5.5 * 2^-23   ('linear');
  * 'gaussian', h = exp(-x), x = d2 / g: |delta d2| <= 2 u (2 |d|^2 + 1.5e |d|) from the inputs, times exp(-x) / g: <= 4.5 u (maxima of
    x exp(-x) and sqrt(x) exp(-x)); six roundings of d2, three of g, the division and expf at 1 ulp, each times x exp(-x) <= 0.37 or
    exp(-x) <= 1: <= 13 u = 6.5 * 2^-23;  'constant': h = 1, no error;
  * K FMAs of accumulation (a shadow slot adds an exact 0), each rounding a partial sum of magnitude <= sum_k h_k |f_k|.
  |wf - wf64| <= 2^-23 * (c_h * sum_k |f_k| + n / 2 * sum_k h_k |f_k|),   c_h = 5.5 / 6.5 / 0,  n = valid neighbours of the query,
which is at most the c(K) * 2^-23 * sum_k |f_k| with c(K) = c_h + K / 2 that holds for any influences <= 1.  Each test prints the
largest error / bound it saw and asserts <= 1.  inv_cnt is compared as a count: round(1 / inv_cnt) == max(count, 1) exactly and
|inv_cnt * max(count, 1) - 1| <= 2^-22.

Fused fp32 outputs (Cin = 1 included), against float64 with the epilogue applied: max |got - want| <= 5e-6 * max |want| (the figure
of tests/test_gpu_kpconv_x3.py) and <= 1e-4 absolute (BASELINE.json; the outputs are of order 1); the fp32-MFMA and operand-split
forms of one case agree within 2e-6 * max |want|.  bfloat16 outputs: |got - want| <= 2^-8 |want| + the fp32 bar, per element (one
bfloat16 ulp of the float64 value; the only bar these kernels had was 1e-2 on unit-norm descriptors after 38 layers).  Recorded, not
asserted: does a bfloat16 instantiation equal bf16_rne(the fp32 instantiation on the up-converted features) bit for bit.

Instantiation -> test (52; profiles/kpconv_branch_tests_kernel_stats.csv is the kernel trace of this file)
---------------------------------------------------------------------------------------------------------
  kp_rowpos_vec_kernel<4 / 8 / 16 / 32 / 64>, kp_rowpos_kernel, kp_rowpos_vec_kernel<8 / 16 / 32 / 64, unsigned short>   (10)
      test_row_positive[<id names the instantiation>]
  kpconv_agg_vec4<LQ, true>, <LQ, false>, LQ = 1 .. 256   (18)          test_aggregate_vec4[LQ-FAST], [LQ-general]
  kpconv_agg_scalar   (1)          test_aggregate_scalar[Cin6 / Cin1 / Cin32-ldf33 / Cin32-base+4B], test_aggregate_beyond_24_bit_addressing
  kpconv_agg_vec4<64 / 128, true, unsigned short>   (2)          test_aggregate_bf16[64], [128]
  kpconv_fused32_kernel<true, 4, float, X3>, <false, 8, float, X3>, <true, 4, unsigned short, X3>, X3 = false / true   (6)
      test_fused32[FAST], [general], [bf16]
  kpconv_fused_kernel<16 / 32 / 64, 4, float / unsigned short, X3>, X3 = false / true   (12)          test_fused[LQ-float], [LQ-bf16]
  kpconv_c1_kp_kernel<float>, <unsigned short>, kpconv_c1_fused_kernel   (3)          test_c1_sum[float], [bf16], test_c1_closest

Measured on an MI355X (the largest ratio over the cases of each kernel; printed by every test, never used as a bar)
  wf error / bound      agg_vec4<LQ, true>, LQ = 1 .. 256:   0.19 0.19 0.23 0.13 0.09 0.09 0.07 0.07 0.14
                        agg_vec4<LQ, false>:                 0.50 0.46 0.50 0.45 0.18 0.17 0.13 0.07 0.07
                        agg_scalar: 0.26 (Cin 6, 1), 0.40 (ldf 33, base + 4 B), 0.12 (ld_idx 2^24);  agg_vec4<64 / 128, .., bf16>: 0.08 0.06
  fused fp32 error / (5e-6 max |want|)      fused32 FAST 0.08, general 0.17;  fused<16 / 32 / 64> 0.16 0.18 0.23;  c1 'sum' 0.07, 'closest' 0.03
  fp32 MFMA vs operand-split / (2e-6 max |want|)      fused32 0.19, 0.25;  fused<16 / 32 / 64> 0.35 0.49 0.67
  bf16 error / (2^-8 |want| + fp32 bar)      0.98 .. 0.99 for all five (rounding to nearest bfloat16 alone reaches 1.0)
  bf16 instantiation == bf16_rne(fp32 instantiation): bit for bit in all eleven (aggregates: == the float instantiation), 0 of 661 484 elements differ
No defect was found.  Cost: the 56 cases take 4.7 s run alone and 2.1 s of the full GPU suite's 233 s (the slowest 0.2 s);
nothing allocates more than a few MB but the one 128 MB index stride.

The launchers hold 52 instantiations, not 53: d3f_row_positive has 10 (five float vector widths, the scalar form, four bfloat16 widths).
"""
import math

import numpy as np
import pytest
import torch

from conftest import bits

pytestmark = pytest.mark.gpu

S = -124.0                        # sentinel of pre-filled outputs (a bfloat16 value too)
OK, ERR_ARG = 0, -3               # D3F_OK, D3F_ERR_ARG (include/d3feat_amd.h)
ALPHA = float(np.float32(0.1))    # a LeakyReLU slope that is not the default
C_H = {"constant": 0.0, "linear": 5.5, "gaussian": 6.5}
FAST = ("linear", "sum", 15)      # kp_fast_config: num_kp == 15 && influence == linear && aggregation == sum
NONFAST = (("gaussian", "sum", 13), ("linear", "closest", 15), ("constant", "sum", 4))
_INF = {"constant": 0, "linear": 1, "gaussian": 2}
_AGG = {"sum": 0, "closest": 1}
BF16_EQUALS_ROUNDED_F32 = {}      # recorded, not asserted: instantiation -> (elements that differ, elements)

NAMES = {
    "agg": "q Nq s Ns idx ld_idx K f ldf Cin rowpos kp num_kp extent influence aggregation wf inv nq_dev ns_dev order bf16 stream",
    "fused32": "q Nq s Ns idx ld_idx K f ldf rowpos kp num_kp extent influence aggregation W cs ch res ldr leaky alpha out ldo "
               "nq_dev ns_dev order bf16 stream",
    "fused": "q Nq s Ns idx ld_idx K f ldf Cin rowpos kp num_kp extent influence aggregation W Cout cs ch res ldr leaky alpha out ldo "
             "nq_dev ns_dev order bf16 stream",
    "c1": "q Nq s Ns idx ld_idx K f ldf kp num_kp extent influence aggregation W Cout cs ch res ldr leaky alpha out ldo "
          "nq_dev ns_dev order bf16 stream",
}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(v, dev):
    return torch.tensor([int(v)], dtype=torch.int32, device=dev)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _lib():
    from d3feat_amd import _lib
    return _lib.load()


def _view(a, dev, ld=None, off=0, fill=np.nan, bf16=False):
    """a [n, C] on the device: contiguous, or (ld given) the column slice [off, off + C) of an [n, ld] matrix filled with `fill`."""
    n, C = a.shape
    if ld is None:
        t = _t(a, dev)
        return t.to(torch.bfloat16) if bf16 else t
    big = np.full((n, ld), fill, a.dtype)
    big[:, off:off + C] = a
    t = _t(big, dev)
    return (t.to(torch.bfloat16) if bf16 else t)[:, off:off + C]


def _np(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _call(fn, kind, a):
    """The C ABI entry point `fn` with the named arguments of `a` (tensors -> device addresses, host arrays -> host addresses)."""
    vals = []
    for n in NAMES[kind].split():
        v = a.get(n)
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        elif isinstance(v, np.ndarray):
            v = v.ctypes.data
        vals.append(v)
    return getattr(_lib(), fn)(*vals)


def _case(kernel, Cin, Nq, K, cfg=FAST, bf16=False, self_queries=False):
    from oracle import kpconv_cases as kc
    return kc.shape_case(kernel, Cin, Nq, K, num_kp=cfg[2], bf16=bf16, self_queries=self_queries)


def _operands(dev, c, cfg, strided=False, bf16=False, cap=False, order=False, rowpos=True):
    """The gather / kernel-point arguments of a case as a dict of named C ABI arguments (NAMES), tensors kept alive in it.
    cap: the tensors keep their capacity rows and Nq_dev / Ns_dev name the effective counts (attributes n_dev for the wrappers);
    strided: ld_idx = K + 3 (padding 0x3fffffff) and ldf = Cin + 16 (padding NaN); order: a random permutation as q_order."""
    from oracle import kpconv_cases as kc
    nq, ns = (len(c.q), len(c.s)) if cap else (c.Nq, c.Ns)
    K, Cin = c.idx.shape[1], c.f.shape[1]
    a = dict(Nq=nq, Ns=ns, K=K, Cin=Cin, kp=np.ascontiguousarray(c.KP, np.float32), num_kp=cfg[2], extent=kc.EXTENT,
             influence=_INF[cfg[0]], aggregation=_AGG[cfg[1]], bf16=1 if bf16 else 0, stream=_stream(dev), ldr=0, leaky=0, alpha=0.2)
    a["q"], a["s"] = _t(c.q[:nq], dev), _t(c.s[:ns], dev)
    if K == 0:
        a["idx"], a["ld_idx"] = _t(np.ones((nq, 3), np.int32), dev), 3          # (a non-NULL dummy)
    else:
        a["idx"] = _view(c.idx[:nq], dev, K + 3, 2, fill=kc.GARBAGE) if strided else _t(c.idx[:nq], dev)
        a["ld_idx"] = K + 3 if strided else K
    a["f"] = _view(c.f[:ns], dev, Cin + 16 if strided else None, 8, bf16=bf16)
    a["ldf"] = Cin + 16 if strided else Cin
    if cap:
        a["nq_dev"], a["ns_dev"] = _i32(c.Nq, dev), _i32(c.Ns, dev)
        a["q"].n_dev, a["s"].n_dev = a["nq_dev"], a["ns_dev"]
    if order:
        a["order"] = _t(np.random.default_rng(K + nq).permutation(c.Nq).astype(np.int32), dev)
        a["q"].order = a["order"]
    if rowpos:
        a["rowpos"] = torch.ones((max(ns, 1),), dtype=torch.uint8, device=dev)      # (rows beyond Ns_dev stay 1: never read)
        assert _lib().d3f_row_positive(a["f"].data_ptr(), ns, a["ldf"], Cin, a["rowpos"].data_ptr(),
                                       a["ns_dev"].data_ptr() if cap else None, a["bf16"], a["stream"]) == OK
    return a


def _wf_check(wf, inv, c, cfg):
    """wf [>= Nq, num_kp * Cin], inv [>= Nq] (numpy) against kpconv_f64 -> the largest error / bound (module docstring)."""
    from oracle import kpconv_cases as kc
    from oracle import network_np as onp
    inf, mode, P = cfg
    Nq, Cin = c.Nq, c.f.shape[1]
    memo = c.setdefault("_ref", {})
    if cfg not in memo:      # (a case is checked several times: plain, strided, capacity mode)
        ref = lambda f: onp.kpconv_f64(c.q, c.s, c.idx, f, c.KP, None, kc.EXTENT, inf, mode, Nq=c.Nq, Ns=c.Ns)
        want, count, _ = ref(c.f)
        af = np.abs(c.f[:c.Ns]).astype(np.float64)
        valid = (c.idx[:Nq] >= 0) & (c.idx[:Nq] < c.Ns)
        s_hf = ref(np.abs(c.f))[0]                                                            # sum_k h_k |f_k|   [Nq, P, Cin]
        s_f = (af[np.where(valid, c.idx[:Nq], 0)] * valid[:, :, None]).sum(1)[:, None, :]     # sum_k |f_k|       [Nq, 1, Cin]
        memo[cfg] = want, count, 2.0 ** -23 * (C_H[inf] * s_f + 0.5 * valid.sum(1)[:, None, None] * s_hf)
    want, count, bound = memo[cfg]
    err = np.abs(wf[:Nq].astype(np.float64).reshape(Nq, P, Cin) - want)
    assert np.isfinite(wf[:Nq]).all()
    assert np.all(err[bound == 0] == 0)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    cnt = np.maximum(count, 1)
    assert np.array_equal(np.round(1.0 / inv[:Nq].astype(np.float64)), cnt), "neighbour count"
    assert np.abs(inv[:Nq].astype(np.float64) * cnt - 1).max() <= 2.0 ** -22
    return ratio


def _report(name, ratio, what="error / bound"):
    print("%s: largest %s %.3f" % (name, what, ratio))
    assert ratio <= 1.0, "%s: %s %.3f > 1" % (name, what, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# 1. d3f_row_positive
# ---------------------------------------------------------------------------------------------------------------------
ROWPOS = [
    pytest.param(4, None, 0, False, id="kp_rowpos_vec_kernel<4>-C4"),                  # q4 = Cin / 4 <= 4
    pytest.param(16, 24, 4, False, id="kp_rowpos_vec_kernel<4>-C16-ldf24"),
    pytest.param(20, None, 0, False, id="kp_rowpos_vec_kernel<8>-C20"),                # q4 <= 8
    pytest.param(32, 40, 4, False, id="kp_rowpos_vec_kernel<8>-C32-ldf40"),
    pytest.param(64, None, 0, False, id="kp_rowpos_vec_kernel<16>-C64"),               # q4 <= 16
    pytest.param(128, None, 0, False, id="kp_rowpos_vec_kernel<32>-C128"),             # q4 <= 32
    pytest.param(1024, None, 0, False, id="kp_rowpos_vec_kernel<64>-C1024"),           # else
    pytest.param(6, None, 0, False, id="kp_rowpos_kernel-C6"),                         # Cin % 4 != 0
    pytest.param(70, None, 0, False, id="kp_rowpos_kernel-C70"),
    pytest.param(32, 35, 0, False, id="kp_rowpos_kernel-C32-ldf35"),                   # ldf % 4 != 0
    pytest.param(32, 36, 1, False, id="kp_rowpos_kernel-C32-base+4B"),                 # (f & 15) != 0
    pytest.param(32, None, 0, True, id="kp_rowpos_vec_kernel<8,bf16>-C32"),            # feat_bf16, q4 <= 8
    pytest.param(64, 80, 8, True, id="kp_rowpos_vec_kernel<16,bf16>-C64-ldf80"),       # q4 <= 16
    pytest.param(128, None, 0, True, id="kp_rowpos_vec_kernel<32,bf16>-C128"),         # q4 <= 32
    pytest.param(512, None, 0, True, id="kp_rowpos_vec_kernel<64,bf16>-C512"),         # else
]


@pytest.mark.parametrize("Cin,ld,off,bf16", ROWPOS)
def test_row_positive(device, Cin, ld, off, bf16):
    """d3f_row_positive: feat_bf16 -> kp_rowpos_vec_kernel<8 / 16 / 32 / 64, unsigned short> by `q4 = Cin / 4 <= 8 / 16 / 32 / else`;
    `Cin % 4 == 0 && ldf % 4 == 0 && (f & 15) == 0` -> kp_rowpos_vec_kernel<4 / 8 / 16 / 32 / 64> by `q4 <= 4 / 8 / 16 / 32 / else`;
    otherwise kp_rowpos_kernel.  Its stated claim -- the sign of the real-number sum whatever the order -- holds exactly: the flag
    equals math.fsum(row) > 0 on cancelling rows, {2^20, 1, -2^20}, {2^25, 1, -2^25}, -0.0 rows, a lone subnormal; Ns = 77 is no multiple of the rows
    per wavefront; with Ns_dev < Ns the rows beyond it keep the sentinel; padding columns are NaN."""
    from oracle import kpconv_cases as kc
    Ns, Nd = 77, 50
    x, want = kc.rowpos_case(Cin + (ld or 0) + off, Ns, Cin, bf16)
    f = _view(x, device, ld, off, bf16=bf16)
    ldf = ld or Cin
    for nd in (None, Nd):
        pos = torch.full((Ns,), 7, dtype=torch.uint8, device=device)
        nd_t = _i32(nd, device) if nd else None
        assert _lib().d3f_row_positive(f.data_ptr(), Ns, ldf, Cin, pos.data_ptr(), nd_t.data_ptr() if nd else None,
                                       1 if bf16 else 0, _stream(device)) == OK
        got = pos.cpu().numpy()
        n = nd or Ns
        assert np.array_equal(got[:n], want[:n]), np.nonzero(got[:n] != want[:n])[0]
        assert np.all(got[n:] == 7)
    assert 0 < want.sum() < Ns


def test_row_positive_argument_errors(device):
    f = torch.zeros((8, 32), dtype=torch.float32, device=device)
    pos = torch.zeros((8,), dtype=torch.uint8, device=device)
    rp = lambda *a: _lib().d3f_row_positive(*a, _stream(device))
    assert rp(f.data_ptr(), 8, 32, 32, pos.data_ptr(), None, 0) == OK
    assert rp(f.data_ptr(), 8, 16, 32, pos.data_ptr(), None, 0) == ERR_ARG          # ldf < Cin
    assert rp(f.data_ptr(), 8, 32, 0, pos.data_ptr(), None, 0) == ERR_ARG           # Cin < 1
    assert rp(None, 0, 32, 32, None, None, 0) == OK                                 # Ns == 0
    assert rp(f.data_ptr(), 8, 32, 30, pos.data_ptr(), None, 1) == ERR_ARG          # bf16: Cin % 4
    assert rp(f.data_ptr(), 8, 34, 32, pos.data_ptr(), None, 1) == ERR_ARG          # bf16: ldf % 4
    assert rp(f.data_ptr() + 2, 8, 32, 32, pos.data_ptr(), None, 1) == ERR_ARG      # bf16: base not 8-byte aligned


# ---------------------------------------------------------------------------------------------------------------------
# 2. d3f_kpconv_aggregate
# ---------------------------------------------------------------------------------------------------------------------
def _aggregate(dev, c, cfg, strided=False, bf16=False, cap=False, order=False, abi=False):
    """-> (wf, inv) as numpy, through ops.kpconv_aggregate, or the C ABI (K = 0; capacity mode: sentinel-filled outputs)."""
    from d3feat_amd import ops
    from oracle import kpconv_cases as kc
    K, Cin, P = c.idx.shape[1], c.f.shape[1], cfg[2]
    a = _operands(dev, c, cfg, strided, bf16, cap, order, rowpos=abi or K == 0)
    if not (abi or K == 0):
        wf, inv = ops.kpconv_aggregate(a["q"], a["s"], a["idx"], a["f"], c.KP, kc.EXTENT, cfg[0], cfg[1])
        return _np(wf), _np(inv)
    a["wf"] = torch.full((a["Nq"], P * Cin), S, dtype=torch.float32, device=dev)
    a["inv"] = torch.full((a["Nq"],), S, dtype=torch.float32, device=dev)
    assert _call("d3f_kpconv_aggregate", "agg", a) == OK
    wf, inv = _np(a["wf"]), _np(a["inv"])
    assert np.all(wf[c.Nq:] == S) and np.all(inv[c.Nq:] == S)                     # rows beyond Nq_dev keep the sentinel
    return wf, inv


def _aggregate_all(dev, kernel, Cin, cfgs, shapes, bf16=False):
    """Every (Nq, K) of `shapes` with the configurations of `cfgs` in turn; odd cases on strided views; the last (largest) case
    again with q_order (bit-equal to the unordered call) and in capacity mode (Nq_dev < Nq, Ns_dev < Ns) -> largest ratio."""
    worst = 0.0
    for j, (Nq, K) in enumerate(shapes):
        cfg = cfgs[j % len(cfgs)]
        c = _case(kernel, Cin, Nq, K, cfg, bf16, self_queries=j % 3 == 2)
        wf, inv = _aggregate(dev, c, cfg, strided=j % 2 == 1, bf16=bf16)
        worst = max(worst, _wf_check(wf, inv, c, cfg))
        if j == len(shapes) - 1:
            for cfg in cfgs:
                if cfg[2] != c.KP.shape[0]:
                    c = _case(kernel, Cin, Nq, K, cfg, bf16)
                wf, inv = _aggregate(dev, c, cfg, bf16=bf16)
                worst = max(worst, _wf_check(wf, inv, c, cfg))
                wo, io = _aggregate(dev, c, cfg, bf16=bf16, order=True)
                assert np.array_equal(bits(wo), bits(wf)) and np.array_equal(bits(io), bits(inv))
                wc, ic = _aggregate(dev, c, cfg, strided=True, bf16=bf16, cap=True, order=True, abi=True)
                worst = max(worst, _wf_check(wc, ic, c, cfg))
                h = _wf_nonzero_share(c, cfg)
                assert Nq * K < 300 or h > 0.02, h                                  # the pairs are inside the kernel's reach
    return worst


def _wf_nonzero_share(c, cfg):
    from oracle import kpconv_cases as kc
    from oracle import network_np as onp
    w = onp.kpconv_f64(c.q, c.s, c.idx, np.ones_like(c.f[:, :1]), c.KP, None, kc.EXTENT, cfg[0], cfg[1], Nq=c.Nq, Ns=c.Ns)[0]
    return float((w > 0).mean())


@pytest.mark.parametrize("fast", [True, False], ids=["FAST", "general"])
@pytest.mark.parametrize("LQ", [1, 2, 4, 8, 16, 32, 64, 128, 256])
def test_aggregate_vec4(device, LQ, fast):
    """d3f_kpconv_aggregate: `vec = Cin % 4 == 0 && ldf % 4 == 0 && (f & 15) == 0 && (wf & 15) == 0 && kp_fits_u24`, `vec && Cin ==
    4 LQ` -> kpconv_agg_vec4<LQ, fast>, `fast = kp_fast_config` (linear / sum / 15 points).  TQ = 256 / LQ queries per workgroup, chunks
    of KC = LQ neighbours, PF = min(KC, 8) rows in flight: K in {0, 1, KC - 1, KC, KC + 1, 37} (+ 7, 8, 9 at LQ <= 8; 1, 40, 257 at
    LQ = 256, where one query spans four wavefronts and the count goes through atomics).  The general form runs (gaussian, sum, 13),
    (linear, closest, 15) and (constant, sum, 4) in turn, and all three on the largest case."""
    from oracle import kpconv_cases as kc
    name = "kpconv_agg_vec4<%d, %s>" % (LQ, "true" if fast else "false")
    shapes = kc.shapes_of("agg_vec4", 4 * LQ)      # Nq in {1, TQ - 1, 3 TQ + 5} x the K values above, sparse (kc.combos)
    i = int(math.log2(LQ))
    cfgs = (FAST,) if fast else tuple(NONFAST[(i + k) % 3] for k in range(3))
    _report(name, _aggregate_all(device, "agg_vec4", 4 * LQ, cfgs, shapes))


@pytest.mark.parametrize("Cin,ld,off", [pytest.param(6, None, 0, id="Cin6"), pytest.param(1, None, 0, id="Cin1"),
                                        pytest.param(32, 33, 0, id="Cin32-ldf33"), pytest.param(32, 36, 1, id="Cin32-base+4B")])
def test_aggregate_scalar(device, Cin, ld, off):
    """kpconv_agg_scalar by each of its reasons but the address range: `Cin % 4 != 0` (6, 1), `ldf % 4 != 0` (ldf = 33),
    `(f & 15) != 0` (a view that starts one float into a row).  All six influence x aggregation modes."""
    from d3feat_amd import ops
    from oracle import kpconv_cases as kc
    worst = 0.0
    for j, (inf, mode) in enumerate(kc.MODES):
        cfg = (inf, mode, (15, 13, 4)[j % 3])
        Nq, K = kc.shapes_of("agg_scalar", Cin)[j % 2]
        c = _case("agg_scalar", Cin, Nq, K, cfg)
        f = _view(c.f[:c.Ns], device, ld, off)
        if off:
            assert f.data_ptr() % 16 == 4
        wf, inv = ops.kpconv_aggregate(_t(c.q[:Nq], device), _t(c.s[:c.Ns], device), _t(c.idx[:Nq], device), f, c.KP, kc.EXTENT, inf, mode)
        worst = max(worst, _wf_check(_np(wf), _np(inv), c, cfg))
        wc, ic = _aggregate(device, c, cfg, cap=True, abi=True) if ld is None else (None, None)
        if wc is not None:
            worst = max(worst, _wf_check(wc, ic, c, cfg))
    _report("kpconv_agg_scalar (Cin %d ldf %s)" % (Cin, ld), worst)


def test_aggregate_beyond_24_bit_addressing(device):
    """`kp_fits_u24(Nq, Ns, ld_idx, ldf)` is false once ld_idx >= 2^24: three index rows at a row stride of 2^24 (128 MB, freed here)
    send a Cin = 32 stack to kpconv_agg_scalar; d3f_kpconv_fused32 returns D3F_ERR_ARG for the same call, and
    convolution_ops.KPConv_ops on it (aggregation + contraction) still equals the reference."""
    from d3feat_amd import ops
    from d3feat_amd.kernels import convolution_ops as conv_ops
    from oracle import kpconv_cases as kc
    from oracle import network_np as onp
    (Nq, K), ld = kc.shapes_of("agg_scalar", 32)[1], 1 << 24
    assert Nq == 3
    c = _case("agg_scalar", 32, Nq, K)
    a = _operands(device, c, FAST)
    store = torch.empty(((Nq - 1) * ld + K,), dtype=torch.int32, device=device)
    iv = store.as_strided((Nq, K), (ld, 1))
    iv.copy_(a["idx"])
    wf, inv = ops.kpconv_aggregate(a["q"], a["s"], iv, a["f"], c.KP, kc.EXTENT)
    _report("kpconv_agg_scalar (ld_idx 2^24)", _wf_check(_np(wf), _np(inv), c, FAST))
    W = kc.weights(1, 15, 32, 32)
    Wt = _t(W, device)
    out = torch.full((Nq, 32), S, dtype=torch.float32, device=device)
    a.update(idx=iv, ld_idx=ld, W=Wt.reshape(480, 32), out=out, ldo=32)
    assert _call("d3f_kpconv_fused32", "fused32", a) == ERR_ARG
    assert torch.all(out == S)
    got = conv_ops.KPConv_ops(a["q"], a["s"], iv, a["f"], c.KP, Wt, kc.EXTENT, "linear", "sum")
    want = onp.kpconv_f64(c.q, c.s, c.idx, c.f, c.KP, W, kc.EXTENT, Nq=c.Nq, Ns=c.Ns)[2]
    _report("KPConv_ops (ld_idx 2^24)", _out_check(_np(got), want), "error / (5e-6 max |want|)")
    del iv, store, a


@pytest.mark.parametrize("LQ", [64, 128])
def test_aggregate_bf16(device, LQ):
    """feat_bf16: `fast && ldf % 4 == 0 && (f & 7) == 0 && (wf & 15) == 0 && Cin in {256, 512}` -> kpconv_agg_vec4<64 / 128, true,
    unsigned short>; anything else is D3F_ERR_ARG.  The features ARE bfloat16 values and the reference is evaluated on them, so the
    fp32 bound applies unchanged (kp_gather4's unpacking of a 64-bit word into four channels is exact)."""
    from oracle import kpconv_cases as kc
    Cin = 4 * LQ
    shapes = kc.shapes_of("agg_vec4", Cin)
    assert kc.has_bf16("agg_vec4", Cin)
    _report("kpconv_agg_vec4<%d, true, unsigned short>" % LQ, _aggregate_all(device, "agg_vec4", Cin, (FAST,), shapes, bf16=True))
    # recorded: the same values as fp32 features through the fp32 instantiation
    Nq, K = shapes[-1]
    c = _case("agg_vec4", Cin, Nq, K, FAST, True)
    wh, _ = _aggregate(device, c, FAST, bf16=True)
    wf, _ = _aggregate(device, c, FAST, bf16=False)
    BF16_EQUALS_ROUNDED_F32["kpconv_agg_vec4<%d, true, unsigned short>" % LQ] = (int((bits(wh) != bits(wf)).sum()), wf.size)
    print("bf16 == fp32 instantiation on the same values: %d of %d differ" % BF16_EQUALS_ROUNDED_F32["kpconv_agg_vec4<%d, true, unsigned short>" % LQ])
    # argument errors of the bf16 form
    for Cin_bad, cfg, shift in ((128, FAST, 0), (Cin, NONFAST[0], 0), (Cin, NONFAST[1], 0), (Cin, FAST, 4)):
        cb = _case("errors", Cin_bad, 7, 9, cfg, True)
        a = _operands(device, cb, cfg, bf16=True)
        buf = torch.full((7 * cfg[2] * Cin_bad + 4,), S, dtype=torch.float32, device=device)
        a["wf"] = buf[shift // 4:]
        a["inv"] = torch.full((7,), S, dtype=torch.float32, device=device)
        assert _call("d3f_kpconv_aggregate", "agg", a) == ERR_ARG, (Cin_bad, cfg, shift)
        assert torch.all(buf == S)


def test_aggregate_argument_errors(device):
    c = _case("errors", 16, 9, 5)
    a = _operands(device, c, FAST)
    a["wf"] = torch.full((9, 15 * 16), S, dtype=torch.float32, device=device)
    a["inv"] = torch.full((9,), S, dtype=torch.float32, device=device)
    bad = [dict(ld_idx=4), dict(ldf=12), dict(Cin=0), dict(num_kp=0), dict(num_kp=16), dict(extent=0.0), dict(extent=float("nan")),
           dict(influence=3), dict(aggregation=2), dict(K=-1), dict(q=None), dict(rowpos=None), dict(wf=None)]
    for b in bad:
        assert _call("d3f_kpconv_aggregate", "agg", dict(a, **b)) == ERR_ARG, b
    assert torch.all(a["wf"] == S)
    none = {k: None for k in ("q", "s", "idx", "f", "rowpos", "kp", "wf", "inv")}
    assert _call("d3f_kpconv_aggregate", "agg", dict(a, Nq=0, **none)) == OK       # Nq == 0: nothing to do, NULL pointers
    assert _call("d3f_kpconv_aggregate", "agg", a) == OK


# ---------------------------------------------------------------------------------------------------------------------
# 3. d3f_kpconv_fused32[_x3], d3f_kpconv_fused[_x3]
# ---------------------------------------------------------------------------------------------------------------------
EPILOGUES = ("none", "scale", "shift", "residual", "leaky", "all")


def _epilogue(kind, Cout, rows, seed, bf16=False):
    """-> host operands {col_scale, col_shift, residual, leaky, alpha} of one epilogue variant (bf16 feature storage: no residual)."""
    rng = np.random.default_rng(seed)
    e = {}
    if kind in ("scale", "all"):
        e["col_scale"] = (rng.random(Cout) + 0.5).astype(np.float32)
    if kind in ("shift", "all"):
        e["col_shift"] = rng.standard_normal(Cout).astype(np.float32)
    if kind in ("residual", "all") and not bf16:
        e["residual"] = rng.standard_normal((rows, Cout)).astype(np.float32)
    if kind in ("leaky", "all"):
        e["leaky"], e["alpha"] = True, ALPHA
    return e


def _epi_dev(e, dev, Cout):
    """The epilogue on the device: the residual is a column slice of a wider NaN-padded matrix (ldr = Cout + 8)."""
    d = {k: (_t(v, dev) if k != "residual" else _view(v, dev, Cout + 8, 4)) if isinstance(v, np.ndarray) else v for k, v in e.items()}
    return d


def _out_check(got, want, bf16=False):
    """Fused outputs against float64 -> error / (5e-6 max |want|), after the absolute and (bf16) per-element bars."""
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    scale = float(np.abs(want).max()) if want.size else 0.0
    assert scale <= 30.0, scale                                                     # (outputs of order 1)
    if bf16:
        r = err / (2.0 ** -8 * np.abs(want) + 5e-6 * scale + 1e-300)
        assert np.all(err[(want == 0) & (scale == 0)] == 0)
        return float(r.max()) if r.size else 0.0
    if scale == 0:
        assert np.all(err == 0)
        return 0.0
    assert err.max() <= 1e-4, err.max()
    return float(err.max() / (5e-6 * scale))


def _fused_wrapper(dev, kernel, c, cfg, Wt, e, x3, strided=False, bf16=False, cap=False, order=False):
    from d3feat_amd import ops
    from oracle import kpconv_cases as kc
    a = _operands(dev, c, cfg, strided, bf16, cap, order, rowpos=False)
    fn = ops.kpconv_fused32 if kernel == "fused32" else ops.kpconv_fused
    keep = ops.KP_X3
    try:
        ops.KP_X3 = x3
        out = fn(a["q"], a["s"], a["idx"], a["f"], c.KP, Wt, kc.EXTENT, cfg[0], cfg[1], **_epi_dev(e, dev, Wt.shape[2]))
    finally:
        ops.KP_X3 = keep
    assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    return _np(out)


def _fused_abi(dev, kernel, c, cfg, Wt, e, x3, strided=True, bf16=False, cap=True, order=True, ldo_pad=8, **over):
    """The C ABI: out is a column slice of a wider sentinel-filled matrix (ldo = Cout + 8), capacity rows included -> numpy out,
    after checking that padding columns and rows beyond Nq_dev keep the sentinel; or the error code when it is not D3F_OK."""
    from d3feat_amd import ops
    Cout = Wt.shape[2]
    a = _operands(dev, c, cfg, strided, bf16, cap, order)
    ed = _epi_dev(e, dev, Cout)
    if kernel == "fused32":
        W = ops.packed_kpconv_weights_x3(Wt) if x3 else Wt.reshape(-1, Cout).contiguous()
    else:
        W = ops.packed_kpconv_weights_x3(Wt) if x3 else ops.packed_kpconv_weights(Wt)
    big = torch.full((a["Nq"], Cout + ldo_pad), S, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    a.update(W=W, Cout=Cout, cs=ed.get("col_scale"), ch=ed.get("col_shift"), res=ed.get("residual"), ldr=Cout + 8 if "residual" in ed else 0,
             leaky=1 if e.get("leaky") else 0, alpha=e.get("alpha", 0.2), out=big, ldo=Cout + ldo_pad)
    a.update(over)
    fn = {"fused32": "d3f_kpconv_fused32", "fused": "d3f_kpconv_fused", "c1": "d3f_kpconv_fused_c1"}[kernel] + ("_x3" if x3 else "")
    rc = _call(fn, kernel, a)
    got = _np(big)
    if rc != OK:
        assert np.all(got == S)
        return rc
    assert np.all(got[c.Nq:] == S) and np.all(got[:, Cout:] == S)
    return got[:c.Nq, :Cout]


def _want(c, cfg, W, e):
    from oracle import kpconv_cases as kc
    from oracle import network_np as onp
    return onp.kpconv_f64(c.q, c.s, c.idx, c.f, c.KP, W, kc.EXTENT, cfg[0], cfg[1], Nq=c.Nq, Ns=c.Ns, **e)[2]


def _fused_all(dev, kernel, Cin, cfgs, shapes, bf16, name):
    """Every (Nq, K) with both contraction forms (fp32 MFMA, operand-split): even cases without epilogue, odd cases on strided views
    with all operands; the last (largest) case with every epilogue operand alone and all together through the wrapper, and through
    the C ABI with q_order, Nq_dev, Ns_dev, ldr > Cout and ldo > Cout."""
    from oracle import kpconv_cases as kc
    worst = agree = 0.0
    same = [0, 0]
    for j, (Nq, K) in enumerate(shapes):
        last = j == len(shapes) - 1
        for cfg in (cfgs if last else (cfgs[j % len(cfgs)],)):
            c = _case(kernel, Cin, Nq, K, cfg, bf16, self_queries=j % 3 == 2)
            W = kc.weights(Cin + K, cfg[2], Cin, Cin)
            Wt = _t(W, dev)
            for kind in (EPILOGUES if last else (("none", "all")[j % 2],)):
                e = _epilogue(kind, Cin, len(c.q), 7 * j + K, bf16)
                want = _want(c, cfg, W, e)
                got = [_fused_wrapper(dev, kernel, c, cfg, Wt, e, x3, strided=j % 2 == 1, bf16=bf16) for x3 in (False, True)]
                if last and kind == "all":
                    got += [_fused_abi(dev, kernel, c, cfg, Wt, e, x3, bf16=bf16) for x3 in (False, True)]
                worst = max([worst] + [_out_check(g, want, bf16) for g in got])
                scale = np.abs(want).max()
                for g3, g32 in zip(got[1::2], got[0::2]):
                    if bf16:          # (both forms round the same value up to 2e-6: one bfloat16 ulp apart at most)
                        assert np.all(np.abs(g3 - g32) <= 2.0 ** -7 * np.abs(want) + 2e-6 * scale)
                    else:
                        agree = max(agree, float(np.abs(g3 - g32).max() / (2e-6 * scale)) if scale else float(np.abs(g3 - g32).max()))
                if bf16:              # recorded: the fp32 instantiation on the up-converted features, rounded
                    for x3 in (False, True):
                        r = kc.bf16_values(_fused_wrapper(dev, kernel, c, cfg, Wt, e, x3, strided=j % 2 == 1))
                        same[0] += int((bits(r) != bits(np.ascontiguousarray(got[int(x3)], np.float32))).sum())
                        same[1] += r.size
    if bf16:
        BF16_EQUALS_ROUNDED_F32[name] = tuple(same)
        print("%s == bf16_rne(fp32 instantiation): %d of %d elements differ" % (name, same[0], same[1]))
    else:
        _report(name + " fp32 MFMA vs operand-split", agree, "difference / (2e-6 max |want|)")
    return worst


@pytest.mark.parametrize("form", ["FAST", "general", "bf16"])
def test_fused32(device, form):
    """d3f_kpconv_fused32 / _x3 (Cin = Cout = 32, TQ = 32, chunks of KF_LQ = 8; K in {1, 7, 8, 9, 37}): `feat_bf16` ->
    kpconv_fused32_kernel<true, 4, unsigned short, X3>; `!kp_fast_config` -> <false, 8, float, X3>; else <true, 4, float, X3>;
    X3 off and on."""
    from oracle import kpconv_cases as kc
    shapes = kc.shapes_of("fused32", 32)
    name = {"FAST": "kpconv_fused32_kernel<true, 4, float, X3>", "general": "kpconv_fused32_kernel<false, 8, float, X3>",
            "bf16": "kpconv_fused32_kernel<true, 4, unsigned short, X3>"}[form]
    worst = _fused_all(device, "fused32", 32, NONFAST if form == "general" else (FAST,), shapes, form == "bf16", name)
    _report(name, worst, "error / (2^-8 |want| + 5e-6 max |want|)" if form == "bf16" else "error / (5e-6 max |want|)")


@pytest.mark.parametrize("bf16", [False, True], ids=["float", "bf16"])
@pytest.mark.parametrize("LQ", [16, 32, 64])
def test_fused(device, LQ, bf16):
    """d3f_kpconv_fused / _x3 (`d3f_kpconv_fused_supported`: Cin == Cout in {64, 128, 256}, kp_fast_config; TQ = 16): `Cin == 64` ->
    kpconv_fused_kernel<16, 4, FT, X3>, `Cin == 256` -> <64, 4, FT, X3>, else <32, 4, FT, X3>; FT = float / unsigned short, X3 off and
    on.  Chunks of KC = min(LQ, 32) neighbours: K in {1, LQ - 1, LQ, LQ + 1} (and 31, 33 at LQ = 64)."""
    from oracle import kpconv_cases as kc
    name = "kpconv_fused_kernel<%d, 4, %s, X3>" % (LQ, "unsigned short" if bf16 else "float")
    worst = _fused_all(device, "fused", 4 * LQ, (FAST,), kc.shapes_of("fused", 4 * LQ), bf16, name)
    _report(name, worst, "error / (2^-8 |want| + 5e-6 max |want|)" if bf16 else "error / (5e-6 max |want|)")


@pytest.mark.parametrize("kernel,Cin", [("fused32", 32), ("fused", 64)])
def test_fused_argument_errors(device, kernel, Cin):
    """The launchers' rejections that tests/test_cabi.py does not hold: bf16 feature storage with a residual or a general
    configuration; Cin != Cout and unsupported Cin (fused); misaligned weights (fused) / features; ldf % 4; num_kp 0 and 16;
    KP_extent 0 and NaN; and Nq == 0 with NULL pointers is D3F_OK."""
    from oracle import kpconv_cases as kc
    c = _case("errors", Cin, 9, 5)
    Wt = _t(kc.weights(3, 15, Cin, Cin), device)
    e_res = _epilogue("residual", Cin, len(c.q), 1)
    for x3 in (False, True):
        run = lambda cfg=FAST, e={}, bf16=False, **over: _fused_abi(device, kernel, c if not bf16 else _case("errors", Cin, 9, 5, cfg, True),
                                                                   cfg, Wt[:cfg[2]].contiguous(), e, x3, bf16=bf16, **over)
        assert not isinstance(run(), int)
        assert run(e=e_res, bf16=True) == ERR_ARG                                                       # bf16: no residual operand
        assert run(cfg=NONFAST[1], bf16=True) == ERR_ARG                                                # bf16: the shipped configuration only
        for over in (dict(ldf=Cin + 18), dict(num_kp=0), dict(num_kp=16), dict(extent=0.0), dict(extent=float("nan")),
                     dict(ld_idx=4), dict(ldo=Cin - 1), dict(rowpos=None)):
            assert run(**over) == ERR_ARG, over
        fm = torch.zeros((len(c.f) * Cin + 4,), dtype=torch.float32, device=device)[1:]
        assert run(strided=False, f=fm) == ERR_ARG                                                      # (f & 15) != 0
        if kernel == "fused":
            assert run(Cout=Cin // 2) == ERR_ARG and run(Cout=Cin * 2, ldo=Cin * 2 + 8) == ERR_ARG      # Cin != Cout
            for cin_bad in (32, 96, 512):
                assert run(Cin=cin_bad, Cout=cin_bad) == ERR_ARG                                        # unsupported Cin
            wm = torch.zeros((15 * Cin * Cin * 2 + 4,), dtype=torch.float32, device=device)[1:]
            assert run(W=wm) == ERR_ARG                                                                 # (W_packed & 15) != 0
            assert run(cfg=NONFAST[0]) == ERR_ARG and run(cfg=NONFAST[2]) == ERR_ARG                    # no general fused form
        none = {k: None for k in ("q", "s", "idx", "f", "rowpos", "kp", "W", "out")}
        a = dict(_operands(device, c, FAST), Cout=Cin, ldo=Cin, **none)
        a["Nq"] = 0
        assert _call({"fused32": "d3f_kpconv_fused32", "fused": "d3f_kpconv_fused"}[kernel] + ("_x3" if x3 else ""), kernel, a) == OK


# ---------------------------------------------------------------------------------------------------------------------
# 4. d3f_kpconv_fused_c1
# ---------------------------------------------------------------------------------------------------------------------
def _c1(dev, c, cfg, W, e, bf16=False, abi=False, order=False, **over):
    """ops.kpconv_fused_c1 (features: column 3 of a [Ns, 5] NaN-padded matrix), or the C ABI in capacity mode with ldo > Cout."""
    from d3feat_amd import ops
    from oracle import kpconv_cases as kc
    Cout = W.shape[2]
    a = _operands(dev, c, cfg, strided=True, cap=abi, order=order, rowpos=False)
    a["f"], a["ldf"] = _view(c.f[:a["Ns"]], dev, 5, 3), 5
    Wt = _t(W, dev)
    ed = _epi_dev(e, dev, Cout)
    if not abi:
        with ops.bf16_contraction(bf16, features=bf16):
            out = ops.kpconv_fused_c1(a["q"], a["s"], a["idx"], a["f"], c.KP, Wt, kc.EXTENT, cfg[0], cfg[1], **ed)
        assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
        return _np(out)
    big = torch.full((a["Nq"], Cout + 3), S, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    a.update(W=Wt.reshape(cfg[2], Cout), Cout=Cout, cs=ed.get("col_scale"), ch=ed.get("col_shift"), res=ed.get("residual"),
             ldr=Cout + 8 if "residual" in ed else 0, leaky=1 if e.get("leaky") else 0, alpha=e.get("alpha", 0.2), out=big, ldo=Cout + 3,
             bf16=1 if bf16 else 0)
    a.update(over)
    rc = _call("d3f_kpconv_fused_c1", "c1", a)
    got = _np(big)
    if rc != OK:
        assert np.all(got == S)
        return rc
    assert np.all(got[c.Nq:] == S) and np.all(got[:, Cout:] == S)
    return got[:c.Nq, :Cout]


def _c1_all(dev, kernel, mode, bf16=False):
    """K in {1, 2, 37, 64, 65, 130} x Cout in {1, 10, 64, 65, 130, 256} (paired), the three influences in turn, num_kp 15 / 4; the
    largest case with every epilogue operand alone and all together, q_order ('sum'), and capacity mode through the C ABI."""
    from oracle import kpconv_cases as kc
    shapes = kc.shapes_of(kernel, 1)              # TQ = 16 ('sum') / 32 ('closest')
    worst, same = 0.0, [0, 0]
    for j, ((Nq, K), Cout) in enumerate(zip(shapes, kc.C1_COUT)):
        last = j == len(shapes) - 1
        for i, inf in enumerate(("constant", "linear", "gaussian") if last else (("linear", "gaussian", "constant")[j % 3],)):
            cfg = (inf, mode, (15, 4)[(i + j) % 2])
            c = _case(kernel, 1, Nq, K, cfg, self_queries=j % 3 == 2)
            valid = (c.idx[:Nq] >= 0) & (c.idx[:Nq] < c.Ns)
            if Nq * K >= 300:      # positive, zero and negative features: the count is not the number of valid slots
                assert ((c.f[:c.Ns, 0] > 0)[np.where(valid, c.idx[:Nq], 0)] & valid).sum() < valid.sum()
            W = kc.weights(Cout + K, cfg[2], 1, Cout)
            for kind in (EPILOGUES if last and i == 1 else (("none", "all")[j % 2],)):
                e = _epilogue(kind, Cout, len(c.q), 3 * j + K)
                want = _want(c, cfg, W, e)
                got = [_c1(dev, c, cfg, W, e, bf16)]
                if last and kind == "all":
                    got.append(_c1(dev, c, cfg, W, e, bf16, abi=True, order=mode == "sum"))
                    if mode == "sum":
                        go = _c1(dev, c, cfg, W, e, bf16, order=True)
                        assert np.array_equal(bits(np.ascontiguousarray(go, np.float32)), bits(np.ascontiguousarray(got[0], np.float32)))
                worst = max([worst] + [_out_check(g, want, bf16) for g in got])
                if bf16:
                    r = kc.bf16_values(_c1(dev, c, cfg, W, e))
                    same[0] += int((bits(r) != bits(np.ascontiguousarray(got[0], np.float32))).sum())
                    same[1] += r.size
    if bf16:
        BF16_EQUALS_ROUNDED_F32["kpconv_c1_kp_kernel<unsigned short>"] = tuple(same)
        print("kpconv_c1_kp_kernel<unsigned short> == bf16_rne(fp32 instantiation): %d of %d elements differ" % tuple(same))
    return worst


@pytest.mark.parametrize("bf16", [False, True], ids=["float", "bf16"])
def test_c1_sum(device, bf16):
    """d3f_kpconv_fused_c1, `aggregation == 0 && num_kp <= 15` -> kpconv_c1_kp_kernel<float> / <unsigned short> (out_bf16): 16
    queries per workgroup, passes of 64 neighbours walked in pairs (K = 2, 37, 64, 65, 130: odd K, one pass exactly, one more)."""
    name = "kpconv_c1_kp_kernel<%s>" % ("unsigned short" if bf16 else "float")
    _report(name, _c1_all(device, "c1_sum", "sum", bf16), "error / (2^-8 |want| + 5e-6 max |want|)" if bf16 else "error / (5e-6 max |want|)")


def test_c1_closest(device):
    """d3f_kpconv_fused_c1, aggregation 'closest' -> kpconv_c1_fused_kernel (lanes = neighbours, 8 queries per wavefront, 32 per
    block; fp32 output only: `out_bf16 && !(aggregation == 0 && num_kp <= 15)` is D3F_ERR_ARG)."""
    from oracle import kpconv_cases as kc
    _report("kpconv_c1_fused_kernel", _c1_all(device, "c1_closest", "closest"), "error / (5e-6 max |want|)")
    cfg = ("linear", "closest", 15)
    c = _case("errors", 1, 31, 37, cfg)
    W = kc.weights(1, 15, 1, 10)
    assert _c1(device, c, cfg, W, {}, bf16=True, abi=True) == ERR_ARG
    assert not isinstance(_c1(device, c, cfg, W, {}, abi=True), int)
    for over in (dict(Cout=0), dict(ldo=9), dict(ldf=0), dict(num_kp=16), dict(extent=0.0), dict(kp=None)):
        assert _c1(device, c, cfg, W, {}, abi=True, **over) == ERR_ARG, over
