"""d3feat_amd.ops.kpconv_backward / neighbor_transpose_supports without a GPU.  What is pinned is the DEFINITION (include/d3feat_amd.h,
tests/kpconv_grad_np.py): against float64 torch autograd of a line-by-line torch restatement of kernels/convolution_ops.py:161-255,
against difference quotients of oracle.network_np.kpconv_f64 (the forward that existing tests tie to the kernels), the fixture, the
rectangular table against a brute-force loop, and the argument errors that come before the device is asked."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import kpconv_grad_np as kg
from conftest import GOLDEN
from oracle import kpconv_cases as kc
from oracle import network_np


def test_restatement_against_torch_float64_autograd():
    """kpconv_grad_np.gradients against autograd of kpconv_grad_np.torch_kpconv in float64, every case of GRID and all six modes: 1e-12
    of the largest entry, both outputs."""
    for name in kg.GRID:
        c = kg.grid_case(name)
        assert kc.row_sums_decided(c.f[:c.Ns]) and kc.closest_decided(c)
        W, gout = kg.grid_operands(name)
        for influence, aggregation in kg.MODES:
            got = kg.gradients(c, W, gout, influence, aggregation)
            want = kg.torch_gradients(c, W, gout, influence, aggregation)
            for key, w in zip(("gf", "gW"), want):
                assert got[key].shape == w.shape
                assert np.abs(got[key] - w).max() <= 1e-12 * np.abs(w).max(), (name, influence, aggregation, key)


def test_restatement_against_difference_quotients_of_the_pinned_forward():
    """Central differences of F(f, W) = sum gout * out, out = oracle.network_np.kpconv_f64, in entries of f and of W.  While no row
    sum changes sign the counts are constants and F is a polynomial of degree one in every single entry: the central difference has no
    truncation error.  The step of an entry of f is the power of two at or below half of its row's |sum|, so the sum keeps its sign;
    the cases' condition |sum| >= 2^-10 sum |f| keeps that step at 2^-12 sum |f| or more, and rows whose sum is exactly 0 (where any
    step flips the count) are not perturbed.  The step of an entry of W is 2^-10.  All perturbed values are exact in float64.
    Tolerance: F is a sum of products gout h f W / cnt, evaluated in float64 through sums of K, num_kp Cin and Nq Cout terms; no term
    passes more than L = K + num_kp Cin + Nq Cout additions, so each of the two values carries at most (L + 16) 2^-53 T, T the sum of
    the absolute values of all the products (computed from the perturbed operands), and the quotient twice that over 2 step."""
    name = "c5"
    c = kg.grid_case(name)
    W, gout = kg.grid_operands(name)
    influence, aggregation = "gaussian", "sum"
    Nq, Ns = c.Nq, c.Ns
    f0, W0, g0 = c.f[:Ns].astype(np.float64), W.astype(np.float64), gout[:Nq].astype(np.float64)
    P, Cin, Cout = W0.shape
    K = c.idx.shape[1]
    L = K + P * Cin + Nq * Cout
    h, valid, safe = kg.influences(c, influence, aggregation)

    def value(f, Wv):
        _, _, out = network_np.kpconv_f64(c.q, c.s, c.idx, f, c.KP, Wv, kg.EXTENT, influence, aggregation, Nq=Nq, Ns=Ns)
        return (out * g0).sum()

    def terms(f, Wv, count):
        awf = np.einsum("nkp,nkc->npc", h, np.abs(f)[safe] * valid[:, :, None])
        return (np.einsum("npc,pco->no", awf, np.abs(Wv)) / np.maximum(count, 1)[:, None] * np.abs(g0)).sum()

    res = kg.gradients(c, W, gout, influence, aggregation)
    named = np.unique(safe[valid])
    sums = np.asarray([math.fsum(r) for r in f0])
    rows = [int(r) for r in named if sums[r] != 0][:6]
    assert len(rows) == 6
    worst = 0.0
    for r in rows:
        step = 2.0 ** math.floor(math.log2(abs(sums[r]) / 2))
        assert step >= 2.0 ** -12 * np.abs(f0[r]).sum() and abs(sums[r]) - step > 0
        for ch in range(Cin):
            fp, fm = f0.copy(), f0.copy()
            fp[r, ch] += step
            fm[r, ch] -= step
            assert (fp[r, ch] - f0[r, ch] == step) and (f0[r, ch] - fm[r, ch] == step)
            tol = 2 * (L + 16) * 2.0 ** -53 * max(terms(fp, W0, res["count"]), terms(fm, W0, res["count"])) / (2 * step)
            quotient = (value(fp, W0) - value(fm, W0)) / (2 * step)
            assert abs(quotient - res["gf"][r, ch]) <= tol, (r, ch, quotient, res["gf"][r, ch], tol)
            worst = max(worst, abs(quotient - res["gf"][r, ch]) / tol)
    step = 2.0 ** -10
    for p, ch, o in ((0, 0, 0), (3, 4, 2), (14, 2, 1), (7, 1, 0)):
        Wp, Wm = W0.copy(), W0.copy()
        Wp[p, ch, o] += step
        Wm[p, ch, o] -= step
        tol = 2 * (L + 16) * 2.0 ** -53 * max(terms(f0, Wp, res["count"]), terms(f0, Wm, res["count"])) / (2 * step)
        quotient = (value(f0, Wp) - value(f0, Wm)) / (2 * step)
        assert abs(quotient - res["gW"][p, ch, o]) <= tol, (p, ch, o)
        worst = max(worst, abs(quotient - res["gW"][p, ch, o]) / tol)
    print("largest |quotient - gradient| / tolerance: %.3f" % worst)
    assert tol < 1e-9 * np.abs(res["gW"]).max()


def test_fixture_against_the_restatement():
    """tests/golden/kpconv_grad.npz (tools/make_golden_kpconv_grad.py): the keys are the grid's cases and modes, the recorded largest
    entries are what the restatement gives today, and the float32 deviations are of the size of float32 rounding."""
    path = os.path.join(GOLDEN, "kpconv_grad.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    keys = [str(k) for k in z["keys"]]
    assert keys == ["%s/%s/%s" % (n, i, a) for n in kg.GRID for i, a in kg.modes_of(n)]
    assert [str(o) for o in z["outputs"]] == ["gf", "gW"]
    assert z["err32"].shape == z["largest"].shape == (len(keys), 2)
    assert (z["err32"] > 0).all() and (z["err32"] <= 2e-6 * z["largest"]).all()
    for at, key in enumerate(keys):
        name, influence, aggregation = key.split("/")
        res = kg.grid_gradients(name, influence, aggregation)
        for o, out in enumerate(("gf", "gW")):
            assert abs(np.abs(res[out]).max() - z["largest"][at, o]) <= 1e-12 * z["largest"][at, o], key


def test_tolerances_are_finite_and_small():
    """The derived bounds of every case and mode of the grid: finite, non-negative, and of the size of fp32 rounding against the
    largest entry (they are bounds of an fp32 evaluation, not an allowance)."""
    for name in kg.GRID:
        for influence, aggregation in kg.modes_of(name):
            res = kg.grid_gradients(name, influence, aggregation)
            tf_, tw = kg.tolerances(res)
            assert tf_.shape == res["gf"].shape and tw.shape == res["gW"].shape
            assert np.isfinite(tf_).all() and np.isfinite(tw).all() and (tf_ >= 0).all() and (tw >= 0).all()
            assert tf_.max() <= 1e-4 * np.abs(res["gf"]).max() and tw.max() <= 1e-3 * np.abs(res["gW"]).max(), (name, influence, aggregation)


def test_transpose_qs_np_against_a_brute_force_loop():
    """transpose_qs_np (argsort, searchsorted) against "who names j": a loop over j, edges in ascending e, at Nq != Ns."""
    rng = np.random.default_rng(4)
    for nq, ns, Nq, Ns, K in ((0, 5, 3, 5, 4), (7, 4, 7, 4, 0), (9, 30, 12, 33, 5), (40, 11, 40, 11, 17), (5, 0, 5, 3, 2)):
        idx = rng.integers(-3, ns + 4, (Nq, K)).astype(np.int32)
        if ns > 2 and nq > 1 and K:
            idx[1, :] = 2
            idx[idx == 0] = 1
        start, edges = kg.transpose_qs_np(idx, nq, ns, Ns)
        flat = idx[:nq].reshape(-1)
        pos = 0
        assert len(start) == Ns + 1
        for j in range(Ns + 1):
            assert start[j] == pos
            if j < ns:
                who = [e for e in range(nq * K) if flat[e] == j]
                assert edges[pos:pos + len(who)].tolist() == who
                pos += len(who)
        assert pos == len(edges) == int(((flat >= 0) & (flat < ns)).sum())


def _args(Nq=20, Ns=30, K=8, Cin=32, Cout=16, num_kp=15, **over):
    a = dict(query_points=torch.zeros(Nq, 3), support_points=torch.zeros(Ns, 3), neighbors_indices=torch.zeros(Nq, K, dtype=torch.int32),
             features=torch.zeros(Ns, Cin), K_points=np.zeros((num_kp, 3), np.float32), K_values=torch.zeros(num_kp, Cin, Cout),
             grad_out=torch.zeros(Nq, Cout), KP_extent=0.03)
    a.update(over)
    return a


def test_argument_errors():
    """The checks of kpconv_backward, neighbor_transpose_supports and the wrappers above them, made before the device is asked for."""
    from d3feat_amd import _lib
    from d3feat_amd.kernels.autograd import kpconv_trainable
    from d3feat_amd.kernels.convolution_ops import KPConv_ops_backward
    from d3feat_amd.ops import kpconv_backward, neighbor_transpose_supports
    with pytest.raises(TypeError):
        kpconv_backward(**_args(features=torch.zeros(30, 32, dtype=torch.float64)))
    with pytest.raises(TypeError):
        kpconv_backward(**_args(neighbors_indices=torch.zeros(20, 8, dtype=torch.int64)))
    with pytest.raises(TypeError):
        kpconv_backward(**_args(grad_out=np.zeros((20, 16), np.float32)))
    with pytest.raises(TypeError):
        kpconv_backward(**_args(K_values=torch.zeros(15, 32, 16, dtype=torch.float16)))
    with pytest.raises(ValueError, match="grad_out"):
        kpconv_backward(**_args(grad_out=torch.zeros(19, 16)))
    with pytest.raises(ValueError, match="grad_out"):
        kpconv_backward(**_args(grad_out=torch.zeros(20, 17)))
    with pytest.raises(ValueError, match="channels"):
        kpconv_backward(**_args(features=torch.zeros(30, 31)))
    with pytest.raises(ValueError, match="index rows"):
        kpconv_backward(**_args(neighbors_indices=torch.zeros(19, 8, dtype=torch.int32)))
    with pytest.raises(ValueError, match="feature rows"):
        kpconv_backward(**_args(features=torch.zeros(29, 32)))
    with pytest.raises(ValueError, match="K_points"):
        kpconv_backward(**_args(K_points=np.zeros((14, 3), np.float32)))
    with pytest.raises(ValueError, match="kernel points"):
        kpconv_backward(**_args(num_kp=16))
    with pytest.raises(ValueError, match="influence"):
        kpconv_backward(**_args(), KP_influence="cubic")
    with pytest.raises(ValueError, match="convolution mode"):
        kpconv_backward(**_args(), aggregation_mode="mean")
    with pytest.raises(ValueError, match="neither"):
        kpconv_backward(**_args(), need_features=False, need_weights=False)
    with pytest.raises(ValueError, match="no support"):
        kpconv_backward(**_args(Ns=0))
    with pytest.raises(ValueError, match="KP_extent"):
        kpconv_backward(**_args(KP_extent=0.0))
    with pytest.raises(ValueError, match="out_features"):
        kpconv_backward(**_args(), out_features=torch.zeros(30, 31))
    with pytest.raises(ValueError, match="out_weights"):
        kpconv_backward(**_args(), out_weights=torch.zeros(15, 32, 17))
    with pytest.raises(ValueError, match="transpose"):
        kpconv_backward(**_args(), transpose=(torch.zeros(30, dtype=torch.int32), torch.zeros(160, dtype=torch.int32)))
    with pytest.raises(TypeError):
        kpconv_backward(**_args(), transpose=(torch.zeros(31, dtype=torch.int64), torch.zeros(160, dtype=torch.int32)))
    with pytest.raises(TypeError):
        neighbor_transpose_supports(torch.zeros(20, 8), 30)
    with pytest.raises(ValueError, match="num_supports"):
        neighbor_transpose_supports(torch.zeros(20, 8, dtype=torch.int32), -1)
    with pytest.raises(ValueError, match="one int32"):
        neighbor_transpose_supports(torch.zeros(20, 8, dtype=torch.int32), 30, ns_dev=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        neighbor_transpose_supports(torch.zeros(20, 8, dtype=torch.int32), 30, nq_dev=torch.zeros(1, dtype=torch.int64))
    # well-formed host tensors: there is no CPU path
    with pytest.raises(_lib.D3FeatLibraryError):
        kpconv_backward(**_args())
    with pytest.raises(_lib.D3FeatLibraryError):
        neighbor_transpose_supports(torch.zeros(20, 8, dtype=torch.int32), 30)
    a = _args()
    with pytest.raises(_lib.D3FeatLibraryError):
        KPConv_ops_backward(a["query_points"], a["support_points"], a["neighbors_indices"], a["features"], a["K_points"], a["K_values"], 0.03,
                            "linear", "sum", a["grad_out"])
    with pytest.raises(_lib.D3FeatLibraryError):
        kpconv_trainable(a["query_points"], a["support_points"], a["neighbors_indices"], a["features"], a["K_points"], a["K_values"], 0.03)


def test_entry_points_refuse_bad_sizes_before_the_device():
    from d3feat_amd import _lib
    lib = _lib.load()
    for name in ("d3f_neighbor_transpose_qs", "d3f_kpconv_backward", "d3f_kpconv_backward_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def transpose(Nq=10, ld=8, K=8, Ns=12, start=p, edges=p, idx=p, ws=(p, 1 << 16)):
        return lib.d3f_neighbor_transpose_qs(idx, Nq, ld, K, None, Ns, None, start, edges, ws[0], ws[1], None)
    for bad in (dict(Nq=1 << 20, ld=1 << 11, K=1 << 11), dict(Nq=524287, ld=4096, K=4096), dict(ld=7), dict(Ns=-1), dict(start=None),
                dict(edges=None), dict(idx=None), dict(Nq=-1), dict(K=-1, ld=0)):
        assert transpose(**bad) == -3, bad
    assert transpose(ws=(p, 64)) == -2 and transpose(ws=(None, 0)) == -2

    size = lib.d3f_kpconv_backward_workspace_bytes
    big = 1 << 30
    kp = (ctypes.c_float * 45)()

    def backward(Nq=4, Ns=6, ld=8, K=8, ldf=32, Cin=32, num_kp=15, extent=0.03, influence=1, aggregation=0, W=p, gout=p, ldg=16, Cout=16,
                 start=p, edges=p, gf=p, ldgf=32, gW=p, bf16=0, q=p, s=p, idx=p, f=p, kph=kp, ws=(p, big)):
        return lib.d3f_kpconv_backward(q, Nq, s, Ns, idx, ld, K, f, ldf, Cin, kph, num_kp, extent, influence, aggregation, W, gout, ldg, Cout,
                                       start, edges, gf, ldgf, gW, None, None, None, bf16, ws[0], ws[1], None)
    for bad in (dict(Nq=-1), dict(Ns=-1), dict(K=-1, ld=0), dict(Cin=0, ldf=0, ldgf=0), dict(Cout=0, ldg=0), dict(ld=7), dict(ldf=31),
                dict(ldg=15), dict(ldgf=31), dict(num_kp=0), dict(num_kp=16), dict(influence=3), dict(influence=-1), dict(aggregation=2),
                dict(extent=0.0), dict(extent=float("nan")), dict(Nq=1 << 20, ld=1 << 11, K=1 << 11), dict(Nq=524287, ld=4096, K=4096),
                dict(W=None), dict(gout=None), dict(q=None), dict(s=None), dict(idx=None), dict(f=None), dict(kph=None), dict(start=None),
                dict(edges=None), dict(gf=None, gW=None), dict(Ns=0), dict(bf16=1)):
        assert backward(**bad) == -3, bad
    assert backward(ws=(p, 64)) == -2 and backward(ws=(None, 0)) == -2
    assert size(-1, 6, 8, 32, 16, 15) == 0 and size(4, -1, 8, 32, 16, 15) == 0 and size(4, 6, -1, 32, 16, 15) == 0
    assert size(4, 6, 8, 0, 16, 15) == 0 and size(4, 6, 8, 32, 0, 15) == 0 and size(4, 6, 8, 32, 16, 0) == 0 and size(4, 6, 8, 32, 16, 16) == 0
    assert size(4, 0, 8, 32, 16, 15) == 0 and size(1 << 20, 6, 1 << 11, 32, 16, 15) == 0 and size(524287, 6, 4096, 32, 16, 15) == 0
    assert 0 < size(0, 0, 8, 32, 16, 15) <= size(4, 6, 8, 32, 16, 15) <= size(1000, 900, 8, 32, 16, 15) <= size(30000, 30000, 40, 32, 32, 15)
    # wf / gwf, msg and the partials of ceil(Nq / 256) slices
    Nq, K, Cin, Cout = 30000, 40, 32, 32
    assert size(Nq, 30000, K, Cin, Cout, 15) >= 4 * (Nq * 15 * Cin + Nq * K * Cin + -(-Nq // 256) * 15 * Cin * Cout)
