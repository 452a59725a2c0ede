"""d3f_kpconv_backward / d3f_neighbor_transpose_qs on the GPU against the float64 definition (tests/kpconv_grad_np.py).

Table: ops.neighbor_transpose_supports and the C entry point equal the stable argsort integer for integer at Nq != Ns, with shadow
slots of all three kinds and capacity rows on both sides; for a square stack the table equals ops.neighbor_transpose word for word.

Gradients: every case and mode of kpconv_grad_np.GRID, outputs pre-filled with NaN, capacity rows holding NaN.  Tolerance per output:
the larger of 4 * err32 (tests/golden/kpconv_grad.npz: float32 torch-CPU autograd against float64) and the derived first-order bound
(kpconv_grad_np.tolerances, its largest entry), capped at 1e-4 of the largest entry compared.  Rows that nobody names are exact
zeros, rows of gf at or beyond the support count keep their pre-fill.

Bits: two calls, a table passed in or built inside, one output or both, strided operands, a concatenation of two independent stacks.
Autograd: kernels.autograd.kpconv_trainable gives the bits of ops.kpconv_backward.  Capture: table + backward in one torch.cuda.graph.

Measured on an MI355X over the 38 case-modes (printed by test_gradients_against_float64, never used as a bar): largest deviation
4.2e-7 of the largest entry of gf (c32k17 gaussian / sum) and 6.6e-7 of gW (c4 linear / sum); largest deviation / tolerance 0.024 (gf)
and 0.037 (gW), both at c1024 linear / sum; 4 * err32 is 3e-7 .. 2.6e-6 of the largest entry, the derived bound 4.7e-6 .. 1.5e-4 (it
is the one that counts everywhere, capped at 1e-4 for the gW of `slices`).  The 45 tests take 3 s.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import kpconv_grad_np as kg
from conftest import GOLDEN, bits
from oracle import kpconv_cases as kc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _count(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


def _tensors(c, W, gout, dev, cap=True):
    """The operands of a case on the device; cap: the capacity rows stay and the effective counts ride on the tags."""
    nq, ns = (len(c.q), len(c.s)) if cap else (c.Nq, c.Ns)
    a = dict(q=_t(c.q[:nq], dev), s=_t(c.s[:ns], dev), idx=_t(c.idx[:nq], dev), f=_t(c.f[:ns], dev), W=_t(W, dev), gout=_t(gout[:nq], dev))
    if cap:
        a["q"].n_dev, a["s"].n_dev = _count(c.Nq, dev), _count(c.Ns, dev)
    return a


def _backward(a, c, influence="linear", aggregation="sum", **kw):
    from d3feat_amd import ops
    return ops.kpconv_backward(a["q"], a["s"], a["idx"], a["f"], c.KP, a["W"], a["gout"], kg.EXTENT, influence, aggregation, **kw)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "kpconv_grad.npz"))
    return {str(k): z["err32"][i] for i, k in enumerate(z["keys"])}


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_table_against_the_stable_argsort(device):
    from d3feat_amd import _lib, ops
    c = kc.kpconv_case(811, 4, 9, 37, Ns=150, cap_q=5, cap_s=7)
    Nq, Ns, K = len(c.q), len(c.s), c.idx.shape[1]
    flat = c.idx[:c.Nq].reshape(-1)
    assert (flat == c.Ns).any() and (flat > c.Ns).any() and (flat < 0).any()              # shadow slots of all three kinds
    want_start, want_edges = kg.transpose_qs_np(c.idx, c.Nq, c.Ns, Ns)
    idx = _t(c.idx, device)
    start, edges = ops.neighbor_transpose_supports(idx, Ns, _count(c.Nq, device), _count(c.Ns, device))
    assert start.shape == (Ns + 1,) and edges.shape == (Nq * K,)
    assert np.array_equal(start.cpu().numpy(), want_start)
    assert np.array_equal(edges.cpu().numpy()[:len(want_edges)], want_edges)
    # the tag of the index matrix is the query count
    idx.n_dev = _count(c.Nq, device)
    start2, edges2 = ops.neighbor_transpose_supports(idx, Ns, ns_dev=_count(c.Ns, device))
    assert torch.equal(start2, start) and torch.equal(edges2[:len(want_edges)], edges[:len(want_edges)])
    # the C ABI: ld_idx > K (padding columns hold garbage), outputs pre-filled with -1
    lib = _lib.load()
    wide = np.full((Nq, K + 3), kc.GARBAGE, np.int32)
    wide[:, :K] = c.idx
    widx = _t(wide, device)
    s3 = torch.full((Ns + 1,), -1, dtype=torch.int32, device=device)
    e3 = torch.full((Nq * K,), -1, dtype=torch.int32, device=device)
    nbytes = lib.d3f_neighbor_transpose_workspace_bytes(Nq, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    nqd, nsd = _count(c.Nq, device), _count(c.Ns, device)
    rc = lib.d3f_neighbor_transpose_qs(widx.data_ptr(), Nq, K + 3, K, nqd.data_ptr(), Ns, nsd.data_ptr(), s3.data_ptr(), e3.data_ptr(),
                                       ws.data_ptr(), nbytes, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    assert rc == 0
    assert np.array_equal(s3.cpu().numpy(), want_start)
    got = e3.cpu().numpy()
    assert np.array_equal(got[:len(want_edges)], want_edges) and (got[len(want_edges):] == -1).all()


def test_square_table_equals_neighbor_transpose(device):
    from d3feat_amd import ops
    rng = np.random.default_rng(5)
    N, n, K = 90, 83, 11
    nb = rng.integers(-4, n + 6, (N, K)).astype(np.int32)
    lens = torch.tensor([40, 0, 43], dtype=torch.int32, device=device)
    t = _t(nb, device)
    s0, e0 = ops.neighbor_transpose(t, lens)
    s1, e1 = ops.neighbor_transpose_supports(t, N, _count(n, device), _count(n, device))
    valid = int(s0[-1].item())
    assert valid == int(((nb[:n] >= 0) & (nb[:n] < n)).sum())
    assert torch.equal(s0, s1) and torch.equal(e0[:valid], e1[:valid])


# ---- gradients against float64 ----------------------------------------------------------------------------------------------------
CASES = [(name, i, a) for name in kg.GRID for i, a in kg.modes_of(name)]


@pytest.mark.parametrize("name,influence,aggregation", CASES, ids=["%s-%s-%s" % t for t in CASES])
def test_gradients_against_float64(device, golden, name, influence, aggregation):
    c = kg.grid_case(name)
    W, gout = kg.grid_operands(name)
    res = kg.grid_gradients(name, influence, aggregation)
    Nq, Ns, Cin = c.Nq, c.Ns, c.f.shape[1]
    if Nq >= 4:                                                    # the two rows without a valid slot
        assert not res["valid"][1].any() and not res["valid"][Nq // 2].any()
    idx = np.where(res["valid"], c.idx[:Nq], -1)
    if idx.shape[1] >= 17 and Nq >= 7:                             # supports named several times by one query
        assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in idx)
    a = _tensors(c, W, gout, device)
    gf = torch.full((len(c.s), Cin), float("nan"), device=device)
    gW = torch.full(W.shape, float("nan"), device=device)
    out = _backward(a, c, influence, aggregation, out_features=gf, out_weights=gW)
    assert out[0] is gf and out[1] is gW
    gf, gW = gf.cpu().numpy(), gW.cpu().numpy()
    assert np.isnan(gf[Ns:]).all()                                 # rows at or beyond ns are left alone
    assert np.isfinite(gf[:Ns]).all() and np.isfinite(gW).all()
    named = np.zeros(Ns, bool)
    named[res["safe"][res["valid"]]] = True
    if idx.shape[1] == 1 or Nq <= 7:
        assert (~named).any()
    assert (gf[:Ns][~named] == 0).all()                            # supports nobody names: exact zeros
    tol_f, tol_w = kg.tolerances(res)
    err32 = golden["%s/%s/%s" % (name, influence, aggregation)]
    for label, got, want, bound, e32 in (("gf", gf[:Ns], res["gf"], tol_f, err32[0]), ("gW", gW, res["gW"], tol_w, err32[1])):
        big = np.abs(want).max()
        tol = kg.cap(max(4 * e32, bound.max()), big)
        dev = np.abs(got - want).max()
        print("%s %s/%s %s: largest %.3e, deviation %.2e of it, tolerance %.2e of it (4 err32 %.2e, bound %.2e), deviation / tolerance %.3f" % (
            name, influence, aggregation, label, big, dev / big, tol / big, 4 * e32 / big, bound.max() / big, dev / tol))
        assert dev <= tol, label


def test_no_neighbour_slot_and_no_query_give_exact_zeros(device):
    from d3feat_amd import ops
    c = kc.kpconv_case(33, 32, 5, 20, Ns=40)
    W = kc.weights(33, 15, 32, 16)
    s, f, Wt = _t(c.s, device), _t(c.f, device), _t(W, device)
    for Nq, K in ((20, 0), (0, 5)):
        q = _t(c.q[:Nq], device)
        idx = torch.zeros((Nq, K), dtype=torch.int32, device=device)
        gout = torch.ones((Nq, 16), device=device)
        gf = torch.full((40, 32), float("nan"), device=device)
        gW = torch.full((15, 32, 16), float("nan"), device=device)
        ops.kpconv_backward(q, s, idx, f, c.KP, Wt, gout, kg.EXTENT, out_features=gf, out_weights=gW)
        assert (gf == 0).all() and (gW == 0).all(), (Nq, K)


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def _same(x, y):
    return np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()))


def test_repeated_partial_and_strided_calls_give_equal_bits(device):
    from d3feat_amd import ops
    name = "c32k17"
    c = kg.grid_case(name)
    W, gout = kg.grid_operands(name)
    Ns, Cin, Cout = c.Ns, 32, 32
    a = _tensors(c, W, gout, device)
    gf0, gW0 = _backward(a, c)
    gf1, gW1 = _backward(a, c)
    assert _same(gf0[:Ns], gf1[:Ns]) and _same(gW0, gW1)                                      # two calls
    table = ops.neighbor_transpose_supports(a["idx"], len(c.s), a["q"].n_dev, a["s"].n_dev)
    gf2, gW2 = _backward(a, c, transpose=table)
    assert _same(gf0[:Ns], gf2[:Ns]) and _same(gW0, gW2)                                      # a table passed in
    gf3, none = _backward(a, c, need_weights=False)
    assert none is None and _same(gf0[:Ns], gf3[:Ns])
    none, gW4 = _backward(a, c, need_features=False)
    assert none is None and _same(gW0, gW4)
    # a strided gout (column view, ldg > Cout) and a strided out_features
    block = torch.full((len(c.q), Cout + 9), float("nan"), device=device)
    block[:, 5:5 + Cout] = a["gout"]
    wide = torch.full((len(c.s), Cin + 12), float("nan"), device=device)
    b = dict(a, gout=block[:, 5:5 + Cout])
    gf5, gW5 = _backward(b, c, out_features=wide[:, 4:4 + Cin])
    assert _same(gf0[:Ns], wide[:Ns, 4:4 + Cin]) and _same(gW0, gW5)
    assert torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + Cin:]).all() and torch.isnan(wide[Ns:]).all()
    # an unaligned out_features (the scalar form of the segment gather)
    odd = torch.full((len(c.s), Cin + 1), float("nan"), device=device)
    _backward(a, c, out_features=odd[:, 1:], need_weights=False)
    assert _same(gf0[:Ns], odd[:Ns, 1:])


def test_concatenated_stacks_give_the_rows_of_the_stacks_alone(device):
    """gf of two independent stacks run as one call equals, row for row, the gf of each run alone (gW does not: its slices differ)."""
    A = kc.kpconv_case(901, 32, 17, 150, Ns=150)
    B = kc.kpconv_case(902, 32, 17, 70, Ns=90)
    W = kc.weights(901, 15, 32, 32)
    rng = np.random.default_rng(9)
    gA, gB = rng.standard_normal((150, 32)).astype(np.float32), rng.standard_normal((70, 32)).astype(np.float32)
    idxB = np.where((B.idx >= 0) & (B.idx < B.Ns), B.idx + A.Ns, np.where(B.idx >= B.Ns, B.idx + A.Ns + 1000, B.idx))
    idxA = np.where(A.idx >= A.Ns, A.idx + B.Ns + 1000, A.idx)
    both = kc.Case(q=np.concatenate([A.q, B.q]), s=np.concatenate([A.s, B.s]), idx=np.concatenate([idxA, idxB]).astype(np.int32),
                   f=np.concatenate([A.f, B.f]), KP=A.KP, Nq=220, Ns=240)
    B = kc.Case(B, KP=A.KP)
    alone = [_backward(_tensors(c, W, g, device, cap=False), c, need_weights=False)[0] for c, g in ((A, gA), (B, gB))]
    got = _backward(_tensors(both, W, np.concatenate([gA, gB]), device, cap=False), both, need_weights=False)[0]
    assert _same(got[:150], alone[0]) and _same(got[150:], alone[1])


# ---- autograd and capture -----------------------------------------------------------------------------------------------------------
def test_autograd_function_gives_the_bits_of_the_operator(device):
    from d3feat_amd.kernels.autograd import kpconv_trainable
    from d3feat_amd.kernels.convolution_ops import KPConv_ops
    for name in ("c32k17", "c5"):
        c = kg.grid_case(name)
        W, gout = kg.grid_operands(name)
        a = _tensors(c, W, gout, device, cap=False)
        f = a["f"].clone().requires_grad_(True)
        Wp = a["W"].clone().requires_grad_(True)
        out = kpconv_trainable(a["q"], a["s"], a["idx"], f, c.KP, Wp, kg.EXTENT, "linear", "sum")
        want_out = KPConv_ops(a["q"], a["s"], a["idx"], a["f"], c.KP, a["W"], kg.EXTENT, "linear", "sum")
        assert _same(out.detach(), want_out)
        (out * a["gout"]).sum().backward()
        gf, gW = _backward(a, c)
        assert _same(f.grad, gf) and _same(Wp.grad, gW), name


def test_capture_then_replay_on_other_gradients(device):
    """Table and backward hold no host decision: captured once in torch.cuda.graph, replayed twice on other gout written into the same
    tensor, they give the bits of direct calls."""
    from d3feat_amd import ops
    name = "c32k17"
    c = kg.grid_case(name)
    W, gout = kg.grid_operands(name)
    a = _tensors(c, W, gout, device)
    gf = torch.zeros((len(c.s), 32), device=device)
    gW = torch.zeros(W.shape, device=device)
    stream = torch.cuda.Stream(device=device)

    def call():
        table = ops.neighbor_transpose_supports(a["idx"], len(c.s), a["q"].n_dev, a["s"].n_dev)
        _backward(a, c, transpose=table, out_features=gf, out_weights=gW)
        return table
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            call()                                                   # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                table = call()
    stream.synchronize()
    rng = np.random.default_rng(12)
    for _ in range(2):
        g = rng.standard_normal(gout.shape).astype(np.float32)
        a["gout"].copy_(_t(g, device))
        gf.fill_(float("nan"))
        gW.fill_(float("nan"))
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        want_f, want_w = _backward(a, c)
        assert _same(gf[:c.Ns], want_f[:c.Ns]) and _same(gW, want_w)
    del pw, table
