"""d3f_batch_norm_train / d3f_batch_norm_backward / d3f_gemm_tn_f32 on the GPU against the float64 definition (tests/bn_grad_np.py).

Every case of bn_grad_np.GRID: operands embedded in NaN-filled buffers (capacity rows, padding columns), outputs pre-filled with NaN.
Tolerance per output: the larger of 4 * err32 (tests/golden/bn_grad.npz: float32 torch-CPU autograd against float64) and the derived
first-order bound (bn_grad_np.tolerances), capped at 1e-4 of the largest entry compared; y, gx and gres are compared PER COLUMN against
that column's largest entry.  The batch variance is read through the moving update: with momentum 0 and a zero moving variance the
update returns it bit for bit.  The largest measured deviations are printed, never used as a bar.

Bits: the moving update, aliases, two calls, capture and replay with n changed on the device, the autograd wrappers, gemm_tn against the
gW of d3f_kpconv_backward.

Measured on an MI355X over the 31 cases (printed by test_against_float64, never used as a bar): largest deviation 2.2e-7 of the column's
largest entry for y (c130p4), 5.2e-7 for gx (n2), 6.6e-8 for gres (n2); 8.6e-8 of the largest entry for ggamma (c16p4), 4.8e-8 for gbeta,
5.4e-8 for mean, 4.5e-8 for rstd, 5.0e-8 for var; largest deviation / tolerance 0.45 (gx, f_l1_r1_bn), and 0.91 for mean, whose bound is
the one rounding 2^-24 |mean|.  unary_backward: 4.4e-7 (gx) and 7.8e-7 (gW) of the largest entry.  The 48 tests take 3 s.
"""
import os

import numpy as np
import pytest
import torch

import bn_grad_np as bg
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _count(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


def _same(x, y):
    return np.array_equal(bits(x.detach().cpu().numpy()), bits(y.detach().cpu().numpy()))


def _embed(a, n, C, pad, dev, n_dev=None):
    """rows [:n] of a NaN-filled [n + CAP_ROWS, C + pad] buffer -> the [:, :C] view (leading dimension C + pad), tagged with n."""
    buf = torch.full((n + bg.CAP_ROWS, C + pad), NAN, dtype=torch.float32, device=dev)
    if a is not None:
        buf[:n, :C] = _t(a, dev)
    view = buf[:, :C]
    view.n_dev = n_dev if n_dev is not None else _count(n, dev)
    return buf, view


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "bn_grad.npz"))
    return {k: z[k] for k in z.files if k != "keys"}


class Run:
    """One case on the device: the operands at construction; go() runs forward (moving statistics at `momentum`) and backward and
    keeps everything."""

    def __init__(self, c, dev, momentum=0.99, moving=True, alias_y=False, alias_gx=False, alias_gres=False, n_dev=None, go=True):
        n, C, pad = c.n, c.C, c.pad
        self.c, self.momentum = c, momentum
        self.n_dev = n_dev if n_dev is not None else _count(n, dev)
        self.xb, self.x = _embed(c.x, n, C, pad, dev, self.n_dev)
        self.rb, self.res = _embed(c.residual, n, C, pad, dev, self.n_dev) if c.residual is not None else (None, None)
        self.gb, self.gy = _embed(c.gy, n, C, pad, dev, self.n_dev)
        self.gamma = _t(c.gamma, dev) if c.gamma is not None else None
        self.beta = _t(c.beta, dev)
        self.mm = _t(c.moving_mean, dev) if moving else None
        self.mv = _t(c.moving_var, dev) if moving else None
        self.yb, self.y = (self.rb, self.res) if alias_y else _embed(None, n, C, pad, dev, self.n_dev)
        self.gxb, self.gx = (self.gb, self.gy) if alias_gx else _embed(None, n, C, pad, dev, self.n_dev)
        self.grb, self.gres = _embed(None, n, C, pad, dev, self.n_dev) if c.residual is not None else (None, None)
        if alias_gres:
            self.grb, self.gres = self.gb, self.gy
        if go:
            self.go()

    def go(self):
        from d3feat_amd import ops
        c = self.c
        out = ops.batch_norm_train(self.x, self.gamma, self.beta, bg.EPS, self.res, c.leaky, bg.ALPHA, self.mm, self.mv, self.momentum,
                                   out=self.y)
        assert out[0] is self.y
        self.mean, self.rstd = out[1], out[2]
        back = ops.batch_norm_backward(self.x, self.y, self.gy, self.gamma, self.mean, self.rstd, c.leaky, bg.ALPHA,
                                       need_residual=c.residual is not None, out=self.gx, out_residual=self.gres)
        assert back[0] is self.gx and back[3] is self.gres
        self.ggamma, self.gbeta = back[1], back[2]

    def outputs(self):
        return [t for t in (self.yb, self.mean, self.rstd, self.gxb, self.grb, self.ggamma, self.gbeta, self.mm, self.mv) if t is not None]


def _batch_variance(c, dev):
    """(mean, var) as the device hands them to the moving update: momentum 0 on zero moving statistics returns them bit for bit."""
    from d3feat_amd import ops
    _, x = _embed(c.x, c.n, c.C, c.pad, dev)
    mm, mv = torch.zeros(c.C, device=dev), torch.zeros(c.C, device=dev)
    ops.batch_norm_train(x, _t(c.gamma, dev), _t(c.beta, dev), bg.EPS, moving_mean=mm, moving_variance=mv, momentum=0.0)
    return mm.cpu().numpy(), mv.cpu().numpy()


def _check(label, name, got, want, bound, e32, per_column):
    """The project's rule.  -> deviation / tolerance (the largest over the columns)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), (name, label)
    if per_column:
        big, dev = np.abs(want).max(0), np.abs(got - want).max(0)
    else:
        big, dev = np.abs(want).max(), np.abs(got - want).max()
    tol = bg.cap(np.maximum(4 * e32, bound), big)
    worst = np.max(dev / np.maximum(tol, 1e-300))
    rel = np.max(dev / np.maximum(big, 1e-300))
    print("%s %s: deviation %.2e of the largest entry%s, deviation / tolerance %.3f" % (name, label, rel, " of its column" if per_column else
                                                                                       "", worst))
    assert (dev <= tol).all(), (name, label, float(worst))
    return worst


@pytest.mark.parametrize("name", list(bg.GRID))
def test_against_float64(device, golden, name):
    c = bg.grid_case(name)
    fw, bw = bg.grid_reference(name)
    n, C, pad = c.n, c.C, c.pad
    r = Run(c, device)
    tol = bg.tolerances(fw, bw, c.gamma, c.beta, c.residual, c.x, c.leaky)
    e32 = lambda out: golden.get("%s/%s" % (name, out), 0.0)                                   # noqa: E731
    for label, buf, want in (("y", r.yb, fw["y"]), ("gx", r.gxb, bw["gx"]), ("gres", r.grb, bw["gres"])):
        if buf is None:
            continue
        got = buf.cpu().numpy()
        assert np.isnan(got[n:]).all() and np.isnan(got[:, C:]).all(), label                   # capacity rows and padding are left alone
        _check(label, name, got[:n, :C], want, tol[label], e32(label), True)
    _check("gbeta", name, r.gbeta.cpu().numpy(), bw["gbeta"], tol["gbeta"], e32("gbeta"), False)
    if c.gamma is None:
        assert r.mean is None and r.rstd is None and r.ggamma is None
        return
    _check("ggamma", name, r.ggamma.cpu().numpy(), bw["ggamma"], tol["ggamma"], e32("ggamma"), False)
    mean = r.mean.cpu().numpy()
    _check("mean", name, mean[0], fw["mean"], tol["mean"], 0.0, False)
    both = mean[0].astype(np.float64) + mean[1].astype(np.float64)                             # the two parts: the float64 mean
    assert (np.abs(both - fw["mean"]) <= 2.0 ** -44 * (np.abs(fw["mean"]) + np.abs(c.x).max(0))).all()
    _check("rstd", name, r.rstd.cpu().numpy(), fw["rstd"], tol["rstd"], 0.0, False)
    bm, bv = _batch_variance(c, device)
    assert np.array_equal(bits(bm), bits(mean[0]))
    _check("var", name, bv, fw["var"], tol["var"], 0.0, False)
    assert (np.abs(bv - fw["var"]) <= 1e-5 * fw["var"]).all()                                  # every column, the offset column included
    # the moving statistics: TF's three fp32 operations on what the device returned
    assert np.array_equal(bits(r.mm.cpu().numpy()), bits(bg.moving_update(c.moving_mean, bm, 0.99)))
    assert np.array_equal(bits(r.mv.cpu().numpy()), bits(bg.moving_update(c.moving_var, bv, 0.99)))
    if c.special == "constant":
        assert (bv == 0).all()                                                                 # var == 0 exactly
        gx = r.gx.cpu().numpy()[:n]
        assert (gx[:, 0] == 0).all() and (n > 1 or (gx == 0).all())                            # exactly zero gx
    if c.special == "offset":
        assert abs(fw["mean"][0] - 1e3) < 1e-2 and fw["var"][0] < 2e-4
        # a one-pass sum of squares in fp32 is nowhere near (why the definition is two passes, and why the sums are float64)
        x32 = c.x[:, 0]
        one_pass = np.float32((x32 * x32).sum(dtype=np.float32) / np.float32(n)) - np.float32(x32.sum(dtype=np.float32) / np.float32(n)) ** 2
        assert abs(one_pass - fw["var"][0]) > 1e-5 * fw["var"][0]
    if c.special == "zerogamma":
        assert (r.y.cpu().numpy()[:n, 0] == 0).all()                                           # y == 0 everywhere: the mask is alpha
        want = (c.gy[:, 0] * np.float32(bg.ALPHA)).astype(np.float32).astype(np.float64).sum()
        assert abs(r.gbeta.cpu().numpy()[0] - want) <= 4 * bg.U * np.abs(c.gy[:, 0]).sum()
        assert (r.gx.cpu().numpy()[:n, 0] == 0).all()


@pytest.mark.parametrize("momentum", [0.98, 0.99])
def test_moving_update_and_null_moving_pointers(device, momentum):
    c = bg.grid_case("c64")
    a = Run(c, device, momentum=momentum)
    bm, bv = _batch_variance(c, device)
    assert np.array_equal(bits(a.mm.cpu().numpy()), bits(bg.moving_update(c.moving_mean, bm, momentum)))
    assert np.array_equal(bits(a.mv.cpu().numpy()), bits(bg.moving_update(c.moving_var, bv, momentum)))
    assert not np.array_equal(a.mm.cpu().numpy(), c.moving_mean)
    b = Run(c, device, moving=False)                                                           # nothing else changes
    for p, q in ((a.yb, b.yb), (a.mean, b.mean), (a.rstd, b.rstd), (a.gxb, b.gxb), (a.ggamma, b.ggamma), (a.gbeta, b.gbeta)):
        assert _same(p, q)


@pytest.mark.parametrize("name", ["c32", "c32p1", "f_l1_r1_off", "c130p4"])
def test_aliases_and_repeated_calls_give_equal_bits(device, name):
    c = bg.grid_case(name)
    a, b = Run(c, device), Run(c, device)
    for p, q in zip(a.outputs(), b.outputs()):
        assert _same(p, q)                                                                     # two calls
    al = Run(c, device, alias_y=True, alias_gx=True)                                           # y on residual, gx on gy
    assert _same(al.yb, a.yb) and _same(al.gxb, a.gxb) and _same(al.grb, a.grb) and _same(al.gbeta, a.gbeta)
    if c.gamma is not None:
        assert _same(al.ggamma, a.ggamma) and _same(al.mean, a.mean) and _same(al.rstd, a.rstd)
    ar = Run(c, device, alias_gres=True)                                                       # gres on gy, gx on its own
    assert _same(ar.grb, a.grb) and _same(ar.gxb, a.gxb) and _same(ar.gbeta, a.gbeta)


def test_no_row_writes_nothing(device):
    """n == 0 on the device under a capacity of 9 rows, through the C ABI: every output and the moving statistics keep their pre-fill."""
    from d3feat_amd import _lib
    lib = _lib.load()
    M, C = 9, 32
    zero = _count(0, device)
    fill = lambda *shape: torch.full(shape, 7.5, dtype=torch.float32, device=device)           # noqa: E731
    x, gy = torch.full((M, C), NAN, device=device), torch.full((M, C), NAN, device=device)
    gamma, beta = torch.ones(C, device=device), torch.zeros(C, device=device)
    y, mean, rstd, mm, mv, gx, gres, ggamma, gbeta = fill(M, C), fill(2, C), fill(C), fill(C), fill(C), fill(M, C), fill(M, C), fill(C), fill(C)
    nbytes = lib.d3f_batch_norm_workspace_bytes(M, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    for g in (gamma, None):
        gp = g.data_ptr() if g is not None else None
        rc = lib.d3f_batch_norm_train(x.data_ptr(), C, M, C, gp, beta.data_ptr(), 1e-6, 0.99, mm.data_ptr(), mv.data_ptr(), None, 0, 1, 0.2,
                                      y.data_ptr(), C, mean.data_ptr(), rstd.data_ptr(), zero.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == 0
        rc = lib.d3f_batch_norm_backward(x.data_ptr(), C, y.data_ptr(), C, gy.data_ptr(), C, M, C, gp, mean.data_ptr(), rstd.data_ptr(), 1,
                                         0.2, gx.data_ptr(), C, ggamma.data_ptr(), gbeta.data_ptr(), gres.data_ptr(), C, zero.data_ptr(),
                                         ws.data_ptr(), nbytes, stream)
        assert rc == 0
        torch.cuda.synchronize(device)
        for t in (y, mean, rstd, mm, mv, gx, gres, ggamma, gbeta):
            assert (t == 7.5).all()
    # a capacity of zero rows is success before anything touches the device
    assert lib.d3f_batch_norm_train(None, C, 0, C, gamma.data_ptr(), beta.data_ptr(), 1e-6, 0.99, None, None, None, 0, 0, 0.2, None, C,
                                    mean.data_ptr(), rstd.data_ptr(), None, ws.data_ptr(), nbytes, stream) == 0


def test_capture_then_replay_with_other_row_counts(device):
    """Forward and backward hold no host decision: captured once in torch.cuda.graph and replayed with n changed on the device, they
    give the bits of direct calls."""
    from d3feat_amd import ops
    c = bg.grid_case("c64")
    n_dev = _count(c.n, device)
    stream = torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    r = Run(c, device, n_dev=n_dev, go=False)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            r.go()                                                       # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                r.go()
    stream.synchronize()
    for n in (c.n, 257, 1):
        n_dev.fill_(n)
        r.mm.copy_(_t(c.moving_mean, device))
        r.mv.copy_(_t(c.moving_var, device))
        for buf in (r.yb, r.gxb, r.grb):
            buf.fill_(NAN)
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        want = Run(c, device, n_dev=n_dev)
        for p, q in zip(r.outputs(), want.outputs()):
            assert _same(p, q), n
        assert torch.isnan(r.yb[n:]).all() and torch.isfinite(r.yb[:n, :c.C]).all()
    del pw


def test_autograd_wrappers_give_the_bits_of_the_operators(device):
    from d3feat_amd import ops
    from d3feat_amd.kernels.autograd import batch_norm_trainable, unary_trainable
    for name in ("c32", "f_l1_r1_off", "f_l0_r0_bn"):
        c = bg.grid_case(name)
        r = Run(c, device)
        n = c.n
        leaf = lambda a: None if a is None else _t(a, device).requires_grad_(True)             # noqa: E731
        x, gamma, beta, res = leaf(c.x), leaf(c.gamma), leaf(c.beta), leaf(c.residual)
        mm, mv = _t(c.moving_mean, device), _t(c.moving_var, device)
        y = batch_norm_trainable(x, gamma, beta, res, c.leaky, bg.ALPHA, mm, mv, 0.99, bg.EPS)
        assert _same(y, r.y[:n])
        (y * _t(c.gy, device)).sum().backward()
        assert _same(x.grad, r.gx[:n]) and _same(beta.grad, r.gbeta), name
        if gamma is not None:
            assert _same(gamma.grad, r.ggamma) and _same(mm, r.mm) and _same(mv, r.mv)
        if res is not None:
            assert _same(res.grad, r.gres[:n])
    rng = np.random.default_rng(3)
    x, W, gy = (_t(rng.standard_normal(s).astype(np.float32), device) for s in ((281, 64), (64, 32), (281, 32)))
    xl, Wl = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    out = unary_trainable(xl, Wl)
    assert _same(out, ops.gemm(x, W))
    (out * gy).sum().backward()
    gx, gW = ops.unary_backward(x, W, gy)
    assert _same(xl.grad, gx) and _same(Wl.grad, gW)


# ---- gemm_tn and the unary convolution's backward -----------------------------------------------------------------------------------
WIDTHS = (1, 3, 32, 33, 64, 128)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 128 * bg.SLICE + 1])
def test_unary_backward_against_float64(device, n):
    """Cin x Cout over WIDTHS^2 (a diagonal of it at 32,769 rows), capacity rows of NaN behind the real ones."""
    from d3feat_amd import ops
    rng = np.random.default_rng(n)
    pairs = [(a, b) for a in WIDTHS for b in WIDTHS]
    if n > 1000:
        pairs = [(3, 3), (1, 33), (33, 32), (64, 128), (128, 1)]
    xs = rng.standard_normal((n, max(WIDTHS))).astype(np.float32)
    gs = rng.standard_normal((n, max(WIDTHS))).astype(np.float32)
    worst = [0.0, 0.0]
    for cin, cout in pairs:
        W = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
        _, x = _embed(xs[:, :cin], n, cin, 0, device)
        _, gy = _embed(gs[:, :cout], n, cout, 0, device)
        gx, gW = ops.unary_backward(x, _t(W, device), gy)
        want_x, want_w = bg.unary_backward(xs[:, :cin], W, gs[:, :cout])
        tol_x, tol_w = bg.unary_tolerances(xs[:, :cin], W, gs[:, :cout])
        for k, (got, want, tol) in enumerate(((gx.cpu().numpy()[:n], want_x, tol_x), (gW.cpu().numpy(), want_w, tol_w))):
            big, dev = np.abs(want).max(), np.abs(got - want).max()
            assert np.isfinite(got).all() and dev <= bg.cap(tol, big), (cin, cout, k, dev / big)
            worst[k] = max(worst[k], dev / big)
    print("n %d: largest deviation %.2e of the largest entry of gx, %.2e of gW" % (n, worst[0], worst[1]))


def test_gemm_tn_strided_repeated_and_empty(device):
    from d3feat_amd import ops
    rng = np.random.default_rng(8)
    A, B = rng.standard_normal((300, 33)).astype(np.float32), rng.standard_normal((300, 7)).astype(np.float32)
    a, b = _t(A, device), _t(B, device)
    out = ops.gemm_tn(a, b)
    assert _same(out, ops.gemm_tn(a, b))
    _, av = _embed(A, 300, 33, 3, device)
    _, bv = _embed(B, 300, 7, 5, device)
    assert _same(out, ops.gemm_tn(av, bv))                          # leading dimensions and capacity rows change no bit
    av.n_dev = bv.n_dev = _count(0, device)
    assert (ops.gemm_tn(av, bv) == 0).all()                          # no row: exact zeros


@pytest.mark.parametrize("n,cin,cout", [(300, 32, 64), (513, 5, 3)])
def test_gemm_tn_is_the_gw_contraction_of_kpconv_backward(device, n, cin, cout):
    """One kernel point at the centre under the constant influence, every query its own only neighbour: wf = f and the count is 1, so
    d3f_kpconv_backward's gW is f^T gout -- by the same two kernels, slice for slice: equal bits."""
    from d3feat_amd import ops
    rng = np.random.default_rng(n)
    pts = _t(rng.random((n, 3)).astype(np.float32), device)
    idx = torch.arange(n, dtype=torch.int32, device=device).reshape(n, 1)
    f = _t(rng.standard_normal((n, cin)).astype(np.float32), device)
    gout = _t(rng.standard_normal((n, cout)).astype(np.float32), device)
    W = _t(rng.standard_normal((1, cin, cout)).astype(np.float32), device)
    _, gW = ops.kpconv_backward(pts, pts, idx, f, np.zeros((1, 3), np.float32), W, gout, 0.05, "constant", "sum", need_features=False)
    assert _same(gW[0], ops.gemm_tn(f, gout))
