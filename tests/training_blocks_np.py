"""TEST INFRASTRUCTURE ONLY.  The encoder blocks in training mode (models/network_blocks.py with training=True: unary, simple, resnetb)
restated in float64 numpy from bn_grad_np (batch norm, the unary convolution's backward) and kpconv_grad_np (the KPConv's backward), a
torch restatement of the same compositions for autograd, and the one geometry the CPU and the GPU tests share.

    geometry()                                  two clouds of 150 + 131 points, 12 neighbour slots (shadow index 281), 15 kernel points
    BLOCKS                                      name -> (block type, Cin, fdim)
    block_variables(name, use_bn)               {full variable name: float32 array}, in the blocks' creation order
    reference(name, use_bn)                     float64: dict(out, gfeat, grads {variable: gradient}, moving {variable: updated})
    torch_reference(name, use_bn, dtype)        the same by torch autograd (moving statistics apart)
"""
import functools
from types import SimpleNamespace

import numpy as np

import bn_grad_np as bg
import kpconv_grad_np as kg
from oracle import kpconv_cases as kc
from oracle import network_np

LENS = (150, 131)
N = sum(LENS)
K = 12
NUM_KP = 15
MOMENTUM = 0.98
BLOCKS = {"unary": ("unary", 16, 32), "simple": ("simple", 16, 32), "resnetb_shortcut": ("resnetb", 16, 32),
          "resnetb_identity": ("resnetb", 64, 32)}
INFLUENCE, AGGREGATION = "linear", "sum"


def scope_of(name):
    return "layer_0/%s_0" % BLOCKS[name][0]


@functools.lru_cache(maxsize=None)
def geometry():
    rng = np.random.default_rng(77)
    pts = (rng.random((N, 3)) * 0.25).astype(np.float32)
    nb = np.full((N, K), N, np.int32)
    lo = 0
    for n in LENS:
        p = pts[lo:lo + n].astype(np.float64)
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        order = np.argsort(d, 1, kind="stable")[:, :K]
        near = np.take_along_axis(d, order, 1) <= 0.06
        nb[lo:lo + n] = np.where(near, order + lo, N)
        lo += n
    assert (nb == N).any() and (nb[:, 0] == np.arange(N)).all()
    return SimpleNamespace(points=pts, neighbors=nb, lens=np.asarray(LENS, np.int32), KP=kc.kernel_points(3, NUM_KP))


def make_config(use_bn):
    """-> (config, radius): the block's extent KP_extent * radius / density_parameter is oracle.kpconv_cases.EXTENT."""
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    cfg.num_kernel_points = NUM_KP
    cfg.KP_influence, cfg.convolution_mode = INFLUENCE, AGGREGATION
    cfg.use_batch_norm = bool(use_bn)
    cfg.batch_norm_momentum = MOMENTUM
    cfg.KP_extent, cfg.density_parameter = 1.0, 5.0
    return cfg, 5.0 * kc.EXTENT


def _seed(name, use_bn):
    return 500 + 17 * sorted(BLOCKS).index(name) + (1 if use_bn else 0)


def _draw(name, use_bn, seed):
    kind, cin, fdim = BLOCKS[name]
    rng = np.random.default_rng(seed)
    V = {}

    def weights(scope, shape):
        fan = int(np.prod(shape[:-1])) if len(shape) == 2 else shape[1] * 4
        V[scope + "/weights"] = (rng.standard_normal(shape) / np.sqrt(fan)).astype(np.float32)

    def bn(scope, ch):
        if not use_bn:
            V[scope + "/offset"] = (0.1 * rng.standard_normal(ch)).astype(np.float32)
            return
        b = scope + "/batch_normalization/"
        V[b + "gamma"] = (1.0 + 0.2 * rng.standard_normal(ch)).astype(np.float32)
        V[b + "beta"] = (0.1 * rng.standard_normal(ch)).astype(np.float32)
        V[b + "moving_mean"] = (0.1 * rng.standard_normal(ch)).astype(np.float32)
        V[b + "moving_variance"] = (0.5 + rng.random(ch)).astype(np.float32)

    def kpconv(scope, ci, co):
        weights(scope, (NUM_KP, ci, co))
        V[scope + "/kernel_points"] = geometry().KP

    s = scope_of(name)
    if kind == "unary":
        weights(s, (cin, fdim)); bn(s, fdim)
        cout = fdim
    elif kind == "simple":
        kpconv(s, cin, fdim); bn(s, fdim)
        cout = fdim
    else:
        weights(s + "/conv1", (cin, fdim // 2)); bn(s + "/conv1", fdim // 2)
        kpconv(s + "/conv2", fdim // 2, fdim // 2); bn(s + "/conv2", fdim // 2)
        weights(s + "/conv3", (fdim // 2, 2 * fdim)); bn(s + "/conv3", 2 * fdim)
        if cin != 2 * fdim:
            weights(s + "/shortcut", (cin, 2 * fdim)); bn(s + "/shortcut", 2 * fdim)
        cout = 2 * fdim
    feats = rng.standard_normal((N, cin)).astype(np.float32)
    R = rng.standard_normal((N, cout)).astype(np.float32)
    return V, feats, R


# ---- float64 numpy ------------------------------------------------------------------------------------------------------------------
class _Tape:
    """The block's layers on float64 arrays: every layer returns its output and pushes its backward."""

    def __init__(self, V, use_bn, scope):
        self.V = {k: np.asarray(v, np.float64) for k, v in V.items()}
        self.use_bn, self.scope = use_bn, scope
        self.grads, self.moving, self.margin = {}, {}, np.inf

    def unary(self, sub, x):
        name = self.scope + sub + "/weights"
        W = self.V[name]

        def back(g):
            gx, gW = bg.unary_backward(x, W, g)
            self.grads[name] = gW
            return gx
        return x @ W, back

    def kpconv(self, sub, x):
        geo = geometry()
        name = self.scope + sub + "/weights"
        W = self.V[name]
        case = kc.Case(q=geo.points, s=geo.points, idx=geo.neighbors, f=x, KP=geo.KP, Nq=N, Ns=N)
        out = network_np.kpconv_f64(geo.points, geo.points, geo.neighbors, x, geo.KP, W, kc.EXTENT, INFLUENCE, AGGREGATION)[2]
        sums = np.abs(x.sum(1))
        self.margin = min(self.margin, sums.min() / np.abs(x).sum(1).max())          # the row-positive flags are decided

        def back(g):
            res = kg.gradients(case, W, g, INFLUENCE, AGGREGATION)
            self.grads[name] = res["gW"]
            return res["gf"]
        return out, back

    def bn(self, sub, x, leaky, residual=None):
        s = self.scope + sub
        if self.use_bn:
            b = s + "/batch_normalization/"
            gamma, beta = self.V[b + "gamma"], self.V[b + "beta"]
        else:
            gamma, beta = None, self.V[s + "/offset"]
        fw = bg.forward(x, gamma, beta, bg.EPS, residual, leaky)
        if leaky:
            self.margin = min(self.margin, np.abs(fw["z"]).min())
        if self.use_bn:
            f = np.float64(bg.one_minus(MOMENTUM))
            for key, batch in (("moving_mean", fw["mean"]), ("moving_variance", fw["var"])):
                self.moving[b + key] = self.V[b + key] - (self.V[b + key] - batch) * f

        def back(g):
            bw = bg.backward(fw, g, gamma, leaky)
            if self.use_bn:
                self.grads[b + "gamma"], self.grads[b + "beta"] = bw["ggamma"], bw["gbeta"]
            else:
                self.grads[s + "/offset"] = bw["gbeta"]
            return bw["gx"], bw["gres"]
        return fw["y"], back


def _run(name, use_bn, V, feats, R):
    kind, cin, fdim = BLOCKS[name]
    t = _Tape(V, use_bn, scope_of(name))
    f = np.asarray(feats, np.float64)
    G = np.asarray(R, np.float64)
    if kind in ("unary", "simple"):
        a, back_a = (t.unary if kind == "unary" else t.kpconv)("", f)
        out, back_n = t.bn("", a, True)
        gfeat = back_a(back_n(G)[0])
    else:
        a1, b_u1 = t.unary("/conv1", f)
        x1, b_n1 = t.bn("/conv1", a1, True)
        a2, b_k2 = t.kpconv("/conv2", x1)
        x2, b_n2 = t.bn("/conv2", a2, True)
        a3, b_u3 = t.unary("/conv3", x2)
        if cin != 2 * fdim:
            asc, b_us = t.unary("/shortcut", f)
            sc, b_ns = t.bn("/shortcut", asc, False)
        else:
            sc = f
        out, b_n3 = t.bn("/conv3", a3, True, residual=sc)
        g3, gsc = b_n3(G)
        gfeat = b_u1(b_n1(b_k2(b_n2(b_u3(g3))[0]))[0])
        gfeat = gfeat + (b_us(b_ns(gsc)[0]) if cin != 2 * fdim else gsc)
    return dict(out=out, gfeat=gfeat, grads=t.grads, moving=t.moving, margin=t.margin)


@functools.lru_cache(maxsize=None)
def block_case(name, use_bn):
    """(variables, features f32[281, Cin], R f32[281, Cout]): the first draw whose pre-activations under a LeakyReLU stay 1e-5 clear
    of zero and whose KPConv input rows have sums 1e-4 of their absolute sums clear of zero -- the masks and the neighbour counts of the
    fp32 evaluation are then the float64 ones."""
    for k in range(64):
        V, feats, R = _draw(name, use_bn, _seed(name, use_bn) + 1000 * k)
        if _run(name, use_bn, V, feats, R)["margin"] > 1e-5:
            return V, feats, R
    raise AssertionError(name)


def block_variables(name, use_bn):
    return block_case(name, use_bn)[0]


@functools.lru_cache(maxsize=None)
def reference(name, use_bn):
    return _run(name, use_bn, *block_case(name, use_bn))


# ---- the same compositions in torch, for autograd --------------------------------------------------------------------------------------
def torch_reference(name, use_bn, dtype="float64"):
    import torch
    dt = getattr(torch, dtype)
    kind, cin, fdim = BLOCKS[name]
    V, feats, R = block_case(name, use_bn)
    geo = geometry()
    s = scope_of(name)
    P = {k: torch.tensor(v, dtype=dt, requires_grad=not k.endswith(("kernel_points", "moving_mean", "moving_variance"))) for k, v in V.items()}
    f = torch.tensor(feats, dtype=dt, requires_grad=True)
    pts, KP = torch.tensor(geo.points, dtype=dt), torch.tensor(geo.KP, dtype=dt)
    idx = torch.tensor(geo.neighbors.astype(np.int64))

    def unary(sub, x):
        return x @ P[s + sub + "/weights"]

    def kpconv(sub, x):
        return kg.torch_kpconv(pts, pts, idx, x, KP, P[s + sub + "/weights"], kc.EXTENT, INFLUENCE, AGGREGATION)

    def bn(sub, x, leaky, residual=None):
        b = s + sub + "/batch_normalization/"
        if use_bn:
            return bg.torch_block(x, P[b + "gamma"], P[b + "beta"], residual, leaky)
        return bg.torch_block(x, None, P[s + sub + "/offset"], residual, leaky)

    if kind == "unary":
        out = bn("", unary("", f), True)
    elif kind == "simple":
        out = bn("", kpconv("", f), True)
    else:
        x = bn("/conv1", unary("/conv1", f), True)
        x = bn("/conv2", kpconv("/conv2", x), True)
        sc = bn("/shortcut", unary("/shortcut", f), False) if cin != 2 * fdim else f
        out = bn("/conv3", unary("/conv3", x), True, residual=sc)
    (out * torch.tensor(R, dtype=dt)).sum().backward()
    return dict(out=out.detach().double().numpy(), gfeat=f.grad.double().numpy(),
                grads={k: p.grad.double().numpy() for k, p in P.items() if p.requires_grad})
