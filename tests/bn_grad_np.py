"""TEST INFRASTRUCTURE ONLY.  Batch normalisation in training mode with its epilogue, its backward, and the backward of the unary
convolution (include/d3feat_amd.h: d3f_batch_norm_train, d3f_batch_norm_backward, d3f_gemm_tn_f32) in float64 numpy -- the definition
the device code is held to -- with first-order error bounds of the fp32 evaluation, a torch restatement of
tf.layers.batch_normalization(training=True) for autograd, and the grid of cases the CPU and the GPU tests share.

    forward(x, gamma, beta, eps, residual, leaky, alpha)        -> dict(y, z, mean, var, rstd, xhat)
    moving_update(moving, batch, momentum)                      -> float32, TF's operation order
    backward(fw, gy, gamma, leaky, alpha)                       -> dict(gx, ggamma, gbeta, gres, g)
    unary_backward(x, W, gy)                                    -> (gx, gW)
    tolerances(case, fw, bw)                                    -> dict(output -> absolute bound; per column for y, gx, gres)
    cap(tol, largest)                                           -> min(tol, 1e-4 largest)
    GRID, grid_case(name), grid_reference(name)                 the cases
"""
import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
BAR = 1e-4                       # the project's cap: 1e-4 of the largest entry compared
EPS = 1e-6
ALPHA = 0.2
SLICE = 256                      # D3F_SLICE_MIN of csrc/common.h
CAP_ROWS = 5                     # capacity rows beyond n: NaN


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def forward(x, gamma, beta, eps=EPS, residual=None, leaky=False, alpha=ALPHA):
    """gamma None: the form without batch norm, z = x + beta [+ residual]."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    beta = np.asarray(beta, np.float64)
    if gamma is None:
        mean = var = rstd = xhat = None
        z = x + beta
    else:
        gamma = np.asarray(gamma, np.float64)
        mean = x.sum(0) / max(n, 1)
        var = ((x - mean) ** 2).sum(0) / max(n, 1)                # two passes, biased
        rstd = 1.0 / np.sqrt(var + eps)
        xhat = (x - mean) * rstd
        z = xhat * gamma + beta
    if residual is not None:
        z = z + np.asarray(residual, np.float64)
    y = np.where(z > 0, z, z * alpha) if leaky else z
    return dict(y=y, z=z, mean=mean, var=var, rstd=rstd, xhat=xhat, n=n)


def one_minus(momentum):
    """float32(1 - momentum), the difference taken in float64 from the float32 argument (the C ABI passes momentum as a float)."""
    return np.float32(1.0 - np.float64(np.float32(momentum)))


def moving_update(moving, batch, momentum):
    """moving <- moving - (moving - batch) * float32(1 - momentum): three fp32 operations, each rounded on its own."""
    moving, batch = np.asarray(moving, np.float32), np.asarray(batch, np.float32)
    delta = (moving - batch).astype(np.float32)
    step = (delta * one_minus(momentum)).astype(np.float32)
    return (moving - step).astype(np.float32)


def backward(fw, gy, gamma, leaky=False, alpha=ALPHA):
    """From the STORED y of the forward: g = gy (y > 0 ? 1 : alpha)."""
    gy = np.asarray(gy, np.float64)
    n = gy.shape[0]
    g = gy * np.where(fw["y"] > 0, 1.0, alpha) if leaky else gy
    gbeta = g.sum(0)
    if gamma is None:
        return dict(gx=g, ggamma=None, gbeta=gbeta, gres=g, g=g)
    gamma = np.asarray(gamma, np.float64)
    ggamma = (g * fw["xhat"]).sum(0)
    gx = gamma * fw["rstd"] * (g - gbeta / max(n, 1) - fw["xhat"] * ggamma / max(n, 1))
    return dict(gx=gx, ggamma=ggamma, gbeta=gbeta, gres=g, g=g)


def unary_backward(x, W, gy):
    x, W, gy = (np.asarray(a, np.float64) for a in (x, W, gy))
    return gy @ W.T, x.T @ gy


# ---- first-order bounds of the fp32 evaluation ------------------------------------------------------------------------------------
def tolerances(fw, bw, gamma, beta, residual, x, leaky):
    """Absolute bounds of d3f_batch_norm_train / _backward against float64, derived from the case (u = 2^-24, one rounding = u |v|).
    The column sums are float64 on the device, so a statistic carries the rounding of its result only:
      mean   the sum of the two fp32 parts: 2 u^2 |mean| -- taken as u |mean| for the first part compared alone;
      var    compared through the moving update and on its own: 4 u var (the float64 chain and one rounding);
      rstd   2 u rstd;
      xhat   ((x - m0) - m1) rstd: two subtractions and a product of rounded factors: d_xhat = 6 u |xhat| + 2 u^2 |mean| rstd;
      z      xhat gamma + beta + residual: |gamma| d_xhat + 3 u (|xhat gamma| + |beta| + |residual|); y adds u |y| under leaky;
      gbeta  2 u |gbeta| (+ u sum |g| under leaky: g is a rounded product);
      ggamma sum |g| d_xhat + 2 u sum |g xhat|;
      gx     gamma rstd ((g - kb) - xhat kg), kb = gbeta / n, kg = ggamma / n rounded:
             |gamma| rstd (6 u (|g| + |kb| + |xhat kg|) + d_xhat |kg| + |xhat| d_kg + d_kb), d_kb = d_gbeta / n + u |kb|, likewise d_kg;
      gres   u |g| (exact without leaky).
    -> dict; y, gx, gres are vectors over the columns (the largest bound of the column)."""
    n = max(fw["n"], 1)
    absx = np.abs(np.asarray(x, np.float64))
    absb = np.abs(np.asarray(beta, np.float64))
    absr = np.abs(np.asarray(residual, np.float64)) if residual is not None else 0.0
    g = np.abs(bw["g"])
    lk = 1.0 if leaky else 0.0
    if gamma is None:
        d_y = 3 * U * (absx + absb + absr) + lk * U * np.abs(fw["y"])
        return dict(y=d_y.max(0), gx=(lk * U * g + 1e-300).max(0), gres=(lk * U * g + 1e-300).max(0),
                    gbeta=(2 * U * np.abs(bw["gbeta"]) + lk * U * g.sum(0)).max() + 1e-300)
    ga = np.abs(np.asarray(gamma, np.float64))
    mean, rstd, xhat = np.abs(fw["mean"]), fw["rstd"], np.abs(fw["xhat"])
    d_xhat = 6 * U * xhat + 2 * U * U * mean * rstd
    d_y = ga * d_xhat + 3 * U * (xhat * ga + absb + absr) + lk * U * np.abs(fw["y"])
    d_gbeta = 2 * U * np.abs(bw["gbeta"]) + lk * U * g.sum(0)
    d_ggamma = (g * d_xhat).sum(0) + 2 * U * (g * xhat).sum(0) + lk * U * (g * xhat).sum(0)
    kb, kg = np.abs(bw["gbeta"]) / n, np.abs(bw["ggamma"]) / n
    d_kb, d_kg = d_gbeta / n + U * kb, d_ggamma / n + U * kg
    d_gx = ga * rstd * (6 * U * (g + kb + xhat * kg) + d_xhat * kg + xhat * d_kg + d_kb)
    tiny = 1e-300
    return dict(y=d_y.max(0), mean=(U * mean).max() + tiny, var=(4 * U * fw["var"]).max() + tiny, rstd=(2 * U * rstd).max(),
                gx=d_gx.max(0) + tiny, gres=(lk * U * g).max(0) + tiny, gbeta=d_gbeta.max() + tiny, ggamma=d_ggamma.max() + tiny)


def term_scales(case, fw, bw):
    """The largest magnitude of the TERMS each output is made of, per output: two float64 evaluations that factor the expressions
    differently (x inv - mean inv against (x - mean) rstd) agree to a rounding of these, not of the result, where the result cancels
    (a constant column: xhat == 0 here, 1e-13 there)."""
    g = np.abs(bw["g"])
    n = max(fw["n"], 1)
    res = np.abs(case.residual).max() if case.residual is not None else 0.0
    if case.gamma is None:
        return dict(y=np.abs(case.x).max() + np.abs(case.beta).max() + res, gx=g.max(), gres=g.max(), gbeta=g.sum(0).max())
    ga = np.abs(np.asarray(case.gamma, np.float64))
    xh = (np.abs(np.asarray(case.x, np.float64)) + np.abs(fw["mean"])) * fw["rstd"]
    T = (g * xh).sum(0)
    return dict(y=(xh * ga).max() + np.abs(case.beta).max() + res, ggamma=T.max(), gbeta=g.sum(0).max(), gres=g.max(),
                gx=(ga * fw["rstd"] * (g + g.sum(0) / n + xh * T / n)).max())


def cap(tol, largest):
    return np.minimum(tol, BAR * largest)


def unary_tolerances(x, W, gy):
    """gx = gy W^T: Cout terms; gW = x^T gy: n terms (a slice's chain, then the chain over the slices).  (L + 16) u sum |terms|."""
    ax, aW, ag = (np.abs(np.asarray(a, np.float64)) for a in (x, W, gy))
    return ((W.shape[1] + 16) * U * (ag @ aW.T)).max(), ((x.shape[0] + 16) * U * (ax.T @ ag)).max()


# ---- the second statement: tf.layers.batch_normalization(training=True) line by line, in torch ------------------------------------
def torch_batch_norm_training(x, gamma, beta, eps=EPS):
    """The non-fused path of TF 1.x on a rank-2 input: nn.moments over axis 0 (the mean inside the variance behind a stop-gradient),
    then nn.batch_normalization's factoring."""
    mean = x.mean(0, keepdim=True)                                           # math_ops.reduce_mean(y, axes, keepdims=True)
    variance = ((x - mean.detach()) ** 2).mean(0, keepdim=True)              # reduce_mean(squared_difference(y, stop_gradient(mean)))
    mean, variance = mean.squeeze(0), variance.squeeze(0)
    inv = (variance + eps).rsqrt()                                           # inv = math_ops.rsqrt(variance + variance_epsilon)
    inv = inv * gamma                                                        # inv *= scale
    return x * inv + (beta - mean * inv), mean, variance                     # x * inv + (offset - mean * inv)


def torch_block(x, gamma, beta, residual, leaky, alpha=ALPHA):
    """batch_norm (either form of models/network_blocks.py:149-165), then the add and leaky_relu (:185-186)."""
    import torch
    z = torch_batch_norm_training(x, gamma, beta)[0] if gamma is not None else x + beta
    if residual is not None:
        z = z + residual
    return torch.nn.functional.leaky_relu(z, alpha) if leaky else z


def torch_gradients(case, dtype="float64"):
    """y and the gradients of sum(y gy) by torch autograd on the CPU, as float64 numpy."""
    import torch
    dt = getattr(torch, dtype)
    leaf = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)   # noqa: E731
    x, gamma, beta, res = leaf(case.x), leaf(case.gamma), leaf(case.beta), leaf(case.residual)
    y = torch_block(x, gamma, beta, res, case.leaky)
    (y * torch.tensor(case.gy, dtype=dt)).sum().backward()
    num = lambda t: None if t is None or t.grad is None else t.grad.double().numpy()                     # noqa: E731
    return dict(y=y.detach().double().numpy(), gx=num(x), ggamma=num(gamma), gbeta=num(beta), gres=num(res))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# name -> dict(n, C, pad (leading dimension = C + pad), leaky, residual, bn, special)
def _case(n, C, pad=0, leaky=True, residual=True, bn=True, special=None):
    return dict(n=n, C=C, pad=pad, leaky=leaky, residual=residual, bn=bn, special=special)


GRID = {}
for _n in (1, 2, 255, 256, 257):                                   # rows round the slice edge; constant columns at n <= 2
    GRID["n%d" % _n] = _case(_n, 32, special="constant" if _n <= 2 else None)
GRID["slices"] = _case(128 * SLICE + 1, 3)                         # 32,769 rows: the first capacity whose slices double to 512 rows
for _c in (1, 3, 16, 32, 64, 130, 256):                            # scalar and 16-byte quads, narrow and wide, two column blocks at 130
    GRID["c%d" % _c] = _case(300, _c)
    GRID["c%dp4" % _c] = _case(300, _c, pad=4)
GRID["c32p1"] = _case(300, 32, pad=1)                              # a vectorisable C on the scalar path
GRID["offset"] = _case(300, 8, special="offset")                   # column 0: mean 1e3, spread 1e-2
GRID["zerogamma"] = _case(300, 8, residual=False, special="zerogamma")   # column 0: gamma = beta = 0, y == 0 everywhere
for _l in (0, 1):
    for _r in (0, 1):
        for _b in (0, 1):
            GRID["f_l%d_r%d_%s" % (_l, _r, "bn" if _b else "off")] = _case(300, 32, leaky=bool(_l), residual=bool(_r), bn=bool(_b))


def _seed(name):
    return 9000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def _draw(name, spec, seed):
    rng = np.random.default_rng(seed)
    n, C = spec["n"], spec["C"]
    x = (rng.standard_normal((n, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.0, 1.0, C)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    residual = rng.standard_normal((n, C)).astype(np.float32) if spec["residual"] else None
    gy = rng.standard_normal((n, C)).astype(np.float32)
    if spec["special"] == "constant":
        # every column constant: var == 0 exactly.  (Two DIFFERENT points normalise to +-1 whatever they are, so their gx cancels to
        # eps / var of its terms: no fp32 evaluation can hold a relative bound there, and no network layer sees a batch of two.)
        x[:] = x[0]
        if n == 2:                                                 # column 0: equal rows throughout, gx is exactly zero there
            gy[1, 0] = gy[0, 0]
            if residual is not None:
                residual[1, 0] = residual[0, 0]
    elif spec["special"] == "offset":
        x[:, 0] = (1e3 + 1e-2 * rng.standard_normal(n)).astype(np.float32)
    elif spec["special"] == "zerogamma":
        gamma[0] = beta[0] = 0.0
    moving_mean = rng.standard_normal(C).astype(np.float32)
    moving_var = rng.uniform(0.5, 1.5, C).astype(np.float32)
    return SimpleNamespace(name=name, n=n, C=C, pad=spec["pad"], leaky=spec["leaky"], x=x, gamma=gamma if spec["bn"] else None, beta=beta,
                           residual=residual, gy=gy, moving_mean=moving_mean, moving_var=moving_var, special=spec["special"])


def _clear_of_zero(case):
    """No pre-activation within 1e-5 of zero (a column that is zero by construction apart; the fp32 evaluation is a few 1e-7 off): the
    LeakyReLU mask of the fp32 evaluation is then the float64 one."""
    if not case.leaky:
        return True
    z = np.abs(forward(case.x, case.gamma, case.beta, EPS, case.residual)["z"])
    if case.special == "zerogamma":
        assert (z[:, 0] == 0).all()
        z = z[:, 1:]
    return z.size == 0 or z.min() > 1e-5


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """The operands of a case: the first draw (seeds _seed(name), + 1000, ...) that keeps every pre-activation clear of zero."""
    for k in range(64):
        case = _draw(name, GRID[name], _seed(name) + 1000 * k)
        if _clear_of_zero(case):
            return case
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """The float64 definition of one case, computed once and shared (never modified by a test) -> (forward dict, backward dict)."""
    c = grid_case(name)
    fw = forward(c.x, c.gamma, c.beta, EPS, c.residual, c.leaky)
    return fw, backward(fw, c.gy, c.gamma, c.leaky)


OUTPUTS = ("y", "gx", "ggamma", "gbeta", "gres")                   # the outputs tests/golden/bn_grad.npz holds err32 for
PER_COLUMN = ("y", "gx", "gres")
