"""The trainable operators of an encoder block: torch.autograd around the device operators.

    kpconv_trainable(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                     KP_influence='linear', aggregation_mode='sum')

Forward: convolution_ops.KPConv_ops without epilogue (its dispatch unchanged).  Backward: ops.kpconv_backward, which gives the
gradients with respect to `features` and `K_values`; points, indices and kernel points get none (the kernel points are
trainable=False in the reference, the points are inputs).  The transposed neighbour table is built once, at the first backward that
needs the feature gradient, and kept on the context.

    batch_norm_trainable(x, gamma, beta, residual=None, leaky=False, alpha=0.2, moving_mean=None, moving_variance=None,
                         momentum=0.99, eps=1e-6)

Forward: ops.batch_norm_train (batch statistics, the moving statistics updated in place, the residual add and LeakyReLU in the same
pass).  Backward: ops.batch_norm_backward -> gradients to x, gamma, beta and residual.  gamma=None is the form without batch norm.

    unary_trainable(x, W)

Forward: ops.gemm.  Backward: ops.unary_backward (gx = gy W^T on the contraction router, gW = x^T gy by ops.gemm_tn).
"""
import torch

from .. import ops
from .convolution_ops import KPConv_ops


def _plain(t):
    """The tensor without its autograd history, with its device-resident row count (ops._tag)."""
    return ops._tag(t.detach(), t)


class _KPConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, K_values, query_points, support_points, neighbors_indices, K_points, KP_extent, KP_influence,
                aggregation_mode):
        ctx.geometry = (query_points, support_points, neighbors_indices, K_points, KP_extent, KP_influence, aggregation_mode)
        ctx.table = None
        f, W = _plain(features), K_values.detach()
        ctx.save_for_backward(f, W)
        return KPConv_ops(query_points, support_points, neighbors_indices, f, K_points, W, KP_extent, KP_influence, aggregation_mode)

    @staticmethod
    def backward(ctx, grad_output):
        q, s, idx, kp, extent, influence, aggregation = ctx.geometry
        f, W = ctx.saved_tensors
        f = ops._tag(f, s)
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 7
        if not (need_f or need_w):
            return (None, None) + none
        rows, cols = grad_output.shape
        if (cols > 1 and grad_output.stride(1) != 1) or (rows > 1 and grad_output.stride(0) < cols):
            grad_output = grad_output.contiguous()               # (an expanded or transposed gradient: rows must be rows)
        if need_f and ctx.table is None:
            ctx.table = ops.neighbor_transpose_supports(idx, s.shape[0], getattr(q, "n_dev", None),
                                                        getattr(s, "n_dev", None) if getattr(s, "n_dev", None) is not None
                                                        else getattr(f, "n_dev", None))
        gf, gW = ops.kpconv_backward(q, s, idx, f, kp, W, grad_output, extent, influence, aggregation, transpose=ctx.table,
                                     need_features=need_f, need_weights=need_w)
        return (gf, gW) + none


def kpconv_trainable(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent, KP_influence='linear',
                     aggregation_mode='sum'):
    """KPConv_ops (no epilogue) whose result carries gradients to `features` and `K_values`."""
    return _KPConv.apply(features, K_values, query_points, support_points, neighbors_indices, K_points, KP_extent, KP_influence,
                         aggregation_mode)


class _Count:
    """The row-count tag of a tensor, kept on the context: saved tensors come back without their attributes."""

    def __init__(self, *tensors):
        for t in tensors:
            if t is not None and getattr(t, "n_dev", None) is not None:
                self.n_dev, self.n_hint = t.n_dev, getattr(t, "n_hint", 0)
                return


def _as_rows(g):
    """A gradient whose rows are rows (an expanded or transposed one is copied)."""
    rows, cols = g.shape
    if (cols > 1 and g.stride(1) != 1) or (rows > 1 and g.stride(0) < cols):
        g = g.contiguous()
    return g


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, leaky, alpha, moving_mean, moving_variance, momentum, eps):
        xp = _plain(x)
        y, mean, rstd = ops.batch_norm_train(xp, None if gamma is None else gamma.detach(), beta.detach(), eps,
                                             None if residual is None else _plain(residual), leaky, alpha, moving_mean, moving_variance,
                                             momentum)
        ctx.flags = (bool(leaky), float(alpha), gamma is not None)
        ctx.count = _Count(x, residual)
        ctx.save_for_backward(*((xp, y, gamma.detach(), mean, rstd) if gamma is not None else (y,)))
        return y

    @staticmethod
    def backward(ctx, grad_y):
        leaky, alpha, has_gamma = ctx.flags
        if has_gamma:
            x, y, gamma, mean, rstd = ctx.saved_tensors
        else:
            (y,), x, gamma, mean, rstd = ctx.saved_tensors, None, None, None, None
        g = ops._tag(_as_rows(grad_y).detach(), ctx.count)
        gx, ggamma, gbeta, gres = ops.batch_norm_backward(x, y, g, gamma, mean, rstd, leaky, alpha, need_residual=ctx.needs_input_grad[3])
        need = ctx.needs_input_grad
        return (gx if need[0] else None, ggamma if need[1] else None, gbeta if need[2] else None, gres) + (None,) * 6


def batch_norm_trainable(x, gamma, beta, residual=None, leaky=False, alpha=0.2, moving_mean=None, moving_variance=None, momentum=0.99,
                         eps=1e-6):
    """ops.batch_norm_train whose result carries gradients to x, gamma, beta and residual (gamma=None: the offset-only form)."""
    return _BatchNorm.apply(x, gamma, beta, residual, leaky, alpha, moving_mean, moving_variance, momentum, eps)


class _Unary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W):
        xp, Wp = _plain(x), W.detach()
        ctx.save_for_backward(xp, Wp)
        ctx.count = _Count(x)
        with ops.f32_output():
            return ops.gemm(xp, Wp)

    @staticmethod
    def backward(ctx, grad_y):
        x, W = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad
        if not (need_x or need_w):
            return None, None
        return ops.unary_backward(ops._tag(x, ctx.count), W, ops._tag(_as_rows(grad_y).detach(), ctx.count), need_input=need_x,
                                  need_weights=need_w)


def unary_trainable(x, W):
    """ops.gemm(x, W) whose result carries gradients to x and W."""
    return _Unary.apply(x, W)
