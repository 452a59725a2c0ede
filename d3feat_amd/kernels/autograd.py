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

    ind_max_pool_trainable(x, inds)                          closest_pool_cat_trainable(x, inds, skip)

The two gathers at a level boundary.  Forward: ops.ind_max_pool / ops.closest_pool_cat.  Backward: ops.ind_max_pool_backward (from the
stored output) / ops.closest_pool_cat_backward for x and the column view of the gradient for skip.  The transposed table is built at the
first backward and kept on the context.

    detection_head_trainable(features, neighbors, lens_dev, include_zero, stack_group)       -> (descriptors, scores)

Forward: ops.detect_head.  Backward: ops.detect_head_backward; either incoming gradient may be None.

    pair_loss_trainable(features, scores, points, anc_idx, pos_idx, **loss settings)         -> (loss scalar, PairGradients)

ONE validation.loss_gradients call in the forward: the scalar is the sum over the pairs of status 0 of circle + det, the stored
gradients are scaled by the incoming scalar in the backward, and the result object carries the five validation figures of the same call.
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


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inds):
        xp = _plain(x)
        y = ops.ind_max_pool(xp, inds)
        ctx.inds, ctx.table = inds, None
        ctx.counts = (_Count(x), _Count(inds))
        ctx.save_for_backward(xp, y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        if not ctx.needs_input_grad[0]:
            return None, None
        x, y = ctx.saved_tensors
        x, y = ops._tag(x, ctx.counts[0]), ops._tag(y, ctx.counts[1])
        if ctx.table is None:
            ctx.table = ops.neighbor_transpose_supports(ctx.inds, x.shape[0], getattr(y, "n_dev", None), getattr(x, "n_dev", None))
        return ops.ind_max_pool_backward(x, ctx.inds, y, _as_rows(grad_y).detach(), transpose=ctx.table), None


def ind_max_pool_trainable(x, inds):
    """ops.ind_max_pool(x, inds) whose result carries the gradient to x (float32 rows)."""
    return _MaxPool.apply(x, inds)


class _UpsampleCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, inds):
        ctx.inds, ctx.table = inds, None
        ctx.shape = (int(x.shape[0]), int(x.shape[1]))
        ctx.count = _Count(x)
        return ops.closest_pool_cat(_plain(x), inds, None if skip is None else _plain(skip))

    @staticmethod
    def backward(ctx, grad_out):
        need_x, need_skip = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = ops._tag(_as_rows(grad_out).detach(), ctx.inds)
        N1, C1 = ctx.shape
        gx = None
        if need_x:
            gx = ops._tag(torch.empty((N1, C1), dtype=torch.float32, device=g.device), ctx.count)
            if ctx.table is None:
                ctx.table = ops.neighbor_transpose_supports(ops._tag(ctx.inds[:, :1], ctx.inds), N1, None, getattr(gx, "n_dev", None))
            ops.closest_pool_cat_backward(g, ctx.inds, N1, C1, transpose=ctx.table, out=gx)
        return gx, (g[:, C1:] if need_skip else None), None


def closest_pool_cat_trainable(x, inds, skip=None):
    """ops.closest_pool_cat(x, inds, skip) whose result carries gradients to x and skip."""
    return _UpsampleCat.apply(x, skip, inds)


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, neighbors, lens_dev, include_zero, stack_group):
        f = _plain(features)
        ctx.geometry = (neighbors, lens_dev, include_zero, stack_group)
        ctx.table = None
        ctx.count = _Count(features)
        ctx.set_materialize_grads(False)                             # (an unused output hands None, not zeros, to the backward)
        ctx.save_for_backward(f)
        desc, score = ops.detect_head(f, neighbors, lens_dev, include_zero, stack_group=stack_group)
        return desc, score

    @staticmethod
    def backward(ctx, grad_desc, grad_score):
        if not ctx.needs_input_grad[0] or (grad_desc is None and grad_score is None):
            return (None,) * 5
        neighbors, lens_dev, include_zero, stack_group = ctx.geometry
        (f,) = ctx.saved_tensors
        if ctx.table is None:
            ctx.table = ops.neighbor_transpose(neighbors, lens_dev)
        gd = None if grad_desc is None else _as_rows(grad_desc).detach()
        gs = None if grad_score is None else grad_score.detach()
        if gs is not None and gs.dim() == 2 and gs.shape[0] > 1 and gs.stride(0) < 1:
            gs = gs.contiguous()                                     # (an expanded gradient)
        gx = ops.detect_head_backward(ops._tag(f, ctx.count), neighbors, lens_dev, include_zero, gd, gs, stack_group=stack_group,
                                      transpose=ctx.table)
        return (gx,) + (None,) * 4


def detection_head_trainable(features, neighbors, lens_dev, include_zero, stack_group=0):
    """ops.detect_head -> (descriptors, scores) whose gradients (either may be missing) reach `features`."""
    return _Head.apply(features, neighbors, lens_dev, include_zero, stack_group)


class _PairLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, scores, result):
        v = result.values
        ok = (result.status == 0).to(torch.float32)
        ctx.result = result
        return ((v[:, 0 if result.loss == "circle_loss" else 1] + v[:, 2]) * ok).sum()     # (columns: validation.FIGURES)

    @staticmethod
    def backward(ctx, grad_loss):
        r = ctx.result
        gf = r.features * grad_loss if ctx.needs_input_grad[0] else None
        gs = (r.scores * grad_loss).reshape(-1, 1) if ctx.needs_input_grad[1] else None
        return gf, gs, None


def pair_loss_trainable(features, scores, points, anc_idx, pos_idx, **settings):
    """-> (loss, result): validation.loss_gradients(features, scores, points, anc_idx, pos_idx, **settings) once; loss is the autograd
    scalar circle + det summed over the pairs of status 0, result the PairGradients of that call (its figures are the validation's)."""
    from .. import validation
    result = validation.loss_gradients(_plain(features), _plain(scores), points, anc_idx, pos_idx, **settings)
    return _PairLoss.apply(features, scores, result), result
