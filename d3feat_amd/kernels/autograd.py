"""A trainable rigid KPConv: torch.autograd around the two device operators.

    kpconv_trainable(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                     KP_influence='linear', aggregation_mode='sum')

Forward: convolution_ops.KPConv_ops without epilogue (its dispatch unchanged).  Backward: ops.kpconv_backward, which gives the
gradients with respect to `features` and `K_values`; points, indices and kernel points get none (the kernel points are
trainable=False in the reference, the points are inputs).  The transposed neighbour table is built once, at the first backward that
needs the feature gradient, and kept on the context.  Batch norm in training mode, LeakyReLU and the shortcut add are torch
one-liners around this call.
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
