"""Block library of the KPFCNN encoder/decoder, mirroring models/network_blocks.py of the reference for the
block types of the shipped architectures.  Every block keeps the reference signature
    block(layer_ind, inputs, features, radius, fdim, config, training)
and runs eagerly on the MI355X; variables live in the VariableStore set by `use_variables(...)` (the role of
the TF variable scopes).  With training=False (the reference derives it from dropout_prob < 0.99, :1071) batch norm uses the
moving statistics and is fused, together with LeakyReLU(0.2) and the residual add, into the epilogue of the producing contraction.
With training=True the `unary`, `simple` and `resnetb` blocks run as the unfused composition of the trainable operators
(kernels/autograd.py): batch statistics, the moving statistics updated in place, gradients to every variable of the block
(VariableStore.parameter).  Inside a network walk (training_walk(), entered by assemble_CNN_blocks / assemble_FCNN_blocks) the strided
block and the decoder's unary over a pending nearest-upsample concatenation are trainable too (the backward of the max pooling and of
the nearest upsampling: ops.ind_max_pool_backward, ops.closest_pool_cat_backward); called directly they keep raising
NotImplementedError, as the deformable blocks and bf16 feature storage do everywhere.
"""
import contextlib

import numpy as np
import torch

from .. import ops
from ..kernels import convolution_ops as conv_ops
from ..kernels.autograd import (batch_norm_trainable, closest_pool_cat_trainable, ind_max_pool_trainable, kpconv_trainable,
                                unary_trainable)
from ..kernels.kernel_points import create_kernel_points

_STORE = None


@contextlib.contextmanager
def use_variables(store):
    global _STORE
    prev, _STORE = _STORE, store
    try:
        yield store
    finally:
        _STORE = prev


def _vs():
    if _STORE is None:
        raise RuntimeError('no VariableStore active: wrap the call in network_blocks.use_variables(store)')
    return _STORE


def variable_scope(name):
    return _vs().variable_scope(name)


# ---- utilities (models/network_blocks.py:37-83, :149-186) ----------------------------------------------------------

def weight_variable(shape):
    """:37-41 -> device tensor of the (created or loaded) `weights` variable of the current scope."""
    vs = _vs()
    return vs.tensor(vs.weight_variable(shape))


def ind_max_pool(x, inds):
    """:51-66."""
    return ops.ind_max_pool(x, inds)


def closest_pool(x, inds):
    """:69-83."""
    return ops.closest_pool_cat(x, inds)


def _bn(channels, use_batch_norm=True):
    """(col_scale, col_shift) of the current scope's inference batch norm (:149-165); without batch norm the
    reference adds a learnt `offset` vector (:162-165)."""
    vs = _vs()
    if use_batch_norm:
        return vs.folded_bn(vs.batch_norm_variables(channels))
    return None, vs.tensor(vs.offset_variable(channels))


def _bn_train(x, use_batch_norm, momentum, leaky=False, residual=None):
    """:149-165 with training=True on the variables of the current scope, then the residual add and LeakyReLU(0.2) of the block in
    the same pass: batch statistics, the scope's moving statistics updated in place."""
    vs = _vs()
    channels = int(x.shape[1])
    if not use_batch_norm:
        return batch_norm_trainable(x, None, vs.parameter(vs.offset_variable(channels)), residual, leaky, 0.2)
    gamma, beta, mean, var = vs.batch_norm_variables(channels)
    return batch_norm_trainable(x, vs.parameter(gamma), vs.parameter(beta), residual, leaky, 0.2, vs.tensor(mean), vs.tensor(var),
                                momentum, 1e-6)


def batch_norm(x, use_batch_norm=True, momentum=0.99, training=False):
    """:149-165, as a stand-alone op."""
    if training:
        _check_trainable(x, 'batch_norm')
        return _bn_train(x, use_batch_norm, momentum)
    scale, shift = _bn(int(x.shape[1]), use_batch_norm)
    return ops.affine_act(x, scale, shift)


def leaky_relu(features, alpha=0.2):
    """:185-186."""
    return ops.affine_act(features, leaky=True, alpha=alpha)


def _epilogue(channels, config, leaky, residual=None):
    scale, shift = _bn(channels, config.use_batch_norm)
    return dict(col_scale=scale, col_shift=shift, residual=residual, leaky=leaky, alpha=0.2)


def _kernel_points(config, extent):
    """`kernel_points` variable of the current scope (kernels/convolution_ops.py:128-148): created with radius
    1.5*extent when absent."""
    vs = _vs()
    k = config.num_kernel_points

    def init():
        pts = create_kernel_points(1.5 * extent, k, num_kernels=1, dimension=3, fixed=config.fixed_kernel_points,
                                   rng=vs.rng)
        return pts.reshape((k, 3))
    name = vs.get('kernel_points', (k, 3), init)
    return vs.values[name]


def KPConv(query_points, support_points, neighbors_indices, features, K_values, radius, config, epilogue=None):
    """:86-103: extent = KP_extent * radius / density_parameter, then kernels.convolution_ops.KPConv.  epilogue: the dict, or a
    callable that makes it -- called after `kernel_points` exists, the reference's creation order (weights, kernel_points, then what
    batch_norm creates)."""
    extent = config.KP_extent * radius / config.density_parameter
    K_points = _kernel_points(config, extent)
    return conv_ops.KPConv(query_points, support_points, neighbors_indices, features, K_values,
                           fixed=config.fixed_kernel_points, KP_extent=extent, KP_influence=config.KP_influence,
                           aggregation_mode=config.convolution_mode, K_points=K_points,
                           epilogue=epilogue() if callable(epilogue) else epilogue)


def KPConv_deformable(query_points, support_points, neighbors_indices, features, K_values, radius, config, epilogue=None):
    """:106-124: as KPConv, with the `offset_conv_weights` / `offset_conv_bias` variables of the current scope (created after
    `kernel_points`, zeros: kernels/convolution_ops.py:327-328) and config.modulated."""
    extent = config.KP_extent * radius / config.density_parameter
    K_points = _kernel_points(config, extent)
    vs = _vs()
    k, cin = int(K_values.shape[0]), int(K_values.shape[1])
    offset_dim = (4 if config.modulated else 3) * k
    w0 = vs.tensor(vs.get('offset_conv_weights', (k, cin, offset_dim), lambda: np.zeros((k, cin, offset_dim))))
    b0 = vs.tensor(vs.get('offset_conv_bias', (offset_dim,), lambda: np.zeros(offset_dim)))
    epilogue = epilogue() if callable(epilogue) else epilogue
    return conv_ops.KPConv_deformable(query_points, support_points, neighbors_indices, features, K_values,
                                      fixed=config.fixed_kernel_points, KP_extent=extent, KP_influence=config.KP_influence,
                                      aggregation_mode=config.convolution_mode, modulated=config.modulated, K_points=K_points,
                                      offset_weights=w0, offset_bias=b0, epilogue=epilogue)


# Depth of the training-mode network walks in progress (a module global, as _NEXT_RESNETB below).
_TRAINING_WALK = 0


@contextlib.contextmanager
def training_walk():
    """A training-mode walk over the architecture is in progress.  Inside it resnetb_strided_block(training=True) and unary_block
    (training=True) over an ops.UpsampleCat run their trainable forms; outside it both keep raising NotImplementedError with the
    messages tests/test_gpu_training_blocks.py pins for direct calls.  Re-entrant.  A later change may drop this gate together with
    the two pinned refusals: nothing else depends on it."""
    global _TRAINING_WALK
    _TRAINING_WALK += 1
    try:
        yield
    finally:
        _TRAINING_WALK -= 1


def _check_inference(training, what, in_walk=False):
    """in_walk: the block has a trainable form that a network walk may use."""
    if training and not (in_walk and _TRAINING_WALK > 0):
        raise NotImplementedError('training=True: %s' % what)


def _check_trainable(features, block):
    """The inputs the training path does not take yet."""
    if isinstance(features, ops.UpsampleCat):
        if _TRAINING_WALK == 0:
            raise NotImplementedError('training=True: %s on a pending nearest-upsample concatenation needs the backward of the nearest '
                                      'upsampling, which is not built' % block)
        rows = (features.x,) + ((features.skip,) if features.skip is not None else ())
    else:
        rows = (features,)
    if ops.BF16_FEATURES or any(t.dtype != torch.float32 for t in rows):
        raise NotImplementedError('training=True: %s under bf16 feature storage: the trainable operators take float32 rows only' % block)


# ---- blocks --------------------------------------------------------------------------------------------------------

def last_unary_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:194-205: 1x1 convolution to 32 channels, no batch norm / activation."""
    if training:
        _check_trainable(features, 'last_unary_block')
        vs = _vs()
        return unary_trainable(_upsampled_train(features), vs.parameter(vs.weight_variable([int(features.shape[1]), 32])))
    w = weight_variable([int(features.shape[1]), 32])
    if isinstance(features, ops.PendingUnary):
        # the decoder block before this one was not launched: both contractions in one launch, its 64-column tensor never written
        return features.chain(w)
    if isinstance(features, ops.UpsampleCat):
        features = features.materialize()
    with ops.f32_output():      # descriptors and scores are computed from fp32 values whatever the feature storage
        return conv_ops.unary_convolution(features, w)


def unary_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:207-219."""
    if training:
        _check_trainable(features, 'unary_block')
        vs = _vs()
        w = vs.parameter(vs.weight_variable([int(features.shape[1]), fdim]))
        # (decoder: unfused -- the concatenation is written, no split weights, no PendingUnary)
        return _bn_train(unary_trainable(_upsampled_train(features), w), config.use_batch_norm, config.batch_norm_momentum, leaky=True)
    if isinstance(features, ops.PendingUnary):
        features = features.materialize()
    if isinstance(features, ops.UpsampleCat):
        # decoder: nearest upsampling + skip concatenation (models/D3Feat.py:55-63) fused into this contraction
        vs = _vs()
        w = vs.weight_variable([int(features.shape[1]), fdim])
        if ops.pending_unary_ok(features, fdim):
            # level 0 (resident form): stays pending -- `last_unary` chains its contraction onto this one (ops.gemm_chain); any
            # other consumer materialises it, which is the launch below
            e = _epilogue(fdim, config, True)
            return ops.PendingUnary(features, vs.tensor(w), e['col_scale'], e['col_shift'], True, 0.2)
        if ops.upsample_split_ok(features, fdim):
            # ... with the upsampled half contracted once per COARSE row and gathered in the fine level's epilogue
            if config.use_batch_norm:
                w1, w2, shift = vs.split_decoder(w, vs.batch_norm_variables(fdim), int(features.x.shape[1]))
            else:
                (w1, w2, _), shift = vs.split_decoder(w, None, int(features.x.shape[1])), _bn(fdim, False)[1]
            return ops.gemm_upsample_split(features, w1, w2, col_shift=shift, leaky=True, alpha=0.2)
        e = _epilogue(fdim, config, True)
        return ops.gemm_upsample_cat(features, vs.tensor(w), col_scale=e['col_scale'], col_shift=e['col_shift'], leaky=True, alpha=0.2)
    w = weight_variable([int(features.shape[1]), fdim])
    return conv_ops.unary_convolution(features, w, epilogue=_epilogue(fdim, config, True))


def simple_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:222-244."""
    if training:
        _check_trainable(features, 'simple_block')
        vs = _vs()
        w = vs.parameter(vs.weight_variable([config.num_kernel_points, int(features.shape[1]), fdim]))
        pts = inputs['points'][layer_ind]
        x = _kpconv_train(pts, pts, inputs['neighbors'][layer_ind], features, w, radius, config)
        return _bn_train(x, config.use_batch_norm, config.batch_norm_momentum, leaky=True)
    w = weight_variable([config.num_kernel_points, int(features.shape[1]), fdim])
    return KPConv(inputs['points'][layer_ind], inputs['points'][layer_ind], inputs['neighbors'][layer_ind], features, w,
                  radius, config, epilogue=lambda: _epilogue(fdim, config, True))


def _upsampled_train(features):
    """A pending nearest-upsample concatenation as a tensor that carries gradients to the coarse rows and to the skip."""
    if isinstance(features, ops.UpsampleCat):
        return closest_pool_cat_trainable(features.x, features.inds, features.skip)
    return features


def _kpconv_train(query_points, support_points, neighbors_indices, features, K_values, radius, config):
    """KPConv (:86-103) without epilogue, trainable: the `kernel_points` of the current scope are created after the weights."""
    extent = config.KP_extent * radius / config.density_parameter
    K_points = _kernel_points(config, extent)
    return kpconv_trainable(query_points, support_points, neighbors_indices, features, K_points, K_values, extent, config.KP_influence,
                            config.convolution_mode)


def _resnetb_train(layer_ind, inputs, features, radius, fdim, config, strided=False):
    """:321-368 (strided: :561-612) with training=True, unfused: conv1 unary -> BN -> leaky; conv2 KPConv -> BN -> leaky (strided: from
    points[l] to points[l + 1] through pools[l]); shortcut (strided: the max pooling of the input through pools[l]) unary -> BN iff the
    width changes; conv3 unary -> BN + shortcut -> leaky.  Variables are created in the reference's order (conv3 before shortcut)."""
    _check_trainable(features, 'resnetb_strided_block' if strided else 'resnetb_block')
    vs = _vs()
    bn, momentum = config.use_batch_norm, config.batch_norm_momentum
    cin = int(features.shape[1])
    with variable_scope('conv1'):
        w = vs.parameter(vs.weight_variable([cin, fdim // 2]))
        x = _bn_train(unary_trainable(features, w), bn, momentum, leaky=True)
    with variable_scope('conv2'):
        w = vs.parameter(vs.weight_variable([config.num_kernel_points, fdim // 2, fdim // 2]))
        if strided:
            q, pts, nb = inputs['points'][layer_ind + 1], inputs['points'][layer_ind], inputs['pools'][layer_ind]
        else:
            q = pts = inputs['points'][layer_ind]
            nb = inputs['neighbors'][layer_ind]
        x = _bn_train(_kpconv_train(q, pts, nb, x, w, radius, config), bn, momentum, leaky=True)
    with variable_scope('conv3'):
        w3 = vs.parameter(vs.weight_variable([fdim // 2, 2 * fdim]))
        if bn:
            vs.batch_norm_variables(2 * fdim)
        else:
            vs.offset_variable(2 * fdim)
    shortcut = ind_max_pool_trainable(features, inputs['pools'][layer_ind]) if strided else features
    if cin != 2 * fdim:
        with variable_scope('shortcut'):
            w = vs.parameter(vs.weight_variable([cin, 2 * fdim]))
            shortcut = _bn_train(unary_trainable(shortcut, w), bn, momentum)
    with variable_scope('conv3'):
        return _bn_train(unary_trainable(x, w3), bn, momentum, leaky=True, residual=shortcut)


# While assemble_CNN_blocks runs a block that is followed by a resnetb* block at the SAME level: (depth of the variable scopes
# around the blocks, scope name of the following block).  _resnetb then chains that block's conv1 onto its own last contraction.
_NEXT_RESNETB = None
_CHAINED = '_d3f_chained_conv1'


def _chain_next_conv1(x, shortcut, W, shift, fdim, config):
    """conv3 + shortcut of a resnetb block AND the conv1 of the resnetb* block that follows, in one launch (ops.gemm_chain): the
    128-column tensor is stored as ever, the following block does not read it back for its conv1.  The following block's
    `conv1/weights` and batch-norm variables are created here -- the very next variables the reference creates -- and the result is
    attached to the returned tensor under that weight's name and epilogue.  -> the block's output, or None (launch as ever)."""
    if _NEXT_RESNETB is None or fdim // 2 != 32 or not isinstance(x, torch.Tensor) or not isinstance(shortcut, torch.Tensor):
        return None
    M, K = int(x.shape[0]), int(x.shape[1]) + int(shortcut.shape[1])
    ok = all(t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
             and t.shape[1] % 32 == 0 for t in (x, shortcut))
    if not ok or not ops.gemm_chain_ok(M, 2 * fdim, K, True, int(getattr(x, 'n_hint', 0) or 0)):
        return None
    vs = _vs()
    depth, scope = _NEXT_RESNETB
    saved = vs._scope
    vs._scope = saved[:depth] + [scope, 'conv1']
    try:
        wn = vs.weight_variable([2 * fdim, fdim // 2])
        e = _epilogue(fdim // 2, config, True)
    finally:
        vs._scope = saved
    out, x_next = ops.gemm_chain(x, W, vs.tensor(wn), skip=shortcut, store_first=True, col_shift=shift, leaky=True, alpha=0.2,
                                 col_scale2=e['col_scale'], col_shift2=e['col_shift'], leaky2=True, alpha2=0.2)
    setattr(out, _CHAINED, (wn, e['col_scale'], e['col_shift'], x_next))
    return out


def _resnetb(layer_ind, inputs, features, radius, fdim, config, strided, deformable=False):
    cin = int(features.shape[1])
    with variable_scope('conv1'):
        vs = _vs()
        wn = vs.weight_variable([cin, fdim // 2])
        e = _epilogue(fdim // 2, config, True)
        att = features.__dict__.pop(_CHAINED, None) if isinstance(features, torch.Tensor) else None
        if att is not None and ops.GEMM_CHAIN and att[0] == wn and att[1] is e['col_scale'] and att[2] is e['col_shift']:
            x = att[3]          # computed by the block before, chained onto its last contraction (_chain_next_conv1)
        else:
            x = conv_ops.unary_convolution(features, vs.tensor(wn), epilogue=e)
    with variable_scope('conv2'):
        w = weight_variable([config.num_kernel_points, fdim // 2, fdim // 2])
        if strided:
            q, s, nb = inputs['points'][layer_ind + 1], inputs['points'][layer_ind], inputs['pools'][layer_ind]
        else:
            q, s, nb = inputs['points'][layer_ind], inputs['points'][layer_ind], inputs['neighbors'][layer_ind]
        x = (KPConv_deformable if deformable else KPConv)(q, s, nb, x, w, radius, config,
                                                          epilogue=lambda: _epilogue(fdim // 2, config, True))
    # variables are created in the reference's order (conv3 before shortcut, :342-356 / :585-600) so that lazily created
    # random weights equal build_variables(seed)'s; the compute order below is free
    with variable_scope('conv3'):
        vs = _vs()
        w3 = vs.weight_variable([fdim // 2, 2 * fdim])
        bn3 = None
        if config.use_batch_norm:
            bn3 = vs.batch_norm_variables(2 * fdim)
        else:
            vs.offset_variable(2 * fdim)      # conv3's `offset` (:162-165) before the shortcut's variables, as in the reference
    with variable_scope('shortcut'):
        shortcut = ind_max_pool(features, inputs['pools'][layer_ind]) if strided else features
        need_sc = int(shortcut.shape[1]) != 2 * fdim
        # leaky_relu(bn(conv3(x)) + bn(shortcut(f))): both unary branches as ONE contraction over [x | f], the batch-norm
        # scales folded into the stacked weights -- no shortcut tensor, no residual re-read, one launch less
        fuse = need_sc and config.use_batch_norm and (fdim // 2) % 4 == 0
        sc_w = sc_bn = None
        if need_sc:
            vs = _vs()
            sc_w = vs.weight_variable([int(shortcut.shape[1]), 2 * fdim])
            if fuse:
                sc_bn = vs.batch_norm_variables(2 * fdim)
            else:
                shortcut = conv_ops.unary_convolution(shortcut, vs.tensor(sc_w), epilogue=_epilogue(2 * fdim, config, False))
    with variable_scope('conv3'):
        vs = _vs()
        if fuse:
            W, shift = vs.stacked_branches(w3, bn3, sc_w, sc_bn)
            out = None if (strided or ops.BF16_CONTRACTION) else _chain_next_conv1(x, shortcut, W, shift, fdim, config)
            return out if out is not None else ops.gemm_cat2(x, shortcut, W, col_shift=shift, leaky=True, alpha=0.2)
        # leaky_relu(batch_norm(conv3) + shortcut): the add and the activation ride in the contraction's epilogue
        return conv_ops.unary_convolution(x, vs.tensor(w3), epilogue=_epilogue(2 * fdim, config, True, residual=shortcut))


def resnetb_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:321-368: unary -> KPConv -> unary, shortcut (unary + BN iff the width changes), LeakyReLU(sum)."""
    if training:
        return _resnetb_train(layer_ind, inputs, features, radius, fdim, config)
    return _resnetb(layer_ind, inputs, features, radius, fdim, config, False)


def resnetb_strided_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:561-612: as resnetb but the KPConv queries the next layer's points through `pools`, and the shortcut is
    the max pooling of the input features (+ unary + BN iff the width changes)."""
    _check_inference(training, 'resnetb_strided_block needs the backward of the max pooling of its shortcut, which is not built',
                     in_walk=True)
    if training:
        return _resnetb_train(layer_ind, inputs, features, radius, fdim, config, strided=True)
    return _resnetb(layer_ind, inputs, features, radius, fdim, config, True)


def resnetb_deformable_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:424-471: resnetb with a deformable KPConv as conv2."""
    _check_inference(training, 'resnetb_deformable_block needs the backward of the deformable KPConv, which is not built')
    return _resnetb(layer_ind, inputs, features, radius, fdim, config, False, deformable=True)


def resnetb_deformable_strided_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:672-723: resnetb_strided with a deformable KPConv as conv2."""
    _check_inference(training, 'resnetb_deformable_strided_block needs the backward of the deformable KPConv and of the max pooling, '
                     'which are not built')
    return _resnetb(layer_ind, inputs, features, radius, fdim, config, True, deformable=True)


def nearest_upsample_block(layer_ind, inputs, features, radius, fdim, config, training):
    """:971-979."""
    with variable_scope('nearest_upsample'):
        return closest_pool(features, inputs['upsamples'][layer_ind - 1])


def _materialized(block_fn):
    """Blocks other than `unary` / `last_unary` take a real tensor: materialise a pending nearest-upsample concatenation (or a pending
    unary block over one) first."""
    def wrapped(layer_ind, inputs, features, radius, fdim, config, training):
        if isinstance(features, ops.UpsampleCat):
            features = features.materialize()
        return block_fn(layer_ind, inputs, features, radius, fdim, config, training)
    wrapped.__name__ = block_fn.__name__
    wrapped.__doc__ = block_fn.__doc__
    return wrapped


def get_block_ops(block_name):
    """:982-1042 for the block types of the shipped architectures (results/*/parameters.txt:19) and the deformable resnet
    bottlenecks of the KPConv backbone."""
    table = {'unary': unary_block, 'last_unary': last_unary_block, 'simple': simple_block, 'resnetb': resnetb_block,
             'resnetb_strided': resnetb_strided_block, 'resnetb_deformable': resnetb_deformable_block,
             'resnetb_deformable_strided': resnetb_deformable_strided_block, 'nearest_upsample': nearest_upsample_block}
    if block_name in table:
        return table[block_name] if block_name in ('unary', 'last_unary') else _materialized(table[block_name])
    known_unsupported = ('simple_strided', 'resnet', 'resnetb_light', 'inception_deformable',
                         'resnetb_light_strided', 'inception_deformable_strided', 'vgg',
                         'max_pool', 'max_pool_wide', 'global_average', 'simple_upsample', 'resnetb_upsample')
    if block_name in known_unsupported:
        raise NotImplementedError('block "%s" is not used by any released D3Feat model and is not implemented'
                                  % block_name)
    raise ValueError('Unknown block name in the architecture definition : ' + block_name)


def assemble_CNN_blocks(inputs, config, dropout_prob):
    """:1052-1118: encoder.  Returns the skip list F (features before every strided block, and the last ones)."""
    r = config.first_subsampling_dl * config.density_parameter
    layer = 0
    fdim = config.first_features_dim
    features = inputs['features']
    F = []
    training = dropout_prob < 0.99
    block_in_layer = 0
    global _NEXT_RESNETB
    with training_walk() if training else contextlib.nullcontext():
        for i, block in enumerate(config.architecture):
            if any(tmp in block for tmp in ('pool', 'strided', 'upsample', 'global')):
                F += [features]
            if 'upsample' in block:
                break
            # a resnetb* block that follows at the same level: this block may chain that block's conv1 (_chain_next_conv1)
            nxt = config.architecture[i + 1] if i + 1 < len(config.architecture) else ''
            same_level = not ('pool' in block or 'strided' in block)
            if same_level and nxt.startswith('resnetb') and not training:
                _NEXT_RESNETB = (len(_vs()._scope), 'layer_{:d}/{:s}_{:d}'.format(layer, nxt.replace('_deformable', ''), block_in_layer + 1))
            try:
                with variable_scope('layer_{:d}/{:s}_{:d}'.format(layer, block.replace('_deformable', ''), block_in_layer)):
                    features = get_block_ops(block)(layer, inputs, features, r, fdim, config, training)
            finally:
                _NEXT_RESNETB = None
            block_in_layer += 1
            if 'pool' in block or 'strided' in block:
                layer += 1
                r *= 2
                fdim *= 2
                block_in_layer = 0
            if 'global' in block:
                F += [features]
        return F
