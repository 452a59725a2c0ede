"""TEST INFRASTRUCTURE ONLY: no tests in here.

The reference's inference graph in plain float64 numpy, for the rigid block types (simple, resnetb, resnetb_strided, unary, last_unary,
nearest_upsample) and EVERY field of the configuration that the graph reads: KP_influence, convolution_mode, use_batch_norm (the learnt
`offset` that replaces batch norm), first_features_dim, num_kernel_points, in_features_dim, KP_extent, density_parameter and the
architecture (any number of layers).  It is the definition tests/test_gpu_network_configs.py holds the HIP path to; the KPConv operator
and the detection head are oracle.network_np.kpconv_f64 / detection_head_f64.  Every function cites the lines of the reference it
evaluates (models/network_blocks.py unless another file is named).

    forward(config, W, inputs) -> (descriptors f64[n, 32], scores f64[n, 1], trace, report)

W: {variable name without the KernelPointNetwork/ root: array}; inputs: the dict of oracle.network_np.descriptor_input.
trace: {variable scope: block output f64}, in evaluation order (a nearest_upsample block: the gathered rows, before the concatenation).
report: one dict per KPConv, in evaluation order --
    scope      variable scope of the operator (.../conv2 inside a resnet block)
    margin     min over the rows of its input features of |sum_c f| / sum_c |f|   (rows of zeros do not take part; 1.0 without any)
    share      the share of rows whose sum is <= 0: the neighbours kernels/convolution_ops.py:250-251 does not count
    positive   bool [rows]: sum_c f > 0, from the exact sum
"""
import math

import numpy as np

from oracle.network_np import detection_head_f64, kpconv_f64


def _f64(a):
    return np.asarray(a, np.float64)


def leaky_relu(x, alpha=0.2):
    """:185-186."""
    return np.where(x > 0, x, x * alpha)


def batch_norm(x, W, scope, use_batch_norm=True, eps=1e-6):
    """:149-165 at inference: the moving statistics with epsilon 1e-6 (:156-160), or the `offset` vector alone (:162-165)."""
    if not use_batch_norm:
        return x + _f64(W[scope + "/offset"])
    g, b, m, v = (_f64(W[scope + "/batch_normalization/" + n]) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
    return (x - m) / np.sqrt(v + eps) * g + b


def ind_max_pool(x, inds):
    """:51-66: the shadow row holds every column's minimum."""
    x = np.concatenate([x, x.min(0, keepdims=True)], 0)
    inds = np.asarray(inds, np.int64)
    return x[np.where((inds < 0) | (inds >= len(x) - 1), len(x) - 1, inds)].max(1)


def closest_pool(x, inds):
    """:69-83: the first column of the index matrix, the shadow row zeros."""
    x = np.concatenate([x, np.zeros((1, x.shape[1]))], 0)
    i0 = np.asarray(inds, np.int64)[:, 0]
    return x[np.where((i0 < 0) | (i0 >= len(x) - 1), len(x) - 1, i0)]


def row_sum_report(scope, features):
    f = _f64(features)
    s = np.asarray([math.fsum(r) for r in f])
    a = np.abs(f).sum(1)
    live = a > 0
    return dict(scope=scope, margin=float((np.abs(s[live]) / a[live]).min()) if live.any() else 1.0,
                share=float((s <= 0).mean()), positive=s > 0)


def _kpconv(q, s, idx, features, W, scope, radius, config, report):
    """:86-103 (extent = KP_extent * radius / density_parameter) over kernels/convolution_ops.py:161-255."""
    extent = config.KP_extent * radius / config.density_parameter
    report.append(row_sum_report(scope, features))
    return kpconv_f64(q, s, idx, features, W[scope + "/kernel_points"], W[scope + "/weights"], extent, config.KP_influence,
                      config.convolution_mode)[2]


def simple_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:222-244."""
    p = inputs["points"][layer]
    x = _kpconv(p, p, inputs["neighbors"][layer], features, W, scope, radius, config, report)
    return leaky_relu(batch_norm(x, W, scope, config.use_batch_norm))


def _resnetb(layer, inputs, features, radius, fdim, config, W, scope, report, strided):
    bn = config.use_batch_norm
    x = leaky_relu(batch_norm(features @ _f64(W[scope + "/conv1/weights"]), W, scope + "/conv1", bn))            # :326-332
    if strided:                                                                                                  # :574-582
        q, s, idx = inputs["points"][layer + 1], inputs["points"][layer], inputs["pools"][layer]
    else:                                                                                                        # :334-342
        q, s, idx = inputs["points"][layer], inputs["points"][layer], inputs["neighbors"][layer]
    x = _kpconv(q, s, idx, x, W, scope + "/conv2", radius, config, report)
    x = leaky_relu(batch_norm(x, W, scope + "/conv2", bn))                                                       # :344-347 / :584-587
    x = batch_norm(x @ _f64(W[scope + "/conv3/weights"]), W, scope + "/conv3", bn)                               # :349-355 / :589-595
    shortcut = ind_max_pool(features, inputs["pools"][layer]) if strided else features                           # :600
    if shortcut.shape[1] != 2 * fdim:                                                                            # :357-366 / :604-610
        shortcut = batch_norm(shortcut @ _f64(W[scope + "/shortcut/weights"]), W, scope + "/shortcut", bn)
    return leaky_relu(x + shortcut)                                                                              # :368 / :612


def resnetb_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:321-368."""
    return _resnetb(layer, inputs, features, radius, fdim, config, W, scope, report, False)


def resnetb_strided_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:561-612."""
    return _resnetb(layer, inputs, features, radius, fdim, config, W, scope, report, True)


def unary_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:207-219."""
    return leaky_relu(batch_norm(features @ _f64(W[scope + "/weights"]), W, scope, config.use_batch_norm))


def last_unary_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:194-205: neither batch norm nor offset nor activation."""
    return features @ _f64(W[scope + "/weights"])


def nearest_upsample_block(layer, inputs, features, radius, fdim, config, W, scope, report):
    """:971-979."""
    return closest_pool(features, inputs["upsamples"][layer - 1])


_BLOCKS = {"simple": simple_block, "resnetb": resnetb_block, "resnetb_strided": resnetb_strided_block, "unary": unary_block,
           "last_unary": last_unary_block, "nearest_upsample": nearest_upsample_block}


def forward(config, W, inputs):
    arch = list(config.architecture)
    for b in arch:
        if b not in _BLOCKS:
            raise ValueError("block type outside this definition: " + b)
    trace, report = {}, []
    # ---- encoder: :1052-1118
    r = config.first_subsampling_dl * config.density_parameter
    layer, fdim, bil = 0, config.first_features_dim, 0
    features = _f64(inputs["features"])
    F = []
    start_i = len(arch)
    for i, block in enumerate(arch):
        if "strided" in block or "upsample" in block:
            F.append(features)
        if "upsample" in block:
            start_i = i
            break
        scope = "layer_%d/%s_%d" % (layer, block, bil)
        features = _BLOCKS[block](layer, inputs, features, r, fdim, config, W, scope, report)
        trace[scope] = features
        bil += 1
        if "strided" in block:
            layer, r, fdim, bil = layer + 1, r * 2, fdim * 2, 0
    # ---- decoder: models/D3Feat.py:5-63
    features = F[-1]
    layer = config.num_layers - 1
    r = config.first_subsampling_dl * config.density_parameter * 2 ** layer
    fdim = config.first_features_dim * 2 ** layer
    bil = 0
    for block in arch[start_i:]:
        scope = "uplayer_%d/%s_%d" % (layer, block, bil)
        features = _BLOCKS[block](layer, inputs, features, r, fdim, config, W, scope, report)
        trace[scope] = features
        bil += 1
        if "upsample" in block:
            layer, r, fdim, bil = layer - 1, r * 0.5, fdim // 2, 0
            features = np.concatenate([features, F[layer]], 1)                    # D3Feat.py:55-63
    # ---- l2 normalisation and detection scores: models/D3Feat.py:65-115
    desc, score, _ = detection_head_f64(features, inputs["neighbors"][0], inputs["stack_lengths"])
    return desc, score[:, None], trace, report
