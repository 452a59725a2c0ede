"""TEST INFRASTRUCTURE ONLY.  Plain float64 numpy evaluation of the reference's deformable KPConv (kernels/convolution_ops.py:258-499)
and of its two resnet bottlenecks (models/network_blocks.py:424-471, :672-723), pinned to what the reference's own Python computes
by tests/test_deformable_host.py (fixture tests/golden/deformable.npz) and used as the reference of the GPU tests.

The reference keeps the neighbours that are in range of a deformed kernel point by compacting them (top_k / batch_gather,
:435-451).  Here they are MASKED: a neighbour that is out of range multiplies its influences by 0.  Same sums, no data-dependent
shape.  The four differences to the rigid operator (oracle/network_np.kpconv_f64):
  1. the shadow point sits at 1000 (:414): never in range, zero feature row -- an index outside [0, Ns) contributes nothing;
  2. in range = d2 < KP_extent^2 for at least one DEFORMED kernel point (:435); out of range contributes nothing whatever the
     influence function (gaussian is not 0 there, 'closest' would pick a point anyway);
  3. linear influence max(1 - sqrt(d2 + 1e-10) / KP_extent, 0) (:461; rigid: 2 KP_extent); constant influence = d2 < KP_extent^2 per
     kernel point (:456; rigid: 1);
  4. no division by a neighbour count (:497-499); modulations multiply wf[n, p, :] before the contraction (:489-490).
"""
from unittest import mock

import numpy as np


def deformed_from_raw(raw, num_kp, KP_extent, modulated):
    """The raw output [n, 3 num_kp (4 num_kp)] of the offset convolution -> (offsets [n, num_kp, 3] in the units of the points,
    modulations [n, num_kp] or None)   (:341-359)."""
    raw = np.asarray(raw, np.float64)
    off = raw[:, :3 * num_kp].reshape(-1, num_kp, 3) * float(KP_extent)
    mod = 2.0 / (1.0 + np.exp(-raw[:, 3 * num_kp:4 * num_kp])) if modulated else None
    return off, mod


def epilogue_f64(out, col_scale=None, col_shift=None, residual=None, leaky=False, alpha=0.2):
    if col_scale is not None:
        out = out * np.asarray(col_scale, np.float64)
    if col_shift is not None:
        out = out + np.asarray(col_shift, np.float64)
    if residual is not None:
        out = out + np.asarray(residual, np.float64)[:len(out)]
    if leaky:
        out = np.where(out > 0, out, out * float(alpha))
    return out


def kpconv_deform_f64(query_points, support_points, neighbors_indices, features, K_points, offsets, modulations, K_values, KP_extent,
                      KP_influence="linear", mode="sum", Nq=None, Ns=None, **epi):
    """KPConv_deform_ops (:379-499), all rows at once.  offsets [>= Nq, num_kp, 3] (units of the points), modulations [>= Nq, num_kp]
    or None.  Nq / Ns: the effective counts.
    -> dict(wf [Nq, P, Cin] (modulated), in_range [Nq, K] bool (valid and in range), d2 [Nq, K, P], valid [Nq, K],
            out [Nq, Cout] with the epilogue `epi` applied, or None without K_values)."""
    Nq = len(query_points) if Nq is None else int(Nq)
    Ns = len(support_points) if Ns is None else int(Ns)
    q = np.asarray(query_points, np.float64)[:Nq]
    s = np.asarray(support_points, np.float64)[:Ns]
    f = np.asarray(features, np.float64)[:Ns]
    KP = np.asarray(K_points, np.float64)
    idx = np.asarray(neighbors_indices, np.int64)[:Nq]
    P, Cin, K = KP.shape[0], f.shape[1], idx.shape[1]
    e = float(KP_extent)
    kpd = KP[None] + np.asarray(offsets, np.float64)[:Nq].reshape(Nq, P, 3)              # :424
    valid = (idx >= 0) & (idx < Ns)
    if Ns == 0 or K == 0:
        d2 = np.zeros((Nq, K, P))
        in_range = np.zeros((Nq, K), bool)
        wf = np.zeros((Nq, P, Cin))
    else:
        safe = np.where(valid, idx, 0)
        rel = s[safe] - q[:, None, :]                                                     # :418-421
        d2 = ((rel[:, :, None, :] - kpd[:, None, :, :]) ** 2).sum(-1)                     # :427-432  [Nq, K, P]
        in_range = valid & (d2 < e * e).any(-1)                                           # :435 (+ the shadow at 1000)
        if KP_influence == "constant":                                                    # :454-457
            h = (d2 < e * e).astype(np.float64)
        elif KP_influence == "linear":                                                    # :459-462
            h = np.maximum(1.0 - np.sqrt(d2 + 1e-10) / e, 0.0)
        elif KP_influence == "gaussian":                                                  # :464-468
            h = np.exp(-d2 / (2.0 * (e * 0.3) ** 2 + 1e-9))
        else:
            raise ValueError("Unknown influence function type (config.KP_influence)")
        if mode == "closest":                                                             # :473-475
            h = h * (np.arange(P)[None, None, :] == d2.argmin(-1)[:, :, None])
        elif mode != "sum":
            raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
        h = h * in_range[:, :, None]                                                      # :441-451 as a mask
        wf = np.matmul(h.transpose(0, 2, 1), f[safe])                                     # :483-486  [Nq, P, Cin]
    if modulations is not None:
        wf = wf * np.asarray(modulations, np.float64)[:Nq, :, None]                       # :489-490
    out = None
    if K_values is not None:
        out = epilogue_f64(wf.reshape(Nq, P * Cin) @ np.asarray(K_values, np.float64).reshape(P * Cin, -1), **epi)   # :493-497
    return dict(wf=wf, in_range=in_range, d2=d2, valid=valid, out=out)


def kpconv_deformable_f64(query_points, support_points, neighbors_indices, features, K_points, K_values, offset_weights, offset_bias,
                          KP_extent, KP_influence="linear", mode="sum", modulated=False, Nq=None, Ns=None, **epi):
    """KPConv_deformable (:258-376): the rigid offset convolution + bias, then KPConv_deform_ops.  -> the dict of kpconv_deform_f64
    plus raw [Nq, 3 P (4 P)]."""
    from oracle import network_np as onp
    P = np.asarray(K_points).shape[0]
    raw = onp.kpconv_f64(query_points, support_points, neighbors_indices, features, K_points, offset_weights, KP_extent, KP_influence,
                         mode, Nq=Nq, Ns=Ns, col_shift=offset_bias)[2]                    # :331-339
    off, mod = deformed_from_raw(raw, P, KP_extent, modulated)
    r = kpconv_deform_f64(query_points, support_points, neighbors_indices, features, K_points, off, mod, K_values, KP_extent,
                          KP_influence, mode, Nq=Nq, Ns=Ns, **epi)
    r["raw"] = raw
    return r


# ---- blocks (models/network_blocks.py) ------------------------------------------------------------------------------------------
def _bn(x, W, scope, eps=1e-6):
    g, b, m, v = (np.asarray(W[scope + "/batch_normalization/" + n], np.float64) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv = g / np.sqrt(v + eps)
    return x * inv + (b - m * inv)


def _leaky(x, alpha=0.2):
    return np.where(x > 0, x, x * alpha)


def _ind_max_pool(x, inds):
    x = np.concatenate([x, x.min(0, keepdims=True)], 0)                                   # :51-66
    return x[np.asarray(inds, np.int64)].max(1)


def resnetb_deformable_f64(layer_ind, inputs, features, radius, fdim, config, W, scope, strided=False, trace=None):
    """:424-471 (strided: :672-723) in float64.  features [n, Cin] -> [n (or the next layer's n), 2 fdim]."""
    w = lambda name: np.asarray(W[scope + "/" + name], np.float64)
    f = np.asarray(features, np.float64)
    x = _leaky(_bn(f @ w("conv1/weights"), W, scope + "/conv1"))
    pts = [np.asarray(p, np.float64) for p in inputs["points"]]
    if strided:
        q, s, nb = pts[layer_ind + 1], pts[layer_ind], np.asarray(inputs["pools"][layer_ind])
    else:
        q, s, nb = pts[layer_ind], pts[layer_ind], np.asarray(inputs["neighbors"][layer_ind])
    extent = config.KP_extent * radius / config.density_parameter                        # :112
    r = kpconv_deformable_f64(q, s, nb, x, w("conv2/kernel_points"), w("conv2/weights"), w("conv2/offset_conv_weights"),
                              w("conv2/offset_conv_bias"), extent, config.KP_influence, config.convolution_mode, bool(config.modulated))
    if trace is not None:
        trace[scope] = r
    x = _leaky(_bn(r["out"], W, scope + "/conv2"))
    x = _bn(x @ w("conv3/weights"), W, scope + "/conv3")
    sc = _ind_max_pool(f, inputs["pools"][layer_ind]) if strided else f
    if sc.shape[1] != 2 * fdim:
        sc = _bn(sc @ w("shortcut/weights"), W, scope + "/shortcut")
    return _leaky(x + sc)


def forward(config, W, inputs, trace=None):
    """oracle.network_np.forward for an architecture with deformable blocks: the rigid blocks are that module's own (float32 torch),
    the deformable ones are evaluated in float64 here and handed back as float32 -> (descriptors, scores)."""
    import torch
    from oracle import network_np as onp
    rigid = onp.get_block_ops

    def get_block_ops(name):
        if name not in ("resnetb_deformable", "resnetb_deformable_strided"):
            return rigid(name)

        def block(layer_ind, inp, features, radius, fdim, cfg, W_, scope):
            pts = dict(inp, points=[np.asarray(p) for p in inp["points"]])
            out = resnetb_deformable_f64(layer_ind, pts, features.numpy(), radius, fdim, cfg, W_, scope, strided="strided" in name,
                                         trace=trace)
            return torch.from_numpy(out.astype(np.float32))
        return block
    with mock.patch.object(onp, "get_block_ops", get_block_ops):
        return onp.forward(config, W, inputs)


# ---- what float32 arithmetic may differ from the above by -----------------------------------------------------------------------
# u = 2^-24.  Influence of one (neighbour, kernel point), h, evaluated in float32 (e = KP_extent, m = the query's largest |offset|,
# D = d / e < 1 where h > 0):
#   * deformed point kp' = kp + off: the product off = raw * e and the add round once each, |delta kp'_i| <= u (|off_i| + |kp'_i|);
#     r = s - q and d_i = r_i - kp'_i round once each: |delta d| <= u (|r| + |d| + |off| + |kp'|), and with |d| < e,
#     |kp'| <= 1.5 e + m, |r| <= |d| + |kp'|:  <= u (5 e + 3 m), i.e. (5 + 3 m / e) u in D;
#   * d2 (<= 6 roundings of positive terms): 3 u in D; the square root (<= 1 ulp): 2 u; 1 / e rounded once, or the division: u; the
#     product and the subtraction from 1 (or one fma): 2 u.   'linear':  |delta h| <= (13 + 3 m / e) u = (6.5 + 1.5 m / e) 2^-23;
#   * 'gaussian', h = exp(-x), x = d2 / g, g = 0.18 e^2: |delta d2| <= 2 |d| |delta d| <= 2 u (2 |d|^2 + (3 e + 3 m) |d|), times
#     exp(-x) / g: 4 u max(x exp(-x)) + 2 u (3 + 3 m / e) / sqrt(0.18) max(sqrt(x) exp(-x)) = (1.47 + 6.07 + 6.07 m / e) u; the roundings
#     of d2, g, the division and expf as in the rigid operator's bound (tests/test_gpu_kpconv_branches.py: 13 u of which 4.5 u are
#     the inputs'): 8.5 u.   |delta h| <= (16.1 + 6.1 m / e) u = (8.05 + 3.05 m / e) 2^-23;
#   * 'constant': h is 0 or 1, decided by the inputs' margins: no error.
def c_h(influence, m_over_e):
    """|delta h| <= c_h * 2^-23 (above)."""
    m_over_e = np.asarray(m_over_e, np.float64)
    return {"constant": 0.0 * m_over_e, "linear": 6.5 + 1.5 * m_over_e, "gaussian": 8.05 + 3.05 * m_over_e}[influence]


def wf_bound(case_q, case_s, idx, f, KP, offsets, modulations, extent, influence, mode, Nq, Ns, logits=False):
    """|wf32 - wf64| <= 2^-23 mod (c_h sum_{k in range} |f_k| + n / 2 sum_k h_k |f_k|)  [+ 3 * 2^-23 mod sum_k h_k |f_k| when modulated]:
    the influences' error, n FMAs of accumulation over the n neighbours in range (a dropped neighbour adds an exact 0), and where a
    modulation multiplies: its own rounding (2^-24) and, when the kernel computes it as 2 / (1 + expf(-x)) (logits), the relative
    error of expf (1 ulp), the add and the division, <= 5 * 2^-24.  -> [Nq, P, Cin]."""
    r = kpconv_deform_f64(case_q, case_s, idx, np.abs(f), KP, offsets, None, None, extent, influence, mode, Nq=Nq, Ns=Ns)
    af = np.abs(np.asarray(f, np.float64))[:Ns]
    safe = np.where(r["valid"], np.asarray(idx, np.int64)[:Nq], 0)
    s_f = (af[safe] * r["in_range"][:, :, None]).sum(1)[:, None, :] if r["valid"].size else np.zeros_like(r["wf"][:, :1])
    m = np.linalg.norm(np.asarray(offsets, np.float64)[:Nq].reshape(Nq, -1, 3), axis=-1).max(-1) / float(extent)
    b = 2.0 ** -23 * (c_h(influence, m)[:, None, None] * s_f + 0.5 * r["in_range"].sum(1)[:, None, None] * r["wf"])
    if modulations is not None:
        mod = np.asarray(modulations, np.float64)[:Nq, :, None]
        b = mod * b + (3.0 if logits else 0.5) * 2.0 ** -23 * mod * r["wf"]
    return b


def out_bound(q, s, idx, f, KP, offsets, modulations, K_values, extent, influence, mode):
    """|out32 - out64| of KPConv_deform_ops evaluated in float32 (numpy, any summation order), per output element: wf_bound contracted
    with |K_values|, where the accumulation factor n / 2 becomes (K + P Cin + 4) / 2 -- K terms per weighted feature, P Cin terms of
    contraction (two matmuls and a sum over the kernel points in the reference), the modulation and the final conversions.
    -> [Nq, Cout]."""
    Nq, Ns = len(q), len(s)
    P, Cin, K = np.asarray(KP).shape[0], np.asarray(f).shape[1], np.asarray(idx).shape[1]
    r = kpconv_deform_f64(q, s, idx, np.abs(f), KP, offsets, None, None, extent, influence, mode)
    af = np.abs(np.asarray(f, np.float64))
    safe = np.where(r["valid"], np.asarray(idx, np.int64), 0)
    s_f = (af[safe] * r["in_range"][:, :, None]).sum(1)[:, None, :]
    m = np.linalg.norm(np.asarray(offsets, np.float64).reshape(Nq, -1, 3), axis=-1).max(-1) / float(extent)
    b = 2.0 ** -23 * (c_h(influence, m)[:, None, None] * s_f + 0.5 * (K + P * Cin + 4) * r["wf"])
    if modulations is not None:
        b = b * np.asarray(modulations, np.float64)[:, :, None]
    return b.reshape(Nq, P * Cin) @ np.abs(np.asarray(K_values, np.float64)).reshape(P * Cin, -1)


def block_bound(layer_ind, inputs, features, radius, fdim, config, W, scope, strided=False):
    """First-order bound of |block32 - block64| for resnetb_deformable[_strided] with 'linear' influence and 'sum' aggregation (the
    only discontinuity left, the range test, is then harmless: a neighbour at the boundary has h = 0 on either side), every stage's
    incoming error propagated through the stage's own absolute-value operator and its local roundings added, u = 2^-24:
      conv1   E1 = (Cin + 6) u (|f| |W1| |s1| + |t1|)                          (a Cin-term dot product, the affine batch norm, leaky)
      offsets Er = [ sum |W0| sum_k h0 E1 ] / cnt + 2^-23 [ 5.5 S|x1| + (K + P C + 4) / 2 S_h0|x1| ] |W0| / cnt + 2 u |raw|
              (the rigid operator: c_h = 5.5 of tests/test_gpu_kpconv_branches.py; needs the neighbour counts decided: asserted)
      conv2   a kernel point moves by e |delta raw[n, 3p .. 3p+2]| and 'linear' is 1 / e-Lipschitz in it: dh[n,p] <= sum_3 Er + c_h 2^-23;
              a modulation has slope <= 1 / 2: dm[n,p] <= Er / 2 + 2.5 * 2^-23 m
              E2 = sum |W2| m sum_k h E1 + sum |W2| m dh S'|x1| + sum |W2| dm sum_k h |x1| + 2^-23 (K + P C + 4) / 2 sum |W2| m sum_k h |x1|
              (S': over the neighbours within 1.001 KP_extent of a deformed point), then batch norm + leaky: E2 |s2| + 2 u |x2|
      conv3   E3 = (E2 |W3| + (C + 4) u |x2| |W3|) |s3| + 2 u |y3|;  shortcut Es likewise (none for an identity / max-pool shortcut)
      out     E3 + Es + u |out|
    -> (out64 [n, 2 fdim], bound [n, 2 fdim])."""
    from oracle import network_np as onp
    assert config.KP_influence == "linear" and config.convolution_mode == "sum"
    u = 2.0 ** -24
    w = lambda name: np.asarray(W[scope + "/" + name], np.float64)

    def affine(sc):
        g, b, m, v = (np.asarray(W[sc + "/batch_normalization/" + n], np.float64) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        inv = g / np.sqrt(v + 1e-6)
        return inv, b - m * inv
    f = np.asarray(features, np.float64)
    cin = f.shape[1]
    s1, t1 = affine(scope + "/conv1")
    x1 = _leaky((f @ w("conv1/weights")) * s1 + t1)
    E1 = (cin + 6) * u * ((np.abs(f) @ np.abs(w("conv1/weights"))) * np.abs(s1) + np.abs(t1))
    pts = [np.asarray(p, np.float64) for p in inputs["points"]]
    if strided:
        q, s, nb = pts[layer_ind + 1], pts[layer_ind], np.asarray(inputs["pools"][layer_ind], np.int64)
    else:
        q, s, nb = pts[layer_ind], pts[layer_ind], np.asarray(inputs["neighbors"][layer_ind], np.int64)
    e = config.KP_extent * radius / config.density_parameter
    KP, W0, b0, W2 = w("conv2/kernel_points"), w("conv2/offset_conv_weights"), w("conv2/offset_conv_bias"), w("conv2/weights")
    P, C, K, Nq = KP.shape[0], x1.shape[1], nb.shape[1], len(q)
    modulated = bool(config.modulated)
    # the neighbour count of the rigid offset convolution: row sums of x1 decided
    rs = x1.sum(1)
    assert np.all(np.abs(rs) > 4 * E1.sum(1)), "a row sum of conv1's output is within rounding of 0"
    rigid = lambda feats, Wt: onp.kpconv_f64(q, s, nb, feats, KP, Wt, e, "linear", "sum")
    wf0, cnt, raw = onp.kpconv_f64(q, s, nb, x1, KP, W0, e, "linear", "sum", col_shift=b0)
    cnt = np.maximum(onp.kpconv_f64(q, s, nb, x1, KP, None, e)[1], 1)[:, None]
    aW0 = np.abs(W0)
    valid = (nb >= 0) & (nb < len(s))
    S_x1 = (np.abs(x1)[np.where(valid, nb, 0)] * valid[:, :, None]).sum(1)                              # [Nq, C]
    prop = rigid(E1, aW0)[0].reshape(Nq, P * C) @ aW0.reshape(P * C, -1) / cnt
    loc = 2.0 ** -23 * (5.5 * np.tile(S_x1, (1, P)) + 0.5 * (K + P * C + 4) * rigid(np.abs(x1), None)[0].reshape(Nq, P * C)) \
        @ aW0.reshape(P * C, -1) / cnt
    Er = prop + loc + 2 * u * np.abs(raw)
    off, mod = deformed_from_raw(raw, P, e, modulated)
    m1 = mod if modulated else np.ones((Nq, P))
    m_e = np.linalg.norm(off, axis=-1).max(-1) / e
    dh = Er[:, :3 * P].reshape(Nq, P, 3).sum(-1) + (c_h("linear", m_e) * 2.0 ** -23)[:, None]           # [Nq, P]
    dm = 0.5 * Er[:, 3 * P:] + 2.5 * 2.0 ** -23 * m1 if modulated else np.zeros((Nq, P))
    aW2 = np.abs(W2).reshape(P * C, -1)
    con = lambda feats, ext: kpconv_deform_f64(q, s, nb, feats, KP, off, None, None, ext, "linear", "sum")
    r = kpconv_deformable_f64(q, s, nb, x1, KP, W2, W0, b0, e, "linear", "sum", modulated)
    wide = con(np.abs(x1), 1.001 * e)["in_range"]
    S_wide = (np.abs(x1)[np.where(valid, nb, 0)] * wide[:, :, None]).sum(1)                             # [Nq, C]
    h_abs = con(np.abs(x1), e)["wf"]                                                                    # sum_k h |x1|   [Nq, P, C]
    E2 = (con(E1, e)["wf"] * m1[:, :, None]).reshape(Nq, P * C) @ aW2 \
        + ((m1 * dh)[:, :, None] * S_wide[:, None, :]).reshape(Nq, P * C) @ aW2 \
        + (dm[:, :, None] * h_abs).reshape(Nq, P * C) @ aW2 \
        + 2.0 ** -23 * 0.5 * (K + P * C + 4) * (m1[:, :, None] * h_abs).reshape(Nq, P * C) @ aW2
    s2, t2 = affine(scope + "/conv2")
    x2 = _leaky(r["out"] * s2 + t2)
    E2 = E2 * np.abs(s2) + 2 * u * (np.abs(r["out"] * s2) + np.abs(t2))
    s3, t3 = affine(scope + "/conv3")
    y3 = (x2 @ w("conv3/weights")) * s3 + t3
    E3 = (E2 @ np.abs(w("conv3/weights")) + (C + 4) * u * (np.abs(x2) @ np.abs(w("conv3/weights")))) * np.abs(s3) + 2 * u * (np.abs(y3) + np.abs(t3))
    sc = _ind_max_pool(f, inputs["pools"][layer_ind]) if strided else f
    Es = 0.0
    if sc.shape[1] != 2 * fdim:
        ss, ts = affine(scope + "/shortcut")
        Es = (sc.shape[1] + 6) * u * ((np.abs(sc) @ np.abs(w("shortcut/weights"))) * np.abs(ss) + np.abs(ts))
        sc = (sc @ w("shortcut/weights")) * ss + ts
    out = _leaky(y3 + sc)
    return out, E3 + Es + u * (np.abs(y3) + np.abs(sc))
