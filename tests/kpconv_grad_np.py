"""TEST INFRASTRUCTURE ONLY.  The backward of the rigid KPConv (include/d3feat_amd.h, d3f_kpconv_backward) in float64 numpy -- the
definition the device code is held to -- with the rectangular transposed table, first-order error bounds of the fp32 evaluation,
a torch restatement of kernels/convolution_ops.py:161-255 for autograd, and the grid of cases the CPU and the GPU tests share.

    gradients(case, W, gout, influence, aggregation)   -> dict(gf [Ns, Cin], gW [num_kp, Cin, Cout], count [Nq], ...)
    transpose_qs_np(idx, nq, ns, Ns)                   -> (start i32[Ns + 1], edges i32[valid edges])
    tolerances(res)                                    -> (bound of gf per entry, bound of gW per entry)
    cap(tol, largest)                                  -> min(tol, 1e-4 largest)
    GRID, grid_case(name), grid_operands(name)         the cases (oracle.kpconv_cases.kpconv_case: its row-sum and arg-min
                                                       conditions are asserted there on everything it returns)
"""
import functools

import numpy as np

from oracle import kpconv_cases as kc
from oracle import network_np

U = 2.0 ** -24
BAR = 1e-4                       # the project's cap: 1e-4 of the largest entry compared
EXTENT = kc.EXTENT
MODES = kc.MODES
C_H = {"constant": 0.0, "linear": 5.5, "gaussian": 6.5}        # |delta h| <= C_H * 2^-23 (tests/test_gpu_kpconv_branches.py)
SLICE = 256                      # KPB_SLICE_MIN of csrc/kp_backward.h: the gW slice of every capacity up to 128 * 256 rows


def influences(c, influence, aggregation):
    """h f64[Nq, K, P] (zero on shadow slots, masked to the arg-min kernel point under 'closest'), valid bool[Nq, K], safe i64[Nq, K]:
    the expressions of oracle.network_np.kpconv_f64, lines :194-234."""
    Nq, Ns = c.Nq, c.Ns
    q, s, KP = np.asarray(c.q, np.float64)[:Nq], np.asarray(c.s, np.float64)[:Ns], np.asarray(c.KP, np.float64)
    idx = np.asarray(c.idx, np.int64)[:Nq]
    P = KP.shape[0]
    valid = (idx >= 0) & (idx < Ns)
    safe = np.where(valid, idx, 0)
    if Ns == 0 or idx.shape[1] == 0:
        return np.zeros(idx.shape + (P,)), valid, safe
    rel = s[safe] - q[:, None, :]
    d2 = ((rel[:, :, None, :] - KP[None, None]) ** 2).sum(-1)
    if influence == "constant":
        h = np.ones_like(d2)
    elif influence == "linear":
        h = np.maximum(1.0 - np.sqrt(d2 + 1e-10) / (2.0 * EXTENT), 0.0)
    elif influence == "gaussian":
        h = np.exp(-d2 / (2.0 * (EXTENT * 0.3) ** 2 + 1e-9))
    else:
        raise ValueError(influence)
    if aggregation == "closest":
        h = h * (np.arange(P)[None, None, :] == d2.argmin(-1)[:, :, None])
    elif aggregation != "sum":
        raise ValueError(aggregation)
    return h * valid[:, :, None], valid, safe


def gradients(c, W, gout, influence="linear", aggregation="sum"):
    """The definition: g = gout / max(count, 1); gW = sum_n wf g; gwf = sum_o g W; msg = sum_p h gwf; gf = the scatter of msg."""
    Nq, Ns = c.Nq, c.Ns
    W = np.asarray(W, np.float64)
    P, Cin, Cout = W.shape
    f = np.asarray(c.f, np.float64)[:Ns]
    gout = np.asarray(gout, np.float64)[:Nq]
    wf, count, _ = network_np.kpconv_f64(c.q, c.s, c.idx, c.f, c.KP, None, EXTENT, influence, aggregation, Nq=Nq, Ns=Ns)
    h, valid, safe = influences(c, influence, aggregation)
    g = gout / np.maximum(count, 1)[:, None]
    gW = np.einsum("npc,no->pco", wf, g)
    gwf = np.einsum("no,pco->npc", g, W)
    msg = np.einsum("nkp,npc->nkc", h, gwf)
    gf = np.zeros((Ns, Cin))
    np.add.at(gf, safe[valid], msg[valid])
    return dict(gf=gf, gW=gW, count=count, wf=wf, h=h, valid=valid, safe=safe, g=g, gwf=gwf, msg=msg, f=f, W=W, influence=influence,
                Nq=Nq, Ns=Ns, K=valid.shape[1])


def transpose_qs_np(idx, nq, ns, Ns=None):
    """The rectangular table of include/d3feat_amd.h (d3f_neighbor_transpose_qs): the stable argsort of the valid edges' keys."""
    idx = np.asarray(idx, np.int64)[:nq]
    Ns = ns if Ns is None else int(Ns)
    keys = idx.reshape(-1)
    e = np.arange(keys.size, dtype=np.int64)
    valid = (keys >= 0) & (keys < ns)
    kv, ev = keys[valid], e[valid]
    order = np.argsort(kv, kind="stable")
    start = np.searchsorted(kv[order], np.minimum(np.arange(Ns + 1), ns), side="left")
    return start.astype(np.int32), ev[order].astype(np.int32)


def tolerances(res):
    """Absolute first-order bounds of the fp32 evaluation of d3f_kpconv_backward against float64, per entry, derived from the case.
    A sum of L fp32 terms is bounded by (L + 16) u sum |terms| (u = 2^-24; the 16 covers the few roundings of forming a term), and
    the errors of the terms are added on top:
      h      |dh| <= C_H 2^-23 (the derivation of tests/test_gpu_kpconv_branches.py; 0 for 'constant');
      wf     2^-23 (C_H sum_k |f_k| + K / 2 sum_k h_k |f_k|), the bound of the forward's tests;
      g      gout * inv_cnt, inv_cnt a rounded reciprocal: 2 u |g|;
      gW     L = nq terms wf g (a slice's chain, then the chain over the slices: no term passes more than nq + 1 additions):
             (nq + 16) u sum_n |wf g| + sum_n (dwf |g| + |wf| dg);
      gwf    L = Cout terms, then the product with inv_cnt: (Cout + 18) u sum_o |g W|;
      msg    L = num_kp fused multiply-adds: (P + 16) u sum_p h |gwf| + sum_p (dh |gwf| + h dgwf);
      gf     L = the in-degree of the row: (deg + 16) u sum |msg| + sum dmsg.
    -> (tol_gf f64[Ns, Cin], tol_gW f64[P, Cin, Cout])."""
    h, valid, safe, g, W, f = res["h"], res["valid"], res["safe"], res["g"], res["W"], res["f"]
    Nq, Ns, K = res["Nq"], res["Ns"], res["K"]
    P, Cin, Cout = W.shape
    ch = C_H[res["influence"]]
    absf = np.abs(f)[safe] * valid[:, :, None] if Ns and K else np.zeros((Nq, K, Cin))        # [Nq, K, Cin]
    abs_wf = np.einsum("nkp,nkc->npc", h, absf)
    d_wf = 2 * U * (ch * absf.sum(1)[:, None, :] + K / 2.0 * abs_wf)
    d_g = 2 * U * np.abs(g)
    tol_gW = (Nq + 16) * U * np.einsum("npc,no->pco", np.abs(res["wf"]), np.abs(g)) + np.einsum("npc,no->pco", d_wf, np.abs(g)) + \
        np.einsum("npc,no->pco", np.abs(res["wf"]), d_g)
    d_gwf = (Cout + 18) * U * np.einsum("no,pco->npc", np.abs(g), np.abs(W))
    abs_gwf = np.abs(res["gwf"])
    d_h = 2 * U * ch * valid[:, :, None]
    abs_msg = np.einsum("nkp,npc->nkc", h, abs_gwf)
    d_msg = (P + 16) * U * abs_msg + np.einsum("nkp,npc->nkc", d_h * np.ones_like(h), abs_gwf) + np.einsum("nkp,npc->nkc", h, d_gwf)
    deg = np.zeros(Ns)
    sum_abs, sum_d = np.zeros((Ns, Cin)), np.zeros((Ns, Cin))
    np.add.at(deg, safe[valid], 1)
    np.add.at(sum_abs, safe[valid], abs_msg[valid])
    np.add.at(sum_d, safe[valid], d_msg[valid])
    tol_gf = ((deg + 16) * U)[:, None] * sum_abs + sum_d
    return tol_gf, tol_gW


def cap(tol, largest):
    return min(tol, BAR * largest)


# ---- the second statement: autograd of a torch restatement of kernels/convolution_ops.py:161-255 ------------------------------------
def torch_kpconv(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent, KP_influence, aggregation_mode):
    """KPConv_ops line by line (tf -> torch).  neighbors_indices: shadow slots already mapped to n0 (the reference's own shadow index)."""
    import torch
    n_kp = int(K_points.shape[0])
    shadow_point = torch.ones_like(support_points[:1, :]) * 1e6                                          # :190
    support_points = torch.cat([support_points, shadow_point], 0)                                        # :191
    neighbors = support_points[neighbors_indices]                                                        # :194
    neighbors = neighbors - query_points.unsqueeze(1)                                                    # :197
    neighbors = neighbors.unsqueeze(2)                                                                   # :200
    neighbors = neighbors.repeat(1, 1, n_kp, 1)                                                          # :201
    differences = neighbors - K_points                                                                   # :202
    sq_distances = (differences ** 2).sum(3)                                                             # :205
    if KP_influence == "constant":                                                                       # :208-211
        all_weights = torch.ones_like(sq_distances).permute(0, 2, 1)
    elif KP_influence == "linear":                                                                       # :213-216
        all_weights = torch.clamp_min(1 - torch.sqrt(sq_distances + 1e-10) / (2 * KP_extent), 0.0).permute(0, 2, 1)
    elif KP_influence == "gaussian":                                                                     # :218-222
        sigma = KP_extent * 0.3
        all_weights = torch.exp(-sq_distances / (2 * sigma ** 2 + 1e-9)).permute(0, 2, 1)
    else:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation_mode == "closest":                                                                    # :227-229
        neighbors_1nn = sq_distances.argmin(2)
        all_weights = all_weights * torch.nn.functional.one_hot(neighbors_1nn, n_kp).permute(0, 2, 1).to(all_weights.dtype)
    elif aggregation_mode != "sum":
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    features = torch.cat([features, torch.zeros_like(features[:1, :])], 0)                               # :234
    neighborhood_features = features[neighbors_indices]                                                  # :237
    weighted_features = torch.matmul(all_weights, neighborhood_features)                                 # :240
    weighted_features = weighted_features.permute(1, 0, 2)                                               # :243
    kernel_outputs = torch.matmul(weighted_features, K_values)                                           # :244
    output_features = kernel_outputs.sum(0)                                                              # :247
    neighbor_features_sum = neighborhood_features.sum(-1)                                                # :250
    neighbor_num = (neighbor_features_sum > 0.0).to(features.dtype).sum(-1)                              # :251
    neighbor_num = torch.clamp_min(neighbor_num, 1)                                                      # :252
    return output_features / neighbor_num.unsqueeze(1)                                                   # :253


def torch_gradients(c, W, gout, influence, aggregation, dtype="float64"):
    """(gf, gW) of autograd through torch_kpconv on the CPU, as float64 numpy.  The rows whose exact sum is 0 (the cases plant
    them) are decided by the float sum of torch here: the +- pairs of multiples of 2^-8 and the zero rows sum to exactly 0 in any
    order and precision, every other row is 2^-10 of its absolute sum away from 0 (oracle.kpconv_cases, condition 1)."""
    import torch
    dt = getattr(torch, dtype)
    Nq, Ns = c.Nq, c.Ns
    idx = np.asarray(c.idx, np.int64)[:Nq]
    idx = np.where((idx >= 0) & (idx < Ns), idx, Ns)
    f = torch.tensor(np.asarray(c.f)[:Ns], dtype=dt, requires_grad=True)
    Wt = torch.tensor(np.asarray(W), dtype=dt, requires_grad=True)
    out = torch_kpconv(torch.tensor(np.asarray(c.q)[:Nq], dtype=dt), torch.tensor(np.asarray(c.s)[:Ns], dtype=dt), torch.tensor(idx), f,
                       torch.tensor(np.asarray(c.KP), dtype=dt), Wt, EXTENT, influence, aggregation)
    (out * torch.tensor(np.asarray(gout)[:Nq], dtype=dt)).sum().backward()
    return f.grad.double().numpy(), Wt.grad.double().numpy()


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# name -> (Cin, Cout, K, Nq, Ns, num_kp, self_queries, modes).  Every case carries 5 capacity query rows and 7 capacity support rows
# (NaN points and features, index rows that point at valid supports); with Nq >= 4 rows 1 and Nq // 2 hold no valid slot.
_FAST = (("linear", "sum"),)
GRID = {
    "c1": (1, 32, 17, 150, 150, 15, False, _FAST + (("gaussian", "closest"),)),
    "c5": (5, 3, 17, 150, 150, 15, False, _FAST + (("constant", "closest"),)),
    "c32k1": (32, 32, 1, 150, 150, 15, False, _FAST),
    "c32k17": (32, 32, 17, 150, 150, 15, False, tuple(MODES)),
    "c32k42": (32, 32, 42, 150, 150, 15, False, _FAST),
    "c32k1p13": (32, 32, 1, 150, 150, 13, False, _FAST),
    "c32k17p13": (32, 32, 17, 150, 150, 13, False, _FAST),
    "c32k42p13": (32, 32, 42, 150, 150, 13, False, _FAST),
    "c32k1p4": (32, 32, 1, 150, 150, 4, False, _FAST),
    "c32k17p4": (32, 32, 17, 150, 150, 4, False, _FAST),
    "c32k42p4": (32, 32, 42, 150, 150, 4, False, _FAST),
    "c64": (64, 64, 17, 150, 150, 15, False, _FAST),
    "c128": (128, 64, 17, 150, 150, 15, False, _FAST + (("linear", "closest"),)),
    "self": (32, 32, 17, 150, 150, 15, True, _FAST),
    "nq1": (32, 32, 17, 1, 150, 15, False, _FAST),
    "nq7": (32, 32, 17, 7, 150, 15, False, _FAST),
    "slices": (32, 32, 17, 2 * SLICE + 37, 150, 15, False, _FAST),       # two slices of the gW reduction and a ragged remainder
    # the other steps of the message kernel's lanes-per-query ladder (Cin = 4 LQ), each in its straight-line and its general form
    "c4": (4, 8, 17, 150, 150, 15, False, _FAST + (("gaussian", "sum"),)),
    "c8": (8, 8, 9, 150, 150, 15, False, _FAST + (("linear", "closest"),)),
    "c16": (16, 40, 17, 150, 150, 15, False, _FAST + (("constant", "closest"),)),
    "c256": (256, 16, 17, 40, 150, 15, False, _FAST + (("linear", "closest"),)),
    "c512": (512, 8, 9, 20, 150, 15, False, _FAST + (("gaussian", "sum"),)),
    "c1024": (1024, 8, 5, 9, 150, 15, False, _FAST + (("gaussian", "closest"),)),
    "c12": (12, 7, 17, 150, 150, 15, False, _FAST),                      # Cin % 4 == 0 off the ladder: the general message kernel
}
CAP_Q, CAP_S = 5, 7


def _seed(name):
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def grid_case(name):
    Cin, Cout, K, Nq, Ns, num_kp, self_q, _ = GRID[name]
    return kc.kpconv_case(_seed(name), Cin, K, Nq, Ns=Ns, num_kp=num_kp, self_queries=self_q, cap_q=CAP_Q, cap_s=CAP_S)


@functools.lru_cache(maxsize=None)
def grid_operands(name):
    """-> (W f32[num_kp, Cin, Cout], gout f32[Nq + CAP_Q, Cout]: N(0, 1) rows, NaN in the capacity rows)."""
    Cin, Cout, K, Nq, Ns, num_kp, _, _ = GRID[name]
    W = kc.weights(_seed(name), num_kp, Cin, Cout)
    gout = np.random.default_rng(_seed(name) + 1).standard_normal((Nq + CAP_Q, Cout)).astype(np.float32)
    gout[Nq:] = np.nan
    return W, gout


def modes_of(name):
    return GRID[name][7]


@functools.lru_cache(maxsize=None)
def grid_gradients(name, influence, aggregation):
    """The float64 definition of one case and mode, computed once and shared (never modified by a test)."""
    W, gout = grid_operands(name)
    return gradients(grid_case(name), W, gout, influence, aggregation)
