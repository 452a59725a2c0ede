"""CPU side of the whole-network configuration tests (tests/test_gpu_network_configs.py holds the HIP path to the same definition):

  * tests/network_f64_np.py, the float64 definition, against what the REFERENCE'S OWN PYTHON computed (tests/golden/network_3dmatch.npz,
    network_kitti.npz: descriptors, scores, the sampled rows of every block) at the fixtures' bar of 1e-4;
  * the float32 CPU oracle (oracle/network_np.forward) against the definition at every case of tests/network_config_cases.py: the
    reference-against-reference figure the GPU bars rest on, printed per case (run with -s);
  * the conditions on the cases' inputs (near ties of 'closest', decided and mixed row-sum signs);
  * build_variables without batch norm: names, shapes and creation order of the reference, usable by a model that may create nothing.
"""
import numpy as np
import pytest
import torch

import network_config_cases as nc
import network_f64_np as f64
from oracle.golden_network import GoldenNetwork

ALL = list(nc.CASES)


@pytest.mark.parametrize("name", ["3dmatch", "kitti"])
def test_definition_equals_the_reference_python(name):
    g = GoldenNetwork(name)
    desc, score, trace, report = f64.forward(g.config(), g.W, g.inputs)
    assert list(trace) == g.block_order and len(report) == 10
    for scope in g.block_order:
        rows, want = g.block(scope)
        err = np.abs(trace[scope][rows] - want).max()
        assert err <= nc.BAR * max(1.0, float(np.abs(want).max())), (scope, err)
    assert desc.shape == g.descriptors.shape and score.shape == g.scores.shape
    ed, es = np.abs(desc - g.descriptors).max(), np.abs(score - g.scores).max()
    print("%s: float64 definition vs the reference's float32 run: descriptors %.2e scores %.2e" % (name, ed, es))
    assert ed <= nc.BAR and es <= nc.BAR, (ed, es)


def test_cases_are_the_issue_table():
    assert ALL == ["shipped", "constant", "gaussian", "closest", "class_defaults", "no_bn", "w32", "w128", "w18", "kp13", "kp4", "cin4",
                   "geometry", "three_layers", "mixed"]
    assert set(nc.CPU_DEVIATION) == set(ALL)
    cfg = nc.config("class_defaults")
    from d3feat_amd.utils.config import Config
    assert (cfg.KP_influence, cfg.convolution_mode) == (Config.KP_influence, Config.convolution_mode) == ("gaussian", "closest")
    assert nc.config("three_layers").num_layers == 3 and nc.config("shipped").num_layers == 5
    assert [len(p) for p in nc.inputs("shipped")["points"]] == [5192, 3442, 1190, 324, 80]
    w18 = nc.weights("w18")
    assert w18["layer_0/resnetb_1/conv2/weights"].shape == (15, 9, 9) and w18["layer_1/resnetb_0/conv2/weights"].shape == (15, 18, 18)
    assert nc.weights("kp4")["layer_2/resnetb_0/conv2/kernel_points"].shape == (4, 3)
    assert nc.inputs("cin4")["features"].shape == (5192, 4)


@pytest.mark.parametrize("case", ALL)
def test_float32_oracle_against_the_definition(case):
    """Reference against reference: one float32 evaluation (torch CPU) of the network against the float64 one.  bar(case) -- 1e-4, or
    four times the recorded figure (CPU_DEVIATION) where that exceeds 2.5e-5 -- must be at least four times what is measured here."""
    d, s, trace, _ = nc.oracle32(case)
    ref = nc.reference(case)
    assert list(trace) == list(ref[2])
    fig, figs = nc.deviation(d, s, trace, ref)
    worst = max(figs, key=figs.get)
    print("%-15s float32 CPU vs float64: %.2e (%s)   recorded %.1e   bar %.1e" % (case, fig, worst, nc.CPU_DEVIATION[case], nc.bar(case)))
    assert 4 * fig <= nc.bar(case)
    assert nc.bar(case) == (nc.BAR if nc.CPU_DEVIATION[case] <= 2.5e-5 else 4 * nc.CPU_DEVIATION[case])


@pytest.mark.parametrize("case", ALL)
def test_conditions_on_the_inputs(case):
    fig = nc.check_conditions(case)
    print("%-15s margins >= %.1e, shares %s, replaced %s" % (case, min(fig["margins"]), [round(x, 2) for x in fig["shares"]],
                                                              {"%s_%d" % k: v for k, v in fig["replaced"].items() if v[0]}))
    cfg = nc.config(case)
    if cfg.convolution_mode == "closest":
        assert len(fig["replaced"]) == 2 * cfg.num_layers - 1                  # every neighbour and pool matrix a KPConv reads
    else:
        assert not fig["replaced"]


def test_shifted_betas_are_what_mixes_the_signs():
    """With the unshifted weights the row-count rule is degenerate (every neighbour counts) -- what the shift is there to change."""
    shares = [r["share"] for r in nc.reference("shipped", shifted=False)[3]]
    assert sum(1 for s in shares if 0.05 <= s <= 0.95) < 3
    assert sum(1 for r in nc.reference("shipped")[3] if 0.05 <= r["share"] <= 0.95) >= 3


# ---- build_variables without batch norm -----------------------------------------------------------------------------------------------

def _reference_variables(cfg):
    """A shape-only walk of the variables the reference creates, in its order (models/network_blocks.py): weight_variable (:37-41), for a
    KPConv then `kernel_points` (kernels/convolution_ops.py:145-148), then what batch_norm creates -- gamma, beta, moving_mean,
    moving_variance of tf.layers.batch_normalization (:156-160) or `offset` (:162-165); blocks :194-244, :321-368, :561-612, the
    encoder loop :1052-1118, the decoder models/D3Feat.py:19-63."""
    out = []
    K = cfg.num_kernel_points

    def norm(scope, ch):
        if cfg.use_batch_norm:
            out.extend((scope + "/batch_normalization/" + n, (ch,)) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        else:
            out.append((scope + "/offset", (ch,)))

    def unary(scope, ci, co, normed=True):
        out.append((scope + "/weights", (ci, co)))
        if normed:
            norm(scope, co)

    def kpconv(scope, ci, co):
        out.append((scope + "/weights", (K, ci, co)))
        out.append((scope + "/kernel_points", (K, 3)))
        norm(scope, co)

    layer, fdim, bil, cin, skips = 0, cfg.first_features_dim, 0, cfg.in_features_dim, []
    arch = list(cfg.architecture)
    start = len(arch)
    for i, block in enumerate(arch):
        if "strided" in block or "upsample" in block:
            skips.append(cin)
        if "upsample" in block:
            start = i
            break
        scope = "layer_%d/%s_%d" % (layer, block, bil)
        if block == "simple":
            kpconv(scope, cin, fdim)
            cin = fdim
        else:
            unary(scope + "/conv1", cin, fdim // 2)
            kpconv(scope + "/conv2", fdim // 2, fdim // 2)
            unary(scope + "/conv3", fdim // 2, 2 * fdim)
            if cin != 2 * fdim:
                unary(scope + "/shortcut", cin, 2 * fdim)
            cin = 2 * fdim
        bil += 1
        if "strided" in block:
            layer, fdim, bil = layer + 1, fdim * 2, 0
    layer = cfg.num_layers - 1
    fdim, bil = cfg.first_features_dim * 2 ** layer, 0
    for block in arch[start:]:
        scope = "uplayer_%d/%s_%d" % (layer, block, bil)
        if block == "unary":
            unary(scope, cin, fdim)
            cin = fdim
        elif block == "last_unary":
            unary(scope, cin, 32, normed=False)
            cin = 32
        bil += 1
        if "upsample" in block:
            layer, fdim, bil = layer - 1, fdim // 2, 0
            cin += skips[layer]
    return out


def _shape_only_run(cfg, store, monkeypatch, calls=None):
    """assemble_FCNN_blocks on the case's pyramid with every kernel replaced by zeros of its output shape (host tensors, no GPU): the
    Python between the configuration and the kernels -- scopes, variable lookups, routing predicates -- runs as it is.  calls: the
    list that receives the names of the entry points taken (network_config_cases.spy_ops)."""
    from d3feat_amd.models import D3Feat as d3, network_blocks as nb
    z = lambda rows, cols: torch.zeros((int(rows), int(cols)))
    fused = lambda q, s, idx, f, kp, kv, *a, **k: z(q.shape[0], kv.shape[2])
    stubs = dict(kpconv_fused_c1=fused, kpconv_fused32=fused, kpconv_fused=fused,
                 kpconv_aggregate=lambda q, s, idx, f, kp, *a, **k: (z(q.shape[0], len(kp) * f.shape[1]), torch.ones(q.shape[0])),
                 gemm=lambda A, B, *a, **k: z(A.shape[0], B.shape[1]), gemm_cat2=lambda A1, A2, W, **k: z(A1.shape[0], W.shape[1]),
                 gemm_upsample_cat=lambda u, W, **k: z(u.shape[0], W.shape[1]),
                 gemm_upsample_split=lambda u, W1, W2, **k: z(u.shape[0], W2.shape[1]),
                 ind_max_pool=lambda x, inds: z(inds.shape[0], x.shape[1]))
    from d3feat_amd import ops
    monkeypatch.setattr(ops, "closest_pool_cat", lambda x, inds, skip=None: z(inds.shape[0], x.shape[1] + (skip.shape[1] if skip is not None else 0)))
    monkeypatch.setattr(d3, "detection_head", lambda features, inputs: (features, features[:, :1]))
    inp = nc.inputs("shipped" if cfg.num_layers == 5 else "three_layers")
    t = {k: [torch.from_numpy(np.ascontiguousarray(m)) for m in inp[k]] for k in ("points", "neighbors", "pools", "upsamples")}
    t["features"] = torch.ones((len(inp["points"][0]), cfg.in_features_dim))
    t["stack_lengths"] = torch.from_numpy(inp["stack_lengths"])
    with nc.spy_ops([] if calls is None else calls, stubs), nb.use_variables(store):
        d, s = d3.assemble_FCNN_blocks(t, cfg, 1.0)
    assert tuple(d.shape) == (len(inp["points"][0]), 32)


def test_routes_the_cases_take_as_the_host_predicts_them(monkeypatch):
    """What tests/test_gpu_network_configs.py::test_routes_really_taken asserts of the device runs, predicted here from the routing
    Python alone (kernels stubbed): the cases do spread over every KPConv route, both shortcut forms and both decoder forms."""
    from d3feat_amd.models.variables import VariableStore
    calls = {}
    for case in ALL:
        calls[case] = []
        _shape_only_run(nc.config(case), VariableStore(nc.weights(case), device=torch.device("cpu"), create=False), monkeypatch, calls[case])
        print("%-15s %s" % (case, {n: calls[case].count(n) for n in sorted(set(calls[case]))}))
    nc.assert_routes(calls)


@pytest.mark.parametrize("case", ["shipped", "no_bn", "w18", "mixed", "three_layers"])
def test_build_variables_creates_the_reference_variables(case, monkeypatch):
    """Names, shapes and creation order of build_variables equal the reference's, with and without batch norm (`offset` where the
    reference creates it, :162-165, and no batch_normalization/* then); a model that may create nothing finds every variable it asks
    for; and a model that creates its variables itself creates the same ones in the same order (_resnetb's promise)."""
    from d3feat_amd.models.variables import VariableStore, build_variables
    cfg = nc.config(case)
    kp = None if cfg.num_kernel_points == 15 else nc.drawn_kernel_points
    vs = build_variables(cfg, seed=3, kernel_points=kp)
    have = [(n, tuple(v.shape)) for n, v in vs.values.items()]
    want = _reference_variables(cfg)
    assert have == want
    if not cfg.use_batch_norm:
        assert not any("batch_normalization" in n for n, _ in have) and sum(n.endswith("/offset") for n, _ in have) >= 20
        assert all(not vs.values[n].any() for n, _ in have if n.endswith("/offset"))           # zeros, as tf.zeros (:164)
    cpu = torch.device("cpu")
    _shape_only_run(cfg, VariableStore(vs.values, device=cpu, create=False), monkeypatch)     # no KeyError
    if kp is None:
        lazy = VariableStore(seed=3, device=cpu)
        _shape_only_run(cfg, lazy, monkeypatch)
        assert [(n, tuple(v.shape)) for n, v in lazy.values.items()] == want
        assert all(np.array_equal(lazy.values[n], vs.values[n]) for n, _ in want)


def test_a_missing_offset_is_an_error(monkeypatch):
    from d3feat_amd.models.variables import VariableStore, build_variables
    cfg = nc.config("no_bn")
    W = dict(build_variables(cfg, seed=3).values)
    del W["layer_1/resnetb_0/conv3/offset"]
    with pytest.raises(KeyError):
        _shape_only_run(cfg, VariableStore(W, device=torch.device("cpu"), create=False), monkeypatch)
