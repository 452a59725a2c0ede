"""The whole network on the MI355X at every value of the configuration, against float64.

Every other test that runs KernelPointFCNN or FragmentEngine on a device uses threedmatch_config() or kitti_config(): one point of the
configuration space (linear / sum, batch norm, width 64, 15 kernel points, one input feature, five layers).  The Python between the
configuration and the kernels branches on all of these values -- the four KPConv routes of kernels/convolution_ops.KPConv_ops, the
fused / non-fused shortcut of models/network_blocks._resnetb, the `offset` path without batch norm, the contraction router and the
two decoder forms of d3feat_amd.ops.  This module runs the cases of tests/network_config_cases.py (inputs, weights, conditions) and
compares every materialised block output, the descriptors and the scores with tests/network_f64_np.py, the float64 definition.

Block outputs: max |diff| <= bar * max(1, max |want|); descriptors and scores: max |diff| <= bar, absolute.  The blocks are compared
because the outputs hide scale: descriptors are l2-normalised and scores divide by a per-cloud maximum.

The bar is the project's 1e-4 (BASELINE.json north star), or four times the float32-CPU-against-float64 figure of the case where that
figure exceeds 2.5e-5 (network_config_cases.bar; the factor allows for another summation order and FMA contraction).  No case needs
the second form.  float32 CPU: tests/test_network_config_host.py::test_float32_oracle_against_the_definition; MI355X: the figure of
test_forward_equals_the_float64_definition (the worst of blocks, descriptors, scores), as measured when this module was written:

    case             float32 CPU   bar     MI355X
    shipped          2.3e-06       1e-4    1.5e-06
    constant         2.8e-06       1e-4    2.5e-06
    gaussian         2.4e-06       1e-4    2.4e-06
    closest          1.5e-06       1e-4    1.3e-06
    class_defaults   3.2e-06       1e-4    2.3e-06
    no_bn            2.6e-06       1e-4    1.7e-06
    w32              1.7e-06       1e-4    1.5e-06
    w128             1.9e-06       1e-4    1.9e-06
    w18              7.3e-06       1e-4    4.7e-06
    kp13             1.6e-06       1e-4    1.6e-06
    kp4              1.6e-06       1e-4    1.9e-06
    cin4             1.6e-06       1e-4    1.3e-06
    geometry         2.3e-06       1e-4    1.7e-06
    three_layers     1.3e-06       1e-4    1.1e-06
    mixed            2.0e-06       1e-4    1.3e-06
    engine replays   class_defaults 2.1e-06, mixed 1.6e-06 (against the definition on the engine's own pyramid)
"""
import numpy as np
import pytest
import torch

import network_config_cases as nc
from test_gpu_golden_network import _dev, _record_blocks

pytestmark = pytest.mark.gpu
ALL = list(nc.CASES)
_RUNS = {}


def _flat(inp, device):
    """The positional list of datasets/common.py:1410-1413 + the dataset tail (datasets/ThreeDMatch.py:322) from a pyramid dict."""
    flat = [_dev(p, device) for p in inp["points"]] + [_dev(m, device) for m in inp["neighbors"]]
    flat += [_dev(m, device) for m in inp["pools"]] + [_dev(m, device) for m in inp["upsamples"]]
    flat += [_dev(inp["features"], device), _dev(inp["batch_weights"], device), _dev(inp["in_batches"], device),
             _dev(inp["out_batches"], device)]
    flat += [_dev(inp["stack_lengths"], device), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ["a", "b"],
             _dev(inp["points"][0], device)]
    return flat


def _forward(case, device, W=None):
    """One KernelPointFCNN run of the case -> (descriptors, scores, {scope: block output}, [entry points taken])."""
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    got, restore = _record_blocks()
    calls = []
    try:
        with nc.spy_ops(calls):
            model = KernelPointFCNN(_flat(nc.inputs(case), device), nc.config(case), weights=dict(nc.weights(case) if W is None else W))
    finally:
        restore()
    assert set(model.weights()) == set(nc.weights(case))                       # the model created no variable of its own
    return model.out_features.cpu().numpy(), model.out_scores.cpu().numpy(), {k: v.cpu().numpy() for k, v in got.items()}, calls


def _run(case, device):
    if case not in _RUNS:
        _RUNS[case] = _forward(case, device)
    return _RUNS[case]


@pytest.mark.parametrize("case", ALL)
def test_forward_equals_the_float64_definition(device, case):
    nc.check_conditions(case)
    d, s, blocks, _ = _run(case, device)
    ref = nc.reference(case)
    cfg = nc.config(case)
    # every block but the nearest_upsample ones, which stay lazy on the HIP path (contracted by the unary block that follows)
    assert set(blocks) == {k for k in ref[2] if "nearest_upsample" not in k} and len(blocks) == len(ref[2]) - (cfg.num_layers - 1)
    assert np.isfinite(d).all() and np.isfinite(s).all()
    fig, figs = nc.deviation(d, s, blocks, ref)
    print("%-15s MI355X vs float64: %.2e (%s)   bar %.1e" % (case, fig, max(figs, key=figs.get), nc.bar(case)))
    nc.deviation(d, s, blocks, ref, bound=nc.bar(case))


def test_routes_really_taken(device):
    """The guard against a later router change silently emptying a case: over all cases every KPConv route ran in at least two, the
    non-fused shortcut (a contraction with `residual=`) ran where the width or the missing batch norm asks for it, both decoder
    forms ran."""
    calls = {case: _run(case, device)[3] for case in ALL}
    for case in ALL:
        print("%-15s %s" % (case, {n: calls[case].count(n) for n in sorted(set(calls[case]))}))
    nc.assert_routes(calls)


def test_row_count_rule_is_exercised(device):
    """The shipped case again with the unshifted betas: the outputs differ, on the device as in the definition, and both runs meet the
    definition -- so the shifted weights do change which neighbours count, and the flags follow the features from block to block."""
    d1, s1, b1, _ = _run("shipped", device)
    W0 = nc.weights("shipped", shifted=False)
    d0, s0, b0, _ = _forward("shipped", device, W0)
    ref0 = nc.reference("shipped", shifted=False)
    nc.deviation(d0, s0, b0, ref0, bound=nc.bar("shipped"))
    assert np.abs(d1 - d0).max() > 100 * nc.BAR and np.abs(s1 - s0).max() > 100 * nc.BAR
    shares0, shares1 = ([r["share"] for r in ref[3]] for ref in (ref0, nc.reference("shipped")))
    mixed = lambda shares: sum(1 for x in shares if 0.05 <= x <= 0.95)
    assert mixed(shares0) < 3 <= mixed(shares1)                                            # degenerate without the shift


@pytest.mark.parametrize("case", ["geometry", "three_layers"])
def test_pyramid_equals_the_oracle(device, case):
    """FragmentDataset's mapping under other radii / another depth == the oracle pyramid, matrix by matrix, bit for bit (exact
    shapes); the fast (padded) variant equals it on the valid columns and holds the shadow index elsewhere -- as
    tests/test_gpu_network.py::test_pyramid_vs_oracle does at the shipped configuration."""
    from d3feat_amd.datasets.common import FragmentDataset
    cfg = nc.config(case)
    want = nc.engine_inputs(case)                      # the unedited oracle pyramid of the self-pair
    limits = nc.limits(cfg)
    L = cfg.num_layers
    assert len(want["points"]) == L
    for fast in (False, True):
        ds = FragmentDataset([nc.cloud()], fast=fast)
        ds.neighborhood_limits = limits
        gen, _, _ = ds.get_batch_gen("test", cfg)
        flat = ds.get_tf_mapping(cfg)(*ds._to_device(next(iter(gen()))))
        for l in range(L):
            assert np.array_equal(flat[l].cpu().numpy().view(np.uint32), want["points"][l].view(np.uint32))
            for name, off in (("neighbors", L), ("pools", 2 * L), ("upsamples", 3 * L)):
                g, w = flat[off + l].cpu().numpy(), want[name][l]
                if w.shape[0] == 0:
                    assert g.shape[0] == 0
                    continue
                if not fast:
                    assert np.array_equal(g, w), (name, l)
                elif name == "upsamples":
                    assert np.array_equal(g[:, 0], w[:, 0])
                else:
                    pad = want["points"][l].shape[0]
                    assert g.shape[1] == limits[l]
                    assert np.array_equal(g[:, :w.shape[1]], w), (name, l)
                    assert np.all(g[:, w.shape[1]:] == pad)
        if not fast:
            assert np.array_equal(flat[4 * L + 2].cpu().numpy(), want["in_batches"])
            assert np.array_equal(flat[4 * L + 3].cpu().numpy(), want["out_batches"])
            assert np.allclose(flat[4 * L + 1].cpu().numpy(), want["batch_weights"])


def _close(a, b, tol):
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("case", ["class_defaults", "mixed"])
def test_engine_carries_the_configuration(device, case):
    """The captured sequence of FragmentEngine at a configuration that is not the shipped one: one replay against run_eager (held to
    what tests/test_gpu_engine.py::test_engine_matches_eager_and_oracle demands of the shipped configuration) and against the float64
    definition on the engine's own pyramid, at the case's bar; no fallback.  (level_ratio: level 1 of this sparse cloud keeps 0.66 of
    level 0's rows, above the default capacity ratio of 0.4.)"""
    from d3feat_amd.engine import FragmentEngine
    fig = nc.check_engine_conditions(case)
    cfg = nc.config(case)
    eng = FragmentEngine(cfg, dict(nc.weights(case)), nc.limits(cfg), raw_cap=8192, n0_cap=4096, level_ratio=0.7, slots=1, device=device)
    raw = torch.from_numpy(nc.raw_cloud()).to(device)
    pts, d, s = (t.clone() for t in eng.run(raw))
    assert eng.fallbacks == 0
    ep, ed, es = eng.run_eager(raw)
    assert pts.shape == ep.shape and torch.equal(pts, ep)
    _close(d, ed, 2e-6)
    _close(s, es, 2e-6)
    sub = nc.cloud()
    assert np.array_equal(pts.cpu().numpy()[:len(sub)].view(np.uint32), sub.view(np.uint32))
    ref = nc.engine_reference(case)
    d, s = d.cpu().numpy().reshape(ref[0].shape), s.cpu().numpy().reshape(ref[1].shape)
    dev, _ = nc.deviation(d, s, {}, ref)
    print("%-15s engine replay vs float64: %.2e   bar %.1e   smallest arg-min gap %.1e" % (case, dev, nc.bar(case), fig["gap"]))
    nc.deviation(d, s, {}, ref, bound=nc.bar(case))
