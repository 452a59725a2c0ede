"""Whole encoder blocks in training mode on the GPU (models/network_blocks.py, training=True) against the float64 restatement
(tests/training_blocks_np.py): unary, simple, resnetb with a unary + BN shortcut (Cin 16 -> 64) and with the identity shortcut
(Cin 64 -> 64), each with batch norm and without, on a two-cloud stack of 150 + 131 rows, 12 neighbour slots, 15 kernel points.

Held against float64: the training-mode output, the gradient of sum(out R) with respect to the input features and to every entry of
vs.parameters(), and the updated moving statistics.  Tolerance per output, the project's rule: the larger of 4 * err32
(tests/golden/bn_grad.npz, "block/..." keys: float32 torch-CPU autograd of the same composition against float64) and the bound of the
longest sum an entry ends -- (L + 16) u of the largest entry, L = max(rows, num_kp * Cin of the KPConv) terms, u = 2^-24 --, capped at
1e-4 of the largest entry compared.  The moving statistics: three fp32 operations on a float64 statistic, 4 u of the largest entry.
The cases keep every pre-activation clear of zero (training_blocks_np.block_case), so the LeakyReLU masks are the float64 ones.

Measured on an MI355X (printed, never used as a bar): largest deviation 4.1e-7 of the largest entry of an output (simple, after the
in-place change), 2.6e-7 of an input gradient (resnetb_shortcut), 9.4e-7 of a parameter gradient (simple_0/weights) -- at most 0.053 of
the tolerance -- and 4.4e-8 of a moving statistic.  The 19 tests take 2 s.
"""
import os

import numpy as np
import pytest
import torch

import bn_grad_np as bg
import training_blocks_np as tb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "bn_grad.npz"))
    return {k: float(z[k]) for k in z.files if k.startswith("block/")}


def _inputs(dev):
    geo = tb.geometry()
    pts = torch.from_numpy(geo.points).to(dev)
    nb = torch.from_numpy(geo.neighbors).to(dev)
    return dict(points=[pts, pts], neighbors=[nb, nb], pools=[nb], upsamples=[nb])


def _store(name, use_bn, dev):
    from d3feat_amd.models.variables import VariableStore
    return VariableStore(values=tb.block_variables(name, use_bn), device=dev, create=False)


def _forward(name, vs, cfg, radius, feats, dev, training=True, block=None):
    from d3feat_amd.models import network_blocks as nb
    kind, _, fdim = tb.BLOCKS[name]
    with nb.use_variables(vs), nb.variable_scope(tb.scope_of(name)):
        return nb.get_block_ops(block or kind)(0, _inputs(dev), feats, radius, fdim, cfg, training)


def _held(label, key, got, want, golden, terms, bound_u=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    big = np.abs(want).max()
    bound = (bound_u if bound_u is not None else terms + 16) * bg.U * big
    tol = bg.cap(max(4 * golden.get(key, 0.0), bound), big)
    dev = np.abs(got - want).max()
    print("%s: largest %.3e, deviation %.2e of it, tolerance %.2e of it" % (label, big, dev / big, tol / big))
    assert dev <= tol, label
    return dev / big


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
@pytest.mark.parametrize("name", list(tb.BLOCKS))
def test_block_against_float64(device, golden, name, use_bn):
    kind, cin, fdim = tb.BLOCKS[name]
    V, feats, R = tb.block_case(name, use_bn)
    ref = tb.reference(name, use_bn)
    cfg, radius = tb.make_config(use_bn)
    vs = _store(name, use_bn, device)
    f = torch.from_numpy(feats).to(device).requires_grad_(True)
    out = _forward(name, vs, cfg, radius, f, device)
    (out * torch.from_numpy(R).to(device)).sum().backward()
    terms = max(tb.N, tb.NUM_KP * (cin if kind == "simple" else fdim // 2) if kind != "unary" else tb.N)
    prefix = "block/%s/%s/" % (name, "bn" if use_bn else "off")
    _held(name + " out", prefix + "out", out.detach().cpu().numpy(), ref["out"], golden, terms)
    _held(name + " gfeat", prefix + "gfeat", f.grad.cpu().numpy(), ref["gfeat"], golden, terms)
    params = vs.parameters()
    assert set(params) == set(ref["grads"])                       # every trainable variable of the block, and nothing else
    for k, p in params.items():
        assert p.grad is not None, k
        _held(k + " grad", prefix + k, p.grad.cpu().numpy(), ref["grads"][k], golden, terms)
    assert len(ref["moving"]) == (2 * sum(k.endswith("gamma") for k in params))
    for k, want in ref["moving"].items():
        got = vs.tensor(k).cpu().numpy()
        assert not np.array_equal(got, V[k])
        _held(k, None, got, want, golden, 0, bound_u=4)


@pytest.mark.parametrize("name", ["unary", "simple"])
def test_in_place_weight_change_reaches_the_next_forward(device, golden, name):
    """No stale packed copy: a weight changed in place between two training forwards changes the output as the definition says."""
    V, feats, R = tb.block_case(name, True)
    cfg, radius = tb.make_config(True)
    vs = _store(name, True, device)
    f = torch.from_numpy(feats).to(device)
    first = _forward(name, vs, cfg, radius, f, device).detach().clone()
    wname = tb.scope_of(name) + "/weights"
    delta = (0.05 * np.random.default_rng(1).standard_normal(V[wname].shape)).astype(np.float32)
    with torch.no_grad():
        vs.parameter(wname).add_(torch.from_numpy(delta).to(device))
    second = _forward(name, vs, cfg, radius, f, device).detach()
    V2 = dict(V)
    V2[wname] = (V[wname] + delta).astype(np.float32)
    want = tb._run(name, True, V2, feats, R)
    assert want["margin"] > 1e-6
    assert not torch.equal(first, second)
    terms = max(tb.N, tb.NUM_KP * tb.BLOCKS[name][1])
    _held(name + " out after the change", "block/%s/bn/out" % name, second.cpu().numpy(), want["out"], golden, terms)


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
@pytest.mark.parametrize("name", list(tb.BLOCKS))
def test_commit_then_inference_equals_the_oracle_on_the_committed_values(device, name, use_bn):
    from oracle import network_np as onp
    kind, cin, fdim = tb.BLOCKS[name]
    V, feats, R = tb.block_case(name, use_bn)
    cfg, radius = tb.make_config(use_bn)
    vs = _store(name, use_bn, device)
    f = torch.from_numpy(feats).to(device)
    before = _forward(name, vs, cfg, radius, f, device, training=False).clone()          # (also makes the folded / stacked copies)
    out = _forward(name, vs, cfg, radius, f.clone().requires_grad_(True), device)
    (out * torch.from_numpy(R).to(device)).sum().backward()
    with torch.no_grad():
        for p in vs.parameters().values():
            p.sub_(0.01 * p.grad)                                                          # one plain gradient step on the device
    vs.commit()
    changed = [k for k in V if not np.array_equal(vs.values[k], V[k])]
    assert set(changed) == set(vs.parameters()) | {k for k in V if "moving_" in k}
    after = _forward(name, vs, cfg, radius, f, device, training=False)
    geo = tb.geometry()
    inputs = dict(points=[geo.points], neighbors=[geo.neighbors])
    want = getattr(onp, kind + "_block")(0, inputs, torch.from_numpy(feats), radius, fdim, cfg, vs.values, tb.scope_of(name)).numpy()
    assert not torch.equal(before, after)
    assert np.abs(after.cpu().numpy() - want).max() <= 1e-4


def test_what_is_not_built_still_raises(device):
    from d3feat_amd import ops
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import VariableStore
    cfg, radius = tb.make_config(True)
    f = torch.from_numpy(tb.block_case("resnetb_shortcut", True)[1]).to(device)
    for block, word in (("resnetb_strided", "max pooling"), ("resnetb_deformable", "deformable"),
                        ("resnetb_deformable_strided", "deformable")):
        vs = VariableStore(seed=1, device=device)
        with pytest.raises(NotImplementedError, match=word):
            _forward("resnetb_shortcut", vs, cfg, radius, f, device, block=block)
    geo = tb.geometry()
    up = ops.UpsampleCat(f, torch.from_numpy(geo.neighbors).to(device), f)
    with pytest.raises(NotImplementedError, match="upsample"):
        _forward("unary", VariableStore(seed=1, device=device), cfg, radius, up, device)
    with ops.bf16_contraction(features=True):
        with pytest.raises(NotImplementedError, match="bf16"):
            _forward("unary", VariableStore(seed=1, device=device), cfg, radius, f, device)
    with pytest.raises(NotImplementedError, match="bf16"):
        _forward("unary", VariableStore(seed=1, device=device), cfg, radius, f.to(torch.bfloat16), device)
