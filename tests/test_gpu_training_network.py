"""The training-mode network on the GPU against the float64 numpy tape of tests/training_network_np.py (composed from bn_grad_np,
kpconv_grad_np, pool_grad_np, head_grad_np and loss_grad_np, and held against float64 torch autograd to 1e-12 by
tests/test_training_network_host.py), on the shared case: two clouds of 300 + 260 points, three levels (two strided blocks, two
upsamplings), first_features_dim 8, 15 kernel points, 64 index pairs, with batch norm and without.

One resnetb_strided block inside network_blocks.training_walk() (with and without a width change): output, input gradient, every
parameter gradient, moving statistics.  The whole KernelPointFCNN at dropout_prob = 0.5: descriptors, scores, desc_loss, det_loss,
regularization_loss, loss, the gradient of every variable, every moving statistic, the parameters after one MomentumSGD step, the
inference forward after commit(), and which operators ran.

Tolerance per compared tensor, the project's rule: the larger of 4 * err32 (tests/golden/training_network.npz: float32 torch-CPU
autograd of the same composition against float64) and (L + 16) * 2^-24 of the largest entry, L = 560 (the rows of the finest level: the
longest sum any entry ends), capped at 1e-4 of the largest entry -- except where 4 * err32 itself exceeds that cap, where the bar is
4 * err32 (network_config_cases.bar) -- which happens for no tensor of this case (the largest 4 * err32 is 5.6e-5 of the largest entry).

Measured on an MI355X (printed, never used as a bar), as fractions of each tensor's largest entry.  Strided block: output 5.0e-7, input
gradient 1.4e-7, at most 0.015 of the tolerance.  Whole model: descriptors 5.9e-6 (0.17 of the tolerance), scores 1.9e-6, desc_loss
7.7e-8, det_loss 1.9e-7, regularization_loss 3.5e-8, loss 8.7e-8; the largest parameter gradient deviation 2.0e-5 with batch norm
(layer_2/resnetb_0/conv3/batch_normalization/gamma, 0.57 of its tolerance) and 1.3e-5 without; moving statistics 1.1e-7 (0.19 of the
tolerance); the inference forward after commit() within 9.5e-7 of the float32 oracle.  The 8 tests take 2 s.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import training_network_np as tn
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TERMS = 560
TAG = {True: "bn", False: "off"}


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "training_network.npz"))
    return {k: float(z[k]) for k in z.files}


def _held(label, err32, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    big = np.abs(want).max()
    tol = max(min(max(4 * err32, (TERMS + 16) * U * big), 1e-4 * big), 4 * err32)
    dev = np.abs(got - want).max()
    print("%s: largest %.3e, deviation %.2e of it, tolerance %.2e of it" % (label, big, dev / max(big, 1e-300), tol / max(big, 1e-300)))
    assert dev <= tol, label
    return dev / max(big, 1e-300)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _flat(inp, device):
    """The positional list of datasets/common.py:1410-1413 + the dataset tail, with the keypoint indices on the device."""
    flat = [_dev(p, device) for p in inp["points"]] + [_dev(m, device) for m in inp["neighbors"]]
    flat += [_dev(m, device) for m in inp["pools"]] + [_dev(m, device) for m in inp["upsamples"]]
    flat += [_dev(inp["features"], device), _dev(inp["batch_weights"], device), _dev(inp["in_batches"], device), _dev(inp["out_batches"], device)]
    flat += [_dev(inp["stack_lengths"], device), _dev(inp["anc"], device), _dev(inp["pos"], device), ["a", "b"], _dev(inp["points"][0], device)]
    return flat


SPIED = ("ind_max_pool", "ind_max_pool_backward", "closest_pool_cat", "closest_pool_cat_backward", "gemm_upsample_split", "gemm_chain",
         "gemm_cat2", "gemm_upsample_cat", "detect_head_backward", "kpconv_backward", "batch_norm_backward")


@contextlib.contextmanager
def _spy(calls):
    """Every call of the named entry points of d3feat_amd.ops appends its name (the manner of network_config_cases.spy_ops)."""
    from d3feat_amd import ops
    orig = {n: getattr(ops, n) for n in SPIED}

    def wrap(name):
        def run(*a, **k):
            calls.append(name)
            return orig[name](*a, **k)
        return run
    for n in SPIED:
        setattr(ops, n, wrap(n))
    try:
        yield calls
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)


@pytest.mark.parametrize("widen", [True, False], ids=["widen", "same"])
@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_strided_block_against_float64(device, golden, use_bn, widen):
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import VariableStore
    cfg, inp = tn.config(use_bn), tn.geometry()
    V, feats, R, fdim = tn.strided_case(use_bn, widen)
    ref = tn.tape_strided(use_bn, widen)
    vs = VariableStore(values=V, device=device, create=False)
    inputs = dict(points=[_dev(p, device) for p in inp["points"][:2]], neighbors=[_dev(inp["neighbors"][0], device)],
                  pools=[_dev(inp["pools"][0], device)])
    f = _dev(feats, device).requires_grad_(True)
    radius = cfg.first_subsampling_dl * cfg.density_parameter
    block = nb.get_block_ops("resnetb_strided")
    with nb.use_variables(vs), nb.variable_scope(tn.STRIDED_SCOPE):
        with pytest.raises(NotImplementedError, match="max pooling"):          # outside a walk the refusal stands
            block(0, inputs, f, radius, fdim, cfg, True)
        with nb.training_walk(), nb.training_walk():                            # (re-entrant)
            out = block(0, inputs, f, radius, fdim, cfg, True)
    (out * _dev(R, device)).sum().backward()
    key = "err32/strided/%s/%s/" % (TAG[use_bn], "widen" if widen else "same")
    _held("out", golden[key + "out"], out.detach().cpu().numpy(), ref["out"])
    _held("gfeat", golden[key + "gfeat"], f.grad.cpu().numpy(), ref["gfeat"])
    params = vs.parameters()
    assert set(params) == set(ref["grads"]) and ((tn.STRIDED_SCOPE + "/shortcut/weights") in params) == widen
    for k, p in params.items():
        _held(k + " grad", golden[key + "grad/" + k], p.grad.cpu().numpy(), ref["grads"][k])
    assert len(ref["moving"]) == 2 * sum(k.endswith("gamma") for k in params)
    for k, want in ref["moving"].items():
        got = vs.tensor(k).cpu().numpy()
        assert not np.array_equal(got, V[k])
        _held(k, golden[key + "moving/" + k], got, want)


_RUNS = {}


def _model_run(use_bn, device):
    """One training-mode run + backward of the whole model, shared by the tests below."""
    if use_bn not in _RUNS:
        from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
        cfg, inp = tn.config(use_bn), tn.geometry()
        model = KernelPointFCNN(iter(()), cfg, weights=dict(tn.variables(use_bn)), device=device)
        model.dropout_prob = 0.5
        calls = []
        with _spy(calls):
            model.run(_flat(inp, device))
            model.backward()
        grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.variables.parameters().items()}
        _RUNS[use_bn] = (model, grads, calls)
    return _RUNS[use_bn]


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_whole_model_against_float64(device, golden, use_bn):
    model, grads, calls = _model_run(use_bn, device)
    ref, V = tn.tape(use_bn), tn.variables(use_bn)
    key = "err32/net/%s/" % TAG[use_bn]
    assert set(model.weights()) == set(V)                                       # the model created no variable of its own
    assert set(grads) == set(ref["grads"]) == {k for k in V if tn.trainable(k)}
    _held("descriptors", golden[key + "desc"], model.out_features.detach().cpu().numpy(), ref["desc"])
    _held("scores", golden[key + "score"], model.out_scores.detach().cpu().numpy(), ref["score"])
    for name in ("desc_loss", "det_loss", "regularization_loss", "loss"):
        _held(name, golden[key + name], float(getattr(model, name).detach()), ref[name])
    assert model.loss.requires_grad and float(model.accuracy) >= 0
    worst = 0.0
    for k in grads:
        worst = max(worst, _held(k + " grad", golden[key + "grad/" + k], grads[k], ref["grads"][k]))
    for k, want in ref["moving"].items():
        got = model.variables.tensor(k).cpu().numpy()
        assert not np.array_equal(got, V[k])
        _held(k, golden[key + "moving/" + k], got, want)
    print("largest deviation of a parameter gradient: %.2e of its largest entry" % worst)
    # routing: the two new operators once per level boundary, none of the fused inference forms
    L = model.config.num_layers
    assert calls.count("ind_max_pool") == calls.count("ind_max_pool_backward") == L - 1
    assert calls.count("closest_pool_cat") == calls.count("closest_pool_cat_backward") == L - 1
    assert calls.count("detect_head_backward") == 1
    assert not {"gemm_upsample_split", "gemm_chain", "gemm_cat2", "gemm_upsample_cat"} & set(calls)


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_momentum_step_commit_and_inference(device, golden, use_bn):
    """One MomentumSGD step from the gradients above (some variables clipped, some not), commit(), then the inference forward on the
    committed values against the float32 oracle within the project's 1e-4."""
    from d3feat_amd.training import MomentumSGD
    from oracle import network_np as onp
    model, grads, _ = _model_run(use_bn, device)
    ref, V = tn.tape(use_bn), tn.variables(use_bn)
    clip = tn.clip_norm(ref["grads"])
    want, clipped = tn.momentum_step(V, ref["grads"], tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    assert any(clipped.values()) and not all(clipped.values())
    opt = MomentumSGD(model.variables, tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    assert set(opt.step(commit=True)) == set(want)
    key = "err32/net/%s/grad/" % TAG[use_bn]
    for k, w in want.items():
        # the update is lr * g' with |g' - g'_64| within the gradient's own tolerance (clipping only shrinks it), plus the rounding of
        # the float32 parameter
        got = model.variables.tensor(k).cpu().numpy().astype(np.float64)
        big_g = np.abs(ref["grads"][k]).max()
        tol_g = max(min(max(4 * golden[key + k], (TERMS + 16) * U * big_g), 1e-4 * big_g), 4 * golden[key + k])
        assert np.abs(got - w).max() <= 2 * tn.LEARNING_RATE * tol_g + 4 * U * np.abs(w).max(), k
        assert np.array_equal(model.variables.values[k], model.variables.tensor(k).cpu().numpy())          # committed
    model.dropout_prob = 1.0
    try:
        inp = tn.geometry()
        d, s = model.run(_flat(inp, device))
        assert model.loss is None and not d.requires_grad
        want_d, want_s = onp.forward(model.config, model.variables.values, inp)
        ed, es = np.abs(d.cpu().numpy() - want_d).max(), np.abs(s.cpu().numpy() - want_s).max()
        print("inference after commit: descriptors %.2e, scores %.2e" % (ed, es))
        assert ed <= 1e-4 and es <= 1e-4
    finally:
        _RUNS.pop(use_bn, None)                                                  # (the parameters have moved)
