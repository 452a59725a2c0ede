"""The float64 restatement the device tests hold the kernels to (tests/bn_grad_np.py, tests/training_blocks_np.py), pinned on the CPU:
against float64 torch autograd of a line-by-line torch restatement of tf.layers.batch_normalization(training=True) -- nn.moments with
the stop-gradient on the mean inside the variance, nn.batch_normalization's factoring, then the add and leaky_relu --, against central
difference quotients of its own forward, the moving update against TF's three fp32 operations, and a whole resnetb block against
autograd of the same composition.  The reference cannot emit training-mode numbers (no TensorFlow; the eager shim refuses
training=True): what is pinned is the definition, as for the other gradients.

Agreement is held to 1e-12 of the largest entry -- or of the largest TERM where the output cancels (a constant column: xhat is exactly 0
in one factoring and a rounding of x inv - mean inv in the other): bn_grad_np.term_scales.
"""
import numpy as np
import pytest
import torch

import bn_grad_np as bg
import training_blocks_np as tb


@pytest.mark.parametrize("name", list(bg.GRID))
def test_definition_against_float64_autograd(name):
    c = bg.grid_case(name)
    fw, bw = bg.grid_reference(name)
    want = bg.torch_gradients(c)
    scales = bg.term_scales(c, fw, bw)
    got = dict(bw, y=fw["y"])
    for out in bg.OUTPUTS:
        if want[out] is None:
            assert got[out] is None or c.residual is None
            continue
        bar = 1e-12 * max(np.abs(want[out]).max(), scales[out])
        assert np.abs(got[out] - want[out]).max() <= bar, (name, out)


def test_moments_are_two_pass_and_biased():
    c = bg.grid_case("offset")
    fw, _ = bg.grid_reference("offset")
    x = torch.tensor(c.x, dtype=torch.float64)
    _, mean, var = bg.torch_batch_norm_training(x, torch.ones(c.C, dtype=torch.float64), torch.zeros(c.C, dtype=torch.float64))
    assert np.abs(mean.numpy() - fw["mean"]).max() <= 1e-12 * np.abs(fw["mean"]).max()
    assert (np.abs(var.numpy() - fw["var"]) <= 1e-9 * fw["var"]).all()
    assert np.allclose(fw["var"], c.x.astype(np.float64).var(0, ddof=0), rtol=1e-9)              # no Bessel correction


@pytest.mark.parametrize("form", ["bn", "offset"])
def test_backward_against_difference_quotients(form):
    rng = np.random.default_rng(4)
    n, C, h = 7, 3, 1e-6
    x, res, gy = rng.standard_normal((n, C)), rng.standard_normal((n, C)), rng.standard_normal((n, C))
    gamma = rng.uniform(0.5, 1.5, C) if form == "bn" else None
    beta = rng.standard_normal(C)

    def loss(x, gamma, beta, res):
        return (bg.forward(x, gamma, beta, bg.EPS, res, True)["y"] * gy).sum()
    fw = bg.forward(x, gamma, beta, bg.EPS, res, True)
    assert np.abs(fw["z"]).min() > 1e-3                                                          # no mask flips inside the step
    bw = bg.backward(fw, gy, gamma, True)

    def quotient(arg, i):
        args = [np.array(a, np.float64) if a is not None else None for a in (x, gamma, beta, res)]
        hi, lo = [a.copy() if a is not None else None for a in args], [a.copy() if a is not None else None for a in args]
        hi[arg][i] += h
        lo[arg][i] -= h
        return (loss(*hi) - loss(*lo)) / (2 * h)
    for arg, grad in ((0, bw["gx"]), (1, bw["ggamma"]), (2, bw["gbeta"]), (3, bw["gres"])):
        if grad is None:
            continue
        for i in np.ndindex(grad.shape):
            assert abs(quotient(arg, i) - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])), (arg, i)


def test_unary_backward_against_autograd():
    rng = np.random.default_rng(5)
    x, W, gy = rng.standard_normal((9, 5)), rng.standard_normal((5, 3)), rng.standard_normal((9, 3))
    xt, Wt = torch.tensor(x, requires_grad=True), torch.tensor(W, requires_grad=True)
    ((xt @ Wt) * torch.tensor(gy)).sum().backward()
    gx, gW = bg.unary_backward(x, W, gy)
    assert np.abs(gx - xt.grad.numpy()).max() <= 1e-12 and np.abs(gW - Wt.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("momentum", [0.98, 0.99])
def test_moving_update_is_tf_s_three_fp32_operations(momentum):
    """assign_moving_average: variable - (variable - value) * decay with decay = float32(1 - momentum), every operation in fp32."""
    rng = np.random.default_rng(6)
    moving, batch = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
    decay = torch.tensor(1.0 - float(np.float32(momentum)), dtype=torch.float64).to(torch.float32)
    m, b = torch.from_numpy(moving), torch.from_numpy(batch)
    want = m - (m - b) * decay
    got = bg.moving_update(moving, batch, momentum)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    fused = (moving.astype(np.float64) - (moving.astype(np.float64) - batch) * np.float64(decay.item())).astype(np.float32)
    assert not np.array_equal(fused.view(np.uint32), got.view(np.uint32))                       # the roundings in between are part of it


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("name", list(tb.BLOCKS))
def test_blocks_against_float64_autograd(name, use_bn):
    """unary, simple and both resnetb blocks restated from bn_grad_np + kpconv_grad_np + matmul against autograd of the same composition."""
    ref, want = tb.reference(name, use_bn), tb.torch_reference(name, use_bn)
    assert set(ref["grads"]) == set(want["grads"])
    for label, a, b in [("out", ref["out"], want["out"]), ("gfeat", ref["gfeat"], want["gfeat"])] + \
            [(k, ref["grads"][k], want["grads"][k]) for k in want["grads"]]:
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0), (name, label)
    assert len(ref["moving"]) == (2 * sum(k.endswith("gamma") for k in ref["grads"]))
