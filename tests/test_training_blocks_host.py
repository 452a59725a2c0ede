"""The variable store's training bookkeeping on the CPU device (parameter / parameters / commit), and the variables the training-mode
blocks create: names, shapes, order and -- from the same seed -- values equal build_variables's.  The device operators are replaced by
shape-only stand-ins here; tests/test_gpu_training_blocks.py runs the real ones."""
import numpy as np
import pytest
import torch

from d3feat_amd.models import network_blocks as nb
from d3feat_amd.models.variables import VariableStore, build_variables
from d3feat_amd.utils.config import threedmatch_config


def _store():
    vs = VariableStore(seed=3, device=torch.device("cpu"))
    with vs.variable_scope("layer_0/unary_0"):
        w = vs.weight_variable([4, 8])
        bn = vs.batch_norm_variables(8)
    return vs, w, bn


def test_parameter_is_a_cached_leaf_on_the_storage_of_the_device_copy():
    vs, w, bn = _store()
    assert vs.parameters() == {}
    p = vs.parameter(w)
    assert p is vs.parameter(w) and p.requires_grad and p.is_leaf
    assert p.data_ptr() == vs.tensor(w).data_ptr() and not vs.tensor(w).requires_grad
    g = vs.parameter(bn[0])
    assert list(vs.parameters()) == [w, bn[0]] and vs.parameters()[bn[0]] is g
    version = vs.tensor(w)._version
    with torch.no_grad():
        p.add_(1.0)
    assert vs.tensor(w)._version > version                                   # packed copies are keyed on it
    assert np.array_equal(vs.tensor(w).numpy(), vs.values[w] + 1.0)
    (p.sum() * 2).backward()
    assert torch.equal(p.grad, torch.full((4, 8), 2.0))
    vs.invalidate_device()
    assert vs.parameters() == {}


def test_commit_copies_back_and_rederives_the_folded_copies():
    vs, w, bn = _store()
    scale, shift = vs.folded_bn(bn)
    addr = (scale.data_ptr(), shift.data_ptr(), vs.tensor(w).data_ptr())
    old = {k: v.copy() for k, v in vs.values.items()}
    with torch.no_grad():
        vs.parameter(w).mul_(0.5)
        vs.parameter(bn[0]).add_(0.25)                                       # gamma
        vs.tensor(bn[2]).add_(0.125)                                         # moving_mean, as a training forward updates it
        vs.tensor(bn[3]).mul_(2.0)                                           # moving_variance
    touched = vs.commit()
    assert np.array_equal(vs.values[w], old[w] * 0.5) and np.array_equal(vs.values[bn[0]], old[bn[0]] + 0.25)
    assert np.array_equal(vs.values[bn[1]], old[bn[1]])
    assert np.array_equal(vs.values[bn[2]], old[bn[2]] + 0.125) and np.array_equal(vs.values[bn[3]], old[bn[3]] * 2.0)
    want_scale, want_shift = vs._bn_host(bn, 1e-6)
    assert np.array_equal(scale.numpy(), want_scale) and np.array_equal(shift.numpy(), want_shift)     # in place: the same tensors
    assert (scale.data_ptr(), shift.data_ptr(), vs.tensor(w).data_ptr()) == addr
    assert any(t is scale for t in touched) and vs.parameter(w).requires_grad


@pytest.mark.parametrize("use_bn", [True, False])
def test_training_blocks_create_the_variables_of_build_variables(monkeypatch, use_bn):
    cfg = threedmatch_config()
    cfg.architecture = ["simple", "resnetb", "resnetb", "unary"]
    cfg.first_features_dim, cfg.in_features_dim, cfg.num_layers = 8, 1, 1
    cfg.use_batch_norm = use_bn
    want = build_variables(cfg, seed=11)
    calls = []

    def unary(x, W):
        assert W.requires_grad and W.is_leaf
        calls.append("unary")
        return x.detach() @ W.detach()

    def kpconv(q, s, idx, f, K_points, W, extent, influence, mode):
        assert W.requires_grad and np.asarray(K_points).shape == (cfg.num_kernel_points, 3)
        calls.append("kpconv")
        return torch.zeros((q.shape[0], W.shape[2]))

    def bn(x, gamma, beta, residual=None, leaky=False, alpha=0.2, moving_mean=None, moving_variance=None, momentum=0.99, eps=1e-6):
        assert (gamma is not None) == use_bn and beta.requires_grad and (gamma is None or momentum == cfg.batch_norm_momentum)
        assert (moving_mean is not None) == use_bn and (moving_mean is None or not moving_mean.requires_grad)
        assert residual is None or residual.shape == x.shape
        calls.append("bn+res" if residual is not None else "bn")
        return x
    monkeypatch.setattr(nb, "unary_trainable", unary)
    monkeypatch.setattr(nb, "kpconv_trainable", kpconv)
    monkeypatch.setattr(nb, "batch_norm_trainable", bn)
    vs = VariableStore(seed=11, device=torch.device("cpu"))
    pts = torch.rand(20, 3)
    inputs = dict(points=[pts], neighbors=[torch.zeros((20, 5), dtype=torch.int32)], features=torch.ones(20, 1))
    with nb.use_variables(vs):
        F = nb.assemble_CNN_blocks(inputs, cfg, dropout_prob=0.5)            # dropout_prob < 0.99: training
    assert F == []
    assert list(vs.values) == list(want.values)                              # names in creation order
    for k in want.values:
        assert vs.values[k].shape == want.values[k].shape and np.array_equal(vs.values[k], want.values[k]), k
    trainable = [k for k in want.values if not k.endswith(("kernel_points", "moving_mean", "moving_variance"))]
    assert sorted(vs.parameters()) == sorted(trainable)
    # simple; resnetb 8 -> 16 with a shortcut convolution; resnetb 16 -> 16 with the identity; unary
    first = ["unary", "bn", "kpconv", "bn", "unary", "bn", "unary", "bn+res"]
    assert calls == ["kpconv", "bn"] + first + ["unary", "bn", "kpconv", "bn", "unary", "bn+res"] + ["unary", "bn"]
