"""The training-mode network on the GPU at every configuration value of tests/training_network_np.CASES, and the default configuration
over three optimiser steps, against the float64 reference of tests/training_network_np.py: the configuration cases against its numpy
tape, the step cases against trajectory() -- float64 torch autograd of the same composition threaded through the optimiser -- which
tests/test_training_config_host.py holds against the tape to 1e-12 at every step.  All on the geometry of the shared case (560 / 189 /
59 rows, 64 index pairs).

Per configuration case, one model.run() and one model.backward() through KernelPointFCNN: descriptors, scores, the four losses, the
gradient of every variable, every moving statistic; and, by a spy on the operators, that every KPConv (forward and backward) received the
case's influence, aggregation, kernel-point count and the extent of its level, every batch norm the case's momentum, the loss the
case's safe_radius, keypts_num and det_loss_weight, and that none of the fused inference forms ran.  tests/test_training_config_host.py
shows that each changed setting moves a compared tensor by at least 100 tolerances, so a device path that ignored it fails here.

steps_bn / steps_off: three rounds of run(), backward(), MomentumSGD.step() (commit at the third only).  At every step the losses, every
gradient, every moving statistic, every accumulator and every parameter after the update; after the third the host masters equal the
device tensors bit for bit, the inference forward is within 1e-4 of the float32 oracle on the committed values, a fresh model built from
model.weights() gives the same inference bits, and two fresh models taken through the same steps agree bit for bit in everything.

Tolerance per tensor, the rule of test_gpu_training_network._held on tests/golden/training_configs.npz: the larger of 4 * err32 and
(560 + 16) * 2^-24 of the largest entry, capped at 1e-4 of the largest entry, 4 * err32 where that exceeds the cap.  Accumulators:
sum_j momentum^(k - j) tol_g(j); parameters: 2 lr times the sum of the accumulator tolerances so far, plus 4 * 2^-24 of the largest entry.

What the module catches (each a local edit tried once on an MI355X, never committed; the tests named failed, the others passed):
  network_blocks._kpconv_train passing 'linear', 'sum' whatever the config    test_configuration_against_float64[gaussian, closest,
                                                                              class_defaults, mixed]
  network_blocks._bn_train passing 0.99                                       every case with batch norm (9 configuration cases, steps_bn)
  MomentumSGD.step without a.mul_(self.momentum)                              test_three_steps_against_float64[steps_bn, steps_off]
  KernelPointFCNN.backward() without clearing .grad                           test_three_steps_against_float64[steps_bn, steps_off]
  VariableStore.commit() skipping the moving statistics                       test_three_steps_against_float64[steps_bn]
With the code as it is every test passes: no defect found.

Measured on an MI355X (printed, never used as a bar): the largest deviation of any compared tensor as a fraction of its largest entry,
and the worst deviation / tolerance with the tensor that has it.
  gaussian        1.4e-5   0.40  gradient of layer_0/resnetb_1/conv2/batch_normalization/gamma
  closest         3.9e-6   0.12  gradient of layer_0/simple_0/batch_normalization/beta
  class_defaults  8.3e-5   0.44  gradient of layer_2/resnetb_0/conv1/offset
  kp13            2.0e-5   0.59  gradient of layer_0/resnetb_strided_2/conv1/batch_normalization/gamma
  kp4             1.6e-5   0.47  gradient of layer_0/resnetb_1/conv1/batch_normalization/gamma
  geometry        2.7e-5   0.66  gradient of layer_0/resnetb_strided_2/conv1/batch_normalization/gamma
  w18             7.2e-6   0.21  gradient of layer_1/resnetb_0/conv1/weights
  w16             3.1e-6   0.09  gradient of layer_1/resnetb_0/shortcut/weights
  cin4            7.9e-6   0.23  gradient of layer_1/resnetb_0/conv2/batch_normalization/gamma
  bn_momentum     2.0e-5   0.57  gradient of layer_2/resnetb_0/conv3/batch_normalization/gamma
  loss_values     1.1e-5   0.32  gradient of layer_2/resnetb_0/shortcut/weights
  mixed           2.0e-5   0.58  gradient of layer_0/resnetb_strided_2/conv1/offset
  steps_bn, steps 1 / 2 / 3: gradients 1.6e-5 / 1.4e-5 / 4.4e-5 (0.42 / 0.38 / 0.38 of the tolerance), accumulators 1.6e-5 / 1.1e-5 /
                  1.7e-5 (0.42 / 0.29 / 0.24), parameters 6.5e-8 / 1.4e-7 / 2.4e-7 (0.17 / 0.26 / 0.26), moving statistics 2.8e-7 at
                  most (0.01), descriptors 2.8e-6 (0.08), scores 2.6e-6 (0.08), the four losses 1.5e-7 at most; the inference forward
                  after the third step within 6.0e-7 of the float32 oracle
  steps_off, steps 1 / 2 / 3: gradients 2.6e-6 / 2.8e-6 / 8.1e-6 (0.07 / 0.08 / 0.24), accumulators 2.6e-6 / 1.9e-6 / 1.6e-6 (0.07 /
                  0.05 / 0.03), parameters 6.6e-8 / 1.0e-7 / 1.2e-7 (0.16 / 0.21 / 0.28), descriptors 6.0e-7 (0.02), scores 3.9e-7
                  (0.01), the four losses 3.8e-7 at most (0.01); the inference forward within 3.0e-7 of the float32 oracle
Every bit-for-bit comparison holds.  The 14 tests take 4 s (steps_bn 1.9 s, the first case 0.6 s, the others under 0.2 s each).
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import network_config_cases as nc
import training_network_np as tn
from conftest import GOLDEN, bits
from test_gpu_training_network import _flat

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SCALARS = ("desc_loss", "det_loss", "regularization_loss", "loss")
FUSED = ("gemm_upsample_split", "gemm_chain", "gemm_cat2", "gemm_upsample_cat")
CONFIG_CASES = [c for c in tn.CASES if c not in tn.STEP_RATES]


@pytest.fixture(scope="module")
def golden():
    return tn.load_golden(os.path.join(GOLDEN, "training_configs.npz"))


class _Worst:
    def __init__(self):
        self.ratio, self.dev, self.what = 0.0, 0.0, ""

    def note(self, label, dev, tol, big):
        if dev / tol > self.ratio:
            self.ratio, self.what = dev / tol, label
        self.dev = max(self.dev, dev / max(big, 1e-300))


def _held(label, tol, got, want, worst):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    big, dev = np.abs(want).max(), np.abs(got - want).max()
    print("%s: largest %.3e, deviation %.2e of it, tolerance %.2e of it" % (label, big, dev / max(big, 1e-300), tol / max(big, 1e-300)))
    worst.note(label, dev, tol, big)
    assert dev <= tol, label


def _tol(golden, case, step, name, want):
    return tn.tolerance(golden["err32/%s/%d/%s" % (case, step, name)], np.abs(np.asarray(want, np.float64)).max())


@contextlib.contextmanager
def _spy(calls):
    """Every call of the operators below appends (name, positional arguments, keyword arguments): the entry points of d3feat_amd.ops
    the training walk and the inference path choose between, the forward the KPConv backward pairs with, and the loss."""
    from d3feat_amd import ops, validation
    from d3feat_amd.kernels import autograd
    spied = [(ops, n) for n in FUSED + ("kpconv_backward", "batch_norm_train", "batch_norm_backward", "ind_max_pool_backward",
                                        "closest_pool_cat_backward", "detect_head_backward")]
    spied += [(autograd, "KPConv_ops"), (validation, "loss_gradients")]
    orig = [(mod, n, getattr(mod, n)) for mod, n in spied]

    def wrap(name, fn):
        def run(*a, **k):
            calls.append((name, a, k))
            return fn(*a, **k)
        return run
    for mod, n, fn in orig:
        setattr(mod, n, wrap(n, fn))
    try:
        yield calls
    finally:
        for mod, n, fn in orig:
            setattr(mod, n, fn)


def _model(case, device):
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    model = KernelPointFCNN(iter(()), tn.config(case), weights={k: v.copy() for k, v in tn.variables(case).items()}, device=device)
    model.dropout_prob = 0.5
    return model


def _compare_step(golden, case, step, model, ref, worst):
    """Losses, outputs, gradients and moving statistics of one run() + backward() against the reference of that step."""
    V = tn.variables(case)
    for name in SCALARS:
        _held(name, _tol(golden, case, step, name, ref[name]), float(getattr(model, name).detach()), ref[name], worst)
    _held("descriptors", _tol(golden, case, step, "desc", ref["desc"]), model.out_features.detach().cpu().numpy(), ref["desc"], worst)
    _held("scores", _tol(golden, case, step, "score", ref["score"]), model.out_scores.detach().cpu().numpy(), ref["score"], worst)
    params = model.variables.parameters()
    assert set(params) == set(ref["grads"]) == {k for k in V if tn.trainable(k)} and set(model.weights()) == set(V)
    for k, p in params.items():
        _held(k + " grad", _tol(golden, case, step, "grad/" + k, ref["grads"][k]), p.grad.cpu().numpy(), ref["grads"][k], worst)
    assert len(ref["moving"]) == 2 * sum(k.endswith("gamma") for k in params)
    for k, want in ref["moving"].items():
        _held(k, _tol(golden, case, step, "moving/" + k, want), model.variables.tensor(k).cpu().numpy(), want, worst)


def _check_calls(case, calls):
    cfg, inp = tn.config(case), tn.geometry(case)
    rows = [len(p) for p in inp["points"]]
    per_level = {}
    for (key, l), scopes in nc.kpconv_readers(cfg).items():
        per_level[l] = per_level.get(l, 0) + len(scopes)
    by = {}
    for name, a, k in calls:
        by.setdefault(name, []).append((a, k))
    assert not set(FUSED) & set(by)
    for name, at in (("KPConv_ops", (4, 6, 7, 8)), ("kpconv_backward", (4, 7, 8, 9))):          # (K_points, extent, influence, aggregation)
        seen = {}
        for a, k in by[name]:
            assert len(a) > at[3], name
            level = rows.index(a[1].shape[0])                                                   # (the support points' level)
            seen[level] = seen.get(level, 0) + 1
            extent = cfg.KP_extent * (cfg.first_subsampling_dl * cfg.density_parameter * 2 ** level) / cfg.density_parameter
            assert a[at[0]].shape[0] == cfg.num_kernel_points and a[at[2]] == cfg.KP_influence and a[at[3]] == cfg.convolution_mode, name
            assert abs(float(a[at[1]]) - extent) <= 1e-12 * extent, (name, level, a[at[1]], extent)
        assert seen == per_level, (name, seen)
    bn = by.get("batch_norm_train", [])
    assert len(bn) == len(by["batch_norm_backward"]) > 0
    for a, k in bn:
        if a[1] is not None:
            assert a[9] == cfg.batch_norm_momentum
        assert (a[1] is not None) == cfg.use_batch_norm
    (a, k), = by["loss_gradients"]
    assert (k["safe_radius"], k["keypts_num"], k["det_loss_weight"]) == (cfg.safe_radius, cfg.keypts_num, cfg.det_loss_weight)
    L = cfg.num_layers
    assert len(by["ind_max_pool_backward"]) == len(by["closest_pool_cat_backward"]) == L - 1 and len(by["detect_head_backward"]) == 1


@pytest.mark.parametrize("case", CONFIG_CASES)
def test_configuration_against_float64(device, golden, case):
    ref = tn.tape(case)
    model = _model(case, device)
    calls, worst = [], _Worst()
    with _spy(calls):
        model.run(_flat(tn.geometry(case), device))
        model.backward()
    _compare_step(golden, case, 0, model, ref, worst)
    for k, want in ref["moving"].items():
        assert not np.array_equal(model.variables.tensor(k).cpu().numpy(), tn.variables(case)[k])
    _check_calls(case, calls)
    print("%s: worst deviation / tolerance %.3f (%s), largest deviation %.2e of the largest entry" % (case, worst.ratio, worst.what, worst.dev))


def _three_steps(case, device, golden=None, worst=None):
    """Three rounds of run(), backward(), step() on a fresh model -> (model, optimiser, [per step the compared tensors as numpy])."""
    from d3feat_amd.training import MomentumSGD
    T = tn.trajectory(case)
    lr, mom = tn.learning_rate(case), tn.SGD_MOMENTUM
    model = _model(case, device)
    opt = MomentumSGD(model.variables, lr, mom, tn.clip_norm(T[0]["grads"]))
    flat = _flat(tn.geometry(case), device)
    record, tol_a, tol_p = [], {}, {}
    for step in range(tn.STEPS):
        ref = T[step]
        model.run(flat)
        params = model.backward()
        rec = {n: float(getattr(model, n).detach()) for n in SCALARS}
        rec.update(desc=model.out_features.detach().cpu().numpy(), score=model.out_scores.detach().cpu().numpy())
        rec.update({"grad/" + k: p.grad.cpu().numpy().copy() for k, p in params.items()})
        rec.update({"moving/" + k: model.variables.tensor(k).cpu().numpy().copy() for k in ref["moving"]})
        if golden is not None:
            _compare_step(golden, case, step, model, ref, worst)
        before = {k: model.variables.values[k].copy() for k in params}
        assert set(opt.step(commit=step == tn.STEPS - 1)) == set(ref["grads"])
        rec.update({"accum/" + k: opt.accum[k].cpu().numpy().copy() for k in params})
        rec.update({"param/" + k: p.detach().cpu().numpy().copy() for k, p in params.items()})
        record.append(rec)
        if golden is None:
            continue
        for k in params:
            # the clipped gradient is within the gradient's own tolerance (clipping only shrinks it); the accumulator carries the
            # earlier ones scaled by the momentum; the parameter every accumulator so far, and the rounding of the float32 value
            tol_a[k] = mom * tol_a.get(k, 0.0) + _tol(golden, case, step, "grad/" + k, ref["grads"][k])
            tol_p[k] = tol_p.get(k, 0.0) + tol_a[k]
            _held(k + " accumulator", tol_a[k], rec["accum/" + k], ref["accum"][k], worst)
            _held(k + " after step %d" % (step + 1), 2 * lr * tol_p[k] + 4 * U * np.abs(ref["param"][k]).max(), rec["param/" + k],
                  ref["param"][k], worst)
            committed = np.array_equal(model.variables.values[k], rec["param/" + k])
            assert committed == (step == tn.STEPS - 1) and (committed or np.array_equal(model.variables.values[k], before[k])), k
    return model, opt, record


@pytest.mark.parametrize("case", sorted(tn.STEP_RATES))
def test_three_steps_against_float64(device, golden, case):
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from oracle import network_np as onp
    worst = _Worst()
    model, opt, record = _three_steps(case, device, golden, worst)
    print("%s: worst deviation / tolerance %.3f (%s), largest deviation %.2e of the largest entry" % (case, worst.ratio, worst.what, worst.dev))
    # commit(): every host master is the device tensor, moving statistics included
    for k in model.weights():
        assert np.array_equal(bits(model.variables.values[k]), bits(model.variables.tensor(k).cpu().numpy())), k
    for k in tn.trajectory(case)[0]["moving"]:
        assert not np.array_equal(model.variables.values[k], tn.variables(case)[k])
    # the inference forward of the trained model: the float32 oracle on the committed values, and a fresh model built from them
    inp = tn.geometry(case)
    flat = _flat(inp, device)
    model.dropout_prob = 1.0
    d, s = model.run(flat)
    assert model.loss is None and not d.requires_grad
    want_d, want_s = onp.forward(model.config, model.variables.values, inp)
    ed, es = np.abs(d.cpu().numpy() - want_d).max(), np.abs(s.cpu().numpy() - want_s).max()
    print("inference after three steps: descriptors %.2e, scores %.2e" % (ed, es))
    assert ed <= 1e-4 and es <= 1e-4
    fresh = KernelPointFCNN(iter(()), tn.config(case), weights={k: v.copy() for k, v in model.weights().items()}, device=device)
    d2, s2 = fresh.run(flat)
    assert np.array_equal(bits(d.cpu().numpy()), bits(d2.cpu().numpy())) and np.array_equal(bits(s.cpu().numpy()), bits(s2.cpu().numpy()))
    # a second fresh model through the same three steps: every compared tensor, bit for bit
    _, _, again = _three_steps(case, device)
    for step, (a, b) in enumerate(zip(record, again)):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(bits(np.asarray(a[k], np.float32)), bits(np.asarray(b[k], np.float32))), (step, k)
