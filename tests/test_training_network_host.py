"""The shared case of the training-mode network tests (tests/training_network_np.py) without a GPU: the fixture and the condition on the
case (the head's and the loss's margins included), the float64 numpy tape against float64 torch autograd to 1e-12, the float32
yardstick, and training.MomentumSGD against the float64 statement of the trainer's update."""
import os

import numpy as np
import pytest
import torch

import training_network_np as tn
from conftest import GOLDEN

TAG = {True: "bn", False: "off"}


@pytest.fixture(scope="module")
def golden():
    path = os.path.join(GOLDEN, "training_network.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    return {k: float(z[k]) for k in z.files}


def test_geometry_is_the_smallest_at_which_every_level_boundary_is_real():
    g, cfg = tn.geometry(), tn.config(True)
    assert cfg.num_layers == 3 and [b for b in cfg.architecture if "strided" in b or "upsample" in b] == ["resnetb_strided"] * 2 + ["nearest_upsample"] * 2
    n = [len(p) for p in g["points"]]
    assert g["stack_lengths"].tolist() == [300, 260] and n[0] == 560 and 100 < n[1] < n[0] and 20 < n[2] < n[1]
    for key, rows, named in (("neighbors", n, n), ("pools", n[1:], n[:2]), ("upsamples", n[:2], n[1:])):
        for m, r, s in zip(g[key], rows, named):
            assert m.shape[0] == r and (m >= s).any() and (m < s).any(), key
    assert len(g["anc"]) == len(g["pos"]) == tn.PAIRS == cfg.keypts_num
    assert (g["anc"] < 300).all() and (g["pos"] >= 300).all() and len(set(g["anc"].tolist())) < tn.PAIRS       # drawn with replacement


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_condition_on_the_case(golden, use_bn):
    """Every discrete decision of the float64 evaluation has a margin of at least 100 times the float32-CPU-against-float64 deviation of
    the quantity it is taken on, at the recorded seed (not an exclusion from any comparison: the seed was searched for it)."""
    tag = TAG[use_bn]
    assert tn.WEIGHT_SEEDS[use_bn] == int(golden["seed/" + tag])
    r, r32 = tn.run(use_bn), tn.run(use_bn, "float32")
    kinds = set()
    for k, m in r["margins"].items():
        dev = tn.margin_deviation(m, r32["margins"][k])
        assert np.isclose(m, golden["margin/%s/%s" % (tag, k)], rtol=1e-9), k
        assert m > 0 and m >= 100 * dev and m >= 100 * golden["deviation/%s/%s" % (tag, k)], (k, m, dev)
        kinds.add(k.split()[0])
    assert kinds == {"leaky", "rowsum", "pool", "head", "loss"} and sum(k.startswith("pool") for k in r["margins"]) == 2
    assert {k for k in r["margins"] if k.startswith(("head", "loss"))} == {"head " + k for k in tn.HEAD_MARGINS} | {"loss " + k for k in tn.LOSS_MARGINS}
    # the losses are real ones: the pair is not under the skip rule, the score path carries a gradient, every variable gets one
    assert r["desc_loss"] > 0.1 and abs(r["det_loss"]) > 1e-3 and r["regularization_loss"] > 0
    assert np.isclose(r["loss"], r["desc_loss"] + r["det_loss"] + r["regularization_loss"], rtol=1e-12)
    assert set(r["grads"]) == {k for k in tn.variables(use_bn) if tn.trainable(k)}
    assert all(np.abs(g).max() > 0 for g in r["grads"].values())
    assert len(r["moving"]) == (2 * sum(k.endswith("gamma") for k in r["grads"]))


def _close(label, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, label
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (label, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_numpy_tape_against_torch_float64_autograd(use_bn):
    """The float64 numpy tape composed from bn_grad_np, kpconv_grad_np, pool_grad_np, head_grad_np and loss_grad_np against float64
    torch autograd of the composition of their torch restatements, 1e-12 of each tensor's largest entry: output features and scores,
    the three losses and their sum, the gradient of every variable, the updated moving statistics, and the parameters after one
    MomentumSGD step at a grad_clip_norm that clips some variables and not others."""
    T, r = tn.tape(use_bn), tn.run(use_bn)
    for k in ("desc", "score", "desc_loss", "det_loss", "regularization_loss", "loss"):
        _close(k, T[k], r[k])
    assert set(T["grads"]) == set(r["grads"]) and set(T["moving"]) == set(r["moving"])
    for k in r["grads"]:
        _close(k + " grad", T["grads"][k], r["grads"][k])
    for k in r["moving"]:
        _close(k, T["moving"][k], r["moving"][k])
    V = tn.variables(use_bn)
    clip = tn.clip_norm(r["grads"])
    stepped, clipped = tn.momentum_step(V, T["grads"], tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    assert any(clipped.values()) and not all(clipped.values())
    leaves = {k: torch.tensor(V[k], dtype=torch.float64, requires_grad=True) for k in r["grads"]}
    for k, p in leaves.items():                                    # the update written out in torch on the autograd gradients
        g = torch.tensor(r["grads"][k])
        g = g * clip / torch.maximum(torch.linalg.vector_norm(g), torch.tensor(clip, dtype=torch.float64))
        _close(k + " after the step", stepped[k], (p.detach() - tn.LEARNING_RATE * (tn.SGD_MOMENTUM * 0.0 + g)).numpy())
    for widen in (True, False):
        a, b = tn.tape_strided(use_bn, widen), tn.strided(use_bn, widen)
        for k in ("out", "gfeat"):
            _close(k, a[k], b[k])
        assert set(a["grads"]) == set(b["grads"]) and set(a["moving"]) == set(b["moving"])
        for k in b["grads"]:
            _close(k + " grad", a["grads"][k], b["grads"][k])
        for k in b["moving"]:
            _close(k, a["moving"][k], b["moving"][k])


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_float32_yardstick_is_of_the_recorded_size(golden, use_bn):
    """The float32 CPU evaluation deviates from float64 by what the fixture records, up to the run-to-run freedom of a float32 sum
    (another BLAS, another thread count): a factor of four, plus 2^-22 of the largest entry where the record is smaller than that."""
    tag = TAG[use_bn]
    r, r32 = tn.run(use_bn), tn.run(use_bn, "float32")
    for k, want in r["grads"].items():
        dev, big = np.abs(r32["grads"][k] - want).max(), np.abs(want).max()
        assert dev <= 4 * golden["err32/net/%s/grad/%s" % (tag, k)] + 2.0 ** -22 * big, k
    for k in ("desc", "score"):
        assert np.abs(r32[k] - r[k]).max() <= 4 * golden["err32/net/%s/%s" % (tag, k)] + 2.0 ** -22 * np.abs(r[k]).max()
    for widen in (True, False):
        s, s32 = tn.strided(use_bn, widen), tn.strided(use_bn, widen, "float32")
        key = "err32/strided/%s/%s/" % (tag, "widen" if widen else "same")
        assert ("layer_0/resnetb_strided_0/shortcut/weights" in s["grads"]) == widen
        for k in ("out", "gfeat"):
            assert np.abs(s32[k] - s[k]).max() <= 4 * golden[key + k] + 2.0 ** -22 * np.abs(s[k]).max()
        assert all(m >= 100 * abs(m - s32["margins"][n]) for n, m in s["margins"].items())


class _Store:
    """What MomentumSGD asks of a VariableStore."""

    def __init__(self, V):
        self.leaves = {k: torch.tensor(v, dtype=torch.float32, requires_grad=True) for k, v in V.items()}
        self.commits = 0

    def parameters(self):
        return dict(self.leaves)

    def commit(self):
        self.commits += 1


def test_momentum_sgd_against_the_float64_update():
    """Two steps on the CPU leaves of the shared case with the float64 gradients rounded to float32: per-variable clipping at a norm
    between the gradient norms (some variables clipped, some not), the accumulator, the update, commit on request."""
    from d3feat_amd.training import MomentumSGD
    r = tn.run(True)
    V = {k: v for k, v in tn.variables(True).items() if tn.trainable(k)}
    clip = tn.clip_norm(r["grads"])
    want, clipped = tn.momentum_step(V, r["grads"], tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    assert any(clipped.values()) and not all(clipped.values())
    store = _Store(V)
    opt = MomentumSGD(store, tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    for k, p in store.leaves.items():
        p.grad = torch.tensor(r["grads"][k], dtype=torch.float32)
    assert set(opt.step()) == set(V) and store.commits == 0
    for k, p in store.leaves.items():
        big = max(np.abs(want[k]).max(), tn.LEARNING_RATE * clip)
        assert np.abs(p.detach().double().numpy() - want[k]).max() <= 8 * 2.0 ** -24 * big, k
    # a second step with the same gradients: accum = (1 + momentum) g
    opt.step(commit=True)
    assert store.commits == 1
    for k, p in store.leaves.items():
        g = (np.asarray(V[k], np.float64) - want[k]) / tn.LEARNING_RATE
        second = want[k] - tn.LEARNING_RATE * (1 + tn.SGD_MOMENTUM) * g
        assert np.abs(p.detach().double().numpy() - second).max() <= 16 * 2.0 ** -24 * max(np.abs(second).max(), tn.LEARNING_RATE * clip), k
    # without clipping, and a leaf without a gradient is left alone
    store = _Store(V)
    opt = MomentumSGD(store, 0.5, 0.9, 0.0)
    first = next(iter(V))
    store.leaves[first].grad = torch.ones_like(store.leaves[first]) * 1000
    assert opt.step() == [first]
    assert np.allclose(store.leaves[first].detach().numpy(), V[first] - 500.0)
    assert all(np.array_equal(p.detach().numpy(), V[k]) for k, p in store.leaves.items() if k != first)
