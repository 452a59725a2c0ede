"""The optimiser's step without a GPU: tests/optimizer_np.py's float32 restatement of d3f_momentum_sgd against training.MomentumSGD
and against its own float64 form, the host-side chunk plan, and the model's fold_regularization / backward(keep_grads=True) on the CPU
walk of tests/test_training_walk_host.py (its operators are float32 torch statements; the device call of DeviceMomentumSGD is replaced
by the restatement here and runs in tests/test_gpu_optimizer.py).

Measured here (printed, never used as a bar).  Restatement against MomentumSGD over three steps: accumulators of unclipped variables
bit-equal; accumulators at most 0.46 of their bound, variables at most 0.92 of theirs (bounds + one rounding of lr a' for torch's fused
add).  Float32 against float64: at most 0.99 of the first-order bound (a one-element variable spends its roundings in full).  Folded
gradient g_pair + wd v against the autograd one: largest difference 0 (bit-equal for every variable)."""
import numpy as np
import pytest
import torch

import optimizer_np as onp
import training_network_np as tn
from test_training_walk_host import _flat, torch_operators  # noqa: F401  (the fixture and the input list of the CPU walk)

U = onp.U
SHAPES = {"a/weights": (15, 8, 16), "a/beta": (16,), "b/weights": (37, 5), "b/gamma": (1,), "c/weights": (3, 1031)}


def _case(seed=0, big=("a/weights", "c/weights")):
    """Variables and three gradients; the variables named in `big` have gradient norms above the clip of 1.0."""
    rng = np.random.default_rng(seed)
    V = {k: rng.standard_normal(s).astype(np.float32) for k, s in SHAPES.items()}
    G = [{k: (rng.standard_normal(s) * (1.0 if k in big else 0.02 / np.sqrt(np.prod(s)))).astype(np.float32) for k, s in SHAPES.items()}
         for _ in range(3)]
    return V, G


def test_restatement_against_the_torch_class_over_three_steps():
    from d3feat_amd.models.variables import VariableStore
    from d3feat_amd.training import MomentumSGD
    V, G = _case()
    hyper = (0.05, 0.98, 1.0, 0.0)
    store = VariableStore(values=dict(V), device=torch.device("cpu"), create=False)
    params = {k: store.parameter(k) for k in V}
    opt = MomentumSGD(store, hyper[0], hyper[1], hyper[2])
    A = onp.zeros_like(V)
    worst_a = worst_v = 0.0
    for step, g in enumerate(G):
        for k, p in params.items():
            p.grad = torch.from_numpy(g[k].copy())
        # each step starts from the torch class's own state, so one step's deviation is what is bounded
        Vin = {k: p.detach().numpy().copy() for k, p in params.items()}
        Ain = {k: (opt.accum[k].numpy().copy() if k in opt.accum else A[k]) for k in V}
        case = onp.step32(Vin, g, Ain, hyper)
        assert set(opt.step()) == set(V)
        V2, A2, _, info = case
        clipped = {k for k in V if info[k]["clipped"]}
        assert clipped == {"a/weights", "c/weights"}
        for k, (ba, bv) in onp.bounds(case, hyper).items():
            da = np.abs(opt.accum[k].numpy().astype(np.float64) - A2[k])
            dv = np.abs(params[k].detach().numpy().astype(np.float64) - V2[k])
            bv = bv + U * np.abs(info[k]["step"])                   # torch's add_(a, alpha=-lr) is one fused multiply-add on the CPU
            if k not in clipped:
                assert np.array_equal(opt.accum[k].numpy(), A2[k]), k
            assert (da <= ba).all() and (dv <= bv).all(), (step, k)
            worst_a, worst_v = max(worst_a, (da / np.maximum(ba, 1e-300)).max()), max(worst_v, (dv / np.maximum(bv, 1e-300)).max())
    print("against MomentumSGD: accumulators %.2f of the bound, variables %.2f" % (worst_a, worst_v))


@pytest.mark.parametrize("wd", [0.0, 1e-3], ids=["plain", "decay"])
def test_float32_restatement_against_float64(wd):
    V, G = _case(1)
    decay = [k for k in V if "weights" in k] if wd else []
    lrs = (0.1, 0.05, 0.025)
    V32, A32, V64, A64 = V, onp.zeros_like(V), {k: v.astype(np.float64) for k, v in V.items()}, {k: np.zeros(s) for k, s in SHAPES.items()}
    ea = ev = None
    worst = 0.0
    for g, lr in zip(G, lrs):
        hyper = (lr, 0.98, 1.0, wd)
        case = onp.step32(V32, g, A32, hyper, decay)
        ea, ev = onp.bounds64(case, V32, hyper, decay, ea, ev)
        V32, A32, reg32, _ = case
        V64, A64, reg64, _ = onp.step64(V64, g, A64, hyper, decay)
        for k in V:
            da, dv = np.abs(A32[k] - A64[k]), np.abs(V32[k] - V64[k])
            assert (da <= ea[k]).all() and (dv <= ev[k]).all(), k
            worst = max(worst, (da / np.maximum(ea[k], 1e-300)).max(), (dv / np.maximum(ev[k], 1e-300)).max())
        assert abs(float(reg32) - reg64) <= 4 * U * reg64
    assert (reg64 > 0) == bool(wd)
    print("float32 against float64: %.2f of the bound" % worst)


def test_skipped_zero_and_non_finite_gradients_in_the_restatement():
    V, G = _case(2)
    g = dict(G[0])
    g["a/beta"] = None
    g["b/weights"] = np.zeros_like(g["b/weights"])
    g["b/gamma"] = np.array([np.inf], np.float32)
    V2, A2, _, info = onp.step32(V, g, onp.zeros_like(V), (0.1, 0.9, 1.0, 0.0))
    assert "a/beta" not in info and np.array_equal(V2["a/beta"], V["a/beta"])
    assert info["b/weights"]["s"] == 1 and np.array_equal(V2["b/weights"], V["b/weights"])
    assert np.isnan(V2["b/gamma"]).all() and all(np.isfinite(V2[k]).all() for k in V if k != "b/gamma")
    _, _, _, info = onp.step32(V, G[0], onp.zeros_like(V), (0.1, 0.9, 0.0, 0.0))
    assert all(i["s"] == 1 and not i["clipped"] for i in info.values())


def _plan(counts):
    from d3feat_amd import _lib, ops
    table = ops.momentum_sgd_plan(counts)
    C = _lib.SGD_CHUNK
    seen = [np.zeros(n, np.int32) for n in counts]
    last = (-1, 0)
    for t, b in table:
        assert 0 <= t < len(counts) and b % C == 0 and 0 <= b < counts[t]
        assert (t, b) == (last[0], last[1] + C) or (t > last[0] and b == 0), "a variable's chunks are contiguous and ascending"
        seen[t][b:b + C] += 1
        last = (t, b)
    assert all((s == 1).all() for s in seen)                            # every element exactly once
    assert len(table) == sum(-(-n // C) for n in counts)
    return table


def test_chunk_plan_covers_every_element_once():
    import re
    import os
    from conftest import ROOT
    from d3feat_amd import _lib
    header = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    C = int(re.search(r"#define\s+D3F_SGD_CHUNK\s+(\d+)", header).group(1))
    assert C == _lib.SGD_CHUNK and C % 4 == 0
    _plan([1, 3, C - 1, C, C + 1, 2 * C + 1])
    _plan([0, 5, 0, 0, 2 * C, 0])
    assert len(_plan([1] * 300)) == 300
    assert _plan([]).shape == (0, 2)
    lib = _lib.load()
    bad = np.array([4, -1], np.int32)
    assert lib.d3f_momentum_sgd_plan(bad.ctypes.data, 2, None, 0) == -3 and lib.d3f_momentum_sgd_plan(None, 2, None, 0) == -3
    assert lib.d3f_momentum_sgd_plan(bad.ctypes.data, -1, None, 0) == -3 and lib.d3f_momentum_sgd_plan(bad.ctypes.data, 1, None, -1) == -3


# ---- the model's side: fold_regularization, backward(keep_grads=True), DeviceMomentumSGD's bookkeeping on a host store -----------------
def _restated_launch(opt):
    """DeviceMomentumSGD._launch as the numpy restatement on a host store's tensors (in place, as the device call works)."""
    def launch(params, table, live):
        names = opt._names
        V = {k: params[k].detach().numpy() for k in names}
        G = {k: (params[k].grad.numpy() if k in live else None) for k in names}
        A = {k: opt.accum[k].numpy() for k in names}
        hyper = tuple(float(h) for h in opt.hyper)
        V2, A2, reg, _ = onp.step32(V, G, A, hyper, [k for k, d in zip(names, opt._decay) if d])
        for k in live:
            V[k][...] = V2[k]
            A[k][...] = A2[k]
            if opt.persistent_grads:
                G[k][...] = 0
        opt._reg[0] = float(reg)
    return launch


@pytest.fixture
def one_thread():
    """The walk's torch statements add in an order that depends on the number of threads and on their timing: two runs of one model
    differ in the last bits.  With one thread they are equal, and bit-level comparisons between runs mean something."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _model(fold):
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    model = KernelPointFCNN(iter(()), tn.config(True), weights=dict(tn.variables(True)), device=torch.device("cpu"))
    model.dropout_prob = 0.5
    model.fold_regularization = fold
    return model


def test_folded_gradient_equals_the_autograd_one(torch_operators, one_thread):
    flat = _flat(tn.geometry())
    plain, folded = _model(False), _model(True)
    plain.run(flat)
    gA = {k: p.grad.numpy().copy() for k, p in plain.backward().items()}
    folded.run(flat)
    assert folded.regularization_loss is None                          # (no optimiser attached: nobody computes it)
    assert float(folded.loss.detach()) == float((plain.desc_loss + plain.det_loss).detach())
    params = folded.backward()
    wd = np.float32(folded.config.weights_decay)
    worst = 0.0
    assert any("weights" in k for k in params) and not all("weights" in k for k in params)
    for k, p in params.items():
        g, v = p.grad.numpy(), p.detach().numpy()
        got = g + wd * v if "weights" in k else g
        bound = 2 * U * (np.abs(g) + np.abs(wd * v)) if "weights" in k else 0.0
        d = np.abs(got.astype(np.float64) - gA[k])
        assert (d <= bound).all(), k
        worst = max(worst, d.max())
    print("folded against autograd gradient: largest difference %.3e" % worst)


def test_persistent_gradients_and_the_folded_loss_on_a_host_store(torch_operators, monkeypatch, one_thread):
    """Two steps: gradient buffers that stay in place (keep_grads=True, zeroed by the step) against fresh ones, bit for bit; the
    regularisation scalar is the previous step's until step() has run."""
    from d3feat_amd.training import DeviceMomentumSGD
    flat = _flat(tn.geometry())
    cfg = tn.config(True)
    runs = {}
    for persistent in (False, True):
        model = _model(True)
        opt = DeviceMomentumSGD(model.variables, tn.LEARNING_RATE, tn.SGD_MOMENTUM, 1.0, weights_decay=cfg.weights_decay,
                                persistent_grads=persistent).attach(model)
        monkeypatch.setattr(opt, "_launch", _restated_launch(opt))
        regs, ptrs = [], []
        for step in range(2):
            model.run(flat)
            # before step(): still the figure of the step before (zero before the first)
            assert model.regularization_loss is opt.regularization_loss and float(model.regularization_loss) == ([0.0] + regs)[step]
            params = model.backward(keep_grads=persistent)
            want = sum(0.5 * float((p.detach().double() ** 2).sum()) for k, p in params.items() if "weights" in k) * float(np.float32(cfg.weights_decay))
            assert set(opt.step()) == set(params)
            regs.append(float(opt.regularization_loss))
            assert abs(regs[-1] - want) <= 4 * U * want
            ptrs.append([p.grad.data_ptr() for p in params.values()])
            if persistent:
                assert all(not p.grad.any() for p in params.values())
        assert not persistent or ptrs[0] == ptrs[1]
        assert set(opt.accum) == set(params) and all((opt.accum[k].data_ptr() - opt.accum_arena.data_ptr()) % 256 == 0 for k in params)
        runs[persistent] = ({k: p.detach().numpy().copy() for k, p in params.items()}, {k: a.numpy().copy() for k, a in opt.accum.items()})
    for k in runs[False][0]:
        assert np.array_equal(runs[False][0][k], runs[True][0][k]) and np.array_equal(runs[False][1][k], runs[True][1][k]), k
    assert not np.array_equal(runs[True][0]["layer_0/simple_0/weights"], tn.variables(True)["layer_0/simple_0/weights"])
