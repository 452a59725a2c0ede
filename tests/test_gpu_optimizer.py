"""d3f_momentum_sgd on the GPU against tests/optimizer_np.py, and training.DeviceMomentumSGD on the training_network golden case.

The kernel's cases are the smallest at which it can go wrong: counts around the quad (1, 3, 4, 5) and around the chunk (C - 1, C, C + 1,
2 C + 1, C = D3F_SGD_CHUNK), one variable of ten chunks (40000), 300 variables of one element, pointers off the 16-byte grid, a skipped
variable between live ones, a zero gradient, clip <= 0, an infinite entry.  Every table lies in three arenas filled with a sentinel, so
each case also checks that no word outside the counts is written.
Bits: inputs that are multiples of 2^-6 with |.| <= 4 (and wd = 2^-3) make every square and partial sum exact in float64, so a', v' and
the regularisation loss equal the float32 restatement bit for bit, clipped or not; on other inputs the unclipped variables are bit-equal
and the clipped ones lie within optimizer_np.bounds.

Measured on an MI355X (printed, never used as a bar): every exact-sum case bit-equal, clipped ones included -- the device's float64 square
root is correctly rounded; on inexact sums the clipped variables also came out bit-equal (0.000 of the bound, aligned and shifted).  On
the model: against MomentumSGD on a clone 0.878 of the bound (bounds plus one rounding of lr a'); the inference forward after commit()
within 5.2e-7 (descriptors) and 1.5e-6 (scores) of the float32 oracle; 21 packed weight copies and no derived tensor before the step of
the no-batch-norm model; folded against autograd regularisation bit-equal parameters, the regularisation loss 1.9e-9 of its value off
the float64 figure.  The 17 tests take 3.5 s."""
import os
import re

import numpy as np
import pytest
import torch

import optimizer_np as onp
import training_network_np as tn
from conftest import ROOT
from test_gpu_training_network import TAG, TERMS, _flat, golden  # noqa: F401  (the loaders, the golden fixture)

pytestmark = pytest.mark.gpu
U = onp.U
SENT = 777.25
C = int(re.search(r"#define\s+D3F_SGD_CHUNK\s+(\d+)", open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()).group(1))
COUNTS = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1, 40000)


class _Table:
    """Variables, gradients and accumulators inside three sentinel-filled arenas, every offset a multiple of 64 elements (plus one
    element for the names in `shift`), and the device tables of one d3f_momentum_sgd call."""

    def __init__(self, device, V, G, A, decay=(), shift=()):
        from d3feat_amd import ops
        self.names, self.device = list(V), device
        self.off, cur = {}, 64
        for k in self.names:
            self.off[k] = (cur + 63) // 64 * 64 + (1 if k in shift else 0)
            cur = self.off[k] + V[k].size + 64
        self.size = cur + 64
        self.mask = np.ones(self.size, bool)
        host = {}
        for which, src in (("v", V), ("g", G), ("a", A)):
            h = np.full(self.size, SENT, np.float32)
            for k in self.names:
                if src.get(k) is not None:
                    h[self.off[k]:self.off[k] + V[k].size] = src[k].reshape(-1)
                self.mask[self.off[k]:self.off[k] + V[k].size] = False
            host[which] = h
        self.start = host
        self.arena = {w: torch.from_numpy(h.copy()).to(device) for w, h in host.items()}
        desc = np.zeros((len(self.names), 4), np.int64)
        for i, k in enumerate(self.names):
            desc[i, 0] = self.arena["v"].data_ptr() + 4 * self.off[k]
            desc[i, 1] = self.arena["g"].data_ptr() + 4 * self.off[k] if G.get(k) is not None else 0
            desc[i, 2] = self.arena["a"].data_ptr() + 4 * self.off[k]
            desc[i, 3] = V[k].size + ((1 if k in decay else 0) << 32)
        self.desc = torch.from_numpy(desc).to(device)
        self.chunks = torch.from_numpy(ops.momentum_sgd_plan([V[k].size for k in self.names])).to(device)
        self.reg = torch.full((1,), SENT, dtype=torch.float32, device=device)
        self.shapes = {k: V[k].shape for k in self.names}
        self.live = {k for k in self.names if G.get(k) is not None}

    def step(self, hyper, zero_grad=False):
        from d3feat_amd import ops
        ops.momentum_sgd_step(self.desc, self.chunks, hyper, zero_grad=zero_grad, reg_loss=self.reg)

    def read(self, which):
        h = self.arena[which].cpu().numpy()
        assert np.array_equal(h[self.mask], self.start[which][self.mask]), "a word outside the counts of %s was written" % which
        return {k: h[self.off[k]:self.off[k] + int(np.prod(self.shapes[k]))].reshape(self.shapes[k]) for k in self.names}

    def set_grads(self, G):
        h = self.start["g"].copy()
        for k in self.live:
            h[self.off[k]:self.off[k] + G[k].size] = G[k].reshape(-1)
        self.start["g"] = h
        self.arena["g"].copy_(torch.from_numpy(h))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, label):
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d of %d words differ, largest %.3e" % (
        label, int((_bits(got) != _bits(want)).sum()), got.size, np.nanmax(np.abs(got.astype(np.float64) - want)))


def _hyper(device, values):
    return torch.tensor(values, dtype=torch.float32, device=device)


def _inputs(rng, counts, quantised, grad_scale=1.0):
    names = ["t%02d_%d" % (i, n) for i, n in enumerate(counts)]
    draw = (lambda n: onp.quantised(rng, n)) if quantised else (lambda n: rng.standard_normal(n).astype(np.float32))
    V = {k: draw(n) for k, n in zip(names, counts)}
    G = {k: (draw(n) * np.float32(grad_scale)).astype(np.float32) for k, n in zip(names, counts)}
    A = {k: draw(n) for k, n in zip(names, counts)}
    return names, V, G, A


def _check(table, case, zero_grad, G, exact, hyper):
    """The device's a', v', reg and g against step32's: bit for bit (exact: every variable; else the unclipped ones, the clipped within
    bounds).  -> the largest fraction of a bound used."""
    V2, A2, reg, info = case
    gv, ga, gg = table.read("v"), table.read("a"), table.read("g")
    bnd, worst = onp.bounds(case, hyper), 0.0
    for k in table.names:
        if exact or k not in info or not info[k]["clipped"]:
            _same(ga[k], A2[k], k + " accumulator")
            _same(gv[k], V2[k], k + " variable")
        else:
            da, dv = np.abs(ga[k].astype(np.float64) - A2[k]), np.abs(gv[k].astype(np.float64) - V2[k])
            assert (da <= bnd[k][0]).all() and (dv <= bnd[k][1]).all(), k
            worst = max(worst, (da / np.maximum(bnd[k][0], 1e-300)).max(), (dv / np.maximum(bnd[k][1], 1e-300)).max())
        if k in table.live:
            if zero_grad:
                assert not _bits(gg[k]).any(), k + ": the gradient is +0 after a zeroing step"
            else:
                _same(gg[k], G[k], k + " gradient")
    return worst, float(table.reg.cpu()[0]), float(reg)


@pytest.mark.parametrize("clip,wd", [(8.0, 0.125), (8.0, 0.0), (0.0, 0.125), (-1.0, 0.0)], ids=["clip-decay", "clip", "noclip-decay", "negclip"])
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep", "zero"])
def test_every_count_bit_for_bit_on_exact_sums(device, clip, wd, zero_grad):
    rng = np.random.default_rng(5)
    counts = COUNTS + (100, 77, 9)
    names, V, G, A = _inputs(rng, counts, True)
    G[names[-3]] = np.zeros_like(G[names[-3]])                       # an all-zero gradient
    G[names[-2]] = None                                              # skipped, between two live ones
    decay = names[::2] if wd else []
    hyper = (0.0625 + 0.01, 0.98, clip, wd)
    case = onp.step32(V, G, A, hyper, decay)
    if clip > 0:
        flags = [i["clipped"] for i in case[3].values()]
        assert any(flags) and not all(flags)
    table = _Table(device, V, G, A, decay)
    table.step(_hyper(device, hyper), zero_grad)
    _, reg, want = _check(table, case, zero_grad, G, True, hyper)
    assert np.float32(reg).view(np.uint32) == np.float32(want).view(np.uint32), (reg, want)
    assert (want > 0) == bool(wd)
    assert np.array_equal(table.read("v")[names[-2]], V[names[-2]]) and np.array_equal(table.read("a")[names[-2]], A[names[-2]])


def test_three_hundred_one_element_variables(device):
    rng = np.random.default_rng(6)
    names, V, G, A = _inputs(rng, (1,) * 300, True)
    hyper = (0.1, 0.9, 2.0, 0.125)
    case = onp.step32(V, G, A, hyper, names[1::3])
    table = _Table(device, V, G, A, names[1::3])
    assert table.chunks.shape[0] == 300
    table.step(_hyper(device, hyper), True)
    _, reg, want = _check(table, case, True, G, True, hyper)
    assert reg == want


def test_unaligned_pointers_give_the_bits_of_aligned_ones_and_clipped_variables_their_bounds(device):
    """Inexact sums: the 4-byte path adds in the order of the 16-byte one; unclipped variables bit for bit, clipped within bounds."""
    rng = np.random.default_rng(7)
    names, V, G, A = _inputs(rng, COUNTS, False, grad_scale=0.05)
    hyper = (0.1, 0.98, 1.0, 1e-3)
    decay = names[::2]
    case = onp.step32(V, G, A, hyper, decay)
    flags = [i["clipped"] for i in case[3].values()]
    assert any(flags) and not all(flags)
    out = []
    for shift in ((), names):
        table = _Table(device, V, G, A, decay, shift)
        table.step(_hyper(device, hyper), False)
        worst, reg, want = _check(table, case, False, G, False, hyper)
        assert abs(reg - want) <= 4 * U * want
        out.append((table.read("v"), table.read("a"), reg))
        print("clipped variables: %.3f of the bound (pointers %s)" % (worst, "shifted" if shift else "aligned"))
    for k in names:
        _same(out[1][0][k], out[0][0][k], k + " variable, 4-byte path")
        _same(out[1][1][k], out[0][1][k], k + " accumulator, 4-byte path")
    assert out[0][2] == out[1][2]


def test_an_infinite_entry_poisons_its_own_variable_only(device):
    rng = np.random.default_rng(8)
    names, V, G, A = _inputs(rng, (5, C + 1, 77), True)
    G[names[1]][C - 3] = np.inf
    hyper = (0.1, 0.98, 8.0, 0.0)
    case = onp.step32(V, G, A, hyper)
    table = _Table(device, V, G, A)
    table.step(_hyper(device, hyper))
    gv, ga = table.read("v"), table.read("a")
    want_nan = np.isnan(case[0][names[1]])
    assert want_nan.sum() == 1 and np.array_equal(np.isnan(gv[names[1]]), want_nan) and np.array_equal(np.isnan(ga[names[1]]), np.isnan(case[1][names[1]]))
    _same(gv[names[1]][~want_nan], case[0][names[1]][~want_nan], "the finite entries")
    for k in (names[0], names[2]):
        _same(gv[k], case[0][k], k)
        _same(ga[k], case[1][k], k)


def test_three_steps_with_the_hyper_parameters_rewritten_on_the_device_twice_over(device):
    rng = np.random.default_rng(9)
    counts = (3, C + 1, 2 * C + 1, 130)
    names, V, _, _ = _inputs(rng, counts, True)
    grads = [_inputs(rng, counts, True)[2] for _ in range(3)]
    hypers = [(0.125, 0.5, 8.0, 0.125), (0.0625, 0.75, 16.0, 0.125), (0.03125, 0.5, 0.0, 0.25)]
    runs = []
    for _ in range(2):
        table = _Table(device, V, grads[0], onp.zeros_like(V), names[:2])
        hyper = _hyper(device, hypers[0])
        regs = []
        for s in range(3):
            if s:
                table.set_grads(grads[s])
                hyper.copy_(_hyper(device, hypers[s]))
            # every step against the restatement FROM THE DEVICE'S OWN STATE (after a step the variables are no multiples of 2^-6
            # any more): unclipped variables bit for bit, clipped ones within the one-step bounds; the last step clips nothing
            case = onp.step32(table.read("v"), grads[s], table.read("a"), hypers[s], names[:2])
            table.step(hyper, False)
            _, reg, want = _check(table, case, False, grads[s], s == 0, hypers[s])
            assert abs(reg - want) <= 4 * U * want and want > 0
            regs.append(reg)
        runs.append((table.read("v"), table.read("a"), regs))
    for k in names:
        _same(runs[0][0][k], runs[1][0][k], k + ": two runs")
        _same(runs[0][1][k], runs[1][1][k], k + ": two runs")
    assert runs[0][2] == runs[1][2]


# ---- training.DeviceMomentumSGD ------------------------------------------------------------------------------------------------------
def _store(device, V):
    from d3feat_amd.models.variables import VariableStore
    store = VariableStore(values={k: v.copy() for k, v in V.items()}, device=device, create=False)
    return store, {k: store.parameter(k) for k in V}


def _paint_padding(opt, arena, views):
    """Sentinels into every word of an arena that no view covers -> the mask."""
    mask = torch.ones(arena.numel(), dtype=torch.bool, device=arena.device)
    for t in views.values():
        o = (t.data_ptr() - arena.data_ptr()) // 4
        assert o % 64 == 0
        mask[o:o + t.numel()] = False
    arena[mask] = SENT
    return mask


def test_captured_step_follows_the_learning_rate_and_keeps_the_paddings(device):
    from d3feat_amd.training import DeviceMomentumSGD
    rng = np.random.default_rng(10)
    V = {"a/weights": rng.standard_normal((3, C + 5)).astype(np.float32), "a/beta": rng.standard_normal(7).astype(np.float32),
         "b/weights": rng.standard_normal((5, 13)).astype(np.float32), "b/gamma": rng.standard_normal(1).astype(np.float32)}
    grads = [{k: (rng.standard_normal(v.shape) * (0.5 if "a/" in k else 0.001)).astype(np.float32) for k, v in V.items()} for _ in range(4)]
    lrs = (0.1, 0.05, 0.025, 0.0125)
    out = {}
    for mode in ("eager", "replay"):
        store, params = _store(device, V)
        opt = DeviceMomentumSGD(store, lrs[0], 0.9, 1.0, weights_decay=1e-3, persistent_grads=True)
        for k, p in params.items():
            p.grad = torch.from_numpy(grads[0][k]).to(device)
        assert set(opt.step()) == set(V)                              # (the first step installs the arenas; eager in both modes)
        masks = (_paint_padding(opt, opt.accum_arena, opt.accum), _paint_padding(opt, opt.grad_arena, opt.grads))
        ptrs = [p.grad.data_ptr() for p in params.values()]
        assert all(not p.grad.any() for p in params.values())
        graph = None
        if mode == "replay":                                          # (a capture runs nothing: the state stays where step 0 left it)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
        regs = []
        for s in range(1, 4):
            opt.set_learning_rate(lrs[s])
            for k, p in params.items():
                p.grad.copy_(torch.from_numpy(grads[s][k]).to(device))
            if graph is None:
                opt.step()
            else:
                graph.replay()
                opt.mark_updated()
            regs.append(float(opt.regularization_loss))
            assert all(not p.grad.any() for p in params.values())
        assert [p.grad.data_ptr() for p in params.values()] == ptrs
        assert bool((opt.accum_arena[masks[0]] == SENT).all()) and bool((opt.grad_arena[masks[1]] == SENT).all())
        out[mode] = ({k: p.detach().cpu().numpy() for k, p in params.items()}, {k: a.cpu().numpy() for k, a in opt.accum.items()}, regs)
    for k in V:
        _same(out["replay"][0][k], out["eager"][0][k], k + " variable, replayed")
        _same(out["replay"][1][k], out["eager"][1][k], k + " accumulator, replayed")
    assert out["replay"][2] == out["eager"][2]
    want = onp.run32(V, [(g, (lr, 0.9, 1.0, 1e-3)) for g, lr in zip(grads, lrs)], [k for k in V if "weights" in k])
    flags = [i["clipped"] for i in want[0][3].values()]
    assert any(flags) and not all(flags)
    for k in V:
        if "b/" in k:                                                 # never clipped: the restatement's bits after four steps
            _same(out["eager"][0][k], want[-1][0][k], k)


def _trained(device, use_bn, fold=False, **opt_kw):
    """A model after one training-mode run and backward, and its optimiser (not stepped)."""
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.training import DeviceMomentumSGD
    cfg, inp = tn.config(use_bn), tn.geometry()
    model = KernelPointFCNN(iter(()), cfg, weights=dict(tn.variables(use_bn)), device=device)
    model.dropout_prob = 0.5
    flat = _flat(inp, device)
    clip = tn.clip_norm(tn.tape(use_bn)["grads"])
    opt = DeviceMomentumSGD(model.variables, tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip, weights_decay=cfg.weights_decay if fold else 0.0, **opt_kw)
    if fold:
        opt.attach(model)
    model.run(flat)
    model.backward(keep_grads=bool(opt_kw.get("persistent_grads")))
    return model, opt, flat, clip


def _host(params):
    return {k: p.detach().cpu().numpy().copy() for k, p in params.items()}


def test_model_step_meets_the_golden_parameters_the_torch_class_and_the_oracle(device, golden):
    from d3feat_amd.training import MomentumSGD
    from oracle import network_np as onet
    use_bn = True
    model, opt, flat, clip = _trained(device, use_bn)
    ref, V = tn.tape(use_bn), tn.variables(use_bn)
    params = model.variables.parameters()
    before, grads = _host(params), {k: p.grad.cpu().numpy().copy() for k, p in params.items()}
    twin_store, twin = _store(device, before)
    for k, p in twin.items():
        p.grad = torch.from_numpy(grads[k]).to(device)
    MomentumSGD(twin_store, tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip).step()
    versions = {k: p._version for k, p in params.items()}
    assert set(opt.step(commit=True)) == set(params)
    assert all(p._version > versions[k] for k, p in params.items())
    want, clipped = tn.momentum_step(V, ref["grads"], tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    key = "err32/net/%s/grad/" % TAG[use_bn]
    after = _host(params)
    for k, w in want.items():                                         # the bar of test_gpu_training_network's own step test
        big_g = np.abs(ref["grads"][k]).max()
        tol_g = max(min(max(4 * golden[key + k], (TERMS + 16) * U * big_g), 1e-4 * big_g), 4 * golden[key + k])
        assert np.abs(after[k].astype(np.float64) - w).max() <= 2 * tn.LEARNING_RATE * tol_g + 4 * U * np.abs(w).max(), k
        assert np.array_equal(model.variables.values[k], after[k])
    hyper = (tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip, 0.0)
    case = onp.step32(before, grads, onp.zeros_like(before), hyper)
    worst = 0.0
    for k, (ba, bv) in onp.bounds(case, hyper).items():
        if not case[3][k]["clipped"]:
            _same(after[k], case[0][k], k + " against the restatement")
        d = np.abs(after[k].astype(np.float64) - twin[k].detach().cpu().numpy())
        bound = bv + U * np.abs(case[3][k]["step"])                  # (one rounding of lr a' for a fused add)
        assert (d <= bound).all(), k
        worst = max(worst, (d / np.maximum(bound, 1e-300)).max())
    print("against MomentumSGD: %.3f of the bound" % worst)
    model.dropout_prob = 1.0
    d, s = model.run(flat)
    want_d, want_s = onet.forward(model.config, model.variables.values, tn.geometry())
    ed, es = np.abs(d.cpu().numpy() - want_d).max(), np.abs(s.cpu().numpy() - want_s).max()
    print("inference after commit: descriptors %.2e, scores %.2e" % (ed, es))
    assert ed <= 1e-4 and es <= 1e-4


def test_inference_forms_see_the_step_before_any_commit(device):
    """Without batch norm the inference forms read the device copies and their packed copies directly: after step() alone -- no
    commit(), whose in-place copies would move the version counters anyway -- the forward must use the new weights, which it does only
    when the step has bumped the version the packed copies are keyed on."""
    from d3feat_amd import ops
    from oracle import network_np as onet
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.training import DeviceMomentumSGD
    cfg, inp = tn.config(False), tn.geometry()
    model = KernelPointFCNN(iter(()), cfg, weights=dict(tn.variables(False)), device=device)
    flat = _flat(inp, device)
    model.run(flat)                                                   # the inference forms make their packed copies
    packed = sum(len(getattr(t, slot, None) or {}) for k, t in model.variables._dev.items() if isinstance(k, str) for slot, _ in ops._PACKERS)
    derived = [k for k in model.variables._dev if not isinstance(k, str)]
    model.dropout_prob = 0.5
    model.run(flat)
    model.backward()
    opt = DeviceMomentumSGD(model.variables, tn.LEARNING_RATE, tn.SGD_MOMENTUM, tn.clip_norm(tn.tape(False)["grads"]))
    versions = {k: p._version for k, p in model.variables.parameters().items()}
    live = opt.step()
    assert live and all(model.variables.parameters()[k]._version > versions[k] for k in live)
    print("packed copies before the step: %d, derived tensors: %d" % (packed, len(derived)))
    if derived:
        return                                                        # (folded copies exist: only commit() refreshes those)
    model.dropout_prob = 1.0
    d, s = model.run(flat)
    values = dict(model.variables.values)
    values.update({k: t.detach().cpu().numpy() for k, t in model.variables._dev.items() if isinstance(k, str)})
    want_d, want_s = onet.forward(cfg, values, inp)
    assert np.abs(d.cpu().numpy() - want_d).max() <= 1e-4 and np.abs(s.cpu().numpy() - want_s).max() <= 1e-4


def test_persistent_gradients_equal_fresh_ones_over_two_steps(device):
    out = {}
    for persistent in (False, True):
        model, opt, flat, _ = _trained(device, True, persistent_grads=persistent)
        opt.step()
        ptrs = [p.grad.data_ptr() for p in model.variables.parameters().values()]
        model.run(flat)
        params = model.backward(keep_grads=persistent)
        if persistent:
            assert [p.grad.data_ptr() for p in params.values()] == ptrs
        opt.step()
        out[persistent] = (_host(params), {k: a.cpu().numpy() for k, a in opt.accum.items()})
    for k in out[False][0]:
        _same(out[True][0][k], out[False][0][k], k + " variable")
        _same(out[True][1][k], out[False][1][k], k + " accumulator")


def test_folded_regularisation_against_the_autograd_mode(device):
    plain, opt_p, _, clip = _trained(device, True)
    folded, opt_f, _, _ = _trained(device, True, fold=True)
    assert folded.regularization_loss is opt_f.regularization_loss and float(folded.regularization_loss) == 0.0
    assert abs(float(folded.loss.detach()) - float((plain.desc_loss + plain.det_loss).detach())) <= 4 * U * abs(float(plain.loss.detach()))
    before = _host(plain.variables.parameters())
    grads = {k: p.grad.cpu().numpy().copy() for k, p in plain.variables.parameters().items()}
    opt_p.step()
    opt_f.step()
    hyper = (tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip, 0.0)
    case = onp.step32(before, grads, onp.zeros_like(before), hyper)
    a, b = _host(plain.variables.parameters()), _host(folded.variables.parameters())
    worst = 0.0
    for k, (ba, bv) in onp.bounds(case, hyper).items():
        d = np.abs(a[k].astype(np.float64) - b[k])
        assert (d <= bv).all(), k
        worst = max(worst, (d / np.maximum(bv, 1e-300)).max())
    wd = float(np.float32(plain.config.weights_decay))
    want = wd * sum(0.5 * float((v.astype(np.float64) ** 2).sum()) for k, v in before.items() if "weights" in k)
    got = float(opt_f.regularization_loss)
    print("folded against autograd mode: %.3f of the bound; regularisation loss %.3e of its value off" % (worst, abs(got - want) / want))
    assert abs(got - want) <= 4 * U * want
    assert abs(got - float(plain.regularization_loss.detach())) <= 1e-5 * want
