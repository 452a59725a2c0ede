"""The deformable KPConv above the kernel: the operator (ops.kpconv_deformable, kernels.convolution_ops.KPConv_deformable /
KPConv_deform_ops), the two blocks, a whole network with deformable blocks, and the fragment engine -- against the reference's own
results (tests/golden/deformable.npz) and the float64 restatement (tests/deformable_np.py).

Bars (set by the project, never by a measurement): fused outputs of the operator <= 5e-6 max |want| and <= 1e-4 absolute, the bars of
the rigid fused outputs (tests/test_gpu_kpconv_branches.py); blocks, descriptors and scores <= 1e-4 (BASELINE.json); a replayed
graph equals the same launch sequence run without a graph bit for bit.
Measured on an MI355X (printed by the tests, never used as a bar):
  KPConv_deform_ops against float64, error / (5e-6 max |want|): 0.02 .. 0.06 over the twelve mode combinations
  kpconv_deformable with epilogue, the same ratio: 0.03 .. 0.15 (Cout 32 / 45 / 60 / 64, largest |offset| 0.5 KP_extent, 23 % in range)
  blocks against the reference's float32 output: 9.5e-6, 5.7e-6 (resnetb_deformable plain / modulated), 6.7e-6, 4.3e-6 (strided), outputs up to 15
  network: descriptors 1.7e-6 / 1.4e-6, scores 2.7e-6 / 2.7e-6 (plain / modulated), 15556 rows; largest |offset| 0.17 / 0.41 / 1.58 KP_extent
  at layer_3/resnetb_0, layer_3/resnetb_strided_1, layer_4/resnetb_0, 83 % / 59 % / 70 % of the valid neighbours in range
  engine: replay == the same sequence without a graph, bit for bit (on the first cloud also == the op-by-op path on exact shapes)
"""
import json
import os

import numpy as np
import pytest
import torch

import deformable_cases as dc
import deformable_np as dn
from conftest import GOLDEN, surface_cloud

pytestmark = pytest.mark.gpu

ALPHA = float(np.float32(0.1))    # a LeakyReLU slope that is not the default


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "deformable.npz"))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out_ratio(got, want):
    """max |got - want| / (5e-6 max |want|), and the absolute bar."""
    err = np.abs(np.asarray(got, np.float64) - want).max()
    assert err <= 1e-4, err
    return float(err / (5e-6 * np.abs(want).max()))


# ---- operator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["plain", "mod"])
@pytest.mark.parametrize("agg", ["sum", "closest"])
@pytest.mark.parametrize("infl", ["constant", "linear", "gaussian"])
def test_deform_ops_matches_the_reference(device, gold, infl, agg, tag):
    """KPConv_deform_ops with the reference's signature on the fixture's inputs, against the reference's own float32 result: the
    fused bars, plus the float32 reference's own distance to float64 (deformable_np.out_bound: what its numpy kernels may round)."""
    from d3feat_amd.kernels import convolution_ops as co
    g = gold
    mod = _t(g["ops/modulations"], device) if tag == "mod" else None
    got = co.KPConv_deform_ops(_t(g["ops/q"], device), _t(g["ops/s"], device), _t(g["ops/idx"], device), _t(g["ops/f"], device), g["ops/kp"],
                               _t(g["ops/offsets"], device), mod, _t(g["ops/w"], device), float(g["ops/extent"]), infl, agg).cpu().numpy()
    a = (g["ops/q"], g["ops/s"], g["ops/idx"], g["ops/f"], g["ops/kp"], g["ops/offsets"], g["ops/modulations"] if tag == "mod" else None,
         g["ops/w"], float(g["ops/extent"]), infl, agg)
    want64 = dn.kpconv_deform_f64(*a)["out"]
    r = _out_ratio(got, want64)
    print("KPConv_deform_ops %s / %s / %s: error / (5e-6 max |want|) %.3f" % (infl, agg, tag, r))
    assert r <= 1.0
    want32 = g["ops/%s/%s/%s" % (infl, agg, tag)].astype(np.float64)
    slack = dn.out_bound(*a) + 5e-6 * np.abs(want64).max()
    assert np.all(np.abs(got - want32) <= slack)


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "mod"])
@pytest.mark.parametrize("Cout", [32, 45, 60, 64])
def test_kpconv_deformable_with_epilogue(device, Cout, modulated):
    """ops.kpconv_deformable / KPConv_deformable (offset convolution -> deformed aggregation -> contraction + batch-norm scale / shift,
    residual, LeakyReLU) against deformable_np on a synthetic case whose range and arg-min decisions have margins; Cout 45 / 60 are
    the widths of the offset convolution itself (no 4-column alignment), 32 / 64 the network's.  Modes in turn with Cout."""
    from d3feat_amd import ops
    from d3feat_amd.kernels import convolution_ops as co
    from oracle import kpconv_cases as kc
    infl, agg = kc.MODES[(Cout // 4 + (3 if modulated else 0)) % 6]
    Cin, Nq, K, P = 32, 101, 19, 15
    D = (4 if modulated else 3) * P
    margin = lambda r: (np.abs(r["d2"][r["valid"]] / dc.EXTENT ** 2 - 1) >= 1e-4).all() and \
        (lambda srt: (srt[:, 1] - srt[:, 0] >= 1e-4 * srt[:, 1]).all())(np.sort(r["d2"][r["valid"]], -1))
    for attempt in range(50):
        # offset weights scaled so that the convolution's own output moves a kernel point by up to KP_extent / 2.  The offsets are the convolution's, not the case generator's, so the margins of the range test
        # and of the arg-min (deformable_cases conditions 1 and 2) are checked here on what the float64 convolution produces, with
        # these weights and with zero weights: "change the seed, not the bar"
        c = dc.deform_case(kc.shape_seed("deform_operator", Cin, Nq, K) + 1000 * attempt, Cin, K, Nq)
        rng = np.random.default_rng(Cout + 1000 * attempt)
        W0 = (rng.standard_normal((P, Cin, D)) * (1.5 / np.sqrt(P * Cin))).astype(np.float32)
        b0 = (0.1 * rng.standard_normal(D)).astype(np.float32)
        W = kc.weights(Cout, P, Cin, Cout)
        cs, ch = (1.0 + 0.2 * rng.standard_normal(Cout)).astype(np.float32), (0.1 * rng.standard_normal(Cout)).astype(np.float32)
        res = rng.standard_normal((Nq, Cout)).astype(np.float32)
        run = lambda: dn.kpconv_deformable_f64(c.q, c.s, c.idx, c.f, c.KP, W, W0, b0, dc.EXTENT, infl, agg, modulated, Nq=Nq, Ns=c.Ns,
                                               col_scale=cs, col_shift=ch, residual=res, leaky=True, alpha=ALPHA)
        scale = 0.5 / np.linalg.norm(run()["raw"][:, :3 * P].reshape(Nq, P, 3), axis=-1).max()    # largest |offset| = KP_extent / 2
        W0, b0 = (W0 * scale).astype(np.float32), (b0 * scale).astype(np.float32)
        want = run()
        z = dn.kpconv_deform_f64(c.q, c.s, c.idx, c.f, c.KP, np.zeros((Nq, P, 3)), np.ones((Nq, P)) if modulated else None, W, dc.EXTENT,
                                 infl, agg, Nq=Nq, Ns=c.Ns)
        if margin(want) and margin(z):
            break
    assert margin(want) and margin(z)
    kept, valid = want["in_range"].sum(), want["valid"].sum()
    assert 0 < kept < valid
    reach = np.linalg.norm(want["raw"][:, :3 * P].reshape(Nq, P, 3), axis=-1).max()
    assert 0.45 < reach < 0.55, reach
    q, s, idx, f = _t(c.q[:Nq], device), _t(c.s[:c.Ns], device), _t(c.idx[:Nq], device), _t(c.f[:c.Ns], device)
    epi = dict(col_scale=_t(cs, device), col_shift=_t(ch, device), residual=_t(res, device), leaky=True, alpha=ALPHA)
    got = ops.kpconv_deformable(q, s, idx, f, c.KP, _t(W, device), _t(W0, device), _t(b0, device), dc.EXTENT, infl, agg, modulated, **epi)
    r = _out_ratio(got.cpu().numpy(), want["out"])
    got2 = co.KPConv_deformable(q, s, idx, f, _t(W, device), KP_extent=dc.EXTENT, KP_influence=infl, aggregation_mode=agg,
                                modulated=modulated, K_points=c.KP, offset_weights=_t(W0, device), offset_bias=_t(b0, device), epilogue=epi)
    assert torch.equal(got, got2)
    print("kpconv_deformable Cout %d %s / %s %s: error / (5e-6 max |want|) %.3f, largest |offset| %.2f KP_extent, %d of %d neighbours in range"
          % (Cout, infl, agg, "modulated" if modulated else "", r, reach, kept, valid))
    assert r <= 1.0
    # zero offset weights (the reference's initial values): the rigid points, KP_extent as the influence radius
    zero = co.KPConv_deformable(q, s, idx, f, _t(W, device), KP_extent=dc.EXTENT, KP_influence=infl, aggregation_mode=agg,
                                modulated=modulated, K_points=c.KP)
    assert _out_ratio(zero.cpu().numpy(), z["out"]) <= 1.0


# ---- blocks ---------------------------------------------------------------------------------------------------------------------
def _cfg(modulated):
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    cfg.modulated = bool(modulated)
    return cfg


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "mod"])
@pytest.mark.parametrize("name", ["resnetb_deformable", "resnetb_deformable_strided"])
def test_blocks_match_the_reference(device, gold, name, modulated):
    """Both blocks on the fixture's crop with the fixture's variables against the reference's own output, at the parity bar."""
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import VariableStore
    g = gold
    tag = "block/%s/%s" % (name, "mod" if modulated else "plain")
    W = {"b/" + n: g["%s/var/%s" % (tag, n)] for n, _ in json.loads(str(g[tag + "/varlist"]))}
    inputs = dict(points=[_t(g["block/points_0"], device), _t(g["block/points_1"], device)], neighbors=[_t(g["block/neighbors_0"], device)],
                  pools=[_t(g["block/pools_0"], device)])
    vs = VariableStore(W, device=device, create=False)
    with nb.use_variables(vs), vs.variable_scope("b"):
        out = nb.get_block_ops(name)(0, inputs, _t(g["block/features"], device), float(g["block/radius"]), int(g["block/fdim"]),
                                     _cfg(modulated), False)
    err = np.abs(out.cpu().numpy().astype(np.float64) - g[tag + "/out"]).max()
    print("%s: max |out - reference| %.2e (largest |reference| %.1f)" % (tag, err, np.abs(g[tag + "/out"]).max()))
    assert err <= 1e-4


# ---- whole network --------------------------------------------------------------------------------------------------------------
def _deformable_config(modulated):
    """The shipped 3DMatch architecture with level 3's resnetb, level 3's resnetb_strided and level 4's resnetb deformable."""
    cfg = _cfg(modulated)
    arch = list(cfg.architecture)
    assert arch[7:10] == ["resnetb", "resnetb_strided", "resnetb"]
    arch[7:10] = ["resnetb_deformable", "resnetb_deformable_strided", "resnetb_deformable"]
    cfg.architecture = arch
    return cfg


@pytest.fixture(scope="module")
def cloud():
    return surface_cloud(11, n_raw=16000)


@pytest.fixture(scope="module")
def limits(device, cloud):
    """calibrate_neighbors, as for any architecture (the limits do not depend on `modulated`)."""
    from d3feat_amd.datasets.common import FragmentDataset
    cfg = _deformable_config(False)
    ds = FragmentDataset([cloud])
    hist_n = int(np.ceil(4 / 3 * np.pi * (cfg.density_parameter + 1) ** 3))
    ds.neighborhood_limits = np.full(cfg.num_layers, hist_n, dtype=np.int32)
    ds.calibrate_neighbors(cfg, samples_threshold=1)
    return np.asarray(ds.neighborhood_limits, np.int32)


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "mod"])
def test_network_with_deformable_blocks(device, cloud, limits, modulated):
    from d3feat_amd.datasets.common import FragmentDataset
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.models.variables import build_variables
    cfg = _deformable_config(modulated)
    assert 2000 <= len(cloud) <= 9000
    W = build_variables(cfg, seed=42, randomize_bn=True, randomize_offsets=True).values
    ds = FragmentDataset([cloud])
    ds.neighborhood_limits = limits
    gen, _, _ = ds.get_batch_gen("test", cfg)
    flat = ds.get_tf_mapping(cfg)(*ds._to_device(next(iter(gen()))))
    model = KernelPointFCNN(flat, cfg, weights=W, device=device)
    a = model.anchor_inputs
    L = cfg.num_layers
    host = lambda t: t.cpu().numpy()
    inp = dict(points=[host(p) for p in a["points"]], neighbors=[host(p) for p in a["neighbors"]], pools=[host(p) for p in a["pools"]],
               upsamples=[host(p) for p in a["upsamples"]], features=host(a["features"]), in_batches=host(a["in_batches"]),
               stack_lengths=host(a["stack_lengths"]))
    # the search radii (datasets/common.py:1340-1364): a pool matrix is widened to r_normal * density_parameter / (KP_extent * 2.5)
    # = 2 r_normal when ITS block is deformable -- level 3's, which the deformable strided block convolves over; a conv matrix only
    # when a deformable block stands before the last of the layer's non-strided blocks (`layer_blocks[:-1]`) -- none here: level 3
    # and level 4 hold one such block each, so their conv matrices keep r_normal, as in the reference.  Read from a pyramid whose
    # rows are not cut to the calibrated limits (a limit keeps the nearest neighbours of a row: a cut row says nothing of the radius).
    r3 = cfg.first_subsampling_dl * cfg.KP_extent * 2.5 * 2 ** 3
    wide = r3 * cfg.density_parameter / (cfg.KP_extent * 2.5)
    assert wide == 2 * r3
    full = FragmentDataset([cloud])
    full.neighborhood_limits = np.full(L, 1000, np.int32)
    fl = [host(p) for p in full.get_tf_mapping(cfg)(*full._to_device(next(iter(gen()))))[:3 * L]]
    for l in range(L):
        assert np.array_equal(fl[l], inp["points"][l])

    def reach(q, s, idx):
        valid = idx < len(s)
        d = np.linalg.norm(s[np.where(valid, idx, 0)].astype(np.float64) - q[:, None, :], axis=-1)
        return float((d * valid).max())
    tol = 1 + 1e-6          # (the searches compare float32 squared distances)
    assert r3 < reach(fl[4], fl[3], fl[2 * L + 3]) <= wide * tol                 # pools[3]: deformable strided block
    assert r3 / 2 < reach(fl[3], fl[3], fl[L + 3]) <= r3 * tol                   # neighbors[3]
    assert r3 / 4 < reach(fl[3], fl[2], fl[2 * L + 2]) <= r3 / 2 * tol           # pools[2]: rigid
    assert r3 < reach(fl[4], fl[4], fl[L + 4]) <= 2 * r3 * tol                   # neighbors[4]
    trace = {}
    want_d, want_s = dn.forward(cfg, W, inp, trace=trace)
    assert sorted(trace) == ["layer_3/resnetb_0", "layer_3/resnetb_strided_1", "layer_4/resnetb_0"]
    for scope, r in trace.items():
        off = np.linalg.norm(r["raw"][:, :45].reshape(-1, 15, 3), axis=-1)
        kept, valid = r["in_range"].sum(), r["valid"].sum()
        print("%s: largest |offset| %.2f KP_extent, %d of %d neighbours in range" % (scope, off.max(), kept, valid))
        assert off.max() > 0.1 and 0 < kept < valid
    d, s = model.out_features.cpu().numpy(), model.out_scores.cpu().numpy()
    ed, es = np.abs(d - want_d).max(), np.abs(s - want_s).max()
    print("network (%s): %d rows, descriptor max err %.2e, score max err %.2e" % ("modulated" if modulated else "plain", len(d), ed, es))
    assert ed <= 1e-4 and es <= 1e-4


# ---- fragment engine ------------------------------------------------------------------------------------------------------------
def _same_sequence_without_a_graph(eng, slot):
    """The slot's launch sequence on the inputs it still holds, issued eagerly (same capacities, so the same kernels and launch
    plans as the captured graph) -> (desc, score) clones; the slot's own static tensors are put back afterwards."""
    from d3feat_amd import ops
    sl = eng.slots[slot]
    saved, saved_ds = dict(vars(sl)), dict(vars(sl.ds))
    with torch.cuda.stream(sl.stream), ops.private_workspace():
        _, desc, score, status, _ = eng._sequence(sl)
        out = desc.clone(), score.clone()
        status[:, 1].zero_()
    sl.stream.synchronize()
    vars(sl).clear(), vars(sl).update(saved)
    vars(sl.ds).clear(), vars(sl.ds).update(saved_ds)
    return out


def test_engine_replays_a_deformable_architecture(device, limits):
    """A deformable architecture through FragmentEngine: the default numbering resolves to the reference's, the launch sequence
    captures (no host read-back, no data-dependent shape), two different clouds replayed from the ONE captured graph each equal
    the same sequence issued without a graph bit for bit, and the op-by-op path on exact shapes within the parity bar; an explicit
    internal_order=True still raises."""
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.synthetic import room_fragment
    cfg = _deformable_config(True)
    W = build_variables(cfg, seed=42, randomize_bn=True, randomize_offsets=True).values
    eng = FragmentEngine(cfg, W, limits, raw_cap=40000, n0_cap=12000, slots=1, device=device)
    assert eng.internal is False
    graph = eng.slots[0].graph
    raws = [torch.from_numpy(room_fragment(s, n_raw=n, edge=1.0)).to(device) for s, n in ((21, 30000), (22, 24000))]
    outs = []
    for raw in raws:
        pts, d, s = (t.clone() for t in eng.run(raw, slot=0))
        assert eng.fallbacks == 0                                      # the replay's own result, not the op-by-op path's
        ed, es = _same_sequence_without_a_graph(eng, 0)
        n = len(pts)
        assert torch.equal(d, ed[:n]) and torch.equal(s, es[:n])
        outs.append((pts, d, s))
    assert eng.fallbacks == 0 and eng.slots[0].graph is graph
    assert outs[0][0].shape != outs[1][0].shape
    pts, d, s = (t.clone() for t in eng.run(raws[0], slot=0))          # and the graph still replays after the eager passes
    assert torch.equal(pts, outs[0][0]) and torch.equal(d, outs[0][1]) and torch.equal(s, outs[0][2])
    for raw, (pts, d, s) in zip(raws, outs):
        ep, ed, es = eng.run_eager(raw)
        assert torch.equal(pts, ep)
        for x, y in ((d, ed), (s, es)):          # (other launch plans: exact shapes instead of capacities)
            assert np.abs(x.cpu().numpy().astype(np.float64) - y.cpu().numpy()).max() <= 1e-4
    with pytest.raises(ValueError, match="deformable"):
        FragmentEngine(cfg, W, limits, raw_cap=40000, n0_cap=12000, slots=1, device=device, internal_order=True)
