"""d3f_validation_pairs / d3feat_amd.validation on the MI355X: the validation figures of the reference's model class (circle loss,
contrastive loss, detection loss, accuracy, mean positive / negative distance) and the trainer's split means -- against the
reference's own Python (tests/golden/validation.npz, tools/make_golden_validation.py) and against the float64 restatement
tests/validation_np.py with tolerances derived from each case (validation_np.tolerances); counts must be EQUAL, which
validation_np.margins makes a property of every input used here."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import validation_np as vnp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
FIG = ("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg")
GRID_N = (2, 3, 63, 64, 65, 255, 256, 257, 1024)
_cache = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _grid_case(C, n):
    """One clean case of the size grid (0.4 m cube, noise 1.6: accuracies well inside (0, 1)), computed once."""
    if (C, n) not in _cache:
        _cache[(C, n)] = vnp.clean_case(100 * C + n, n, C, 0.1, keypts_num=2, cube=0.4, noise=1.6)
    return _cache[(C, n)]


def _run(device, case, n=None, **kw):
    from d3feat_amd.validation import validation_pairs
    f, s, x, ai, pi = case
    return validation_pairs(_dev(f, device), _dev(s, device), _dev(x, device), _dev(ai, device), _dev(pi, device), n, **kw)


def _check(values, want, C, what):
    """One row f32[8] of PairValidation.values against validation_np.figures."""
    values = np.asarray(values, np.float64)
    if want["skipped"]:
        assert values[:6].tolist() == list(vnp.SKIP), (what, values)
        return
    tol = vnp.tolerances(C, want["Dmax"], want["smax"])
    for k, name in enumerate(FIG):
        if name == "accuracy":
            continue
        err = abs(values[k] - want[name])
        print("%s %-11s got %.9g want %.9g err %.2e tol %.2e" % (what, name, values[k], want[name], err, tol[name]))
    assert int(values[6]) == want["accurate"] and int(values[7]) == want["n"], (what, values[6:], want["accurate"])
    assert values[3] == np.float32(want["accurate"]) / np.float32(want["n"]), what
    for k, name in enumerate(FIG):
        if name != "accuracy":
            assert abs(values[k] - want[name]) <= tol[name], (what, name, values[k], want[name], tol[name])


def test_the_fixture_of_the_reference(device):
    """The pairs the reference's loss.py evaluated: six figures within the stored tolerances (4 x the reference's own float32
    deviation from float64), accurate-row counts equal, split means as utils/trainer.py:442-471 computes them."""
    from d3feat_amd.validation import validation_pairs
    z = np.load(os.path.join(GOLDEN, "validation.npz"))
    P = len(z["n"])
    got, st = [], []
    for kn in sorted(set(z["keypts_num"].tolist())):              # keypts_num is a parameter of the call: one call per value
        out = validation_pairs(_dev(z["features"], device), _dev(z["scores"], device), _dev(z["points"], device),
                               _dev(z["anc_idx"], device), _dev(z["pos_idx"], device), _dev(z["n"], device), _dev(z["row0"], device),
                               safe_radius=float(z["safe_radius"]), keypts_num=int(kn), det_loss_weight=float(z["det_loss_weight"]))
        got.append((kn, out.values.cpu().numpy(), out))
        st.append(out.status.cpu().numpy())
    assert not np.any(st)
    values = np.stack([next(v for kn, v, _ in got if kn == z["keypts_num"][p])[p] for p in range(P)])
    ref, tol = z["reference"].astype(np.float64), z["tolerance"]
    for p in range(P):
        for k, name in enumerate(FIG):
            print("pair %d %-11s got %.9g reference %.9g diff %.2e tol %.2e" % (p, name, values[p, k], ref[p, k],
                                                                              abs(values[p, k] - ref[p, k]), tol[k]))
    for p in range(P):
        n = int(z["n"][p])
        if ref[p, 3] >= 0:
            assert int(values[p, 6]) == int(round(ref[p, 3] * n)), (p, values[p, 6], ref[p, 3] * n)
        for k, name in enumerate(FIG):
            assert abs(values[p, k] - ref[p, k]) <= tol[k], (p, name, values[p, k], ref[p, k], tol[k])
    # the split means of ONE call, keypts_num = 256: it evaluates the pairs the fixture evaluated at 256 and skips every other (their
    # n is below 128) -- exactly the device's own figures averaged as the trainer does, and within the tolerances of the reference's
    kn, v, out = got[-1]
    assert kn == 256
    have = out.means()
    own = vnp.split_means(v[:, [0, 2, 3, 4, 5]].astype(np.float64))
    assert np.allclose(have, own, rtol=1e-12, atol=0, equal_nan=True), (have, own)
    expect = np.where(z["keypts_num"][:, None] == 256, ref, np.asarray(vnp.SKIP)[None])
    assert (expect[:, 3] > 0).sum() >= 2 and (expect[:, 3] < 0).sum() >= 2
    want = vnp.split_means(expect[:, [0, 2, 3, 4, 5]])
    print("split means", have, "reference", want)
    assert all(abs(h - w) <= t for h, w, t in zip(have, want, tol[[0, 2, 3, 4, 5]] + 1e-15))


@pytest.mark.parametrize("C", [16, 32, 64])
def test_size_grid_against_float64(device, C):
    """n around the 64-row tiles, the 256-thread strides and the largest list, every descriptor width: each pair alone from separate
    arrays, then all of them in ONE call as column views of [xyz | desc | score] records with row0."""
    from d3feat_amd.validation import validation_pairs, validation_records
    recs, lens, anc, pos, masked = [], [], np.zeros((len(GRID_N), 1024), np.int32), np.zeros((len(GRID_N), 1024), np.int32), []
    alone = []
    for k, n in enumerate(GRID_N):
        case, want, _ = _grid_case(C, n)
        f, s, x, ai, pi = case
        out = _run(device, case, keypts_num=2)
        v = out.values.cpu().numpy()[0]
        _check(v, want, C, "C=%d n=%d alone" % (C, n))
        assert int(out.status.item()) == 0
        alone.append(v)
        if n >= 63:
            masked.append(want["masked"])
        recs.append(np.concatenate([x, f, s[:, None]], 1))
        lens += [n + 7, n + 5]
        anc[k, :n], pos[k, :n] = ai, pi
    assert min(masked) >= 0.02                                    # the safe radius does mask a few percent of every case
    rec = _dev(np.concatenate(recs).astype(np.float32), device)
    assert rec.shape[1] == C + 4
    nd = _dev(np.asarray(GRID_N, np.int32), device)
    out = validation_records(rec, lens, _dev(anc, device), _dev(pos, device), nd, keypts_num=2)
    assert out._inputs[0].data_ptr() == rec.data_ptr() + 12        # a view: no copy was made
    v = out.values.cpu().numpy()
    assert np.array_equal(v.view(np.uint32), np.stack(alone).view(np.uint32))      # the same arithmetic whatever the layout
    row0 = np.concatenate([[0], np.cumsum(np.asarray(lens).reshape(-1, 2).sum(1))]).astype(np.int32)
    out2 = validation_pairs(rec[:, 3:3 + C], rec[:, 3 + C:], rec[:, :3], _dev(anc, device), _dev(pos, device), nd, _dev(row0, device),
                            keypts_num=2)
    assert torch.equal(out2.values.view(torch.int32), out.values.view(torch.int32)) and torch.equal(out2.sums, out.sums)


def test_every_negative_masked(device):
    """All keypoints inside the safe radius: every negative is a false negative, each contributes exp(0) and lse = log n; the closest
    negative still counts for the accuracy and the contrastive loss."""
    case, want, _ = vnp.clean_case(7, 70, 32, 0.1, cube=0.05, noise=1.6)
    assert want["masked"] == 1.0 and np.allclose(want["lse"], np.log(70), rtol=1e-15) and 0 < want["accuracy"] < 1
    v = _run(device, case, keypts_num=2).values.cpu().numpy()[0]
    _check(v, want, 32, "all masked")
    assert v[5] == 0.0
    fp = want["fp"]
    assert abs(v[0] - np.mean(vnp.softplus(25 * (fp - 0.1) + np.log(70)) / 25)) <= vnp.tolerances(32, want["Dmax"], want["smax"])["circle"]


def test_duplicated_index_pairs(device):
    """Sampling with replacement repeats (ai, pi) entries: D[i, j] is bit-equal to D[i, i], the difference is exactly 0 and the row
    counts as accurate -- although the two anchors coincide and the entry is a false negative: cn ignores the mask (loss.py:151)."""
    f, s, x, ai, pi = vnp.make_case(21, 96, 32, noise=0.3)             # (noise 0.3: every row is accurate, by a wide margin)
    base = vnp.figures(f, s, x, ai, pi, 0.1, 2)
    assert base["accurate"] == 96
    dup = [(3 * k, 3 * k + 50) for k in range(8)]
    for i, j in dup:
        ai[j], pi[j] = ai[i], pi[i]
    want = vnp.figures(f, s, x, ai, pi, 0.1, 2)
    rows = [r for d in dup for r in d]
    vnp.margins(f, x, ai, pi, 0.1, 32, planted_rows=rows, planted_kd=dup)
    # an exact tie in 16 rows: accurate only because the test is fp - cn <= 0 and the two distances are the same bits; the tied
    # entries are false negatives (the anchors coincide) and still set cn
    assert all(want["fp"][r] == want["cn"][r] for r in rows) and want["accurate"] == 96 and all(want["KD"][i, j] < 0.1 for i, j in dup)
    v = _run(device, (f, s, x, ai, pi), keypts_num=2).values.cpu().numpy()[0]
    _check(v, want, 32, "duplicates")


def test_safe_radius_is_strict(device):
    """r set to the fp32 value of a planted keypoint distance: KD < r is false for it, the pair stays a negative."""
    (f, s, x, ai, pi), _, _ = vnp.clean_case(31, 12, 32, 0.25, noise=1.0)
    x[ai[0]] = (0.125, 0.25, 0.125)
    x[ai[1]] = (0.375, 0.25, 0.125)                                    # 0.25 apart, exactly, in fp32 and in float64
    r = float(np.sqrt(np.float32(0.0625) + np.float32(1e-12), dtype=np.float32))
    assert r == 0.25
    want = vnp.figures(f, s, x, ai, pi, r, 2)
    vnp.margins(f, x, ai, pi, r, 32, planted_kd=[(0, 1)])
    masked = vnp.figures(f, s, x, ai, pi, float(np.nextafter(np.float32(r), np.float32(1))), 2)
    tol = vnp.tolerances(32, want["Dmax"], want["smax"])
    assert abs(masked["d_neg"] - want["d_neg"]) > 100 * tol["d_neg"]    # a <= in the kernel would show
    v = _run(device, (f, s, x, ai, pi), safe_radius=r, keypts_num=2).values.cpu().numpy()[0]
    _check(v, want, 32, "strict radius")


def test_skip_rule_and_tiny_pairs(device):
    """n < 0.5 keypts_num on both sides of the bound (even and odd keypts_num), n = 0, and n = 1 computed as written: cn = fp + 1e5,
    d_neg = 0 * 1 / 0 = NaN as the reference gives."""
    skip = np.asarray(vnp.SKIP, np.float32)
    for kn, n, skipped in ((20, 9, True), (20, 10, False), (21, 10, True), (21, 11, False)):
        case, want, _ = vnp.clean_case(40 + n, n, 16, 0.1, keypts_num=kn)
        assert want["skipped"] == skipped
        out = _run(device, case, keypts_num=kn)
        v = out.values.cpu().numpy()[0]
        _check(v, want, 16, "kn=%d n=%d" % (kn, n))
        assert int(v[7]) == n and int(out.status.item()) == 0
    case = vnp.make_case(50, 5, 16)
    for kn in (0, 2, 256):
        out = _run(device, case, n=0, keypts_num=kn)
        assert np.array_equal(out.values.cpu().numpy()[0, :6], skip) and int(out.status.item()) == 0
    empty = (case[0], case[1], case[2], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert np.array_equal(_run(device, empty, keypts_num=0).values.cpu().numpy()[0, :6], skip)
    f, s, x, ai, pi = case
    out = _run(device, case, n=1, keypts_num=2)
    v = out.values.cpu().numpy()[0].astype(np.float64)
    want = vnp.figures(f, s, x, ai[:1], pi[:1], 0.1, 2)
    assert np.isnan(want["d_neg"]) and want["accurate"] == 1
    tol = vnp.tolerances(16, want["Dmax"], want["smax"])
    # The one figure whose bound is not the descriptor's: cn = fp + 1e5 in fp32 carries half an ulp of 1e5 (2^-8) into the detection
    # term, times the score weight; and the result, of magnitude 1e5 itself, is returned as ONE fp32 number: half an ulp of it (a
    # relative 2^-24, which the bounds of validation_np leave out because it is far below them at magnitudes near 1)
    tol["det"] += 2.0 ** -8 * want["smax"] + 2.0 ** -24 * abs(want["det"])
    have = dict(zip(FIG, v[:6]))
    for name in FIG:
        print("n=1 %-11s got %.9g want %.9g" % (name, have[name], want[name]))
        assert (np.isnan(have[name]) and np.isnan(want[name])) or abs(have[name] - want[name]) <= tol.get(name, 0.0), name
    assert np.isnan(have["d_neg"]) and have["accuracy"] == 1.0
    sums, counts = out.sums.cpu().numpy(), out.counts.cpu().numpy()
    assert np.isnan(sums[5]) and counts[5] == 1                       # NaN != 0: the trainer appends it


def test_index_out_of_range_is_flagged(device):
    """An index -1 or N: status 1 and the skip tuple for that pair, nothing read through it; the neighbours' results untouched."""
    from d3feat_amd import _lib
    from d3feat_amd.validation import validation_pairs
    cases = [vnp.clean_case(60 + k, 40, 32, 0.1)[0] for k in range(3)]
    f, s, x = (np.concatenate([c[i] for c in cases]) for i in range(3))
    row0 = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int32)
    alone = [_run(device, c, keypts_num=2).values.cpu().numpy()[0] for c in cases]
    for bad, where in ((-1, 3), (len(cases[1][0]), 3), (-1, 4), (2 ** 31 - 1, 4)):
        anc, pos = np.stack([c[3] for c in cases]), np.stack([c[4] for c in cases])
        (anc if where == 3 else pos)[1, 17] = bad
        out = validation_pairs(_dev(f, device), _dev(s, device), _dev(x, device), _dev(anc, device), _dev(pos, device), 40,
                               _dev(row0, device), keypts_num=2)
        v, st = out.values.cpu().numpy(), out.status.cpu().numpy()
        assert st.tolist() == [0, _lib.VP_INDEX_RANGE, 0]
        assert v[1, :6].tolist() == list(vnp.SKIP)
        assert np.array_equal(v[0].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(v[2].view(np.uint32), alone[2].view(np.uint32))
        assert out.counts.cpu().numpy()[0] == 2
    # a count beyond the lists: flagged too
    nd = _dev(np.asarray([40, 41, 40], np.int32), device)
    anc, pos = np.stack([c[3] for c in cases]), np.stack([c[4] for c in cases])
    out = validation_pairs(_dev(f, device), _dev(s, device), _dev(x, device), _dev(anc, device), _dev(pos, device), nd, _dev(row0, device),
                           keypts_num=2)
    assert out.status.cpu().numpy().tolist() == [0, _lib.VP_COUNT_RANGE, 0] and out.values.cpu().numpy()[1, :6].tolist() == list(vnp.SKIP)


def test_three_thousand_pairs_and_their_totals(device):
    """P = 3000 pairs of n <= 16 in one call: every pair against float64, and the filtered sums and
    counts of the totals against the per-pair figures.  keypts_num = 16: the pairs with n < 8 are skipped."""
    from d3feat_amd.validation import validation_pairs
    P, C, ld = 3000, 32, 16
    rng = np.random.default_rng(5)
    ns = rng.integers(4, 17, P)
    fs, ss, xs, wants, row0 = [], [], [], [], [0]
    anc, pos = np.zeros((P, ld), np.int32), np.zeros((P, ld), np.int32)
    for p in range(P):
        n = int(ns[p])
        (f, s, x, ai, pi), want, _ = vnp.clean_case(10000 + p, n, C, 0.1, keypts_num=16, n_anchor=18, n_positive=18,
                                                    noise=(0.3, 1.6, 50.0)[p % 3])
        fs.append(f), ss.append(s), xs.append(x), wants.append(want), row0.append(row0[-1] + 36)
        anc[p, :n], pos[p, :n] = ai, pi
    out = validation_pairs(_dev(np.concatenate(fs), device), _dev(np.concatenate(ss), device), _dev(np.concatenate(xs), device),
                           _dev(anc, device), _dev(pos, device), _dev(ns.astype(np.int32), device),
                           _dev(np.asarray(row0, np.int32), device), keypts_num=16)
    v = out.values.cpu().numpy()
    assert not out.status.any().item()
    worst = dict.fromkeys(FIG, 0.0)
    for p in range(P):
        want = wants[p]
        if want["skipped"]:
            assert v[p, :6].tolist() == list(vnp.SKIP), p
            continue
        tol = vnp.tolerances(C, want["Dmax"], want["smax"])
        assert int(v[p, 6]) == want["accurate"], p
        for k, name in enumerate(FIG):
            if name != "accuracy":
                worst[name] = max(worst[name], abs(v[p, k] - want[name]) / tol[name])
    print("largest error / tolerance over the pairs:", worst)
    assert max(worst.values()) <= 1.0, worst
    assert sum(w["skipped"] for w in wants) > 500 and sum((not w["skipped"]) and w["accurate"] == 0 for w in wants) > 10
    sums, counts = out.sums.cpu().numpy(), out.counts.cpu().numpy()
    for k in range(6):
        col = v[:, k].astype(np.float64)
        sel = col > 0 if k == 3 else col != 0
        assert counts[k] == sel.sum(), (k, counts[k], sel.sum())
        assert abs(sums[k] - col[sel].sum()) <= 1e-12 * np.abs(col[sel]).sum(), (k, sums[k], col[sel].sum())
    assert np.allclose(out.means(), vnp.split_means(v[:, [0, 2, 3, 4, 5]]), rtol=1e-12, atol=0)


def test_capture_then_replay_on_other_data(device):
    """The call holds no host decision: captured once, replayed on other descriptors, indices and counts written into the same
    tensors, it gives what an eager call gives, bit for bit."""
    from d3feat_amd import ops
    from d3feat_amd.validation import PairValidation, validation_pairs
    C, ld = 32, 128
    a = [vnp.clean_case(70 + k, n, C, 0.1, n_anchor=140, n_positive=140)[0] for k, n in enumerate((100, 128))]
    b = [vnp.clean_case(80 + k, n, C, 0.1, n_anchor=140, n_positive=140)[0] for k, n in enumerate((128, 65))]

    def pack(cases):
        anc, pos = np.zeros((2, ld), np.int32), np.zeros((2, ld), np.int32)
        for k, c in enumerate(cases):
            anc[k, :len(c[3])], pos[k, :len(c[3])] = c[3], c[4]
        return [np.concatenate([c[i] for c in cases]) for i in range(3)] + [anc, pos, np.asarray([len(c[3]) for c in cases], np.int32)]
    st = [_dev(t, device) for t in pack(a)]
    row0 = _dev(np.asarray([0, 280, 560], np.int32), device)
    out = PairValidation(2, device)
    stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            validation_pairs(*st, row0, keypts_num=2, out=out)        # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                validation_pairs(*st, row0, keypts_num=2, out=out)
    stream.synchronize()
    for cases in (b, a):
        for dst, src in zip(st, pack(cases)):
            dst.copy_(_dev(src, device))
        out.values.fill_(7.0)
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        eager = validation_pairs(*[t.clone() for t in st], row0, keypts_num=2)
        assert torch.equal(out.values.view(torch.int32), eager.values.view(torch.int32))
        assert torch.equal(out.sums, eager.sums) and torch.equal(out.counts, eager.counts) and not out.status.any().item()
        for k, c in enumerate(cases):
            _check(out.values[k].cpu().numpy(), vnp.figures(*c, 0.1, 2), C, "replay pair %d" % k)
    del pw


def test_two_calls_give_equal_bits(device):
    case, _, _ = _grid_case(32, 1024)
    one, two = _run(device, case, keypts_num=2), _run(device, case, keypts_num=2)
    assert torch.equal(one.values.view(torch.int32), two.values.view(torch.int32))
    assert torch.equal(one.sums.view(torch.int64), two.sums.view(torch.int64)) and torch.equal(one.counts, two.counts)


def _golden_flat(g, device, anc=None, pos=None):
    i = g.inputs
    flat = [_dev(p, device) for p in i["points"]] + [_dev(m, device) for m in i["neighbors"]]
    flat += [_dev(m, device) for m in i["pools"]] + [_dev(m, device) for m in i["upsamples"]]
    flat += [_dev(i["features"], device), _dev(i["batch_weights"], device), _dev(i["in_batches"], device), _dev(i["out_batches"], device)]
    flat += [_dev(i["stack_lengths"], device), anc, pos, ["a", "b"], _dev(i["points"][0], device)]
    return flat


def test_model_attributes(device):
    """KernelPointFCNN.run: the five attributes are validation_pairs (P = 1) on the model's own outputs, with safe_radius, keypts_num
    and det_loss_weight of the config; without keypoint indices they are the skip tuple."""
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.validation import validation_pairs
    from oracle.golden_network import GoldenNetwork
    g = GoldenNetwork("3dmatch")
    cfg = g.config()
    cfg.keypts_num, cfg.det_loss_weight, cfg.safe_radius = 64, 1.0, 0.1
    na, nb = (int(v) for v in g.inputs["stack_lengths"])
    rng = np.random.default_rng(3)
    ai = rng.integers(0, na, 200).astype(np.int32)
    pi = (ai + na).astype(np.int32)                                   # the same point of the stack's second copy ...
    pi[::3] = (rng.integers(0, nb, len(pi[::3])) + na).astype(np.int32)   # ... and a third of them wrong
    model = KernelPointFCNN(_golden_flat(g, device, _dev(ai, device), _dev(pi, device)), cfg, weights=dict(g.W))
    five = [model.desc_loss, model.det_loss, model.accuracy, model.ave_d_pos, model.ave_d_neg]
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 0 for t in five)
    want = validation_pairs(model.out_features, model.out_scores, _dev(g.inputs["points"][0], device), _dev(ai, device), _dev(pi, device),
                            safe_radius=0.1, keypts_num=64, det_loss_weight=1.0).values[0].cpu().numpy()
    have = np.asarray([t.item() for t in five], np.float32)
    print("model figures", have.tolist())
    assert np.array_equal(have.view(np.uint32), want[[0, 2, 3, 4, 5]].view(np.uint32))
    assert 0 < have[2] < 1 and have[0] > 0 and have[1] != 0
    f64 = vnp.figures(model.out_features.cpu().numpy(), model.out_scores.cpu().numpy(), g.inputs["points"][0], ai, pi, 0.1, 64)
    tol = vnp.tolerances(32, f64["Dmax"], f64["smax"])
    assert abs(have[0] - f64["circle"]) <= tol["circle"] and abs(have[3] - f64["d_pos"]) <= tol["d_pos"]
    # below half of keypts_num, and without indices (every caller before this feature: None, empty arrays, a host placeholder)
    cfg.keypts_num = 512
    model.run(_golden_flat(g, device, _dev(ai, device), _dev(pi, device)))
    assert [t.item() for t in (model.desc_loss, model.det_loss, model.accuracy, model.ave_d_pos, model.ave_d_neg)] == [0, 0, -1, 0, 0]
    cfg.keypts_num = 64
    for none in (None, np.array([], np.int32), torch.zeros(1, dtype=torch.int32)):
        d, s = model.run(_golden_flat(g, device, none, none))
        assert [t.item() for t in (model.desc_loss, model.det_loss, model.accuracy, model.ave_d_pos, model.ave_d_neg)] == [0, 0, -1, 0, 0]
        assert np.abs(d.cpu().numpy() - g.descriptors).max() <= 1e-4


def test_engine_two_clouds_without_stage0(device):
    """A validation pair arrives at first_subsampling_dl and its indices address those rows: FragmentEngine(two_clouds=True,
    stage0=False) takes the stack [cloud_a; cloud_b] as fed.  Records bit-equal to run_eager, on two crops of the 4000-point golden
    cloud; validation_records on the records equals the array form."""
    from d3feat_amd import ops
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.validation import validation_pairs, validation_records
    from oracle.golden_network import GoldenNetwork
    g = GoldenNetwork("3dmatch_4k")
    cfg = g.config()
    cloud = g.clouds()[0]
    order = np.argsort(cloud[:, 0], kind="stable")
    a, b = np.ascontiguousarray(cloud[np.sort(order[:2600])]), np.ascontiguousarray(cloud[np.sort(order[1400:])])
    eng = FragmentEngine(cfg, dict(g.W), g.limits, n0_cap=6144, level_ratio=0.45, slots=1, device=device, two_clouds=True, stage0=False)
    pair = (_dev(a, device), _dev(b, device))
    eng.submit(0, pair)
    rec = eng.fetch(0, packed=True)
    assert eng.fallbacks == 0 and rec.shape == (len(a) + len(b), 36)
    assert np.array_equal(rec[:, :3].cpu().numpy().view(np.uint32), np.concatenate([a, b]).view(np.uint32))
    want = ops.pack_descriptors(*eng.run_eager(pair))
    diff = (rec - want).abs().max().item()
    print("two_clouds, stage0=False: largest |replay - eager| over the records %.3e" % diff)
    assert torch.equal(rec.view(torch.int32), want.view(torch.int32))
    # indices: points the crops share (the overlap of the two x ranges), as datasets/ThreeDMatch.py:222-229 feeds them
    ia, ib = np.sort(order[:2600]), np.sort(order[1400:])
    common = np.intersect1d(ia, ib)[:256]
    ai = np.searchsorted(ia, common).astype(np.int32)
    pi = (np.searchsorted(ib, common) + len(a)).astype(np.int32)
    kw = dict(safe_radius=0.1, keypts_num=256, det_loss_weight=1.0)
    one = validation_records(rec, [len(a), len(b)], _dev(ai, device), _dev(pi, device), **kw)
    two = validation_pairs(rec[:, 3:35].contiguous(), rec[:, 35].contiguous(), rec[:, :3].contiguous(), _dev(ai, device), _dev(pi, device),
                           **kw)
    assert torch.equal(one.values.view(torch.int32), two.values.view(torch.int32)) and one.values[0, 3].item() > 0
    print("engine pair figures", one.values[0].cpu().numpy().tolist())


def test_validation_split_tool(device, tmp_path):
    """tools/validation_split.py on pickles and a checkpoint the test writes itself, in the layouts of datasets/ThreeDMatch.py:101-136
    and of a training folder: prints the trainer's line."""
    import re
    from conftest import write_tf_bundle
    from oracle.golden_network import GoldenNetwork
    g = GoldenNetwork("3dmatch_4k")
    cloud = g.clouds()[0]
    order = np.argsort(cloud[:, 1], kind="stable")
    ia, ib = np.sort(order[:int(len(cloud) * 0.7)]), np.sort(order[int(len(cloud) * 0.3):])
    assert min(len(ia), len(ib)) >= 2000                               # the generator skips smaller clouds
    common = np.intersect1d(ia, ib)
    corr = np.stack([np.searchsorted(ia, common), np.searchsorted(ib, common)], 1).astype(np.int64)
    with open(tmp_path / "points.pkl", "wb") as f:
        pickle.dump({"scene/seq-01/cloud_bin_0": cloud[ia], "scene/seq-01/cloud_bin_1": cloud[ib]}, f)
    with open(tmp_path / "keypts.pkl", "wb") as f:
        pickle.dump({"scene/seq-01/cloud_bin_0@scene/seq-01/cloud_bin_1": corr}, f)
    os.makedirs(tmp_path / "log" / "snapshots")
    write_tf_bundle(str(tmp_path / "log" / "snapshots" / "snap-3"),
                    {"KernelPointNetwork/" + k: np.asarray(v, np.float32) for k, v in dict(g.W).items()}, crc=False)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "validation_split.py"), "--points", str(tmp_path / "points.pkl"), "--keypts",
           str(tmp_path / "keypts.pkl"), "--weights", str(tmp_path / "log"), "--limits", ",".join(str(int(v)) for v in g.limits),
           "--seed", "1", "--epoch", "7"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("3DMatch Epoch")]
    assert len(line) == 1, r.stdout
    print(line[0])
    m = re.fullmatch(r"3DMatch Epoch +7: desc_loss = (\S+) det_loss = (\S+) accuracy = (\S+)%  d_pos = (\S+) d_neg = (\S+)", line[0])
    assert m, line[0]
    vals = [float(x) for x in m.groups()]
    assert 0 < vals[2] <= 100 and vals[0] > 0 and vals[3] > 0 and vals[4] > 0
