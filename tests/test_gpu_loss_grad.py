"""d3f_loss_gradients / d3feat_amd.validation.loss_gradients on the MI355X: the gradient of desc_loss + det_loss with respect to the
descriptor and score rows, against the float64 definition tests/loss_grad_np.py (itself pinned on the CPU by
tests/test_loss_grad_host.py; the reference cannot emit gradients here).

Tolerance, per case and separately for features and scores: the device's largest absolute difference from float64 is held against
the larger of (a) four times the same difference of the float32 torch-CPU autograd evaluation of the restated loss (recorded in
tests/golden/loss_grad.npz for the size grid, evaluated here for the small planted cases) and (b) loss_grad_np.tolerances, a
first-order worst-case bound derived from the case -- and neither may exceed 1e-4 of the pair's largest gradient entry
(loss_grad_np.cap).  Every input keeps loss_grad_np.margins, except at planted bit-equal ties.

What the device measured against these: the docstring of test_size_grid."""
import os

import numpy as np
import pytest
import torch

import loss_grad_np as lg
import validation_np as vnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
LOSSES = ("circle_loss", "desc_loss")
GRID_N = (1, 2, 63, 64, 65, 256, 1024)
_cache = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _fixture():
    if "z" not in _cache:
        z = np.load(os.path.join(GOLDEN, "loss_grad.npz"))
        _cache["z"] = {tuple(int(v) for v in k): (z["err32"][at], z["largest"][at], int(z["seeds"][at])) for at, k in enumerate(z["keys"])}
    return _cache["z"]


def _grid_case(C, n):
    """The case of the size grid, as tools/make_golden_loss_grad.py makes it; computed once."""
    if (C, n) not in _cache:
        _cache[(C, n)] = lg.clean_case(100 * C + n, n, C, 0.1, cube=0.4, noise=1.6)
    return _cache[(C, n)]


def _run(device, case, n=None, nan=True, **kw):
    """loss_gradients on one pair; the outputs are pre-filled with NaN: every word must be overwritten."""
    from d3feat_amd.validation import PairGradients, loss_gradients
    f, s, x, ai, pi = case
    out = None
    if nan:
        out = PairGradients(1, len(f), f.shape[1], torch.device(device))
        out.features.fill_(float("nan"))
        out.scores.fill_(float("nan"))
        out.values.fill_(float("nan"))
    return loss_gradients(_dev(f, device), _dev(s, device), _dev(x, device), _dev(ai, device), _dev(pi, device), n, out=out, **kw)


def _check(gf, gs, want, ai, pi, C, w, what, err32=None, case=None, loss="circle_loss", r=0.1):
    """Device gradients (numpy) of one pair against loss_grad_np.gradients.  -> the two relative errors."""
    gf, gs = np.asarray(gf, np.float64), np.asarray(gs, np.float64)
    if want["skipped"]:
        assert not gf.any() and not gs.any(), what
        return 0.0, 0.0
    if err32 is None and case is not None:                       # (a), evaluated here: small cases only
        tf, ts = lg.torch_gradients(*case, r, 2, w, loss=loss, dtype="float32")
        err32 = (np.abs(tf - want["features"]).max(), np.abs(ts - want["scores"]).max())
    err32 = (0.0, 0.0) if err32 is None else err32
    bound = lg.tolerances(want, ai, pi, C, w)
    rel = []
    for k, (got, name) in enumerate(((gf, "features"), (gs, "scores"))):
        big = np.abs(want[name]).max()
        tol = lg.cap(max(4 * err32[k], bound[k]), big)
        err = np.abs(got - want[name]).max()                      # (a NaN left in the output makes this NaN: the assertion fails)
        print("%s %-8s largest %.3e  |device - float64| %.2e  float32 torch %.2e  bound %.2e  tolerance %.2e" % (
            what, name, big, err, err32[k], bound[k], tol))
        assert err <= tol, (what, name, err, tol)
        rel.append(err / big if big > 0 else 0.0)
    named = np.zeros(len(gs), bool)
    named[np.asarray(ai)] = named[np.asarray(pi)] = True
    assert not gf[~named].any() and not gs[~named].any(), what    # rows no list names: exactly zero
    if w == 0:
        assert not gs.any(), what
    return tuple(rel)


@pytest.mark.parametrize("C", [16, 32, 64])
def test_size_grid(device, C):
    """n at the tile edges of 64 and at D3F_VALIDATION_NMAX, every descriptor width, both descriptor losses, det_loss_weight 0 and 1,
    the outputs pre-filled with NaN; values and status bit-equal to validation_pairs.  (a) is the fixture's float32 torch figure.
    Measured on the MI355X, the largest |device - float64| over the largest entry, beside the fixture's float32 torch figure:
    features 9.9e-8 (torch 9.6e-8) at n = 1, 2.9e-7 (3.0e-7) at n = 64, 4.1e-7 (4.1e-7) at n = 256, 6.6e-7 (4.5e-7) at n = 1024;
    scores 2.2e-7 (2.2e-7) at n = 2, 6.4e-7 (3.5e-7) at n = 64, 7.9e-7 (4.7e-7) at n = 256, 7.7e-7 (5.1e-7) at n = 1024; no case
    uses more than 0.041 of its tolerance."""
    from d3feat_amd.validation import validation_pairs
    fix = _fixture()
    worst = [0.0, 0.0]
    for n in GRID_N:
        case, DKD, _ = _grid_case(C, n)
        f, s, x, ai, pi = case
        for w in (0.0, 1.0):
            fwd = validation_pairs(_dev(f, device), _dev(s, device), _dev(x, device), _dev(ai, device), _dev(pi, device), keypts_num=2,
                                   det_loss_weight=w)
            for li, loss in enumerate(LOSSES):
                err32, largest, seed = fix[(C, n, li, int(w))]
                assert np.array_equal(vnp.make_case(seed, n, C, cube=0.4, noise=1.6)[0], f)      # the case the fixture measured
                want = lg.gradients(f, s, x, ai, pi, 0.1, 2, w, loss=loss, DKD=DKD)
                assert np.isclose(np.abs(want["features"]).max(), largest[0], rtol=1e-9)
                out = _run(device, case, keypts_num=2, det_loss_weight=w, loss=loss)
                rel = _check(out.features.cpu().numpy(), out.scores.cpu().numpy(), want, ai, pi, C, w,
                             "C=%d n=%d %s w=%d" % (C, n, loss, w), err32=err32)
                worst = [max(a, b) for a, b in zip(worst, rel)]
                assert torch.equal(out.values.view(torch.int32), fwd.values.view(torch.int32)) and torch.equal(out.status, fwd.status)
                assert out.figures(0)[0].item() == fwd.values[0, li].item()
    print("C=%d: largest relative error over the grid: features %.2e scores %.2e" % (C, worst[0], worst[1]))


def _duplicated(seed, n, C):
    """Lists as the loader draws them (replace=True): the same (ai, pi) three times, a positive named by three entries (exact ties in
    cn for the rows whose closest negative it is), a row named by both lists.  The first seed that keeps the margins and has a row
    outside the planted ones whose closest negative is the triple positive.  (noise 0.3: every row is accurate.)"""
    for k in range(40):
        f, s, x, ai, pi = vnp.make_case(seed + 1000 * k, n, C, noise=0.3)
        ai[50], pi[50] = ai[3], pi[3]
        ai[77], pi[77] = ai[3], pi[3]
        pi[11] = pi[13] = pi[12]
        ai[20] = pi[21]
        try:
            # rows 3, 50, 77 have fp == cn bit for bit (the copies of their own positive) and their anchors coincide; so has row 12,
            # and rows 11, 13 would if the triple positive were their closest negative
            lg.margins(f, x, ai, pi, 0.1, C, planted_rows=(3, 50, 77, 11, 12, 13), planted_kd=((3, 50), (3, 77), (50, 77)))
        except AssertionError:
            continue
        ties = lg.gradients(f, s, x, ai, pi, 0.1, 2)["ties"]
        if any(ties[i] == 3 for i in range(n) if i not in (11, 12, 13)):
            return f, s, x, ai, pi
    raise AssertionError("no clean seed")


@pytest.mark.parametrize("loss", LOSSES)
def test_duplicated_entries(device, loss):
    """The equal split among bit-equal minima, and the resolve sum over all entries that name a row (anchor entries, then positive
    entries).  A split that is not equal, or a duplicate that overwrites instead of adding, is an error of the size of an entry."""
    C, n = 32, 96
    case = _duplicated(21, n, C)
    f, s, x, ai, pi = case
    want = lg.gradients(f, s, x, ai, pi, 0.1, 2, 1.0, loss=loss)
    # the two copies of a row's own positive tie for its cn; the triple positive ties three ways where it is the closest negative
    assert all(want["ties"][r] == 2 and want["fp"][r] == want["cn"][r] for r in (3, 50, 77)) and want["ties"].max() == 3
    assert want["D"][20, 21] < 1.1e-6                                  # the row named by both lists meets itself
    out = _run(device, case, keypts_num=2, loss=loss)
    _check(out.features.cpu().numpy(), out.scores.cpu().numpy(), want, ai, pi, C, 1.0, "duplicates %s" % loss, case=case, loss=loss)
    # the rows the duplicates name carry gradients far above the tolerance: a duplicate that overwrote instead of adding would show
    bar = 100 * lg.BAR * np.abs(want["features"]).max()
    # (under the contrastive loss the triple anchor's own terms cancel exactly: fp - cn is identically 0 there)
    assert np.abs(want["features"][pi[12]]).max() > bar and (loss == "desc_loss" or np.abs(want["features"][ai[3]]).max() > bar)


def _hinge_case():
    """n = 5, C = 16: rows on both sides of each contrastive hinge.  Anchors near unit vectors e_i; positive j = e_j minus 0.3 of
    the other anchors' axes, so every negative lies beyond sqrt(2) > m -- except that positive 3 leans towards anchor 2 (cn_2 < m) and
    positive 0 nearly equals anchor 0 (fp_0 < q); positive 4 is placed at D = m - 2e-4 from anchor 1: a live entry just below m."""
    rng = np.random.default_rng(3)
    n, C, m = 5, 16, vnp.NEG_MARGIN
    e = np.eye(C)
    a = e[:n] + 0.02 * rng.standard_normal((n, C))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    p = np.stack([e[j] - 0.3 * (e[:n].sum(0) - e[j]) for j in range(n)]) + 0.02 * rng.standard_normal((n, C))
    p[0] = a[0] + 0.01 * rng.standard_normal(C)
    p[3] = e[3] + 0.5 * e[2]
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    c = 1 - (m - 2e-4) ** 2 / 2                                        # a_1 . p_4 for |a_1 - p_4| = m - 2e-4
    u = e[9] - (e[9] @ a[1]) * a[1]
    p[4] = c * a[1] + np.sqrt(1 - c * c) * u / np.linalg.norm(u)
    f = np.concatenate([a, rng.standard_normal((2, C)), p]).astype(np.float32)
    x = rng.uniform(0, 2.0, (len(f), 3)).astype(np.float32)             # far apart: nothing is masked
    s = rng.uniform(0.05, 1.0, len(f)).astype(np.float32)
    return f, s, x, np.arange(n, dtype=np.int32), (np.arange(n) + n + 2).astype(np.int32)


def test_planted_hinges(device):
    """Both sides of fp - q and of m - cn (make_case never comes near them: fp is about 0.3 and cn below 1.4), and a live entry with D
    just below m, whose factor (m - D) is 2e-4."""
    case = _hinge_case()
    f, s, x, ai, pi = case
    lg.margins(f, x, ai, pi, 0.1, 16)
    for loss in LOSSES:
        for w in (0.0, 1.0):
            want = lg.gradients(f, s, x, ai, pi, 0.1, 2, w, loss=loss)
            q, m = vnp.POS_MARGIN, vnp.NEG_MARGIN
            assert (want["fp"] < q).any() and (want["fp"] > q).any() and (want["cn"] > m).any() and (want["cn"] < m).any()
            d32 = np.sqrt(np.float32(((f[ai[1]] - f[pi[4]]) ** 2).sum()))
            assert want["live"][1, 4] and 0 < m - want["D"][1, 4] < 1e-3 and d32 < np.float32(m)
            out = _run(device, case, keypts_num=2, det_loss_weight=w, loss=loss)
            _check(out.features.cpu().numpy(), out.scores.cpu().numpy(), want, ai, pi, 16, w, "hinges %s w=%d" % (loss, w), case=case, loss=loss)


def test_every_negative_masked(device):
    """All keypoints inside the safe radius: no entry is live, the circle term is its diagonal alone; cn and its ties ignore the mask."""
    case, DKD, _ = lg.clean_case(7, 70, 32, 0.1, cube=0.05, noise=1.6)
    f, s, x, ai, pi = case
    for loss in LOSSES:
        want = lg.gradients(f, s, x, ai, pi, 0.1, 2, 1.0, loss=loss, DKD=DKD)
        assert not want["live"].any()
        out = _run(device, case, keypts_num=2, loss=loss)
        _check(out.features.cpu().numpy(), out.scores.cpu().numpy(), want, ai, pi, 32, 1.0, "all masked %s" % loss, case=case, loss=loss)


def test_safe_radius_is_strict(device):
    """r set to the fp32 value of a planted keypoint distance: KD < r is false for it and the entry stays live."""
    (f, s, x, ai, pi), (D, _), _ = lg.clean_case(31, 12, 32, 0.25, noise=1.0)
    j = 1 + int(np.argmin(D[0, 1:]))                                   # the closest negative of row 0: well below m, a live entry
    x[ai[0]] = (0.125, 0.25, 0.125)
    x[ai[j]] = (0.375, 0.25, 0.125)                                    # 0.25 apart, exactly, in fp32 and in float64
    r = 0.25
    case = (f, s, x, ai, pi)
    lg.margins(f, x, ai, pi, r, 32, planted_kd=[(0, j)])
    want = lg.gradients(f, s, x, ai, pi, r, 2, 0.0)
    masked = lg.gradients(f, s, x, ai, pi, float(np.nextafter(np.float32(r), np.float32(1))), 2, 0.0)
    assert want["live"][0, j] and not masked["live"][0, j]
    tol = lg.cap(lg.tolerances(want, ai, pi, 32, 0.0)[0], np.abs(want["features"]).max())
    assert np.abs(masked["features"] - want["features"]).max() > 100 * tol      # a <= in the kernel would show
    out = _run(device, case, safe_radius=r, keypts_num=2, det_loss_weight=0.0)
    _check(out.features.cpu().numpy(), out.scores.cpu().numpy(), want, ai, pi, 32, 0.0, "strict radius", case=case, r=r)


def _pack(cases, ld):
    anc, pos = np.zeros((len(cases), ld), np.int32), np.zeros((len(cases), ld), np.int32)
    for k, c in enumerate(cases):
        anc[k, :len(c[3])], pos[k, :len(c[3])] = c[3], c[4]
    row0 = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int32)
    return [np.concatenate([c[i] for c in cases]) for i in range(3)] + [anc, pos, np.asarray([len(c[3]) for c in cases], np.int32), row0]


def test_ragged_pairs_status_and_one_call_against_many(device):
    """41 pairs of ragged n in ONE call -- among them a pair under the skip rule, a pair with n = 0 and a pair with an index out of
    range: zero gradients and the forward's status for those, every other pair against float64, values / status bit-equal to
    validation_pairs, and the bits of 41 calls of one pair each.  Then no pairs at all: zeros."""
    from d3feat_amd import _lib
    from d3feat_amd.validation import PairGradients, loss_gradients, validation_pairs
    C, ld, kn = 32, 160, 20
    rng = np.random.default_rng(9)
    ns = [int(v) for v in rng.integers(10, 150, 41)]
    ns[4], ns[17] = 7, 64                                              # 7 < 0.5 * 20: skipped
    cases = [lg.clean_case(500 + k, n, C, 0.1, noise=(0.3, 1.0, 1.6)[k % 3])[0] for k, n in enumerate(ns)]
    f, s, x, anc, pos, nd, row0 = _pack(cases, ld)
    nd[9] = 0
    anc[17, 33] = len(cases[17][0])                                    # one past the pair's rows
    st = [_dev(t, device) for t in (f, s, x, anc, pos, nd, row0)]
    out = PairGradients(41, len(f), C, torch.device(device))
    out.features.fill_(float("nan"))
    out.scores.fill_(float("nan"))
    loss_gradients(*st, keypts_num=kn, out=out)
    fwd = validation_pairs(*st, keypts_num=kn)
    assert torch.equal(out.values.view(torch.int32), fwd.values.view(torch.int32)) and torch.equal(out.status, fwd.status)
    status = out.status.cpu().numpy()
    assert status.tolist() == [_lib.VP_INDEX_RANGE if p == 17 else 0 for p in range(41)]
    gf, gs = out.features.cpu().numpy(), out.scores.cpu().numpy()
    for p, c in enumerate(cases):
        lo, hi = int(row0[p]), int(row0[p + 1])
        if p in (4, 9, 17):
            assert not gf[lo:hi].any() and not gs[lo:hi].any(), p
            assert out.values[p, 3].item() == -1.0
            continue
        want = lg.gradients(*c, 0.1, kn, 1.0)
        _check(gf[lo:hi], gs[lo:hi], want, c[3], c[4], C, 1.0, "pair %d n=%d" % (p, ns[p]), case=c if p % 8 == 0 else None)
        one = loss_gradients(*[_dev(t, device) for t in c], keypts_num=kn)
        assert np.array_equal(one.features.cpu().numpy().view(np.uint32), gf[lo:hi].view(np.uint32)), p
        assert np.array_equal(one.scores.cpu().numpy().view(np.uint32), gs[lo:hi].view(np.uint32)), p
        assert torch.equal(one.values.view(torch.int32), out.values[p:p + 1].view(torch.int32))
    # no pairs: every word is still written
    out0 = PairGradients(0, len(f), C, torch.device(device))
    out0.features.fill_(float("nan"))
    out0.scores.fill_(float("nan"))
    loss_gradients(st[0], st[1], st[2], st[3][:0], st[4][:0], st[5][:0], st[6][:1], keypts_num=kn, out=out0)
    assert not out0.features.any().item() and not out0.scores.any().item()


def test_two_calls_give_equal_bits(device):
    case, _, _ = _grid_case(32, 1024)
    one, two = _run(device, case, keypts_num=2), _run(device, case, nan=False, keypts_num=2)
    assert torch.equal(one.features.view(torch.int32), two.features.view(torch.int32))
    assert torch.equal(one.scores.view(torch.int32), two.scores.view(torch.int32))
    assert torch.equal(one.values.view(torch.int32), two.values.view(torch.int32))


def test_capture_then_replay_on_other_data(device):
    """The call holds no host decision: captured once, replayed on other descriptors, indices and counts written into the same
    tensors, it gives what an eager call gives, bit for bit."""
    from d3feat_amd import ops
    from d3feat_amd.validation import PairGradients, loss_gradients
    C, ld = 32, 128
    a = [lg.clean_case(70 + k, n, C, 0.1, n_anchor=140, n_positive=140)[0] for k, n in enumerate((100, 128))]
    b = [lg.clean_case(80 + k, n, C, 0.1, n_anchor=140, n_positive=140)[0] for k, n in enumerate((128, 65))]
    st = [_dev(t, device) for t in _pack(a, ld)]
    out = PairGradients(2, 560, C, torch.device(device))
    stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            loss_gradients(*st, keypts_num=2, out=out)                 # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                loss_gradients(*st, keypts_num=2, out=out)
    stream.synchronize()
    for cases in (b, a):
        for dst, src in zip(st, _pack(cases, ld)):
            dst.copy_(_dev(src, device))
        out.features.fill_(float("nan"))
        out.scores.fill_(7.0)
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        eager = loss_gradients(*[t.clone() for t in st], keypts_num=2)
        assert torch.equal(out.features.view(torch.int32), eager.features.view(torch.int32))
        assert torch.equal(out.scores.view(torch.int32), eager.scores.view(torch.int32))
        assert torch.equal(out.values.view(torch.int32), eager.values.view(torch.int32)) and not out.status.any().item()
        gf, gs = out.features.cpu().numpy(), out.scores.cpu().numpy()
        for k, c in enumerate(cases):
            want = lg.gradients(*c, 0.1, 2, 1.0)
            _check(gf[280 * k:280 * k + 280], gs[280 * k:280 * k + 280], want, c[3], c[4], C, 1.0, "replay pair %d" % k)
    del pw


def test_column_views_of_a_record_block_in_and_out(device):
    """[xyz | desc | score] records in, and the gradients written into the descriptor and score columns of a block of the same shape:
    no copy is made, the xyz columns are left alone, and the bits are those of the call on separate arrays."""
    from d3feat_amd.validation import loss_gradients, loss_gradients_records
    C = 16
    cases = [lg.clean_case(900 + k, n, C, 0.1, noise=1.0)[0] for k, n in enumerate((65, 30, 130))]
    f, s, x, anc, pos, nd, row0 = _pack(cases, 130)
    rec = _dev(np.concatenate([x, f, s[:, None]], 1).astype(np.float32), device)
    lens = [v for c in cases for v in (len(c[3]) + 7, len(c[3]) + 5)]
    grad = torch.full_like(rec, float("nan"))
    grad[:, :3] = 7.0
    out = loss_gradients_records(rec, lens, _dev(anc, device), _dev(pos, device), _dev(nd, device), keypts_num=2, out_records=grad)
    assert out._inputs[0].data_ptr() == rec.data_ptr() + 12            # a view: no copy was made
    assert out.features.data_ptr() == grad.data_ptr() + 12 and out.scores.data_ptr() == grad.data_ptr() + 4 * (3 + C)
    g = grad.cpu().numpy()
    assert (g[:, :3] == 7.0).all() and not np.isnan(g).any()
    sep = loss_gradients(_dev(f, device), _dev(s, device), _dev(x, device), _dev(anc, device), _dev(pos, device), _dev(nd, device),
                         _dev(row0, device), keypts_num=2)
    assert np.array_equal(g[:, 3:3 + C].view(np.uint32), sep.features.cpu().numpy().view(np.uint32))
    assert np.array_equal(g[:, 3 + C].view(np.uint32), sep.scores.cpu().numpy().view(np.uint32))
    assert torch.equal(out.values.view(torch.int32), sep.values.view(torch.int32))
    for k, c in enumerate(cases):
        want = lg.gradients(*c, 0.1, 2, 1.0)
        lo, hi = int(row0[k]), int(row0[k + 1])
        _check(g[lo:hi, 3:3 + C], g[lo:hi, 3 + C], want, c[3], c[4], C, 1.0, "records pair %d" % k, case=c)
