"""ops.ind_max_pool_backward and ops.closest_pool_cat_backward on the device against tests/pool_grad_np.py on the SAME float32 inputs, so
ties are the same ties on both sides (equality of values does not change when float32 is widened).

Bar: (L + 4) * 2^-24 of the largest entry of the gradient, L the longest segment of the transposed table: one rounding per term
(gs = g / T), one per addition of the fp32 chain, the shadow share (a rounded product per term, a float64 sum, one rounded division, one
addition).  Max pooling: fine rows 281, pooled rows 90, K in (1, 7, 40) -- below, at and beyond the forward's batches of eight and a
wavefront's 32 -- C in (1, 3, 4, 64, 130): both access paths, one and three column blocks.  Capacities above the device-resident
counts, sentinel rows beyond; a fine row named by every pooled row but two (an 88-edge segment), one named by none, and the tie cases of
the host file (pool_grad_np.pool_case); a 90-edge segment in a case of its own.  Upsampling: coarse rows 50, fine rows 300, C1 in
(1, 4, 32, 130), C2 in (0, 32).

Beyond one slice of pooled rows (slices of 256 rows, doubled until 128 cover the capacity; the last workgroup of the row kernel folds the
float64 partials of the shadow share over the slices of pooled rows, and the column minima over the slices of fine rows): fine rows
3 * 256 + 25, pooled rows 2 * 256 + 7, K = 7, C in (3, 64, 130), tie rows and all-shadow pooled rows in every slice, a column minimum
held in the last slice of fine rows only, a shadow share every pooled slice feeds (pool_grad_np.sliced_pool_case), the longest segment
85; the same at capacities a whole slice above the counts (a trailing slice that leaves at once on either side); a capacity of
128 * 256 + 1 rows on the fine and on the pooled side (slices of 512 rows); a column whose zeros are +0 in the first slice of fine rows
and -0 beyond (one minimum as values: M counts both, both take the share, colmin comes back as -0); capture at 500 / 300 rows, replay
at 793 / 519, 200 / 100 and 500 / 300 rows.  Tried once, never committed: with the last workgroup adding only slice 0 of the partials,
the six sliced cases, the zero case and the replay fail (the others pass).  With the code as it is every test passes: no defect found.

Measured on an MI355X (printed, never used as a bar): over the 15 max-pooling and 8 upsampling cases the largest deviation is 5.4e-7 of
the largest entry (upsampling, C1 = 32, a 263-edge segment), at most 0.056 of the bar; every equal-bits comparison holds.  The sliced
cases: 1.8e-7 / 1.5e-7 / 1.1e-7 of the largest entry at C = 3 / 64 / 130 (0.034 / 0.028 / 0.021 of the bar), the same at the larger
capacities; at the 512-row slices 1.3e-7 (C = 64) and 1.6e-7 (C = 3), 0.030 of the bar at most; the zero column's cases 5.7e-8 and
8.4e-8 (0.016); the replays 1.7e-7, 8.1e-8 and 9.7e-8 (0.03 of the bar at most).  The 36 tests take 3 s."""
import numpy as np
import pytest
import torch

import pool_grad_np as pg
from conftest import bits

pytestmark = pytest.mark.gpu

N1, N2, PAD1, PAD2 = 281, 90, 7, 5
U1, U2 = 50, 300


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _count(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


def _same(a, b):
    return np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


def _view(t, lead, trail, fill=float("nan")):
    """t as a column view of a wider block (leading dimension > columns); lead = 4 keeps 16-byte alignment, lead = 1 breaks it."""
    block = torch.full((t.shape[0], lead + t.shape[1] + trail), fill, dtype=t.dtype, device=t.device)
    block[:, lead:lead + t.shape[1]] = t
    v = block[:, lead:lead + t.shape[1]]
    for k in ("n_dev", "n_hint"):
        if hasattr(t, k):
            setattr(v, k, getattr(t, k))
    return v


def _pool_operands(seed, K, C, dev):
    """Capacity-sized operands: x rows beyond the count hold -1e30 (read, they would become the column minimum), index rows beyond name
    row 0 (read, they would lengthen its segment), y / grad_y rows beyond are NaN."""
    from d3feat_amd import ops
    x, inds, g = pg.pool_case(seed, N1, N2, K, C)
    xc = np.concatenate([x, np.full((PAD1, C), -1e30, np.float32)])
    ic = np.concatenate([inds, np.zeros((PAD2, K), np.int32)])
    gc = np.concatenate([g, np.full((PAD2, C), np.nan, np.float32)])
    a = dict(x=_t(xc, dev), inds=_t(ic, dev), g=_t(gc, dev))
    a["x"].n_dev, a["inds"].n_dev = _count(N1, dev), _count(N2, dev)
    a["y"] = ops.ind_max_pool(a["x"], a["inds"])
    y = a["y"][:N2].cpu().numpy()
    assert np.array_equal(bits(y), bits(pg.max_pool_forward(x, inds)))
    return a, x, inds, y, g


@pytest.mark.parametrize("C", [1, 3, 4, 64, 130])
@pytest.mark.parametrize("K", [1, 7, 40])
def test_max_pool_backward_against_float64(device, K, C):
    from d3feat_amd import ops
    a, x, inds, y, g = _pool_operands(100 * K + C, K, C, device)
    want = pg.max_pool_backward(x, inds, y, g, parts=True)
    L = pg.longest_segment(inds, N1)
    assert L >= N2 - 2 and want["shadow_ties"].max() >= 1 and (want["M"][:2] >= 1).all() and want["T"].max() >= min(K, 2)
    out = torch.full((N1 + PAD1, C), float("nan"), device=device)
    out.n_dev = a["x"].n_dev
    got = ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"], out=out)
    assert got.data_ptr() == out.data_ptr() and torch.isnan(out[N1:]).all()                    # sentinel rows left alone
    gx = out[:N1].cpu().numpy()
    big = np.abs(want["gx"]).max()
    err = np.abs(gx - want["gx"]).max()
    print("K %d C %d: longest segment %d, largest %.3e, deviation %.2e (bar %.2e)" % (K, C, L, big, err, (L + 4) * 2.0 ** -24 * big))
    assert np.isfinite(gx).all() and err <= (L + 4) * 2.0 ** -24 * big
    # rows nobody names: exactly the shadow share or zero
    named = np.zeros(N1, bool)
    named[inds[(inds >= 0) & (inds < N1)]] = True
    holds = x[~named] == want["colmin"]
    assert not named[4] and not gx[~named][~holds].any()
    for c in range(C):                                                 # (one share per column, the same bits in every row that takes it)
        assert len(set(bits(gx[~named][:, c][holds[:, c]]).tolist())) <= 1
    # two calls; a table passed in; column views on both access paths: equal bits
    again = ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"])
    assert _same(again[:N1], out[:N1])
    table = ops.neighbor_transpose_supports(a["inds"], N1 + PAD1, a["inds"].n_dev, a["x"].n_dev)
    start, edges = pg.transpose_np(inds, N1)
    assert np.array_equal(table[0].cpu().numpy()[:N1 + 1], start) and np.array_equal(table[1].cpu().numpy()[:len(edges)], edges)
    passed = ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"], transpose=table)
    assert _same(passed[:N1], out[:N1])
    for lead in (4, 1):
        wide = torch.full((N1 + PAD1, C + 8), float("nan"), device=device)
        o = wide[:, lead:lead + C]
        o.n_dev = a["x"].n_dev
        ops.ind_max_pool_backward(_view(a["x"], lead, 4 - lead, -1e30), a["inds"], _view(a["y"], lead, 8 - lead), _view(a["g"], lead, 4 - lead),
                                  transpose=table, out=o)
        assert _same(o[:N1], out[:N1]), lead
        assert torch.isnan(wide[:, :lead]).all() and torch.isnan(wide[:, lead + C:]).all() and torch.isnan(wide[N1:]).all()


def test_fine_row_named_by_every_pooled_row(device):
    """A 90-edge segment: every pooled row names fine row 3 in its first slot (no planted tie rows in the way), K = 7, C = 64 and 3."""
    from d3feat_amd import ops
    for C in (64, 3):
        x, inds, g = pg.pool_case(900 + C, N1, N2, 7, C, ties=False)
        inds[:, 0] = 3
        inds[:, 1:][inds[:, 1:] == 3] = 8
        xt, it, gt = _t(x, device), _t(inds, device), _t(g, device)
        y = ops.ind_max_pool(xt, it)
        want = pg.max_pool_backward(x, inds, y.cpu().numpy(), g)
        assert pg.longest_segment(inds, N1) == N2 == 90
        got = ops.ind_max_pool_backward(xt, it, y, gt).cpu().numpy()
        big, err = np.abs(want).max(), np.abs(got - want).max()
        print("C %d: 90-edge segment, largest %.3e, deviation %.2e (bar %.2e)" % (C, big, err, 94 * 2.0 ** -24 * big))
        assert err <= 94 * 2.0 ** -24 * big and np.abs(got[3] - want[3]).max() <= 94 * 2.0 ** -24 * big


def test_max_pool_backward_without_pooled_rows_writes_zeros(device):
    from d3feat_amd import ops
    a, x, inds, y, g = _pool_operands(7, 7, 5, device)
    for case in ("count", "capacity", "K"):
        out = torch.full((N1 + PAD1, 5), float("nan"), device=device)
        out.n_dev = a["x"].n_dev
        if case == "count":
            idx = a["inds"].clone()
            idx.n_dev = _count(0, device)
            ops.ind_max_pool_backward(a["x"], idx, a["y"], a["g"], out=out)
        elif case == "capacity":
            ops.ind_max_pool_backward(a["x"], a["inds"][:0], a["y"][:0], a["g"][:0], out=out)
        else:
            ops.ind_max_pool_backward(a["x"], a["inds"][:, :0], a["y"], a["g"], out=out)
        assert (out[:N1] == 0).all() and torch.isnan(out[N1:]).all(), case


def _upsample_operands(seed, C1, C2, dev):
    inds, g = pg.upsample_case(seed, U1, U2, 3, C1, C2)
    ic = np.concatenate([inds, np.zeros((PAD2, 3), np.int32)])
    gc = np.concatenate([g, np.full((PAD2, C1 + C2), np.nan, np.float32)])
    a = dict(inds=_t(ic, dev), g=_t(gc, dev))
    a["inds"].n_dev = _count(U2, dev)
    return a, inds, g


@pytest.mark.parametrize("C2", [0, 32])
@pytest.mark.parametrize("C1", [1, 4, 32, 130])
def test_upsample_backward_against_float64(device, C1, C2):
    from d3feat_amd import ops
    a, inds, g = _upsample_operands(10 * C1 + C2, C1, C2, device)
    want, _ = pg.upsample_cat_backward(g, inds, U1, C1)
    L = pg.longest_segment(inds[:, :1], U1)
    first = inds[:, 0]
    assert L >= 230 and ((first < 0) | (first >= U1)).sum() >= 2 and not (first == 2).any()
    out = torch.full((U1 + PAD1, C1), float("nan"), device=device)
    out.n_dev = _count(U1, device)
    got = ops.closest_pool_cat_backward(a["g"], a["inds"], U1 + PAD1, C1, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.isnan(out[U1:]).all()
    gx = out[:U1].cpu().numpy()
    big, err = np.abs(want).max(), np.abs(gx - want).max()
    print("C1 %d C2 %d: longest segment %d, largest %.3e, deviation %.2e (bar %.2e)" % (C1, C2, L, big, err, (L + 4) * 2.0 ** -24 * big))
    assert np.isfinite(gx).all() and err <= (L + 4) * 2.0 ** -24 * big and not gx[2].any()
    again = ops.closest_pool_cat_backward(a["g"], a["inds"], U1 + PAD1, C1, out=torch.empty_like(out).copy_(out))
    assert _same(again[:U1], out[:U1])
    # the table of the one-column view (its leading dimension is the full width), passed in
    col = a["inds"][:, :1]
    assert col.stride(0) == 3
    table = ops.neighbor_transpose_supports(col, U1 + PAD1, a["inds"].n_dev, out.n_dev)
    start, edges = pg.transpose_np(inds[:, :1], U1)
    assert np.array_equal(table[0].cpu().numpy()[:U1 + 1], start) and np.array_equal(table[1].cpu().numpy()[:len(edges)], edges)
    for lead in (4, 1):                                                # grad_out and out as column views, both access paths
        wide = torch.full((U1 + PAD1, C1 + 8), float("nan"), device=device)
        o = wide[:, lead:lead + C1]
        o.n_dev = out.n_dev
        ops.closest_pool_cat_backward(_view(a["g"], lead, 4 - lead), a["inds"], U1 + PAD1, C1, transpose=table, out=o)
        assert _same(o[:U1], out[:U1]), lead
        assert torch.isnan(wide[:, :lead]).all() and torch.isnan(wide[:, lead + C1:]).all() and torch.isnan(wide[U1:]).all()
    # no fine row: zeros
    none = a["inds"].clone()
    none.n_dev = _count(0, device)
    z = torch.full((U1, C1), float("nan"), device=device)
    ops.closest_pool_cat_backward(a["g"], none, U1, C1, out=z)
    assert (z == 0).all()


def test_capture_then_replay_on_other_gradients(device):
    """Tables and both backward operators hold no host decision: captured once in a single-stream torch.cuda.graph, replayed on other
    gradients written into the same tensors, they give the bits of direct calls."""
    from d3feat_amd import ops
    a, x, inds, y, g = _pool_operands(11, 7, 64, device)
    u, uinds, ug = _upsample_operands(12, 32, 32, device)
    gx = torch.zeros((N1 + PAD1, 64), device=device)
    gx.n_dev = a["x"].n_dev
    gu = torch.zeros((U1 + PAD1, 32), device=device)
    gu.n_dev = _count(U1, device)
    stream = torch.cuda.Stream(device=device)

    def call():
        ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"], out=gx)
        ops.closest_pool_cat_backward(u["g"], u["inds"], U1 + PAD1, 32, out=gu)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            call()                                                   # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                call()
    stream.synchronize()
    rng = np.random.default_rng(12)
    for _ in range(2):
        a["g"][:N2].copy_(_t(rng.standard_normal((N2, 64)).astype(np.float32), device))
        u["g"][:U2].copy_(_t(rng.standard_normal((U2, 64)).astype(np.float32), device))
        gx.fill_(float("nan"))
        gu.fill_(float("nan"))
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        want = ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"])
        wantu = torch.empty((U1 + PAD1, 32), device=device)
        wantu.n_dev = gu.n_dev
        ops.closest_pool_cat_backward(u["g"], u["inds"], U1 + PAD1, 32, out=wantu)
        assert _same(gx[:N1], want[:N1]) and _same(gu[:U1], wantu[:U1])
        assert torch.isnan(gx[N1:]).all() and torch.isnan(gu[U1:]).all()
    del pw


# ---- beyond one slice of pooled rows ------------------------------------------------------------------------------------------------
S = 256                                  # common.h: D3F_SLICE_MIN, doubled until at most 128 slices cover the capacity
M1, M2 = 3 * S + 25, 2 * S + 7
LONG = 128 * S + 1                       # the smallest capacity whose slices are 512 rows long


def _at_capacity(case, cap1, cap2, dev, zero_column=None):
    """_pool_operands for a given case and given capacities (the same sentinel rows)."""
    from d3feat_amd import ops
    x, inds, g = case
    (n1, C), (n2, K) = x.shape, inds.shape
    xc = np.concatenate([x, np.full((cap1 - n1, C), -1e30, np.float32)])
    ic = np.concatenate([inds, np.zeros((cap2 - n2, K), np.int32)])
    gc = np.concatenate([g, np.full((cap2 - n2, C), np.nan, np.float32)])
    a = dict(x=_t(xc, dev), inds=_t(ic, dev), g=_t(gc, dev))
    a["x"].n_dev, a["inds"].n_dev = _count(n1, dev), _count(n2, dev)
    a["y"] = ops.ind_max_pool(a["x"], a["inds"])
    y = a["y"][:n2].cpu().numpy()
    ref = pg.max_pool_forward(x, inds)
    keep = [c for c in range(C) if c != zero_column]                 # (a maximum over zeros of both signs has no defined sign)
    assert np.array_equal(y, ref) and np.array_equal(bits(y[:, keep]), bits(ref[:, keep]))
    return a, y


def _held_over_slices(label, a, case, y, dev, views=True):
    """The device's gradient against the float64 reference under the file's bar; sentinel rows left alone; equal bits from a second
    call and from column views on both access paths.  -> (reference parts, gx)."""
    from d3feat_amd import ops
    x, inds, g = case
    (n1, C), cap1 = x.shape, a["x"].shape[0]
    want = pg.max_pool_backward(x, inds, y, g, parts=True)
    L = pg.longest_segment(inds, n1)
    assert L <= 90
    out = torch.full((cap1, C), float("nan"), device=dev)
    out.n_dev = a["x"].n_dev
    ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"], out=out)
    assert torch.isnan(out[n1:]).all()
    gx = out[:n1].cpu().numpy()
    big, err = np.abs(want["gx"]).max(), np.abs(gx - want["gx"]).max()
    bar = (L + 4) * 2.0 ** -24 * big
    print("%s: longest segment %d, largest %.3e, deviation %.2e of it (%.3f of the bar)" % (label, L, big, err / big, err / bar))
    assert np.isfinite(gx).all() and err <= bar, label
    assert _same(ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"])[:n1], out[:n1])
    for lead in (4, 1) if views else ():
        wide = torch.full((cap1, C + 8), float("nan"), device=dev)
        o = wide[:, lead:lead + C]
        o.n_dev = a["x"].n_dev
        ops.ind_max_pool_backward(_view(a["x"], lead, 4 - lead, -1e30), a["inds"], _view(a["y"], lead, 8 - lead), _view(a["g"], lead, 4 - lead), out=o)
        assert _same(o[:n1], out[:n1]), lead
        assert torch.isnan(wide[:, :lead]).all() and torch.isnan(wide[:, lead + C:]).all() and torch.isnan(wide[n1:]).all()
    return want, gx


def _slices(n, s=S):
    return [slice(a, min(a + s, n)) for a in range(0, n, s)]


@pytest.mark.parametrize("extra", [(PAD1, PAD2), (S, S)], ids=["pads", "slice_above"])
@pytest.mark.parametrize("C", [3, 64, 130])
def test_max_pool_backward_over_slices_of_pooled_rows(device, C, extra):
    """Four slices of fine rows and three of pooled rows (the last workgroup of the row kernel folds three float64 partials of the
    shadow share); capacities a whole slice above the counts: a trailing slice on either side that leaves at once."""
    case = pg.pool_case(2000 + C, M1, M2, 7, C, slice_rows=S)
    x, inds, g = case
    a, y = _at_capacity(case, M1 + extra[0], M2 + extra[1], device)
    want, gx = _held_over_slices("C %d, capacities + %s" % (C, extra), a, case, y, device)
    shadow = (inds < 0) | (inds >= M1)
    per_slice = np.stack([(want["shadow_ties"][s] * want["gs"][s]).sum(0) for s in _slices(M2)])
    assert len(per_slice) == 3 and (per_slice != 0).all(0).any()                 # a column whose share every slice feeds
    assert np.abs(want["S"]).max() > 0 and not np.allclose(per_slice[0], want["S"])
    for s in _slices(M2):
        assert shadow[s].all(1).any() and (want["T"][s] >= 2).any()              # all-shadow rows and tie rows in every slice
    assert np.nonzero(x[:, 0] == want["colmin"][0])[0].min() >= 3 * S and want["M"][0] == 1      # held in the last fine slice only
    if C > 1:
        assert want["M"][1] == 3
    holds = x == want["colmin"]
    assert (np.abs(gx[holds]) > 0).any()


@pytest.mark.parametrize("side", ["fine", "pooled"])
def test_max_pool_backward_at_the_doubled_slice_length(device, side):
    """A capacity of 128 * 256 + 1 rows on one side: slices of 512 rows there, 281 real fine rows and 90 real pooled rows."""
    for C in (64, 3):
        case = pg.pool_case(3000 + C, N1, N2, 7, C)
        inds = case[1]
        inds[2:, 0][inds[2:, 0] == 3] = 8                  # (the 88-edge segment goes: the bar's L stays at or below 90 either way)
        a, y = _at_capacity(case, LONG if side == "fine" else N1 + PAD1, LONG if side == "pooled" else N2 + PAD2, device)
        _held_over_slices("C %d, %s capacity %d" % (C, side, LONG), a, case, y, device, views=C == 64)


def test_column_minimum_held_as_zeros_of_both_signs(device):
    """Column 2: non-negative multiples of 1/8 whose zeros are +0 in the first slice of fine rows and -0 beyond.  They are equal values:
    M counts both, both take the share, and the minimum comes back as -0 (the lower of the two in the ordered-integer key)."""
    from d3feat_amd import ops
    for C in (4, 3):
        case = pg.pool_case(4000 + C, M1, M2, 7, C, slice_rows=S, zero_column=2)
        x, inds, g = case
        zero = x[:, 2] == 0
        assert not np.signbit(x[:S, 2][zero[:S]]).any() and zero[:S].any() and np.signbit(x[S:, 2][zero[S:]]).all() and zero[S:].sum() >= 3
        a, y = _at_capacity(case, M1 + PAD1, M2 + PAD2, device, zero_column=2)
        want, gx = _held_over_slices("zeros of both signs, C %d" % C, a, case, y, device)
        assert want["colmin"][2] == 0 and want["M"][2] == zero.sum() and want["S"][2] != 0
        share = want["S"][2] / want["M"][2]
        named = np.zeros(M1, bool)
        named[inds[(inds >= 0) & (inds < M1)]] = True
        lone = zero & ~named
        assert lone[:S].any() and lone[S:].any()                                  # unnamed holders of either sign: the share alone
        assert np.abs(gx[lone, 2] - share).max() <= 8 * 2.0 ** -24 * abs(share) and len(set(bits(gx[lone, 2]).tolist())) == 1
        # the minimum the last workgroup wrote, read from the operator's workspace: ticket, pmin, pcnt, Spart, colmin in the arena order
        # of d3f_ind_max_pool_backward (ph_pool_backward.h, which points back here), 256-byte aligned, slices of 256 rows
        ops.ind_max_pool_backward(a["x"], a["inds"], a["y"], a["g"])
        torch.cuda.synchronize(device)
        al = lambda b: (b + 255) // 256 * 256                                     # noqa: E731
        cap1, cap2 = a["x"].shape[0], a["inds"].shape[0]
        off = al(4) + 2 * al(-(-cap1 // S) * C * 4) + al(-(-cap2 // S) * C * 8)
        ws = ops.workspace(0, device)
        colmin = ws[off:off + 4 * C].clone().view(torch.float32).cpu().numpy()
        assert np.array_equal(colmin, want["colmin"]) and np.signbit(colmin[2]) and not colmin[2]
        assert np.signbit(y[0, 2]) and not y[0, 2]                                # (the forward's shadow row holds the same -0)


def test_capture_then_replay_with_other_row_counts(device):
    """Captured once with 500 fine and 300 pooled rows on the device (two slices each), replayed with 793 / 519 (four and three), with
    200 / 100 (one each) and with 500 / 300 again: the bits of direct calls, and the float64 reference under the bar."""
    from d3feat_amd import ops
    C = 64
    case = pg.pool_case(5000, M1, M2, 7, C, slice_rows=S)
    x, inds, g = case
    a, _ = _at_capacity(case, M1 + PAD1, M2 + PAD2, device)
    n1_dev, n2_dev = a["x"].n_dev, a["inds"].n_dev
    gx = torch.zeros((M1 + PAD1, C), device=device)
    gx.n_dev = n1_dev
    ybuf = torch.zeros_like(a["y"])
    ybuf.n_dev = n2_dev

    def call():
        ops.ind_max_pool_backward(a["x"], a["inds"], ybuf, a["g"], out=gx)

    def set_counts(n1, n2):
        n1_dev.fill_(n1)
        n2_dev.fill_(n2)
        ybuf.fill_(float("nan"))
        ybuf[:n2].copy_(ops.ind_max_pool(a["x"], a["inds"])[:n2])
    stream = torch.cuda.Stream(device=device)
    set_counts(500, 300)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            call()                                                   # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                call()
    stream.synchronize()
    for n1, n2 in ((M1, M2), (200, 100), (500, 300)):
        set_counts(n1, n2)
        gx.fill_(float("nan"))
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        direct = ops.ind_max_pool_backward(a["x"], a["inds"], ybuf, a["g"])
        assert _same(gx[:n1], direct[:n1]) and torch.isnan(gx[n1:]).all(), (n1, n2)
        want = pg.max_pool_backward(x[:n1], inds[:n2], ybuf[:n2].cpu().numpy(), g[:n2])
        L = pg.longest_segment(inds[:n2], n1)
        big, err = np.abs(want).max(), np.abs(gx[:n1].cpu().numpy() - want).max()
        print("replay at %d / %d rows: deviation %.2e of the largest entry (bar %.2e)" % (n1, n2, err / big, (L + 4) * 2.0 ** -24))
        assert L <= 90 and err <= (L + 4) * 2.0 ** -24 * big, (n1, n2)
    del pw
