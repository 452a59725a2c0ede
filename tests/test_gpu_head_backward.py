"""d3f_neighbor_transpose and d3f_detect_head_backward (d3feat_amd.ops.neighbor_transpose / detect_head_backward) on the MI355X.

The transposed table is compared integer for integer with head_grad_np.transpose_np (np.argsort(kind="stable") -- the definition).

The backward is compared with the float64 definition tests/head_grad_np.py (itself pinned on the CPU by tests/test_head_grad_host.py)
on the case grid of head_grad_np.GRID, in three evaluations: (gdesc, 0), (0, gscore) and both.  Tolerance per evaluation: the larger of
(a) four times the deviation of float32 torch-CPU autograd of the restated head from float64 (err32 of tests/golden/head_grad.npz) and
(b) head_grad_np.tolerances, a first-order worst-case bound derived from the case -- and never more than 1e-4 of the largest entry
compared (head_grad_np.cap).  The clamp rows (ss < 1e-10) are compared on their own by the same rule in EVERY evaluation: their
entries are some 1e5 times the rest in the descriptor path, and the same rows have w_i of about 1e-6 and dominate the score path by as
much -- under one 'largest entry' bar an ordinary row (entries of order 1) could come back as zero and pass.  The all-non-positive
padded cloud (den = 1e-6, entries of 1e12 and more) is compared per entry relatively, the same rule applied to relative deviations.  One exception, reasoned rather than measured: at C = 1 the (gdesc, 0)
gradient of a non-clamp row is identically zero (x / |x| is constant), "a fraction of the largest entry" is a fraction of nothing,
and the bound (b) -- 2 (C + 16) 2^-24 |gdesc| / |x| -- stands alone.

What the device measured against these: the docstring of test_backward_against_float64."""
import os

import numpy as np
import pytest
import torch

import head_grad_np as hg
import loss_grad_np as lg
from conftest import GOLDEN
from oracle import head_cases

pytestmark = pytest.mark.gpu
_cache = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _fixture():
    if "z" not in _cache:
        z = np.load(os.path.join(GOLDEN, "head_grad.npz"))
        _cache["z"] = {str(name): dict(err32=z["err32"][at], err32_clamp=z["err32_clamp"][at], err32_rel=z["err32_rel"][at])
                       for at, name in enumerate(z["names"])}
    return _cache["z"]


def _want(name, ev):
    """float64 gradients of a grid case and evaluation; computed once"""
    if (name, ev) not in _cache:
        c = hg.grid_case(name)
        gd, gs = hg.seeds_of(c, ev)
        _cache[(name, ev)] = hg.gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])
    return _cache[(name, ev)]


def _stack(device, c):
    return dict(x=_dev(c["x"], device), nb=_dev(c["nb"], device), lens=_dev(np.asarray(c["lens"], np.int32), device),
                pads=None if c["pads"] is None else _dev(np.asarray(c["pads"], np.int32), device))


def _run(device, c, ev, st=None, **kw):
    """ops.detect_head_backward on a grid case; the output is pre-filled with NaN: every word must be overwritten."""
    from d3feat_amd import ops
    st = st or _stack(device, c)
    gd, gs = hg.seeds_of(c, ev)
    out = torch.full((c["n"], c["C"]), float("nan"), device=device)
    got = ops.detect_head_backward(st["x"], st["nb"], st["lens"], st["pads"], None if gd is None else _dev(gd, device),
                                   None if gs is None else _dev(gs, device), stack_group=c["group"], out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _check(have, name, ev, what=""):
    """Device gradients of a grid case against head_grad_np.gradients by the rule of the module docstring -> the relative figures."""
    c, res, fx = hg.grid_case(name), _want(name, ev), _fixture()[name]
    e = hg.EVALS.index(ev)
    assert np.isfinite(have).all(), "%s %s %s: a word was not written" % (name, ev, what)
    neg = hg.NEGATIVE_ROWS.get(name)
    d = hg.deviations(have, res["gx"], ev, res["clamp"], neg)
    E = hg.tolerances(res, c["K"])["score"]
    if ev != "score":
        E = E + hg.desc_tolerances(c["x"], c["gd"])
    rows = np.ones(c["n"], bool)
    if neg is not None:
        rows[neg] = False
    figures = {}
    if "clamp" in d:
        dev, big = d["clamp"]
        tol = hg.cap(max(4 * fx["err32_clamp"][e], E[res["clamp"] & rows].max()), big)
        figures["clamp"] = dev / big
        print("%s %s %s clamp rows: largest %.3e, deviation %.2e of it (tolerance %.2e)" % (name, ev, what, big, dev / big, tol / big))
        assert dev <= tol, (name, ev, what, "clamp rows")
        rows &= ~res["clamp"]
    dev, big = d["main"]
    bound = E[rows].max() if rows.any() else 0.0
    tol = max(4 * fx["err32"][e], bound)
    if not (name == "c1" and ev == "desc"):                # (C = 1, (gdesc, 0): the gradient is identically zero -- module docstring)
        tol = hg.cap(tol, big)
    figures["main"] = dev / max(big, 1e-300)
    print("%s %s %s: largest %.3e, deviation %.2e of it (tolerance %.2e)" % (name, ev, what, big, dev / max(big, 1e-300), tol / max(big, 1e-300)))
    assert dev <= tol, (name, ev, what)
    if neg is not None:
        w = res["gx"][neg]
        nz = w != 0
        tol = min(max(4 * fx["err32_rel"][e], (E[neg][nz] / np.abs(w[nz])).max()), hg.BAR)
        figures["rel"] = d["rel"]
        print("%s %s %s all-non-positive cloud: largest relative deviation %.2e (tolerance %.2e)" % (name, ev, what, d["rel"], tol))
        assert d["rel_zero_ok"] and d["rel"] <= tol, (name, ev, what, "relative")
    return figures


# ---- the transposed table -----------------------------------------------------------------------------------------------------------------
def _neighbours(seed, lens, K, N=None, shadow=0.2):
    """uniform neighbours inside the point's own cloud, a fraction `shadow` of the slots one of head_cases.SHADOWS; rows at or beyond
    n = sum(lens) (capacity) hold garbage that must not be read as edges"""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    N = n if N is None else N
    nb = rng.integers(0, max(n, 1), (N, K)).astype(np.int64)
    a = 0
    for l in lens:
        if l:
            nb[a:a + l] = rng.integers(a, a + l, (l, K))
        a += l
    sh = rng.random((N, K)) < shadow
    vals = np.asarray([n + head_cases.SHADOWS[0], n + head_cases.SHADOWS[1]] + list(head_cases.SHADOWS[2:]), np.int64)
    nb = np.where(sh, vals[rng.integers(0, len(vals), (N, K))], nb)
    return nb.astype(np.int32)


def _planted(seed):
    """300 + 20 rows, K = 3: row 5 is named by every row of its cloud (in-degree 300 > 256), row 7 by nobody, row 9 names row 11 twice"""
    nb = _neighbours(seed, (300, 20), 3)
    nb[nb == 7] = 8
    nb[:300, 0] = 5
    nb[9, 1] = nb[9, 2] = 11
    return nb


TRANSPOSE = {
    "k0": lambda: (_neighbours(1, (30, 20), 0), (30, 20), 0),
    "k1": lambda: (_neighbours(2, (30, 20), 1), (30, 20), 0),
    "k33": lambda: (_neighbours(3, (30, 20), 33), (30, 20), 0),
    "k65_ld": lambda: (_neighbours(4, (30, 20), 65), (30, 20), 7),                    # ld_idx = K + 7
    "shadows": lambda: (_neighbours(5, (40,), 10, shadow=0.7), (40,), 0),            # all five shadow values, most slots
    "planted": lambda: (_planted(6), (300, 20), 0),
    "capacity": lambda: (_neighbours(7, (30, 20), 9, N=64), (30, 20), 3),            # N = 64 > n = 50
    "empty_cloud": lambda: (_neighbours(8, (30, 0, 20), 9), (30, 0, 20), 0),
    "empty_stack": lambda: (_neighbours(9, (0, 0), 4, N=6), (0, 0), 0),
    "tiles": lambda: (_neighbours(10, (600, 500), 65), (600, 500), 0),               # 71,500 edges: nine 8192-item tiles, two digit passes
    "b255": lambda: (_neighbours(12, hg.LENS_B255, 5), hg.LENS_B255, 0),             # D3F_MAX_BATCH lengths summed by the key kernel
    # 66,000 rows: keys of 17 bits, THREE 8-bit digit passes -- the finishing kernel reads the other buffer pair (four need 2^24 rows)
    "rows_66000": lambda: (_neighbours(13, (40000, 26000), 2), (40000, 26000), 1),   # ld_idx = K + 1
}


@pytest.mark.parametrize("name", list(TRANSPOSE))
def test_transposed_table_is_the_stable_argsort(device, name):
    """d3f_neighbor_transpose through the C ABI, outputs pre-filled with -1: start (all N + 1 words) and the valid edges equal
    head_grad_np.transpose_np integer for integer; the words of `edges` beyond the valid edges are left alone."""
    from d3feat_amd import _lib
    lib = _lib.load()
    nb, lens, extra = TRANSPOSE[name]()
    N, K = nb.shape
    n = int(sum(lens))
    if name == "shadows":
        assert all(((nb == v).any() for v in (n, n + 3, -1, -9, 1 << 30)))
    wide = np.full((N, K + extra), 12345, np.int32)
    wide[:, :K] = nb
    it = _dev(wide, device)
    lt = _dev(np.asarray(lens, np.int32), device)
    start = torch.full((N + 1,), -1, dtype=torch.int32, device=device)
    edges = torch.full((max(N * K, 1),), -1, dtype=torch.int32, device=device)
    nbytes = lib.d3f_neighbor_transpose_workspace_bytes(N, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    rc = lib.d3f_neighbor_transpose(it.data_ptr(), N, K + extra, K, lt.data_ptr(), len(lens), start.data_ptr(), edges.data_ptr(),
                                    ws.data_ptr(), nbytes, torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(device)
    ws_, we_ = hg.transpose_np(nb, n, N)
    hs, he = start.cpu().numpy(), edges.cpu().numpy()
    assert np.array_equal(hs, ws_), name
    assert np.array_equal(he[:len(we_)], we_) and (he[len(we_):] == -1).all(), name
    if name == "planted":
        assert ws_[6] - ws_[5] >= 300 and ws_[8] == ws_[7]
    if name == "tiles":
        assert N * K > 8 * 8192 and len(we_) > 6 * 8192
    passes = (max(n.bit_length(), 1) + 7) // 8                                       # 32 - clz(n) significant bits, 8 per digit pass
    assert passes == {"rows_66000": 3, "tiles": 2, "empty_stack": 1}.get(name, passes)
    if name == "b255":
        assert len(lens) == 255 and lens[-1] == 0 and n == 507


def test_transpose_through_ops(device):
    from d3feat_amd import ops
    nb = _neighbours(11, (30, 20), 9)
    start, edges = ops.neighbor_transpose(_dev(nb, device), _dev(np.asarray([30, 20], np.int32), device))
    ws_, we_ = hg.transpose_np(nb, 50)
    assert start.dtype == torch.int32 and edges.shape == (450,)
    assert np.array_equal(start.cpu().numpy(), ws_) and np.array_equal(edges.cpu().numpy()[:len(we_)], we_)


# ---- the backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hg.GRID))
def test_backward_against_float64(device, name):
    """Every case of head_grad_np.GRID in the three evaluations: C in (1, 20, 32, 33, 64, 100, 128) (the three channel-per-lane forms,
    full and partial last lanes), K in (0, 1, 33, 65), B = 1 / 2 / 3 / 6 with stack_group 0 / 1 / 2 / 3 and an empty cloud, equal lengths,
    explicit pad counts (as a flag on positive clouds, and as a COUNT -- 3, neither the derived 10 nor 1 -- on the all-non-positive
    cloud with planted zeros, where it sets the number of ties), the duplicated column (bit-equal ties in T, W), the padded all-non-positive cloud without and with planted
    zeros (pads * C + 2 ties for the cloud maximum).

    Measured on one MI355X (float32 torch-CPU autograd on the same case in brackets).  Ordinary rows (largest entry 0.3 to 1.7): the
    largest |device - float64| is 3.63e-7 of the largest entry compared at C >= 20 (c32, both: 2.4e-7; float32 torch reaches 3.8e-7 on
    b3empty) and 1.05e-6 at C = 1 (c1, (0, gscore): 3.7e-7); no such comparison uses more than 0.033 of its tolerance, which in the two
    evaluations with gscore is mostly the 1e-4 cap (the first-order bound exceeds it).  Clamp rows (largest entry 9e3 to 4e5): 2.59e-7
    (negzero, (0, gscore): 1.82e-7), at most 0.21 of the tolerance (b3g1, (gdesc, 0): 5.09e-8 against 2.38e-7).  Per entry relatively
    on the all-non-positive cloud: 7.70e-5 (neg, (0, gscore): 7.70e-5 -- sums of gS terms of both signs at 1e12 cancel; the tolerance
    there is the 1e-4 cap, of which this is 0.77).  At C = 1 the identically-zero (gdesc, 0) rows came back at 9.4e-7 absolute against
    the bound 1.5e-5.

    b255 / b255g5 / b129: stacks of 255 and 129 clouds of a few rows each (one thread per cloud in head_max_init_kernel, its serial
    prefix and group scans, d3f_find_elem's steps of 128 / 64 / 32, whole empty groups of five), by the same rule.  Measured: at
    most 1.36e-7 of the largest entry (b255g5, (0, gscore); float32 torch 1.09e-7), clamp rows of b129 1.21e-7; no comparison uses more
    than 0.17 of its tolerance (b129's clamp rows, (gdesc, 0)), the ordinary rows at most 0.035.  Each of the three cases takes under
    0.1 s (--durations inside the whole suite: b129 0.07 s, b255 and b255g5 0.04 s; the transposed table rows_66000 0.01 s, b255 under
    0.005 s)."""
    c = hg.grid_case(name)
    st = _stack(device, c)
    for ev in hg.EVALS:
        _check(_run(device, c, ev, st), name, ev)


def test_layouts_and_capacity(device):
    """ldx != C, an unaligned view, the seeds as strided column views of a [xyz | desc | score] record block (ldg = ldgs = C + 4), a
    caller-kept table, capacity N > n with rows at or beyond n left alone: all give the bits of the plain call."""
    from d3feat_amd import ops
    for name in ("c32", "c20"):
        c = hg.grid_case(name)
        n, C, K = c["n"], c["C"], c["K"]
        plain = _run(device, c, "both")
        _check(plain, name, "both", "plain")
        N = n + 14
        buf = torch.full((N * (C + 5) + 1,), float("nan"), device=device)
        xv = buf[1:].view(N, C + 5)[:, :C]                                           # base 4 bytes off 16-byte alignment, ldx = C + 5
        xv[:n] = _dev(c["x"], device)
        nbw = np.full((N, K + 2), -7, np.int32)
        nbw[:n, :K] = c["nb"]
        nbt = _dev(nbw, device)[:, :K]
        rec = torch.full((N, C + 4), float("nan"), device=device)
        rec[:n, 3:3 + C] = _dev(c["gd"], device)
        rec[:n, 3 + C] = _dev(c["gs"], device)
        lens = _dev(np.asarray(c["lens"], np.int32), device)
        table = ops.neighbor_transpose(nbt, lens)
        out = torch.full((N, C + 3), float("nan"), device=device)
        ops.detect_head_backward(xv, nbt, lens, None, rec[:, 3:3 + C], rec[:, 3 + C:4 + C], transpose=table, out=out[:, :C])
        o = out.cpu().numpy()
        assert np.array_equal(o[:n, :C].view(np.uint32), plain.view(np.uint32)), name
        assert np.isnan(o[n:]).all() and np.isnan(o[:, C:]).all(), name


def test_bits(device):
    """Two calls give equal bits; a stack_group = 2 concatenation of two stacks gives the bits of the stacks run alone."""
    from d3feat_amd import ops
    a, b = hg.grid_case("c32"), hg.grid_case("eqlen")
    ga, gb = _run(device, a, "both"), _run(device, b, "both")
    assert np.array_equal(ga.view(np.uint32), _run(device, a, "both").view(np.uint32))

    def shifted(c, off, total):
        nb = c["nb"].astype(np.int64)
        real = (nb >= 0) & (nb < c["n"])
        return np.where(real, nb + off, total).astype(np.int32)
    total = a["n"] + b["n"]
    nb = np.concatenate([shifted(a, 0, total), shifted(b, a["n"], total)])
    assert head_cases.neighbours_stay_in_cloud(nb, a["lens"] + b["lens"])
    x = np.concatenate([a["x"], b["x"]])
    gd, gs = np.concatenate([a["gd"], b["gd"]]), np.concatenate([a["gs"], b["gs"]])
    got = ops.detect_head_backward(_dev(x, device), _dev(nb, device), _dev(np.asarray(a["lens"] + b["lens"], np.int32), device), None,
                                   _dev(gd, device), _dev(gs, device), stack_group=2).cpu().numpy()
    assert np.array_equal(got[:a["n"]].view(np.uint32), ga.view(np.uint32))
    assert np.array_equal(got[a["n"]:].view(np.uint32), gb.view(np.uint32))


def test_loss_gradients_feed_the_backward(device):
    """The use case: validation.loss_gradients_records on a small pair's head outputs writes its seeds into a record block, and the
    block's column views go straight into detect_head_backward -- no host round trip.  Against float64 autograd of
    loss_grad_np.torch_loss composed with head_grad_np.torch_head; tolerance by the rule of the module docstring, err32 evaluated here
    (float32 autograd of the same composition on the CPU)."""
    from d3feat_amd import ops
    from d3feat_amd.validation import loss_gradients_records
    from oracle import network_np
    C, K, lens, n_pairs = 32, 17, (40, 30), 24
    n = sum(lens)
    for k in range(64):
        x, nb = head_cases.head_case(700 + k, C, K, lens, specials=False)
        rng = np.random.default_rng(700 + k)
        pts = rng.random((n, 3)).astype(np.float32)
        ai = rng.choice(lens[0], n_pairs, replace=False).astype(np.int32)
        pi = (lens[0] + rng.choice(lens[1], n_pairs, replace=False)).astype(np.int32)
        try:
            hg.margins(x, nb, lens)
            desc64, _, _ = network_np.detection_head_f64(x, nb, lens)
            lg.margins(desc64.astype(np.float32), pts, ai, pi, 0.1, C)
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no clean pair found")

    def composed(dtype):
        dt = getattr(torch, dtype)
        xt = torch.tensor(x, dtype=dt, requires_grad=True)
        desc, score = hg.torch_head(xt, torch.tensor(nb.astype(np.int64)), lens, hg.pad_counts(lens))
        val = lg.torch_loss(desc, score.reshape(-1), torch.tensor(pts, dtype=dt), torch.tensor(ai.astype(np.int64)),
                            torch.tensor(pi.astype(np.int64)), float(np.float32(0.1)), 2, 1.0)
        val.backward()
        return xt.grad.double().numpy()
    want, w32 = composed("float64"), composed("float32")
    xt, nbt, lt = _dev(x, device), _dev(nb, device), _dev(np.asarray(lens, np.int32), device)
    desc, score = ops.detect_head(xt, nbt, lt, None)
    rec = torch.cat([_dev(pts, device), desc, score], 1).contiguous()
    grad = torch.full_like(rec, float("nan"))
    loss_gradients_records(rec, list(lens), _dev(ai, device), _dev(pi, device), n_pairs, keypts_num=2, out_records=grad)
    gx = ops.detect_head_backward(xt, nbt, lt, None, grad[:, 3:3 + C], grad[:, 3 + C:4 + C]).cpu().numpy()
    g = grad.cpu().numpy().astype(np.float64)
    res = hg.gradients(x, nb, lens, g[:, 3:3 + C], g[:, 3 + C])
    assert not res["clamp"].any()
    E = hg.tolerances(res, K)["score"] + hg.desc_tolerances(x, g[:, 3:3 + C])
    big = np.abs(want).max()
    tol = hg.cap(max(4 * np.abs(w32 - want).max(), E.max()), big)
    dev = np.abs(gx - want).max()
    print("loss -> head: largest %.3e, deviation %.2e of it (float32 autograd %.2e, tolerance %.2e)" % (
        big, dev / big, np.abs(w32 - want).max() / big, tol / big))
    assert np.isfinite(gx).all() and dev <= tol


def test_capture_then_replay_on_other_data(device):
    """The table and the backward hold no host decision: captured once in torch.cuda.graph, replayed twice with other x (and other
    seeds) written into the same tensors, they give the bits of direct calls."""
    from d3feat_amd import ops
    a, b = hg.grid_case("c32"), hg.grid_case("pads")            # same shapes: C = 32, K = 17, 70 and 50 rows -> capacity 70
    N, C = a["n"], a["C"]

    def padded(c):
        x = np.zeros((N, C), np.float32)
        nb = np.full((N, c["K"]), -1, np.int32)
        gd, gs = np.zeros((N, C), np.float32), np.zeros(N, np.float32)
        x[:c["n"]], nb[:c["n"]], gd[:c["n"]], gs[:c["n"]] = c["x"], c["nb"], c["gd"], c["gs"]
        return [x, nb, np.asarray(c["lens"], np.int32), gd, gs]
    st = [_dev(t, device) for t in padded(a)]
    out = torch.zeros((N, C), device=device)
    stream = torch.cuda.Stream(device=device)

    def call():
        table = ops.neighbor_transpose(st[1], st[2])
        ops.detect_head_backward(st[0], st[1], st[2], None, st[3], st[4], transpose=table, out=out)
        return table
    with torch.cuda.stream(stream):
        with ops.private_workspace() as pw:
            call()                                                   # warm-up: sizes the scratch
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                table = call()
    stream.synchronize()
    for c in (b, a):
        for dst, src in zip(st, padded(c)):
            dst.copy_(_dev(src, device))
        out.fill_(float("nan"))
        torch.cuda.synchronize(device)
        graph.replay()
        torch.cuda.synchronize(device)
        eager = ops.detect_head_backward(st[0].clone(), st[1].clone(), st[2].clone(), None, st[3].clone(), st[4].clone())
        o = out.cpu().numpy()
        assert np.array_equal(o[:c["n"]].view(np.uint32), eager.cpu().numpy()[:c["n"]].view(np.uint32))
        assert np.isnan(o[c["n"]:]).all()
        ws_, we_ = hg.transpose_np(c["nb"], c["n"], N)
        assert np.array_equal(table[0].cpu().numpy(), ws_) and np.array_equal(table[1].cpu().numpy()[:len(we_)], we_)
        if c is a:
            _check(o, "c32", "both", "replay")
    del pw, table
