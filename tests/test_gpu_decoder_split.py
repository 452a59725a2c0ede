"""The decoder's unary blocks in split form (ops.gemm_upsample_split, d3f_gemm_x3_gres): the upsampled half of
[ x'[up[m, 0]] | skip[m] ] @ W is contracted once per COARSE row, Y = x @ W[:C1] * s, and the fine level computes
leaky(skip @ W[C1:] * s + t + Y[up[m, 0]]) with the row gather in the epilogue of gemm_x3_kernel (one K slice) or of the K-split
reduction (several).  Checked against a float64 numpy reference of leaky(([gathered | skip] @ W) * s + t) with the bound of the
family (tests/test_gpu_gemm_x3.py): max |got - ref| <= 4e-6 max(1, max |ref|).  The reference and the inputs are checked on the CPU
by tests/test_decoder_split_host.py (same generator)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N1 = 700
# (C1, C2, N, m): the fine-level launch of each is planned (d3f_gemm_x3_plan) as 128 x 64 / one slice, 128 x 64 / three slices,
# 128 x 64 / one slice over 235 row tiles, 256 x 128 / three slices with a ragged last tile, 256 x 128 / one slice, ragged
CASES = [(128, 64, 64, 2500), (2048, 1024, 512, 2500), (256, 256, 128, 30000), (2048, 1024, 512, 4517), (128, 128, 512, 8501)]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_case(C1, C2, N, m, n1=N1):
    """Inputs of one decoder block.  idx: three columns, only column 0 is used; values over [0, n1]; every 17th row the shadow
    index n1, every 29th a negative index, every 31st one above n1."""
    rng = np.random.default_rng(C1 + C2 + N + m)
    x = rng.standard_normal((n1, C1)).astype(np.float32)
    skip = rng.standard_normal((m, C2)).astype(np.float32)
    idx = rng.integers(0, n1 + 1, (m, 3)).astype(np.int32)
    idx[5::29, 0] = -1 - (np.arange(len(idx[5::29])) % 7).astype(np.int32)
    idx[7::31, 0] = n1 + 1 + (np.arange(len(idx[7::31])) * 1000003 % 100000).astype(np.int32)
    idx[::17, 0] = n1
    W = (rng.standard_normal((C1 + C2, N)) / np.sqrt(C1 + C2)).astype(np.float32)
    s, t = rng.random(N).astype(np.float32) + 0.5, rng.standard_normal(N).astype(np.float32)
    return x, skip, idx, W, s, t


def reference(x, skip, idx, W, s, t, n1=None):
    """float64 leaky((concat @ W) * s + t); a row whose index is outside [0, n1) gathers the zero row."""
    n1 = x.shape[0] if n1 is None else n1
    i0 = idx[:, 0].astype(np.int64)
    live = (i0 >= 0) & (i0 < n1)
    g = np.where(live[:, None], x[np.where(live, i0, 0)], np.float32(0))
    full = np.concatenate([g, skip], 1).astype(np.float64)
    ref = full @ W.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)
    return np.where(ref > 0, ref, 0.2 * ref), live


def halves(W, s, C1):
    Ws = (W * s[None, :]).astype(np.float32)
    return np.ascontiguousarray(Ws[:C1]), np.ascontiguousarray(Ws[C1:])


@functools.lru_cache(maxsize=None)
def _case(C1, C2, N, m):
    arrs = make_case(C1, C2, N, m)
    ref, live = reference(*arrs)
    ref.setflags(write=False)
    return arrs, ref, live


def _plan(M, N, K, hint=0):
    from d3feat_amd import _lib
    r, c, s = C.c_int(), C.c_int(), C.c_int()
    assert _lib.load().d3f_gemm_x3_plan(M, N, K, hint, C.byref(r), C.byref(c), C.byref(s)) == 0
    return r.value, c.value, s.value


def test_the_cases_cover_both_workgroup_shapes_and_both_epilogues():
    """The fine-level launch (M = m, K = C2) of the cases, as the library plans it."""
    from d3feat_amd import ops
    plans = {_plan(m, N, C2) for C1, C2, N, m in CASES}
    assert {p[:2] for p in plans} >= {(128, 64), (256, 128)}
    for shape in ((128, 64), (256, 128)):
        assert any(p[:2] == shape and p[2] == 1 for p in plans), shape     # direct epilogue
        assert any(p[:2] == shape and p[2] > 1 for p in plans), shape      # reduce kernel
    assert any(m % 32 for _, _, _, m in CASES)
    assert all(ops._split_ok(m, C1, C2, N) for C1, C2, N, m in CASES)


def _run(device, arrs, **kw):
    from d3feat_amd import ops
    x, skip, idx, W, s, t = arrs
    w1, w2 = halves(W, s, x.shape[1])
    u = ops.UpsampleCat(_t(x, device), _t(idx, device), _t(skip, device))
    return u, _t(w1, device), _t(w2, device), _t(t, device)


@pytest.mark.parametrize("C1,C2,N,m", CASES)
def test_against_float64(device, C1, C2, N, m):
    from d3feat_amd import ops
    arrs, ref, live = _case(C1, C2, N, m)
    assert 0 < (~live).sum() < m and (arrs[2][:, 0] < 0).any() and (arrs[2][:, 0] > N1).any() and (arrs[2][::17, 0] == N1).all()
    u, w1, w2, t = _run(device, arrs)
    got = ops.gemm_upsample_split(u, w1, w2, col_shift=t, leaky=True)
    err, bound = np.abs(got.cpu().numpy() - ref).max(), 4e-6 * max(1.0, np.abs(ref).max())
    print("C1 %d C2 %d N %d m %d plan %s: max err %.3e (bound %.3e)" % (C1, C2, N, m, _plan(m, N, C2), err, bound))
    assert err <= bound
    # shadow, negative and too large indices add exact zeros: those rows are the skip-only result, bit for bit
    dead = torch.from_numpy(np.flatnonzero(~live)).to(device)
    only = ops.gemm(u.skip, w2, col_shift=t, leaky=True)
    assert torch.equal(got[dead], only[dead])
    # and the one-launch form it replaces is as close to the reference
    fused = ops.gemm_upsample_cat(u, _t(arrs[3], device), col_scale=_t(arrs[4], device), col_shift=t, leaky=True)
    assert np.abs(fused.cpu().numpy() - ref).max() <= bound


@pytest.mark.parametrize("C1,C2,N,m,real,real1", [(128, 64, 64, 2500, 1801, 650), (2048, 1024, 512, 2500, 2011, 700)])
def test_capacity_mode(device, C1, C2, N, m, real, real1):
    """Device-resident row counts below the capacities (direct epilogue and reduce kernel): rows beyond the fine count keep the
    caller's fill, indices beyond the coarse count gather zeros."""
    from d3feat_amd import ops
    arrs, _, _ = _case(C1, C2, N, m)
    ref, live = reference(*arrs, n1=real1)
    u, w1, w2, t = _run(device, arrs)
    u.x.n_dev, u.x.n_hint = torch.tensor([real1], dtype=torch.int32, device=device), real1
    u.inds.n_dev, u.inds.n_hint = torch.tensor([real], dtype=torch.int32, device=device), real
    out = torch.full((m, N), 12345.0, dtype=torch.float32, device=device)
    got = ops.gemm_upsample_split(u, w1, w2, col_shift=t, leaky=True, out=out)
    assert got.data_ptr() == out.data_ptr() and got.n_dev is u.inds.n_dev
    assert np.abs(out[:real].cpu().numpy() - ref[:real]).max() <= 4e-6 * max(1.0, np.abs(ref[:real]).max())
    assert bool((out[real:] == 12345.0).all())


@pytest.mark.parametrize("C1,C2,N,m", [CASES[0], CASES[3]])
def test_row_position_does_not_matter(device, C1, C2, N, m):
    """A stacked self-pair: the second half of the rows repeats the first; both halves come out bit-equal."""
    from d3feat_amd import ops
    (x, skip, idx, W, s, t), _, _ = _case(C1, C2, N, m)
    h = m // 2
    skip2, idx2 = np.concatenate([skip[:h], skip[:h]]), np.concatenate([idx[:h], idx[:h]])
    u, w1, w2, tt = _run(device, (x, skip2, idx2, W, s, t))
    got = ops.gemm_upsample_split(u, w1, w2, col_shift=tt, leaky=True)
    assert torch.equal(got[:h].view(torch.int32), got[h:].view(torch.int32))


def test_argument_rules_of_the_entry_point(device):
    from d3feat_amd import _lib
    lib = _lib.load()
    m, K, N, n1 = 256, 64, 64, 50
    skip, Y = torch.zeros((m, K), device=device), torch.zeros((n1 + 1, N), device=device)
    idx = torch.zeros((m, 3), dtype=torch.int32, device=device)
    out = torch.full((m, N), 7.0, device=device)
    wx = torch.zeros(int(lib.d3f_gemm_x3_packed_bytes(K, N)), dtype=torch.uint8, device=device)
    ws = torch.empty(4096, dtype=torch.uint8, device=device)

    def call(res=Y.data_ptr(), ld=3, k=K, ridx=idx.data_ptr(), rows=n1):
        return lib.d3f_gemm_x3_gres(skip.data_ptr(), m, K, k, None, 0, None, 0, 0, wx.data_ptr(), out.data_ptr(), N, m, N, None, None, None,
                                    res, N, ridx, ld, rows, None, 1, 0.2, ws.data_ptr(), C.c_size_t(4096), None, None, 0, None)
    assert call(res=Y.data_ptr() + 4) == -3       # misaligned residual
    assert call(ld=0) == -3                       # leading dimension of the index matrix
    assert call(k=48) == -3                       # K not a multiple of 32
    assert call(res=None) == -3                   # an index without a residual tensor
    assert call(rows=-1) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())               # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def test_switch_off_gives_the_bits_of_the_one_launch_form(device, monkeypatch):
    """unary_block on an UpsampleCat: the split form by default (close to float64), ops.DECODER_SPLIT = False the bits of
    gemm_upsample_cat with the block's own weights and folded batch norm."""
    from d3feat_amd import ops
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import VariableStore
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    C1, C2, N, m = CASES[0]
    (x, skip, idx, _, _, _), _, _ = _case(C1, C2, N, m)
    vs = VariableStore(seed=3, device=device)
    with vs.variable_scope('uplayer_1/unary_0'):
        w = vs.weight_variable([C1 + C2, N])
        bn = vs.batch_norm_variables(N)
    rng = np.random.default_rng(9)
    vs.values[bn[0]] = (1.0 + 0.2 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[1]] = (0.1 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[2]] = (0.1 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[3]] = (0.5 + rng.random(N)).astype(np.float32)
    u = ops.UpsampleCat(_t(x, device), _t(idx, device), _t(skip, device))

    def block():
        with nb.use_variables(vs), vs.variable_scope('uplayer_1/unary_0'):
            return nb.unary_block(1, {}, u, 0.1, N, cfg, False)
    assert ops.DECODER_SPLIT and ops.upsample_split_ok(u, N)
    on = block()
    monkeypatch.setattr(ops, "DECODER_SPLIT", False)
    off = block()
    scale, shift = vs.folded_bn(bn)
    assert torch.equal(off, ops.gemm_upsample_cat(u, vs.tensor(w), col_scale=scale, col_shift=shift, leaky=True, alpha=0.2))
    s, t = vs._bn_host(bn, 1e-6)
    ref, _ = reference(x, skip, idx, vs.values[w], s, t)
    bound = 4e-6 * max(1.0, np.abs(ref).max())
    assert np.abs(on.cpu().numpy() - ref).max() <= bound and np.abs(off.cpu().numpy() - ref).max() <= bound
    assert not torch.equal(on, off)               # (the two forms sum in a different order)


def test_refresh_of_decoder_weights_under_a_live_graph(device):
    """FragmentEngine.refresh_weights on one decoder weight and one decoder batch-norm vector: the split halves (and their packed
    copies) are rewritten in place, the next replay equals an engine built from the new values, bit for bit."""
    from d3feat_amd import ops
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    from d3feat_amd.utils.synthetic import room_fragment
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    limits = np.asarray([37, 35, 36, 38, 38], np.int32)
    raw = torch.from_numpy(room_fragment(11, n_raw=30000, edge=1.0)).to(device)
    eng = FragmentEngine(cfg, W, limits, raw_cap=40000, n0_cap=10000, slots=1, device=device)
    assert any(isinstance(k, tuple) and k[0] == 'split' for k in eng.model.variables._dev), "no decoder block took the split form"
    p0, d0, s0 = (t.clone() for t in eng.run(raw))
    rng = np.random.default_rng(5)
    kw, kb = 'uplayer_3/unary_0/weights', 'uplayer_2/unary_0/batch_normalization/gamma'
    new = {kw: (W[kw] * (1.0 + 0.1 * rng.standard_normal(W[kw].shape))).astype(np.float32),
           kb: (W[kb] * (1.0 + 0.1 * rng.standard_normal(W[kb].shape))).astype(np.float32)}
    assert eng.refresh_weights(new) > 0
    p1, d1, s1 = (t.clone() for t in eng.run(raw))
    assert eng.fallbacks == 0
    W2 = dict(W)
    W2.update(new)
    ref = FragmentEngine(cfg, W2, limits, raw_cap=40000, n0_cap=10000, slots=1, device=device)
    p2, d2, s2 = ref.run(raw)
    assert torch.equal(p1, p2) and torch.equal(d1, d2) and torch.equal(s1, s2)
    assert (d1 - d0).abs().max().item() > 1e-4            # the update was really seen
