"""Every dispatch branch of csrc/pool_head.hip -- max pooling, nearest upsampling + concatenation, the detection head, the record
packer and the stand-alone epilogue -- against plain numpy references written here (oracle/network_np.py: detection_head_f64).

The launchers choose a kernel by channel count, alignment, leading dimension, address range and feature dtype; each test names the
instantiation it is meant to execute and quotes the launcher's condition its shapes follow from.  Gathers, comparisons and the
contraction-free epilogue are exact (np.array_equal); the head is compared with a float64 restatement at the project's bars and,
on two-cloud stacks, at a multiple of the float32 oracle's own error.

Padding columns of every strided view and capacity rows hold NaN: a kernel that reads outside its operand poisons its result.
K = 0 goes through the C ABI: torch reports a NULL address for a tensor without elements, and the launchers reject a NULL index
matrix.

Cost on an MI355X: the 111 cases take 2.4 s run alone and 0.6 s of the full GPU suite's 278 s (only the three large-stride cases
allocate more than a few MB: 0.2 GB and 0.1 GB for pooling, 4 GiB for the head, freed in the test).  The eight cases on stacks of
129 / 255 clouds (six of test_detect_head, two of test_pack_descriptors_to_255_clouds) came after that count: inside the full suite
head_kernel<1>-B255-g0 takes 0.07 s, every other one 0.01 s or less."""
import numpy as np
import pytest
import torch

import head_grad_np as hg
from conftest import bits

pytestmark = pytest.mark.gpu

S = np.float32(-124.0)            # sentinel of pre-filled outputs (a bfloat16 value too)
ERR_ARG = -3                      # D3F_ERR_ARG (include/d3feat_amd.h)
KS = (0, 1, 7, 8, 9, 17, 40)      # pooling: around the NB = 8 neighbour batches of maxpool_kernel


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(v, dev):
    return torch.tensor([int(v)], dtype=torch.int32, device=dev)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _load():
    from d3feat_amd import _lib
    return _lib.load()


def _view(a, dev, ld=None, off=0, fill=np.nan, bf16=False):
    """a [n, C] on the device: contiguous, or (ld given) the column slice [off, off + C) of an [n, ld] matrix filled with `fill`."""
    n, C = a.shape
    if ld is None:
        t = _t(a, dev)
        return t.to(torch.bfloat16) if bf16 else t
    big = np.full((n, ld), fill, a.dtype)
    big[:, off:off + C] = a
    t = _t(big, dev)
    return (t.to(torch.bfloat16) if bf16 else t)[:, off:off + C]


def _bf16_values(a):
    """float32 array -> the same array rounded to bfloat16 values (still float32)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# ind_max_pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_x(rng, n1, C, bf16=False):
    """Features whose column 0 is >= 0 and holds both +0 (row 0) and -0 (row 1): its ordered-key minimum is -0, by bits."""
    x = rng.standard_normal((n1, C)).astype(np.float32)
    x[:, 0] = np.abs(x[:, 0])
    x[0, 0], x[1, 0] = 0.0, -0.0
    if C > 1:
        m = min(n1, 6) - 2
        x[2:2 + m, C - 1] = (0.0, -0.0, -0.0, 0.0)[:m]      # signed zeros among the valid neighbours too: compared by value
    return _bf16_values(x) if bf16 else x


def _pool_idx(rng, n2, K, n1):
    """valid, == N1, > N1 and negative entries; rows 0 and n2 // 2 without any valid slot (the shadow row)."""
    idx = rng.integers(0, n1, (n2, K)).astype(np.int64)
    r = rng.random((n2, K))
    idx = np.where(r < 0.12, n1, idx)
    idx = np.where((r >= 0.12) & (r < 0.2), n1 + 1 + rng.integers(0, 1000, (n2, K)), idx)
    idx = np.where((r >= 0.2) & (r < 0.28), -1 - rng.integers(0, 1000, (n2, K)), idx)
    for row in (0, n2 // 2):
        idx[row] = np.where(np.arange(K) % 2 == 0, n1, -3)
    return idx.astype(np.int32)


def _pool_ref(x, idx, n1=None, n2=None):
    """models/network_blocks.py:51-66 with integer gathers: -> (out, rows that took the shadow row).  The shadow row is the column
    minimum by ordered key (sign-magnitude order, -0 < +0), as the kernel states."""
    n1 = len(x) if n1 is None else n1
    n2 = len(idx) if n2 is None else n2
    xs, idx = np.ascontiguousarray(x[:n1], np.float32), idx[:n2]
    u = xs.view(np.uint32)
    key = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    colmin = xs[key.argmin(0), np.arange(xs.shape[1])]
    valid = (idx >= 0) & (idx < n1)
    g = np.where(valid[:, :, None], xs[np.where(valid, idx, 0)], -np.inf)
    out = g.max(1) if idx.shape[1] else np.full((n2, xs.shape[1]), -np.inf)
    shadow = ~valid.any(1)
    out[shadow] = colmin
    return out.astype(np.float32), shadow


def _check_pool(got, x, idx, n1=None, n2=None, zero_rule=True):
    want, shadow = _pool_ref(x, idx, n1, n2)
    if got.dtype == torch.bfloat16:
        got = got.float()            # exact: the 16-bit patterns are compared through their float32 expansions
    got = got.cpu().numpy()[:len(want)]
    assert np.array_equal(got, want)                                   # by value: -0 == +0
    nz = want != 0
    assert np.array_equal(bits(got)[nz], bits(want)[nz])
    assert shadow.any()
    if zero_rule:    # the stated bit-level rule of the all-shadow row: column 0 holds +0, -0 and nothing smaller -> -0
        assert np.all(bits(got)[shadow, 0] == 0x80000000)


def _pool_abi(dev, xt, n1, C, it, n2, ldi, K, out, n1_dev=None, n2_dev=None, order=None):
    lib = _load()
    return lib.d3f_ind_max_pool(xt.data_ptr(), n1, xt.stride(0), C, it.data_ptr(), n2, ldi, K, out.data_ptr(), out.stride(0), None,
                                n1_dev.data_ptr() if n1_dev is not None else None, n2_dev.data_ptr() if n2_dev is not None else None,
                                order.data_ptr() if order is not None else None, 1 if xt.dtype == torch.bfloat16 else 0, _stream(dev))


def _pool_all_k(dev, C, ld, off, bf16, seed):
    from d3feat_amd import ops
    rng = np.random.default_rng(seed)
    n1, n2 = 50, 37
    x = _pool_x(rng, n1, C, bf16)
    xt = _view(x, dev, ld, off, bf16=bf16)
    for K in KS:
        idx = _pool_idx(rng, n2, K, n1)
        if K == 0:
            it = _t(np.ones((n2, 3), np.int32), dev)
            out = torch.empty((n2, C), dtype=xt.dtype, device=dev)
            assert _pool_abi(dev, xt, n1, C, it, n2, 3, 0, out) == 0
        else:
            # odd K: the index matrix is a column slice (ld_idx = K + 3 > K); the other columns name a valid row
            it = _view(idx, dev, K + 3, 2, fill=1) if K % 2 else _t(idx, dev)
            out = ops.ind_max_pool(xt, it)
        assert out.dtype == xt.dtype
        _check_pool(out, x, idx)


POOL_F32 = [
    pytest.param(128, None, 0, id="maxpool<4,float,U24>-C128"),            # C % 4 == 0 && ldx % 4 == 0 && (x & 15) == 0 && u24
    pytest.param(64, None, 0, id="maxpool<4,float,U24>-C64"),
    pytest.param(64, 72, 4, id="maxpool<4,float,U24>-C64-ldx72"),          # ldx > C, ldx % 4 == 0, base 16-byte aligned: stays <4>
    pytest.param(6, None, 0, id="maxpool<1>-C6"),                          # C % 4 != 0
    pytest.param(1, None, 0, id="maxpool<1>-C1"),
    pytest.param(128, 132, 1, id="maxpool<1>-C128-view-1:129-unaligned"),  # (x & 15) != 0 (ldx % 4 == 0)
    pytest.param(64, 70, 0, id="maxpool<1>-C64-ldx70"),                    # ldx % 4 != 0
]


@pytest.mark.parametrize("C,ld,off", POOL_F32)
def test_ind_max_pool_f32(device, C, ld, off):
    """d3f_ind_max_pool: `C % 4 == 0 && ldx % 4 == 0 && (x & 15) == 0 && u24` -> maxpool_kernel<4, float, true>, else (any of the
    first three false) maxpool_kernel<1>.  K in {0, 1, 7, 8, 9, 17, 40}, every index pattern, exact."""
    _pool_all_k(device, C, ld, off, False, 10 + C + (ld or 0))


@pytest.mark.parametrize("C,ld,off", [pytest.param(64, None, 0, id="maxpool<4,bf16,U24>-C64"),
                                      pytest.param(128, None, 0, id="maxpool<4,bf16,U24>-C128"),
                                      pytest.param(64, 72, 4, id="maxpool<4,bf16,U24>-C64-ldx72")])
def test_ind_max_pool_bf16(device, C, ld, off):
    """feat_bf16 (`C % 4 == 0, ldx % 4 == 0, x 8-byte aligned`, u24) -> maxpool_kernel<4, unsigned short, true>: the output is
    bfloat16 and bit-equal to the maximum over the same bfloat16 values."""
    _pool_all_k(device, C, ld, off, True, 20 + C + (ld or 0))


@pytest.mark.parametrize("bf16", [False, True], ids=["maxpool<4,float,false>", "maxpool<4,bf16,false>"])
def test_ind_max_pool_beyond_24_bit_addressing(device, bf16):
    """`u24 = d3f_fits_u24(N1, ldx) && ...` is false once ldx >= 2^24: four rows at a row stride of 2^24 elements take the non-U24
    form (size_t row addressing)."""
    from d3feat_amd import ops
    rng = np.random.default_rng(31)
    n1, n2, C, K, ld = 4, 20, 64, 9, 1 << 24
    x = _pool_x(rng, n1, C, bf16)
    store = torch.empty(((n1 - 1) * ld + C,), dtype=torch.bfloat16 if bf16 else torch.float32, device=device)
    xt = store.as_strided((n1, C), (ld, 1))
    xt.copy_(_t(x, device))
    idx = _pool_idx(rng, n2, K, n1)
    out = ops.ind_max_pool(xt, _t(idx, device))
    _check_pool(out, x, idx)
    del xt, store


@pytest.mark.parametrize("C,bf16", [(128, False), (6, False), (64, True)],
                         ids=["maxpool<4,float,U24>", "maxpool<1>", "maxpool<4,bf16,U24>"])
def test_ind_max_pool_order_and_device_counts(device, C, bf16):
    """row_order (a random permutation gives the same output), N1_dev < N1 (indices in [N1_dev, N1) become shadow slots and the
    column minima run over N1_dev rows only), N2_dev < N2 (rows >= N2_dev keep the sentinel)."""
    from d3feat_amd import ops
    rng = np.random.default_rng(40 + C)
    n1, n2, K, n1d, n2d = 60, 45, 11, 33, 29
    x = _pool_x(rng, n1, C, bf16)
    x[n1d:, :] -= 50.0                                 # the rows beyond N1_dev would change every column minimum
    if bf16:
        x = _bf16_values(x)
    idx = _pool_idx(rng, n2, K, n1)
    xt, it = _view(x, device, bf16=bf16), _t(idx, device)
    it.order = _t(rng.permutation(n2).astype(np.int32), device)
    _check_pool(ops.ind_max_pool(xt, it), x, idx, zero_rule=False)     # (column 0 is negative in the rows beyond N1_dev)
    # device row counts through ops (attribute n_dev), with the visiting order: a permutation of the first N2_dev rows
    xt.n_dev, it.n_dev = _i32(n1d, device), _i32(n2d, device)
    it.order = _t(rng.permutation(n2d).astype(np.int32), device)
    assert np.any((idx[:n2d] >= n1d) & (idx[:n2d] < n1))
    out = ops.ind_max_pool(xt, it)
    _check_pool(out, x, idx, n1d, n2d)
    # ... and through the C ABI into a pre-filled output of a wider leading dimension
    out = torch.full((n2, C + 4), float(S), dtype=xt.dtype, device=device)
    assert _pool_abi(device, xt, n1, C, it, n2, K, K, out, xt.n_dev, it.n_dev, it.order) == 0
    _check_pool(out[:, :C], x, idx, n1d, n2d)
    o = out.float().cpu().numpy()
    assert np.all(o[n2d:] == S) and np.all(o[:, C:] == S)


# ---------------------------------------------------------------------------------------------------------------------
# closest_pool_cat
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C1,C2", [(1, 0), (5, 3), (256, 128), (5, 0), (1, 128), (256, 3)])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "views"])
def test_closest_pool_cat(device, C1, C2, strided):
    """upsample_cat_kernel (the one kernel of d3f_closest_pool_cat): first-column index valid / == N1 / > N1 / negative, strided x and
    skip, ld_idx > 1, C2 = 0, device row counts on both operands.  Exact."""
    from d3feat_amd import ops
    rng = np.random.default_rng(C1 * 7 + C2)
    n1, n2, n1d, n2d = 40, 53, 31, 47
    x = rng.standard_normal((n1, C1)).astype(np.float32)
    skip = rng.standard_normal((n2, C2)).astype(np.float32) if C2 else None
    idx = rng.integers(0, n1, (n2, 3)).astype(np.int32)
    idx[0::7, 0], idx[1::7, 0], idx[2::7, 0] = n1, -1 - np.arange(len(idx[1::7])), n1 + 5
    idx[:, 1:] = 0                                     # columns that must not be read name a valid row

    def want(n1_, n2_):
        i0 = idx[:n2_, 0]
        ok = (i0 >= 0) & (i0 < n1_)
        up = np.where(ok[:, None], x[np.where(ok, i0, 0)], np.float32(0))
        return np.concatenate([up, skip[:n2_]], 1) if C2 else up
    xt = _view(x, device, C1 + 3, 2) if strided else _t(x, device)
    st = None if not C2 else (_view(skip, device, C2 + 5, 1) if strided else _t(skip, device))
    it = _view(idx, device, 7, 2, fill=0) if strided else _t(idx, device)
    out = ops.closest_pool_cat(xt, it, st)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want(n1, n2)))
    xt.n_dev, it.n_dev = _i32(n1d, device), _i32(n2d, device)
    assert np.any((idx[:n2d, 0] >= n1d) & (idx[:n2d, 0] < n1))
    out = ops.closest_pool_cat(xt, it, st)
    assert np.array_equal(bits(out.cpu().numpy()[:n2d]), bits(want(n1d, n2d)))
    # rows >= N2_dev stay untouched (C ABI, pre-filled output, ldo > C1 + C2)
    lib = _load()
    o = torch.full((n2, C1 + C2 + 2), float(S), device=device)
    rc = lib.d3f_closest_pool_cat(xt.data_ptr(), n1, xt.stride(0), C1, it.data_ptr(), n2, it.stride(0), st.data_ptr() if C2 else None,
                                  st.stride(0) if C2 else 0, C2, o.data_ptr(), C1 + C2 + 2, xt.n_dev.data_ptr(), it.n_dev.data_ptr(),
                                  _stream(device))
    assert rc == 0
    o = o.cpu().numpy()
    assert np.array_equal(bits(o[:n2d, :C1 + C2]), bits(want(n1d, n2d))) and np.all(o[n2d:] == S) and np.all(o[:, C1 + C2:] == S)


# ---------------------------------------------------------------------------------------------------------------------
# affine_act
# ---------------------------------------------------------------------------------------------------------------------
def _affine_ref(x, cs, ch, res, leaky, alpha):
    """((x * cs) + ch) + res, then the leaky select, in float32 in that order: the file is compiled without contraction, so this
    is the exact result."""
    v = x.astype(np.float32)
    if cs is not None:
        v = v * cs
    if ch is not None:
        v = v + ch
    if res is not None:
        v = v + res
    if leaky:
        v = np.where(v > 0, v, v * np.float32(alpha))
    return v.astype(np.float32)


@pytest.mark.parametrize("N", [1, 7, 64, 100])
def test_affine_act_every_operand_combination(device, N):
    """affine_act_kernel: all 16 combinations of scale / shift / residual / leaky, alpha in {0.2, 0.0}, contiguous and strided x and
    residual.  Bit-exact."""
    from d3feat_amd import ops
    rng = np.random.default_rng(N)
    M = 23
    x = rng.standard_normal((M, N)).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    cs = (rng.random(N) + 0.5).astype(np.float32) * np.where(rng.random(N) < 0.3, -1, 1).astype(np.float32)
    ch = rng.standard_normal(N).astype(np.float32)
    cst, cht = _t(cs, device), _t(ch, device)
    for strided in (False, True):
        xt = _view(x, device, N + 3, 1) if strided else _t(x, device)
        rt = _view(res, device, N + 5, 2) if strided else _t(res, device)
        for m in range(16):
            a = (cs if m & 1 else None, ch if m & 2 else None, res if m & 4 else None, bool(m & 8))
            for alpha in (0.2, 0.0):
                got = ops.affine_act(xt, cst if m & 1 else None, cht if m & 2 else None, rt if m & 4 else None, bool(m & 8), alpha)
                assert np.array_equal(bits(got.cpu().numpy()), bits(_affine_ref(x, *a, alpha))), (m, alpha, strided)


def test_affine_act_device_row_count_and_empty(device):
    """M_dev < M: rows >= M_dev keep the sentinel (C ABI, ldo > N); through ops (n_dev) the first rows are right; M = 0 is a no-op."""
    from d3feat_amd import ops
    rng = np.random.default_rng(3)
    M, N, md = 31, 20, 17
    x, res = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    cs, ch = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    xt, rt, cst, cht = _view(x, device, N + 4, 3), _t(res, device), _t(cs, device), _t(ch, device)
    want = _affine_ref(x, cs, ch, res, True, 0.2)
    xt.n_dev = _i32(md, device)
    got = ops.affine_act(xt, cst, cht, rt, True, 0.2)
    assert np.array_equal(bits(got.cpu().numpy()[:md]), bits(want[:md]))
    o = torch.full((M, N + 2), float(S), device=device)
    rc = _load().d3f_affine_act(xt.data_ptr(), xt.stride(0), M, N, cst.data_ptr(), cht.data_ptr(), rt.data_ptr(), N, 1, 0.2, o.data_ptr(),
                                N + 2, xt.n_dev.data_ptr(), _stream(device))
    assert rc == 0
    o = o.cpu().numpy()
    assert np.array_equal(bits(o[:md, :N]), bits(want[:md])) and np.all(o[md:] == S) and np.all(o[:, N:] == S)
    assert tuple(ops.affine_act(torch.empty((0, N), device=device), cst, cht).shape) == (0, N)


# ---------------------------------------------------------------------------------------------------------------------
# pack_descriptors
# ---------------------------------------------------------------------------------------------------------------------
def _pack_inputs(rng, n, C):
    return (rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32))


def _pack_ref(xyz, desc, score, n_eff, out, lens=None, group=1, keep=0, dsts=None, row_map=None):
    """The packer restated row by row: record n = [xyz | desc | score] goes to row row_map[n] of `out`, or -- when the row lies in one
    of the first `keep` clouds of a fragment (group consecutive clouds) whose destination exists -- to that destination, the
    fragment's kept rows packed from its row 0."""
    starts = np.concatenate([[0], np.cumsum(lens)]) if lens is not None else None
    for n in range(n_eff):
        rec = np.concatenate([xyz[n], desc[n], score[n:n + 1]])
        no = int(row_map[n]) if row_map is not None else n
        tgt, row = out, no
        if dsts is not None:
            b = int(np.searchsorted(starts[1:len(lens)], no, side="right"))     # last cloud whose start is <= no
            f = b // group
            if dsts[f] is not None and b - f * group < keep:
                tgt, row = dsts[f], no - int(starts[f * group])
        tgt[row] = rec


def _pack_abi(dev, xyz, dt, score, C, n, out, n_dev=None, lens=None, group=1, keep=0, dst=None, row_map=None):
    lib = _load()
    if dst is None and row_map is None:
        return lib.d3f_pack_descriptors(xyz.data_ptr(), dt.data_ptr(), dt.stride(0), C, score.data_ptr(), n, out.data_ptr(), out.stride(0),
                                        n_dev.data_ptr() if n_dev is not None else None, _stream(dev))
    return lib.d3f_pack_descriptors_to(xyz.data_ptr(), dt.data_ptr(), dt.stride(0), C, score.data_ptr(), n, out.data_ptr(), out.stride(0),
                                       n_dev.data_ptr() if n_dev is not None else None, lens.data_ptr() if lens is not None else None,
                                       lens.numel() if lens is not None else 0, group, keep,
                                       dst.data_ptr() if dst is not None else None, row_map.data_ptr() if row_map is not None else None,
                                       _stream(dev))


@pytest.mark.parametrize("C,kernel", [(32, "pack_rows_kernel"), (28, "pack_rows_kernel"), (5, "pack_rows_scalar_kernel"),
                                      (1, "pack_rows_scalar_kernel")])
def test_pack_descriptors_plain(device, C, kernel):
    """pack_launch: `((C + 4) & 3) || (ldo & 3) || (out & 15)` -> pack_rows_scalar_kernel (C = 5, 1), else pack_rows_kernel (C = 32,
    28: 16-byte pieces).  Strided desc, N_dev.  The scalar path with dst or row_map is D3F_ERR_ARG."""
    from d3feat_amd import _lib, ops
    rng = np.random.default_rng(C)
    n, nd = 77, 50
    xyz, desc, score = _pack_inputs(rng, n, C)
    want = np.full((n, C + 4), S, np.float32)
    _pack_ref(xyz, desc, score, n, want)
    xt, st = _t(xyz, device), _t(score, device)
    for dt in (_t(desc, device), _view(desc, device, C + 7, 3)):
        assert np.array_equal(bits(ops.pack_descriptors(xt, dt, st).cpu().numpy()), bits(want))
        dt.n_dev = _i32(nd, device)
        assert np.array_equal(bits(ops.pack_descriptors(xt, dt, st).cpu().numpy()[:nd]), bits(want[:nd]))
        out = torch.full((n, C + 4), float(S), device=device)
        assert _pack_abi(device, xt, dt, st, C, n, out, dt.n_dev) == 0
        o = out.cpu().numpy()
        assert np.array_equal(bits(o[:nd]), bits(want[:nd])) and np.all(o[nd:] == S)
    if kernel == "pack_rows_scalar_kernel":
        rm = _t(np.arange(n, dtype=np.int32), device)
        with pytest.raises(_lib.D3FeatLibraryError):
            ops.pack_descriptors(xt, _t(desc, device), st, row_map=rm)
        lens = _t(np.asarray([n], np.int32), device)
        with pytest.raises(_lib.D3FeatLibraryError):
            ops.pack_descriptors(xt, _t(desc, device), st, lens=lens, group=1, keep=1, dst=torch.zeros((1,), dtype=torch.int64, device=device))


# six clouds; fragments of 2: (0, 12) (7, 0) (10, 9), of 3: (5, 0, 8) (0, 13, 0) -- empty clouds at the start, in the middle and at
# the end of a group
PACK_LENS = {1: (9, 0, 14, 5, 0, 11), 2: (0, 12, 7, 0, 10, 9), 3: (5, 0, 8, 0, 13, 0)}


@pytest.mark.parametrize("C", [32, 28])
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("mode", ["row_map", "dst", "both"])
def test_pack_descriptors_to(device, C, group, mode):
    """pack_rows_kernel with per-fragment destinations and / or a row map: B = 6 clouds, fragments of `group` clouds, keep in
    {0, 1, group}, one fragment without a destination (address 0: its rows go to `out`), empty clouds at the start, in the middle and
    at the end of a group.  Every destination is its own allocation of exactly the kept rows + 8 guard rows: the guard rows and the
    rows of `out` that were redirected keep the sentinel.  group 2 also reads its row count from the device."""
    rng = np.random.default_rng(C + group)
    lens = PACK_LENS[group]
    n = int(sum(lens))
    cap = n + 6 if group == 2 else n          # group 2: N is a capacity, the real count comes from N_dev
    xyz, desc, score = _pack_inputs(rng, cap, C)
    starts = np.concatenate([[0], np.cumsum(lens)])
    row_map = None
    if mode != "dst":
        row_map = np.concatenate([starts[b] + rng.permutation(lens[b]) for b in range(6)] + [np.arange(n, cap)]).astype(np.int32)
    xt, dt, st = _t(xyz, device), _view(desc, device, C + 8, 4), _t(score, device)
    lt = _t(np.asarray(lens, np.int32), device)
    nfrag = 6 // group
    for keep in ((0, 1, group) if mode != "row_map" else (0,)):
        want_out = np.full((cap, C + 4), S, np.float32)
        kept = [int(sum(lens[f * group:f * group + keep])) for f in range(nfrag)]
        skip_f = 2 if group == 1 else 1                        # this fragment has no destination (address 0)
        want_dst = [None if (mode == "row_map" or f == skip_f) else np.full((kept[f] + 8, C + 4), S, np.float32) for f in range(nfrag)]
        _pack_ref(xyz, desc, score, n, want_out, lens, group, keep, None if mode == "row_map" else want_dst, row_map)
        out = torch.full((cap, C + 4), float(S), device=device)
        dsts = [None if w is None else torch.full(w.shape, float(S), device=device) for w in want_dst]
        dst = None if mode == "row_map" else torch.tensor([0 if d is None else d.data_ptr() for d in dsts], dtype=torch.int64,
                                                          device=device)
        rc = _pack_abi(device, xt, dt, st, C, cap, out, _i32(n, device) if cap != n else None, lt, group, keep, dst,
                       _t(row_map, device) if row_map is not None else None)
        assert rc == 0
        assert np.array_equal(bits(out.cpu().numpy()), bits(want_out)), (keep,)
        for d, w in zip(dsts, want_dst):
            if w is not None:
                assert np.array_equal(bits(d.cpu().numpy()), bits(w)), (keep,)
        if mode != "row_map" and keep:
            assert sum(kept) > 0 and np.any(np.all(want_out[:n] == S, 1))       # some rows really were redirected


@pytest.mark.parametrize("lens", [hg.LENS_B255G5, hg.LENS_B255], ids=["many-empty-clouds", "last-cloud-empty"])
def test_pack_descriptors_to_255_clouds(device, lens):
    """pack_rows_kernel on a stack of D3F_MAX_BATCH = 255 clouds (sStart[D3F_MAX_BATCH + 1] filled to its last word, d3f_find_elem's
    steps of 128 / 64 / 32): fragments of 5 clouds, keep 2, a destination per fragment -- three fragments without one (address 0) --
    and a row map that permutes the rows inside each cloud.  Destinations, guard rows and the redirected rows of `out` as
    test_pack_descriptors_to holds them."""
    C, group, keep, B = 32, 5, 2, 255
    rng = np.random.default_rng(255)
    assert len(lens) == B
    n = int(sum(lens))
    xyz, desc, score = _pack_inputs(rng, n, C)
    starts = np.concatenate([[0], np.cumsum(lens)])
    row_map = np.concatenate([starts[b] + rng.permutation(lens[b]) for b in range(B)]).astype(np.int32)
    nfrag = B // group
    kept = [int(sum(lens[f * group:f * group + keep])) for f in range(nfrag)]
    want_out = np.full((n, C + 4), S, np.float32)
    want_dst = [None if f in (0, 17, nfrag - 1) else np.full((kept[f] + 8, C + 4), S, np.float32) for f in range(nfrag)]
    _pack_ref(xyz, desc, score, n, want_out, lens, group, keep, want_dst, row_map)
    out = torch.full((n, C + 4), float(S), device=device)
    dsts = [None if w is None else torch.full(w.shape, float(S), device=device) for w in want_dst]
    dst = torch.tensor([0 if d is None else d.data_ptr() for d in dsts], dtype=torch.int64, device=device)
    rc = _pack_abi(device, _t(xyz, device), _view(desc, device, C + 8, 4), _t(score, device), C, n, out, None,
                   _t(np.asarray(lens, np.int32), device), group, keep, dst, _t(row_map, device))
    assert rc == 0
    assert np.array_equal(bits(out.cpu().numpy()), bits(want_out))
    for f, (d, w) in enumerate(zip(dsts, want_dst)):
        if w is not None:
            assert np.array_equal(bits(d.cpu().numpy()), bits(w)), f
    redirected = np.all(want_out == S, 1)
    assert 0 < redirected.sum() < n and redirected.sum() == sum(k for k, w in zip(kept, want_dst) if w is not None)
    assert max(kept) >= 3 and not np.all(want_out[starts[(nfrag - 1) * group]:] == S)   # the last fragment went to `out`


def test_pack_descriptors_to_through_ops(device):
    """ops.pack_descriptors(lens, group, keep, dst, row_map) forwards every operand (C = 32, the shipped width, group 2 keep 1)."""
    from d3feat_amd import ops
    rng = np.random.default_rng(9)
    C, lens = 32, (10, 10, 7, 12)
    n = sum(lens)
    xyz, desc, score = _pack_inputs(rng, n, C)
    starts = np.concatenate([[0], np.cumsum(lens)])
    row_map = np.concatenate([starts[b] + rng.permutation(lens[b]) for b in range(4)]).astype(np.int32)
    want_out = np.full((n, C + 4), S, np.float32)
    want_dst = [np.full((lens[0] + 8, C + 4), S, np.float32), np.full((lens[2] + 8, C + 4), S, np.float32)]
    _pack_ref(xyz, desc, score, n, want_out, lens, 2, 1, want_dst, row_map)
    dsts = [torch.full(w.shape, float(S), device=device) for w in want_dst]
    got = ops.pack_descriptors(_t(xyz, device), _t(desc, device), _t(score, device), lens=_t(np.asarray(lens, np.int32), device), group=2,
                               keep=1, dst=torch.tensor([d.data_ptr() for d in dsts], dtype=torch.int64, device=device),
                               row_map=_t(row_map, device)).cpu().numpy()
    written = want_out[:, 0] != S
    assert np.array_equal(bits(got[written]), bits(want_out[written]))
    for d, w in zip(dsts, want_dst):
        assert np.array_equal(bits(d.cpu().numpy()), bits(w))


# ---------------------------------------------------------------------------------------------------------------------
# detect_head
# ---------------------------------------------------------------------------------------------------------------------
# The tight bar of the two-cloud cases: the kernel's score error against the float64 restatement is at most TIGHT times the error
# of the float32 oracle (onp.detection_head) on the same input.  8 is a margin for the reciprocal multiply and the different
# summation order over K <= 80 terms, fixed before any measurement; it is not derived from the kernels' output.
# HEAD_RATIOS -- kernel error / oracle error measured on an MI355X for the 48 two-cloud runs of this file (printed by every run as
# "HEAD-RATIO ..."): 0.67 .. 1.63.  By kernel: head32_kernel<true> 0.67 .. 1.43 (K = 1: 1.25, K = 65: 1.26, K = 80: 1.24, the
# padded all-negative clouds with scores of 3e7: 0.96 .. 1.43), head32_kernel<false> 1.11, head_kernel<1> 0.92 .. 1.49,
# head_kernel<2> 1.00 .. 1.23, head_kernel<4> 0.78 .. 1.63 (the largest: C = 128, both clouds all-negative, length rule).  In 15 runs
# the ratio is 1.00 to two decimals: kernel and oracle miss the float64 value by the same float32 rounding.  No case needs more
# than 8, so the factor stays.
TIGHT = 8.0


def _head_run(dev, x, nb, lens, group=0, inc=None, ldx=None, xoff=0, ldi=None, ldd=None, cap=0, order=None, abi=False):
    """-> (desc [n, C], score [n]) as numpy.  Through ops.detect_head unless the case needs the C ABI (K = 0, ldd > C, capacity rows
    with a sentinel check, include_zero_dev with a group, abi=True); the ABI outputs are pre-filled and everything outside
    [0, n) x [0, C) must keep the sentinel."""
    from d3feat_amd import ops
    n, C = x.shape
    K = nb.shape[1]
    N = n + cap
    xh = np.full((N, C), np.nan, np.float32)
    xh[:n] = x
    nbh = np.zeros((N, max(K, 1)), np.int32)
    nbh[:n, :K] = nb
    xt = _view(xh, dev, ldx, xoff)
    it = _view(nbh, dev, ldi, 1, fill=0) if ldi else _t(nbh, dev)
    lt = _t(np.asarray(lens, np.int32), dev)
    inct = _t(np.asarray(inc, np.int32), dev) if inc is not None else None
    ot = _t(np.asarray(order, np.int32), dev) if order is not None else None
    if not (abi or K == 0 or ldd or cap or (inc is not None and group)):
        if ot is not None:
            it.order = ot
        d, s = ops.detect_head(xt, it, lt, inct, stack_group=group)
        assert tuple(d.shape) == (n, C) and tuple(s.shape) == (n, 1)
        return d.cpu().numpy(), s.cpu().numpy()[:, 0]
    ldd = ldd or C
    B = len(lens)
    desc = torch.full((N, ldd), float(S), device=dev)
    score = torch.full((N,), float(S), device=dev)
    scratch = torch.zeros((2 * B + 2 + (N + 3) // 4,), dtype=torch.int32, device=dev)
    rc = _load().d3f_detect_head(xt.data_ptr(), N, xt.stride(0), C, it.data_ptr(), it.stride(0), K, lt.data_ptr(),
                                 inct.data_ptr() if inct is not None else None, group, B, desc.data_ptr(), ldd, score.data_ptr(),
                                 scratch.data_ptr(), ot.data_ptr() if ot is not None else None, _stream(dev))
    assert rc == 0, rc
    d, s = desc.cpu().numpy(), score.cpu().numpy()
    assert np.all(d[n:] == S) and np.all(d[:, C:] == S) and np.all(s[n:] == S)
    return d[:n, :C], s[:n]


def _head_check(name, gd, gs, x, nb, lens, group=0, inc=None, relative=False):
    """Descriptors 1e-5, scores 1e-4 absolute against the float64 restatement (relative to max(1, |want|) only where a padded cloud of
    all-negative features makes scores of order 1e7); on two-cloud stacks also TIGHT x the float32 oracle's own error."""
    from oracle import head_cases as hc
    from oracle import network_np as onp
    # inside the kernels' stated contract: head32_kernel divides neighbour rows by the point's own denominator
    assert hc.neighbours_stay_in_cloud(nb, lens)
    d64, s64, y = onp.detection_head_f64(x, nb, lens, group, inc)
    # the one discontinuity: a row's sum is exactly zero in every precision (all-zero rows, [t, -t, 0, ...]) or far from zero.  The
    # scale is the row's own cloud (the rounding error of a row sum scales with its terms; a padded all-negative cloud has y ~ 1e7)
    a = 0
    for l in lens:
        if l:
            rs, big = y[a:a + l].sum(1), np.abs(y[a:a + l]).max()
            exact0 = np.all(y[a:a + l] == 0, 1) | ((y[a:a + l, :2].sum(1) == 0) & np.all(y[a:a + l, 2:] == 0, 1))
            assert np.all(exact0 | (np.abs(rs) >= 1e-3 * big)), name
        a += l
    assert np.all(np.isfinite(gd)) and np.all(np.isfinite(gs)), name
    ed = np.abs(gd - d64).max() if len(gd) else 0.0
    assert ed <= 1e-5, "%s: descriptor err %.3e" % (name, ed)
    scale = max(1.0, np.abs(s64).max()) if relative else 1.0
    es = np.abs(gs - s64).max() if len(gs) else 0.0
    msg = "%s: score err %.3e (|want| max %.3g)" % (name, es, np.abs(s64).max() if len(gs) else 0)
    if len(lens) == 2 and min(lens) > 0 and group in (0, 2):
        n = sum(lens)
        inc_v = onp.include_zero_rule(lens) if inc is None else list(inc)
        o32 = onp.detection_head(torch.from_numpy(x), np.where((nb < 0) | (nb >= n), n, nb), hc.in_batches(lens, inc_v),
                                 np.asarray(lens)).numpy()[:, 0]
        e32 = np.abs(o32 - s64).max()
        msg += "; float32 oracle err %.3e, kernel / oracle ratio %.2f" % (e32, es / e32)
        print("HEAD-RATIO " + msg)
        assert es <= 1e-4 * scale, msg
        assert es <= TIGHT * e32, msg
    else:
        print("HEAD " + msg)
        assert es <= 1e-4 * scale, msg


# (id, C, K, lens, group, head_case options, _head_run options, relative)
HEAD = [
    # vec32 = `C == 32 && ldx % 4 == 0 && ldd % 4 == 0 && ((x | desc) & 15) == 0` -> head32_rowflag + head32_kernel<true>
    # (`d3f_fits_u24(N + 1, ldx) && (N + 1) * ldx < 2^30`); `ldx == C && C % 4 == 0 && (x & 15) == 0` -> head_max_kernel<true>
    ("head32<true>+head_max<true>-C32-K33-B2", 32, 33, (60, 45), 0, {}, {}, False),
    ("head32<true>-C32-K1-B2-equal", 32, 1, (40, 40), 0, {}, {}, False),
    ("head32<true>-C32-K15-B2", 32, 15, (45, 60), 0, {}, {}, False),
    ("head32<true>-C32-K16-B2", 32, 16, (50, 30), 2, {}, {}, False),
    ("head32<true>-C32-K17-B2", 32, 17, (50, 30), 0, {}, {}, False),
    ("head32<true>-C32-K31-B2", 32, 31, (33, 64), 0, {}, {}, False),
    ("head32<true>-C32-K32-B2", 32, 32, (33, 64), 0, {}, {}, False),
    ("head32<true>-C32-K65-B2", 32, 65, (48, 48), 0, {}, {}, False),
    ("head32<true>-C32-K80-B2", 32, 80, (70, 41), 0, {}, {}, False),
    ("head32<true>-C32-K0-B2-abi", 32, 0, (40, 25), 0, {}, {}, False),
    # C = 32 as the column slice [16, 48) of a 48-wide matrix: still vec32, but ldx != C -> head_max_kernel<false>
    ("head32<true>+head_max<false>-C32-ldx48", 32, 35, (60, 45), 0, {}, dict(ldx=48, xoff=16, ldi=40), False),
    # C = 32 where vec32 fails -> head_kernel<1> sees 32 channels: ldx = 33 (ldx % 4 != 0), and an unaligned base (slice [1, 33))
    ("head_kernel<1>-C32-ldx33-abi", 32, 35, (60, 45), 0, {}, dict(ldx=33, xoff=0, abi=True), False),
    ("head_kernel<1>-C32-unaligned-view", 32, 30, (60, 45), 0, {}, dict(ldx=48, xoff=1), False),
    ("head_kernel<1>-C32-ldd38-abi", 32, 33, (60, 45), 0, {}, dict(ldd=38), False),           # ldd % 4 != 0 fails vec32 too
    ("head32<true>-C32-ldd40-capacity-abi", 32, 33, (60, 45), 0, {}, dict(ldd=40, cap=13), False),
    # C != 32: `C <= 32` -> head_kernel<1>, `C <= 64` -> <2>, else <4>; head_max<true> iff ldx == C, C % 4 == 0, aligned
    ("head_kernel<1>+head_max<false>-C1-K16", 1, 16, (50, 30), 0, {}, {}, False),
    ("head_kernel<1>+head_max<true>-C20-K7", 20, 7, (45, 70), 0, {}, {}, False),
    ("head_kernel<1>-C20-K33", 20, 33, (45, 70), 0, {}, {}, False),
    ("head_kernel<1>-C20-K0-abi", 20, 0, (45, 30), 0, {}, {}, False),
    ("head_kernel<2>+head_max<false>-C33-K17", 33, 17, (70, 45), 0, {}, {}, False),
    ("head_kernel<2>-C33-K1", 33, 1, (40, 40), 0, {}, {}, False),
    ("head_kernel<2>+head_max<true>-C64-K40", 64, 40, (50, 50), 0, {}, {}, False),
    ("head_kernel<2>-C64-K65", 64, 65, (50, 35), 0, {}, {}, False),
    ("head_kernel<2>-C64-K15-ldx72", 64, 15, (50, 35), 0, {}, dict(ldx=72, xoff=4), False),
    ("head_kernel<4>-C100-K31", 100, 31, (40, 64), 0, {}, {}, False),
    ("head_kernel<4>-C100-K32", 100, 32, (40, 64), 0, {}, {}, False),
    ("head_kernel<4>+head_max<true>-C128-K33", 128, 33, (40, 64), 0, {}, {}, False),
    ("head_kernel<4>-C128-K80", 128, 80, (64, 40), 0, {}, {}, False),
    ("head_kernel<4>-C65-K16-capacity-abi", 65, 16, (30, 50), 0, {}, dict(cap=9, ldd=70), False),
    # stacks: B in {1, 3, 6}, stack_group in {0, 1, 2, 3}, an empty cloud between two others, capacity rows
    ("head32<true>-B1", 32, 30, (77,), 0, {}, {}, False),
    ("head_kernel<2>-B1-g1", 40, 30, (77,), 1, {}, {}, False),
    ("head32<true>-B3-g0-empty-middle", 32, 33, (40, 0, 35), 0, {}, {}, False),
    ("head_kernel<1>-B3-g3-empty-middle-capacity-abi", 20, 17, (40, 0, 35), 3, {}, dict(cap=11), False),
    ("head32<true>-B3-g1", 32, 17, (40, 22, 35), 1, {}, {}, False),
    ("head32<true>-B6-g2-negative", 32, 30, (40, 40, 50, 30, 25, 45), 2, dict(negative=(0, 1, 2, 3, 4, 5)), {}, True),
    ("head32<true>-B6-g0-negative", 32, 30, (40, 40, 50, 30, 25, 45), 0, dict(negative=(0, 1, 2, 3, 4, 5)), {}, True),
    ("head_kernel<4>-B6-g3-negative-empty", 100, 17, (40, 0, 50, 30, 30, 30), 3, dict(negative=(0, 2, 3, 4, 5)), {}, True),
    ("head_kernel<2>-B6-g1", 64, 9, (20, 31, 12, 40, 8, 25), 1, {}, {}, False),
    ("head32<true>-B6-g3-capacity-abi", 32, 33, (20, 31, 12, 40, 8, 25), 3, {}, dict(cap=21), False),
    # all-negative clouds: the padded one (length rule: the shorter / both of an equal pair) has the zero row as its maximum ->
    # y = x / 1e-6 and scores of order 1e7: relative bar.  |y - mean| > 15 on both sides of the softplus shortcuts
    ("head32<true>-B2-equal-negative", 32, 30, (60, 60), 0, dict(negative=(0, 1)), {}, True),
    ("head32<true>-B2-short-negative", 32, 30, (70, 45), 0, dict(negative=(1,)), {}, True),
    ("head32<true>-B2-long-negative", 32, 30, (70, 45), 0, dict(negative=(0,)), {}, False),    # unpadded: den = max < 0, y >= 1
    ("head_kernel<2>-B2-negative", 48, 20, (45, 70), 0, dict(negative=(0, 1)), {}, True),
    ("head32<true>-B2-scaled-1e3", 32, 30, (70, 45), 0, dict(scale={1: 1e3}), {}, False),
    ("head_kernel<4>-B2-scaled-1e3", 128, 17, (70, 45), 0, dict(scale={0: 1e3}), {}, False),
    # stacks of up to D3F_MAX_BATCH = 255 clouds (the stacks of head_grad_np.GRID's b255 / b255g5 / b129): head_max_init_kernel's thread
    # per cloud and its serial prefix and group scans, head_max_kernel's grid (chunks <= ceil(512 / B), B), d3f_find_elem's steps of
    # 128 / 64 / 32 (from 129 / 65 / 33 clouds on) in the head kernels; groups that divide B and groups that do not; whole empty groups
    ("head_kernel<1>-B255-g0", 20, 5, hg.LENS_B255, 0, {}, {}, False),
    ("head32<true>-B255-g5-empty-groups", 32, 5, hg.LENS_B255G5, 5, {}, {}, False),
    ("head_kernel<1>-B129-g0", 20, 9, hg.LENS_B129, 0, {}, {}, False),
    ("head32<true>-B255-g4-not-dividing", 32, 5, hg.LENS_B255, 4, {}, {}, False),
    ("head_kernel<2>-B129-g8-not-dividing-capacity-abi", 64, 9, hg.LENS_B129, 8, {}, dict(cap=5), False),
    ("head32<true>-B255-g7-not-dividing-empty-groups", 32, 5, hg.LENS_B255G5, 7, {}, {}, False),
]


@pytest.mark.parametrize("name,C,K,lens,group,gen,run,relative", HEAD, ids=[h[0] for h in HEAD])
def test_detect_head(device, name, C, K, lens, group, gen, run, relative):
    """d3f_detect_head, one launcher branch per case (the id names the kernels; the conditions are quoted in HEAD).  Inputs from
    oracle.head_cases.head_case: 20 % shadow slots (== N, > N, negative, 2^30), all-zero and cancelling rows that appear as neighbours
    (present, not counted), a point with only shadow slots (count clamps to 1), a row of squared norm 1.8e-11 (descriptor clamp).

    Kernel / float32-oracle error ratios of the two-cloud cases, measured on an MI355X: 0.67 .. 1.43 over the 35 two-cloud cases of
    this test (see HEAD_RATIOS at TIGHT for the figures by kernel); the bar is 8."""
    from oracle import head_cases as hc
    x, nb = hc.head_case(sum(ord(c) for c in name), C, K, lens, **gen)
    gd, gs = _head_run(device, x, nb, lens, group, **run)
    _head_check(name, gd, gs, x, nb, lens, group, None, relative)


@pytest.mark.parametrize("C", [32, 20, 128], ids=["head32<true>", "head_kernel<1>", "head_kernel<4>"])
def test_detect_head_explicit_include_zero(device, C):
    """include_zero_dev given: it replaces the length rule (and stack_group is ignored).  (70, 45) all-negative with (1, 0) -- the
    opposite of the rule's (0, 1) -- and with (0, 0) and (1, 1); B = 4 with stack_group 2 and a vector that contradicts the rule in
    every group (C ABI).  The outputs differ from the rule's wherever the vector does: the operand is really read."""
    from oracle import head_cases as hc
    lens = (70, 45)
    x, nb = hc.head_case(50 + C, C, 21, lens, negative=(0, 1))
    seen = {}
    for inc in ((1, 0), (0, 0), (1, 1), None):
        gd, gs = _head_run(device, x, nb, lens, 0, inc)
        _head_check("include_zero %s C %d" % (inc, C), gd, gs, x, nb, lens, 0, inc, relative=inc is None or any(inc))
        seen[inc] = gs
    assert np.abs(seen[(1, 0)][:70] - seen[None][:70]).max() > 1.0 and np.abs(seen[(1, 0)][70:] - seen[None][70:]).max() > 1.0
    lens = (40, 40, 50, 30)
    x, nb = hc.head_case(60 + C, C, 21, lens, negative=(0, 1, 2, 3))
    inc = (0, 1, 1, 0)                                                # the rule in groups of two: (1, 1, 0, 1)
    gd, gs = _head_run(device, x, nb, lens, 2, inc)
    _head_check("include_zero with a group C %d" % C, gd, gs, x, nb, lens, 2, inc, relative=True)


@pytest.mark.parametrize("C,abi", [(32, False), (32, True), (64, False), (100, True)],
                         ids=["head32<true>-ops-order", "head32<true>-abi", "head_kernel<2>-ops-order", "head_kernel<4>-abi"])
def test_detect_head_row_order(device, C, abi):
    """row_order: a random permutation of the rows gives bit-identical outputs (each row's arithmetic does not depend on the visiting
    order), with capacity rows beyond the real count through the C ABI."""
    from oracle import head_cases as hc
    lens = (37, 0, 52, 20)
    n = sum(lens)
    x, nb = hc.head_case(70 + C, C, 19, lens)
    perm = np.random.default_rng(C).permutation(n)
    kw = dict(cap=7) if abi else {}
    d0, s0 = _head_run(device, x, nb, lens, 2, abi=abi, **kw)
    d1, s1 = _head_run(device, x, nb, lens, 2, order=perm, abi=abi, **kw)
    assert np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(s0), bits(s1))
    _head_check("row_order C %d" % C, d1, s1, x, nb, lens, 2)


@pytest.mark.parametrize("C", [32, 64], ids=["head_max<true>-unrolled+head32<true>", "head_max<true>-unrolled+head_kernel<2>"])
def test_detect_head_one_large_cloud(device, C):
    """head_max_kernel<true>'s four-loads-in-flight loop runs only when a cloud holds more than 3 * gridDim.x * 256 float4 (chunks =
    min(ceil(N * C / 4096), ceil(512 / B))): one cloud of 20000 rows (B = 1: 160000 / 320000 float4 against 3 * 40192 / 80128)."""
    from oracle import head_cases as hc
    lens = (20000,)
    x, nb = hc.head_case(80 + C, C, 8, lens)
    x[12345] = np.abs(x[12345])
    x[12345, 3] = 11.0                       # the cloud's maximum sits deep inside the unrolled range
    gd, gs = _head_run(device, x, nb, lens)
    _head_check("large cloud C %d" % C, gd, gs, x, nb, lens)


def test_detect_head_beyond_24_bit_addressing(device):
    """head32_kernel<false>: `d3f_fits_u24(N + 1, ldx) && (N + 1) * ldx < 2^30` fails for 1024 rows at a row stride of 2^20 floats
    (1025 * 2^20 >= 2^30; a 4 GiB allocation of which only the 32 used columns are written).  Shadow slots must read zeros, not
    row 0.  head_max_kernel<false> (ldx != C)."""
    from d3feat_amd import ops
    from oracle import head_cases as hc
    lens, ld = (600, 424), 1 << 20
    n = sum(lens)
    x, nb = hc.head_case(91, 32, 33, lens)
    x[0] = 7.5                               # row 0 is what a mishandled shadow slot would add
    store = torch.empty(((n - 1) * ld + 32,), dtype=torch.float32, device=device)
    xt = store.as_strided((n, 32), (ld, 1))
    xt.copy_(_t(x, device))
    d, s = ops.detect_head(xt, _t(nb, device), _t(np.asarray(lens, np.int32), device), None)
    gd, gs = d.cpu().numpy(), s.cpu().numpy()[:, 0]
    del xt, store, d, s
    torch.cuda.empty_cache()
    _head_check("head32<false>", gd, gs, x, nb, lens)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: D3F_ERR_ARG without a launch
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(device):
    from d3feat_amd import _lib, ops
    lib, s = _load(), _stream(device)
    x = torch.zeros((16, 132), device=device)
    xb = torch.zeros((16, 8), dtype=torch.bfloat16, device=device)
    idx = torch.zeros((16, 8), dtype=torch.int32, device=device)
    lens = torch.tensor([16], dtype=torch.int32, device=device)
    out = torch.zeros((16, 132), device=device)
    sc = torch.zeros((64,), dtype=torch.int32, device=device)
    p = lambda t: t.data_ptr()
    # head: C = 129; ldx < C; ld_idx < K
    assert lib.d3f_detect_head(p(x), 16, 132, 129, p(idx), 8, 8, p(lens), None, 0, 1, p(out), 132, p(out), p(sc), None, s) == ERR_ARG
    with pytest.raises(_lib.D3FeatLibraryError):
        ops.detect_head(x[:, :129], idx, lens, None)
    assert lib.d3f_detect_head(p(x), 16, 31, 32, p(idx), 8, 8, p(lens), None, 0, 1, p(out), 132, p(out), p(sc), None, s) == ERR_ARG
    assert lib.d3f_detect_head(p(x), 16, 132, 32, p(idx), 7, 8, p(lens), None, 0, 1, p(out), 132, p(out), p(sc), None, s) == ERR_ARG
    # pooling: ldx < C; ld_idx < K; bf16 with C % 4 != 0
    assert lib.d3f_ind_max_pool(p(x), 16, 63, 64, p(idx), 16, 8, 8, p(out), 132, None, None, None, None, 0, s) == ERR_ARG
    assert lib.d3f_ind_max_pool(p(x), 16, 132, 64, p(idx), 16, 7, 8, p(out), 132, None, None, None, None, 0, s) == ERR_ARG
    assert lib.d3f_ind_max_pool(p(xb), 16, 8, 6, p(idx), 16, 8, 8, p(out), 132, None, None, None, None, 1, s) == ERR_ARG
    with pytest.raises(_lib.D3FeatLibraryError):
        ops.ind_max_pool(xb[:, :6], idx)
    # upsampling, epilogue, packer: ldx < C
    assert lib.d3f_closest_pool_cat(p(x), 16, 4, 5, p(idx), 16, 8, None, 0, 0, p(out), 132, None, None, s) == ERR_ARG
    assert lib.d3f_closest_pool_cat(p(x), 16, 132, 5, p(idx), 16, 0, None, 0, 0, p(out), 132, None, None, s) == ERR_ARG
    assert lib.d3f_affine_act(p(x), 4, 16, 5, None, None, None, 0, 0, 0.2, p(out), 132, None, s) == ERR_ARG
    assert lib.d3f_pack_descriptors(p(x), p(x), 31, 32, p(x), 16, p(out), 36, None, s) == ERR_ARG
    torch.cuda.synchronize(device)
    assert float(out.abs().max()) == 0.0                # nothing was launched
