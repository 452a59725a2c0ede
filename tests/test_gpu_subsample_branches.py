"""Every entry form, every one-workgroup instantiation, every sort pass count and every iteration-order round boundary of the grid
subsampling -- csrc/grid_subsample.hip, gs_small.h, radix_sort.h, prims.h -- against the C oracle (coracle.batch_grid_subsampling,
coracle.grid_subsampling): rows through bits(), lengths and status with np.array_equal.  Nothing compares a kernel with a kernel,
nothing has a tolerance.

Inputs: oracle/subsample_cases.py (seeded; the oracle's rows are computed once per process).  Every case states the voxel count it
means to have, the form each of its calls means to take, the width of its sort key and its number of order rounds;
tests/test_subsample_cases.py checks those statements on the CPU against the oracle and a host mirror of the dispatcher, and
profiles/subsample_branch_tests_kernel_stats.csv (the kernel trace of this file alone) shows that the library launched what the
mirror says.  Capacity-mode calls (sort, one-workgroup, in-place) give N_cap > sum(lens) with rows of 1e30 beyond the real points,
write into an output pre-filled with a sentinel whose rows from M on must keep it, and are made TWICE on the same workspace; the
workspace is the one stream-ordered buffer every form shares (ops.workspace).  The in-place calls pass every cloud as its own
allocation, in DEscending address order, the first cloud at a 4-byte-aligned address that is not 16-byte aligned.
The synchronous call is the only way into the hash form (capacity mode always sorts), so "all forms report alike" means the sort,
the one-workgroup and the in-place form for the capacity limits, and the hash form raises.

Branch -> test
--------------
  hash form (gs_insert / gs_chain / gs_rank / gs_accum)       test_case[*-hash]
  sort form (gs_sortkey / rs_hist / rs_scatter / gs_heads / gs_runs / gs_emit)     test_case[*-sort], [*-inplace]
  gs_small_kernel<256,8> <512,8> <1024,8> <1024,12> <1024,16>  test_case[wg-2048 / 2049, 4096 / 4097, 8192 / 8193, 12288 / 12289, 16384
                                                              -small]: both edges of each band; [wg-16385-sort]: one point more
  nbmax 1109 / 2357 / 5087 of the one-workgroup order rounds  test_case[rounds-*-small]; M == elem_cap: 14, 128, 542, 1110, 2358;
                                                              M == elem_cap == nbmax: 1109, 2357, 5087
  order rounds 1..7 in gs_order_small_kernel                  test_case[rounds-1 .. rounds-1109]: M on both sides of 13, 29, .., 1109
  grid-wide rounds (insert / scan_tiles / place), 1..4        test_case[rounds-1110 .. rounds-10274]: both sides of 2357, 5087, 10273
  clouds of different round counts in one launch              test_case[mixed-*] (M = 5, 1110, 60, 2358, 1), [many-255-*] (255 clouds)
  sort passes 1, 2, 3, 4; kb == 32 (no element field)         test_case[passes-8 / 9, 16 / 17, 24 / 25, 32 -sort / -inplace]
  D3F_ST_KEY_WIDTH                                            test_key_width_is_reported (sort with B = 2, one-workgroup > 2^32 cells);
                                                              2^32 cells exactly in one workgroup: test_case[passes-32-small]
  sort tiles of 8192: n = 8191, 8192, 8193, 16385             test_case[tile-*]; wave 1 holds pieces of three clouds (one_cloud == false)
  run walking: LDS part, continuation past position 256       test_case[run-<points>-at-<start mod 256>-*]: 2 at 255 (crosses), 255 at 1 (ends
                                                              on the edge), 256 at 0 (fills a block), 256 at 130, 257 at 0, 700 at 50 and at
                                                              255 (three and four blocks); the same clouds walk the hash form's chains and
                                                              the one-workgroup head's loop
  summation order                                             every run-* and shift-* case has a voxel whose reversed sum differs
  key arithmetic: shifts, flat grid, identical points, points on origin + k dl, dl 0.03 / 0.011 / 0.3     test_case[shift-*], [flat-*],
                                                              [identical-*], [on-grid-*]
  gs_mod with keys in [2^53, 2^56); D3F_ST_KEY_RANGE          test_keys_beyond_2_53_hash_form[10], [40]; test_key_range_raises
  capacities M_cap / elem_cap / elem_points                   test_capacities_*
  D3F_ST_EMPTY_ELEMENT, D3F_ST_NEG_CELL in every form         test_empty_element_*, test_negative_cell_*
  features / classes through the grid-wide rounds             test_features_and_classes[*] (gs_accum with fdim, gs_fill / gs_labels)
  one form after another on one workspace                     test_forms_back_to_back_on_one_workspace

Where include/d3feat_amd.h is silent nothing is asserted: the ROWS and LENGTHS a capacity-mode call returns together with
D3F_ST_EMPTY_ELEMENT or D3F_ST_NEG_CELL (the reference is undefined there: cloud.cpp:30,51 and the (size_t) cast of a negative
index); only the flag is checked.  By the kernels' code no form leaves its buffers for these inputs: an empty cloud is skipped
(gs_prep gives it a 1 x 1 x 1 grid, the one-workgroup kernel returns before it reads) and a negative cell is clamped to 0.

Two defects found, both in how a capacity-mode call REPORTS, both fixed with this file (each case below fails on the parent's
kernels and passes on the fix; no defect found in what any form computes: all other cases pass on the parent's kernels as well):
  * test_capacities_one_voxel_short_are_reported_alike[M_cap], [elem_cap]: the sort form (and with it the in-place form) reported
    [0, D3F_ST_OUT_OVERFLOW] and lengths of 0, as the header says, but gs_emit_kernel took its row count from the workspace's own
    count, which the overflow does not zero, and wrote up to M_cap barycentres into the output it had just declared empty (in
    bounds; for a cloud above elem_cap at positions left over from an earlier call).  The one-workgroup form writes nothing.
    Fix: gs_emit_kernel returns when the call is reported empty.
  * test_capacities_cloud_above_elem_points_is_reported: the header promises D3F_ST_OUT_OVERFLOW for a cloud above elem_points_cap;
    the one-workgroup kernel compared the length with the T * R points of the instantiation it was launched as, so a cloud of
    elem_points_cap + 1 .. T * R points was subsampled without a word.  Fix: the kernel is given the caller's capacity.

Cost, measured on an MI355X: the 196 cases take 3.0 s run alone (pytest's figure; the slowest are the first calls of the process,
test_case[rounds-1-hash] 0.18 s, [rounds-29-hash] 0.13 s, [rounds-10273-hash] 0.12 s; nothing else reaches 0.05 s).  One complete
`pytest -m gpu tests` run with this file took 347.8 s in the same visit (831 passed, 5 skipped) and none of this file's cases is
among that run's 40 slowest (0.43 s and up).  Every other test is the parent's and the two fixes add one load to one kernel each,
so the parent's suite is that run less this file: about 345 s, to which the file adds under 1 %.
"""
import numpy as np
import pytest
import torch

from conftest import bits
from oracle import subsample_cases as sc

pytestmark = pytest.mark.gpu

SENT = sc.SENTINEL
_ORACLE = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle(coracle, case):
    if case.name not in _ORACLE:
        p, lens = case.data()
        want_p, want_l = coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), case.dl)
        want_p.setflags(write=False)
        _ORACLE[case.name] = (want_p, want_l)
    return _ORACLE[case.name]


def _own_allocations(p, lens, dev):
    """every cloud in an allocation of its own -> (address table i64[B] on the device, the tensors that own the memory).  Cloud b
    gets the b-th HIGHEST address, and cloud 0 starts one float into its allocation (4-byte aligned, not 16)."""
    B = len(lens)
    room = 3 * max(max(lens), 1) + 8
    bufs = sorted((torch.full((room,), float(sc.FAR), dtype=torch.float32, device=dev) for _ in range(B)), key=lambda t: -t.data_ptr())
    offs = np.concatenate([[0], np.cumsum(lens)])
    addr = []
    for b in range(B):
        skip = 1 if b == 0 else 4 * (b % 2)
        view = bufs[b][skip: skip + 3 * lens[b]]
        view.copy_(_t(p[offs[b]:offs[b + 1]].reshape(-1), dev))
        addr.append(bufs[b].data_ptr() + 4 * skip)
    assert addr[0] % 16 == 4 and (B < 2 or all(addr[b] > addr[b + 1] for b in range(B - 1)))
    return torch.tensor(addr, dtype=torch.int64, device=dev), bufs


def _capacity_call(call, p, lens, dl, dev, reps=2):
    """`reps` calls of the capacity-mode entry into ONE sentinel-filled output on the shared workspace -> per call
    (rows f32[M_cap, 3], sub_lens, [M, flags])"""
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    n, B = len(p), len(lens)
    assert call.N_cap > n or n == 0
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    if call.kind == "inplace":
        table, keep = _own_allocations(p, lens, dev)
    else:
        P = _t(sc.with_tail(p, call.N_cap - n), dev)
    nbytes = lib.d3f_grid_subsample_workspace_bytes(call.N_cap, B, 0, 0)
    res = []
    for _ in range(reps):
        ws = ops.workspace(nbytes, dev)
        out = torch.full((call.M_cap, 3), float(SENT), dtype=torch.float32, device=dev)
        sub_l = torch.full((B,), -5, dtype=torch.int32, device=dev)
        status = torch.full((2,), 77, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if call.kind == "inplace":
            rc = lib.d3f_batch_grid_subsample_async_inplace(table.data_ptr(), call.N_cap, lens_t.data_ptr(), B, float(dl), out.data_ptr(),
                                                            call.M_cap, call.elem_cap, sub_l.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                            ws.numel(), stream)
        else:
            rc = lib.d3f_batch_grid_subsample_async(P.data_ptr(), call.N_cap, lens_t.data_ptr(), B, float(dl), out.data_ptr(), call.M_cap,
                                                    call.elem_cap, call.elem_points, sub_l.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), stream)
        _lib.check(rc, "batch_grid_subsample_async")
        res.append((out.cpu().numpy(), sub_l.cpu().numpy(), status.tolist()))
    return res


def _equal_oracle(res, want_p, want_l):
    rows, sub_l, st = res
    m = len(want_p)
    assert st == [m, 0], st
    assert np.array_equal(sub_l, want_l)
    assert np.array_equal(bits(rows[:m]), bits(want_p))
    assert (bits(rows[m:]) == bits(np.asarray([SENT]))[0]).all()          # rows from M on keep the sentinel


def _reported(res, flag, B):
    """an over-capacity call: [0, flag], every length 0, no row written"""
    rows, sub_l, st = res
    assert st == [0, flag], st
    assert np.array_equal(sub_l, np.zeros(B, np.int32))
    assert (bits(rows) == bits(np.asarray([SENT]))[0]).all()


def _hash_equal_oracle(p, lens, dl, dev, want_p, want_l):
    from d3feat_amd import ops
    got_p, got_l, _, _ = ops.batch_grid_subsample(_t(p, dev), lens, dl)
    assert np.array_equal(got_l.cpu().numpy(), want_l)
    assert got_p.shape == want_p.shape and np.array_equal(bits(got_p.cpu().numpy()), bits(want_p))


def _run_call(call, case, coracle, dev):
    p, lens = case.data()
    want_p, want_l = _oracle(coracle, case)
    assert list(want_l) == case.M and call.form() == call.want          # (the CPU file checks both for every case as well)
    if call.kind == "hash":
        _hash_equal_oracle(p, lens, case.dl, dev, want_p, want_l)
    else:
        for res in _capacity_call(call, p, lens, case.dl, dev):
            _equal_oracle(res, want_p, want_l)


_PAIRS = [(c.name, k) for c in sc.cases().values() for k in c.kinds]


@pytest.mark.parametrize("name,kind", _PAIRS, ids=["%s-%s" % nk for nk in _PAIRS])
def test_case(device, coracle, name, kind):
    case = sc.cases()[name]
    call = next(k for k in case.calls() if k.kind == kind)
    _run_call(call, case, coracle, device)


def test_forms_back_to_back_on_one_workspace(device, coracle):
    """hash, sort, one-workgroup, in-place and hash again on the 'mixed' stack, one after the other on one workspace buffer: a form
    must not depend on what another left behind (the sort form reuses the hash form's arrays under other names, the one-workgroup
    form lays its staging blocks over all of them)."""
    from d3feat_amd import _lib, ops
    case = sc.cases()["mixed"]
    p, lens = case.data()
    calls = {k.kind: k for k in case.calls()}
    nbytes = max(_lib.load().d3f_grid_subsample_workspace_bytes(k.N_cap or len(p), len(lens), 0, 0) for k in calls.values())
    ws = ops.workspace(nbytes, device)
    for kind in ("hash", "sort", "small", "inplace", "hash", "small", "sort"):
        _run_call(calls[kind], case, coracle, device)
        assert ops.workspace(1, device).data_ptr() == ws.data_ptr()


def test_key_width_is_reported(device, coracle):
    """2048 x 2048 x 1024 cells fill the 32-bit sort key, so a second cloud in the stack (one element bit) is reported by the sort
    form and by the in-place form; one cell layer more is reported by the one-workgroup form.  (With B = 1 the same cloud is
    subsampled by all forms: test_case[passes-32-*].)"""
    case = sc.cases()["passes-32"]
    p32, _ = case.data()
    one = sc.lattice(2001, 1, 1.0, per=1)
    p, lens = sc.stack([p32, one])
    n = len(p)
    assert sc.sort_bits(p, lens, 1.0) == (32, 1, None)
    for kind in ("sort", "inplace"):
        call = sc.Call(kind, max(n + 37, 5200), 5200, 0, 0)
        assert call.form() == "sort"
        for res in _capacity_call(call, p, lens, 1.0, device):
            _reported(res, sc.ST_KEY_WIDTH, 2)
    want_p, want_l = coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), 1.0)
    _hash_equal_oracle(p, lens, 1.0, device, want_p, want_l)             # the synchronous call answers
    wide = sc.box_cloud(3100, 2048, 2048, 1025, 50)
    assert sc.grid_dims(wide, 1.0)[1] == [2048, 2048, 1025]
    call = sc.Call("small", len(wide) + 37, 200, 1109, len(wide))
    assert call.form() == ("small", 256, 8, 1109)
    for res in _capacity_call(call, wide, [len(wide)], 1.0, device):
        _reported(res, sc.ST_KEY_WIDTH, 1)


@pytest.mark.parametrize("M", sorted(sc.KEY64))
def test_keys_beyond_2_53_hash_form(device, coracle, M):
    """dl = 1.0, a grid of 2^19 x 2^19 x 2^16 (M = 10) / 2^18 (M = 40) cells: every voxel but the first corner has a key in
    [2^53, 2^54) / [2^55, 2^56), where (double)key of gs_mod's quotient estimate is inexact; 10 voxels take the 13-bucket round, 40
    the rounds of 13, 29 and 59 buckets.  Hash form only: such keys do not fit the 32-bit sort key."""
    NZ, zmin, lg = sc.KEY64[M]
    p = sc.key64_cloud(M, NZ, zmin)
    k = np.sort(np.unique(sc.voxel_keys(p, 1.0)))
    assert len(k) == M and k[0] == 0 and int(k[1]) >= 1 << lg and int(k[-1]) < 1 << (lg + 1) and int(k[-1]) < 1 << 56
    assert (k[1:] % np.uint64(2) == 1).sum() > 0                         # odd keys above 2^53: not representable as a double
    want_p, want_l = coracle.batch_grid_subsampling(p, np.asarray([len(p)], np.int32), 1.0)
    assert list(want_l) == [M]
    _hash_equal_oracle(p, [len(p)], 1.0, device, want_p, want_l)


def test_key_range_raises(device):
    """one more axis bit: 2^19 x 2^19 x (2^18 + 1) cells, the far corner has key >= 2^56 -> D3F_ST_KEY_RANGE through the status check"""
    from d3feat_amd import _lib, ops
    p = sc.box_cloud(9100, 1 << 19, 1 << 19, (1 << 18) + 1, 10, 1.0, zmin=1 << 17)
    assert int(sc.voxel_keys(p, 1.0).max()) >= 1 << 56
    with pytest.raises(_lib.D3FeatLibraryError, match="2\\^56"):
        ops.batch_grid_subsample(_t(p, device), [len(p)], 1.0)
    status = torch.tensor([0, _lib.ST_KEY_RANGE], dtype=torch.int32, device=device)
    with pytest.raises(_lib.D3FeatLibraryError, match="2\\^56"):
        ops.check_status(status, "test")


# ---- capacities ----------------------------------------------------------------------------------------------------------------
CAP_M = [300, 500, 40]


@pytest.fixture(scope="module")
def cap_stack(coracle):
    p, lens = sc.stack([sc.lattice(9200 + i, M, 0.05, sc.SHIFTS[i]) for i, M in enumerate(CAP_M)])
    want_p, want_l = coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), 0.05)
    assert list(want_l) == CAP_M
    return p, lens, want_p, want_l


def _cap_calls(n, lens, M_cap, elem_cap, elem_points=None):
    """the three capacity-mode forms with the same voxel capacities: the sort form is forced by N_cap > 16384"""
    ep = max(lens) if elem_points is None else elem_points
    calls = [sc.Call("sort", 16500, M_cap, elem_cap, 0), sc.Call("small", n + 37, M_cap, elem_cap, ep), sc.Call("inplace", n + 37, M_cap, elem_cap, 0)]
    assert [c.form() for c in calls] == ["sort", ("small", 256, 8, 1109), "sort"]
    return calls


def test_capacities_exactly_met_are_accepted(device, cap_stack):
    p, lens, want_p, want_l = cap_stack
    for call in _cap_calls(len(p), lens, sum(CAP_M), max(CAP_M)):          # M == M_cap and the largest cloud == elem_cap
        for res in _capacity_call(call, p, lens, 0.05, device):
            _equal_oracle(res, want_p, want_l)


@pytest.mark.parametrize("what", ["M_cap", "elem_cap"])
def test_capacities_one_voxel_short_are_reported_alike(device, cap_stack, what):
    p, lens, _, _ = cap_stack
    M_cap, elem_cap = (sum(CAP_M) - 1, 0) if what == "M_cap" else (sum(CAP_M) + 7, max(CAP_M) - 1)
    for call in _cap_calls(len(p), lens, M_cap, elem_cap):
        for res in _capacity_call(call, p, lens, 0.05, device):
            _reported(res, sc.ST_OUT_OVERFLOW, 3)


def test_capacities_cloud_above_elem_points_is_reported(device, cap_stack):
    p, lens, want_p, want_l = cap_stack
    for ep, ok in ((max(lens), True), (max(lens) - 1, False)):
        call = _cap_calls(len(p), lens, sum(CAP_M) + 7, max(CAP_M), ep)[1]
        for res in _capacity_call(call, p, lens, 0.05, device):
            if ok:
                _equal_oracle(res, want_p, want_l)
            else:
                _reported(res, sc.ST_OUT_OVERFLOW, 3)


# ---- empty element, negative cell --------------------------------------------------------------------------------------------------
def _flag_calls(n, pc):
    calls = [sc.Call("sort", max(n + 37, 5200), 5200, 0, 0), sc.Call("small", n + 37, n + 7, 0, pc), sc.Call("inplace", n + 37, n + 7, 0, 0)]
    assert [c.form() for c in calls] == ["sort", ("small", 256, 8, 1109), "sort"]
    return calls


def test_empty_element_is_flagged_by_every_form(device):
    """lens = [n, 0, m]: the synchronous call raises, every capacity-mode form sets D3F_ST_EMPTY_ELEMENT and nothing else.  The header
    does not say what rows come with the flag (the reference is undefined for an empty cloud): nothing is asserted about them."""
    from d3feat_amd import _lib, ops
    a, b = sc.lattice(9300, 60, 0.05), sc.lattice(9301, 25, 0.05, (3, 0, -2))
    p, lens = np.concatenate([a, b]), [len(a), 0, len(b)]
    with pytest.raises(_lib.D3FeatLibraryError, match="empty"):
        ops.batch_grid_subsample(_t(p, device), lens, 0.05)
    for call in _flag_calls(len(p), max(lens)):
        for rows, sub_l, st in _capacity_call(call, p, lens, 0.05, device):
            assert st[1] == sc.ST_EMPTY_ELEMENT, (call, st)


def test_negative_cell_is_flagged_by_every_form(device):
    """dl = 0.03f and a smallest coordinate of 0.029999997f: origin = floor(min * (1 / dl)) * dl = 0.03f lies ABOVE the point, its
    cell is -1 (the reference casts that to size_t: undefined).  The synchronous call raises, every capacity-mode form sets
    D3F_ST_NEG_CELL and nothing else; the rows are not specified by the header and not looked at."""
    from d3feat_amd import _lib, ops
    p = sc.neg_cell_cloud()
    org, _ = sc.grid_dims(p, 0.03)
    assert org[0] > p[:, 0].min()
    with pytest.raises(_lib.D3FeatLibraryError, match="negative voxel index"):
        ops.batch_grid_subsample(_t(p, device), [len(p)], 0.03)
    for call in _flag_calls(len(p), len(p)):
        for rows, sub_l, st in _capacity_call(call, p, [len(p)], 0.03, device):
            assert st[1] == sc.ST_NEG_CELL, (call, st)


# ---- features and classes --------------------------------------------------------------------------------------------------------
FC_M = [1110, 2358, 60]
LABELS = np.asarray([-2147483647, -5, 0, 3, 2147483646, 2147483647], np.int32)


@pytest.fixture(scope="module")
def fc_stack():
    p, lens = sc.stack([sc.lattice(9400 + i, M, 0.05, sc.SHIFTS[i]) for i, M in enumerate(FC_M)])
    rng = np.random.default_rng(9410)
    f = (rng.standard_normal((len(p), 4)) * np.asarray([1.0, 100.0, 1e-3, 1e4])).astype(np.float32)
    c = LABELS[rng.integers(0, len(LABELS), (len(p), 3))]
    return p, lens, f, c


@pytest.mark.parametrize("fdim,ldim", [(1, 1), (4, 1), (1, 3), (4, 3), (4, 0), (0, 3)])
def test_features_and_classes(device, coracle, fc_stack, fdim, ldim):
    """B = 3 (M = 1110, 2358, 60: the grid-wide rounds place features and labels) against the single-cloud oracle per element,
    concatenated: the batch operation is the single-cloud operation per element.  Labels include negatives and INT_MAX."""
    from d3feat_amd import ops
    p, lens, f, c = fc_stack
    f, c = (f[:, :fdim] if fdim else None), (np.ascontiguousarray(c[:, :ldim]) if ldim else None)
    offs = np.concatenate([[0], np.cumsum(lens)])
    want = []
    for b in range(3):
        s = slice(offs[b], offs[b + 1])
        r = coracle.grid_subsampling(p[s], 0.05, f[s] if fdim else None, c[s] if ldim else None)
        want.append(r if isinstance(r, tuple) else (r,))
    assert [len(w[0]) for w in want] == FC_M
    want = [np.concatenate([w[i] for w in want]) for i in range(len(want[0]))]
    gp, gl, gf, gc = ops.batch_grid_subsample(_t(p, device), lens, 0.05, _t(f, device) if fdim else None, _t(c, device) if ldim else None)
    assert np.array_equal(gl.cpu().numpy(), FC_M)
    assert np.array_equal(bits(gp.cpu().numpy()), bits(want[0]))
    if fdim:
        assert gf.shape == want[1].shape and np.array_equal(bits(gf.cpu().numpy()), bits(want[1]))
    if ldim:
        assert gc.shape == want[-1].shape and np.array_equal(gc.cpu().numpy(), want[-1])
        assert want[-1].min() < 0 and want[-1].max() == 2147483647
