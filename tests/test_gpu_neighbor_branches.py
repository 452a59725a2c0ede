"""Every kernel instantiation and every row-ordering branch of the neighbour search -- csrc/radius_neighbors.hip, nb_cell_search.h,
nb_nearest.h, 13 instantiations behind nb_search_dispatch -- against the brute-force oracle COracle.batch_neighbors(grid=False): the
pinned fp32 metric (dx*dx + dy*dy) + dz*dz, strict d2 < r2, rows ascending by (d2, index).  The results are integers: every
comparison is np.array_equal with the oracle's rows, the pad value or the sentinel; nothing compares a kernel with a kernel, nothing
has a tolerance.  (The 100 000- and 40 000-query cases use the oracle's grid form; tests/test_neighbor_cases.py shows grid=True ==
grid=False on the small clouds of this file.)  Matrices in the INTERNAL numbering are renumbered back through grid.order /
query_grid.order (oracle/neighbor_cases.renumber_back) and compared with the oracle as well.

Inputs: oracle/neighbor_cases.py ("<cloud>-<queries>" scenes, the oracle's rows computed once per process).  Every `out` is
pre-filled with 0x3fffffff and has ld = width + 3: columns [width, ld) must keep the sentinel; capacity-mode cases give supports and
queries NaN rows beyond sum(lens), pass pad_value = PAD_NUM_SUPPORTS (must come out as the real support count) and require the rows
of `out` from the real query count on to keep the sentinel.  status[0] == the oracle's largest count whenever want_kmax is asked
without a hint, 0 with want_kmax=False; ST_HIT_OVERFLOW is set exactly when the oracle has a row with n > cap as the dispatcher
rounds it (to 2: cell kernel, to 4: lane-group kernel); rows with n > cap are not compared.  Every test asserts from the ORACLE's
result that the rows its branch needs exist (hit-count bands, rows with and without a truncated-key clash, stencils above and below
NBC_CHUNK) before it looks at the GPU's.  The dispatcher is steered with D3F_NB_CELL / D3F_NB_NEAREST / D3F_NBC_Q (read per call).

Instantiation -> test (13; profiles/neighbor_branch_tests_kernel_stats.csv is the kernel trace of this file: all 13 are launched)
-----------------------------------------------------------------------------------------------------------
  nb_search_kernel<false, 32, false>                 test_lane_group_32[*], test_many_elements[*], test_default_dispatch[39999]
  nb_search_kernel<false, 64, false>                 test_lane_group_64[*]   (cap = 260, 1024 > 256)
  nb_search_kernel<false, 16, false>                 test_lane_group_16[100000]   ([99999]: 32 lanes, the same oracle rows)
  nb_search_kernel<true, 32, false> / <true, 32, true>     test_first_only_lane_group[*], test_many_elements[*]  (no hint / hint)
  nb_search_kernel<true, 64, false> / <true, 64, true>     test_lane_group_64[*]
  nb_search_kernel<true, 16, false> / <true, 16, true>     test_lane_group_16[100000]
  nb_cell_search_kernel<true, false> / <true, true>  test_cell_kernel[*], test_many_elements[*], test_default_dispatch[40000]
  nb_nearest_kernel<false> / <true>                  test_nearest_kernel[*], test_many_elements[*], test_default_dispatch[40000]

Row-ordering branch -> test
---------------------------
  nb_bitonic64 (32 lanes, n <= 64 <= cap)            test_lane_group_32[slab-* / graded-* / lattice-*], caps 192, 64, 256
  nb_bitonic64x16 (16 lanes)                         test_lane_group_16[100000], cap 192, rows with n <= 64
  lane-group rank counting                           32 lanes: test_lane_group_32[graded-*], rows n > 64, and every row at cap 40;
                                                     16 lanes: test_lane_group_16[100000] rows n > 64 and cap 40; 64 lanes: every row
  nbc_group_sort64 (8 lanes, 26-bit keys)            test_cell_kernel[graded2497*-Q], rows n <= 64 without a clash
  the cell kernel's redo path after a clash          test_cell_kernel[graded2497-Q] (rows with a clash), [lattice797*-Q] (every row)
  nbc_bitonic128 (64 < n <= 128, n <= cap, width < 64)     test_cell_kernel[graded2497*-Q], widths 38 and 63, rows without a clash
  its clash fallback -> dense exact form             the same tests, rows with a clash; [lattice797*-Q]: every 81-hit row
  the cell kernel's dense exact form                 test_cell_kernel[*], widths 64 and 96; n > 128; cap 100 (101..128: overflow)
  the INTERNAL forms (ties through a gather)         test_cell_kernel[lattice797*-Q] with internal=True (redo path and dense form)
  register-resident / streamed candidate list        test_cell_kernel[graded2497-Q], [graded2497x3-Q]: stencils <= 384 and > 384
  B > NB_EL_LDS = 40 (unstaged geometry)             test_many_elements[41*], [255*] in all three kernels; [40*]: the staged side

Where include/d3feat_amd.h is silent nothing is asserted: status[0] of a first_only search with a hint and want_kmax is printed
only (by the kernel's code it is the hit count of the scan that stood -- the restricted one where it found a support within the
hint -- not the oracle's largest count).

No defect found: on an MI355X all 113 cases pass on the parent's kernels.  Recorded there, not asserted: status[0] under a hint is
the oracle's largest count at the hints 0.05 r, 0.7 r and 0.99 r on most scenes and smaller at 0.3 r (59 of 63 on slab, 205 of 222
on graded, 207 of 225 on the 100 000 queries).
Cost, measured on an MI355X: the 113 cases take 5.0 s run alone (pytest's figure; the slowest, the two 100 000-query cases, 0.5 s
and 0.4 s).  One complete `pytest -m gpu tests` run with this file took 307.8 s (589 passed, 5 skipped); the two slowest cases of
this file cost 0.42 s and 0.41 s in it and no other reaches the 0.37 s of that run's 40th-slowest test.  Every other test and every
kernel is the parent's, so the parent's suite is that run less this file: about 303 s, to which the file adds under 2 %.
"""
import numpy as np
import pytest
import torch

from oracle import neighbor_cases as nc

pytestmark = pytest.mark.gpu

SENT = nc.SENTINEL
OVERFLOW = 8                        # D3F_ST_HIT_OVERFLOW (include/d3feat_amd.h)
EXTRA_S, EXTRA_Q = 37, 29           # capacity rows beyond the real counts (NaN)
_DEV = {}


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    for k in ("D3F_NB_CELL", "D3F_NB_NEAREST", "D3F_NBC_Q"):
        monkeypatch.delenv(k, raising=False)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _with_nan_rows(a, extra):
    return np.concatenate([a, np.full((extra, 3), np.nan, np.float32)])


class _Dev:
    """a scene on the device: tensors, the supports' grid, the queries' grid (the supports' when the queries are the supports)"""

    def __init__(self, sc, dev, capacity):
        from d3feat_amd import ops
        self.sc, self.capacity = sc, capacity
        self.ns, self.nq = len(sc.s), len(sc.q)
        self.S = _t(_with_nan_rows(sc.s, EXTRA_S) if capacity else sc.s, dev)
        self.sl, self.ql = ops.as_lens(sc.sl.tolist(), dev), ops.as_lens(sc.ql.tolist(), dev)
        self.grid = ops.NeighborGrid(self.S, self.sl, float(sc.r))
        if sc.same:
            self.Q, self.qgrid = self.S, self.grid
        else:
            self.Q = _t(_with_nan_rows(sc.q, EXTRA_Q) if capacity else sc.q, dev)
            self.qgrid = ops.NeighborGrid(self.Q, self.ql, float(sc.r))
        self.s_order = self.grid.order.cpu().numpy()[: self.ns].astype(np.int64)
        self.q_order = self.qgrid.order.cpu().numpy()[: self.nq].astype(np.int64)


def _dev(coracle, device, name, capacity=False):
    key = (name, capacity)
    if key not in _DEV:
        _DEV[key] = _Dev(nc.scene(coracle, name), device, capacity)
    return _DEV[key]


def _search(dv, width, cap=192, mode="plain", first_only=False, hint=0.0, want_kmax=True, pad=None):
    """one search into a sentinel-filled out of ld = width + 3 -> (matrix in the reference numbering, [kmax, flags], the pad value
    the rows must hold).  mode: plain (d3f_neighbor_grid_search), ordered (query_grid), internal (query_grid + INTERNAL)."""
    from d3feat_amd import _lib
    ld = width + 3
    out = torch.full((dv.Q.shape[0], ld), SENT, dtype=torch.int32, device=dv.Q.device)
    status = torch.full((2,), 77, dtype=torch.int32, device=dv.Q.device)
    if dv.capacity:
        pad_arg, pad = _lib.PAD_NUM_SUPPORTS, dv.ns
    else:
        pad_arg = pad = dv.ns if pad is None else pad
    kw = {} if mode == "plain" else dict(query_grid=dv.qgrid, internal=(mode == "internal"))
    res, st = dv.grid.search(dv.Q, dv.ql, width, ld=ld, pad_value=pad_arg, cap=cap, first_only=first_only, out=out, status=status,
                             want_kmax=want_kmax, nn_hint=float(hint), **kw)
    assert res.data_ptr() == out.data_ptr() and st.data_ptr() == status.data_ptr()
    got = out.cpu().numpy()
    st = status.tolist()
    if mode == "internal":
        got = nc.renumber_back(got, dv.q_order, dv.s_order, dv.ns, dv.nq)
    return got, st, pad


def _untouched(got, dv, width, tag):
    assert (got[:, width:] == SENT).all(), (tag, "columns [width, ld) written")
    assert (got[dv.nq:] == SENT).all(), (tag, "rows beyond the real query count written")


def _check_full(dv, width, cap, cap_round, tag, mode="plain", want_kmax=True, pad=None):
    sc = dv.sc
    got, st, pad = _search(dv, width, cap=cap, mode=mode, want_kmax=want_kmax, pad=pad)
    tag = (sc.name, "capacity" if dv.capacity else "exact", mode, "width", width, "cap", cap) + tuple(tag)
    _untouched(got, dv, width, tag)
    capr = (cap + cap_round - 1) // cap_round * cap_round
    ok = sc.n <= capr
    exp = nc.expected(sc.want, dv.ns, width, pad)
    bad = (got[: dv.nq, :width] != exp).any(1) & ok
    assert not bad.any(), tag + ("rows wrong:", int(bad.sum()), "first", int(np.argmax(bad)), "its n", int(sc.n[np.argmax(bad)]),
                                 "n of wrong rows", np.unique(sc.n[bad])[:8].tolist())
    assert bool(st[1] & OVERFLOW) == bool((~ok).any()), tag + ("flags", st[1], "rows above cap", int((~ok).sum()))
    assert st[0] == (int(sc.n.max()) if want_kmax else 0), tag + ("status[0]", st[0], "kmax", int(sc.n.max()))


def _check_first(dv, width, tag, mode="plain", hint=0.0, want_kmax=False, cap=192, pad=None):
    sc = dv.sc
    got, st, pad = _search(dv, width, cap=cap, mode=mode, first_only=True, hint=hint, want_kmax=want_kmax, pad=pad)
    tag = (sc.name, "capacity" if dv.capacity else "exact", mode, "first_only width", width, "hint", float(hint)) + tuple(tag)
    _untouched(got, dv, width, tag)
    if width > 0:
        col0 = np.where(sc.n > 0, sc.first, pad)
        bad = got[: dv.nq, 0] != col0
        assert not bad.any(), tag + ("rows wrong:", int(bad.sum()), "first", int(np.argmax(bad)))
        assert (got[: dv.nq, 1:width] == pad).all(), tag + ("columns 1 .. width - 1 are not the pad value",)
    assert not (st[1] & OVERFLOW), tag + ("flags", st[1])
    if not want_kmax:
        assert st[0] == 0, tag + ("status[0]", st[0])
    elif not (0.0 < hint < float(sc.r)):
        assert st[0] == int(sc.n.max()), tag + ("status[0]", st[0], "kmax", int(sc.n.max()))
    else:
        print(tag, "status[0] under a hint (recorded, the header is silent):", st[0], "oracle kmax", int(sc.n.max()))


def _hints(r):
    r = float(r)
    return (0.0, 0.05 * r, 0.3 * r, 0.7 * r, 0.99 * r, 1.5 * r)          # >= r: ignored by the entry point


# ---- 1. lane-group kernel, 32 lanes per query ----------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [False, True], ids=["exact", "capacity"])
@pytest.mark.parametrize("mode", ["plain", "ordered", "internal"])
@pytest.mark.parametrize("name", ["slab-self", "slab-other", "graded-self", "graded-other", "lattice-self", "lattice-other"])
def test_lane_group_32(device, coracle, monkeypatch, name, mode, capacity):
    """nb_search_kernel<false, 32, false>.  Dispatcher: D3F_NB_CELL=0 keeps queries = supports off the cell kernel;
    `lpq = cap > 256 ? 64 : (Nq >= 100000 ? 16 : 32)` with cap <= 256 and Nq <= 3000.  In the kernel: `LPQ == 32 && n <= 64 &&
    cap >= 64` -> nb_bitonic64, else rank counting over min(n, cap) hits (n > 64, or every row at cap = 40); `n > cap` -> overflow.
    plain with queries = supports: the `same` test of NeighborGrid.search fires (qorder = the grid's own records)."""
    monkeypatch.setenv("D3F_NB_CELL", "0")
    dv = _dev(coracle, device, name, capacity)
    n = dv.sc.n
    kmax = int(n.max())
    assert kmax <= 256 and (n <= 40).sum() > 0 and ((n > 40) & (n <= 64)).sum() > 0, nc.band_counts(n)
    if name.startswith("graded"):
        assert all(b > 0 for b in nc.band_counts(n)), nc.band_counts(n)        # n <= 64, 65..128, 129..192, > 192
    if name == "lattice-self":
        assert (n == 81).sum() > 0 and (n <= 64).sum() > 0
    if name.startswith("lattice"):
        assert (n > 64).sum() > 0
    for width in (0, 1, 38, 64, 96, kmax + 5):
        _check_full(dv, width, 192, 4, (), mode)
    for cap in (40, 64, 256):          # 40: cap < 64 -> rank counting, rows with n <= 40 exact, overflow flagged
        for width in (38, 96):
            _check_full(dv, width, cap, 4, (), mode)
    _check_full(dv, 38, 192, 4, ("want_kmax=False",), mode, want_kmax=False)
    if not capacity:
        _check_full(dv, 38, 192, 4, ("pad -1",), mode, pad=-1)


@pytest.mark.parametrize("mode", ["plain", "ordered", "internal"])
@pytest.mark.parametrize("name", ["slab-far", "graded-far", "slabdup-other"])
def test_first_only_lane_group(device, coracle, monkeypatch, name, mode):
    """nb_search_kernel<true, 32, HINT>.  Dispatcher: first_only with want_kmax -> never the nearest kernel; with
    want_kmax=False and D3F_NB_NEAREST=0 neither; `FO_ && nn_hint > 0.f` -> HINT = true (a hint >= radius is zeroed by the entry
    point).  Queries outside the support box (beyond the +-2 cell clamp too), 40 duplicated supports: the lowest index wins."""
    monkeypatch.setenv("D3F_NB_NEAREST", "0")
    dv = _dev(coracle, device, name)
    assert (dv.sc.n == 0).sum() > 0 or name == "slabdup-other"
    if name == "slabdup-other":
        assert (dv.sc.first[:40] == 100).all() and (dv.sc.n[:40] >= 40).all()
    for hint in _hints(dv.sc.r):
        _check_first(dv, 4, (), mode, hint, want_kmax=False)
        _check_first(dv, 1, (), mode, hint, want_kmax=True)
    _check_first(dv, 0, (), mode)
    _check_first(dv, 3, ("pad -1",), mode, pad=-1)


# ---- 2. 64 lanes per query -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["graded-self", "graded-other"])
def test_lane_group_64(device, coracle, monkeypatch, name):
    """nb_search_kernel<false, 64, false>, <true, 64, false>, <true, 64, true>.  Dispatcher: `cap > 256` after rounding to 4 -> 64
    lanes (cap = 260: the boundary, no graded row has more than 256 hits; cap = 1024); first_only with want_kmax=True (the nearest
    kernel needs want_kmax=False).  64 lanes have no ordering network: every row is rank counted."""
    monkeypatch.setenv("D3F_NB_CELL", "0")
    dv = _dev(coracle, device, name)
    n = dv.sc.n
    assert all(b > 0 for b in nc.band_counts(n)) and n.max() <= 256, nc.band_counts(n)
    for cap in (260, 1024):
        for mode in ("plain", "internal"):
            for width in (38, 96):
                _check_full(dv, width, cap, 4, (), mode)
            for hint in (0.0, 0.3 * float(dv.sc.r)):
                _check_first(dv, 2, ("cap", cap), mode, hint, want_kmax=True, cap=cap)
    _check_full(dv, int(n.max()) + 5, 1024, 4, ())


# ---- 3. 16 lanes per query -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [100000, 99999])
def test_lane_group_16(device, coracle, monkeypatch, nq):
    """nb_search_kernel<false, 16, false>, <true, 16, false>, <true, 16, true> at Nq = 100000; 99999 runs the same rows on 32 lanes:
    `Nq >= 100000 ? 16 : 32` is the only trigger.  In the kernel: `LPQ == 16 && n <= 64 && cap >= 64` -> nb_bitonic64x16, else rank
    counting (rows above 64 hits; every row at cap 40).  Oracle: grid form (equal to brute force, tests/test_neighbor_cases.py)."""
    monkeypatch.setenv("D3F_NB_NEAREST", "0")
    dv = _dev(coracle, device, "graded-bigq" + ("" if nq == 100000 else str(nq)))
    n = dv.sc.n
    assert dv.Q.shape[0] == nq and all(b > 0 for b in nc.band_counts(n)) and (n == 0).sum() > 0 and (n <= 40).sum() > 0
    for cap in (192, 40):
        for width in (38, 96):
            _check_full(dv, width, cap, 4, ())
    for mode in ("ordered", "internal"):
        _check_full(dv, 38, 192, 4, (), mode)
    r = float(dv.sc.r)
    for hint in (0.0, 0.3 * r, 0.99 * r):
        _check_first(dv, 2, (), "plain", hint, want_kmax=False)
    _check_first(dv, 1, (), "internal", 0.3 * r, want_kmax=True)


# ---- 4. cell kernel ------------------------------------------------------------------------------------------------------------

def _cell_preconditions(sc, name):
    n = sc.n
    assert (n <= 64).sum() > 0 and ((n >= 65) & (n <= 128)).sum() > 0, nc.band_counts(n)
    bits = sc.bits()
    c64 = nc.clash64(bits, n)
    mid = (n >= 65) & (n <= 128)
    if name.startswith("graded"):
        assert nc.cells_not_doubled(sc.s, sc.sl, sc.r)
        T = nc.stencil_candidates(sc.s, sc.sl, sc.r)
        assert (T > nc.NBC_CHUNK).sum() > 0 and (T <= nc.NBC_CHUNK).sum() > 0        # streamed and register-resident stencils
        assert 0 < c64.sum() < (n <= 64).sum()                                       # redo path and 8-lane network
        for width in (38, 63):
            c128 = nc.clash128(bits, n, width)
            assert 0 < c128.sum() < mid.sum(), (width, int(c128.sum()))              # 128-key network and its fallback
    else:
        assert c64[n <= 64].all() and nc.clash128(bits, n, 38)[mid].all()            # lattice: every row has bit-equal d2
    if name == "graded2497":
        assert (n > 128).sum() > 0 and ((n > 100) & (n <= 128)).sum() > 0 and (n > 192).sum() > 0 and n.max() <= 1024
    if name == "lattice797":
        assert (n == 81).sum() > 0


@pytest.mark.parametrize("Q", [1, 3, 8, 9, 16, 32])
@pytest.mark.parametrize("name", ["graded2497", "graded2497x3", "lattice797", "lattice797x3"])
def test_cell_kernel(device, coracle, monkeypatch, name, Q):
    """nb_cell_search_kernel<true, false> and <true, true> (internal).  Dispatcher: `!first_only && queries_are_supports` and
    D3F_NB_CELL=2; Q = D3F_NBC_Q queries per wavefront -- the dispatcher clamps a forced value to 16 like its own (`Q > 16 ? 16 : Q`,
    before NBC_QMAX = 32), so [32] launches the layout of [16]: it is kept because it pins that clamp (a dispatcher that let 32
    through would run an untested layout here); 2497 and 797 are multiples of neither Q nor 4 Q, so the
    last wavefront and the last workgroup are partial, the last batch of eight is short (Q = 9: one query), and in the x3 scenes
    a wavefront's queries straddle two clouds.  In the kernel: n <= 64 -> nbc_group_sort64 on 26-bit keys, a clash -> the redo
    path; `n <= 128 && n <= cap && width < 64` -> nbc_bitonic128 on 25-bit keys (widths 38, 63; not 64, 96; not 101..128 at cap
    100, which overflow), a clash among the first width + 1 keys or anything else -> exact rank counting over min(n, cap) hits;
    `T <= NBC_CHUNK` keeps the stencil in registers, larger ones are streamed per query."""
    monkeypatch.setenv("D3F_NB_CELL", "2")
    monkeypatch.setenv("D3F_NBC_Q", str(Q))
    dv = _dev(coracle, device, name + "-self")
    _cell_preconditions(dv.sc, name)
    for mode in ("ordered", "internal"):
        for width, cap in ((38, 192), (96, 192), (63, 192), (64, 192), (38, 100), (96, 100), (38, 1024), (96, 1024)):
            _check_full(dv, width, cap, 2, ("Q", Q), mode)
    for width in (38, 96):             # the plain entry point: NeighborGrid.search's `same` test fires
        _check_full(dv, width, 192, 2, ("Q", Q), "plain")
    _check_full(dv, 38, 192, 2, ("Q", Q, "want_kmax=False"), "ordered", want_kmax=False)
    _check_full(dv, int(dv.sc.n.max()) + 5, 1024, 2, ("Q", Q), "internal")
    _check_full(dv, 0, 192, 2, ("Q", Q), "ordered")


@pytest.mark.parametrize("Q", [9, 16])
@pytest.mark.parametrize("name", ["graded2497x3", "lattice797"])
def test_cell_kernel_capacity_mode(device, coracle, monkeypatch, name, Q):
    """The same kernel with Ns = Nq = capacities: 37 NaN rows beyond sum(lens), pad = D3F_PAD_NUM_SUPPORTS."""
    monkeypatch.setenv("D3F_NB_CELL", "2")
    monkeypatch.setenv("D3F_NBC_Q", str(Q))
    dv = _dev(coracle, device, name + "-self", True)
    _cell_preconditions(dv.sc, name)
    for mode in ("plain", "ordered", "internal"):
        for width, cap in ((38, 192), (96, 192), (38, 100)):
            _check_full(dv, width, cap, 2, ("Q", Q), mode)


@pytest.mark.parametrize("nq", [40000, 39999])
def test_default_dispatch(device, coracle, nq):
    """No switch set: the thresholds themselves.  Full rows, queries = supports: `Nq >= 40000 || Nq < 6000` -> the cell kernel with
    Q = min(Nq / 2048, 16) = 16 at 40000, the lane-group kernel at 39999; first_only without Kmax: `Nq >= 40000` -> the nearest
    kernel at 40000, the lane-group kernel at 39999.  The slab tiled to 40000 points in three clouds; oracle: grid form."""
    dv = _dev(coracle, device, "tiled%d-self" % nq)
    assert (dv.sc.n <= 64).sum() > 0 and len(dv.sc.sl) == 3
    for mode in ("plain", "ordered", "internal"):
        for width in (38, 96):
            _check_full(dv, width, 192, 2 if nq >= 40000 else 4, (), mode)
    do = _dev(coracle, device, "tiled%d-other" % nq)
    assert (do.sc.n == 0).sum() > 0
    for mode in ("plain", "ordered", "internal"):
        for hint in (0.0, 0.3 * float(do.sc.r)):
            _check_first(do, 2, (), mode, hint, want_kmax=False)


# ---- 5. nearest kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [False, True], ids=["exact", "capacity"])
@pytest.mark.parametrize("mode", ["plain", "ordered", "internal"])
@pytest.mark.parametrize("name", ["slab-far", "graded-far", "slabdup-other", "many255e-other"])
def test_nearest_kernel(device, coracle, monkeypatch, name, mode, capacity):
    """nb_nearest_kernel<false> / <true>.  Dispatcher: `first_only && !want_kmax` and D3F_NB_NEAREST=2; `nn_hint > 0.f` -> <true>
    (restricted walk, accepted when the nearest support lies within 0.998 hint^2, else the full stencil: most queries at the
    small hints); a hint >= radius is zeroed by the entry point.  Column 0 = the oracle's column 0 or pad, the others pad."""
    monkeypatch.setenv("D3F_NB_NEAREST", "2")
    dv = _dev(coracle, device, name, capacity)
    sc = dv.sc
    assert (sc.n == 0).sum() > 0 or name == "slabdup-other"
    if name.endswith("far"):
        mn, inv_h, dims = nc.cell_geometry(sc.s, sc.r)
        c = nc.cell_of(nc.far_queries(sc.s), mn, inv_h)
        assert ((c < -2) | (c > dims + 1)).any() and (((c == -1) | (c == dims)).any(1) & (sc.n[sc.sl[0]: sc.ql[0]] > 0)).any()
        # (queries beyond the +-2 cell clamp, and queries one cell outside the grid that still have a support within the radius)
    if name == "slabdup-other":
        assert (sc.first[:40] == 100).all()                                             # 40 bit-equal candidates: lowest index
    bits = nc.d2_bits(sc.q, sc.s, sc.want[:, :1]) if sc.want.shape[1] else None
    for hint in _hints(sc.r):
        if bits is not None and 0 < hint < float(sc.r):
            h2 = np.float32(0.998) * np.float32(hint) * np.float32(hint)
            d2 = bits[:, 0].view(np.float32)[sc.n > 0]
            if hint == _hints(sc.r)[2]:       # 0.3 r: the restricted walk is accepted for some queries and repeated for others
                assert (d2 <= h2).sum() > 0 and (d2 > h2).sum() > 0
        _check_first(dv, 4, (), mode, hint)
    _check_first(dv, 1, (), mode, 0.3 * float(sc.r))
    _check_first(dv, 0, (), mode)
    if not capacity:
        _check_first(dv, 3, ("pad -1",), mode, pad=-1)


# ---- 6. many elements ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ends", [False, True], ids=["", "ends-empty"])
@pytest.mark.parametrize("B", [40, 41, 255])
def test_many_elements(device, coracle, monkeypatch, B, ends):
    """`B <= NB_EL_LDS` (= 40) stages the elements' geometry in LDS, 41 and 255 (= D3F_MAX_BATCH) read it from memory -- in all
    three kernels.  Empty clouds in the middle (and at both ends), elements with queries and no supports and the reverse."""
    tag = "many%d%s" % (B, "e" if ends else "")
    ds, do = _dev(coracle, device, tag + "-self"), _dev(coracle, device, tag + "-other")
    sl, ql = do.sc.sl, do.sc.ql
    assert (sl[1:-1] == 0).any() and ((sl == 0) & (ql > 0)).any() and ((sl > 0) & (ql == 0)).any()
    assert (not ends) or (sl[0] == 0 and sl[-1] == 0)
    assert (do.sc.n == 0).sum() > 0 and (do.sc.n > 0).sum() > 0 and ds.sc.n.max() > 1
    # the grid's own invariants
    for dv in (ds, do):
        for g, pts in ((dv.grid, dv.S), (dv.qgrid, dv.Q)):
            order, inv = g.order.cpu().numpy().astype(np.int64), g.inv.cpu().numpy().astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(g.Ns)), "order is not a permutation"
            assert np.array_equal(inv[order], np.arange(g.Ns))
            assert np.array_equal(g.xyz.cpu().numpy().view(np.uint32), pts.cpu().numpy()[order].view(np.uint32))
    width = int(max(ds.sc.n.max(), do.sc.n.max())) + 2
    for q_forced in ("", "16", "5"):
        monkeypatch.setenv("D3F_NB_CELL", "2")
        monkeypatch.setenv("D3F_NBC_Q", q_forced) if q_forced else monkeypatch.delenv("D3F_NBC_Q", raising=False)
        for mode in ("plain", "ordered", "internal"):
            _check_full(ds, width, 192, 2, ("cell kernel, Q", q_forced), mode)
    monkeypatch.delenv("D3F_NBC_Q", raising=False)
    monkeypatch.setenv("D3F_NB_CELL", "0")
    for dv in (ds, do):
        for mode in ("plain", "ordered", "internal"):
            _check_full(dv, width, 192, 4, ("lane-group kernel",), mode)
            _check_full(dv, 3, 40, 4, ("lane-group kernel",), mode)
    for nearest in ("0", "2"):
        monkeypatch.setenv("D3F_NB_NEAREST", nearest)
        for mode in ("plain", "ordered", "internal"):
            for hint in (0.0, 0.3 * float(do.sc.r)):
                _check_first(do, 2, ("D3F_NB_NEAREST", nearest), mode, hint)


# ---- 7. empty calls ------------------------------------------------------------------------------------------------------------

def test_empty_calls_leave_out_alone(device, coracle):
    """`if (Nq == 0) return D3F_OK` behind the status reset; Ns = 0 with no real query (capacity mode: q_lens = [0]) launches
    kernels that find no query to work on.  `out` keeps the sentinel in both."""
    from d3feat_amd import ops
    sc = nc.scene(coracle, "slab-self")
    S = _t(sc.s, device)
    grid = ops.NeighborGrid(S, [len(sc.s)], float(sc.r))
    for first_only in (False, True):
        out = torch.full((5, 8), SENT, dtype=torch.int32, device=device)
        status = torch.full((2,), 77, dtype=torch.int32, device=device)
        grid.search(torch.empty((0, 3), dtype=torch.float32, device=device), [0], 6, ld=8, out=out, status=status, first_only=first_only)
        assert (out.cpu().numpy() == SENT).all() and status.tolist() == [0, 0]
        empty = ops.NeighborGrid(torch.empty((0, 3), dtype=torch.float32, device=device), [0], float(sc.r))
        Q = _t(np.full((5, 3), np.nan, np.float32), device)
        for want_kmax in (True, False):
            status.fill_(77)
            empty.search(Q, [0], 6, ld=8, out=out, status=status, first_only=first_only, want_kmax=want_kmax, pad_value=7)
            assert (out.cpu().numpy() == SENT).all() and status.tolist() == [0, 0]


# ---- 8. edges through the public ops -------------------------------------------------------------------------------------------

def test_exact_radius_is_excluded_one_ulp_inside_is_included(device, coracle, monkeypatch):
    """d2 == r2 bit for bit (r = 0.125, axis offsets) is no neighbour -- strict `d2 < r2` -- in all three kernels."""
    from d3feat_amd import ops, tf_custom_ops as tfo
    q, s, r, excluded, included = nc.boundary()
    bits = nc.d2_bits(q[:1], s, np.concatenate([excluded, [included]])[None])
    r2 = np.float32(r * r).view(np.uint32)
    assert (bits[0, :6] == r2).all() and bits[0, 6] < r2
    ql, sl = np.asarray([len(q)], np.int32), np.asarray([len(s)], np.int32)
    want = coracle.batch_neighbors(q, s, ql, sl, r, grid=False)
    row = want[0][want[0] != len(s)]
    assert included in row and not np.isin(excluded, row).any()
    got = tfo.batch_ordered_neighbors(_t(q, device), _t(s, device), _t(ql, device), _t(sl, device), r).cpu().numpy()
    assert np.array_equal(got, want)                                   # lane-group kernel
    both = np.concatenate([q[:1], s])                                  # the query among the supports: the cell kernel
    bl = np.asarray([len(both)], np.int32)
    want_b = coracle.batch_neighbors(both, both, bl, bl, r, grid=False)
    assert not np.isin(excluded + 1, want_b[0]).any() and included + 1 in want_b[0]
    B = _t(both, device)
    assert np.array_equal(tfo.batch_ordered_neighbors(B, B, _t(bl, device), _t(bl, device), r).cpu().numpy(), want_b)
    monkeypatch.setenv("D3F_NB_NEAREST", "2")
    grid = ops.NeighborGrid(_t(s, device), sl.tolist(), float(r))
    for hint in (0.0, 0.5 * float(r), 0.99 * float(r)):
        near, _ = grid.search(_t(q, device), ql.tolist(), 1, first_only=True, want_kmax=False, nn_hint=hint)
        assert np.array_equal(near.cpu().numpy()[:, 0], np.where(nc.counts(want, len(s)) > 0, want[:, 0], len(s)))


def test_public_ops_on_the_graded_cloud(device, coracle):
    """tfo.batch_ordered_neighbors starts at width 96 / cap 192: graded has rows above 192 hits, so the first search reports
    ST_HIT_OVERFLOW and the op searches again at cap = 1024; the result equals the oracle -- with the supports as queries (cell
    kernel: 2500 < 6000) and with other queries (lane-group kernel; cap 1024 -> 64 lanes).  tfo.ordered_neighbors pads with -1."""
    from d3feat_amd import tf_custom_ops as tfo
    for name in ("graded-self", "graded-other"):
        sc = nc.scene(coracle, name)
        assert (sc.n > 192).sum() > 0
        S = _t(sc.s, device)
        Q = S if sc.same else _t(sc.q, device)
        got = tfo.batch_ordered_neighbors(Q, S, _t(sc.ql, device), _t(sc.sl, device), sc.r).cpu().numpy()
        assert got.shape == sc.want.shape and np.array_equal(got, sc.want)
        got = tfo.ordered_neighbors(Q, S, sc.r).cpu().numpy()
        assert np.array_equal(got, np.where(sc.want == len(sc.s), -1, sc.want))


def test_more_duplicates_than_the_cap_is_reported(device, coracle):
    """1100 copies of one point: n = 1100 > D3F_NEIGHBOR_CAP = 1024 in every one of their rows -- ST_HIT_OVERFLOW at the largest
    cap raises D3FeatLibraryError (a status flag, not a GPU fault: the device still answers afterwards).  40 copies: fine."""
    from d3feat_amd import _lib, tf_custom_ops as tfo
    p = nc.duplicates(1100)
    P = _t(p, device)
    lens = _t(np.asarray([len(p)], np.int32), device)
    with pytest.raises(_lib.D3FeatLibraryError):
        tfo.batch_ordered_neighbors(P, P, lens, lens, nc.R)
    with pytest.raises(_lib.D3FeatLibraryError):
        tfo.batch_ordered_neighbors(_t(p, device), P, lens, lens, nc.R)
    torch.cuda.synchronize()
    few = nc.duplicates(40)
    F = _t(few, device)
    fl = _t(np.asarray([len(few)], np.int32), device)
    want = coracle.batch_neighbors(few, few, [len(few)], [len(few)], nc.R, grid=False)
    assert np.array_equal(want[50:, :40], np.tile(np.arange(50, 90), (40, 1)))     # lowest index first, in every copy's row
    assert np.array_equal(tfo.batch_ordered_neighbors(F, F, fl, fl, nc.R).cpu().numpy(), want)
