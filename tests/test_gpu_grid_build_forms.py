"""Neighbour grids built from boxes that the kernels writing the clouds gathered (d3f_neighbor_grid_build_boxed, d3f_geometry_reset,
the *_boxed producers; csrc/radius_neighbors.hip, prims.h d3f_box_accum).

Everything here is an integer or a bit pattern: every comparison is exact, against what the parent's path computes from the same
inputs -- bbox_kernel's boxes (read out of a grid built by d3f_neighbor_grid_build), that grid's geometry, cells and search rows,
the subsampling without boxes, the engine with D3F_GRID_BOXED off.

  boxes        every producing kernel (gs_stack_pair_kernel, which copies its input's; gs_emit_kernel; gs_small_kernel, whose
               barycentres gs_small_pack_kernel only moves) at B = 1 and B = 3 with an empty
               cloud in the middle, a cloud of one point, negative coordinates and a -0.0 that is an extreme of its axis; capacity
               mode, rows past the real count NaN.
  grids        el, ncells word for word and the cell prefix the searches read (d3f_scan_at: cell_start[c] + base[c / 1024]) for every
               c in [0, ncells] wherever the small form's LDS budget is not the binding one.  The large form's cell_start array itself
               is word-equal to the parent's (same scan kernel); the small form stores the complete prefix in cell_start and zero tile
               bases (no workgroup knows the counts of another cloud's cells without waiting for it), so for it the comparison is the
               prefix, which is all any search reads.  Per cell the SET of supports; inv[order[p]] == p; a radius search and a nearest
               search give identical rows.
  shapes       Ns = 0, one point per cloud, ceil(Ns / B) = T and T + 1, a cloud whose cells exceed the LDS budget (el differs, rows do
               not), a large-form cloud whose count ends inside a 256-thread group, B = D3F_MAX_BATCH in both forms, non-finite
               coordinates (one cell).  The form is asserted from the dispatcher's rule: small iff ceil(Ns / B) <= T.
  subsampler   the sort form with finished boxes against the sort form that boxes its input itself: points, lengths, status.
  end to end   FragmentEngine with D3F_GRID_BOXED on against off: the record block bit for bit, F = 1 and F = 2.

Cost on an MI355X: the 25 cases take 3.2 s run alone (the slowest, an engine pair, 0.34 s).
"""
import numpy as np
import pytest
import torch

from conftest import small_cloud
from oracle import subsample_cases as sc

pytestmark = pytest.mark.gpu

T_SMALL = 4096           # D3F_NB_SMALL_T default (csrc/radius_neighbors.hip)
LDS_CELLS = 8192         # NBX_LDS_CELLS
SENT = 0x3fffffff
NEG_ZERO_ORD = 0x7fffffff          # d3f_f2ord(-0.0f): the sign bit set -> all bits flipped


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _align(x):
    return (x + 255) // 256 * 256


def _layout(Ns, B):
    """byte offsets inside a grid object (nb_carve)"""
    budget = min(max(4 * max(Ns, 1), 1 << 16), 1 << 28)
    cells, ns = budget + 8, max(Ns, 1)
    off, o = {}, 0
    for name, nbytes in (("soffs", (B + 1) * 4), ("bbox", B * 24), ("el", B * 48), ("ncells", 64), ("cell_cnt", cells * 8),
                         ("cell_start", cells * 4), ("cell_of", ns * 4), ("sorted", ns * 16), ("order", ns * 4),
                         ("stmp", ((cells + 1023) // 1024 + 64) * 4)):
        off[name] = o
        o += _align(nbytes)
    return off, cells


class _Grid:
    """host copies of what the searches read of a built grid"""

    def __init__(self, g):
        from d3feat_amd import _lib
        off, cells = _layout(g.Ns, g.B)
        assert off["order"] == _lib.load().d3f_neighbor_grid_order_offset(g.Ns, g.B)      # the layout above is the library's
        mem = g.mem.cpu().numpy()

        def words(name, n, dt=np.int32):
            return mem[off[name]: off[name] + 4 * n].view(dt).copy()
        self.soffs = words("soffs", g.B + 1)
        self.bbox = words("bbox", 6 * g.B, np.uint32).reshape(g.B, 6)
        self.el = mem[off["el"]: off["el"] + 48 * g.B].copy().reshape(g.B, 48)      # NbElem: mn[3], inv_h (f64), dims[3], cbase (i32)
        self.dims = self.el[:, 32:48].view(np.int32).reshape(g.B, 4)[:, :3]
        self.ncells = words("ncells", 2)
        nc = int(self.ncells[0])
        assert 0 < nc < cells
        local, base = words("cell_start", nc + 1), words("stmp", nc // 1024 + 1)
        self.cell_start = local
        self.prefix = local.astype(np.int64) + base[np.arange(nc + 1) // 1024]
        n = int(self.soffs[g.B])
        self.n = min(n, g.Ns)
        self.order = g.order.cpu().numpy()[: self.n].astype(np.int64)
        self.inv = g.inv.cpu().numpy()[: self.n].astype(np.int64)
        self.xyz = g.xyz.cpu().numpy()[: self.n]

    def cell_sets(self):
        return [frozenset(self.order[a:b].tolist()) for a, b in zip(self.prefix[:-1], self.prefix[1:])]


def _plain_and_boxed(S, lens, r, dev):
    """the same supports through d3f_neighbor_grid_build and, with ITS boxes, through d3f_neighbor_grid_build_boxed"""
    from d3feat_amd import ops
    St, lt = _t(S, dev), ops.as_lens(list(lens), dev)
    plain = ops.NeighborGrid(St, lt, r)
    P = _Grid(plain)
    chain = ops.GridChain([St.shape[0]], len(lens), dev)
    chain.reset()
    chain.box(0).copy_(_t(P.bbox.view(np.int32), dev))
    boxed = ops.NeighborGrid(St, lt, r, chain=chain, level=0)
    return St, lt, plain, P, boxed, _Grid(boxed), chain


def _rows(g, St, lt, width, first_only):
    out = torch.full((St.shape[0], width + 2), SENT, dtype=torch.int32, device=St.device)
    status = torch.zeros((2,), dtype=torch.int32, device=St.device)
    g.search(St, lt, width, ld=width + 2, first_only=first_only, out=out, status=status, reset_status=False)
    return out.cpu().numpy(), status.cpu().numpy()


def _check_pair(S, lens, r, dev, form, budget_binds=False, T=T_SMALL):
    from d3feat_amd import _lib
    Ns, B = len(S), len(lens)
    # the dispatcher's rule, from the capacities alone
    want = 1 if -(-Ns // B) <= T else 2
    assert want == form and _lib.load().d3f_neighbor_grid_boxed_form(Ns, B) == form
    St, lt, plain, P, boxed, X, chain = _plain_and_boxed(S, lens, r, dev)
    assert chain.forms == [form] and boxed.form == form
    assert np.array_equal(P.soffs, X.soffs) and P.n == X.n == min(sum(lens), Ns)
    if budget_binds:
        assert form == 1 and (P.dims.astype(np.int64).prod(1) > LDS_CELLS).any()        # the parent's grid does not fit the LDS counters
        assert (X.dims.astype(np.int64).prod(1) <= LDS_CELLS).all() and not np.array_equal(P.el, X.el)
    else:
        assert np.array_equal(P.el, X.el) and np.array_equal(P.ncells, X.ncells)
        assert np.array_equal(P.prefix, X.prefix)
        if form == 2:
            assert np.array_equal(P.cell_start, X.cell_start)
        assert P.cell_sets() == X.cell_sets()
    for G in (P, X):
        assert np.array_equal(G.inv[G.order], np.arange(G.n)) and np.array_equal(G.xyz.view(np.uint32), S[G.order].view(np.uint32))
    assert X.prefix[0] == 0 and X.prefix[-1] == X.n and (np.diff(X.prefix) >= 0).all()
    if Ns:
        for width, fo in ((40, False), (1, True)):
            a, sa = _rows(plain, St, lt, width, fo)
            b, sb = _rows(boxed, St, lt, width, fo)
            assert np.array_equal(a, b) and np.array_equal(sa, sb), (width, fo)
            assert (a[: P.n, 0] != SENT).all() and (a[P.n:] == SENT).all()
    return P, X


def _nan_tail(p, extra):
    return np.concatenate([p, np.full((extra, 3), np.nan, np.float32)]).astype(np.float32)


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------
def _box_clouds(B, n=700):
    """B = 1: one cloud; B = 3: [cloud, empty, one point].  x lies in [-2, -0.5] but for ONE point at x = -0.0 (the maximum of the axis,
    alone in its voxel at every cell size used here), y and z take both signs."""
    a = small_cloud(11, n, scale=(1.5, 3.0, 1.0))
    a[:, 0] -= np.float32(1.7)
    a[:, 1] -= np.float32(1.0)
    a[0] = (np.float32(-0.0), np.float32(0.25), np.float32(-0.125))
    assert a[1:, 0].max() < -0.4 and np.signbit(a[0, 0]) and (a[:, 1] < 0).any() and (a[:, 1] > 0).any()
    if B == 1:
        return [a]
    return [a, np.zeros((0, 3), np.float32), np.asarray([[-3.5, 2.0, -0.75]], np.float32)]


def _reference_boxes(pts, lens_t, dev):
    """bbox_kernel's boxes of a stack: what d3f_neighbor_grid_build leaves in its grid object"""
    from d3feat_amd import ops
    return _Grid(ops.NeighborGrid(pts, lens_t, 0.2)).bbox


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("producer", ["stack_pair", "emit", "small"])
def test_producer_boxes_equal_bbox_kernel(device, producer, B):
    from d3feat_amd import ops
    # (emit: more voxels than one 1024-thread workgroup writes, so that workgroups meet on a box)
    clouds = _box_clouds(B, 4500 if producer == "emit" else 700)
    p, lens = sc.stack(clouds)
    # (the sort form is taken from a point capacity AND a voxel capacity above 5087: the one-workgroup form is out)
    P = _t(_nan_tail(p, 5300 - len(p) if producer == "emit" else 41), device)
    lt = ops.as_lens(lens, device)
    if producer == "stack_pair":
        # gs_stack_pair_kernel hands the finished boxes of its input on, one per copy
        chain = ops.GridChain([2 * P.shape[0]], 2 * B, device)
        chain.reset()
        chain.pre[:B].copy_(_t(_reference_boxes(P, lt, device).view(np.int32), device))
        out, lens_out = ops.stack_self_pair(P, lt, bbox_in=chain.pre[:B], bbox_out=chain.box(0))
        assert lens_out.cpu().tolist() == [l for l in lens for _ in (0, 1)]
    else:
        # dl = 0.05: the -0.0 point is alone in its voxel, so its barycentre is the point itself
        m_cap = 5200 if producer == "emit" else 900
        form = sc.form(P.shape[0], m_cap, 0, 0)
        assert (form if isinstance(form, str) else form[0]) == ("sort" if producer == "emit" else "small")
        chain = ops.GridChain([m_cap], B, device)
        chain.reset()
        out, lens_out, st = ops.batch_grid_subsample_async(P, lt, 0.05, m_cap, bbox_out=chain.box(0))
        assert int(st[0]) > (2048 if producer == "emit" else 0) and int(st[1]) == (1 if B == 3 else 0)                     # (the empty cloud is flagged, nothing else)
        if B == 3:
            assert lens_out.cpu().tolist()[1:] == [0, 1]
    ref = _reference_boxes(out, lens_out, device)
    got = chain.box(0).cpu().numpy().view(np.uint32)
    assert ref[0, 3] == NEG_ZERO_ORD                            # the case is reached: the maximum of x is -0.0, not +0.0
    nb = got.shape[0]
    if B == 3:                                                  # the empty cloud keeps the initial values in both
        k = 2 if producer == "stack_pair" else 1
        assert (ref[k] == np.asarray([0xFFFFFFFF] * 3 + [0] * 3, np.uint32)).all()
    assert ref.shape == (nb, 6) and np.array_equal(ref, got)


# ---- grids and searches ------------------------------------------------------------------------------------------------------------------
def test_empty_capacity(device):
    _check_pair(np.zeros((0, 3), np.float32), [0], 0.1, device, form=1)


def test_one_point_per_cloud(device):
    S = _nan_tail(np.asarray([[0.1, -0.2, 0.3], [5.0, 5.0, -5.0], [-0.0, 0.0, 1.0]], np.float32), 5)
    _check_pair(S, [1, 1, 1], 0.2, device, form=1)


@pytest.mark.parametrize("Ns,form", [(T_SMALL, 1), (T_SMALL + 1, 2)])
def test_threshold_between_the_forms(device, Ns, form):
    """B = 1: the capacity of the cloud is Ns itself; 4097 = 16 * 256 + 1 rows of which 4090 are real -- the count kernel's last
    256-thread group and the scatter's last workgroup end inside their range"""
    S = _nan_tail(small_cloud(21, Ns - 7), 7)
    _check_pair(S, [Ns - 7], 0.11, device, form=form)


def test_large_form_three_clouds_with_a_ragged_tail(device):
    """large form, B = 3 with an empty cloud in the middle; 9000 + 2777 real rows = 46 * 256 + 1"""
    S = _nan_tail(np.concatenate([small_cloud(22, 9000), small_cloud(23, 2777) + np.float32(0.5)]), 3 * T_SMALL + 1 - 11777)
    assert (9000 + 2777) % 256 == 1
    _check_pair(S, [9000, 0, 2777], 0.1, device, form=2)


def test_cells_beyond_the_lds_budget_coarsen_the_edge(device):
    """a spread cloud under a small radius: 100 x 75 x 35 cells at the first edge; the parent's budget (65536) takes the second
    edge, the small form's (8192) the third -- other cells, the same rows"""
    S = _nan_tail(small_cloud(24, 3000), 9)
    P, X = _check_pair(S, [3000], 0.02, device, form=1, budget_binds=True)
    assert X.dims.prod() < P.dims.prod()


@pytest.mark.parametrize("form", [1, 2])
def test_max_batch(device, form, monkeypatch):
    """B = D3F_MAX_BATCH clouds of 1..40 points; the large form is reached by lowering T through the library's own switch"""
    lens = sc.many_lens()
    clouds = [small_cloud(300 + b, l, scale=(0.6, 0.6, 0.3)) + np.float32(0.01 * b) for b, l in enumerate(lens)]
    S = _nan_tail(np.concatenate(clouds), 13)
    T = T_SMALL
    if form == 2:
        T = 16
        monkeypatch.setenv("D3F_NB_SMALL_T", str(T))
    assert len(lens) == 255 and (-(-len(S) // len(lens)) <= T) == (form == 1)
    _check_pair(S, lens, 0.15, device, form=form, T=T)


@pytest.mark.parametrize("Ns", [600, T_SMALL + 300])
def test_non_finite_coordinates_take_the_one_cell_path(device, Ns):
    S = small_cloud(25, Ns - 5)
    S[17, 1] = np.inf
    S = _nan_tail(S, 5)
    P, X = _check_pair(S, [Ns - 5], 0.1, device, form=1 if Ns <= T_SMALL else 2)
    assert X.ncells[0] == 1 and (X.dims == 1).all()


# ---- subsampler --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "many-255", "tile-8193", "shift-0", "flat", "identical", "passes-9"])
def test_sort_form_with_finished_boxes(device, name):
    from d3feat_amd import ops
    case = sc.cases()[name]
    call = next(c for c in case.calls() if c.kind == "sort")
    assert call.form() == "sort"
    p, lens = case.data()
    P = _t(sc.with_tail(p, call.N_cap - len(p)), device)
    lt = ops.as_lens(lens, device)
    boxes = _t(_reference_boxes(P, lt, device).view(np.int32), device)

    def run(bbox_in):
        out, sub_l, st = ops.batch_grid_subsample_async(P, lt, case.dl, call.M_cap, elem_cap=call.elem_cap, elem_points=call.elem_points,
                                                        bbox_in=bbox_in)
        torch.cuda.synchronize()
        m = int(st[0])
        return out[:m].cpu().numpy().view(np.uint32), sub_l.cpu().numpy(), st.cpu().numpy()
    a, b = run(None), run(boxes)
    assert a[2][0] == sum(case.M) and a[1].tolist() == case.M
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2])
def test_engine_records_do_not_depend_on_the_switch(device, F, monkeypatch):
    from d3feat_amd import ops
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    from d3feat_amd.utils.synthetic import room_fragment
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    limits = np.asarray([37, 35, 36, 38, 38], np.int32)
    raws = [torch.from_numpy(room_fragment(41 + i, n_raw=30000 - 4000 * i, edge=1.0)).to(device) for i in range(F)]
    kw = dict(raw_cap=40000, n0_cap=12000, slots=1, device=device, batch=F)
    assert ops.GRID_BOXED
    on = FragmentEngine(cfg, W, limits, **kw)
    monkeypatch.setattr(ops, "GRID_BOXED", False)
    off = FragmentEngine(cfg, W, limits, **kw)
    chain = on.slots[0].chain
    assert chain is not None and all(chain.boxed) and off.slots[0].chain is None
    assert 2 in chain.forms and 1 in chain.forms               # both forms are part of the replay
    on.submit(0, raws if F > 1 else raws[0])
    off.submit(0, raws if F > 1 else raws[0])
    ra, rb = on.fetch(0, packed=True), off.fetch(0, packed=True)
    assert on.fallbacks == 0 and off.fallbacks == 0
    ra, rb = (ra, rb) if isinstance(ra, (list, tuple)) else ([ra], [rb])
    assert len(ra) == len(rb) == F
    for x, y in zip(ra, rb):
        assert x.shape == y.shape and x.shape[0] > 1000 and torch.equal(x, y)
