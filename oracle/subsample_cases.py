"""TEST INFRASTRUCTURE ONLY.  Seeded synthetic inputs for the grid-subsampling branch tests (tests/test_gpu_subsample_branches.py on
the GPU, tests/test_subsample_cases.py on the CPU) and a host mirror of the arithmetic by which csrc/grid_subsample.hip chooses
what runs: the entry form (gs_run / gs_run_small), the width and pass count of the radix sort (gs_prep) and the number of
iteration-order rounds (the libstdc++ bucket-count chain).  numpy only: no subsampling of its own -- voxel_keys restates the key of
a point only to say WHERE in the sorted sequence a voxel's run lies, never what the result is.

Builders
  lattice     M distinct cells of a G^3 lattice (G^3 >= 4 M), per[v] points in each at (cell + 0.5 + U(-0.3, 0.3) + shift) * dl,
              shuffled; exactly M occupied voxels, every point at least 0.2 cell from a wall.  crowd = c: voxel 0 holds c points whose
              in-cell offsets span 2^-12 .. 1 (of the cell whose corner is the coordinate origin when the shift puts one into the
              lattice: then the MAGNITUDES span 2^12 and the order of the fp32 sum shows in the bits).  total = n: extra points
              go to existing voxels (at most 3 per voxel unless that cannot reach n) so that len == n with M unchanged.
  box         two corner points that fix the grid dimensions exactly (dl = 1.0, half-integer coordinates: exact in fp32)
  box_cloud   box + M - 2 distinct inner cells with 1..3 points each
  run_cloud   a lattice cloud whose crowded voxel's run starts at a stated position modulo 256 of the sorted sequence
Every case of the GPU file is a `Case` in CASES: the builder, dl, the intended voxel count per cloud and, per call, the intended
form; tests/test_subsample_cases.py checks each against the oracle and against this mirror on a machine without a GPU."""
import numpy as np

CHAIN = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933, 351061, 712697, 1447153, 2938679, 5967347,
         12117689, 24607243, 49969847, 101473717, 206062531, 418451333, 849749479, 1725587117, 3504151727]   # csrc/common.h
SMALL_LAST = 6            # rounds 0..6 (<= 1109 buckets) run in gs_order_small_kernel, later ones grid-wide
NB_MAX = 5087             # GSS_NB_MAX (csrc/gs_small.h)
SMALL_POINTS = 16384
RS_TILE, RS_WAVE_ITEMS = 8192, 1024   # csrc/radix_sort.h
MAX_BATCH = 255
SENTINEL = np.float32(-7.25e9)        # pre-filled output rows
FAR = np.float32(1e30)                # capacity rows beyond the real points
ST_EMPTY_ELEMENT, ST_NEG_CELL, ST_KEY_RANGE, ST_OUT_OVERFLOW, ST_KEY_WIDTH = 1, 2, 4, 16, 32     # include/d3feat_amd.h


# ---- host mirror of the dispatcher -------------------------------------------------------------------------------------------
def chain_ge(n):
    for c in CHAIN:
        if c >= n:
            return c
    return CHAIN[-1]


def form(N_cap, M_cap, elem_cap=0, elem_points=0, in_place=False):
    """What gs_run launches.  M_cap None: the synchronous call -> "hash".  Capacity mode: ("small", T, R, nbmax) when the caller's
    capacities fit one workgroup per cloud (stacked input only), else "sort"."""
    if M_cap is None:
        return "hash"
    if not in_place:
        pc = elem_points if 0 < elem_points < N_cap else N_cap
        ec = elem_cap if 0 < elem_cap < M_cap else M_cap
        ec = min(ec, pc)
        if pc <= SMALL_POINTS and ec <= NB_MAX:
            e = M_cap if (elem_cap <= 0 or elem_cap > M_cap) else elem_cap        # gs_run_small
            e = min(e, pc)
            nbmax = min(max(chain_ge(e), 1109), NB_MAX)
            for lim, T, R in ((2048, 256, 8), (4096, 512, 8), (8192, 1024, 8), (12288, 1024, 12), (16384, 1024, 16)):
                if pc <= lim:
                    return ("small", T, R, nbmax)
    return "sort"


def rounds(M):
    """(rounds in one workgroup, grid-wide rounds) of the iteration order of M voxels in the hash / sort forms"""
    n = next(j for j, c in enumerate(CHAIN) if M <= c) + 1
    return min(n, SMALL_LAST + 1), max(n - SMALL_LAST - 1, 0)


def _f32(x):
    return np.asarray(x, np.float32)


def grid_dims(p, dl):
    """origin f32[3] and cells per axis of one cloud, in the fp32 steps of the reference (grid_subsampling.cpp:24-30)"""
    dl = np.float32(dl)
    inv = np.float32(1.0) / dl
    org = np.floor(p.min(0) * inv) * dl
    dims = np.maximum(np.floor((p.max(0) - org) / dl), 0).astype(np.uint64) + np.uint64(1)
    return org.astype(np.float32), [int(d) for d in dims]


def voxel_keys(p, dl):
    """key ix + NX iy + NX NY iz of every point of ONE cloud (uint64: the keys of this file stay below 2^63)"""
    org, (NX, NY, NZ) = grid_dims(p, dl)
    c = np.floor((p - org) / np.float32(dl))
    assert (c >= 0).all()
    c = c.astype(np.uint64)
    return c[:, 0] + np.uint64(NX) * c[:, 1] + np.uint64(NX * NY) * c[:, 2]


def sort_bits(p, lens, dl):
    """(kb, eb, passes) of gs_prep for the stack; passes is None when kb + eb > 32 (D3F_ST_KEY_WIDTH)"""
    offs = np.concatenate([[0], np.cumsum(lens)])
    cells = 1
    for b in range(len(lens)):
        if lens[b] > 0:
            d = grid_dims(p[offs[b]:offs[b + 1]], dl)[1]
            cells = max(cells, d[0] * d[1] * d[2])
    kb = max(int(cells - 1).bit_length(), 1)
    eb = int(len(lens) - 1).bit_length()
    return kb, eb, ((kb + eb + 7) // 8 if kb + eb <= 32 else None)


def sorted_run(p, lens, dl, b, point):
    """(start, length) of the run of `point`'s voxel (a row of cloud b) in the sort form's sequence: stable by (cloud, key)"""
    offs = np.concatenate([[0], np.cumsum(lens)])
    before = int(offs[b])                    # every point of an earlier cloud sorts first
    k = voxel_keys(p[offs[b]:offs[b + 1]], dl)
    kk = k[point]
    return before + int((k < kk).sum()), int((k == kk).sum())


# ---- builders ----------------------------------------------------------------------------------------------------------------
def _per(rng, M, per, total, crowd):
    """points per voxel: per is a count, an inclusive (lo, hi) tuple or an array of M counts"""
    given = isinstance(per, np.ndarray)
    if given:
        assert len(per) == M
        cnt = per.astype(np.int64).copy()
    elif isinstance(per, tuple):
        cnt = rng.integers(per[0], per[1] + 1, M)
    else:
        cnt = np.full(M, int(per), np.int64)
    if crowd:
        cnt[0] = crowd
    if total is not None:
        if not given:
            cnt[:] = 1                       # exact point count: one point each, the rest dealt out below
            if crowd:
                cnt[0] = crowd
        need = total - int(cnt.sum())
        assert need >= 0, (total, int(cnt.sum()))
        free = np.arange(1 if (crowd and M > 1) else 0, M)
        room = np.maximum(3 - cnt[free], 0)
        if room.sum() >= need:               # keep 1..3 per voxel
            slots = np.repeat(free, room)
            pick = rng.choice(len(slots), need, replace=False)
            np.add.at(cnt, slots[pick], 1)
        else:
            np.add.at(cnt, free[rng.integers(0, len(free), need)], 1)
    return cnt


def lattice_full(seed, M, dl, shift_cells=(0, 0, 0), per=(1, 3), crowd=0, total=None, flat=False):
    """-> (points f32[n, 3], voxel index of every point (into the M chosen cells), the cells i64[M, 3] incl. the shift)"""
    rng = np.random.default_rng(seed)
    if flat:
        G = max(int(np.ceil(np.sqrt(4 * M))), 2)
        flatc = rng.choice(G * G, M, replace=False)
        cells = np.stack([flatc % G, flatc // G, np.zeros(M, np.int64)], 1)
    else:
        G = 2
        while G ** 3 < 4 * M:
            G += 1
        flatc = rng.choice(G ** 3, M, replace=False)
        cells = np.stack([flatc % G, (flatc // G) % G, flatc // (G * G)], 1)
    cells = cells.astype(np.int64) + np.asarray(shift_cells, np.int64)
    at_origin = False
    if crowd:
        zero = np.nonzero((cells == 0).all(1))[0]
        inside = all(-G < s <= 0 for s in (shift_cells[:2] if flat else shift_cells))
        if inside and (not flat or shift_cells[2] == 0):
            if len(zero):
                cells[[0, zero[0]]] = cells[[zero[0], 0]]
            else:
                cells[0] = 0
            at_origin = True
    cnt = _per(rng, M, per, total, crowd)
    vid = np.repeat(np.arange(M), cnt)
    frac = 0.5 + rng.uniform(-0.3, 0.3, (len(vid), 3))
    if crowd:
        # in-cell offsets 0.9 * 2^-u, u in [0, 12]: with the cell at the origin the coordinates themselves span 2^12
        u = rng.uniform(0.0, 12.0, (crowd, 3))
        u[0], u[1 % crowd] = 0.0, 12.0
        frac[:crowd] = 0.9 * 2.0 ** -u if at_origin else 0.2 + 0.6 * 2.0 ** -u
    pts = ((cells[vid] + frac) * float(dl)).astype(np.float32)
    order = rng.permutation(len(vid))
    return pts[order], vid[order], cells


def lattice(seed, M, dl, shift_cells=(0, 0, 0), per=(1, 3), crowd=0, total=None, flat=False):
    return lattice_full(seed, M, dl, shift_cells, per, crowd, total, flat)[0]


def box(NX, NY, NZ, dl=1.0):
    return (np.asarray([[0.5, 0.5, 0.5], [NX - 0.5, NY - 0.5, NZ - 0.5]], np.float64) * dl).astype(np.float32)


def box_cloud(seed, NX, NY, NZ, M, dl=1.0, zmin=0, jitter=0.25):
    """box(NX, NY, NZ) + M - 2 distinct cells (not the corners, z >= zmin) with 1..3 points each at cell + 0.5 +- jitter"""
    rng = np.random.default_rng(seed)
    seen, cells = {(0, 0, 0), (NX - 1, NY - 1, NZ - 1)}, []
    while len(cells) < M - 2:
        c = (int(rng.integers(0, NX)), int(rng.integers(0, NY)), int(rng.integers(zmin, NZ)))
        if c not in seen:
            seen.add(c)
            cells.append(c)
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    vid = np.repeat(np.arange(len(cells)), rng.integers(1, 4, len(cells)))
    steps = rng.integers(-1, 2, (len(vid), 3)) * jitter          # -jitter, 0, +jitter: exact in fp32 next to 2^19
    inner = ((cells[vid] + 0.5 + steps) * dl).astype(np.float32)
    p = np.concatenate([box(NX, NY, NZ, dl), inner])
    return p[rng.permutation(len(p))]


def run_cloud(seed, c, start_mod, M=600, dl=0.05):
    """lattice cloud (cell (0,0,0) in the middle of the lattice) whose crowded voxel of c points starts at sorted position
    start_mod modulo 256: points are added to the voxel with the smallest key until it does"""
    G = 2
    while G ** 3 < 4 * M:
        G += 1
    shift = (-(G // 2),) * 3
    rng = np.random.default_rng(seed + 7919)
    per = rng.integers(1, 4, M)
    per[0] = c
    p, vid, _ = lattice_full(seed, M, dl, shift, per=per, crowd=c)
    k = voxel_keys(p, dl)
    first = int(np.nonzero(vid == 0)[0][0])
    start = int((k < k[first]).sum())
    assert start > 0, "the crowded voxel must not have the smallest key"
    low = int(vid[np.argmin(k)])
    per[low] += (start_mod - start) % 256
    p, vid, _ = lattice_full(seed, M, dl, shift, per=per, crowd=c)
    return p, int(np.nonzero(vid == 0)[0][0])


def neg_cell_cloud():
    """dl = 0.03f, smallest coordinate 0.029999997f: origin = floor(min * (1 / dl)) * dl = 0.03f > min -> cell -1"""
    lo = np.nextafter(np.float32(0.03), np.float32(0))
    p = lattice(901, 40, 0.03, (2, 2, 2))
    return np.concatenate([p[:20], _f32([[lo, 0.1, 0.1]]), p[20:]]).astype(np.float32)


def on_grid_cloud(dl, n=9):
    """points exactly on fl(k * dl), k = 0..n-1 per axis (n^3 points): floor((p - origin) / dl) decides by the last bit"""
    k = np.arange(n, dtype=np.float32) * np.float32(dl)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(902).permutation(len(g))].astype(np.float32)


def stack(clouds):
    return np.concatenate(clouds).astype(np.float32), [len(c) for c in clouds]


def with_tail(p, extra):
    return np.concatenate([p, np.full((extra, 3), FAR, np.float32)])


# ---- the cases -----------------------------------------------------------------------------------------------------------------
class Call:
    """one call of a case: kind in hash / sort / small / inplace, the capacities it passes and the form it must take"""

    def __init__(self, kind, N_cap=None, M_cap=None, elem_cap=0, elem_points=0, want=None):
        self.kind, self.N_cap, self.M_cap, self.elem_cap, self.elem_points, self.want = kind, N_cap, M_cap, elem_cap, elem_points, want

    def form(self):
        return form(self.N_cap, self.M_cap, self.elem_cap, self.elem_points, self.kind == "inplace")

    def __repr__(self):
        return "%s(N_cap=%s M_cap=%s elem_cap=%d elem_points=%d)" % (self.kind, self.N_cap, self.M_cap, self.elem_cap, self.elem_points)


class Case:
    def __init__(self, name, build, dl, M, kinds, small_cap=NB_MAX, bits=None, grow_points=False):
        self.name, self._build, self.dl, self.M, self.kinds, self.small_cap = name, build, dl, list(M), kinds, small_cap
        self.grow_points = grow_points      # one-workgroup call: state a point capacity of at least small_cap (elem_cap is cut to it)
        self.bits = bits          # intended kb + eb of the sort form (None: not stated)
        self._data = None

    def data(self):
        if self._data is None:
            p, lens = self._build()
            self._data = (np.ascontiguousarray(p, np.float32), [int(x) for x in lens])
        return self._data

    def rounds(self):
        """intended (rounds in one workgroup, grid-wide rounds) of the largest cloud in the hash / sort forms"""
        return rounds(max(self.M))

    def calls(self):
        p, lens = self.data()
        n, m = len(p), sum(self.M)
        out = []
        for kind in self.kinds:
            if kind == "hash":
                out.append(Call("hash", want="hash"))
            elif kind == "sort":      # capacities above 5087: the one-workgroup form is out
                out.append(Call("sort", max(n + 37, 5200), max(m + 7, 5200), 0, 0, want="sort"))
            elif kind == "small":
                pc = max(max(lens), self.small_cap) if self.grow_points else max(lens)
                nb = min(max(chain_ge(min(self.small_cap, pc)), 1109), NB_MAX)
                T, R = next((T, R) for lim, T, R in ((2048, 256, 8), (4096, 512, 8), (8192, 1024, 8), (12288, 1024, 12), (16384, 1024, 16))
                            if pc <= lim)
                out.append(Call("small", max(n, pc) + 37, max(m + 7, self.small_cap) if self.grow_points else m + 7, self.small_cap, pc, want=("small", T, R, nb)))
            elif kind == "inplace":   # always the sort form; the order rounds are launched for the largest cloud exactly
                out.append(Call("inplace", n + 37, m + 7, max(self.M), 0, want="sort"))
        return out


ALL4 = ("hash", "sort", "small", "inplace")
# kb of the lattice clouds of the order-round cases (bits of G^3 - 1 where the M cells reach every face of the lattice)
ROUND_KB = {1: 1, 12: 6, 13: 6, 14: 6, 29: 7, 30: 7, 59: 9, 60: 9, 127: 9, 128: 9, 257: 11, 258: 11, 541: 12, 542: 12, 1109: 13, 1110: 13,
            2357: 14, 2358: 14, 5087: 15, 5088: 15, 10273: 16, 10274: 16}
ROUND_M = [1, 12, 13, 14, 29, 30, 59, 60, 127, 128, 257, 258, 541, 542, 1109, 1110, 2357, 2358, 5087, 5088, 10273, 10274]
# voxel capacity of the one-workgroup call per M: nbmax 1109 / 2357 / 5087 in turn, and M == elem_cap exactly (14, 128, 542, 1110, 2358)
# as well as M == elem_cap == nbmax (1109, 2357, 5087)
SMALL_CAP = {1: 1109, 12: 2357, 13: 5087, 14: 14, 29: 2357, 30: 5087, 59: 1109, 60: 2357, 127: 5087, 128: 128, 257: 2357, 258: 5087,
             541: 1109, 542: 542, 1109: 1109, 1110: 1110, 2357: 2357, 2358: 2358, 5087: 5087}
SMALL_NB = {1: 1109, 12: 2357, 13: 5087, 14: 1109, 29: 2357, 30: 5087, 59: 1109, 60: 2357, 127: 5087, 128: 1109, 257: 2357, 258: 5087,
            541: 1109, 542: 1109, 1109: 1109, 1110: 2357, 2357: 2357, 2358: 5087, 5087: 5087}
WG_LEN = {2048: (1900, 256, 8), 2049: (1950, 512, 8), 4096: (3000, 512, 8), 4097: (3100, 1024, 8), 8192: (4000, 1024, 8),
          8193: (4100, 1024, 12), 12288: (4500, 1024, 12), 12289: (4600, 1024, 16), 16384: (5000, 1024, 16)}   # len: (M, T, R)
#            kb + eb: (clouds as (NX, NY, NZ, M))
PASS_BOXES = {8: [(8, 8, 4, 100)], 9: [(8, 8, 4, 100), (4, 4, 3, 20)], 16: [(64, 32, 32, 300)], 17: [(64, 32, 32, 300), (9, 9, 9, 50)],
              24: [(256, 256, 256, 300)], 25: [(256, 256, 256, 300), (100, 100, 100, 200)], 32: [(2048, 2048, 1024, 300)]}
RUNS = [(2, 255), (255, 1), (256, 0), (256, 130), (257, 0), (700, 50), (700, 255)]      # (points in the voxel, start modulo 256)
DLS = (0.03, 0.05, 0.1)
SHIFTS = ((0, 0, 0), (-37, 12, -5), (400, -400, 90))
MIXED_M = [5, 1110, 60, 2358, 1]


def many_lens():
    return [1 + (b * 17) % 40 for b in range(MAX_BATCH)]


def _round_cloud(M):
    # 1..3 points per voxel; from 5088 voxels on the point count is held at 16000 (the largest input of the file is 16385)
    i = ROUND_M.index(M)
    tot = None if M <= 5087 else min(2 * M, 16000)
    return stack([lattice(1000 + M, M, DLS[i % 3], SHIFTS[i % 3], total=tot)])


def _wg_stack(L):
    return stack([lattice(2000 + L, WG_LEN[L][0], 0.05, total=L), lattice(2001, 1, 0.05, per=1)])


def _wg_16385():
    p, _ = _wg_stack(16384)
    a = p[:16384]
    extra = (a[-1] + np.float32(0.002)).astype(np.float32)           # one more point in the last point's voxel
    return stack([np.concatenate([a, extra[None]]), p[16384:]])


def _pass_stack(bits):
    return stack([box_cloud(3000 + bits + i, NX, NY, NZ, M) for i, (NX, NY, NZ, M) in enumerate(PASS_BOXES[bits])])


def _tile_stack(n):
    # wave 1 of tile 0 covers sorted-input rows 1024..2047: cloud 0 ends at 1300, cloud 1 at 1500 -> pieces of three clouds
    return stack([lattice(4000 + n, 400, 0.05, total=1300), lattice(4001, 90, 0.05, (3, 3, 3), total=200),
                  lattice(4002 + n, 2000, 0.05, (-9, 0, 4), total=n - 1500)])


def _mixed():
    return stack([lattice(5000 + i, M, 0.05, SHIFTS[i % 3]) for i, M in enumerate(MIXED_M)])


def _many():
    return stack([lattice(6000 + b, (l + 1) // 2, 0.1, ((b % 5) - 2, 0, b % 3), total=l) for b, l in enumerate(many_lens())])


def _cases():
    cs = []
    for M in ROUND_M:
        kinds = ("hash", "sort", "small") if M <= NB_MAX else ("hash", "sort")
        cs.append(Case("rounds-%d" % M, (lambda M=M: _round_cloud(M)), DLS[ROUND_M.index(M) % 3], [M], kinds, SMALL_CAP.get(M, NB_MAX), bits=ROUND_KB[M], grow_points=True))
    cs.append(Case("mixed", _mixed, 0.05, MIXED_M, ALL4, small_cap=2358, bits=14 + 3))
    cs.append(Case("many-255", _many, 0.1, [(l + 1) // 2 for l in many_lens()], ALL4, small_cap=20, bits=7 + 8))
    for L, (M, T, R) in WG_LEN.items():
        cs.append(Case("wg-%d" % L, (lambda L=L: _wg_stack(L)), 0.05, [M, 1], ("small",)))
    cs.append(Case("wg-16385", _wg_16385, 0.05, [5000, 1], ("sort",), bits=15 + 1))
    for bits in PASS_BOXES:
        cs.append(Case("passes-%d" % bits, (lambda bits=bits: _pass_stack(bits)), 1.0, [b[3] for b in PASS_BOXES[bits]],
                       ALL4 if bits == 32 else ("hash", "sort", "inplace"), small_cap=1109, bits=bits))
    for n in (8191, 8192, 8193, 16385):
        cs.append(Case("tile-%d" % n, (lambda n=n: _tile_stack(n)), 0.05, [400, 90, 2000], ("sort", "inplace"), bits=13 + 2))
    for c, sm in RUNS:
        cs.append(Case("run-%d-at-%d" % (c, sm), (lambda c=c, sm=sm: stack([run_cloud(7000 + c + sm, c, sm)[0]])), 0.05, [600],
                       ALL4, small_cap=1109, bits=12))
    for i, (dl, shift) in enumerate(((0.03, (-37, 12, -5)), (0.011, (400, -400, 90)), (0.3, (-37, 12, -5)), (0.3, (400, -400, 90)),
                                     (0.011, (0, 0, 0)))):
        cs.append(Case("shift-%d" % i, (lambda i=i, dl=dl, shift=shift: stack([lattice(8000 + i, 300, dl, shift, crowd=40),
                                                                                  lattice(8100 + i, 77, dl, shift[::-1])])), dl, [300, 77], ALL4,
                       small_cap=541, bits=11 + 1))
    cs.append(Case("flat", lambda: stack([lattice(8200, 500, 0.03, (5, -3, 0), flat=True)]), 0.03, [500], ALL4, small_cap=1109, bits=11))
    cs.append(Case("identical", lambda: stack([np.repeat(_f32([[0.37, -1.21, 2.5]]), 50, 0), np.repeat(_f32([[0.0, 0.0, 0.0]]), 3, 0)]),
                   0.03, [1, 1], ALL4, small_cap=7, bits=1 + 1))
    for dl, M in ((0.03, None), (0.011, None), (0.3, None)):
        cs.append(Case("on-grid-%g" % dl, (lambda dl=dl: stack([on_grid_cloud(dl)])), dl, [ON_GRID_M[dl]], ALL4, small_cap=1109, bits=10))
    return cs


# voxels of on_grid_cloud(dl): 729 points on fl(k dl).  fl(fl(k dl) / dl) may fall below k, which moves a point one cell down; a
# whole plane moves with it, so the count stays 9^3 unless two planes merge -- these figures are the C oracle's (oracle/d3f_oracle.c),
# checked by tests/test_subsample_cases.py
ON_GRID_M = {0.03: 729, 0.011: 729, 0.3: 729}

CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = {c.name: c for c in _cases()}
    return CASES


# ---- 64-bit keys (hash form only) ------------------------------------------------------------------------------------------------
def key64_cloud(M, NZ, zmin):
    """dl = 1.0, 2^19 x 2^19 x NZ cells, M voxels: the two corners and M - 2 cells with z >= zmin"""
    return box_cloud(9000 + M, 1 << 19, 1 << 19, NZ, M, 1.0, zmin=zmin)


KEY64 = {10: (1 << 16, 1 << 15, 53), 40: (1 << 18, 1 << 17, 55)}      # M: (NZ, zmin, log2 of the smallest inner key)
