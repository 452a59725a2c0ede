"""TEST INFRASTRUCTURE ONLY.  Seeded synthetic inputs for the neighbour-search kernel tests (tests/test_gpu_neighbor_branches.py on
the GPU, tests/test_neighbor_cases.py on the CPU) and the numpy restatements of the conditions by which the kernels of
csrc/radius_neighbors.hip / nb_cell_search.h / nb_nearest.h choose the code that orders a row: numpy only, no search of its own.

Clouds (r = 0.075 unless a test says otherwise)
  slab      3000 uniform points in 1.0 x 1.0 x 0.1: all rows but a handful have n <= 64 hits
  graded    2500 points whose density grows towards x = 0: rows in every band n <= 64 / 65..128 / 129..192 / > 192, none above 256
  lattice   10 x 10 x 8 points, spacing 0.03: interior rows have n = 81, every row has bit-equal d2 (ties by index)
  many      255 clouds of 0 / 5..44 points in a 0.3 box (empty elements inside); prefixes for B = 40 / 41
  big_q     100 000 uniform queries in graded's box grown by 0.05: the only trigger of the 16-lane form
  boundary  supports at distance exactly r = 0.125 of a query (d2 == r2 bit for bit: excluded) and one an ulp inside
  duplicates  n copies of one point

Conditions
  d2_bits            the pinned fp32 metric (dx*dx + dy*dy) + dz*dz of every (query, listed support) pair, as uint32
  clash64 / clash128 do two keys of a row agree after the kernels' truncation (26 bits for lists of <= 64, 25 bits among the first
                     width + 1 keys for 65..128)
  stencil_candidates the candidates of a query's 27 cells under the grid's own geometry (cell edge h = r (1 + 2^-20), fp64 floor((x - min) * (1 / h))),
                     cells_not_doubled: that geometry is the one the build uses (the cell budget does not double the edge)"""
import numpy as np

R = np.float32(0.075)
SENTINEL = 0x3fffffff                 # pre-filled outputs
NBC_CHUNK = 384                       # candidates the cell kernel keeps in registers (csrc/nb_cell_search.h)
BANDS = ((0, 64), (65, 128), (129, 192), (193, 1 << 30))


def slab():
    rng = np.random.default_rng(101)
    return (rng.random((3000, 3)) * np.asarray([1.0, 1.0, 0.1])).astype(np.float32)


def graded(n=2500):
    rng = np.random.default_rng(102)
    g = rng.random((2500, 3))
    g[:, 0] **= 2
    g *= np.asarray([0.8, 0.25, 0.25])
    return g.astype(np.float32)[:n]


def lattice(n=800):
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    return (g * 0.03).astype(np.float32)[:n]


def jitter(p, seed):
    """the same points moved by N(0, 0.02): 'other queries' of the same size"""
    rng = np.random.default_rng(200 + seed)
    return (p + rng.normal(0.0, 0.02, p.shape)).astype(np.float32)


def split3(n):
    """three clouds of unequal, odd sizes"""
    a = (2 * n) // 5 + 1
    b = n // 3 + 2
    return np.asarray([a, b, n - a - b], np.int32)


def tiled_slab(n=40000):
    """the slab repeated on a 4 x 4 raster of unit tiles, the first n points, in three clouds"""
    s = slab()
    tiles = [s + np.asarray([i % 4, i // 4, 0], np.float32) for i in range((n + len(s) - 1) // len(s))]
    p = np.concatenate(tiles)[:n].astype(np.float32)
    return p, np.asarray([n * 3 // 8, n // 3, n - n * 3 // 8 - n // 3], np.int32)


def many_lens(B, ends_empty=False):
    lens = np.asarray([0 if b % 7 == 3 else 5 + (b * 13) % 40 for b in range(B)], np.int32)
    if ends_empty:
        lens[0] = lens[-1] = 0
    return lens


def many(B, ends_empty=False):
    """-> (supports, s_lens, queries, q_lens): B clouds in a 0.3 box; the queries of an element are its supports moved by
    N(0, 0.02), except: every element with b % 11 == 5 has supports but no queries, every EMPTY element with odd b has six
    queries and no supports."""
    rng = np.random.default_rng(103)
    full = many_lens(255)
    pts = [(rng.random((int(n), 3)) * 0.3).astype(np.float32) for n in full]      # the same clouds for every prefix
    extra = [(rng.random((6, 3)) * 0.3).astype(np.float32) for _ in full]
    moved = [(p + rng.normal(0.0, 0.02, p.shape)).astype(np.float32) for p in pts]
    sl = many_lens(B, ends_empty)
    s, q, ql = [], [], []
    for b in range(B):
        sb = pts[b][: sl[b]]
        s.append(sb)
        if b % 11 == 5 and sl[b] > 0:
            qb = moved[b][:0]
        elif sl[b] == 0 and b % 2 == 1:
            qb = extra[b]
        else:
            qb = moved[b][: sl[b]]
        q.append(qb)
        ql.append(len(qb))
    return np.concatenate(s), sl, np.concatenate(q), np.asarray(ql, np.int32)


def big_q(n=100000):
    rng = np.random.default_rng(104)
    lo = np.asarray([-0.05, -0.05, -0.05])
    ext = np.asarray([0.8, 0.25, 0.25]) + 0.1
    return (lo + rng.random((n, 3)) * ext).astype(np.float32)


def far_queries(s):
    """queries outside the support box: within a cell of it, two cells away, and far beyond the +-2 cell clamp of the kernels"""
    lo, hi = s.min(0).astype(np.float64), s.max(0).astype(np.float64)
    mid = 0.5 * (lo + hi)
    out = []
    for d in range(3):
        for step in (0.03, 0.07, 0.16, 0.5, 9.0):
            for sign in (-1.0, 1.0):
                p = mid.copy()
                p[d] = (hi[d] + step) if sign > 0 else (lo[d] - step)
                out.append(p)
    out += [hi + 0.03, lo - 0.03, hi + 5.0, lo - 5.0]
    return np.asarray(out, np.float32)


def boundary():
    """-> (queries [1 + fill, 3], supports, r, excluded indices, included index): r = 0.125 = 2^-3, query c = (0.5, 0.5, 0.5); the
    supports c +- r e_axis have dx = +-0.125 exactly, so d2 == r2 == 2^-6 bit for bit; one more sits one ulp inside on the x axis."""
    r = np.float32(0.125)
    c = np.asarray([0.5, 0.5, 0.5], np.float32)
    rng = np.random.default_rng(105)
    fill = (rng.random((60, 3)) * 0.5 + 0.25).astype(np.float32)
    on = []
    for d in range(3):
        for sign in (-1.0, 1.0):
            p = c.copy()
            p[d] = np.float32(c[d] + sign * r)
            on.append(p)
    inside = c.copy()
    inside[0] = np.nextafter(np.float32(0.625), np.float32(0))
    s = np.concatenate([fill[:20], np.asarray(on, np.float32), inside[None], fill[20:]]).astype(np.float32)
    q = np.concatenate([c[None], jitter(fill, 9)]).astype(np.float32)
    return q, s, r, np.arange(20, 26), 26


def duplicates(n, others=50):
    """`others` random points, then n copies of one point"""
    rng = np.random.default_rng(106)
    p = (rng.random((others + n, 3)) * 0.4).astype(np.float32)
    p[others:] = p[others]
    return p


# ---- conditions ---------------------------------------------------------------------------------------------------------------

def counts(want, n_s):
    """hits per row of an oracle matrix (padded with the number of supports)"""
    return (want != n_s).sum(1).astype(np.int64)


def band_counts(n):
    return [int(((n >= lo) & (n <= hi)).sum()) for lo, hi in BANDS]


def d2_bits(q, s, want):
    """uint32 [Nq, K]: the bits of fp32 (dx*dx + dy*dy) + dz*dz, dx = q - s, for every listed support (padding: 0xffffffff)"""
    q, s = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(s, np.float32)
    valid = want != len(s)
    sx = np.concatenate([s, np.zeros((1, 3), np.float32)])[np.minimum(want, len(s))]
    d = q[:, None, :] - sx
    p = d * d
    d2 = (p[..., 0] + p[..., 1]) + p[..., 2]
    assert d2.dtype == np.float32
    return np.where(valid, d2.view(np.uint32), np.uint32(0xffffffff))


def clash64(bits, n):
    """rows of at most 64 hits: do two of the row's keys agree in bits >> 6 (nb_cell_search.h, the 8-lane network's check)"""
    k = np.sort(np.where(np.arange(bits.shape[1])[None] < n[:, None], bits >> 6, 0xffffffff).astype(np.int64), axis=1)
    eq = (k[:, 1:] == k[:, :-1]) & (np.arange(1, bits.shape[1])[None] < n[:, None])
    return eq.any(1) & (n <= 64)


def clash128(bits, n, width):
    """rows of 65..128 hits: do two neighbours among the first width + 1 sorted keys agree in bits >> 7 (the 128-key network)"""
    k = np.sort(np.where(np.arange(bits.shape[1])[None] < n[:, None], bits >> 7, 0xffffffff).astype(np.int64), axis=1)
    k = k[:, : width + 1]
    eq = k[:, 1:] == k[:, :-1]
    return eq.any(1) & (n >= 65) & (n <= 128)


def cell_geometry(s, r):
    """-> (mn, inv_h, dims) of one element as nb_prep derives them: cell edge h = r (1 + 2^-20), and -- like nb_prep and nb_cell_of --
    the fp64 product with inv_h = 1 / h, not a division by h (a point on a cell border can differ between the two)"""
    inv_h = 1.0 / (float(np.float32(r)) * (1.0 + 1.0 / 1048576.0))
    mn = s.min(0).astype(np.float64)
    mx = s.max(0).astype(np.float64)
    dims = (np.floor((mx - mn) * inv_h) + 1).astype(np.int64)
    return mn, inv_h, dims


def cell_of(p, mn, inv_h):
    """nb_cell_of: floor((x - mn) * inv_h) in fp64, not clamped"""
    return np.floor((np.asarray(p, np.float64) - mn) * inv_h).astype(np.int64)


def cells_not_doubled(s, lens, r):
    """every element's grid fits its share of the cell budget at the first cell edge: dims product <= max(4 Ns, 65536) / B"""
    per = max(4 * len(s), 65536) // len(lens)
    off = 0
    for n in lens:
        if n > 0 and int(np.prod(cell_geometry(s[off: off + n], r)[2])) > per:
            return False
        off += int(n)
    return True


def stencil_candidates(s, lens, r):
    """int64 [Ns]: supports in the 27 cells around every support's own cell, of its own element"""
    out = np.zeros(len(s), np.int64)
    off = 0
    for n in lens:
        n = int(n)
        if n > 0:
            p = s[off: off + n]
            mn, inv_h, dims = cell_geometry(p, r)
            c = np.clip(cell_of(p, mn, inv_h), 0, dims - 1)
            hist = np.zeros(tuple(dims + 2), np.int64)
            np.add.at(hist, (c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1), 1)
            box = np.zeros(tuple(dims), np.int64)
            for dx in range(3):
                for dy in range(3):
                    for dz in range(3):
                        box += hist[dx: dx + dims[0], dy: dy + dims[1], dz: dz + dims[2]]
            out[off: off + n] = box[c[:, 0], c[:, 1], c[:, 2]]
        off += n
    return out


def expected(want, n_s, width, pad):
    """the oracle matrix as a search of `width` columns returns it: truncated / padded, the pad value replaced"""
    nq, k = want.shape
    out = np.full((nq, width), n_s, np.int64)
    out[:, : min(k, width)] = want[:, :width]
    return np.where(out == n_s, pad, out).astype(np.int32)


def renumber_back(mat, q_order, s_order, n_s, nq):
    """a matrix in the INTERNAL numbering -> the reference numbering: row j belongs to query q_order[j], an entry v in [0, n_s) is
    support s_order[v]; every other value (pad, sentinel) and every row from nq on stays"""
    out = mat.copy()
    v = mat[:nq].astype(np.int64)
    ok = (v >= 0) & (v < n_s)
    out[q_order[:nq]] = np.where(ok, s_order[np.where(ok, v, 0)], v).astype(mat.dtype)
    return out


# ---- scenes: "<cloud>-<queries>", inputs + the oracle's rows, computed once per process ---------------------------------------

class Scene:
    """s / sl: supports and their lens, q / ql: queries (q is s when same), r, want: the oracle's matrix (padded with len(s)),
    n: hits per row"""

    def __init__(self, name, s, sl, q, ql, same, r, want):
        self.name, self.s, self.sl, self.q, self.ql, self.same, self.r, self.want = name, s, np.asarray(sl, np.int32), q, \
            np.asarray(ql, np.int32), same, np.float32(r), want
        self.n = counts(want, len(s))
        self.first = np.where(self.n > 0, want[:, 0] if want.shape[1] else len(s), len(s))

    def bits(self):
        return d2_bits(self.q, self.s, self.want)


def _lens(*n):
    return np.asarray(n, np.int32)


def _self(s, sl, grid=False):
    """queries = supports"""
    return s, sl, s, sl, True, R, grid


def _other(s, sl, far=False, grid=False):
    """the supports moved by N(0, 0.02); far: far_queries(s) appended to the first cloud's queries"""
    q, ql = jitter(s, 1), sl.copy()
    if far:
        extra = far_queries(s)
        q = np.concatenate([q[: sl[0]], extra, q[sl[0]:]])
        ql[0] += len(extra)
    return s, sl, q, ql, False, R, grid


def _slabdup():
    """40 copies of slab[100] among the supports, and the first 40 queries on that point"""
    s = slab()
    s[100:140] = s[100]
    s, sl, q, ql, same, r, grid = _other(s, _lens(3000))
    q[:40] = s[100]
    return s, sl, q, ql, same, r, grid


def _bigq(n):
    return graded(), _lens(2500), big_q()[:n], _lens(n), False, R, True


def _many(B, ends_empty, same):
    s, sl, q, ql = many(B, ends_empty)
    return _self(s, sl) if same else (s, sl, q, ql, False, R, False)


# name -> () -> (s, sl, q, ql, queries are the supports, r, use the oracle's grid form); the names are keys, nothing parses them
SCENE_BUILDERS = {
    "slab-self": lambda: _self(slab(), _lens(3000)),
    "slab-other": lambda: _other(slab(), _lens(3000)),
    "slab-far": lambda: _other(slab(), _lens(3000), far=True),
    "slabdup-other": _slabdup,
    "graded-self": lambda: _self(graded(), _lens(2500)),
    "graded-other": lambda: _other(graded(), _lens(2500)),
    "graded-far": lambda: _other(graded(), _lens(2500), far=True),
    "graded-bigq": lambda: _bigq(100000),
    "graded-bigq99999": lambda: _bigq(99999),
    "lattice-self": lambda: _self(lattice(), _lens(800)),
    "lattice-other": lambda: _other(lattice(), _lens(800)),
    "graded2497-self": lambda: _self(graded(2497), _lens(2497)),
    "graded2497x3-self": lambda: _self(graded(2497), split3(2497)),
    "lattice797-self": lambda: _self(lattice(797), _lens(797)),
    "lattice797x3-self": lambda: _self(lattice(797), split3(797)),
    "tiled40000-self": lambda: _self(*tiled_slab(40000), grid=True),
    "tiled40000-other": lambda: _other(*tiled_slab(40000), grid=True),
    "tiled39999-self": lambda: _self(*tiled_slab(39999), grid=True),
    "tiled39999-other": lambda: _other(*tiled_slab(39999), grid=True),
}
for _B in (40, 41, 255):
    for _e in (False, True):
        for _same in (False, True):
            SCENE_BUILDERS["many%d%s-%s" % (_B, "e" if _e else "", "self" if _same else "other")] = \
                (lambda B=_B, e=_e, same=_same: _many(B, e, same))


def scene_inputs(name):
    return SCENE_BUILDERS[name]()


_SCENES = {}


def scene(coracle, name):
    if name not in _SCENES:
        s, sl, q, ql, same, r, grid = scene_inputs(name)
        want = coracle.batch_neighbors(q, s, ql, sl, r, grid=grid)
        _SCENES[name] = Scene(name, s, sl, q, ql, same, r, want)
    return _SCENES[name]
