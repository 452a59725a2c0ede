"""Host-only part of tests/test_gpu_neighbor_branches.py: the case builders of oracle/neighbor_cases.py are seeded and shaped as
stated, the preconditions of the GPU tests (rows in every band, rows with and without a key clash, streamed and register-resident
stencils, bit-exact radius boundary) hold on the oracle's result, and COracle.batch_neighbors(grid=True) equals the brute force
(grid=False) on every small cloud of that file -- which is what lets the 100 000-query cases use grid=True."""
import numpy as np
import pytest

from oracle import neighbor_cases as nc


def _self(coracle, s, lens, r=nc.R, grid=False):
    return coracle.batch_neighbors(s, s, lens, lens, r, grid=grid)


@pytest.fixture(scope="module")
def graded_rows(coracle):
    s = nc.graded()
    lens = np.asarray([len(s)], np.int32)
    want = _self(coracle, s, lens)
    return s, lens, want, nc.counts(want, len(s))


def test_builders_are_seeded_and_shaped():
    assert nc.slab().shape == (3000, 3) and nc.graded().shape == (2500, 3) and nc.lattice().shape == (800, 3)
    for f in (nc.slab, nc.graded, nc.lattice, nc.big_q):
        assert f().dtype == np.float32 and np.array_equal(f(), f())
    assert nc.big_q().shape == (100000, 3)
    assert int(nc.many_lens(255).sum()) == 5406 and (nc.many_lens(255) == 0).sum() == 36
    for B in (40, 41, 255):
        for ends in (False, True):
            s, sl, q, ql = nc.many(B, ends)
            assert len(sl) == len(ql) == B and sl.sum() == len(s) and ql.sum() == len(q)
            assert ((sl == 0) & (ql > 0)).any() and ((sl > 0) & (ql == 0)).any() and (sl[1:-1] == 0).any()
            assert (not ends) or (sl[0] == 0 and sl[-1] == 0 and ql[0] == 0)
    assert np.array_equal(nc.many(40)[0], nc.many(255)[0][: nc.many_lens(40).sum()])       # prefixes of one stack
    p, lens = nc.tiled_slab()
    assert p.shape == (40000, 3) and lens.sum() == 40000 and len(lens) == 3
    for n in (2497, 797):       # the cell kernel's sizes: multiples of neither Q nor 4 Q
        assert all(n % Q and n % (4 * Q) for Q in (3, 8, 9, 16, 32)) and n % 4
        assert nc.split3(n).sum() == n and (nc.split3(n) > 0).all()


def test_bands_of_the_clouds(coracle, graded_rows):
    s = nc.slab()
    n = nc.counts(_self(coracle, s, [len(s)]), len(s))
    assert (n <= 64).sum() >= 2900 and n.max() <= 128
    s, lens, want, n = graded_rows
    b = nc.band_counts(n)
    print("graded bands", b, "kmax", n.max())
    assert all(x > 0 for x in b) and 192 < n.max() <= 256
    s = nc.lattice()
    n = nc.counts(_self(coracle, s, [len(s)]), len(s))
    assert (n == 81).sum() > 0 and (n <= 64).sum() > 0 and n.max() == 81
    # the prefixes the cell kernel runs on keep every band
    for cloud, m in ((nc.graded(2497), 2497), (nc.lattice(797), 797)):
        for lens in ([m], nc.split3(m)):
            n = nc.counts(_self(coracle, cloud, lens), m)
            assert (n <= 64).sum() > 0 and ((n > 64) & (n <= 128)).sum() > 0


def test_clash_classes_both_occur(coracle, graded_rows):
    s, lens, want, n = graded_rows
    bits = nc.d2_bits(s, s, want)
    c64 = nc.clash64(bits, n)
    print("graded: <= 64 rows", int((n <= 64).sum()), "with a 26-bit clash", int(c64.sum()))
    assert 0 < c64.sum() < (n <= 64).sum()
    for width in (38, 63):
        c128 = nc.clash128(bits, n, width)
        mid = (n >= 65) & (n <= 128)
        print("graded: 65..128 rows", int(mid.sum()), "with a 25-bit clash in the first", width + 1, ":", int(c128.sum()))
        assert 0 < c128.sum() < mid.sum()
    s = nc.lattice()
    want = _self(coracle, s, [len(s)])
    n = nc.counts(want, len(s))
    bits = nc.d2_bits(s, s, want)
    assert nc.clash64(bits, n)[n <= 64].all() and nc.clash128(bits, n, 38)[n > 64].all()     # every row has ties
    # d2_bits is the oracle's metric: every listed row is ascending by (d2, index), the first entry of a self-search is the query
    key = (bits.astype(np.int64) << 32) | want
    assert (np.diff(key, axis=1) > 0)[np.arange(1, want.shape[1])[None] < n[:, None]].all()
    assert np.array_equal(want[:, 0], np.arange(len(s)))


def test_streamed_and_resident_stencils_both_occur(graded_rows):
    for m, lens in ((2497, [2497]), (2497, nc.split3(2497))):
        s = nc.graded(m)
        assert nc.cells_not_doubled(s, lens, nc.R)
        T = nc.stencil_candidates(s, lens, nc.R)
        print("graded", list(lens), "stencils above", nc.NBC_CHUNK, ":", int((T > nc.NBC_CHUNK).sum()), "of", m, "max", int(T.max()))
        assert (T > nc.NBC_CHUNK).sum() > 0 and (T <= nc.NBC_CHUNK).sum() > 0
    s, lens, want, n = graded_rows
    assert (nc.stencil_candidates(s, lens, nc.R) >= n).all()          # the 27 cells hold every hit


def test_grid_oracle_equals_brute_force_on_the_small_clouds(coracle):
    clouds = [(nc.slab(), [3000]), (nc.graded(), [2500]), (nc.lattice(), [800]), (nc.graded(2497), nc.split3(2497)),
              (nc.lattice(797), nc.split3(797))]
    for s, lens in clouds:
        q = nc.jitter(s, 1)
        for a in (s, q, np.concatenate([q[: lens[0] - 30], nc.far_queries(s), q[lens[0]:]])):
            ql = np.asarray(lens, np.int32).copy()
            ql[0] += len(a) - len(s)
            assert np.array_equal(coracle.batch_neighbors(a, s, ql, lens, nc.R, grid=True),
                                  coracle.batch_neighbors(a, s, ql, lens, nc.R, grid=False))
    for B in (40, 255):
        s, sl, q, ql = nc.many(B, True)
        assert np.array_equal(coracle.batch_neighbors(q, s, ql, sl, nc.R, grid=True), coracle.batch_neighbors(q, s, ql, sl, nc.R, grid=False))
    bq = nc.big_q()[:5000]
    s = nc.graded()
    assert np.array_equal(coracle.batch_neighbors(bq, s, [5000], [2500], nc.R, grid=True),
                          coracle.batch_neighbors(bq, s, [5000], [2500], nc.R, grid=False))


def test_big_q_has_every_band_and_empty_rows(coracle):
    s = nc.graded()
    want = coracle.batch_neighbors(nc.big_q(), s, [100000], [2500], nc.R, grid=True)
    n = nc.counts(want, 2500)
    print("big-q bands", nc.band_counts(n), "empty", int((n == 0).sum()))
    assert all(x > 0 for x in nc.band_counts(n)) and (n == 0).sum() > 0
    assert all(x > 0 for x in nc.band_counts(n[:99999]))


def test_boundary_supports_are_excluded_bit_for_bit(coracle):
    q, s, r, excluded, included = nc.boundary()
    want = coracle.batch_neighbors(q, s, [len(q)], [len(s)], r, grid=False)
    bits = nc.d2_bits(q[:1], s, np.concatenate([excluded, [included]])[None])
    r2 = np.float32(r * r).view(np.uint32)
    assert (bits[0, :6] == r2).all() and bits[0, 6] < r2
    row = want[0][want[0] != len(s)]
    assert included in row and not np.isin(excluded, row).any()


def test_expected_and_renumber_back():
    want = np.asarray([[0, 2, 5], [1, 5, 5]], np.int32)
    assert np.array_equal(nc.expected(want, 5, 2, -1), [[0, 2], [1, -1]])
    assert np.array_equal(nc.expected(want, 5, 5, 5), [[0, 2, 5, 5, 5], [1, 5, 5, 5, 5]])
    mat = np.asarray([[1, 0, 5, 77], [2, 5, 5, 77], [88, 88, 88, 88]], np.int32)      # rows by position, entries by position
    back = nc.renumber_back(mat, np.asarray([1, 0, 2]), np.asarray([4, 3, 2, 1, 0]), 5, 2)
    assert np.array_equal(back, [[2, 5, 5, 77], [3, 4, 5, 77], [88, 88, 88, 88]])
