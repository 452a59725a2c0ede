"""Host-only part of tests/test_gpu_subsample_branches.py: the builders of oracle/subsample_cases.py are seeded and shaped as stated,
and for EVERY case of the GPU file the oracle's voxel count per cloud is the intended M, the host mirror of the dispatcher
(subsample_cases.form, restating gs_run / gs_run_small) gives the intended form for each call, the sort key has the intended width
and pass count, the iteration order has the intended number of rounds, the crowded voxels are sensitive to the order of the fp32 sum
and sit where the case names say in the sorted sequence.  Where oracle/_ref is built the reference's own C++ equals the C oracle on
the lattice cases."""
import numpy as np
import pytest

from conftest import bits
from oracle import subsample_cases as sc

CASES = sc.cases()


@pytest.fixture(scope="module")
def oracle_rows(coracle):
    out = {}
    for name, c in CASES.items():
        p, lens = c.data()
        out[name] = coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), c.dl)
    return out


def test_builders_are_seeded_and_shaped():
    for f in (lambda: sc.lattice(1, 100, 0.05, (-37, 12, -5)), lambda: sc.box_cloud(2, 64, 32, 32, 50), lambda: sc.run_cloud(3, 257, 0)[0],
              sc.neg_cell_cloud, lambda: sc.on_grid_cloud(0.03), lambda: sc.key64_cloud(10, 1 << 16, 1 << 15)):
        a, b = f(), f()
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and np.array_equal(bits(a), bits(b))
    p, vid, cells = sc.lattice_full(4, 200, 0.1, (400, -400, 90), per=(1, 3))
    assert len(np.unique(cells, axis=0)) == 200 and np.bincount(vid).min() >= 1 and np.bincount(vid).max() <= 3
    G = 10                                                   # 10^3 >= 4 * 200 > 9^3
    assert (cells - np.asarray([400, -400, 90]) >= 0).all() and (cells - np.asarray([400, -400, 90]) < G).all()
    frac = p / np.float32(0.1) - cells[vid]
    assert frac.min() > 0.19 and frac.max() < 0.81           # at least 0.1 cell from every wall (0.2 less the fp32 rounding of 400 cells)
    assert np.array_equal(sc.voxel_keys(p, 0.1) == sc.voxel_keys(p, 0.1)[:1], vid == vid[0])
    assert len(sc.lattice(5, 300, 0.05, total=1000)) == 1000 and len(sc.lattice(5, 300, 0.05, per=2)) == 600
    assert np.array_equal(sc.box(8, 8, 4), [[0.5, 0.5, 0.5], [7.5, 7.5, 3.5]]) and sc.grid_dims(sc.box(8, 8, 4), 1.0)[1] == [8, 8, 4]
    assert sc.grid_dims(sc.box(1 << 19, 1 << 19, 1 << 18), 1.0)[1] == [1 << 19, 1 << 19, 1 << 18]        # half-integers: exact
    assert len(sc.many_lens()) == 255 and min(sc.many_lens()) == 1 and max(sc.many_lens()) == 40 and sum(sc.many_lens()) < 6000
    assert max(len(c.data()[0]) for c in CASES.values()) == 16386        # 16385 + the one-point cloud


@pytest.mark.parametrize("dl", [0.03, 0.05, 0.1])
@pytest.mark.parametrize("shift", sc.SHIFTS)
def test_lattice_has_exactly_M_voxels(coracle, dl, shift):
    for M in sc.ROUND_M:
        p = sc.lattice(1000 + M, M, dl, shift, total=None if M <= 5087 else 16000)
        assert len(coracle.grid_subsampling(p, dl)) == M, (M, dl, shift)


def test_mirror_of_the_dispatcher():
    assert sc.form(5000, None) == "hash"
    assert sc.form(16384, 5087) == ("small", 1024, 16, 5087) and sc.form(16385, 5087) == "sort" and sc.form(16384, 5088) == "sort"
    assert sc.form(16385, 5088, 5087, 16384) == ("small", 1024, 16, 5087) and sc.form(16385, 5088, 5087, 16384, in_place=True) == "sort"
    assert sc.form(9000, 9000, 0, 2048) == ("small", 256, 8, 2357)       # the voxel capacity is cut to the point capacity
    assert sc.form(9000, 9000, 1109, 2049) == ("small", 512, 8, 1109) and sc.form(9000, 9000, 1110, 4097) == ("small", 1024, 8, 2357)
    assert sc.form(20000, 20000, 2358, 8193) == ("small", 1024, 12, 5087) and sc.form(20000, 20000, 13, 12289) == ("small", 1024, 16, 1109)
    assert [sc.rounds(M) for M in (1, 13, 14, 1109, 1110, 2357, 2358, 10273, 10274)] == \
        [(1, 0), (1, 0), (2, 0), (7, 0), (7, 1), (7, 1), (7, 2), (7, 3), (7, 4)]


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_what_it_says(oracle_rows, name):
    c = CASES[name]
    p, lens = c.data()
    want_p, want_l = oracle_rows[name]
    assert list(want_l) == c.M and len(want_p) == sum(c.M)
    calls = c.calls()
    assert [k.kind for k in calls] == list(c.kinds)
    for k in calls:
        assert k.form() == k.want, (k, k.form(), k.want)
        if k.kind != "hash":
            assert k.N_cap > len(p) and k.M_cap >= sum(c.M)
    if "sort" in c.kinds or "inplace" in c.kinds:
        kb, eb, passes = sc.sort_bits(p, lens, c.dl)
        assert c.bits == kb + eb and passes == (c.bits + 7) // 8, (kb, eb, passes)
    else:
        assert c.bits is None                                            # (the one-workgroup form sorts by its own kb alone)
    n_rounds = 1 + sum(nb < max(c.M) for nb in sc.CHAIN)                     # a rehash for every bucket count the map outgrows
    assert sum(c.rounds()) == n_rounds and c.rounds()[0] == min(n_rounds, 7)
    if "small" in c.kinds:        # the one-workgroup form holds every round in LDS: the largest cloud fits the stated nbmax
        nb = next(k for k in calls if k.kind == "small").want[3]
        assert max(c.M) <= nb and max(c.M) <= (c.small_cap or nb)


def test_stated_branches_of_the_case_table():
    ks = {n: [k for k in c.calls()] for n, c in CASES.items()}
    # order-round boundaries: hash and sort for every M, one workgroup up to 5087 with nbmax as stated, M == elem_cap, M == nbmax
    for M in sc.ROUND_M:
        kinds = [k.kind for k in ks["rounds-%d" % M]]
        assert kinds == (["hash", "sort", "small"] if M <= 5087 else ["hash", "sort"])
        if M <= 5087:
            k = ks["rounds-%d" % M][2]
            assert k.want[3] == sc.SMALL_NB[M] and k.elem_cap == sc.SMALL_CAP[M]
    assert {sc.SMALL_NB[M] for M in sc.SMALL_NB} == {1109, 2357, 5087}
    assert all(sc.SMALL_CAP[M] == M for M in (14, 128, 542, 1110, 2358, 1109, 2357, 5087))
    assert all(sc.SMALL_CAP[M] == sc.SMALL_NB[M] == M for M in (1109, 2357, 5087))
    # the five instantiations at both edges of their bands
    got = {L: ks["wg-%d" % L][0].want[1:3] for L in sc.WG_LEN}
    assert got == {2048: (256, 8), 2049: (512, 8), 4096: (512, 8), 4097: (1024, 8), 8192: (1024, 8), 8193: (1024, 12), 12288: (1024, 12),
                   12289: (1024, 16), 16384: (1024, 16)}
    for L, (M, T, R) in sc.WG_LEN.items():
        assert CASES["wg-%d" % L].data()[1] == [L, 1] and 1900 <= M <= 5000 and ks["wg-%d" % L][0].elem_points == L
    assert CASES["wg-16385"].data()[1] == [16385, 1] and ks["wg-16385"][0].want == "sort"
    # pass counts 1..4 and the kb == 32 branch
    assert [(b, (b + 7) // 8) for b in sc.PASS_BOXES] == [(8, 1), (9, 2), (16, 2), (17, 3), (24, 3), (25, 4), (32, 4)]
    assert sc.sort_bits(*CASES["passes-32"].data(), 1.0) == (32, 0, 4)
    # tile edges
    assert [sum(CASES["tile-%d" % n].data()[1]) for n in (8191, 8192, 8193, 16385)] == [8191, 8192, 8193, 16385]
    for n in (8191, 8192, 8193, 16385):
        offs = np.cumsum(CASES["tile-%d" % n].data()[1])
        assert sc.RS_WAVE_ITEMS < offs[0] < offs[1] < 2 * sc.RS_WAVE_ITEMS          # wave 1 (rows 1024..2047) holds three clouds
    assert CASES["mixed"].M == [5, 1110, 60, 2358, 1] and len(CASES["many-255"].M) == sc.MAX_BATCH


def test_wg_16385_differs_from_wg_16384_in_one_row(oracle_rows):
    a, la = oracle_rows["wg-16384"]
    b, lb = oracle_rows["wg-16385"]
    assert np.array_equal(la, lb) and a.shape == b.shape
    assert (bits(a) != bits(b)).any(1).sum() == 1


def _voxel_points(p, dl, point):
    k = sc.voxel_keys(p, dl)
    return p[k == k[point]]


def _sum_bits(q):
    s = np.zeros(3, np.float32)
    for row in q:
        s = (s + row).astype(np.float32)
    return bits(s)


@pytest.mark.parametrize("c,start_mod", sc.RUNS)
def test_runs_lie_where_the_case_names_say(oracle_rows, c, start_mod):
    case = CASES["run-%d-at-%d" % (c, start_mod)]
    p, lens = case.data()
    _, first = sc.run_cloud(7000 + c + start_mod, c, start_mod)
    start, length = sc.sorted_run(p, lens, case.dl, 0, first)
    print("run of", length, "points at sorted positions", start, "..", start + length - 1, "blocks", start // 256, "..", (start + length - 1) // 256)
    assert length == c and start % 256 == start_mod and start >= 256
    blocks = (start + length - 1) // 256 - start // 256 + 1
    assert blocks == {(2, 255): 2, (255, 1): 1, (256, 0): 1, (256, 130): 2, (257, 0): 2, (700, 50): 3, (700, 255): 4}[(c, start_mod)]
    if (c, start_mod) in ((255, 1), (256, 0)):
        assert (start + length) % 256 == 0                                # ends exactly at a block edge
    q = _voxel_points(p, case.dl, first)
    assert len(q) == c and q.min() > 0 and q.max() / q.min() >= 2.0 ** 12    # magnitudes spread over 2^12 inside one cell
    if c > 2:                                                                 # (a sum of two is the same either way)
        assert not np.array_equal(_sum_bits(q), _sum_bits(q[::-1]))           # the order of the sum shows in the bits


def test_crowded_voxels_of_the_shift_cases_are_order_sensitive():
    for i in range(5):
        case = CASES["shift-%d" % i]
        p, lens = case.data()
        a = p[: lens[0]]
        k = sc.voxel_keys(a, case.dl)
        u, cnt = np.unique(k, return_counts=True)
        assert cnt.max() == 40
        q = a[k == u[np.argmax(cnt)]]
        assert not np.array_equal(_sum_bits(q), _sum_bits(q[::-1]))


def test_neg_cell_input_has_its_origin_above_the_minimum():
    p = sc.neg_cell_cloud()
    dl = np.float32(0.03)
    mn = p[:, 0].min()
    assert mn == np.float32(0.029999997) and mn < dl
    org = np.floor(mn * (np.float32(1.0) / dl)) * dl
    assert org.dtype == np.float32 and org == dl and org > mn
    assert np.floor((mn - org) / dl) == -1.0
    assert sc.grid_dims(p, 0.03)[0][0] == org


def test_key64_clouds_have_the_stated_keys():
    for M, (NZ, zmin, lg) in sc.KEY64.items():
        k = np.unique(sc.voxel_keys(sc.key64_cloud(M, NZ, zmin), 1.0))
        assert len(k) == M and k[0] == 0 and (1 << lg) <= int(k[1]) and int(k[-1]) < (1 << (lg + 1)) <= (1 << 56)


def test_c_oracle_equals_the_reference_on_the_lattice_cases(coracle, reflib, refwrap):
    for name, c in CASES.items():
        p, lens = c.data()
        if max(lens) > 5000 and not name.startswith(("wg-16384", "rounds-10274")):
            continue                                                    # (the larger clouds repeat the builder of the smaller ones)
        want_p, want_l = coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), c.dl)
        ref_p, ref_l = reflib.batch_grid_subsampling(p, np.asarray(lens, np.int32), c.dl)
        assert np.array_equal(ref_l, want_l) and np.array_equal(bits(ref_p), bits(want_p)), name
    p = sc.lattice(9400, 1110, 0.05)
    rng = np.random.default_rng(1)
    f = rng.standard_normal((len(p), 4)).astype(np.float32)
    cl = rng.integers(-5, 5, (len(p), 3)).astype(np.int32)
    for a, b in zip(coracle.grid_subsampling(p, 0.05, f, cl), refwrap.grid_subsampling(p, 0.05, f, cl)):
        assert np.array_equal(bits(a), bits(b))


def test_forms_the_workload_size_script_runs(coracle):
    """tests/gs_sort_path_check.py (a GPU subprocess) cannot be imported here, so its table of seeded cases is repeated: the counts
    its docstring and that of test_capacity_mode_forms_of_the_subsampler_equal_the_oracle state are the mirror's, not assumed."""
    rng = np.random.default_rng(3)
    first, second, passes, big = [], [], [], 0
    for B, n, dl, spread in [(1, 5000, 0.05, 1.0), (4, 20000, 0.03, 2.2), (8, 3000, 0.1, 1.0), (3, 40000, 0.02, 0.5), (2, 1, 0.05, 1.0),
                             (5, 700, 0.5, 1.0), (1, 4096, 0.05, 1.0), (1, 4097, 0.05, 1.0), (2, 8192, 0.04, 1.5), (100, 300, 0.1, 1.0),
                             (2, 60000, 0.3, 150.0), (4, 300000, 0.03, 1.68), (1, 1, 0.03, 1.0), (8, 11000, 0.06, 1.68),
                             (8, 16384, 0.1, 2.0), (16, 2500, 0.12, 1.68), (8, 800, 0.24, 1.68), (3, 2048, 0.01, 1.0), (2, 5000, 0.3, 150.0)]:
        lens = [max(1, int(n * f)) for f in rng.uniform(0.5, 1.0, B)] if n > 1 else [1] * B
        pts = [((rng.random((l, 3)) * spread) + rng.uniform(-3, 3, 3)).astype(np.float32) for l in lens]
        pts[0][: min(10, lens[0])] = pts[0][0]
        p = np.concatenate(pts)
        mv = int(coracle.batch_grid_subsampling(p, np.asarray(lens, np.int32), dl)[1].max())
        cap = len(p) + 1000
        first.append(sc.form(cap, cap, max(lens), 0))
        if first[-1] == "sort":
            passes.append(sc.sort_bits(p, lens, dl)[2])
        if max(lens) <= 16384 and mv <= 5087:
            second.append(sc.form(cap, cap, mv, max(lens)))
        if first[-1] != "sort" or (max(lens) <= 16384 and mv <= 5087):
            big = max(big, max(lens))
    assert first.count("sort") == 10 and len(first) == 19 and sorted(passes) == [2, 2, 3, 3, 3, 3, 3, 3, 3, 4]
    assert first[6] == ("small", 1024, 8, 5087) and first[7] == ("small", 1024, 8, 5087)           # (1, 4096) and (1, 4097)
    assert len(second) == 12 and all(f != "sort" for f in second)
    small = {f[1:3] for f in first + second if f != "sort"}
    assert small == {(256, 8), (512, 8), (1024, 8), (1024, 12)} and big == 3980
