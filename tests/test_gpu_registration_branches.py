"""Every kernel and branch of the four single-pair registration entry points -- d3f_feature_nn, d3f_mutual_matches,
d3f_ransac_hypotheses (csrc/registration.hip) and d3f_neighbor_grid_score (csrc/radius_neighbors.hip) -- against float64 / integer
expectations that no kernel had a part in (oracle/registration_np.py, tests/matching_np.d2_f64, three lines of numpy, an integer
restatement).  register_pairs, match_pairs and register_pairs_counts are tested bit for bit against these four (rg_sample and rg_fit
are compiled into them), so this file is what stands between an error here and three more entry points.  Nothing compares a kernel
with a kernel.

Inputs: oracle/registration_cases.py (seeded; every expectation is computed once per process).  Every case states what it means to
exercise; tests/test_registration_cases.py checks those statements, every margin and every cap on the CPU from the oracle alone.
Every entry point is called through _lib.load() with a workspace of exactly the advertised size and output buffers PAD rows longer
than documented, pre-filled with a sentinel that everything past the documented extent must keep.

Branch -> test
--------------
  rg_feature_nn_kernel<16>, <32>, <64> + rg_unpack_kernel        test_feature_nn[16-*], [32-*], [64-*]; each: contiguous and record rows
                                                                 (lda = ldb = C + 4, base 12 bytes into the buffer, NaN in every float
                                                                 that is no descriptor), d2_out given and NULL
  Nb = 1 / one row                                               test_feature_nn[*-1x1-*]
  rows past Na in the last block (255, 257, 700, 3 of 256)       test_feature_nn[*-255x127], [*-257x129], [*-700x1025], [*-3x20000]
  a split that ends exactly on a 128-row tile                    test_feature_nn[*-256x128] (one split, one full tile)
  one tile per split, 157 splits, last tile 32 / 33 rows         test_feature_nn[*-3x20000], [*-3x20001]
  ragged 114-row splits, three row blocks                        test_feature_nn[*-700x1025]
  Nb = 0 (no launch; idx -1, d2 FLT_MAX), Na = 0                 test_feature_nn[*-300x0], [*-0x5]
  operands of magnitude 1e3 (d2 ~ 1e6)                           test_feature_nn[32-*-1000]
  ties across column splits through the atomicMin key            test_feature_nn_ties_take_the_lowest_index[16], [32], [64] (both layouts)
  ties inside one tile through the strict `d2 < best`            the same tests: rows 1, 3, .., 59 of B repeat rows 0, 2, .., 58
  no finite distance: NaN row, overflowing row, NaN column       test_feature_nn_without_a_finite_distance[16], [32], [64]
  scan_fold_kernel<RgMutualIn, RgCountEpi> + rg_mutual_write_kernel      test_mutual_matches[Na]: Na = 0, 1, 1023, 1024, 1025 (both sides of
                                                                 D3F_SCAN_TILE), 3077 (four tiles) x Nb = 0, 7, Na, 2 Na x every pair
                                                                 mutual / none / half / ab with -1 and >= Nb (Nb, Nb + 3, INT_MAX);
                                                                 rows from the count on keep the sentinel; each call twice on one
                                                                 workspace (ticket counter); Nb = 0 with ba == NULL
  rg_hypotheses_kernel: ransac_n 3, 4, 5, 8 (RG_MAXN)            test_ransac_hypotheses[full-n3-*], [full-n4-*], [full-n5-*], [full-n8-*]
  edge checker off / on, distance checker off / on               test_ransac_hypotheses[*-e0-d0-*], [*-e0.9-d0-*], [*-e0-d0.05-*], [*-e0.9-d0.05-*]
  nn entries of -1 and Nt (rg_sample: no match)                  test_ransac_hypotheses[badnn-*]
  seed and it0 above 2^32 (it * 64 + d in 64 bits)               test_ransac_hypotheses[*-s1] (seed 2^63 + 11, it0 2^32 + 5); the draws
                                                                 against d3f_ransac_draw and the oracle's in every case
  H = 1999: 207 threads of the last block idle                   every test_ransac_hypotheses case
  most draws repeat / all repeat                                 test_ransac_hypotheses[five-n4-*], [five-n8-*]
  a target sample with two equal points                          test_ransac_hypotheses[full-*-e0-*] (nn is not injective)
  the identity of a failed sample (rg_hypothesis)                every test_ransac_hypotheses case, bit for bit
  rg_horn (12 Jacobi sweeps) against the SVD and numpy's eigh    every test_ransac_hypotheses case: orthogonality, det, the objective
                                                                 tr(R S) and the translation for EVERY fitted sample, the fp32 neighbour
                                                                 of the oracle's entries wherever the rotation is unique
  nb_score_kernel, V = 5, non-identity hypothesis 0, `nearest`   test_grid_score_exact: lower-index tie rule (lower index met first and
                                                                 met last), d2 == r2 is no inlier, one lattice step inside is, a moved
                                                                 point ON a target; every hypothesis also as hypothesis 0 of a V = 1 call
  V = 1, 2, 37 x Ns = 0, 1, 257, 1000 x Nt = 1, 50, 3000         test_grid_score_random[Nt-Ns-V]; `nearest` of hypothesis 0 with V > 1 and NULL
  clamp of a moved point to cells -2 / dims + 1                  test_grid_score_random[*-2], [*-37]: hypotheses 1 (2, 3) far outside
  cell -1: one cell outside, cell 0 still searched               test_grid_score_random[*-37]: hypotheses 4, 5, 6
  Ns = 0; count / sumd2 overwritten                              test_grid_score_random[*-0-*]; every scoring call starts from garbage

Tolerances (derived in oracle/registration_cases.py, none taken from what the kernels return): d2 within (C + 4) 2^-24 d2; idx = the
float64 argmin wherever the float64 gap exceeds twice that, else one of the two best; RANSAC and scoring as written at the
assertions.  Measured on the CPU (pytest -s tests/test_registration_cases.py): NO row of any feature_nn case has an ambiguous argmin
(0 of 7100 rows in the 36 cases; cap 1 % per case; the fp32 chain evaluated on the CPU stays within 0.33 of the d2 bound); ill-conditioned samples (relgap < 1e-3) are 0.36 % of the sample-passing hypotheses
(7 of 1969) in full-n3-e0-d0-s0 and full-n3-e0-d0.05-s0 and 0 % in the 21 other cases (cap 2 % per case; the per-case figures are
printed); Horn's eigenvector by numpy.linalg.eigh and the oracle's SVD agree to 2.4e-13 on every well-conditioned sample.

The RANSAC parameters are not a full product: every ransac_n meets every checker setting on the 300-point pair (16 cases, the two
(seed, it0) pairs alternating), four more cases use the nn with invalid entries and three the five-point source.

One defect found, in what an entry point ACCEPTS, fixed with this file (no defect found in what any kernel computes: every other
case passes on the parent's library as well):
  * test_mutual_matches[1], [1023], [1024], [1025], [3077], each at Nb = 0: an empty target block has no ba array to point at, and
    RgMutualIn tests j < Nb before it reads ba, but d3f_mutual_matches returned D3F_ERR_ARG for ba == NULL whatever Nb was (so
    registration.build_correspondence raised for an empty target).  Fix: ba may be NULL when Nb == 0.
d3f_feature_nn's answer for a row without a finite distance (idx -1, d2 FLT_MAX) was the kernels' behaviour already and is kept; it
is written into include/d3feat_amd.h now and test_feature_nn_without_a_finite_distance asserts it.

Sensitivity, run once on an MI355X with a copy of the library in which five things were changed (`d2 <= best` in
rg_feature_nn_kernel's walk, 3 Jacobi sweeps instead of 12, the iteration truncated to 32 bits in rg_draw, `d2 <= r2` and the higher
index on ties in nb_score_kernel): the three tie tests, all 23 RANSAC cases (the -s1 cases at the draws, the others at the fp32
neighbour of the oracle's entries) and test_grid_score_exact failed, the 81 other cases passed.

Cost, measured on an MI355X: the 108 cases take 5.1 s run alone (pytest's figure; the slowest is test_grid_score_random[3000-1000-37]
with 0.54 s, its float64 brute force of 37 x 1258 x 3000 distances on the host; nothing else reaches 0.2 s).  One complete
`pytest -m gpu tests` run with this file took 377.5 s (966 passed, 5 skipped; the parent's figure is about 348 s for 831 passed
before the three pull requests that followed it -- its suite today is this run less this file, about 372 s); only that one case
of this file is among the run's 40 slowest (place 33; 0.98 s in that run, before its brute force was shared between the builder
and the test).  The file adds 5.1 s, about 1.4 %, to the full run (the three bench.py configurations that
tests/test_gpu_configs.py starts are 213 s of it); 2 s of the 5.1 are the oracle's 23 x 1999 RANSAC hypotheses on the host.
"""
import numpy as np
import pytest
import torch

import matching_np as mnp
from conftest import bits
from oracle import registration_cases as rc
from oracle import registration_np as onp

pytestmark = pytest.mark.gpu

PAD = rc.PAD


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)        # a copy: the cached case arrays are read-only


def _ws(nbytes, dev):
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)


# ---- d3f_feature_nn ----------------------------------------------------------------------------------------------------------------
def _nn_call(dev, A, B, C, strided, want_d2):
    """-> (idx i32[Na + PAD], d2 f32[Na + PAD] or None) of one d3f_feature_nn call on sentinel-filled outputs"""
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    Na, Nb = len(A), len(B)
    if strided:
        ta, tb, ld = _t(rc.records(A, C), dev), _t(rc.records(B, C), dev), C + 4
        pa, pb = ta.data_ptr() + 12, tb.data_ptr() + 12
        assert pa % 16 != 0 and pa % 4 == 0
    else:
        ta, tb, ld = _t(A, dev), _t(B, dev), C
        pa, pb = (ta.data_ptr() if Na else None), (tb.data_ptr() if Nb else None)
    idx = torch.full((Na + PAD,), int(rc.SENT_I), dtype=torch.int32, device=dev)
    d2 = torch.full((Na + PAD,), float(rc.SENT_F), dtype=torch.float32, device=dev) if want_d2 else None
    ws = _ws(lib.d3f_feature_nn_workspace_bytes(Na), dev)
    _lib.check(lib.d3f_feature_nn(pa, Na, ld, pb, Nb, ld, C, idx.data_ptr(), d2.data_ptr() if want_d2 else None, ws.data_ptr(), ws.numel(),
                                  ops._stream(dev)), "feature_nn")
    return idx.cpu().numpy(), (d2.cpu().numpy() if want_d2 else None)


def _nn_check(ref, C, Na, idx, d2, no_match=()):
    """idx / d2 of one call against the float64 reference; rows `no_match` must report -1 / FLT_MAX"""
    assert np.array_equal(idx[Na:], np.full(PAD, rc.SENT_I)), "idx written past Na"
    if d2 is not None:
        assert np.array_equal(bits(d2[Na:]), bits(np.full(PAD, rc.SENT_F))), "d2 written past Na"
    idx, rows = idx[:Na].astype(np.int64), np.arange(Na)
    none = np.zeros(Na, bool)
    none[list(no_match)] = True
    if ref["D"].shape[1] == 0:
        none[:] = True
    assert np.array_equal(idx[none], np.full(int(none.sum()), -1))
    ok = ~none
    sure = ref["sure"] & ok
    assert np.array_equal(idx[sure], ref["idx"][sure]), np.nonzero(sure & (idx != ref["idx"]))[0][:5]
    loose = ok & ~ref["sure"]
    assert np.all((idx[loose] == ref["idx"][loose]) | (idx[loose] == ref["idx2"][loose]))
    if d2 is not None:
        assert np.array_equal(bits(d2[:Na][none]), bits(np.full(int(none.sum()), rc.FLT_MAX)))
        want = ref["D"][rows[ok], idx[ok]]
        err = np.abs(d2[:Na][ok].astype(np.float64) - want)
        assert np.all(err <= rc.nn_bound(C, want)), float((err / np.maximum(rc.nn_bound(C, want), 1e-300)).max())


NN_PARAMS = [(C, s, 1.0) for C in rc.NN_WIDTHS for s in rc.NN_SHAPES] + [(32, s, 1e3) for s in rc.NN_SHAPES]


@pytest.mark.parametrize("C,shape,scale", NN_PARAMS, ids=["%d-%dx%d-%g" % (C, s[0], s[1], k) for C, s, k in NN_PARAMS])
def test_feature_nn(device, C, shape, scale):
    A, B = rc.nn_data(C, *shape, scale=scale)
    ref = rc.nn_reference(A, B, C, mnp.d2_f64)
    for strided in (False, True):
        for want_d2 in (True, False):
            idx, d2 = _nn_call(device, A, B, C, strided, want_d2)
            _nn_check(ref, C, len(A), idx, d2)


@pytest.mark.parametrize("C", rc.NN_WIDTHS)
def test_feature_nn_ties_take_the_lowest_index(device, C):
    """Bit-equal copies of every row of B in different column splits (the first copy wins through the (d2 bits, column) key) and of
    thirty rows next to each other in one tile (the first wins through the strict comparison of the walk)."""
    A, B, want = rc.nn_tie_data(C)
    for strided in (False, True):
        idx, d2 = _nn_call(device, A, B, C, strided, True)
        assert np.array_equal(idx[:300], want) and np.array_equal(bits(d2[:300]), np.zeros(300, np.uint32))
        assert np.array_equal(idx[300:], np.full(PAD, rc.SENT_I))


@pytest.mark.parametrize("C", rc.NN_WIDTHS)
def test_feature_nn_without_a_finite_distance(device, C):
    """include/d3feat_amd.h: a row of A none of whose distances is below FLT_MAX (all NaN, or every d2 overflows) reports idx -1 and
    d2 FLT_MAX, as for Nb == 0; a NaN row of B is never the answer of another row."""
    A, B = rc.nn_nofinite_data(C)
    ref = rc.nn_reference(A, B, C, mnp.d2_f64)
    for strided in (False, True):
        for want_d2 in (True, False):
            idx, d2 = _nn_call(device, A, B, C, strided, want_d2)
            _nn_check(ref, C, len(A), idx, d2, no_match=rc.NN_NOFINITE_ROWS)
            assert not (idx[:len(A)] == rc.NN_NOFINITE_NAN_COLUMN).any()


# ---- d3f_mutual_matches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Na", rc.MM_NA)
def test_mutual_matches(device, Na):
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    ws = _ws(lib.d3f_mutual_matches_workspace_bytes(Na), device)
    for Nb in rc.mm_nb(Na):
        for fill in rc.MM_FILLS:
            ab, ba = rc.mm_case(Na, Nb, fill)
            want = rc.mm_expected(ab, ba, Nb)
            tab, tba = _t(ab, device), _t(ba, device)
            got = []
            for rep in range(2):                                               # the second call meets the first one's workspace
                pairs = torch.full((Na + PAD, 2), int(rc.SENT_I), dtype=torch.int32, device=device)
                count = torch.full((1 + PAD,), int(rc.SENT_I), dtype=torch.int32, device=device)
                _lib.check(lib.d3f_mutual_matches(tab.data_ptr() if Na else None, Na, tba.data_ptr() if Nb else None, Nb, pairs.data_ptr(),
                                                  count.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(device)), "mutual_matches")
                got.append((pairs.cpu().numpy(), count.cpu().numpy()))
            for pairs, count in got:
                assert count[0] == len(want), (Na, Nb, fill)
                assert np.array_equal(count[1:], np.full(PAD, rc.SENT_I))
                assert np.array_equal(pairs[:len(want)], want), (Na, Nb, fill)
                assert np.array_equal(pairs[len(want):], np.full((Na + PAD - len(want), 2), rc.SENT_I)), (Na, Nb, fill)


# ---- d3f_ransac_hypotheses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.RS_CASES))
def test_ransac_hypotheses(device, name):
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    case = rc.RS_CASES[name]
    ref = rc.rs_reference(case)
    src, tgt, nn = rc.rs_data(case.data)
    Ns, Nt, H = len(src), len(tgt), rc.RS_H
    for h in (0, 1, 77, H - 1):
        for d in range(case.n):
            assert lib.d3f_ransac_draw(case.seed, case.it0 + h, d, Ns) == onp.draw(case.seed, case.it0 + h, d, Ns)
    st, tt, nnt = _t(src, device), _t(tgt, device), _t(nn, device)
    T = torch.full((H + PAD, 12), float(rc.SENT_F), dtype=torch.float32, device=device)
    valid = torch.full((H + PAD,), 0xA5, dtype=torch.uint8, device=device)
    _lib.check(lib.d3f_ransac_hypotheses(st.data_ptr(), Ns, tt.data_ptr(), Nt, nnt.data_ptr(), case.n, case.edge_similarity,
                                         case.checker_distance, case.seed, case.it0, H, T.data_ptr(), valid.data_ptr(),
                                         ops._stream(device)), "ransac_hypotheses")
    T, valid = T.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(bits(T[H:]), bits(np.full((PAD, 12), rc.SENT_F))) and np.array_equal(valid[H:], np.full(PAD, 0xA5, np.uint8))
    T, valid = T[:H], valid[:H]
    assert np.isin(valid, (0, 1)).all()
    stage = ref["stage"]
    fitted = stage >= rc.DISTANCE
    # a failed sample (repeat, no match, edge checker): not valid, and the identity bit for bit
    assert not valid[~fitted].any()
    assert np.array_equal(bits(T[~fitted]), bits(np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (int((~fitted).sum()), 1))))
    if case.all_repeat:
        assert not fitted.any()
        return
    # every hypothesis whose sample passed, whatever the distance checker says and however ill-conditioned
    M = T[fitted].astype(np.float64).reshape(-1, 3, 4)
    R, t = M[:, :, :3], M[:, :, 3]
    Mo = ref["T"][fitted].reshape(-1, 3, 4)
    S, ms, mt, scale = ref["S"][fitted], ref["ms"][fitted], ref["mt"][fitted], ref["scale"][fitted]
    ortho = np.abs(np.einsum("hka,hkb->hab", R, R) - np.eye(3)).max()
    print("%s: |RtR - I| %.2e" % (name, ortho))
    assert ortho <= 1e-6
    assert (np.linalg.det(R) > 0).all()
    obj, obj_o = np.einsum("hab,hba->h", R, S), np.einsum("hab,hba->h", Mo[:, :, :3], S)
    print("  objective shortfall %.2e of the allowance" % float(((obj_o - obj) / (8 * 2.0 ** -24 * scale)).max()))
    assert (obj >= obj_o - 8 * 2.0 ** -24 * scale).all()
    t_err = np.abs(t - (mt - np.einsum("hab,hb->ha", R, ms))).max(1)
    assert (t_err <= 2.0 ** -23 * (1 + np.abs(mt).max(1) + 3 * np.abs(ms).max(1))).all()
    # a unique rotation: the oracle's entries to fp32, or the neighbouring fp32 number; the flag
    well = ref["relgap"][fitted] >= rc.RS_RELGAP
    want = ref["T"][fitted].astype(np.float32)
    near = (T[fitted] == want) | (T[fitted] == np.nextafter(want, np.float32(np.inf))) | (T[fitted] == np.nextafter(want, np.float32(-np.inf)))
    print("  entries equal to the rounded oracle %.4f, neighbours %.4f" % ((T[fitted] == want)[well].mean(), near[well].mean() - (T[fitted] == want)[well].mean()))
    assert near[well].all(), np.nonzero(~near.all(1) & well)[0][:5]
    ok = (stage[fitted] == rc.OK).astype(np.uint8)
    assert np.array_equal(valid[fitted][well], ok[well])
    if not case.checker_distance > 0:
        assert valid[fitted].all()                                             # nothing left that could reject a fitted sample
    assert valid.sum() > 5


# ---- d3f_neighbor_grid_score -------------------------------------------------------------------------------------------------------
GARBAGE_I, GARBAGE_L = 0x5A5A5A5A, -3


def _score(dev, tgt, src, T, radius, want_nearest=True):
    """-> (count i32[V + PAD], sumd2 i64[V + PAD], nearest i32[Ns + PAD] or None): one d3f_neighbor_grid_score call on a grid built
    at the scoring radius, count / sumd2 starting from garbage"""
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    Nt, Ns, V = len(tgt), len(src), len(T)
    tt, st, Tt = _t(tgt, dev), _t(src, dev), _t(T, dev)
    grid = ops.NeighborGrid(tt, ops.as_lens([Nt], dev), float(radius))
    count = torch.full((V + PAD,), GARBAGE_I, dtype=torch.int32, device=dev)
    sumd2 = torch.full((V + PAD,), GARBAGE_L, dtype=torch.int64, device=dev)
    nearest = torch.full((Ns + PAD,), int(rc.SENT_I), dtype=torch.int32, device=dev) if want_nearest else None
    _lib.check(lib.d3f_neighbor_grid_score(grid.mem.data_ptr(), grid.nbytes, Nt, st.data_ptr() if Ns else None, Ns, Tt.data_ptr(), V,
                                           float(radius), count.data_ptr(), sumd2.data_ptr(), nearest.data_ptr() if want_nearest else None,
                                           ops._stream(dev)), "neighbor_grid_score")
    count, sumd2 = count.cpu().numpy(), sumd2.cpu().numpy()
    assert np.array_equal(count[V:], np.full(PAD, GARBAGE_I, np.int32)) and np.array_equal(sumd2[V:], np.full(PAD, GARBAGE_L, np.int64))
    if want_nearest:
        nearest = nearest.cpu().numpy()
        assert np.array_equal(nearest[Ns:], np.full(PAD, rc.SENT_I))
        nearest = nearest[:Ns]
    return count[:V], sumd2[:V], nearest


def test_grid_score_exact(device):
    """Lattice inputs: every fp32 operation of the kernel is exact, so count, nearest and sumd2 equal the integer restatement."""
    c = rc.sc_exact()
    want_count, want_sum, want_near, D = rc.sc_exact_expected(c)
    count, sumd2, nearest = _score(device, c["tgt"], c["src"], c["T"], c["radius"])
    assert np.array_equal(count, want_count) and [int(x) for x in sumd2] == want_sum
    assert np.array_equal(nearest, want_near)
    for nm, row in c["planted"].items():
        assert nearest[row] == want_near[row], nm
    count2, sumd22, _ = _score(device, c["tgt"], c["src"], c["T"], c["radius"], want_nearest=False)
    assert np.array_equal(count2, want_count) and np.array_equal(sumd22, sumd2)
    for v in range(len(c["T"])):                                               # each hypothesis alone: `nearest` under every transform
        cv, sv, nv = _score(device, c["tgt"], c["src"], c["T"][v:v + 1], c["radius"])
        best, j = D[v].min(1), D[v].argmin(1)
        assert cv[0] == want_count[v] and int(sv[0]) == want_sum[v] and np.array_equal(nv, np.where(best < rc.SC_R_INT ** 2, j, -1)), v


SC_PARAMS = [(Nt, Ns, V) for Nt in rc.SC_NT for Ns in rc.SC_NS for V in rc.SC_V]


@pytest.mark.parametrize("Nt,Ns,V", SC_PARAMS)
def test_grid_score_random(device, Nt, Ns, V):
    """Room-surface inputs whose every decision clears its threshold by 8 x the fp32 error (asserted on the CPU): count and nearest
    equal the float64 brute force; |sumd2 / 2^32 - sum d2| <= count (2 r eps_p + 4 2^-24 r^2 + 2^-32)."""
    c = rc.sc_random(Nt, Ns, V)
    br, r = c["brute"], c["radius"]
    inl = br["b1"] < br["r2"][0]
    want_count = inl.sum(1)
    want_sum = np.where(inl, br["b1"], 0.0).sum(1)
    for want_nearest in (True, False):
        count, sumd2, nearest = _score(device, c["tgt"], c["src"], c["T"], r, want_nearest)
        assert np.array_equal(count, want_count)
        if want_nearest:
            assert np.array_equal(nearest, np.where(inl[0], br["j1"][0], -1) if Ns else np.zeros(0, np.int64))
        assert (sumd2 >= 0).all()
        err = np.abs(sumd2.astype(np.float64) / 2.0 ** 32 - want_sum)
        assert (err <= rc.sc_sumd2_tol(want_count, r, rc.sc_eps_p(c["src"], c["T"]))).all()
    for nm, v in c["special"].items():
        if nm.startswith("far"):
            assert count[v] == 0 and sumd2[v] == 0
