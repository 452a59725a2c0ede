"""Host-only part of tests/test_gpu_registration_branches.py: the builders of oracle/registration_cases.py are seeded and shaped as
stated, and for EVERY case of the GPU file the statements its assertions rest on hold in float64 / integers alone -- the tile shapes
the descriptor cases mean to run (a mirror of the launch arithmetic), the share of rows whose argmin fp32 rounding may move (at most
1 % per case), the share of RANSAC samples whose rotation is not unique (at most 2 % per case), the distance of every checker
decision from its threshold, the planted ties / on-the-sphere points of the exact scoring case, and the 8 x margins of the random
scoring cases.  The two measured shares are printed (pytest -s)."""
import numpy as np
import pytest

import matching_np as mnp
from conftest import bits
from oracle import registration_cases as rc
from oracle import registration_np as onp


# ---- d3f_feature_nn ----------------------------------------------------------------------------------------------------------------
def test_builders_are_seeded():
    for f in (lambda: rc.nn_data(32, 257, 129), lambda: rc.nn_data(32, 257, 129, 1e3), lambda: rc.nn_tie_data(16)[:2],
              lambda: rc.nn_nofinite_data(64), lambda: rc.mm_case(1025, 2050, "invalid"), lambda: rc.pair(3, n=300)[:4]):
        for a, b in zip(f(), f()):
            assert np.array_equal(bits(a), bits(b), equal_nan=a.dtype != np.float32)
    import test_gpu_registration as old
    for a, b in zip(rc.pair(3, n=300), old._pair(3, n=300)):
        assert np.array_equal(a, b)
    A, A3 = rc.nn_data(32, 50, 60)[0], rc.nn_data(32, 50, 60, 1e3)[0]
    assert np.array_equal(A3, A * np.float32(1e3)) and abs(np.linalg.norm(A[7].astype(np.float64)) - 1) < 1e-6


def test_nn_launch_mirror_gives_the_intended_tiles():
    for (Na, Nb), (bx, by, per, last) in rc.NN_INTENT.items():
        gx, gy, gper, splits = rc.nn_launch(Na, Nb)
        assert (gx, gy, gper, splits[-1][1] - splits[-1][0]) == (bx, by, per, last), (Na, Nb)
        assert splits[0][0] == 0 and splits[-1][1] == Nb and all(a[1] == b[0] for a, b in zip(splits, splits[1:]))
    # (256, 128): a split that ends exactly on a full tile; (3, 20000 / 20001): one tile per split, the last one ragged;
    # (700, 1025): 114-row splits (one ragged tile each) and rows 700..767 of the last row block past Na
    assert rc.nn_launch(3, 20000)[2] == rc.NN_TILE and rc.nn_launch(700, 1025)[2] < rc.NN_TILE
    _, by, per, _ = rc.nn_launch(300, 600)                                     # the tie case: the copies lie in different splits
    assert by == 5 and per == 120 and all(j // per != (j + 300) // per for j in range(300))
    _, by, per, _ = rc.nn_launch(260, 300)                                     # the no-finite-distance case: two blocks, three splits
    assert by == 3 and per == 100 and sorted(rc.NN_NOFINITE_ROWS)[1] < 256 <= sorted(rc.NN_NOFINITE_ROWS)[2]


NN_PARAMS = [(C, s, 1.0) for C in rc.NN_WIDTHS for s in rc.NN_SHAPES] + [(32, s, 1e3) for s in rc.NN_SHAPES]


@pytest.mark.parametrize("C,shape,scale", NN_PARAMS, ids=["%d-%dx%d-%g" % (C, s[0], s[1], k) for C, s, k in NN_PARAMS])
def test_nn_case_has_few_ambiguous_rows(C, shape, scale):
    A, B = rc.nn_data(C, *shape, scale=scale)
    ref = rc.nn_reference(A, B, C, mnp.d2_f64)
    n = len(A)
    share = float((~ref["sure"]).mean()) if n else 0.0
    print("feature_nn C=%d %dx%d scale %g: ambiguous-argmin rows %d of %d (%.3f %%)" % (C, shape[0], shape[1], scale, int((~ref["sure"]).sum()), n, 100 * share))
    assert share <= 0.01
    assert not ref["sliver"].any()                    # no row sits between twice the bound at the minimum and the sum of both bounds
    if n and len(B):
        chain = mnp.d2_f32_chain(A, B).astype(np.float64)
        ratio = np.abs(chain - ref["D"]) / rc.nn_bound(C, ref["D"])
        print("  fp32 chain on the CPU: %.3f of the bound" % ratio.max())
        assert ratio.max() <= 1.0                     # the bound holds for a straight fp32 evaluation of the chain
        assert np.array_equal(chain.argmin(1)[ref["sure"]], ref["idx"][ref["sure"]])


@pytest.mark.parametrize("C", rc.NN_WIDTHS)
def test_nn_tie_and_no_finite_cases(C):
    A, B, want = rc.nn_tie_data(C)
    ref = rc.nn_reference(A, B, C, mnp.d2_f64)
    assert np.array_equal(ref["idx"], want)
    assert (ref["d2"] == 0).all() and (ref["d2_2"] == 0).all()                 # bit-equal copies: only the index decides
    zeros = (ref["D"] == 0)
    assert set(zeros.sum(1).tolist()) == {2, 4} and (zeros.sum(1) == 4).sum() == 60
    assert np.array_equal(zeros.argmax(1), want)                               # the first of the equal rows
    assert np.where(zeros, np.inf, ref["D"]).min() > 0.1                       # nothing else is near
    _, by, per, _ = rc.nn_launch(300, 600)
    four = np.nonzero(zeros.sum(1) == 4)[0]
    cols = np.stack([np.nonzero(zeros[i])[0] for i in four])                   # two neighbours in split 0, two in a later split
    assert (cols[:, 1] == cols[:, 0] + 1).all() and (cols[:, 1] < min(per, rc.NN_TILE)).all() and (cols[:, 2] // per > 0).all()
    A, B = rc.nn_nofinite_data(C)
    with np.errstate(invalid="ignore", over="ignore"):
        chain = mnp.d2_f32_chain(A, B)
    bad = sorted(rc.NN_NOFINITE_ROWS)
    assert not (chain[bad] < rc.FLT_MAX).any()                                 # NaN or +inf in every column
    assert not (chain[:, rc.NN_NOFINITE_NAN_COLUMN] < rc.FLT_MAX).any()
    ok = np.setdiff1d(np.arange(len(A)), bad)
    ref = rc.nn_reference(A, B, C, mnp.d2_f64)
    assert np.isfinite(ref["d2"][ok]).all() and ref["sure"][ok].all() and (ref["idx"][ok] != rc.NN_NOFINITE_NAN_COLUMN).all()
    rec = rc.records(A, C)
    assert rec.shape == (len(A) + 1, C + 4) and np.isnan(rec[:, :3]).all() and np.isnan(rec[:, -1]).all()


# ---- d3f_mutual_matches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Na", rc.MM_NA)
def test_mutual_cases_are_what_they_say(Na):
    for Nb in rc.mm_nb(Na):
        counts = {}
        for fill in rc.MM_FILLS:
            ab, ba = rc.mm_case(Na, Nb, fill)
            assert ab.dtype == np.int32 and ba.dtype == np.int32 and len(ab) == Na and len(ba) == Nb
            want = rc.mm_expected(ab, ba, Nb)
            assert (np.diff(want[:, 0]) > 0).all()
            slow = [(i, int(ab[i])) for i in range(Na) if 0 <= ab[i] < Nb and ba[ab[i]] == i]
            assert want.tolist() == [list(p) for p in slow]
            counts[fill] = len(want)
            if fill == "invalid" and Na >= 1023:
                assert (ab == -1).sum() > Na // 20 and (ab >= Nb).sum() > Na // 20
                if Nb:
                    assert (ab == Nb).any() and (ab == 2 ** 31 - 1).any()
        assert counts["all"] == min(Na, Nb) and counts["none"] == 0
        if min(Na, Nb) >= 1023:
            assert 0.3 * Na < counts["half"] < 0.7 * Na and 0.2 * Na < counts["invalid"] < counts["half"]
        if Nb == Na and Na > 1:
            ab, ba = rc.mm_case(Na, Nb, "all")
            assert np.array_equal(np.sort(ab), np.arange(Na)) and np.array_equal(ba[ab], np.arange(Na))     # a permutation and its inverse
            ab, ba = rc.mm_case(Na, Nb, "none")
            assert np.array_equal(np.sort(ab), np.arange(Na)) and (ba[ab] != np.arange(Na)).all()


# ---- d3f_ransac_hypotheses ---------------------------------------------------------------------------------------------------------
def test_ransac_data_and_trace():
    src, tgt, nn = rc.rs_data("full")
    assert src.shape == (300, 3) and tgt.shape == (300, 3) and nn.min() >= 0 and nn.max() < 300
    assert len(np.unique(nn)) < 300                                            # not injective: target samples can repeat a point
    _, _, bad = rc.rs_data("badnn")
    assert 15 <= (bad == -1).sum() <= 45 and 15 <= (bad == 300).sum() <= 45
    assert len(rc.rs_data("five")[0]) == 5
    # the trace returns what hypothesis() returns, and hypothesis() what it returned before the trace existed (valid nn)
    for it in range(300):
        h = onp.hypothesis(src, tgt, nn, 4, 0.9, 0.05, 12345, it)
        tr = onp.hypothesis_trace(src, tgt, nn, 4, 0.9, 0.05, 12345, it)
        assert (h is None) == (tr["stage"] != "ok")
        if h is not None:
            assert np.array_equal(h[0], tr["R"]) and np.array_equal(h[1], tr["tr"])
            R, t = onp.kabsch(src[tr["si"]].astype(np.float64), tgt[tr["ti"]].astype(np.float64))
            assert np.array_equal(h[0], R) and np.array_equal(h[1], t)
    assert onp.draw((1 << 63) + 11, (1 << 32) + 5, 3, 300) == onp.draw((1 << 63) + 11, (1 << 32) + 5, 3, 300) < 300
    names = {(c.data, c.n) for c in rc.RS_CASES.values()}
    assert {("full", n) for n in (3, 4, 5, 8)} <= names and ("five", 8) in names and ("badnn", 3) in names
    assert {(c.edge_similarity > 0, c.checker_distance > 0) for c in rc.RS_CASES.values() if c.data == "full" and c.n == 8} == \
        {(False, False), (True, False), (False, True), (True, True)}


@pytest.mark.parametrize("name", list(rc.RS_CASES))
def test_ransac_case_caps_and_margins(name):
    case = rc.RS_CASES[name]
    ref = rc.rs_reference(case)
    stage = ref["stage"]
    fitted = stage >= rc.DISTANCE                                              # the sample passed: the fit was reached
    ill = fitted & (ref["relgap"] < rc.RS_RELGAP)
    nfit, nvalid = int(fitted.sum()), int((stage == rc.OK).sum())
    share = ill.sum() / max(nfit, 1)
    print("ransac %s: stages %s, sample-passing %d, valid %d, ill-conditioned %d (%.3f %%), two equal target points %d"
          % (name, np.bincount(stage, minlength=5).tolist(), nfit, nvalid, int(ill.sum()), 100 * share, int(ref["dup_t"].sum())))
    assert share <= 0.02
    if case.all_repeat:
        assert (stage == rc.REPEAT).all() and nvalid == 0
        return
    assert nvalid > 5
    if case.data == "five":
        assert (stage == rc.REPEAT).mean() > 0.7                               # most draws repeat
    if case.data == "badnn":
        assert (stage == rc.NO_MATCH).sum() > 100
    if case.edge_similarity > 0:
        e = ref["edge"][~np.isnan(ref["edge"])]
        assert len(e) and (np.abs(e - case.edge_similarity) > 1e-9 * case.edge_similarity).all()
        assert (stage == rc.EDGE).any()
    else:
        assert np.isnan(ref["edge"]).all() and not (stage == rc.EDGE).any()
    well = fitted & ~ill
    if case.checker_distance > 0:
        d = ref["dist"][well]
        assert (np.abs(d - case.checker_distance) > 1e-9 * case.checker_distance).all()
    else:
        assert not (stage == rc.DISTANCE).any()
    # Horn's eigenvector (numpy.linalg.eigh) and the SVD agree where the rotation is unique
    worst = 0.0
    for h in np.nonzero(well)[0]:
        worst = max(worst, float(np.abs(rc.horn_rotation(ref["S"][h]) - ref["T"][h].reshape(3, 4)[:, :3]).max()))
    print("  eigh form of Horn against kabsch: %.2e" % worst)
    assert worst <= 5e-13
    # the oracle's rotation is a maximiser of tr(R S), a rotation, and its translation maps the means
    for h in np.nonzero(fitted)[0][:50]:
        M = ref["T"][h].reshape(3, 4)
        assert abs(np.linalg.det(M[:, :3]) - 1) < 1e-12 and np.abs(M[:, 3] - (ref["mt"][h] - M[:, :3] @ ref["ms"][h])).max() < 1e-12


def test_ransac_cases_reach_every_stage():
    seen_dup = 0
    stages = set()
    for c in rc.RS_CASES.values():
        ref = rc.rs_reference(c)
        stages |= set(np.unique(ref["stage"]).tolist())
        seen_dup += int(ref["dup_t"].sum())
    assert stages == {rc.REPEAT, rc.NO_MATCH, rc.EDGE, rc.DISTANCE, rc.OK} and seen_dup > 0


# ---- d3f_neighbor_grid_score -------------------------------------------------------------------------------------------------------
def test_exact_scoring_case():
    c = rc.sc_exact()
    for a, i in ((c["src"], c["src_i"]), (c["tgt"], c["tgt_i"])):
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64) * 64, i) and i.min() >= 0 and i.max() < 256
    T = c["T"].reshape(-1, 3, 4).astype(np.float64)
    assert np.array_equal(T[:, :, :3], c["P"]) and np.array_equal(T[:, :, 3] * 64, c["tau"])
    assert not np.array_equal(c["P"][0], np.eye(3)) and np.array_equal(c["P"][1], np.eye(3)) and (np.abs(c["P"]).sum(2) == 1).all()
    assert c["radius"] * 64 == rc.SC_R_INT and np.float32(c["radius"]) * np.float32(c["radius"]) == (rc.SC_R_INT / 64) ** 2
    count, sumd2, near, D = rc.sc_exact_expected(c)
    assert D.max() < 2 ** 24                                                   # every fp32 intermediate is an exact integer
    assert len(c["src"]) * len(c["T"]) > 256                                   # more than one workgroup
    assert (count[:3] > 20).all() and count[0] != count[1]
    r2, p = rc.SC_R_INT ** 2, c["planted"]
    for nm in ("tie_x", "tie_z", "tie_skew"):
        d = np.sort(D[0, p[nm]])
        two = np.nonzero(D[0, p[nm]] == d[0])[0]
        assert d[0] == d[1] < r2 and d[2] > d[1] and len(two) == 2 and near[p[nm]] == two.min()
    for nm in ("sphere_68", "sphere_10"):
        assert D[0, p[nm]].min() == r2 and near[p[nm]] == -1                   # exactly on the sphere: no inlier
    assert D[0, p["inside"]].min() == 81 and near[p["inside"]] >= 0
    assert (D[0].min(1) == 0).any()                                            # a moved source point ON a target


SC_PARAMS = [(Nt, Ns, V) for Nt in rc.SC_NT for Ns in rc.SC_NS for V in rc.SC_V]


@pytest.mark.parametrize("Nt,Ns,V", SC_PARAMS)
def test_random_scoring_case_margins(Nt, Ns, V):
    c = rc.sc_random(Nt, Ns, V)
    br = c["brute"]
    assert c["src"].shape == (Ns, 3) and c["tgt"].shape == (Nt, 3) and c["T"].shape == (V, 12) and c["T"].dtype == np.float32
    assert rc.sc_margins(br).all()
    if Ns <= 257:                                                              # the kept rows' figures are those of a fresh brute force
        again = rc.sc_brute(c["src"], c["tgt"], c["T"], c["radius"])
        assert all(np.array_equal(again[k], br[k]) for k in ("b1", "b2", "j1", "err_rows")) and again["err"] == br["err"]
    assert abs(br["r2"][0] - br["r2"][1]) < rc.SC_FACTOR * max(br["err"], 1e-12) or Ns == 0
    if Ns == 0:
        return
    inl = br["b1"] < br["r2"][0]
    assert br["err"] < 1e-6
    if Ns >= 257:
        assert 0.3 < inl[0].mean() < 0.9
    if Ns >= 257 and Nt == 3000:
        assert ((br["b2"] < br["r2"][0]).sum() > 50)                           # several targets inside the radius
    M = c["T"].reshape(V, 3, 4).astype(np.float64)
    for nm, v in c["special"].items():
        axis = "xyz".index(nm[-1])
        moved = c["src"].astype(np.float64) @ M[v, :, :3].T + M[v, :, 3]
        hi = c["tgt"].astype(np.float64).max(0)
        if nm.startswith("far"):
            far = np.minimum(np.abs(moved[:, axis] - hi[axis]), np.abs(moved[:, axis] - c["lo"][axis]))
            assert not inl[v].any() and (far > 60 * c["radius"]).all()         # tens of cells outside: the clamp to -2 / dims + 1
        else:
            assert (moved[:, axis] < c["lo"][axis]).all() and (moved[:, axis] > c["lo"][axis] - c["radius"]).all()      # cell -1
            if Ns >= 257 and Nt == 3000:
                assert inl[v].any()                                            # and cell 0 is still searched
    assert ("far_x" in c["special"]) == (V >= 2) and ("flat_z" in c["special"]) == (V == 37)
