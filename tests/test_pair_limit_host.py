"""The calls of tests/test_gpu_pair_limits.py (tests/pair_limit_cases.py), the part that needs no GPU: the arithmetic that makes a
workgroup's second pair the successor kind of its first, that every succession the kernels' comments depend on occurs and is what its
name says, that every input keeps the margins of its restatement (so that fp32 and float64 take the same decisions and equality is a
fair demand), and that the restatements' results differ between successive kinds -- a workgroup that repeated its first pair, or left
its second one out, would be seen in every output.  The six tests take 0.7 s together on a CPU."""
import numpy as np
import pytest

import loss_grad_np as lg
import matching_np as mnp
import overlap_np as onp
import pair_limit_cases as plc
import repeatability_np as rnp
import validation_np as vnp


@pytest.fixture(scope="module")
def kp():
    return plc.keypoint_kinds()


@pytest.fixture(scope="module")
def ov():
    return plc.overlap_kinds()


@pytest.fixture(scope="module")
def vp():
    return plc.validation_kinds()


def test_the_second_pair_of_a_workgroup_is_the_successor_kind():
    assert plc.M == 7 and plc.CAP == 65535 and plc.CAP % plc.M == 1 and plc.P_BIG == 65535 + 301
    assert 4096 < plc.P_MID < plc.CAP
    succ = plc.successions()
    assert len(succ) == 301 and all(b == (a + 1) % 7 for a, b in succ)
    for k in range(7):
        assert succ.count((k, (k + 1) % 7)) >= 43
    for table in (plc.SUCCESSIONS_KP, plc.SUCCESSIONS_OV, plc.SUCCESSIONS_VP):
        for name, pair in table.items():
            assert pair in succ, name
    for P in (7, plc.P_MID):                                           # below the cap no workgroup runs a second pair
        assert plc.successions(P) == []
    assert np.array_equal(plc.cyclic(np.arange(7), 17), np.arange(17) % 7)


def _kp_rows(kinds, k, count):
    n = lambda b: min(len(kinds["blocks"][b]), count) if 0 <= b < len(kinds["blocks"]) else 0
    a, b = kinds["pairs"][k]
    return n(a), n(b)


def test_keypoint_kinds_are_what_their_names_say(kp):
    blocks, pairs = kp["blocks"], kp["pairs"]
    assert [len(b) for b in blocks] == list(plc.KP_ROWS) and all(b.shape[1] == plc.KP_C + 4 and b.dtype == np.float32 for b in blocks)
    assert len(blocks) <= 8 and max(plc.KP_ROWS) <= plc.KP_K and plc.KP_COUNTS == (5, 300)
    assert max(plc.KP_ROWS) > 256 and 0 < plc.KP_ROWS[2] <= 256        # the second 256-rank tile has queries for some pairs only
    top = plc.KP_COUNTS[-1]
    for k in plc.KP_FULL:
        assert max(_kp_rows(kp, k, top)) > 256 and min(_kp_rows(kp, k, top)) >= plc.RANSAC["ransac_n"]
    # direction 0 of the nearest kernel (queries = the source): its second tile works for kinds 0 and 2 and has nothing to do in between
    assert [_kp_rows(kp, k, top)[0] > 256 for k in (0, 1, 2)] == [True, False, True] and plc.KP_SHORT == (1,)
    assert _kp_rows(kp, 1, top) == (40, 300) and _kp_rows(kp, 1, plc.KP_COUNTS[0]) == (5, 5)
    assert sorted(pairs[plc.KP_OUTSIDE[0]].tolist()) == [-1, len(blocks)]                 # both -1 and n_blocks
    assert _kp_rows(kp, plc.KP_ONE_ROW[0], top) == (1, 1) and _kp_rows(kp, plc.KP_EMPTY[0], top) == (300, 0)
    for k in range(7):
        none = all(min(_kp_rows(kp, k, c)) < plc.RANSAC["ransac_n"] for c in plc.KP_COUNTS)
        assert none == (k in plc.KP_NO_HYPOTHESES), k
    assert plc.RANSAC["max_validation"] % 16 != 0 and 100 <= plc.RANSAC["max_iteration"] <= 1000
    for b in blocks:                                                   # ascending score, unit descriptors
        assert np.all(np.diff(b[:, -1]) >= 0) and np.allclose(np.linalg.norm(b[:, 3:3 + plc.KP_C], axis=1), 1, atol=1e-6)


def test_keypoint_kinds_keep_the_margins_and_successive_kinds_differ(kp):
    blocks, pairs, gts = kp["blocks"], [tuple(p) for p in kp["pairs"].tolist()], kp["gts"]
    m = mnp.margins(blocks, pairs, gts, plc.KP_COUNTS, plc.KP_THRESHOLD, C=plc.KP_C)
    assert mnp.margins_ok(m), m
    mc, gi = mnp.match_counts(blocks, pairs, gts, plc.KP_COUNTS, plc.KP_THRESHOLD, C=plc.KP_C)
    for k in range(7):
        nxt = (k + 1) % 7
        assert not np.array_equal(mc[k], mc[nxt]), (k, mc[k], mc[nxt])
    assert mc[0, 1] > 100 and gi[0, 1] > 100 and mc[4].tolist() == [1, 1] and gi[4].tolist() == [1, 1]
    assert not mc[3].any() and not mc[5].any() and mc[6, 1] > 10 and gi[6, 1] > 10
    # repeatability: the point distances stay away from the threshold, and successive kinds differ there too
    real = [k for k in range(7) if k not in plc.KP_OUTSIDE]
    band = rnp.band(blocks, [pairs[k] for k in real], [gts[k] for k in real], plc.KP_COUNTS, plc.KP_THRESHOLD)
    assert band > 1e-6, band                                           # float64 against a threshold of 0.1: far beyond its rounding
    rep = rnp.repeat_counts(blocks, pairs, gts, plc.KP_COUNTS, plc.KP_THRESHOLD)
    for k in range(7):
        assert not np.array_equal(rep[k], rep[(k + 1) % 7]), k
    assert rep[0, 1] > 100 and rep[4].tolist() == [1, 1]


def test_overlap_kinds(ov):
    clouds, pairs = ov["clouds"], [tuple(p) for p in ov["pairs"].tolist()]
    assert [len(c) for c in clouds] == [300, 257, 5, 0, 300] and plc.OV_LD < 257
    by = {p: k for k, p in enumerate(pairs)}
    assert pairs[0] == (1, 0) and pairs[1] == (2, 0) and len(clouds[1]) > 256 > len(clouds[2])      # a long source before a short one
    a, b = clouds[4], clouds[0]                                        # disjoint boxes, even grown by the threshold
    assert (a.min(0) > b.max(0) + 1.0).all()
    assert by[(3, 0)] == 4 and by[(-1, 0)] == 6
    for s, t in pairs:
        if 0 <= s < 5 and 0 <= t < 5 and len(clouds[s]) and len(clouds[t]):
            m = onp.margins(clouds[s], clouds[t], plc.OV_THRESHOLD)
            assert min(m) >= onp.BAND, ((s, t), m)
    count, near = onp.overlap(clouds, pairs, plc.OV_THRESHOLD, ld=plc.OV_LD)
    assert count.tolist()[2] == 0 and count[4] == 0 and count[6] == -1 and min(count[0], count[1], count[3], count[5]) > 0
    assert count[0] > 64 and (near[0] >= 0).sum() < count[0]           # matches beyond the row: the row is shorter than the source
    for k in range(7):
        nxt = (k + 1) % 7
        assert count[k] != count[nxt] and (not np.array_equal(near[k], near[nxt]) or min(count[k], count[nxt]) <= 0), k


def test_training_kinds(vp):
    assert plc.VP_LD == 70 and plc.VP_C == 16 and vp["anc"].shape == (7, 70) and vp["n"].tolist() == list(plc.VP_N)
    assert [n > 64 for n in plc.VP_N[:3]] == [True, False, True] and plc.VP_N[6] <= 64 < plc.VP_N[0]   # the second tile: work, none, work
    assert plc.VP_N[5] > plc.VP_LD and 0 < 2 * plc.VP_N[3] < plc.VP_KEYPTS_NUM <= 2 * plc.VP_N[1]
    sig = []
    for k, (f, s, x, ai, pi) in enumerate(vp["cases"]):
        lo, hi = vp["row0"][k], vp["row0"][k + 1]
        assert hi - lo == len(f) and np.array_equal(vp["f"][lo:hi], f) and np.array_equal(vp["x"][lo:hi], x)
        n = plc.VP_N[k]
        if k in plc.VP_EVALUATED:
            assert len(ai) == n and ai.max() < len(f) and pi.max() < len(f)
            rows, kd = vp["planted"][k]
            vnp.margins(f, x, ai, pi, plc.VP_RADIUS, plc.VP_C, planted_rows=rows, planted_kd=kd)
            lg.margins(f, x, ai, pi, plc.VP_RADIUS, plc.VP_C, planted_rows=rows, planted_kd=kd)
            want = vnp.figures(f, s, x, ai, pi, plc.VP_RADIUS, plc.VP_KEYPTS_NUM)
            assert not want["skipped"]
            sig.append(tuple(float(want[name]) for name in ("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg")) + (0, n))
            for loss in ("circle_loss", "desc_loss"):
                g = lg.gradients(f, s, x, ai, pi, plc.VP_RADIUS, plc.VP_KEYPTS_NUM, 1.0, loss=loss)
                assert not g["skipped"] and np.abs(g["features"]).max() > 1e-3 and np.abs(g["scores"]).max() > 1e-4
                named = np.zeros(len(f), bool)
                named[ai] = named[pi] = True
                assert not named.all() and not g["features"][~named].any()          # rows no list names: zeros
        else:
            status = plc.VP_STATUS[k]
            bad = len(ai) and (max(ai.max(), pi.max()) >= len(f))
            assert (status == 1) == bool(bad) and (status == 2) == (n > plc.VP_LD)
            assert status or n == 0 or 2 * n < plc.VP_KEYPTS_NUM
            sig.append(tuple(vnp.SKIP) + (status, n))
    i, j = plc.VP_DUPLICATE                                              # a row named twice, by the same index pair
    c0 = vp["cases"][0]
    assert c0[3][i] == c0[3][j] and c0[4][i] == c0[4][j] and i < 64 and j < 64
    assert vp["cases"][2][4][66] == len(vp["cases"][2][0])              # the bad index sits in the second tile
    for k in range(7):
        assert sig[k] != sig[(k + 1) % 7], k


def test_the_cyclic_training_call(vp):
    P = 17
    f, s, x, anc, pos, n, row0 = plc.validation_call(vp, P)
    R = int(vp["row0"][-1])
    assert len(row0) == P + 1 and row0[-1] <= len(f) == 3 * R and n.tolist() == [plc.VP_N[p % 7] for p in range(P)]
    for p in range(P):
        lo, hi = vp["row0"][p % 7], vp["row0"][p % 7 + 1]
        assert row0[p] == (p // 7) * R + lo and row0[p + 1] - row0[p] == hi - lo
        assert np.array_equal(f[row0[p]:row0[p + 1]], vp["f"][lo:hi]) and np.array_equal(anc[p], vp["anc"][p % 7])
    reps = -(-plc.P_BIG // 7)
    assert reps * R * (plc.VP_C + 1) < 2 ** 31                            # rows of the big call
