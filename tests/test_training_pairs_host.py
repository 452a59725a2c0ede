"""The definition of d3f_training_pairs on the CPU: tests/training_pairs_np.py (the header's text in numpy) against a float64 brute force,
scipy's KD-tree, the reference's own rotate() and the statistics its sampler must have.  No GPU; tests/test_gpu_training_pairs.py ties
the device to the restatement integer for integer.

Open3D is not available here: the order of get_matching_indices' list inside runs of equal distance, and its voxel grid, stay unpinned.
"""
import os

import numpy as np
import pytest

import training_pairs_cases as tc
import training_pairs_np as tp
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "training_pairs.npz"))


def _fixture_pairs(golden):
    general = (golden["general_anchor"], golden["general_positive"], golden["general_trans"])
    return [(p, tc.RADIUS) for p in tc.three_pairs() + [tc.small_pair(), tc.ends_pair(), tc.cluster_pair(), tc.apart_pair()]] + \
        [(general, float(golden["general_radius"]))]


def test_host_draw_is_the_restatements(golden):
    from d3feat_amd import training_pairs as T
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, step, counter = (int(v) for v in rng.integers(0, 2 ** 63, 3))
        pair, stream = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 256))
        assert T.training_draw(seed, step, pair, stream, counter) == int(tp.draw(seed, step, pair, stream, counter))
    assert T.training_draw(2 ** 64 - 1, 2 ** 64 - 1, 0, 8, 2 ** 64 - 1) == int(tp.draw(2 ** 64 - 1, 2 ** 64 - 1, 0, 8, 2 ** 64 - 1))
    assert (T.STREAM_NOISE, T.STREAM_ROTATION, T.STREAM_SCALE, T.STREAM_SHIFT, T.STREAM_SAMPLE) == \
        (tp.STREAM_NOISE, tp.STREAM_ROTATION, tp.STREAM_SCALE, tp.STREAM_SHIFT, tp.STREAM_SAMPLE)
    assert T.AUGMENT_KITTI == tp.AUGMENT_KITTI and T.AUGMENT_3DMATCH == tp.AUGMENT_3DMATCH


def test_matches_equal_a_float64_brute_force_and_a_kd_tree(golden):
    from scipy.spatial import cKDTree
    assert int(golden["general_excluded_rows"]) == 0 and golden["general_margins"].min() > 1e-4
    ties = strict = 0
    for (a, b, T), radius in _fixture_pairs(golden):
        lst, start = tp.matches(a, b, T, radius)
        assert start[-1] == len(lst) and (np.diff(lst[:, 0]) >= 0).all()
        want = tp.matches_f64(a, b, T, radius)
        assert set(map(tuple, lst.tolist())) == want and len(lst) == len(want)
        # the moved anchor in float64; the radius shrunk by less than any margin of the fixtures: query_ball_point is not strict
        q = a.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
        ball = cKDTree(b.astype(np.float64)).query_ball_point(q, float(radius) * (1 - 1e-9))
        assert {(i, j) for i, js in enumerate(ball) for j in js} == want
        d2 = tp.d2_f32(tp.move(T, a), b)
        for i in range(len(a)):
            js = lst[start[i]:start[i + 1], 1]
            keys = list(zip(d2[i, js].tolist(), js.tolist()))
            assert keys == sorted(keys)                                   # (d2, j) ascending
            ties += len(js) - len(set(d2[i, js].tolist()))
        strict += int((d2 == np.float32(radius) * np.float32(radius)).sum())
    assert ties > 100 and strict > 0          # the index rule and the strict comparison are exercised by the fixture
    assert tc.margins(golden["general_anchor"], golden["general_positive"], golden["general_trans"], float(golden["general_radius"])) == \
        tuple(golden["general_margins"].tolist())


def test_fixture_reaches_the_cases_the_device_test_names():
    a, b, T = tc.cluster_pair()
    _, start = tp.matches(a, b, T, tc.RADIUS)
    assert np.diff(start).max() >= 70
    a, b, T = tc.ends_pair()
    _, start = tp.matches(a, b, T, tc.RADIUS)
    n = np.diff(start)
    assert n[0] == 0 and n[-1] == 0 and n[30] == 0 and n.sum() > 64
    a, b, T = tc.apart_pair()
    assert len(tp.matches(a, b, T, tc.RADIUS)[0]) == 0
    assert max(len(a) for a, _, _ in tc.three_pairs()) == 1100


def test_rotation_is_the_references_rotate(golden):
    """rotate() itself, unmodified, was fed the definition's draws (tools/make_golden_training_pairs.py): the restatement's R applied
    as points @ R gives its result (float32 matmul: the BLAS order is not the header's, hence a few ulp), the transpose does not."""
    pts = golden["rotate_points"]
    for c, (seed, step, pair, side, mode) in enumerate(golden["rotate_cases"].tolist()):
        draws = tp.rotation_draws(seed, step, pair, side, mode)
        assert [a for _, a in draws] == golden["rotate_axis_%d" % c].tolist()
        assert np.array_equal(np.asarray([t for t, _ in draws]), golden["rotate_u_%d" % c] * 2 * np.pi)
        R = tp.cloud_params(seed, step, pair, side, dict(tp.AUGMENT_3DMATCH, augment_rotation=mode))[:9].reshape(3, 3)
        want = golden["rotate_result_%d" % c]
        assert np.abs(pts @ R - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max()
        assert np.abs(pts @ R.T - want).max() > 1e-2
    # the 3DMatch settings leave scale 1 and shift 0: the row pass is then noise and rotation alone
    q = tp.cloud_params(5, 6, 7, 1, tp.AUGMENT_3DMATCH)
    assert q[9] == 1 and not q[10:13].any() and q[15] == 1
    assert np.array_equal(tp.cloud_params(5, 6, 7, 0, dict(tp.AUGMENT_KITTI, augment_rotation=0))[:9], np.eye(3, dtype=np.float32).reshape(9))


def test_augmentation_ranges_and_per_pair_scale():
    A = tp.AUGMENT_KITTI
    scales, shifts = [], []
    for step in range(300):
        qa, qp = tp.cloud_params(3, step, 4, 0, A), tp.cloud_params(3, step, 4, 1, A)
        assert qa[9] == qp[9] and not np.array_equal(qa[10:13], qp[10:13]) and not np.array_equal(qa[:9], qp[:9])
        scales.append(qa[9])
        shifts += [qa[10:13], qp[10:13]]
    scales, shifts = np.asarray(scales), np.asarray(shifts)
    assert 0.8 <= scales.min() < 0.82 and 1.18 < scales.max() < 1.2 and -2 <= shifts.min() < -1.9 and 1.9 < shifts.max() < 2
    rows = np.zeros((500, 3), np.float32)
    ident = np.concatenate([np.eye(3).reshape(9), [1, 0, 0, 0, 0, 0, 0]]).astype(np.float32)
    u = tp.augment_rows(3, 0, 4, 0, 0.01, ident, rows) / np.float32(0.01)        # the noise alone: uniform in [0, 1), not Gaussian
    assert 0 <= u.min() < 0.01 and 0.99 < u.max() < 1.0 and abs(u.mean() - 0.5) < 0.03
    assert not np.array_equal(u, tp.augment_rows(3, 0, 4, 1, 0.01, ident, rows) / np.float32(0.01))


def test_sampler_frequencies():
    """M = 40, keypts_num = 8, 2000 fixed (seed, step): every match's count within 5 standard deviations of 400 (Binomial(2000, 0.2):
    sd 17.9, band +-90), no index twice inside a draw; the with-replacement form likewise."""
    M, k, runs = 40, 8, 2000
    count = np.zeros(M, np.int64)
    for run in range(runs):
        sel = tp.floyd(1000 + run % 50, run // 50, 3, M, k)
        assert len(sel) == k and len(set(sel.tolist())) == k and sel.min() >= 0 and sel.max() < M
        count[sel] += 1
    assert count.sum() == runs * k and np.abs(count - 400).max() <= 90, count
    count = np.zeros(M, np.int64)
    repeats = 0
    for run in range(runs):
        sel = tp.with_replacement(1000 + run % 50, run // 50, 3, M, k)
        assert len(sel) == k and sel.min() >= 0 and sel.max() < M
        repeats += k - len(set(sel.tolist()))
        np.add.at(count, sel, 1)
    assert count.sum() == runs * k and np.abs(count - 400).max() <= 90, count
    assert repeats > 0
    # M == keypts_num returns every match; every draw depends on seed, step and pair
    assert sorted(tp.floyd(1, 2, 3, 8, 8).tolist()) == list(range(8))
    base = tp.floyd(1, 2, 3, 4000, 8).tolist()
    assert base != tp.floyd(2, 2, 3, 4000, 8).tolist() and base != tp.floyd(1, 3, 3, 4000, 8).tolist() and base != tp.floyd(1, 2, 4, 4000, 8).tolist()


def test_restatement_call_conventions():
    pairs = [tc.small_pair(), tc.apart_pair()]
    pts, lens, trans = tc.stack(pairs)
    lst, _ = tp.matches(*pairs[0], tc.RADIUS)
    M = len(lst)
    r = tp.training_pairs(pts, lens, trans, radius=tc.RADIUS, keypts_num=8, min_matches=M, seed=2, step=5)
    assert r["matches"].tolist() == [M, 0] and r["status"].tolist() == [0, tp.FEW_MATCHES | tp.BELOW_KEYPTS] and r["n"].tolist() == [8, 0]
    assert (r["pos_idx"][0] >= lens[0]).all() and (r["pos_idx"][0] < lens[0] + lens[1]).all() and (r["anc_idx"][1] == -1).all()
    got = set(zip(r["anc_idx"][0].tolist(), (r["pos_idx"][0] - lens[0]).tolist()))
    assert len(got) == 8 and got <= tp.matches_f64(*pairs[0], tc.RADIUS)
    assert np.array_equal(r["backup"][:lens[0]], tp.move(trans[0], pts[:lens[0]])) and np.array_equal(r["backup"][lens[0]:lens[0] + lens[1]], pts[lens[0]:lens[0] + lens[1]])
    assert tp.training_pairs(pts, lens, trans, radius=tc.RADIUS, keypts_num=8, min_matches=M + 1, seed=2, step=5)["status"][0] == tp.FEW_MATCHES
    every = tp.training_pairs(pts, lens, trans, radius=tc.RADIUS, keypts_num=M, min_matches=1, seed=2, step=5)
    assert sorted(zip(every["anc_idx"][0].tolist(), (every["pos_idx"][0] - lens[0]).tolist())) == sorted(map(tuple, lst.tolist()))
    # the list form: with replacement from the pair's own rows of the list
    kp, start = tc.keypts_lists([1, 5], [(lens[0], lens[1]), (lens[2], lens[3])])
    r = tp.training_pairs(pts, lens, keypts_pairs=kp, pair_start=start, keypts_num=16, seed=2, step=5, augment=tp.AUGMENT_3DMATCH)
    assert (r["anc_idx"][0] == kp[0, 0]).all() and (r["pos_idx"][0] == kp[0, 1] + lens[0]).all() and r["matches"].tolist() == [1, 5]
    assert set(zip(r["anc_idx"][1].tolist(), (r["pos_idx"][1] - lens[2]).tolist())) <= set(map(tuple, kp[1:].tolist()))
    assert np.array_equal(r["backup"], pts)
