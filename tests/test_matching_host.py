"""Feature matching of every pair at every keypoint count (d3f_match_pairs / registration.match_pairs), the part that needs no GPU: the
entry points are bound, every argument is refused on the host before a launch, the workspace size, the host side of PairMatching and
results.matching_table on hand-made arrays, and the fixture of the reference (tests/golden/matching.npz, tools/make_golden_matching.py):
its recorded margins meet its own rule and the float64 restatement (tests/matching_np.py) reproduces it exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import matching_np as mnp
from conftest import GOLDEN, ROOT

COUNTS = (250, 500, 1000, 2500, 5000)


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "matching.npz"))


def test_entry_points_and_constants(lib):
    from d3feat_amd import _lib
    for name in ("d3f_match_pairs", "d3f_match_pairs_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("D3F_MATCH_KMAX") == define("D3F_TOPK_MAX") == _lib.MATCH_KMAX == _lib.TOPK_MAX == 8192
    assert define("D3F_REPEAT_COUNTS_MAX") == _lib.REPEAT_COUNTS_MAX == 16
    assert define("D3F_PAIRS_KMAX") == 1024                      # register_pairs keeps its limit


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*values)


def _ws_bytes(lib, P, counts, n_counts=None):
    ks = _ints(counts)
    return lib.d3f_match_pairs_workspace_bytes(P, ctypes.addressof(ks), len(counts) if n_counts is None else n_counts)


def _call(lib, P=4, n_blocks=3, K=6000, ld=36, C=32, counts=COUNTS, n_counts=None, thr=0.1, gt=True, gt_inliers=True, null_counts=False,
          ws_bytes=None, null=False):
    """d3f_match_pairs with pointers to a small HOST buffer (or NULL): every call here is refused, or has nothing to do, before a launch."""
    buf = ctypes.create_string_buffer(256)
    ptr = None if null else ctypes.addressof(buf)
    ks = _ints(counts)
    some = ctypes.addressof(buf)
    return lib.d3f_match_pairs(ptr, n_blocks, K, ld, C, ptr, ptr, P, some if gt else None, thr, None if null_counts else ctypes.addressof(ks),
                               len(counts) if n_counts is None else n_counts, ptr, some if gt_inliers else None, ptr,
                               256 if ws_bytes is None else ws_bytes, None)


def test_host_side_argument_checks(lib):
    assert _call(lib, P=-1) == -3 and _call(lib, n_blocks=0) == -3 and _call(lib, K=0) == -3
    assert _call(lib, C=8) == -3 and _call(lib, C=48) == -3 and _call(lib, C=128, ld=200) == -3         # descriptors of 16, 32 or 64 floats
    assert _call(lib, ld=34) == -3                                                                        # ld >= C + 3
    assert _call(lib, counts=(0, 250)) == -3 and _call(lib, counts=(250, 8193)) == -3                     # a count outside 1..8192
    assert _call(lib, counts=(250, 250)) == -3 and _call(lib, counts=(500, 250)) == -3                    # not strictly ascending
    assert _call(lib, counts=(), n_counts=0) == -3 and _call(lib, counts=tuple(range(1, 18))) == -3       # n_counts outside 1..16
    assert _call(lib, null_counts=True) == -3
    assert _call(lib, thr=float("nan")) == -3
    assert _call(lib, gt=False, gt_inliers=True) == -3                                                    # gt_inliers without gt
    assert _call(lib, gt=True, gt_inliers=False) == -3                                                    # and gt without gt_inliers
    assert _call(lib, null=True) == -3                                                                    # valid sizes, P > 0: NULL pointers
    # everything valid but the workspace: 256 bytes, and one byte less than asked for
    need = _ws_bytes(lib, 4, COUNTS)
    assert _call(lib) == -2 and _call(lib, ws_bytes=need - 1) == -2
    assert _call(lib, ld=35) == -2 and _call(lib, C=16, ld=19) == -2 and _call(lib, C=64, ld=67) == -2    # ld = C + 3 is accepted
    assert _call(lib, counts=(1, 8192)) == -2 and _call(lib, counts=tuple(range(1, 17))) == -2            # both ends of the ranges
    assert _call(lib, gt=False, gt_inliers=False) == -2


def test_no_pairs_is_a_no_op(lib):
    assert _call(lib, P=0) == 0
    assert _call(lib, P=0, null=True, gt=False, gt_inliers=False, ws_bytes=0) == 0
    assert _call(lib, P=0, K=20000, counts=(8192,)) == 0                                                  # K itself may exceed every count
    assert _call(lib, P=0, counts=(0,)) == -3                                                             # the sizes are still checked


def test_workspace_bytes(lib):
    total = sum(COUNTS)
    assert total == 9250
    one = _ws_bytes(lib, 1, COUNTS)
    assert 8 * total <= one <= 8 * total + 1024                  # the nearest rank of every row of every count, both directions
    assert 496 * 8 * total <= _ws_bytes(lib, 496, COUNTS) < 38 * 1000 * 1000     # the scene of the issue: about 37 MB
    sizes = [_ws_bytes(lib, P, COUNTS) for P in (0, 1, 2, 3, 100, 496, 4096)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == sizes[1] and sizes[2] > sizes[1]
    assert _ws_bytes(lib, 7, (250,)) <= _ws_bytes(lib, 7, (251,)) < _ws_bytes(lib, 7, (250, 500)) < _ws_bytes(lib, 7, COUNTS)   # (sizes are aligned)
    assert _ws_bytes(lib, 4096, (8192,) ) >= 4096 * 8 * 8192
    assert _ws_bytes(lib, 5000, tuple(range(8177, 8193))) >= 5000 * 8 * sum(range(8177, 8193)) > 2 ** 32   # size_t, not int
    for bad in ((0,), (8193,), (500, 250), tuple(range(1, 18))):
        assert _ws_bytes(lib, 4, bad) == 0
    assert _ws_bytes(lib, -1, COUNTS) == 0 and lib.d3f_match_pairs_workspace_bytes(4, None, 5) == 0


def test_python_validation():
    import torch
    from d3feat_amd import _lib, registration as reg
    assert reg.MATCHING_COUNTS == COUNTS
    kp, count, pairs = torch.zeros(2, 8, 36), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):                 # no CPU path
        reg.match_pairs(kp, count, pairs)


def _result(mutual, inliers, counts):
    """a PairMatching as match_pairs leaves it, on host tensors"""
    import torch
    from d3feat_amd import registration as reg
    mutual = np.asarray(mutual, np.int32)
    res = reg.PairMatching(mutual.shape[0], counts, torch.device("cpu"), inliers is not None)
    res.mutual_count.copy_(torch.from_numpy(mutual))
    if inliers is not None:
        res.gt_inliers.copy_(torch.from_numpy(np.asarray(inliers, np.int32)))
    return res


def test_pair_matching_ratios_and_rows():
    res = _result([[3, 7], [0, 100], [9, 300], [4, 8]], [[1, 2], [0, 5], [0, 100], [4, 8]], (250, 5000))
    assert res.P == 4 and res.num_keypts == (250, 5000)
    r = res.ratios()
    assert r.dtype == np.float64 and r.shape == (4, 2)
    assert np.array_equal(r, np.array([[1 / 3, 2 / 7], [0.0, 0.05], [0.0, 100 / 300], [1.0, 1.0]]))      # no mutual pair: 0.0, not NaN
    rows = res.rows(0, [1, 1, 0, 1])
    assert rows == [[1, 0.33333333, 1], [0, 0.0, 1], [0, 0.0, 0], [4, 1.0, 1]]                            # the 8 decimals of the result file
    rows = res.rows(1, np.array([0, 1, 1, 0], np.int32))
    assert rows == [[0, 0.0, 0], [5, 0.05, 1], [100, 0.33333333, 1], [0, 0.0, 0]]                         # not listed by gt.log: zeros
    assert res.rows(1, np.array([False, True, True, False])) == rows and res.rows(1, (0, 7, 1, 0)) == rows
    assert all(type(a) is int and type(b) is float and type(c) is int for a, b, c in rows)
    for bad in ([1, 1, 1], [[1, 1, 1, 1]], [1.0, 1.0, 0.0, 1.0]):
        with pytest.raises(ValueError):
            res.rows(0, bad)
    with pytest.raises(ValueError):                              # no ground truth was given: no ratios
        _result([[3, 7]], None, (250, 5000)).ratios()


def test_matching_table():
    from d3feat_amd.utils.results import feature_matching_recall, matching_table
    res = _result([[10, 40], [20, 50], [0, 30], [8, 8]], [[1, 1], [0, 3], [0, 9], [8, 8]], (250, 1000))
    flag = [1, 1, 1, 0]
    rows = [res.rows(c, flag) for c in range(2)]
    lines, table = matching_table((250, 1000), rows)
    assert list(table) == [250, 1000]
    # ratios 0.1, 0, 0 | 0.025, 0.06, 0.3 against 0.05; the unlisted pair counts nowhere
    assert table[250] == dict(correct=1, gt=3, recall=float(1 / 3) * 100, ave_num_inliers=1.0, ave_inlier_ratio=0.1)
    assert table[1000]["correct"] == 2 and table[1000]["gt"] == 3 and table[1000]["recall"] == float(2 / 3) * 100
    assert table[1000]["ave_num_inliers"] == 13 / 2 and abs(table[1000]["ave_inlier_ratio"] - (0.025 + 0.06 + 0.3) / 2) < 1e-15
    assert table[250] == feature_matching_recall(rows[0]) and table[1000] == feature_matching_recall(rows[1], 0.05)
    assert matching_table((250, 1000), rows, inlier_ratio=0.2)[1][1000]["correct"] == 1
    assert lines[:5] == ["num_keypts = 250", "Correct Match 1, ground truth Match 3", "Recall %s%%" % (float(1 / 3) * 100),
                         "Average Num Inliners: 1.0", "Average Num Inliner Ratio: 0.1"]
    assert len(lines) == 10 and lines[5] == "num_keypts = 1000"
    with pytest.raises(ValueError):
        matching_table((250,), rows)


def test_fixture_margins_meet_its_own_rule(golden):
    g = golden
    assert tuple(g["num_keypts"]) == (250, 1000, 1536) and tuple(g["kp"].shape) == (3, 1536, 36) and g["count"].tolist() == [1536, 1536, 678]
    assert g["num_keypts"][-1] > 1024 and g["count"].min() < g["num_keypts"][-1]          # beyond register_pairs, and a short block
    assert len(str(g["sha256_evaluate"])) == 64 and float(g["factor"]) == 8.0 and float(g["threshold"]) == 0.1
    assert 0 < float(g["err"]) < 1e-5 and float(g["gap"]) >= 8.0 * float(g["err"])
    assert 0 < float(g["point_err"]) < 1e-5 and float(g["band"]) >= 8.0 * float(g["point_err"])
    assert g["mutual_offsets"].tolist() == np.concatenate([[0], np.cumsum(g["mutual_count"].reshape(-1))]).tolist()
    assert g["mutual"].shape == (int(g["mutual_count"].sum()), 2) and (g["gt_inliers"] <= g["mutual_count"]).all()
    assert g["gt_inliers"][0].min() > 20 and g["mutual_count"].min() > 100                # a pair that overlaps; many mutual pairs everywhere


def test_restatement_reproduces_the_fixture(golden):
    g = golden
    blocks = [g["kp"][f, :n] for f, n in enumerate(g["count"])]
    pairs, counts = [tuple(p) for p in g["pairs"].tolist()], tuple(int(k) for k in g["num_keypts"])
    # the recorded margins are those of the data
    m = mnp.margins(blocks, pairs, g["gt_target_to_source"], counts, float(g["threshold"]), reference_form=True)
    assert mnp.margins_ok(m, float(g["factor"]))
    assert np.isclose(m["err"], float(g["err"]), rtol=0.05) and np.isclose(m["point_err"], float(g["point_err"]), rtol=0.05)   # (a float32 product of BLAS)
    assert np.isclose(m["gap"], float(g["gap"]), rtol=1e-6) and np.isclose(m["band"], float(g["band"]), rtol=1e-6)
    mc, gi = mnp.match_counts(blocks, pairs, g["gt_target_to_source"], counts, float(g["threshold"]))
    assert np.array_equal(mc, g["mutual_count"]) and np.array_equal(gi, g["gt_inliers"])
    off = g["mutual_offsets"]
    for p, (a, b) in enumerate(pairs):
        for c, k in enumerate(counts):
            want = g["mutual"][off[p * len(counts) + c]:off[p * len(counts) + c + 1]]
            assert np.array_equal(mnp.mutual_pairs(mnp.tail(blocks[a], k)[:, 3:35], mnp.tail(blocks[b], k)[:, 3:35]), want), (p, k)
