"""The plumbing the one-call entry points of d3feat_amd.registration share (_counts, _scene_starts, _PairResult / _reuse): each rule
lives in one helper, so each is pinned here once, on the host -- the messages name the calling function, the ctypes arrays hold what
the library will read, `out=` is refused for another call and handed back with its read-back forgotten."""
import numpy as np
import pytest
import torch

from d3feat_amd import _lib
from d3feat_amd import registration as reg

CPU = torch.device("cpu")


# ---- _counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [[], list(range(1, 18)), [0, 4], [4, 9], [4, 4], [8, 4]],
                         ids=["empty", "17 counts", "a count of 0", "a count of kmax + 1", "equal neighbours", "descending"])
def test_counts_refuses(ks):
    with pytest.raises(ValueError, match="some_entry_point"):
        reg._counts("some_entry_point", ks, 8)


def test_counts_round_trip():
    ks, c_ks = reg._counts("f", (np.int64(1), 3, 8), 8)
    assert ks == [1, 3, 8] and all(type(k) is int for k in ks)
    assert len(c_ks) == 3 and list(c_ks) == ks and isinstance(c_ks, _lib.C.c_int * 3)
    most = list(range(1, _lib.REPEAT_COUNTS_MAX + 1))
    assert list(reg._counts("f", most, _lib.PAIRS_KMAX)[1]) == most                 # 16 counts are taken, 17 are not


# ---- _scene_starts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("starts", [[1, 3, 5], [0, 3, 4], [0, 4, 3, 5], [0] * 257 + [5]],
                         ids=["not from 0", "not to P", "descending", "258 entries"])
def test_scene_starts_refuses(starts):
    with pytest.raises(ValueError, match="some_entry_point"):
        reg._scene_starts("some_entry_point", starts, 5)


def test_scene_starts_round_trip():
    starts, c_starts = reg._scene_starts("f", np.asarray([0, 2, 2, 5]), 5)          # an empty scene is fine
    assert starts == [0, 2, 2, 5] and list(c_starts) == starts
    starts, c_starts = reg._scene_starts("f", [0], 0)                              # S = 0: no scene, no pair
    assert starts == [0] and list(c_starts) == [0]
    assert len(reg._scene_starts("f", [0] * 256 + [5], 5)[1]) == _lib.SCENES_MAX + 1     # 257 entries are taken, 258 are not


# ---- the result base ----------------------------------------------------------------------------------------------------------------
def _matching(P=2, ks=(3, 5), gt=True):
    m = reg.PairMatching(P, ks, CPU, gt)
    m.mutual_count.copy_(torch.arange(P * len(ks), dtype=torch.int32).reshape(P, len(ks)))
    if gt:
        m.gt_inliers.zero_()
    return m


def test_reuse_refuses_another_call():
    m = _matching()
    key = (2, (3, 5), True)
    assert m.key == key and m.device == CPU
    make = lambda: pytest.fail("out= was given: nothing is allocated")
    wrong_class = reg.PairRegistrationCounts(2, (3, 5), CPU, True, False)
    for out, k in [(wrong_class, key), (m, (3, (3, 5), True)), (m, (2, (3, 6), True)), (m, (2, (3, 5), False))]:
        with pytest.raises(ValueError, match="some_entry_point: out= was made for another call"):
            reg._reuse("some_entry_point", out, reg.PairMatching, k, CPU, make)
    with pytest.raises(ValueError, match="out= was made for another call"):
        reg._reuse("f", m, reg.PairMatching, key, torch.device("meta"), make)         # the same call on another device


def test_reuse_returns_the_object_with_its_read_back_forgotten():
    m = _matching()
    first = m._host()
    assert m._host() is first                                                        # one read-back, kept
    assert sorted(first) == ["gt_inliers", "mutual_count"] and np.array_equal(first["mutual_count"], [[0, 1], [2, 3]])
    m.mutual_count = m.mutual_count + 1             # (a new tensor: on the CPU a read-back shares the memory of the one it read)
    assert np.array_equal(m._host()["mutual_count"], [[0, 1], [2, 3]])               # still the cached copy
    again = reg._reuse("f", m, reg.PairMatching, (2, (3, 5), True), CPU, lambda: pytest.fail("nothing is allocated"))
    assert again is m and m._cache is None
    assert np.array_equal(m._host()["mutual_count"], [[1, 2], [3, 4]])
    named = reg.PairMatching(2, (3, 5), "cpu", True)                                # the device is the tensors', however it was spelled
    assert named.device == CPU and reg._reuse("f", named, reg.PairMatching, (2, (3, 5), True), CPU, None) is named
    fresh = reg._reuse("f", None, reg.PairMatching, (2, (3, 5), False), CPU, lambda: _matching(gt=False))
    assert isinstance(fresh, reg.PairMatching) and fresh._cache is None and sorted(fresh._host()) == ["mutual_count"]   # None: left out


def test_host_reads_back_once(monkeypatch):
    m = _matching()
    reads = []
    real = reg._PairResult._read
    monkeypatch.setattr(reg._PairResult, "_read", lambda self, name: (reads.append(name), real(self, name))[1])
    m._host()
    m._host()
    m.ratios()
    assert reads == ["mutual_count", "gt_inliers"]


def test_every_result_class_stores_its_key():
    from d3feat_amd import overlap, validation
    made = [(reg.PairRegistration(2, 8, CPU, True, False), (2, 8, True, False)),
            (reg.PairRepeatability(2, (4, 8), CPU), (2, (4, 8))),
            (reg.PairMatching(2, (4, 8), CPU, False), (2, (4, 8), False)),
            (reg.PairRegistrationCounts(2, (4, 8), CPU, True, True), (2, (4, 8), True, True)),
            (reg.PairPoseErrors(2, 3, False, CPU), (2, 3, False)),
            (reg.SceneMatching(2, 1, [0, 2], 0.05, CPU), (2, 1, (0, 2), 0.05)),
            (reg.SceneRecall(2, 1, True, [0, 1, 2], 0.04, False, CPU), (2, 1, True, (0, 1, 2), 0.04, False)),
            (overlap.PairOverlap(2, 7, CPU), (2, True)),
            (overlap.PairOverlap(2, None, CPU), (2, False)),
            (validation.PairValidation(2, CPU), (2,))]
    for obj, key in made:
        assert isinstance(obj, reg._PairResult) and obj.key == key and obj.device == CPU and obj._cache is None, type(obj).__name__


def test_ransac_dict_is_the_same_for_both_result_classes():
    """PairRegistration.host(p) and PairRegistrationCounts.host(p, c) build their common entries from the same fields."""
    one = reg.PairRegistration(2, 4, CPU, False, True)
    many = reg.PairRegistrationCounts(2, (4,), CPU, True, True)
    T = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    vals = dict(inliers=[3, 0], sumd2=[3 << 30, 0], validations=[5, 0], iterations=[40, 7], best_iteration=[12, -1], mutual_count=[2, 0],
                gt_inliers=[1, 0])
    near = torch.tensor([[2, -1, 0, 1], [-1, -1, -1, -1]], dtype=torch.int32)
    ns = torch.tensor([4, 0], dtype=torch.int32)
    one.T.copy_(T); many.T.copy_(T[:, None])
    for k, v in vals.items():
        getattr(one, k).copy_(torch.tensor(v)); getattr(many, k).copy_(torch.tensor(v)[:, None])
    one.nearest.copy_(near); many.nearest.copy_(near)
    one.ns = one.nt = ns
    many.ns = many.nt = ns[:, None]
    for p in range(2):
        a, b = one.host(p), many.host(p, 0)
        assert b.pop("mutual_count") == vals["mutual_count"][p]
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), (p, k)
    a = one.host(0)
    assert a["fitness"] == 0.75 and a["inlier_rmse"] == 0.5 and a["inlier_ratio"] == 0.5 and a["best_iteration"] == 12
    assert np.array_equal(a["correspondence_set"], [[0, 2], [2, 0], [3, 1]]) and np.array_equal(a["transformation"][3], [0, 0, 0, 1])
    assert one.host(1)["fitness"] == 0.0 and one.host(1)["inlier_ratio"] == 0.0 and len(one.host(1)["correspondence_set"]) == 0
