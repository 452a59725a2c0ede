"""RANSAC registration of every pair at every keypoint count (d3f_register_pairs_counts / registration.register_pairs_counts), the part
that needs no GPU: the two entry points are exported and bound, every size is refused on the host before a launch, the workspace
grows with what it holds, and register_pairs keeps its limit."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

COUNTS = (250, 500, 1000, 2500, 5000)
OUTS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers", "nearest")


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def test_entry_points_are_exported_and_bound(lib):
    from d3feat_amd import _lib
    header = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    for name in ("d3f_register_pairs_counts", "d3f_register_pairs_counts_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    m = re.search(r"#define\s+D3F_PAIRS_KMAX\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.PAIRS_KMAX == 1024          # register_pairs keeps its limit


def _ws_bytes(lib, P, counts=COUNTS, n_blocks=3, K=8192, max_validation=1000, n_counts=None):
    ks = (ctypes.c_int * max(len(counts), 1))(*counts)
    return lib.d3f_register_pairs_counts_workspace_bytes(P, n_blocks, K, ctypes.addressof(ks),
                                                         len(counts) if n_counts is None else n_counts, max_validation)


def _call(lib, P=4, n_blocks=3, K=8192, ld=36, C=32, counts=COUNTS, n_counts=None, null_counts=False, radius=0.05, ransac_n=3,
          max_iteration=50000, max_validation=1000, null=(), null_in=(), gt=False, short=0):
    """d3f_register_pairs_counts over one dummy HOST buffer (or NULL): every call here is refused, or has nothing to do, before a launch."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    ks = (ctypes.c_int * max(len(counts), 1))(*counts)
    n = len(counts) if n_counts is None else n_counts
    need = lib.d3f_register_pairs_counts_workspace_bytes(P, n_blocks, K, ctypes.addressof(ks), n, max_validation)
    ins = [None if name in null_in else p for name in ("kp", "count", "pairs")]
    outs = [None if o in null else p for o in OUTS]
    return lib.d3f_register_pairs_counts(ins[0], n_blocks, K, ld, C, ins[1], ins[2], P, None if null_counts else ctypes.addressof(ks), n,
                                         radius, ransac_n, 0.9, 0.05, max_iteration, max_validation, 5, p if gt else None, 0.10,
                                         *outs, p, max(need - short, 0), None)


def test_host_side_argument_checks(lib):
    call = lambda **kw: _call(lib, **kw)
    assert call(short=1) == -2                                   # everything else in order: only the workspace is one byte short
    assert call(counts=(250, 1000, 500)) == -3                   # not ascending
    assert call(counts=(250, 250)) == -3                         # not strictly
    assert call(counts=(0, 250)) == -3 and call(counts=(250, 8193)) == -3
    assert call(counts=(8192,), short=1) == -2                   # the largest count itself is taken
    assert call(counts=tuple(range(1, 18))) == -3                # 17 counts
    assert call(counts=tuple(range(1, 17)), short=1) == -2       # 16 are taken
    assert call(counts=(), n_counts=0) == -3 and call(null_counts=True) == -3
    assert call(n_blocks=256) == -3 and call(n_blocks=0) == -3
    assert call(n_blocks=255, short=1) == -2
    assert call(ransac_n=2) == -3 and call(ransac_n=9) == -3
    assert call(C=24, ld=28) == -3
    assert call(ld=35) == -3                                     # ld < C + 4
    assert call(P=-1) == -3 and call(K=0) == -3
    assert call(max_validation=0) == -3 and call(max_iteration=-1) == -3
    assert call(radius=float("nan")) == -3
    for name in ("kp", "count", "pairs"):
        assert call(null_in=(name,)) == -3, name
    for out in ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count"):
        assert call(null=(out,)) == -3, out
    assert call(gt=True, null=("gt_inliers",)) == -3             # gt without a place for its count
    assert call(null=("nearest",), short=1) == -2                # the correspondences are optional
    assert call(null=("gt_inliers",), short=1) == -2             # and so is gt_inliers without gt
    assert call(P=0) == 0                                        # nothing to do: no launch
    assert call(P=0, null=OUTS, null_in=("kp", "count", "pairs")) == 0


def test_workspace_grows_with_pairs_counts_and_validations(lib):
    w = lambda *a, **kw: _ws_bytes(lib, *a, **kw)
    assert w(819, max_validation=1000) >= 819 * 5 * 1000 * 64    # 64 bytes per pair, count and validation
    assert w(8) < w(16)
    assert w(8, counts=(250,)) < w(8, counts=(250, 500)) < w(8, counts=(250, 500, 1000))
    assert w(8, max_validation=100) < w(8, max_validation=200)
    assert w(8, n_blocks=3) < w(8, n_blocks=32)                  # the stack and its grid
    assert w(8, counts=(250,), K=8192) == w(8, counts=(250,), K=250)       # only the rows used count
    assert w(0) == w(1) > 0
    # sizes the call refuses
    assert w(-1) == 0 and w(8, n_blocks=256) == 0 and w(8, counts=(500, 250)) == 0 and w(8, max_validation=0) == 0
    assert lib.d3f_register_pairs_counts_workspace_bytes(4, 3, 250, None, 5, 100) == 0


def test_cpu_tensors_are_rejected():
    import torch
    from d3feat_amd import _lib, registration as reg
    kp, count, pairs = torch.zeros(2, 8, 36), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.register_pairs_counts(kp, count, pairs, **reg.EVALUATE_3DMATCH)


def test_result_object_slices_by_count():
    """PairRegistrationCounts on host tensors: the offsets of the nearest rows, .at(c) and .host(p, c)."""
    import numpy as np
    import torch
    from d3feat_amd import registration as reg
    res = reg.PairRegistrationCounts(2, (3, 5), torch.device("cpu"), gt=True, nearest=True)
    assert res.offsets == (0, 3) and tuple(res.nearest.shape) == (2, 8) and tuple(res.T.shape) == (2, 2, 3, 4)
    for f in res.FIELDS:
        getattr(res, f).zero_()
    res.T[1, 1] = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    res.inliers[1, 1], res.sumd2[1, 1], res.mutual_count[1, 1], res.gt_inliers[1, 1] = 2, 1 << 31, 4, 1
    res.nearest[1] = torch.tensor([9, 9, 9, -1, 2, -1, 0, 7])
    res.ns, res.nt = torch.tensor([[3, 5], [3, 4]]), torch.tensor([[3, 5], [3, 5]])
    at = res.at(1)
    assert at["nearest"].tolist() == [[0] * 5, [-1, 2, -1, 0, 7]] and tuple(at["T"].shape) == (2, 3, 4) and int(at["inliers"][1]) == 2
    h = res.host(1, 1)
    assert h["fitness"] == 0.5 and h["inlier_rmse"] == 0.5 and h["inlier_ratio"] == 0.25      # the fifth entry is padding: Ns = 4
    assert np.array_equal(h["correspondence_set"], [[1, 2], [3, 0]])
    assert np.array_equal(h["transformation"][:3], np.arange(12.0).reshape(3, 4))
