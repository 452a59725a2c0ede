"""Keypoint repeatability (d3f_repeatability_pairs / registration.repeatability_pairs), the part that needs no GPU: the entry point is
bound, every argument is refused on the host before a launch, the float64 numpy restatement (tests/repeatability_np.py) reproduces
what the reference's own Python computed (tests/golden/repeatability.npz, tools/make_golden_repeatability.py) exactly, and the host
side of tools/repeatability_scene.py (pair filter, printed lines)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import repeatability_np as rnp
from conftest import GOLDEN, ROOT

COUNTS = (4, 8, 16, 32, 64, 128, 256, 512)


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "repeatability.npz"))


def _fixture_blocks(g):
    return [g["kp"][f, :n] for f, n in enumerate(g["count"])]


CONVENTIONS = [("3dmatch", "gt_target_to_source", "target"), ("kitti", "gt_source_to_target", "source")]


def test_entry_point_is_exported_and_bound(lib):
    from d3feat_amd import _lib
    assert "d3f_repeatability_pairs" in _lib.SIGNATURES and hasattr(lib, "d3f_repeatability_pairs")
    header = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    m = re.search(r"#define\s+D3F_REPEAT_COUNTS_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.REPEAT_COUNTS_MAX == 16


def _call(lib, P=4, n_blocks=3, K=512, ld=4, moved=0, thr=0.1, counts=COUNTS, n_counts=None, null_thr=False, null_counts=False):
    """d3f_repeatability_pairs with NULL device pointers: every call here is refused (or has nothing to do) before a launch."""
    c_thr = ctypes.c_double(thr)
    c_ks = (ctypes.c_int * max(len(counts), 1))(*counts)
    return lib.d3f_repeatability_pairs(None, n_blocks, K, ld, None, None, P, None, moved, None if null_thr else ctypes.addressof(c_thr),
                                       None if null_counts else ctypes.addressof(c_ks), len(counts) if n_counts is None else n_counts,
                                       None, None, None)


def test_host_side_argument_checks(lib):
    assert _call(lib, P=-1) == -3
    assert _call(lib, K=0) == -3
    assert _call(lib, ld=2) == -3
    assert _call(lib, counts=(), n_counts=0) == -3 and _call(lib, counts=tuple(range(1, 18))) == -3       # n_counts outside 1..16
    assert _call(lib, counts=(0, 4)) == -3 and _call(lib, counts=(4, 1025)) == -3                         # a count outside 1..1024
    assert _call(lib, counts=(4, 4)) == -3 and _call(lib, counts=(8, 4)) == -3                            # not strictly ascending
    assert _call(lib, moved=2) == -3 and _call(lib, moved=-1) == -3
    assert _call(lib, thr=float("nan")) == -3 and _call(lib, thr=0.0) == -3 and _call(lib, thr=-0.1) == -3
    assert _call(lib, null_thr=True) == -3 and _call(lib, null_counts=True) == -3
    assert _call(lib) == -3                                      # valid sizes, P > 0: the NULL device pointers
    assert _call(lib, P=0) == 0                                  # nothing to do: no launch
    assert _call(lib, P=0, K=4096, counts=tuple(range(1, 17))) == 0          # K itself may exceed D3F_PAIRS_KMAX; 16 counts


def test_python_validation():
    import torch
    from d3feat_amd import _lib, registration as reg
    assert reg.REPEATABILITY_COUNTS == COUNTS
    assert reg.REPEATABILITY_3DMATCH == dict(distance_threshold=0.1, moved="target")
    assert reg.REPEATABILITY_KITTI == dict(distance_threshold=0.5, moved="source")
    kp, count, pairs = torch.zeros(2, 8, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):                 # no CPU path
        reg.repeatability_pairs(kp, count, pairs, np.eye(4)[None])


@pytest.mark.parametrize("name,gt_key,moved", CONVENTIONS)
def test_restatement_reproduces_the_reference(golden, name, gt_key, moved):
    g = golden
    assert tuple(g["num_keypts"]) == COUNTS and tuple(g["kp"].shape) == (6, 512, 3) and sorted(g["count"]) == [300] + [512] * 5
    assert len(str(g["sha256_evaluate_%s_our" % name])) == 64
    blocks, pairs, thr = _fixture_blocks(g), [tuple(p) for p in g["pairs"].tolist()], float(g["threshold_" + name])
    assert thr == (0.1 if name == "3dmatch" else 0.5) and len(pairs) == 15
    want = g["ratios_" + name] * np.asarray(COUNTS, np.float64)
    assert np.array_equal(want, np.rint(want))                   # the reference's ratios are counts / k
    got = rnp.repeat_counts(blocks, pairs, g[gt_key], COUNTS, thr, moved)
    assert np.array_equal(got, want.astype(np.int64))
    listed = g["listed"]
    assert 0 < listed.sum() < len(pairs)
    scene = got[listed].sum(0) / (np.asarray(COUNTS, np.float64) * listed.sum())
    assert np.abs(scene - g["scene_" + name]).max() <= 1e-12
    assert scene[-1] > scene[0] and got.max() > 50 and (got[:, -1] == 0).any()        # a scene with and without overlap
    # the band that makes exact counts a fair demand: no column minimum within 1e-6 of the threshold
    assert rnp.band(blocks, pairs, g[gt_key], COUNTS, thr, moved) >= 1e-6


def test_fixture_gt_log_matches_its_matrices(golden, tmp_path):
    from d3feat_amd.utils.results import read_gt_log
    path = tmp_path / "gt.log"
    path.write_text(str(golden["gt_log"]))
    log = read_gt_log(str(path))
    pairs, listed = [tuple(p) for p in golden["pairs"].tolist()], golden["listed"]
    assert list(log) == ["%d_%d" % p for p, l in zip(pairs, listed) if l]
    for i, p in enumerate(pairs):
        if listed[i]:
            assert np.array_equal(log["%d_%d" % p], golden["gt_target_to_source"][i])
    assert np.allclose(golden["gt_source_to_target"] @ golden["gt_target_to_source"], np.eye(4), atol=1e-12)


def test_repeatability_table():
    from d3feat_amd.utils.results import repeatability_table
    lines, table = repeatability_table((4, 512), np.array([0.0, 0.2345703125]))
    assert lines == ["Average Repeatability at num_keypts = 4: 0.0", "Average Repeatability at num_keypts = 512: 0.2345703125"]
    assert table == {4: 0.0, 512: 0.2345703125}
    ave_repeatability, num_keypts = 1.0 / 3.0, 64                # the reference's own f-string
    assert repeatability_table([64], [1.0 / 3.0])[0] == [f"Average Repeatability at num_keypts = {num_keypts}: {ave_repeatability}"]
    with pytest.raises(ValueError):
        repeatability_table((4, 8), [0.5])


def _tool():
    spec = importlib.util.spec_from_file_location("repeatability_scene", os.path.join(ROOT, "tools", "repeatability_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_keeps_the_listed_pairs():
    from d3feat_amd.utils.results import read_gt_log
    log = read_gt_log(os.path.join(GOLDEN, "gt_log_hotel3.log"))
    n_frag = 1 + max(int(x) for key in log for x in key.split("_"))
    pairs, gt = _tool().listed_pairs(log, n_frag)
    keys = [tuple(int(x) for x in k.split("_")) for k in log]
    assert all(a < b for a, b in keys) and 0 < len(keys) < n_frag * (n_frag - 1) // 2
    assert pairs == sorted(keys) and gt.shape == (len(keys), 4, 4) and gt.dtype == np.float64
    for p, M in zip(pairs, gt):
        assert np.array_equal(M, log["%d_%d" % p])
    few, gt_few = _tool().listed_pairs(log, 10)                 # fewer fragments on disk than the log knows
    assert few == [p for p in pairs if p[1] < 10] and len(gt_few) == len(few)


def test_tool_reads_keypoint_files(tmp_path):
    from d3feat_amd.utils.results import save_3dmatch_keypoints
    rng = np.random.default_rng(0)
    recs = [rng.random((n, 8)).astype(np.float32) for n in (20, 7)]
    for f, r in enumerate(recs):
        save_3dmatch_keypoints(str(tmp_path), "room/seq/cloud_bin_%d.ply" % f, r)
    blocks = _tool().load_scene(str(tmp_path), "room", 16)
    assert [b.shape for b in blocks] == [(16, 4), (7, 4)]
    assert np.array_equal(blocks[0][:, :3], recs[0][-16:, :3]) and np.array_equal(blocks[1][:, 3], np.arange(7))
