"""Overlap of fragment pairs (d3f_overlap_pairs / overlap.overlap_pairs), the part that needs no GPU: the entry point is bound, every
argument is refused on the host before a launch, the Python layer refuses what it must, the fp32 numpy restatement
(tests/overlap_np.py) reproduces what the reference's own Python computed (tests/golden/overlap.npz, tools/make_golden_overlap.py)
exactly -- every count, every nearest row, the selection -- and the fixture keeps both of its margins; the pickle writer round-trips."""
import ctypes
import os
import pickle
import types

import numpy as np
import pytest

import overlap_np as onp
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "overlap.npz"))


def test_entry_point_is_exported_and_bound(lib):
    from d3feat_amd import _lib
    assert "d3f_overlap_pairs" in _lib.SIGNATURES and hasattr(lib, "d3f_overlap_pairs")
    assert "int d3f_overlap_pairs(" in open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()


def _call(lib, grid=1, grid_bytes=None, N=1000, B=4, pairs=1, P=3, thr=0.05, count=1, ld=0):
    """d3f_overlap_pairs without a device pointer: `grid`, `pairs`, `count` are NULL (0) or the address of a 64-byte HOST buffer that
    no call here gets as far as touching -- each is refused (or has nothing to do) before a launch."""
    buf = ctypes.create_string_buffer(64)
    p = lambda on: ctypes.addressof(buf) if on else None
    if grid_bytes is None:
        grid_bytes = lib.d3f_neighbor_grid_bytes(max(N, 0), max(B, 1))
    return lib.d3f_overlap_pairs(p(grid), grid_bytes, N, B, p(pairs), P, thr, p(count), None, ld, None)


def test_host_side_argument_checks(lib):
    assert _call(lib, N=-1) == -3 and _call(lib, P=-1) == -3 and _call(lib, ld=-1) == -3                  # negative sizes
    assert _call(lib, B=0) == -3 and _call(lib, B=256) == -3 and _call(lib, B=-4) == -3                   # B outside 1 .. 255
    for thr in (0.0, -0.05, float("nan"), float("inf")):
        assert _call(lib, thr=thr) == -3
    assert _call(lib, grid=0) == -3 and _call(lib, pairs=0) == -3 and _call(lib, count=0) == -3           # NULL with P > 0
    assert _call(lib, grid=0, pairs=0, count=0) == -3
    assert _call(lib, grid_bytes=64) == -2 and _call(lib, grid_bytes=0) == -2                             # not a whole grid
    assert _call(lib, grid_bytes=lib.d3f_neighbor_grid_bytes(1000, 4) - 2048) == -2
    assert _call(lib, B=255, grid_bytes=64) == -2                                                         # 255 elements are taken
    assert _call(lib, P=0) == 0 and _call(lib, P=0, grid=0, pairs=0, count=0, grid_bytes=0) == 0          # nothing to do: no launch
    assert _call(lib, P=0, thr=0.0) == -3                                                                 # sizes are checked first


def test_python_validation():
    import torch
    from d3feat_amd import _lib, overlap, registration
    assert overlap.OVERLAP_3DMATCH == dict(threshold=0.025, min_ratio=0.30)
    pts, lens = torch.zeros(12, 3), torch.tensor([4, 4, 4], dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):                 # no CPU path
        overlap.overlap_pairs(pts, lens, torch.zeros(1, 2, dtype=torch.int32), 0.05)
    with pytest.raises(ValueError, match="255"):                 # one stack holds D3F_MAX_BATCH fragments
        overlap.overlap_pairs(torch.zeros(256, 3), [1] * 256, None, 0.05)
    with pytest.raises(ValueError, match="255"):
        overlap.overlap_pairs(pts, [], None, 0.05)
    small = types.SimpleNamespace(radius=0.04, Ns=12, B=3)       # a grid built for a smaller radius cannot serve the threshold
    with pytest.raises(ValueError, match="radius"):
        overlap.overlap_pairs(pts, lens, None, 0.05, grid=small)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            overlap.overlap_pairs(pts, lens, None, thr)
    assert registration.PAIRS_PER_CALL == 4096


def test_pair_overlap_figures_from_host_arrays():
    """ratios / selected / matches are host arithmetic on the read-back tensors."""
    import torch
    from d3feat_amd import overlap
    res = overlap.PairOverlap(4, 5, torch.device("cpu"))
    res.count.copy_(torch.tensor([3, 0, -1, 2]))
    res.src_len.copy_(torch.tensor([5, 0, 0, 4]))
    res.nearest.copy_(torch.tensor([[7, -1, 0, 2, -1], [-1] * 5, [-1] * 5, [-1, 1, 1, -1, -1]]))
    r = res.ratios()
    assert r.dtype == np.float64 and r.tolist() == [3 / 5, 0.0, 0.0, 0.5]
    assert res.selected().tolist() == [0, 3] and res.selected(0.5).tolist() == [0] and res.selected(0.6).tolist() == []
    m = res.matches(0)
    assert m.dtype == np.int32 and m.tolist() == [[0, 7], [2, 0], [3, 2]]
    assert res.matches(1).shape == (0, 2) and res.matches(3).tolist() == [[1, 1], [2, 1]]
    bare = overlap.PairOverlap(1, None, torch.device("cpu"))
    bare.count.zero_(), bare.src_len.zero_()
    with pytest.raises(ValueError):
        bare.matches(0)


def test_stack_fragments_moves_in_float64(monkeypatch):
    import torch
    from d3feat_amd import overlap, registration
    monkeypatch.setattr(registration, "_dev", lambda device=None: torch.device("cpu"))
    rng = np.random.default_rng(0)
    clouds = [rng.random((5, 3)).astype(np.float32), np.zeros((0, 3), np.float32), torch.from_numpy(rng.random((2, 3)).astype(np.float32))]
    poses = []
    for _ in clouds:
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = q, rng.uniform(-1, 1, 3)
        poses.append(M)
    pts, lens = overlap.stack_fragments(clouds, poses)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (7, 3) and lens.tolist() == [5, 0, 2] and lens.dtype == torch.int32
    want = np.concatenate([(np.asarray(c, np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32) for c, M in zip(clouds, poses)])
    assert np.array_equal(pts.numpy(), want)
    plain, _ = overlap.stack_fragments(clouds)
    assert np.array_equal(plain.numpy()[:5], clouds[0])
    with pytest.raises(ValueError):
        overlap.stack_fragments(clouds, poses[:2])


def test_restatement_reproduces_the_reference(golden):
    g = golden
    clouds, thr = onp.split(g["points"], g["lens"]), float(g["threshold"])
    assert thr == 0.05 and len(clouds) == 6 and g["points"].dtype == np.float32 and len(str(g["sha256_cal_overlap"])) == 64
    assert all(3000 <= len(c) <= 4100 for c in clouds)
    directed = [tuple(p) for p in g["directed"].tolist()]
    assert directed == [(a, b) for a in range(6) for b in range(6) if a != b]
    count, near = onp.overlap(clouds, directed, thr)
    assert near.shape == g["nearest"].shape
    assert np.array_equal(count, g["count"])
    assert np.array_equal(near, g["nearest"].astype(np.int32))
    assert np.array_equal((g["nearest"] >= 0).sum(1), g["count"])
    # the selection of cal_overlap.py:121 and the ratios it pickled, from the counts
    upper = [tuple(p) for p in g["pairs"].tolist()]
    assert upper == [(a, b) for a in range(6) for b in range(a + 1, 6)]
    ratio = np.array([count[directed.index(p)] / len(clouds[p[0]]) for p in upper])
    assert np.array_equal(ratio > 0.30, g["selected"]) and 0 < g["selected"].sum() < 15
    assert np.array_equal(ratio[g["selected"]], g["selected_ratio"][g["selected"]]) and np.isnan(g["selected_ratio"][~g["selected"]]).all()
    assert ratio.min() == 0.0 and ratio.max() > 0.8 and ((ratio > 0.2) & (ratio < 0.3)).any() and ((ratio > 0.3) & (ratio < 0.45)).any()
    # the margins that make exact equality a fair demand of an fp32 search
    m = [onp.margins(clouds[a], clouds[b], thr) for a, b in directed]
    assert min(x[0] for x in m) >= onp.BAND and min(x[1] for x in m) >= onp.BAND
    assert onp.BAND == 2.0 ** -18


def test_restatement_on_the_edges():
    """The restatement itself, where the answer is known: strictness, ties, padding, indices outside the stack."""
    below = np.nextafter(np.float32(0.5), np.float32(0))
    q = np.zeros((1, 3), np.float32)
    assert onp.nearest_rows(q, np.float32([[0.5, 0, 0]]), 0.5).tolist() == [-1]
    assert onp.nearest_rows(q, np.float32([[below, 0, 0]]), 0.5).tolist() == [0]
    assert onp.nearest_rows(q, np.float32([[0.1, 0, 0], [0, 0.1, 0], [0.1, 0, 0]]), 0.5).tolist() == [0]
    count, near = onp.overlap([q, np.zeros((0, 3), np.float32), np.float32([[0.2, 0, 0], [0.1, 0, 0]])], [(0, 2), (2, 0), (0, 1), (1, 0), (0, 3), (-1, 0)], 0.5)
    assert count.tolist() == [1, 2, 0, 0, -1, -1] and near.tolist() == [[1, -1], [0, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]


def test_tables_round_trip(tmp_path):
    from d3feat_amd.utils.results import save_overlap_tables
    ids = ["room/seq-01/cloud_bin_%d" % k for k in range(3)]
    matches = [np.array([[0, 4], [2, 1], [5, 5]], np.int64), np.zeros((0, 2), np.int32)]
    paths = save_overlap_tables(str(tmp_path), ids, [(0, 1), (1, 2)], [0.75, np.float64(1.0) / 3.0], matches, split="train", downsample=0.025)
    assert [os.path.basename(p) for p in paths] == ["3DMatch_train_0.025_overlap.pkl", "3DMatch_train_0.025_keypts.pkl"]
    with open(paths[0], "rb") as f:
        ratio = pickle.load(f)
    with open(paths[1], "rb") as f:
        keypts = pickle.load(f)
    keys = ["room/seq-01/cloud_bin_0@room/seq-01/cloud_bin_1", "room/seq-01/cloud_bin_1@room/seq-01/cloud_bin_2"]
    assert list(ratio) == keys and list(keypts) == keys
    assert type(ratio[keys[0]]) is float and ratio[keys[0]] == 0.75 and ratio[keys[1]] == 1.0 / 3.0
    assert keypts[keys[0]].dtype == np.int32 and keypts[keys[0]].tolist() == [[0, 4], [2, 1], [5, 5]] and keypts[keys[1]].shape == (0, 2)
    with pytest.raises(ValueError):
        save_overlap_tables(str(tmp_path), ids, [(0, 1)], [0.5], [])
    with pytest.raises(ValueError):
        save_overlap_tables(str(tmp_path), ids, [(0, 1)], [0.5], [np.zeros((3,), np.int32)])


def test_tool_lists_fragments_in_the_reference_order(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("overlap_scene", os.path.join(ROOT, "tools", "overlap_scene.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for seq, ks in (("seq-02", (0, 1)), ("seq-01", (10, 2, 0)), ("other", (5,))):
        os.makedirs(tmp_path / "room" / seq)
        for k in ks:
            (tmp_path / "room" / seq / ("cloud_bin_%d.ply" % k)).write_bytes(b"")
            (tmp_path / "room" / seq / ("cloud_bin_%d.pose.npy" % k)).write_bytes(b"")
    assert tool.scene_ids(str(tmp_path), "room") == ["room/seq-01/cloud_bin_0", "room/seq-01/cloud_bin_2", "room/seq-01/cloud_bin_10",
                                                     "room/seq-02/cloud_bin_0", "room/seq-02/cloud_bin_1"]
