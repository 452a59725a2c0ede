"""Overlap of fragment pairs on the GPU (d3f_overlap_pairs, overlap.overlap_pairs): every pair of a stack in one call, against

  1. what the reference's own Python computed (tests/golden/overlap.npz): all 30 directed pairs and the 6 self pairs -- counts,
     nearest rows, ratios, the selection and the match lists, exactly;
  2. the parent's API on the same scene: the loop of single-cloud grids and d3f_neighbor_grid_score(V = 1, identity), bit for bit;
  3. the smallest shapes that can break it, against the fp32 numpy restatement (tests/overlap_np.py): source lengths around the
     wavefront and the workgroup, empty and far-away fragments, a distance equal to the threshold, duplicate points, self pairs,
     repeated pairs, indices outside the stack, rows longer and shorter than the fragments;
  4. 255 fragments (beyond the 40 elements whose geometry the search kernels keep in LDS);
  5. a threshold 25 x smaller on the fixture's clouds (cells several times the threshold);
  6. more pairs than one entry-point call takes;
  7. capture in a HIP graph, replay on other points with the grid rebuilt inside the graph;
  8. tools/overlap_scene.py end to end."""
import importlib.util
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import overlap_np as onp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _pairs(device, pairs):
    return torch.tensor(np.asarray(pairs, np.int32).reshape(-1, 2), dtype=torch.int32, device=device)


def _run(device, clouds, pairs, thr, nearest=True, **kw):
    from d3feat_amd import overlap
    points, lens = overlap.stack_fragments(clouds, device=device)
    return overlap.overlap_pairs(points, lens, _pairs(device, pairs), thr, nearest=nearest, **kw)


def _check(res, clouds, pairs, thr):
    """Equal to the restatement: counts, whole nearest rows (padding included), source lengths."""
    count, near = onp.overlap(clouds, pairs, thr, ld=res.ld)
    n = len(clouds)
    assert res.count.dtype == torch.int32 and res.nearest.dtype == torch.int32 and res.count.is_cuda
    assert np.array_equal(res.count.cpu().numpy(), count), (res.count.cpu().numpy(), count)
    got = res.nearest.cpu().numpy()
    assert got.shape == near.shape and np.array_equal(got, near), np.argwhere(got != near)[:10]
    assert res.src_len.cpu().tolist() == [len(clouds[a]) if 0 <= a < n else 0 for a, _ in pairs]
    return count, near


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "overlap.npz"))
    return g, onp.split(g["points"], g["lens"])


@pytest.fixture(scope="module")
def golden_result(device, golden):
    """The fixture's scene in one call: the 30 directed pairs, then the 6 self pairs.  Shared, never written to."""
    g, clouds = golden
    pairs = [tuple(p) for p in g["directed"].tolist()] + [(f, f) for f in range(6)]
    return pairs, _run(device, clouds, pairs, float(g["threshold"]))


# ---- 1. the reference's own figures -----------------------------------------------------------------------------------------------
def test_fixture_of_the_reference(device, golden, golden_result):
    from d3feat_amd import overlap
    g, clouds = golden
    pairs, res = golden_result
    lens = g["lens"]
    count, near = res.count.cpu().numpy(), res.nearest.cpu().numpy()
    assert near.shape == (36, lens.max())
    assert np.array_equal(count[:30], g["count"]) and np.array_equal(near[:30], g["nearest"].astype(np.int32))
    assert np.array_equal(count[30:], lens)                                    # a == b: every point has itself at distance 0
    for f in range(6):
        assert np.array_equal(near[30 + f, :lens[f]], np.arange(lens[f])) and (near[30 + f, lens[f]:] == -1).all()
    want_ratio = np.concatenate([g["count"] / np.array([lens[a] for a, _ in pairs[:30]], np.float64), np.ones(6)])
    assert res.ratios().dtype == np.float64 and np.array_equal(res.ratios(), want_ratio)
    assert np.array_equal(res.selected(), np.nonzero(want_ratio > 0.30)[0])
    for p in (0, 4, 17, 29, 33):
        row = g["nearest"][p].astype(np.int32) if p < 30 else np.arange(lens[p - 30])
        q = np.nonzero(row >= 0)[0]
        m = res.matches(p)
        assert m.dtype == np.int32 and np.array_equal(m, np.stack([q, row[q]], 1))
    # the pairs a < b alone, the default pair list, counts only: the selection and the ratios cal_overlap pickled
    points, stack_lens = overlap.stack_fragments(clouds, device=device)
    upper = overlap.overlap_pairs(points, stack_lens, threshold=float(g["threshold"]))
    assert upper.nearest is None and upper.P == 15
    assert np.array_equal(upper.selected(), np.nonzero(g["selected"])[0])
    assert np.array_equal(upper.ratios()[g["selected"]], g["selected_ratio"][g["selected"]])
    with pytest.raises(ValueError):
        upper.matches(0)


# ---- 2. the parent's API ----------------------------------------------------------------------------------------------------------
def _bench_tool():
    spec = importlib.util.spec_from_file_location("overlap_bench", os.path.join(ROOT, "tools", "overlap_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bit_equal_to_the_loop_over_single_cloud_grids(device, golden, golden_result):
    g, clouds = golden
    pairs, res = golden_result
    dev_clouds = [torch.from_numpy(c).to(device) for c in clouds]
    nearest = torch.full((len(pairs), res.ld), -1, dtype=torch.int32, device=device)
    count, nearest = _bench_tool().parent_loop(dev_clouds, pairs, float(g["threshold"]), nearest=nearest)
    assert torch.equal(res.count, count) and torch.equal(res.nearest, nearest)
    assert int(count.sum()) > 30000


# ---- 3. the smallest shapes that can break it ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_clouds():
    """0: a 300-point target; 1-6: sources of 1, 63, 64, 65, 256, 257 points near it; 7: empty; 8: 1000 m away; 9: the target with
    bit-equal duplicates of some of its points appended."""
    rng = np.random.default_rng(7)
    tgt = (rng.random((300, 3)) * 0.5).astype(np.float32)
    clouds = [tgt]
    for n in (1, 63, 64, 65, 256, 257):
        base = tgt[rng.integers(0, 300, n)] if n > 1 else tgt[:1]
        clouds.append((base + rng.normal(scale=0.03, size=(n, 3))).astype(np.float32))
    clouds.append(np.zeros((0, 3), np.float32))
    clouds.append(tgt + np.float32(1000.0))
    clouds.append(np.concatenate([tgt, tgt[[5, 5, 17, 299]]], 0))
    return clouds


def test_small_shapes(device, small_clouds):
    pairs = [(s, 0) for s in range(1, 7)] + [(0, s) for s in range(1, 7)]          # every source length, both directions
    pairs += [(7, 0), (0, 7), (7, 7)]                                              # an empty fragment as source, target, both
    pairs += [(8, 0), (0, 8), (8, 8)]                                              # 1000 m away (and near itself)
    pairs += [(0, 0), (9, 9), (0, 9), (6, 9)]                                      # self pairs, duplicates in the target
    pairs += [(5, 0), (5, 0), (3, 0)]                                              # repeated pairs
    pairs += [(-1, 0), (0, 10), (10, 10), (0, -3), (1 << 30, 2)]                   # indices outside the stack
    res = _run(device, small_clouds, pairs, 0.05)
    count, near = _check(res, small_clouds, pairs, 0.05)
    by = {p: i for i, p in enumerate(pairs)}
    assert all(0 < count[by[(s, 0)]] for s in (3, 4, 5, 6)) and count[by[(6, 0)]] < 257
    assert count[by[(7, 0)]] == count[by[(0, 7)]] == count[by[(7, 7)]] == 0 and count[by[(8, 0)]] == count[by[(0, 8)]] == 0
    assert count[by[(0, 0)]] == 300 and np.array_equal(near[by[(0, 0)], :300], np.arange(300)) and count[by[(8, 8)]] == 300
    # duplicates: the lowest index wins -- the appended copies 300..303 find the originals, and nobody finds a copy
    assert count[by[(9, 9)]] == 304 and near[by[(9, 9)], 300:304].tolist() == [5, 5, 17, 299]
    assert near[by[(9, 9)]].max() <= 299 and near[by[(0, 9)]].max() <= 299 and np.array_equal(near[by[(0, 9)], :300], np.arange(300))
    rows = res.nearest.cpu().numpy()
    same = [i for i, p in enumerate(pairs) if p == (5, 0)]
    assert len(same) == 3 and all(np.array_equal(rows[i], rows[same[0]]) and count[i] == count[same[0]] for i in same)
    for bad in pairs[-5:]:
        assert count[by[bad]] == -1 and (rows[by[bad]] == -1).all()
    assert res.ratios()[by[(7, 0)]] == 0.0 and res.ratios()[by[(-1, 0)]] == 0.0 and res.selected().tolist() == np.nonzero(res.ratios() > 0.3)[0].tolist()


def test_distance_equal_to_the_threshold_is_no_match(device):
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert below == np.float32(0.49999997)
    clouds = [np.zeros((1, 3), np.float32), np.float32([[0.5, 0, 0]]), np.float32([[below, 0, 0]]), np.float32([[0.5, 0, 0], [0, below, 0]])]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)]
    res = _run(device, clouds, pairs, 0.5)
    assert res.count.cpu().tolist() == [0, 1, 1, 0, 1, 1]                        # d2 == r2 exactly: not inside
    assert res.nearest.cpu().tolist() == [[-1, -1], [0, -1], [1, -1], [-1, -1], [0, -1], [-1, 0]]
    _check(res, clouds, pairs, 0.5)


def test_rows_longer_and_shorter_than_the_fragments(device, small_clouds):
    from d3feat_amd import _lib, ops, overlap
    pairs = [(6, 0), (0, 6), (2, 0)]
    points, lens = overlap.stack_fragments(small_clouds, device=device)
    wide = overlap.PairOverlap(3, 400, device)
    wide.nearest.fill_(123)
    res = overlap.overlap_pairs(points, lens, _pairs(device, pairs), 0.05, nearest=True, out=wide)
    assert res is wide and tuple(res.nearest.shape) == (3, 400)
    count, near = _check(res, small_clouds, pairs, 0.05)
    assert (near[:, 304:] == -1).all() and (near[0, 257:] == -1).all()
    with pytest.raises(ValueError):                                              # the Python layer refuses rows shorter than a fragment
        overlap.overlap_pairs(points, lens, _pairs(device, pairs), 0.05, nearest=True, out=overlap.PairOverlap(3, 100, device))
    with pytest.raises(ValueError):
        overlap.overlap_pairs(points, lens, _pairs(device, pairs), 0.05, nearest=False, out=wide)
    # the entry point itself with rows of 10: the first 10 entries of every row, and nothing past the last row
    grid = ops.NeighborGrid(points, lens, 0.05)
    buf = torch.full((3 * 10 + 64,), 77, dtype=torch.int32, device=device)
    cnt = torch.empty((3,), dtype=torch.int32, device=device)
    rc = _lib.load().d3f_overlap_pairs(grid.mem.data_ptr(), grid.nbytes, points.shape[0], len(small_clouds), _pairs(device, pairs).data_ptr(), 3,
                                       0.05, cnt.data_ptr(), buf.data_ptr(), 10, ops._stream(device))
    assert rc == 0
    assert np.array_equal(cnt.cpu().numpy(), count)                              # the count does not depend on the row length
    assert np.array_equal(buf[:30].view(3, 10).cpu().numpy(), near[:, :10]) and (buf[30:] == 77).all()
    # a grid of a larger radius serves a smaller threshold; one of a smaller radius is refused
    res2 = overlap.overlap_pairs(points, lens, _pairs(device, pairs), 0.03, nearest=True, grid=grid)
    _check(res2, small_clouds, pairs, 0.03)
    with pytest.raises(ValueError, match="radius"):
        overlap.overlap_pairs(points, lens, _pairs(device, pairs), 0.06, grid=grid)
    with pytest.raises(ValueError):                                              # a grid over other points
        overlap.overlap_pairs(points.clone(), lens, _pairs(device, pairs), 0.05, grid=grid)


# ---- 4. many elements -------------------------------------------------------------------------------------------------------------
def test_255_fragments(device):
    from d3feat_amd import _lib
    rng = np.random.default_rng(3)
    assert _lib.MAX_BATCH == 255
    clouds = [(rng.random((int(n), 3)) * np.float32([0.4, 0.3, 0.2])).astype(np.float32) for n in rng.integers(15, 26, 255)]
    pairs = [(0, 39), (39, 40), (40, 254), (254, 0), (40, 40), (0, 254), (100, 200), (253, 254), (41, 38), (254, 254), (255, 0)]
    res = _run(device, clouds, pairs, 0.05)
    count, _ = _check(res, clouds, pairs, 0.05)
    assert count[-1] == -1 and (count[:-1] > 0).all() and (count[:4] < 26).all()


# ---- 5. coarser cells -------------------------------------------------------------------------------------------------------------
def test_threshold_25_times_smaller(device, golden):
    g, clouds = golden
    thr = float(g["threshold"]) / 25.0
    pairs = [(0, 1), (1, 0), (2, 3), (4, 5), (5, 4), (3, 3)]
    res = _run(device, clouds, pairs, thr)
    count, _ = _check(res, clouds, pairs, thr)
    assert count[5] == len(clouds[3]) and 0 < count[:5].sum() < 500              # matches are rare at 2 mm, and there are some


# ---- 6. chunking ------------------------------------------------------------------------------------------------------------------
def test_more_pairs_than_one_call_takes(device):
    from d3feat_amd import registration
    rng = np.random.default_rng(5)
    clouds = [(rng.random((50, 3)) * 0.3).astype(np.float32) for _ in range(3)]
    nine = [(a, b) for a in range(3) for b in range(3)]
    alone = _run(device, clouds, nine, 0.05)
    _check(alone, clouds, nine, 0.05)
    P = registration.PAIRS_PER_CALL + 4
    many = (nine * (P // 9 + 1))[:P]
    res = _run(device, clouds, many, 0.05)
    idx = torch.arange(P, device=device) % 9
    assert res.P == P and torch.equal(res.count, alone.count[idx]) and torch.equal(res.nearest, alone.nearest[idx])
    assert 0 < int(alone.count[1]) < 50


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_in_a_hip_graph_and_replay_on_other_points(device, small_clouds):
    from d3feat_amd import overlap
    rng = np.random.default_rng(9)
    lens_host = [len(c) for c in small_clouds]
    other = [(c + rng.normal(scale=0.02, size=c.shape)).astype(np.float32) for c in small_clouds]
    pairs_host = [(6, 0), (0, 6), (5, 9), (0, 0), (7, 0), (8, 0), (2, 5)]
    pairs = _pairs(device, pairs_host)
    pts1, lens = overlap.stack_fragments(small_clouds, device=device)
    pts2, _ = overlap.stack_fragments(other, device=device)
    eager1 = overlap.overlap_pairs(pts1, lens, pairs, 0.05, nearest=True)
    eager2 = overlap.overlap_pairs(pts2, lens, pairs, 0.05, nearest=True)
    _check(eager2, other, pairs_host, 0.05)
    assert not torch.equal(eager1.count, eager2.count)
    points = pts1.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        res = overlap.overlap_pairs(points, lens, pairs, 0.05, nearest=True)     # eager warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        overlap.overlap_pairs(points, lens, pairs, 0.05, nearest=True, out=res)  # builds its grid inside the capture
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert torch.equal(res.count, eager1.count) and torch.equal(res.nearest, eager1.nearest)
    first = res.ratios()
    points.copy_(pts2)
    res.count.fill_(-7)
    res.nearest.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res._cache = None
    assert torch.equal(res.count, eager2.count) and torch.equal(res.nearest, eager2.nearest)
    assert np.array_equal(res.ratios(), eager2.ratios()) and not np.array_equal(res.ratios(), first)
    assert res.src_len.cpu().tolist() == [lens_host[a] for a, _ in pairs_host]


# ---- 8. the scene tool --------------------------------------------------------------------------------------------------------------
def test_overlap_scene_tool(device, golden, tmp_path):
    from d3feat_amd import overlap
    from d3feat_amd.utils.ply import write_ply
    g, clouds = golden
    rng = np.random.default_rng(2)
    clouds = [c[:1200] for c in clouds[:4]]
    local, poses = [], []
    for k, c in enumerate(clouds):                                               # every fragment in a frame of its own, two sequences
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, 3)
        loc = ((c.astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(np.float32)
        d = tmp_path / "frag" / "room" / ("seq-01" if k < 3 else "seq-02")
        os.makedirs(d, exist_ok=True)
        write_ply(str(d / ("cloud_bin_%d.ply" % k)), [loc], ["x", "y", "z"])
        np.save(str(d / ("cloud_bin_%d.pose.npy" % k)), M)
        local.append(loc)
        poses.append(M)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "overlap_scene.py"), "--root", str(tmp_path / "frag"), "--scene", "room",
           "--downsample", "0", "--threshold", "0.05", "--out", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    # what the tool must have computed: the moved clouds (host arithmetic of stack_fragments), then the restatement
    moved = [(l.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32) for l, M in zip(local, poses)]
    upper = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    count, near = onp.overlap(moved, upper, 0.05)
    ratio = count / np.array([len(moved[a]) for a, _ in upper], np.float64)
    keep = [i for i in range(6) if ratio[i] > 0.30]
    assert rec["fragments"] == 4 and rec["pairs"] == 6 and rec["selected"] == len(keep) and 0 < len(keep) < 6
    ids = ["room/seq-01/cloud_bin_%d" % k for k in range(3)] + ["room/seq-02/cloud_bin_3"]
    with open(tmp_path / "out" / "3DMatch_train_0.000_overlap.pkl", "rb") as f:
        table = pickle.load(f)
    with open(tmp_path / "out" / "3DMatch_train_0.000_keypts.pkl", "rb") as f:
        keypts = pickle.load(f)
    keys = ["%s@%s" % (ids[upper[i][0]], ids[upper[i][1]]) for i in keep]
    assert list(table) == keys and list(keypts) == keys
    for i, key in zip(keep, keys):
        q = np.nonzero(near[i] >= 0)[0]
        assert table[key] == ratio[i] and keypts[key].dtype == np.int32 and np.array_equal(keypts[key], np.stack([q, near[i][q]], 1))
