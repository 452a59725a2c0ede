"""Feature matching on the GPU (d3f_match_pairs, registration.match_pairs): every pair at every keypoint count in one call, against

  1. what the reference's own Python computed (tests/golden/matching.npz: counts up to 1536 rows, a short block), exactly -- the
     fixture was written only with its margins met (tools/make_golden_matching.py);
  2. register_pairs(..., num_keypts=k, gt=gt) for every count k <= 1024, bit for bit (mutual_count and gt_inliers), and
     build_correspondence on the tails: 300-row blocks, counts on both sides of the 128-row tile and of the 256-row pass;
  3. planted exact ties (duplicate descriptor rows at ranks on either side of a count boundary, in the target and in the source): the
     lowest row index wins at every count;
  4. the float64 restatement (tests/matching_np.py) on 1300-row blocks at counts on both sides of 1024, after asserting its margins;
  5. descriptors of 16 and 64 floats;
  6. unequal, empty and missing blocks, pair indices outside the blocks;
  7. more pairs than one entry-point call takes (PAIRS_PER_CALL patched);
  8. capture in a HIP graph, replay on other data with out=;
  9. tools/matching_scene.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import matching_np as mnp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TILE_COUNTS = (1, 7, 127, 128, 129, 255, 256, 257, 300)


def _unit(rng, n, C):
    d = rng.standard_normal((n, C))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _inputs(device, blocks, pairs, gts=None, K=None):
    from d3feat_amd import registration as reg
    kp, count = reg.stack_keypoints(blocks, K, device=device)
    pairs = torch.tensor(np.asarray(pairs).reshape(-1, 2), dtype=torch.int32, device=device)
    gt = None if gts is None else torch.from_numpy(np.ascontiguousarray(np.asarray(gts, np.float64)[:, :3], dtype=np.float32)).to(device)
    return kp, count, pairs, gt


def _by_register_pairs(kp, count, pairs, gt, counts):
    """(mutual_count, gt_inliers) i32[P, n] from one register_pairs call per count (no RANSAC iterations: only its matching stage)"""
    from d3feat_amd import registration as reg
    cols = [reg.register_pairs(kp, count, pairs, 0.05, num_keypts=k, gt=gt, max_iteration=0, max_validation=1) for k in counts]
    return torch.stack([c.mutual_count for c in cols], 1).cpu().numpy(), torch.stack([c.gt_inliers for c in cols], 1).cpu().numpy()


def _check(res, mutual, inliers):
    got_m, got_g = res.mutual_count.cpu().numpy(), res.gt_inliers.cpu().numpy()
    assert got_m.dtype == got_g.dtype == np.int32 and got_m.shape == got_g.shape == np.asarray(mutual).shape
    assert np.array_equal(got_m, mutual), np.argwhere(got_m != mutual)[:10]
    assert np.array_equal(got_g, inliers), np.argwhere(got_g != inliers)[:10]


def _scene(seed, n_frag, K):
    from d3feat_amd.utils.synthetic import scene
    blocks, poses = scene(seed, n_frag=n_frag, K=K)
    pairs = [(a, b) for a in range(n_frag) for b in range(n_frag) if a != b]
    gts = np.array([np.linalg.inv(poses[a]) @ poses[b] for a, b in pairs])
    return blocks, pairs, gts


# ---- 1. the reference's own figures ---------------------------------------------------------------------------------------------------
def test_fixture_of_the_reference(device):
    from d3feat_amd import registration as reg
    g = np.load(os.path.join(GOLDEN, "matching.npz"))
    assert float(g["gap"]) >= 8.0 * float(g["err"]) and float(g["band"]) >= 8.0 * float(g["point_err"])
    kp, count, pairs = (torch.from_numpy(g[k]).to(device) for k in ("kp", "count", "pairs"))
    gt = torch.from_numpy(g["gt_target_to_source"][:, :3].astype(np.float32)).to(device)
    counts = tuple(int(k) for k in g["num_keypts"])
    res = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, distance_threshold=float(g["threshold"]))
    _check(res, g["mutual_count"], g["gt_inliers"])
    assert res.mutual_count.is_cuda and res.num_keypts == (250, 1000, 1536)
    assert np.array_equal(res.ratios(), g["gt_inliers"] / g["mutual_count"])
    # without gt: the mutual counts alone
    res = reg.match_pairs(kp, count, pairs, num_keypts=counts)
    assert res.gt_inliers is None and np.array_equal(res.mutual_count.cpu().numpy(), g["mutual_count"])


# ---- 2. the contract with register_pairs and build_correspondence -----------------------------------------------------------------
def test_equal_to_register_pairs_and_build_correspondence(device):
    from d3feat_amd import registration as reg
    blocks, pairs, gts = _scene(3, 4, 300)
    assert all(len(b) == 300 for b in blocks) and len(pairs) == 12
    kp, count, dpairs, gt = _inputs(device, blocks, pairs, gts)
    res = reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=TILE_COUNTS)
    want_m, want_g = _by_register_pairs(kp, count, dpairs, gt, TILE_COUNTS)
    _check(res, want_m, want_g)
    assert want_g.max() > 20 and (want_m[:, -1] > 50).all() and (want_m[:, 0] <= 1).all()
    for p in (0, 5, 7):                                          # the mutual set is build_correspondence's on the two tails
        a, b = pairs[p]
        for c, k in enumerate(TILE_COUNTS):
            corr = reg.build_correspondence(kp[a, 300 - k:, 3:35], kp[b, 300 - k:, 3:35])
            assert len(corr) == want_m[p, c], (p, k)


# ---- 3. exact ties -------------------------------------------------------------------------------------------------------------------
def test_planted_ties_keep_the_lowest_row_at_every_count(device):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(21)
    n, counts = 300, (100, 200, 300)
    row = lambda rank: n - 1 - rank                               # rank 0 is the LAST row
    S = np.concatenate([rng.random((n, 3)), _unit(rng, n, 32), np.arange(n)[:, None]], 1).astype(np.float32)
    T = np.concatenate([rng.random((n, 3)) + 1000.0, _unit(rng, n, 32), np.arange(n)[:, None]], 1).astype(np.float32)
    far = np.float32([500, 500, 500])
    # A: target ranks 50 and 150 carry the descriptor of source rank 10.  At 100 only rank 50 exists (far away: no inlier); from 200 on
    #    both do and the LOWER row, rank 150, must win (it sits on the source point: an inlier).
    for rank, xyz in ((50, far), (150, S[row(10), :3])):
        T[row(rank), 3:35], T[row(rank), :3] = S[row(10), 3:35], xyz
    # B: source ranks 30 and 250 carry the descriptor of target rank 20.  Up to 200 only rank 30 exists (on the target point: an
    #    inlier); at 300 the target's nearest is the LOWER row, rank 250 (far away), and rank 30 is no longer mutual.
    T[row(20), :3] = rng.random(3)
    for rank, xyz in ((30, T[row(20), :3]), (250, far)):
        S[row(rank), 3:35], S[row(rank), :3] = T[row(20), 3:35], xyz
    # C: target ranks 5 and 8, the same side of every boundary, carry the descriptor of source rank 3: rank 8 (an inlier) at every count
    for rank, xyz in ((5, far), (8, S[row(3), :3])):
        T[row(rank), 3:35], T[row(rank), :3] = S[row(3), 3:35], xyz
    kp, count, pairs, gt = _inputs(device, [S, T], [(0, 1)], [np.eye(4)])
    res = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts)
    assert res.gt_inliers.cpu().tolist() == [[2, 3, 2]]          # A: 0 1 1, B: 1 1 0, C: 1 1 1; nothing else is within 0.1 m
    _check(res, *_by_register_pairs(kp, count, pairs, gt, counts))
    for c, k in enumerate(counts):
        corr = reg.build_correspondence(kp[0, n - k:, 3:35], kp[1, n - k:, 3:35])
        assert len(corr) == int(res.mutual_count[0, c])
        local = lambda rank: k - 1 - rank                         # the row inside the tail
        have = {tuple(r) for r in corr.tolist()}
        assert (local(10), local(150 if k >= 200 else 50)) in have and (local(3), local(8)) in have
        assert (local(250 if k == 300 else 30), local(20)) in have and ((local(30), local(20)) in have) == (k < 300)


# ---- 4. above 1024 rows: the restatement -------------------------------------------------------------------------------------------
def test_1300_row_blocks_equal_the_restatement(device):
    from d3feat_amd import registration as reg
    counts = (250, 1024, 1025, 1300)
    blocks, pairs, gts = _scene(0, 2, 1300)
    assert [len(b) for b in blocks] == [1300, 1300] and pairs == [(0, 1), (1, 0)]
    m = mnp.margins(blocks, pairs, gts, counts, 0.1)
    assert mnp.margins_ok(m), m                                    # else exact equality with float64 code is no fair demand
    want_m, want_g = mnp.match_counts(blocks, pairs, gts, counts, 0.1)
    assert want_m[0, -1] > 600 and want_g[0, -1] > 100 and np.array_equal(want_m[0], want_m[1])
    kp, count, dpairs, gt = _inputs(device, blocks, pairs, gts)
    _check(reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=counts), want_m, want_g)
    # K beyond every count; one count alone
    kp2, count2, _, _ = _inputs(device, blocks, pairs, gts, K=1300)
    _check(reg.match_pairs(kp2, count2, dpairs, gt=gt, num_keypts=(1025,)), want_m[:, 2:3], want_g[:, 2:3])


# ---- 5. other descriptor widths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64])
def test_descriptors_of_16_and_64_floats(device, C):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(C)
    world, wdesc = rng.random((260, 3)), _unit(rng, 260, C)
    blocks = []
    for f, n in enumerate((200, 260)):
        sel = rng.permutation(260)[:n]
        d = wdesc[sel] + 0.05 * rng.standard_normal((n, C))
        blocks.append(np.concatenate([world[sel] + rng.normal(scale=0.003, size=(n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True),
                                      np.sort(rng.random(n))[:, None]], 1).astype(np.float32))
    pairs, counts = [(0, 1), (1, 0)], (64, 150, 257)
    kp, count, dpairs, gt = _inputs(device, blocks, pairs, [np.eye(4)] * 2)
    assert tuple(kp.shape) == (2, 260, C + 4)
    res = reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=counts)
    want_m, want_g = _by_register_pairs(kp, count, dpairs, gt, counts)
    _check(res, want_m, want_g)
    assert want_g.min() > 10 and want_m[0, 0] < want_m[0, 2]


# ---- 6. unequal, empty and missing blocks ------------------------------------------------------------------------------------------
def test_unequal_empty_and_missing_blocks(device):
    from d3feat_amd import registration as reg
    blocks, _, _ = _scene(3, 3, 300)
    blocks = [blocks[0], blocks[1][-120:], blocks[2][:0], blocks[2][-2:], blocks[2][-1:]]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (2, 2), (3, 0), (0, 3), (4, 4), (4, 1), (0, 0)]
    outside = [(-1, 0), (0, -1), (5, 1), (1, 5), (7, 9)]          # block indices outside [0, 5): no rows
    rng = np.random.default_rng(2)
    gts = np.tile(np.eye(4), (len(pairs) + len(outside), 1, 1))
    gts[:2, :3, 3] = rng.normal(scale=0.02, size=(2, 3))
    counts = (1, 2, 100, 120, 121, 128, 300)
    kp, count, dpairs, gt = _inputs(device, blocks, pairs + outside, gts)
    assert count.tolist() == [300, 120, 0, 2, 1]
    res = reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=counts)
    n = len(pairs)                                                # register_pairs' Python side indexes the counts with the pairs: in range only
    want_m, want_g = _by_register_pairs(kp, count, dpairs[:n].contiguous(), gt[:n].contiguous(), counts)
    zeros = np.zeros((len(outside), len(counts)), np.int32)
    _check(res, np.concatenate([want_m, zeros]), np.concatenate([want_g, zeros]))
    row = dict(zip(pairs, want_m))
    for empty in ((0, 2), (2, 0), (2, 2)):
        assert not row[empty].any()
    assert list(row[(0, 0)]) == list(counts) and list(row[(4, 4)]) == [1] * 7 and row[(3, 0)][0] == 1 and 1 <= row[(3, 0)].max() <= 2
    assert row[(0, 1)][-1] > 20 and row[(1, 0)][-1] == row[(0, 1)][-1]
    assert list(want_g[pairs.index((0, 0))]) == list(counts)


# ---- 7. chunking -------------------------------------------------------------------------------------------------------------------
def test_more_pairs_than_one_call_takes(device, monkeypatch):
    from d3feat_amd import registration as reg
    blocks, pairs, gts = _scene(3, 3, 60)
    pairs, gts = pairs[:5], gts[:5]
    kp, count, dpairs, gt = _inputs(device, blocks, pairs, gts)
    whole = reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=(10, 60))
    monkeypatch.setattr(reg, "PAIRS_PER_CALL", 2)                  # three entry-point calls: 2 + 2 + 1 pairs
    parts = reg.match_pairs(kp, count, dpairs, gt=gt, num_keypts=(10, 60))
    _check(parts, whole.mutual_count.cpu().numpy(), whole.gt_inliers.cpu().numpy())
    _check(parts, *_by_register_pairs(kp, count, dpairs, gt, (10, 60)))
    assert whole.mutual_count.sum() > 50


# ---- 8. capture --------------------------------------------------------------------------------------------------------------------
def test_capture_in_a_hip_graph_and_replay_on_other_data(device):
    from d3feat_amd import registration as reg
    counts, data = (5, 100, 257, 300), []
    for seed in (3, 4):
        blocks, pairs, gts = _scene(seed, 3, 300)
        blocks[1] = blocks[1][-(100 * seed - 90):]                 # 210 rows in scene 3, all 300 in scene 4
        data.append(_inputs(device, blocks, pairs, gts, K=300))
    (kp3, count3, pairs, gt3), (kp4, count4, _, gt4) = data
    assert not torch.equal(count3, count4)
    eager3 = reg.match_pairs(kp3, count3, pairs, gt=gt3, num_keypts=counts)
    eager4 = reg.match_pairs(kp4, count4, pairs, gt=gt4, num_keypts=counts)
    assert not torch.equal(eager3.mutual_count, eager4.mutual_count) and not torch.equal(eager3.gt_inliers, eager4.gt_inliers)
    kp, count, gt = kp3.clone(), count3.clone(), gt3.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        res = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts)             # eager warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=counts, out=res)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert torch.equal(res.mutual_count, eager3.mutual_count) and torch.equal(res.gt_inliers, eager3.gt_inliers)
    first = res.ratios()
    kp.copy_(kp4)
    count.copy_(count4)
    gt.copy_(gt4)
    res.mutual_count.fill_(-7)
    res.gt_inliers.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res._cache = None
    assert torch.equal(res.mutual_count, eager4.mutual_count) and torch.equal(res.gt_inliers, eager4.gt_inliers)
    assert np.array_equal(res.ratios(), eager4.ratios()) and not np.array_equal(res.ratios(), first)
    with pytest.raises(ValueError):
        reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=(5, 100), out=res)
    with pytest.raises(ValueError):
        reg.match_pairs(kp, count, pairs, num_keypts=counts, out=res)                 # made with gt


# ---- 9. the scene tool -------------------------------------------------------------------------------------------------------------
def test_matching_scene_tool(device, tmp_path):
    from d3feat_amd.utils import results
    g = np.load(os.path.join(GOLDEN, "matching.npz"))
    root = str(tmp_path / "results")
    for f, n in enumerate(g["count"]):
        results.save_3dmatch_keypoints(root, "room/seq-01/cloud_bin_%d.ply" % f, g["kp"][f, :n])
    listed = [0, 2]                                               # gt.log lists pairs (0, 1) and (1, 2)
    with open(tmp_path / "gt.log", "w") as f:
        for p in listed:
            f.write("%d\t %d\t 3\n" % tuple(g["pairs"][p]) + "".join("\t ".join(repr(float(v)) for v in r) + "\t \n"
                                                                   for r in g["gt_target_to_source"][p]))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "matching_scene.py"), "--root", root, "--scene", "room", "--gt", str(tmp_path / "gt.log"),
           "--counts", "250,1000,1536"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    rec = json.loads(lines[-1])
    assert (rec["fragments"], rec["pairs"], rec["num_keypts"], rec["gt"]) == (3, 3, [250, 1000, 1536], [2, 2, 2])
    flag = np.array([1, 0, 1])
    rows = [[[int(n) * int(fl), float("%.8f" % (n / m)) * int(fl), int(fl)] for n, m, fl in zip(g["gt_inliers"][:, c], g["mutual_count"][:, c], flag)]
            for c in range(3)]
    want_lines, table = results.matching_table((250, 1000, 1536), rows)
    assert lines[:-1] == want_lines and len(lines) == 16
    assert rec["recall"] == [table[k]["recall"] for k in (250, 1000, 1536)] == [50.0, 50.0, 50.0]
    assert rec["ave_num_inliers"] == [float(g["gt_inliers"][0, c]) for c in range(3)]
