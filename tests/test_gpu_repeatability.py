"""Keypoint repeatability on the GPU (d3f_repeatability_pairs, registration.repeatability_pairs): every pair at every keypoint count
in one call, against

  1. what the reference's own Python computed (tests/golden/repeatability.npz), both conventions: counts exactly, scene averages
     within 1e-12 (a sum of at most 15 ratios in double);
  2. the float64 numpy restatement (tests/repeatability_np.py: per count, slice, move, all distances, column minimum -- not the
     prefix walk of the kernel), every count equal: all pairs of scene(3, K=512), empty / short / missing blocks, counts on both
     sides of the 256-row passes and of the row counts, 1024-row blocks, K beyond D3F_PAIRS_KMAX;
  3. planted neighbours that must count from one keypoint count on and not before (the prefix rule);
  4. a distance that equals the threshold exactly in binary (strict comparison);
  5. both conventions with poses that are inverses of each other;
  6. 5000 pairs (two entry-point calls, totals added up);
  7. capture in a HIP graph, replay on other data;
  8. blocks as keypoints.topk_records makes them;
  9. tools/repeatability_scene.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import repeatability_np as rnp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

COUNTS = (4, 8, 16, 32, 64, 128, 256, 512)
ODD_COUNTS = (1, 3, 100, 257, 300, 511, 512)


def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, 3)
    return M


def _run(device, blocks, pairs, gts, counts, thr, moved, K=None, **kw):
    """repeatability_pairs on host blocks -> the result; blocks may have any number of columns >= 3 (all the same)."""
    from d3feat_amd import registration as reg
    kp, count = reg.stack_keypoints(blocks, K, device=device)
    return reg.repeatability_pairs(kp, count, torch.tensor(np.asarray(pairs).reshape(-1, 2), dtype=torch.int32, device=device),
                                   np.asarray(gts, np.float64), num_keypts=counts, distance_threshold=thr, moved=moved, **kw)


def _check(res, want):
    got = res.repeat.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert np.array_equal(res.totals.cpu().numpy(), want.sum(0))


@pytest.fixture(scope="module")
def scene512():
    """scene(3, K=512): 8 blocks, 28 pairs, gt target -> source; plus an empty block (8), block 1 cut to its best 300 rows (9), two
    rows (10), and pairs with them, a self pair and indices outside the blocks."""
    from d3feat_amd.utils.synthetic import scene
    blocks, poses = scene(3, K=512)
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)]
    gts = [np.linalg.inv(poses[a]) @ poses[b] for a, b in pairs]
    blocks = blocks + [blocks[0][:0], blocks[1][-300:], blocks[5][-2:]]
    rng = np.random.default_rng(11)
    extra = [(0, 0), (8, 3), (3, 8), (9, 4), (4, 9), (9, 9), (10, 1), (1, 10), (-1, 2), (2, -1), (11, 2), (2, 3)]
    pairs = pairs + extra
    gts = gts + [np.eye(4), _pose(rng), _pose(rng), np.linalg.inv(poses[1]) @ poses[4], np.linalg.inv(poses[4]) @ poses[1], np.eye(4),
                 np.linalg.inv(poses[5]) @ poses[1], np.linalg.inv(poses[1]) @ poses[5], np.eye(4), np.eye(4), np.eye(4), np.eye(4)]
    return blocks, poses, pairs, np.array(gts)


# ---- 1. the reference's own figures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gt_key,moved", [("3dmatch", "gt_target_to_source", "target"), ("kitti", "gt_source_to_target", "source")])
def test_fixture_of_the_reference(device, name, gt_key, moved):
    from d3feat_amd import registration as reg
    g = np.load(os.path.join(GOLDEN, "repeatability.npz"))
    kw = reg.REPEATABILITY_3DMATCH if name == "3dmatch" else reg.REPEATABILITY_KITTI
    assert kw["moved"] == moved and kw["distance_threshold"] == float(g["threshold_" + name])
    listed = g["listed"]
    kp, count = torch.from_numpy(g["kp"]).to(device), torch.from_numpy(g["count"]).to(device)
    pairs = torch.from_numpy(g["pairs"][listed]).to(device)
    res = reg.repeatability_pairs(kp, count, pairs, g[gt_key][listed], num_keypts=reg.REPEATABILITY_COUNTS, **kw)
    want = np.rint(g["ratios_" + name][listed] * np.asarray(COUNTS)).astype(np.int64)
    _check(res, want)
    assert res.totals.dtype == torch.int64 and res.repeat.is_cuda
    assert np.array_equal(res.ratios(), want / np.asarray(COUNTS, np.float64))
    assert np.abs(res.scene() - g["scene_" + name]).max() <= 1e-12
    # every pair, listed or not; the matrices as a [P, 4, 4] device tensor
    res_all = reg.repeatability_pairs(kp, count, torch.from_numpy(g["pairs"]).to(device), torch.from_numpy(g[gt_key]).to(device), **kw)
    _check(res_all, np.rint(g["ratios_" + name] * np.asarray(COUNTS)).astype(np.int64))


# ---- 2. the restatement ---------------------------------------------------------------------------------------------------------
def test_equal_to_the_restatement_on_every_pair(device, scene512):
    blocks, _, pairs, gts = scene512
    res = _run(device, blocks, pairs, gts, ODD_COUNTS, 0.1, "target")
    want = rnp.repeat_counts(blocks, pairs, gts, ODD_COUNTS, 0.1, "target")
    _check(res, want)
    row = dict(zip(pairs[28:], want[28:]))
    assert list(row[(0, 0)]) == list(ODD_COUNTS)                              # a self pair under the identity: min(rows, k)
    assert list(row[(9, 9)]) == [min(k, 300) for k in ODD_COUNTS]
    for empty in ((8, 3), (3, 8), (-1, 2), (2, -1), (11, 2)):
        assert not row[empty].any()
    assert want[:28].max() > 100 and (want[:28, -1] == 0).any() and row[(4, 9)][-1] > 0


def test_1024_row_blocks_and_more_rows_than_kmax(device):
    rng = np.random.default_rng(5)
    world = rng.random((1500, 3)) * 2.0
    M = _pose(rng)
    src = np.concatenate([world + rng.normal(scale=0.04, size=world.shape), rng.random((1500, 1))], 1).astype(np.float32)
    tgt_xyz = (world[rng.permutation(1500)] - M[:3, 3]) @ M[:3, :3]           # M takes the target frame into the source frame
    tgt = np.concatenate([tgt_xyz, rng.random((1500, 1))], 1).astype(np.float32)
    # one count of 1024 on 1024-row blocks, ld = 4
    blocks = [src[:1024], tgt[:1024]]
    res = _run(device, blocks, [(0, 1), (1, 0)], [M, np.linalg.inv(M)], (1024,), 0.1, "target")
    want = rnp.repeat_counts(blocks, [(0, 1), (1, 0)], [M, np.linalg.inv(M)], (1024,), 0.1, "target")
    _check(res, want)
    assert 100 < want[0, 0] < 1024
    # K = 1500 rows per block (beyond D3F_PAIRS_KMAX), the largest count 1000; one block holds 1200 rows
    blocks = [src, tgt[:1200]]
    res = _run(device, blocks, [(0, 1), (1, 0)], [M, np.linalg.inv(M)], (5, 999, 1000), 0.1, "target", K=1500)
    _check(res, rnp.repeat_counts(blocks, [(0, 1), (1, 0)], [M, np.linalg.inv(M)], (5, 999, 1000), 0.1, "target"))


# ---- 3. the prefix rule -----------------------------------------------------------------------------------------------------------
def test_planted_neighbours_count_from_their_rank_on(device):
    n = 300
    lattice = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float32)
    src, tgt = lattice * 2.0, lattice * 2.0 + np.float32(1000.0)             # 2 m apart inside a block, the blocks 1 km apart
    row = lambda rank: n - 1 - rank                                           # rank 0 is the LAST row
    tgt[row(10)] = src[row(100)] + np.float32([0.01, 0, 0])                    # needs source rank 100: k >= 101
    tgt[row(200)] = src[row(0)] + np.float32([0, 0.01, 0])                     # the target's own rank: k >= 201
    counts = (11, 100, 101, 200, 201, 300)
    res = _run(device, [src, tgt], [(0, 1)], [np.eye(4)], counts, 0.1, "target")
    assert res.repeat.cpu().tolist() == [[0, 0, 1, 1, 2, 2]]
    _check(res, rnp.repeat_counts([src, tgt], [(0, 1)], [np.eye(4)], counts, 0.1, "target"))


# ---- 4. the comparison is strict --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", ["target", "source"])
def test_distance_equal_to_the_threshold_does_not_count(device, moved):
    below = np.nextafter(np.float32(0.5), np.float32(0))
    blocks = [np.zeros((1, 3), np.float32), np.float32([[0.5, 0, 0]]), np.float32([[below, 0, 0]]), np.float32([[0.5, 0, 0], [0, below, 0]])]
    pairs = [(0, 1), (0, 2), (0, 3)]
    res = _run(device, blocks, pairs, [np.eye(4)] * 3, (2,), 0.5, moved)
    assert res.repeat.cpu().tolist() == [[0], [1], [1]]                       # d2 == thr2 exactly: not closer
    assert res.totals.cpu().tolist() == [2]


# ---- 5. both conventions ----------------------------------------------------------------------------------------------------------
def test_source_moved_with_the_inverse_pose(device, scene512):
    blocks, poses, pairs, gts = scene512
    blocks, pairs, gts = blocks[:8], pairs[:28], gts[:28]
    inv = np.array([np.linalg.inv(M) for M in gts])
    res_s = _run(device, blocks, pairs, inv, COUNTS, 0.1, "source")
    want_s = rnp.repeat_counts(blocks, pairs, inv, COUNTS, 0.1, "source")
    _check(res_s, want_s)
    _check(_run(device, blocks, pairs, gts, COUNTS, 0.1, "target"), rnp.repeat_counts(blocks, pairs, gts, COUNTS, 0.1, "target"))
    assert want_s.sum() > 1000
    # the wrong convention for these poses is another computation
    assert not np.array_equal(rnp.repeat_counts(blocks, pairs, gts, COUNTS, 0.1, "source"), want_s)


# ---- 6. chunking ------------------------------------------------------------------------------------------------------------------
def test_5000_pairs_in_one_call(device):
    from d3feat_amd import registration as reg
    from d3feat_amd.utils.synthetic import scene
    assert reg.PAIRS_PER_CALL == 4096
    blocks, poses = scene(3, K=8)
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)]
    gts = np.array([np.linalg.inv(poses[a]) @ poses[b] for a, b in pairs])
    want = rnp.repeat_counts(blocks, pairs, gts, (2, 8), 0.5, "target")
    assert want.sum() > 20
    rep = (5000 + 27) // 28
    many, many_gt = (pairs * rep)[:5000], np.tile(gts, (rep, 1, 1))[:5000]
    res = _run(device, blocks, many, many_gt, (2, 8), 0.5, "target")
    _check(res, np.tile(want, (rep, 1))[:5000])
    assert np.abs(res.scene() - np.tile(want, (rep, 1))[:5000].sum(0) / (np.array([2.0, 8.0]) * 5000)).max() <= 1e-12


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_in_a_hip_graph_and_replay_on_other_data(device):
    from d3feat_amd import registration as reg
    from d3feat_amd.utils.synthetic import scene
    data = []
    for seed in (3, 4):
        blocks, poses = scene(seed, n_frag=5, K=300)
        blocks[seed] = blocks[seed][-(100 * seed - 90):]                       # block 3 of scene 3 keeps 210 rows, scene 4 is whole
        kp, count = reg.stack_keypoints(blocks, 300, device=device)
        pairs = reg.scene_pairs(5, device=device)
        gt = torch.from_numpy(np.array([(np.linalg.inv(poses[a]) @ poses[b])[:3] for a, b in pairs.cpu().tolist()])).to(device)
        data.append((blocks, kp, count, pairs, gt))
    (_, kp3, count3, pairs, gt3), (_, kp4, count4, _, gt4) = data
    assert gt3.dtype == torch.float64 and not torch.equal(count3, count4)
    counts = (5, 100, 256, 300)
    eager3 = reg.repeatability_pairs(kp3, count3, pairs, gt3, num_keypts=counts)
    eager4 = reg.repeatability_pairs(kp4, count4, pairs, gt4, num_keypts=counts)
    assert not torch.equal(eager3.repeat, eager4.repeat)
    kp, count, gt = kp3.clone(), count3.clone(), gt3.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        res = reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts)         # eager warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=counts, out=res)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert torch.equal(res.repeat, eager3.repeat) and torch.equal(res.totals, eager3.totals)
    first = res.scene()
    kp.copy_(kp4)
    count.copy_(count4)
    gt.copy_(gt4)
    res.repeat.fill_(-7)
    res.totals.fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res._cache = None
    assert torch.equal(res.repeat, eager4.repeat) and torch.equal(res.totals, eager4.totals)
    assert np.array_equal(res.scene(), eager4.scene()) and not np.array_equal(res.scene(), first)
    with pytest.raises(ValueError):
        reg.repeatability_pairs(kp, count, pairs, gt, num_keypts=(5, 100), out=res)


# ---- 8. blocks of topk_records ----------------------------------------------------------------------------------------------------
def test_blocks_of_topk_records_go_in_as_they_are(device):
    from d3feat_amd import keypoints
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(9)
    world = rng.random((400, 3)).astype(np.float64)
    M = _pose(rng)
    recs = []
    for f in range(2):
        xyz = world + rng.normal(scale=0.02, size=world.shape)
        if f == 1:
            xyz = (xyz - M[:3, 3]) @ M[:3, :3]
        score = (rng.permutation(400) + rng.random(400) * 0.5) / 400.0       # distinct scores, a different order in each block
        recs.append(np.concatenate([xyz, rng.standard_normal((400, 16)), score[:, None]], 1).astype(np.float32))
    dev_blocks, host_blocks = [], []
    for rec in recs:
        kp, cnt = keypoints.topk_records(torch.from_numpy(rec).to(device), 64)
        assert cnt.tolist() == [64]
        dev_blocks.append(kp[0])
        host_blocks.append(rec[np.argsort(rec[:, -1], kind="stable")[-64:]])
    kp, count = reg.stack_keypoints(dev_blocks)
    assert kp.is_cuda and tuple(kp.shape) == (2, 64, 20)
    pairs = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32, device=device)
    gts = np.array([M, np.linalg.inv(M)])
    counts = (4, 16, 63, 64)
    res = reg.repeatability_pairs(kp, count, pairs, gts, num_keypts=counts, distance_threshold=0.1)
    want = rnp.repeat_counts(host_blocks, [(0, 1), (1, 0)], gts, counts, 0.1, "target")
    _check(res, want)
    assert 0 < want[0, -1] < 64


# ---- 9. the scene tool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3dmatch", "kitti"])
def test_repeatability_scene_tool(device, tmp_path, name):
    from d3feat_amd.utils import results
    g = np.load(os.path.join(GOLDEN, "repeatability.npz"))
    root = str(tmp_path / "results")
    for f, n in enumerate(g["count"]):
        xyz = g["kp"][f, :n]
        results.save_3dmatch_keypoints(root, "room/seq-01/cloud_bin_%d.ply" % f, np.concatenate([xyz, np.zeros((n, 2), np.float32)], 1))
    gt_path = tmp_path / "gt.log"
    if name == "3dmatch":
        gt_path.write_text(str(g["gt_log"]))
    else:                                                                         # the same pairs, source -> target matrices
        with open(gt_path, "w") as f:
            for (a, b), M in zip(g["pairs"][g["listed"]].tolist(), g["gt_source_to_target"][g["listed"]]):
                f.write("%d\t %d\t 6\n" % (a, b) + "".join("\t ".join(repr(float(v)) for v in row) + "\t \n" for row in M))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "repeatability_scene.py"), "--root", root, "--scene", "room", "--gt", str(gt_path)]
    out = subprocess.run(cmd + (["--kitti"] if name == "kitti" else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    rec = json.loads(lines[-1])
    assert rec["pairs"] == int(g["listed"].sum()) and rec["fragments"] == 6 and rec["num_keypts"] == list(COUNTS)
    assert np.abs(np.asarray(rec["repeatability"]) - g["scene_" + name]).max() <= 1e-12
    assert lines[0] == "Average Repeatability at num_keypts = 4: %s" % rec["repeatability"][0] and len(lines) == 9
