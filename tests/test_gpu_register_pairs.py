"""Batched registration on the GPU (d3f_register_pairs, registration.register_pairs): every pair of a synthetic scene in one call.

The input is utils.synthetic.scene: 8 keypoint blocks of 250 [xyz | 32-d unit desc | score] rows cut out of one room, 28 pairs.  With
registration.EVALUATE_3DMATCH (the call of geometric_registration/evaluate.py:93-99) and seed 5 the oracle exhausts the 50 000
iterations on 27 pairs of scene(3) (10 to 733 validations) and stops early on one, (4, 6), with 1000 validations at iteration 45 592;
9 pairs register, 19 fail: both exits of the loop, success and failure, in one input.

  1. per pair the result is BIT-IDENTICAL to registration.register_keypoints (the single-pair host loop) -- no tolerance;
  2. against oracle/registration_np.py directly (float64), with the bounds tests/test_gpu_registration.py already uses; the oracle
     takes about 40 s of CPU for the 28 pairs, which is this module's time budget;
  3. ties in the descriptors go to the lowest index in both directions;
  4. the call is captured in a HIP graph and replayed on other data: no host decision between the launches;
  5. 5000 pairs in one Python call (two entry-point calls) equal the 28 results repeated;
  6. the blocks FragmentEngine(keypoints=K) returns go in as they are."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 5
RESULT_FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "nearest", "mutual",
                 "gt_inliers")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _gt(poses, pairs):
    """[P, 3, 4] float32, target -> source: inv(poses[a]) @ poses[b]."""
    return np.stack([(np.linalg.inv(poses[a]) @ poses[b])[:3] for a, b in pairs]).astype(np.float32)


def _scene_on_device(seed, device):
    from d3feat_amd import registration as reg
    from d3feat_amd.utils.synthetic import scene
    blocks, poses = scene(seed)
    kp, count = reg.stack_keypoints(blocks, 250, device=device)
    pairs = reg.scene_pairs(len(blocks), device=device)
    gt = torch.from_numpy(_gt(poses, pairs.cpu().tolist())).to(device)
    return blocks, poses, kp, count, pairs, gt


@pytest.fixture(scope="module")
def scene3(device):
    return _scene_on_device(3, device)


def _same_tensors(a, b):
    for k in RESULT_FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        if not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y):
            return False
    return True


# ---- 1. equal to the single-pair path, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("num_keypts", [None, 128])
@pytest.mark.parametrize("params", ["evaluate_3dmatch", "defaults_ransac_n_4"])
def test_equal_to_register_keypoints_bit_for_bit(device, scene3, num_keypts, params):
    from d3feat_amd import registration as reg
    blocks, poses, kp8, count8, pairs28, _ = scene3
    kw = dict(reg.EVALUATE_3DMATCH) if params == "evaluate_3dmatch" else dict(max_correspondence_distance=0.05, ransac_n=4)
    kw["seed"] = SEED
    # blocks 0..7 of the scene, 8: block 1 cut to its first 100 rows, 9: two rows only (< ransac_n)
    kp = torch.cat([kp8, kp8[1:2], kp8[5:6]]).contiguous()
    count = torch.cat([count8, torch.tensor([100, 2], dtype=torch.int32, device=device)])
    extra = [(0, 0), (8, 3), (9, 1), (1, 9)]
    pairs = torch.cat([pairs28, torch.tensor(extra, dtype=torch.int32, device=device)])
    res = reg.register_pairs(kp, count, pairs, num_keypts=num_keypts, correspondences=True, **kw)
    host_count = count.cpu().tolist()
    for p, (a, b) in enumerate(pairs.cpu().tolist()):
        got = res.host(p)
        want = reg.register_keypoints(kp[a, :host_count[a]], kp[b, :host_count[b]], num_keypts=num_keypts, device=device, **kw)
        where = "pair %d = (%d, %d)" % (p, a, b)
        assert np.array_equal(_bits(got["transformation"]), _bits(want["transformation"])), where
        assert got["fitness"] == want["fitness"] and got["inlier_rmse"] == want["inlier_rmse"], where
        assert got["validations"] == want["validations"], where
        assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), where
        assert got["correspondence_set"].dtype == want["correspondence_set"].dtype == np.int64
        assert np.array_equal(got["correspondences"], want["correspondences"]), where
        if min(host_count[a], host_count[b]) < kw["ransac_n"]:
            assert got["validations"] == 0 and got["iterations"] == 0 and got["best_iteration"] == -1, where
            assert np.array_equal(got["transformation"], np.eye(4)) and got["fitness"] == 0.0, where
            assert len(got["correspondences"]) > 0, where              # the mutual pairs are still computed
    # the self pair registers onto itself
    self_pair = res.host(28)
    assert self_pair["fitness"] == 1.0 and np.abs(self_pair["transformation"] - np.eye(4)).max() < 1e-5
    assert np.array_equal(self_pair["correspondences"][:, 0], self_pair["correspondences"][:, 1])


@pytest.mark.parametrize("C,K,num_keypts", [(16, 300, None), (64, 1024, None), (64, 1500, 1000)])
def test_other_descriptor_widths_and_long_blocks(device, C, K, num_keypts):
    """C = 16 / 64 and blocks up to D3F_PAIRS_KMAX rows (several row passes and LDS tiles per pair), different counts per block."""
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(C + K)
    base = rng.uniform(-1, 1, (K, 3))
    desc = rng.standard_normal((K, C))
    blocks = []
    for f in range(3):
        n = K - 37 * f
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        sel = rng.permutation(K)[:n]
        d = desc[sel] + 0.05 * rng.standard_normal((n, C))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        blocks.append(np.concatenate([base[sel] @ q.T + rng.uniform(-1, 1, 3), d, np.sort(rng.random(n))[:, None]], 1).astype(np.float32))
    kp, count = reg.stack_keypoints(blocks, K, device=device)
    pairs = torch.tensor([(0, 1), (2, 0), (1, 2), (2, 2)], dtype=torch.int32, device=device)
    kw = dict(max_correspondence_distance=0.05, ransac_n=4, max_iteration=20000, max_validation=50, seed=11)
    res = reg.register_pairs(kp, count, pairs, num_keypts=num_keypts, correspondences=True, **kw)
    for p, (a, b) in enumerate(pairs.cpu().tolist()):
        got = res.host(p)
        want = reg.register_keypoints(kp[a, :len(blocks[a])], kp[b, :len(blocks[b])], num_keypts=num_keypts, device=device, **kw)
        assert np.array_equal(_bits(got["transformation"]), _bits(want["transformation"])), p
        assert (got["fitness"], got["inlier_rmse"], got["validations"]) == (want["fitness"], want["inlier_rmse"], want["validations"]), p
        assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), p
        assert np.array_equal(got["correspondences"], want["correspondences"]), p
        # the motion between two copies of one cloud is found (at least 2/3 of the source rows have their twin among the target rows)
        assert got["validations"] == 50 and got["fitness"] > 0.4, p


def test_rejected_sizes_name_the_single_pair_path(device):
    from d3feat_amd import registration as reg
    kp = torch.zeros((2, 1100, 36), device=device)
    count = torch.zeros((2,), dtype=torch.int32, device=device)
    pairs = torch.zeros((1, 2), dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="register_keypoints"):
        reg.register_pairs(kp, count, pairs, 0.05)
    with pytest.raises(ValueError, match="register_keypoints"):
        reg.register_pairs(kp[:, :100, :28].contiguous(), count, pairs, 0.05)         # 24-d descriptors
    with pytest.raises(ValueError, match="register_keypoints"):
        reg.register_pairs(kp[:, :100].contiguous(), count, pairs, 0.05, ransac_n=9)
    res = reg.register_pairs(kp, count, pairs, 0.05, num_keypts=250)                   # empty blocks: nothing to register
    h = res.host(0)
    assert h["validations"] == 0 and h["best_iteration"] == -1 and np.array_equal(h["transformation"], np.eye(4))
    assert int(res.mutual_count[0]) == 0


# ---- 2. against the oracle --------------------------------------------------------------------------------------------------------
def test_against_the_oracle(device, scene3):
    """Figures of this input (scene(3), seed 5), from the oracle on the CPU: validations 10..1000, iterations 45592 (pair (4, 6)) or
    50000, mutual counts 108..139, gt_inliers 0..72."""
    from d3feat_amd import registration as reg
    from oracle import registration_np as onp
    blocks, poses, kp, count, pairs, gt = scene3
    kw = dict(reg.EVALUATE_3DMATCH, seed=SEED)
    res = reg.register_pairs(kp, count, pairs, gt=gt, correspondences=True, **kw)
    same_winner, near_threshold, early = 0, 0, 0
    for p, (a, b) in enumerate(pairs.cpu().tolist()):
        where = "pair %d = (%d, %d)" % (p, a, b)
        src, tgt = blocks[a][:, :3], blocks[b][:, :3]
        sd, td = blocks[a][:, 3:35], blocks[b][:, 3:35]
        # precondition (asserted, never skipped): the fp32 device pick of every nearest descriptor is the float64 pick; if this
        # fails the input is wrong for this test
        for A, B in ((sd, td), (td, sd)):
            assert np.array_equal(reg.feature_nn(A, B, device=device).cpu().numpy(), onp.feature_nn(A, B)[0]), where
        want = onp.ransac_feature_matching(src, tgt, sd, td, kw["max_correspondence_distance"], ransac_n=kw["ransac_n"],
                                           edge_similarity=kw["edge_similarity"], checker_distance=kw["checker_distance"],
                                           max_iteration=kw["max_iteration"], max_validation=kw["max_validation"], seed=SEED)
        got = res.host(p)
        Ns = len(src)
        print(where, "iterations", got["iterations"], "validations", got["validations"], "best", got["best_iteration"],
              want.get("best_iteration"), "fitness", got["fitness"], want["fitness"], "mutual", len(got["correspondences"]),
              "gt_inliers", got["gt_inliers"])
        assert got["iterations"] == want["iterations"] and got["validations"] == want["validations"], where
        early += got["iterations"] < kw["max_iteration"]
        assert abs(got["fitness"] - want["fitness"]) <= 1.0 / Ns + 1e-9, where       # a point on the radius may flip
        M = got["transformation"]
        rescored = onp.evaluate(src, tgt, M[:3, :3], M[:3, 3], kw["max_correspondence_distance"])[0]
        assert rescored >= round(want["fitness"] * Ns) - 1, where
        if got["best_iteration"] == want.get("best_iteration", -1):
            same_winner += 1
            assert np.abs(M - want["transformation"]).max() < 1e-3, where
        # mutual pairs and their inliers under the ground truth, float64
        corr = onp.build_correspondence(sd.astype(np.float64), td.astype(np.float64))
        assert np.array_equal(got["correspondences"], corr), where
        G = np.linalg.inv(poses[a]) @ poses[b]
        moved = tgt[corr[:, 1]].astype(np.float64) @ G[:3, :3].T + G[:3, 3]
        dist = np.sqrt(np.sum(np.power(src[corr[:, 0]].astype(np.float64) - moved, 2), axis=1))
        close = int(np.sum(np.abs(dist - 0.10) <= 1e-5))
        near_threshold += close
        assert abs(got["gt_inliers"] - int(np.sum(dist < 0.10))) <= close, where
        assert got["inlier_ratio"] == got["gt_inliers"] / len(corr), where
    print("same winner on %d of 28 pairs; %d correspondences within 1e-5 of the gt threshold; %d early exits"
          % (same_winner, near_threshold, early))
    assert same_winner >= 25
    assert early >= 1                                                          # both exits of the loop were taken


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------
def test_descriptor_ties_take_the_lowest_index_in_both_directions(device):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(0)
    d = rng.standard_normal((300, 32)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perm = rng.permutation(300)
    xyz = rng.uniform(-1, 1, (600, 3)).astype(np.float32)
    score = np.sort(rng.random(600).astype(np.float32))[:, None]
    # every descriptor twice in BOTH blocks: the first copy must win as source -> target and as target -> source
    A = np.concatenate([xyz, np.concatenate([d, d]), score], 1)
    B = np.concatenate([xyz[::-1], np.concatenate([d[perm], d[perm]]), score], 1)
    kp, count = reg.stack_keypoints([A, B], 600, device=device)
    pairs = torch.tensor([(0, 1), (1, 0)], dtype=torch.int32, device=device)
    res = reg.register_pairs(kp, count, pairs, 0.05, max_iteration=512, max_validation=8, correspondences=True)
    inv = np.argsort(perm)
    m = res.host(0)["correspondences"]
    assert len(m) == 300 and np.array_equal(m[:, 0], np.arange(300)) and np.array_equal(m[:, 1], inv)
    m = res.host(1)["correspondences"]
    assert len(m) == 300 and np.array_equal(m[:, 0], np.arange(300)) and np.array_equal(m[:, 1], perm)
    assert np.array_equal(res.host(0)["correspondences"], reg.build_correspondence(A[:, 3:35], B[:, 3:35], device=device))


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_in_a_hip_graph_and_replay_on_other_data(device, scene3):
    from d3feat_amd import ops
    from d3feat_amd import registration as reg
    _, _, kp3, count, pairs, gt3 = scene3
    _, _, kp4, count4, _, gt4 = _scene_on_device(4, device)
    assert torch.equal(count, count4)
    kw = dict(reg.EVALUATE_3DMATCH, seed=SEED, correspondences=True)
    eager3 = reg.register_pairs(kp3, count, pairs, gt=gt3, **kw)
    eager4 = reg.register_pairs(kp4, count, pairs, gt=gt4, **kw)
    assert not _same_tensors(eager3, eager4)
    kp, gt = kp3.clone(), gt3.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            res = reg.register_pairs(kp, count, pairs, gt=gt, **kw)              # eager warm-up on this stream (scratch)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            reg.register_pairs(kp, count, pairs, gt=gt, out=res, **kw)
    keep = pw.kept
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same_tensors(res, eager3)
    kp.copy_(kp4)
    gt.copy_(gt4)
    for k in RESULT_FIELDS:
        getattr(res, k).fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res._cache = None
    assert _same_tensors(res, eager4) and not _same_tensors(res, eager3)
    assert res.host(5)["validations"] == eager4.host(5)["validations"]
    del keep


# ---- 5. chunking ------------------------------------------------------------------------------------------------------------------
def test_5000_pairs_in_one_call(device, scene3):
    from d3feat_amd import registration as reg
    _, _, kp, count, pairs, gt = scene3
    assert reg.PAIRS_PER_CALL == 4096
    kw = dict(reg.EVALUATE_3DMATCH, seed=SEED, correspondences=True)
    want = reg.register_pairs(kp, count, pairs, gt=gt, **kw)
    rep = (5000 + 27) // 28
    many, many_gt = pairs.repeat(rep, 1)[:5000].contiguous(), gt.repeat(rep, 1, 1)[:5000].contiguous()
    got = reg.register_pairs(kp, count, many, gt=many_gt, **kw)
    for k in RESULT_FIELDS:
        x, y = getattr(got, k), getattr(want, k)
        y = y.repeat(rep, *([1] * (y.dim() - 1)))[:5000]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k


# ---- 6. engine hand-over ------------------------------------------------------------------------------------------------------------
def test_engine_keypoint_blocks_go_in_as_they_are(device):
    from d3feat_amd import registration as reg
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    from d3feat_amd.utils.synthetic import room_fragment
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    limits = np.asarray([37, 35, 36, 38, 38], np.int32)
    eng = FragmentEngine(cfg, W, limits, device=device, keypoints=64, raw_cap=45000, n0_cap=14000, slots=1)
    eng.submit(0, torch.from_numpy(room_fragment(301, n_raw=40000, edge=1.0)).to(device))
    block = eng.fetch(0, keypoints=True)
    assert eng.fallbacks == 0 and tuple(block.shape) == (64, 36)
    kp, count = reg.stack_keypoints([block], 64)
    assert kp.is_cuda and tuple(kp.shape) == (1, 64, 36) and count.tolist() == [64]
    res = reg.register_pairs(kp, count, torch.zeros((1, 2), dtype=torch.int32, device=device), seed=SEED, **reg.EVALUATE_3DMATCH)
    h = res.host(0)
    assert h["fitness"] == 1.0 and h["validations"] > 0
    assert np.abs(h["transformation"] - np.eye(4)).max() < 1e-5
    assert np.array_equal(h["correspondence_set"], np.stack([np.arange(64), np.arange(64)], 1))


# ---- the scene tool ---------------------------------------------------------------------------------------------------------------
def test_register_scene_tool_writes_the_files_of_evaluate_py(device, scene3, tmp_path):
    """tools/register_scene.py on the files save_3dmatch_keypoints writes for scene(3), with a gt.log that lists the pairs of even
    a + b: one .rt.txt per pair, gt_flag and counts as register_pairs gives them, .log blocks for the listed pairs only."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from d3feat_amd import registration as reg
    from d3feat_amd.utils import results
    blocks, poses, kp, count, pairs, gt = scene3
    root, out = str(tmp_path / "results"), str(tmp_path / "out")
    for f, b in enumerate(blocks):
        results.save_3dmatch_keypoints(root, "synth/seq-01/cloud_bin_%d.ply" % f, b)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    listed = [p for p in host_pairs if (p[0] + p[1]) % 2 == 0]
    with open(tmp_path / "gt.log", "w") as f:
        for a, b in listed:
            G = np.linalg.inv(poses[a]) @ poses[b]
            f.write("%d\t%d\t%d\n" % (a, b, len(blocks)))
            for r in range(4):
                f.write("\t".join(repr(float(x)) for x in G[r]) + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "register_scene.py"), "--root", root, "--scene", "synth", "--gt",
                          str(tmp_path / "gt.log"), "--seed", str(SEED), "--out", out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["fragments"] == 8 and line["pairs"] == 28 and line["gt"] == len(listed)
    # the same call here; the tool's gt is the float32 of the doubles the log holds, as here
    res = reg.register_pairs(kp, count, pairs, gt=gt, seed=SEED, **reg.EVALUATE_3DMATCH)
    inl, mutual = res.gt_inliers.cpu().numpy(), res.mutual_count.cpu().numpy()
    rows = []
    for p, (a, b) in enumerate(host_pairs):
        text = open(os.path.join(out, "cloud_bin_%d_cloud_bin_%d.rt.txt" % (a, b))).read()
        if (a, b) in listed:
            assert text == "cloud_bin_%d\tcloud_bin_%d\t%d\t%.8f\t1" % (a, b, inl[p], inl[p] / mutual[p]), text
        else:
            assert text == "cloud_bin_%d\tcloud_bin_%d\t0\t%.8f\t0" % (a, b, 0.0), text
        nums = text.split("\t")[2:5]
        rows.append([int(nums[0]), float(nums[1]), int(nums[2])])
    want = results.feature_matching_recall(rows, 0.05)
    assert all(line[k] == want[k] for k in want)
    back = results.read_gt_log(os.path.join(out, "D3Feat.log"))
    assert list(back) == ["%d_%d" % p for p in listed]
    for p, (a, b) in enumerate(host_pairs):
        if (a, b) in listed:
            M = np.eye(4)
            M[:3] = res.T[p].cpu().numpy().astype(np.float64)
            assert np.array_equal(back["%d_%d" % (a, b)], np.linalg.inv(M))
