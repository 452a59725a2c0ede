"""RANSAC registration of every pair at every keypoint count on the GPU (d3f_register_pairs_counts, registration.register_pairs_counts).

The input is utils.synthetic.scene(3, n_frag=4, K=1500): four keypoint blocks of 1500 [xyz | 32-d unit desc | score] rows cut out of
one room, with registration.EVALUATE_3DMATCH at max_iteration=20000, max_validation=100, seed 5.  The definition is an equality with
code the project already has, so nothing here has a tolerance except the comparison with the float64 oracle:

  1. per pair and count BIT-IDENTICAL to registration.register_keypoints(num_keypts=k), for k <= 1024 to register_pairs(num_keypts=k)
     on every tensor, and to match_pairs on the two matching counts; counts on both sides of the old 1024-row limit and of the 256-row
     tiles, one larger than any block; a self pair, a two-row block on either side, a block index out of range;
  2. both exits of the RANSAC loop above 1024 rows, against oracle/registration_np.py (float64);
  3. ties in xyz across a count boundary go to the lower row of that count's numbering;
  4. C = 16 / 64 and K = 8192 with 5000 rows in use;
  5. the call is captured in a HIP graph and replayed on other data;
  6. more than PAIRS_PER_CALL (pair, count) results in one Python call equal the unrepeated call, repeated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 5
COUNTS = (3, 250, 1024, 1025, 1300, 2000)
BLOCK_COUNTS = (1500, 1463, 1100, 2)
PAIRS = ((0, 1), (1, 0), (2, 0), (0, 2), (1, 1), (3, 0), (0, 3), (0, 7))
FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers", "nearest")


def _kw():
    from d3feat_amd import registration as reg
    return dict(reg.EVALUATE_3DMATCH, max_iteration=20000, max_validation=100, seed=SEED)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _eq(x, y):
    return torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def _same_tensors(a, b):
    return all(_eq(getattr(a, k), getattr(b, k)) for k in FIELDS)


def _gt(poses, pairs, device):
    """[P, 3, 4] float32, target -> source: inv(poses[a]) @ poses[b]; the identity for a pair with an index out of range."""
    n = len(poses)
    return torch.from_numpy(np.stack([(np.linalg.inv(poses[a]) @ poses[b])[:3] if max(a, b) < n else np.eye(4)[:3]
                                      for a, b in pairs]).astype(np.float32)).to(device)


def _scene_on_device(seed, device):
    from d3feat_amd import registration as reg
    from d3feat_amd.utils.synthetic import scene
    blocks, poses = scene(seed, n_frag=4, K=1500)
    kp, count = reg.stack_keypoints(blocks, 1500, device=device)
    return blocks, poses, kp, count


@pytest.fixture(scope="module")
def scene3(device):
    return _scene_on_device(3, device)


@pytest.fixture(scope="module")
def cut(device, scene3):
    """the call of part 1: the blocks cut to BLOCK_COUNTS rows on the device, PAIRS, COUNTS"""
    from d3feat_amd import registration as reg
    _, poses, kp, _ = scene3
    count = torch.tensor(BLOCK_COUNTS, dtype=torch.int32, device=device)
    pairs = torch.tensor(PAIRS, dtype=torch.int32, device=device)
    gt = _gt(poses, PAIRS, device)
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=COUNTS, gt=gt, nearest=True, **_kw())
    return kp, count, pairs, gt, res


def _rows(p, c):
    """(Ns, Nt) of PAIRS[p] at COUNTS[c]"""
    a, b = PAIRS[p]
    n = lambda f: min(BLOCK_COUNTS[f], COUNTS[c]) if f < len(BLOCK_COUNTS) else 0
    return n(a), n(b)


# ---- 1. equal to the code the project already has, bit for bit ---------------------------------------------------------------------
def test_equal_to_register_keypoints_bit_for_bit(device, cut):
    from d3feat_amd import registration as reg
    kp, count, pairs, gt, res = cut
    kw = _kw()
    assert res.num_keypts == COUNTS and res.offsets == (0, 3, 253, 1277, 2302, 3602) and tuple(res.nearest.shape) == (len(PAIRS), 5602)
    near = res.nearest.cpu().numpy()
    for p, (a, b) in enumerate(PAIRS):
        for c, k in enumerate(COUNTS):
            where = "pair %d = (%d, %d) at count %d" % (p, a, b, k)
            got = res.host(p, c)
            Ns, Nt = _rows(p, c)
            assert np.all(near[p, res.offsets[c] + Ns:res.offsets[c] + k] == -1), where            # padding
            if min(Ns, Nt) < kw["ransac_n"]:
                assert got["validations"] == 0 and got["iterations"] == 0 and got["best_iteration"] == -1, where
                assert np.array_equal(got["transformation"], np.eye(4)) and got["fitness"] == 0.0 and got["inlier_rmse"] == 0.0, where
                assert len(got["correspondence_set"]) == 0, where
                if min(Ns, Nt) == 0:
                    assert got["mutual_count"] == 0, where
                    continue
            want = reg.register_keypoints(kp[a, :BLOCK_COUNTS[a]], kp[b, :BLOCK_COUNTS[b]], num_keypts=k, device=device, **kw)
            assert np.array_equal(_bits(got["transformation"]), _bits(want["transformation"])), where
            assert got["fitness"] == want["fitness"] and got["inlier_rmse"] == want["inlier_rmse"], where
            assert got["validations"] == want["validations"], where
            assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), where
            assert got["correspondence_set"].dtype == want["correspondence_set"].dtype == np.int64
            assert got["mutual_count"] == len(want["correspondences"]), where
            if a == b:                                                                             # the self pair registers onto itself
                assert got["fitness"] == 1.0 and np.abs(got["transformation"] - np.eye(4)).max() < 1e-5, where
                assert np.array_equal(got["correspondence_set"][:, 0], got["correspondence_set"][:, 1]), where
    v = res.validations.cpu().numpy()
    assert np.all(v[4] == 100) and v[:4].max() > 0 and np.all(v[5:] == 0)                          # the other pairs did run


def _register_pairs_entry_point(kp, count, pairs, gt, k, kw):
    """d3f_register_pairs itself for num_keypts = k -> dict of device tensors.  registration.register_pairs reads the rows of a pair
    through the block index on the host side of the call, so a pair with an index out of range goes to the entry point, which takes
    it as an empty block."""
    from d3feat_amd import _lib, ops
    lib, dev = _lib.load(), kp.device
    (n_blocks, K, ld), P = kp.shape, pairs.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(T=torch.empty((P, 3, 4), dtype=torch.float32, device=dev), sumd2=torch.empty((P,), dtype=torch.int64, device=dev),
               nearest=torch.empty((P, k), **i32))
    for f in ("inliers", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers"):
        out[f] = torch.empty((P,), **i32)
    ws = ops.workspace(lib.d3f_register_pairs_workspace_bytes(P, K, k, kw["max_validation"]), dev)
    rc = lib.d3f_register_pairs(kp.data_ptr(), n_blocks, K, ld, ld - 4, count.data_ptr(), pairs.data_ptr(), P, k,
                                kw["max_correspondence_distance"], kw["ransac_n"], kw["edge_similarity"], kw["checker_distance"],
                                kw["max_iteration"], kw["max_validation"], kw["seed"], gt.data_ptr(), 0.10, out["T"].data_ptr(),
                                out["inliers"].data_ptr(), out["sumd2"].data_ptr(), out["validations"].data_ptr(),
                                out["iterations"].data_ptr(), out["best_iteration"].data_ptr(), out["mutual_count"].data_ptr(),
                                out["nearest"].data_ptr(), None, out["gt_inliers"].data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "register_pairs")
    return out


@pytest.mark.parametrize("c", [0, 1, 2])
def test_equal_to_register_pairs_up_to_1024_rows(device, cut, c):
    from d3feat_amd import registration as reg
    kp, count, pairs, gt, res = cut
    k = COUNTS[c]
    assert k <= reg._lib.PAIRS_KMAX
    got = res.at(c)
    want = _register_pairs_entry_point(kp, count, pairs, gt, k, _kw())                              # all eight pairs
    for f in FIELDS:
        assert _eq(got[f].contiguous(), want[f]), (f, k)
    n = len(PAIRS) - 1                                                                             # the pairs of blocks that exist
    want = reg.register_pairs(kp, count, pairs[:n].contiguous(), num_keypts=k, gt=gt[:n].contiguous(), **_kw())
    for f in FIELDS:
        assert _eq(got[f][:n].contiguous(), getattr(want, f)), (f, k)
    with pytest.raises(ValueError, match="register_keypoints"):                                    # the old call keeps its limit
        reg.register_pairs(kp, count, pairs[:n].contiguous(), num_keypts=COUNTS[3], **_kw())


def test_matching_counts_equal_match_pairs(device, cut):
    from d3feat_amd import registration as reg
    kp, count, pairs, gt, res = cut
    want = reg.match_pairs(kp, count, pairs, gt=gt, num_keypts=COUNTS)
    assert torch.equal(res.mutual_count, want.mutual_count) and torch.equal(res.gt_inliers, want.gt_inliers)
    assert int(res.mutual_count[:5].min()) > 0 and int(res.gt_inliers.max()) > 0


# ---- 2. against the oracle, above the old limit --------------------------------------------------------------------------------------
def test_both_exits_above_1024_rows_against_the_oracle(device, scene3):
    """The full blocks (1500 rows each).  Figures of this input from oracle/registration_np.py on the CPU (scene(3, n_frag=4, K=1500),
    EVALUATE_3DMATCH with max_iteration=20000, max_validation=100, seed 5):

        pair    count   iterations          validations   fitness        outcome
        (0, 3)    250    5993                100           0.58 - 0.88    early stop
        (0, 3)   1025    2266                100           across these   early stop
        (0, 3)   1300    2179                100           counts         early stop
        (1, 2)   1025   20000 (exhausted)     65           0.64           registers
        (1, 2)   1300   20000 (exhausted)     60           0.66           registers
        (0, 1)   1025   20000 (exhausted)     11           --             fails

    Pairs (0, 3) and (0, 1) at counts 250 and 1025 are compared with the oracle here (about 8 s of CPU), with the bounds of
    tests/test_gpu_register_pairs.py::test_against_the_oracle."""
    from d3feat_amd import registration as reg
    from oracle import registration_np as onp
    blocks, poses, kp, count = scene3
    kw = _kw()
    counts, host_pairs = (250, 1025, 1300), [(0, 3), (0, 1), (1, 2)]
    pairs = torch.tensor(host_pairs, dtype=torch.int32, device=device)
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, gt=_gt(poses, host_pairs, device), nearest=True, **kw)
    early, exhausted = 0, 0
    for p, (a, b) in enumerate(host_pairs[:2]):
        for c, k in enumerate(counts[:2]):
            where = "pair (%d, %d) at count %d" % (a, b, k)
            A, B = blocks[a][-k:], blocks[b][-k:]
            src, tgt, sd, td = A[:, :3], B[:, :3], A[:, 3:35], B[:, 3:35]
            # precondition (asserted, never skipped): the fp32 device pick of every nearest descriptor is the float64 pick
            for X, Y in ((sd, td), (td, sd)):
                assert np.array_equal(reg.feature_nn(X, Y, device=device).cpu().numpy(), onp.feature_nn(X, Y)[0]), where
            want = onp.ransac_feature_matching(src, tgt, sd, td, kw["max_correspondence_distance"], ransac_n=kw["ransac_n"],
                                               edge_similarity=kw["edge_similarity"], checker_distance=kw["checker_distance"],
                                               max_iteration=kw["max_iteration"], max_validation=kw["max_validation"], seed=SEED)
            got = res.host(p, c)
            Ns = len(src)
            print(where, "iterations", got["iterations"], "validations", got["validations"], "best", got["best_iteration"],
                  want.get("best_iteration"), "fitness", got["fitness"], want["fitness"])
            assert got["iterations"] == want["iterations"] and got["validations"] == want["validations"], where
            assert abs(got["fitness"] - want["fitness"]) <= 1.0 / Ns + 1e-9, where       # a point on the radius may flip
            M = got["transformation"]
            rescored = onp.evaluate(src, tgt, M[:3, :3], M[:3, 3], kw["max_correspondence_distance"])[0]
            assert rescored >= round(want["fitness"] * Ns) - 1, where
            if got["best_iteration"] == want.get("best_iteration", -1):
                assert np.abs(M - want["transformation"]).max() < 1e-3, where
            if k > 1024:
                early += got["iterations"] < kw["max_iteration"]
                exhausted += got["iterations"] == kw["max_iteration"]
    assert early >= 1 and exhausted >= 1                                                 # both exits of the loop, above 1024 rows
    it = res.iterations.cpu().numpy()
    assert np.all(it[0] < 20000) and np.all(it[2, 1:] == 20000)                          # (0, 3) stops early, (1, 2) never does


# ---- 3. ties in xyz across a count boundary ---------------------------------------------------------------------------------------------
def test_xyz_ties_across_a_count_boundary_take_the_lower_row(device):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    d = rng.standard_normal((600, 32)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    score = np.sort(rng.random(600).astype(np.float32))[:, None]
    block = np.concatenate([np.concatenate([pts, pts]), d, score], 1)                    # rows j and j + 300 hold the same point
    kp, count = reg.stack_keypoints([block], 600, device=device)
    pairs = torch.zeros((1, 2), dtype=torch.int32, device=device)
    counts = (300, 450, 600)
    kw = dict(max_correspondence_distance=0.05, max_iteration=512, max_validation=8, seed=SEED)
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, nearest=True, **kw)
    # count 300: rows 300..599, all distinct: every row finds itself.  Count 450: rows 150..599, numbered from 0: rows 150..299 (0..149)
    # come before their twins 450..599 (300..449), which therefore find them; rows 300..449 (150..299) have no twin in use.  Count 600:
    # every row of the second half finds its twin in the first.
    expect = {300: np.arange(300), 450: np.concatenate([np.arange(300), np.arange(150)]), 600: np.concatenate([np.arange(300)] * 2)}
    for c, k in enumerate(counts):
        got = res.host(0, c)
        assert got["fitness"] == 1.0 and got["validations"] == 8, k
        assert np.array_equal(res.at(c)["nearest"][0].cpu().numpy(), expect[k]), k
        want = reg.register_keypoints(kp[0], kp[0], num_keypts=k, device=device, **kw)
        assert np.array_equal(_bits(got["transformation"]), _bits(want["transformation"])), k
        assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), k
        assert np.array_equal(got["correspondence_set"], np.stack([np.arange(k), expect[k]], 1)), k


# ---- 4. other shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64])
def test_other_descriptor_widths_and_blocks_of_5000_rows(device, C):
    """K = 8192 with one block of 5000 rows and one of 844, counts (250, 5000): twenty 256-row tiles per pass, the grid over 5844 points."""
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(C)
    base = rng.uniform(-1, 1, (5000, 3))
    desc = rng.standard_normal((5000, C))
    blocks = []
    for n in (5000, 844):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        sel = rng.permutation(5000)[:n]
        d = desc[sel] + 0.05 * rng.standard_normal((n, C))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        blocks.append(np.concatenate([base[sel] @ q.T + rng.uniform(-1, 1, 3), d, np.sort(rng.random(n))[:, None]], 1).astype(np.float32))
    kp, count = reg.stack_keypoints(blocks, 8192, device=device)
    assert tuple(kp.shape) == (2, 8192, C + 4) and count.tolist() == [5000, 844]
    host_pairs, counts = [(0, 1), (1, 0), (0, 0)], (250, 5000)
    pairs = torch.tensor(host_pairs, dtype=torch.int32, device=device)
    kw = dict(reg.EVALUATE_3DMATCH, max_iteration=2000, max_validation=20, seed=11)
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, nearest=True, **kw)
    for p, (a, b) in enumerate(host_pairs):
        for c, k in enumerate(counts):
            got = res.host(p, c)
            want = reg.register_keypoints(kp[a, :len(blocks[a])], kp[b, :len(blocks[b])], num_keypts=k, device=device, **kw)
            assert np.array_equal(_bits(got["transformation"]), _bits(want["transformation"])), (p, k)
            assert (got["fitness"], got["inlier_rmse"], got["validations"]) == (want["fitness"], want["inlier_rmse"], want["validations"]), (p, k)
            assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), (p, k)
            assert got["mutual_count"] == len(want["correspondences"]), (p, k)
    # the motion between two copies of one cloud is found where most rows have their twin (all of them at the full count)
    assert res.host(1, 1)["validations"] == 20 and res.host(1, 1)["fitness"] > 0.9
    assert res.host(2, 1)["fitness"] == 1.0


# ---- 5. capture ---------------------------------------------------------------------------------------------------------------------
def test_capture_in_a_hip_graph_and_replay_on_other_data(device, scene3):
    from d3feat_amd import ops
    from d3feat_amd import registration as reg
    _, poses3, kp3, count = scene3
    _, poses4, kp4, count4 = _scene_on_device(4, device)
    assert not torch.equal(count, count4)                                            # two short blocks: the sizes are read on the device
    pairs = reg.scene_pairs(4, device=device)
    host_pairs = pairs.cpu().tolist()
    gt3, gt4 = _gt(poses3, host_pairs, device), _gt(poses4, host_pairs, device)
    kw = dict(_kw(), num_keypts=(250, 1025), nearest=True)
    eager3 = reg.register_pairs_counts(kp3, count, pairs, gt=gt3, **kw)
    eager4 = reg.register_pairs_counts(kp4, count4, pairs, gt=gt4, **kw)
    assert not _same_tensors(eager3, eager4)
    kp, cnt, gt = kp3.clone(), count.clone(), gt3.clone()
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            res = reg.register_pairs_counts(kp, cnt, pairs, gt=gt, **kw)             # eager warm-up on this stream (scratch)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            reg.register_pairs_counts(kp, cnt, pairs, gt=gt, out=res, **kw)
    keep = pw.kept
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    assert _same_tensors(res, eager3)
    kp.copy_(kp4)
    cnt.copy_(count4)
    gt.copy_(gt4)
    for k in FIELDS:
        getattr(res, k).fill_(-7)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    res._cache = None
    assert _same_tensors(res, eager4) and not _same_tensors(res, eager3)
    assert res.host(5, 1)["validations"] == eager4.host(5, 1)["validations"]
    del keep


# ---- 6. chunking --------------------------------------------------------------------------------------------------------------------
def test_more_results_than_one_entry_point_call_holds(device, cut):
    from d3feat_amd import registration as reg
    kp, count, pairs, gt, _ = cut
    counts = (3, 250, 1025)
    kw = dict(_kw(), max_iteration=2000, max_validation=20, num_keypts=counts, nearest=True)
    want = reg.register_pairs_counts(kp, count, pairs, gt=gt, **kw)
    assert reg.PAIRS_PER_CALL == 4096
    rep = reg.PAIRS_PER_CALL // (len(counts) * len(PAIRS)) + 1
    assert rep * len(PAIRS) * len(counts) > reg.PAIRS_PER_CALL                       # two entry-point calls
    got = reg.register_pairs_counts(kp, count, pairs.repeat(rep, 1).contiguous(), gt=gt.repeat(rep, 1, 1).contiguous(), **kw)
    for f in FIELDS:
        y = getattr(want, f)
        assert _eq(getattr(got, f), y.repeat(rep, *([1] * (y.dim() - 1)))), f


# ---- the scene tool -------------------------------------------------------------------------------------------------------------------
def test_register_scene_tool_writes_the_files_of_every_count(device, scene3, tmp_path):
    """tools/register_scene.py --counts on the files save_3dmatch_keypoints writes for the scene, with a gt.log that lists the pairs of
    even a + b: per count a directory with one .rt.txt per pair and the .log blocks of the listed pairs, as register_pairs_counts
    gives them, and one recall line per count."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from d3feat_amd import registration as reg
    from d3feat_amd.utils import results
    blocks, poses, kp, count = scene3
    counts = (250, 1025)
    root, out = str(tmp_path / "results"), str(tmp_path / "out")
    for f, b in enumerate(blocks):
        results.save_3dmatch_keypoints(root, "synth/seq-01/cloud_bin_%d.ply" % f, b)
    pairs = reg.scene_pairs(len(blocks), device=device)
    host_pairs = [tuple(p) for p in pairs.cpu().tolist()]
    listed = [p for p in host_pairs if (p[0] + p[1]) % 2 == 0]
    with open(tmp_path / "gt.log", "w") as f:
        for a, b in listed:
            G = np.linalg.inv(poses[a]) @ poses[b]
            f.write("%d\t%d\t%d\n" % (a, b, len(blocks)))
            for r in range(4):
                f.write("\t".join(repr(float(x)) for x in G[r]) + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "register_scene.py"), "--root", root, "--scene", "synth", "--gt",
                          str(tmp_path / "gt.log"), "--seed", str(SEED), "--out", out, "--counts", ",".join(str(k) for k in counts)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [json.loads(x) for x in run.stdout.strip().splitlines()[-len(counts):]]
    assert [x["num_keypts"] for x in lines] == list(counts)
    # the same call here; the tool's gt is the float32 of the doubles the log holds, the identity for a pair the log does not list
    gt = np.tile(np.eye(4)[:3], (len(host_pairs), 1, 1))
    for i, (a, b) in enumerate(host_pairs):
        if (a, b) in listed:
            gt[i] = (np.linalg.inv(poses[a]) @ poses[b])[:3]
    res = reg.register_pairs_counts(kp, count, pairs, num_keypts=counts, gt=torch.from_numpy(gt.astype(np.float32)).to(device), seed=SEED,
                                    **reg.EVALUATE_3DMATCH)
    inl, mutual = res.gt_inliers.cpu().numpy(), res.mutual_count.cpu().numpy()
    for c, k in enumerate(counts):
        d, rows = os.path.join(out, "num_keypts_%d" % k), []
        assert lines[c]["fragments"] == 4 and lines[c]["pairs"] == 6 and lines[c]["gt"] == len(listed)
        for p, (a, b) in enumerate(host_pairs):
            text = open(os.path.join(d, "cloud_bin_%d_cloud_bin_%d.rt.txt" % (a, b))).read()
            if (a, b) in listed:
                assert text == "cloud_bin_%d\tcloud_bin_%d\t%d\t%.8f\t1" % (a, b, inl[p, c], inl[p, c] / mutual[p, c]), text
            else:
                assert text == "cloud_bin_%d\tcloud_bin_%d\t0\t%.8f\t0" % (a, b, 0.0), text
            nums = text.split("\t")[2:5]
            rows.append([int(nums[0]), float(nums[1]), int(nums[2])])
        want = results.feature_matching_recall(rows, 0.05)
        assert all(lines[c][key] == want[key] for key in want)
        back = results.read_gt_log(os.path.join(d, "D3Feat.log"))
        assert list(back) == ["%d_%d" % p for p in listed]
        for p, (a, b) in enumerate(host_pairs):
            if (a, b) in listed:
                M = np.eye(4)
                M[:3] = res.T[p, c].cpu().numpy().astype(np.float64)
                assert np.array_equal(back["%d_%d" % (a, b)], np.linalg.inv(M))
