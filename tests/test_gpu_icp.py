"""ICP on the GPU (d3f_icp_pairs, d3feat_amd.icp.icp_pairs) against the float64 restatement (tests/icp_np.py) and its fixture
(tests/golden/icp.npz, tools/make_golden_icp.py):

  1. a single search (max_iteration = 0): sources of 0, 1, 257 and 700 rows against targets of 1 to 900 rows -- several workgroup
     partials and ragged tails -- with a target at exactly d2 == r r, equal d2 (lowest index), queries far outside the grid's box and
     a moved query on a cell boundary whose correspondence sits a radius away in the neighbouring cell: nearest and count equal,
     sum d2 / fitness / rmse bit-equal;
  2. the whole loop on the golden pair: iterations, converged, nearest, count, fitness equal, T within 64 x the recorded difference
     between the two fit formulations (floor 1e-12: Jacobi on the device against LAPACK over up to 200 composed updates);
  3. the branches: identical clouds, max_iteration = 3, an empty source, clouds 10 m apart, a single correspondence;
  4. batching and skipping: those pairs in one call = each alone with B = 1, bit for bit;
  5. check_every = 0 equals check_every = 4 bit for bit, and the check_every = 0 call captured in a graph and replayed twice;
  6. compat/open3d's registration_icp = the direct call, bit for bit.
"""
import os

import numpy as np
import pytest
import torch

import icp_np
from conftest import GOLDEN, ROOT
from icp_cases import H, R, branch_pairs as _branch_pairs, single_pass_pairs as _single_pass_pairs      # the input builders

pytestmark = pytest.mark.gpu

KITTI = dict(max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6, relative_rmse=1e-6)
OUT = ("T", "count", "sumd2", "fitness", "rmse", "iterations", "converged", "nearest")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "icp.npz"))


def _run(device, pairs, **kw):
    """pairs: [(src, tgt, init or None)] -> PairICP of ONE call over all of them"""
    from d3feat_amd import icp
    src = np.concatenate([np.asarray(p[0], np.float32).reshape(-1, 3) for p in pairs])
    tgt = np.concatenate([np.asarray(p[1], np.float32).reshape(-1, 3) for p in pairs])
    init = np.stack([np.eye(4) if p[2] is None else p[2] for p in pairs])
    return icp.icp_pairs(torch.from_numpy(src).to(device), [len(p[0]) for p in pairs], torch.from_numpy(tgt).to(device),
                         [len(p[1]) for p in pairs], init=init, **kw)


def _host(res):
    return {k: res.dev[k].cpu().numpy() for k in OUT}


def _rows(pairs):
    return np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(int)


def _check_exact_part(h, p, off, want):
    """what has the device's bits in the restatement: the integers, sum d2 and the figures"""
    assert h["count"][p] == want.count and h["iterations"][p] == want.iterations and h["converged"][p] == want.converged, p
    assert np.array_equal(h["nearest"][off[p]:off[p + 1]], want.nearest), p
    assert h["fitness"][p] == want.fitness, p


# ---- 1. a single search --------------------------------------------------------------------------------------------------------------------
def test_single_search(device):
    pairs = _single_pass_pairs()
    assert [len(p[0]) for p in pairs] == [0, 1, 257, 700, 300] and [len(p[1]) for p in pairs] == [1, 1, 300, 603, 900]
    kw = dict(max_correspondence_distance=R, max_iteration=0)
    want = [icp_np.icp(s, t, T0, **kw) for s, t, T0 in pairs]
    # the cases are what they claim to be
    assert want[1].count == 0 and want[1].margin_r == 0.0                             # d2 == r r exactly
    nn = want[2].nearest
    assert nn[250] == 293 and want[2].margin_nn == 0.0                                # three at equal d2: the lowest index
    assert nn[251] == -1 and np.all(nn[252:] == -1) and 0 < (nn[:250] >= 0).sum()
    p3 = icp_np.move(pairs[3][2][:3], pairs[3][0])
    assert p3[699, 0] == 3 * H and want[3].nearest[699] == 601 and want[3].nearest[698] == 602
    assert R * R * (1 - 1e-5) < icp_np._d2(p3[699:700], pairs[3][1][601:602].astype(np.float64))[0, 0] < R * R
    assert 0 < want[4].count < 300
    h = _host(_run(device, pairs, check_every=0, **kw))
    off = _rows(pairs)
    for p, w in enumerate(want):
        _check_exact_part(h, p, off, w)
        assert h["sumd2"][p] == w.sumd2 and h["rmse"][p] == w.rmse, p                # bit-equal: the sums are in the header's order
        assert h["iterations"][p] == 0 and h["converged"][p] == 0
        assert np.array_equal(h["T"][p].reshape(3, 4), w.T[:3]), p                    # untouched: the init's bits


# ---- 2. the whole loop ---------------------------------------------------------------------------------------------------------------------
def _tolerance(gold, tag=""):
    return max(64.0 * float(gold[tag + "fit_difference"]), 1e-12)


def _check_gold(h, p, off, gold, tag=""):
    assert h["iterations"][p] == int(gold[tag + "iterations"]) and h["converged"][p] == int(gold[tag + "converged"])
    assert np.array_equal(h["nearest"][off[p]:off[p + 1]], gold[tag + "nearest"])
    assert h["count"][p] == int(gold[tag + "count"]) and h["fitness"][p] == float(gold[tag + "fitness"])
    err = np.max(np.abs(h["T"][p].reshape(3, 4) - gold[tag + "T"][:3]))
    print("%sT: max difference to the restatement %.3e (allowed %.3e)" % (tag, err, _tolerance(gold, tag)))
    assert err <= _tolerance(gold, tag)
    # 2000 rows, d <= 0.2, coordinates below 6 m: a T within 1e-12 moves sum d2 by at most 2000 * 0.4 * 1.9e-11 = 1.5e-8
    assert abs(h["rmse"][p] - float(gold[tag + "rmse"])) <= 1e-9 and abs(h["sumd2"][p] - float(gold[tag + "sumd2"])) <= 1e-7


def test_whole_loop_on_the_golden_pair(device, gold):
    res = _run(device, [(gold["src"], gold["tgt"], None)], **KITTI)
    _check_gold(_host(res), 0, [0, 2000], gold)
    c = res.correspondences(0)
    assert c.shape == (int(gold["count"]), 2) and np.array_equal(c[:, 1], gold["nearest"][c[:, 0]])
    assert res.transformation.shape == (1, 4, 4) and np.array_equal(res.transformation[0, 3], [0, 0, 0, 1])


# ---- 3. the branches -----------------------------------------------------------------------------------------------------------------------
def _check_branch(h, p, off, pair, **kw):
    w = icp_np.icp(pair[0], pair[1], pair[2], **kw)
    _check_exact_part(h, p, off, w)
    assert np.max(np.abs(h["T"][p].reshape(3, 4) - w.T[:3])) <= 1e-12, p
    assert abs(h["rmse"][p] - w.rmse) <= 1e-9 and abs(h["sumd2"][p] - w.sumd2) <= 1e-7
    return w


def test_branches(device, gold):
    pairs = _branch_pairs(gold)
    for p in (1, 2, 3, 4):
        h = _host(_run(device, [pairs[p]], **KITTI))
        w = _check_branch(h, 0, [0, len(pairs[p][0])], pairs[p], **KITTI)
        # they stop at k = 1; the single correspondence at k = 2 (its rmse drops from 6 cm to 0 in the one update)
        assert w.iterations == (2 if p == 4 else 1) and w.converged == 1, p
        if p == 1:
            assert w.count == 500 and w.fitness == 1.0 and h["rmse"][0] <= 1e-12
        if p in (2, 3):
            assert w.count == 0 and np.array_equal(h["T"][0], np.eye(4)[:3].reshape(12))      # U = identity: the init's bits
        if p == 4:
            assert w.count == 1 and np.array_equal(h["T"][0].reshape(3, 4)[:, :3], np.eye(3))  # S = 0: the identity rotation
            assert np.allclose(h["T"][0].reshape(3, 4)[:, 3], pairs[4][1][1].astype(np.float64) - pairs[4][0][1], atol=1e-15)
    h = _host(_run(device, [pairs[0]], **dict(KITTI, max_iteration=3)))
    _check_gold(h, 0, [0, 2000], gold, "it3_")
    assert h["iterations"][0] == 3 and h["converged"][0] == 0


# ---- 4. batching and skipping, 5. check_every ------------------------------------------------------------------------------------------------
def test_batch_equals_every_pair_alone_and_check_every(device, gold):
    pairs = _branch_pairs(gold)
    off = _rows(pairs)
    every4 = _host(_run(device, pairs, check_every=4, **KITTI))
    _check_gold(every4, 0, off, gold)
    for p, pair in enumerate(pairs):
        alone = _host(_run(device, [pair], check_every=4, **KITTI))
        for k in OUT:
            a = every4[k][off[p]:off[p + 1]] if k == "nearest" else every4[k][p]
            assert np.array_equal(np.atleast_1d(a), alone[k].reshape(np.atleast_1d(a).shape)), (p, k)
    every0 = _host(_run(device, pairs, check_every=0, **KITTI))
    for k in OUT:
        assert np.array_equal(every0[k], every4[k]), k


def test_captured_in_a_graph_and_replayed_twice(device, gold):
    from d3feat_amd import icp
    pairs = _branch_pairs(gold)
    eager = _host(_run(device, pairs, check_every=0, **KITTI))
    src = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(device)
    tgt = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(device)
    sl = torch.tensor([len(p[0]) for p in pairs], dtype=torch.int32, device=device)
    tl = torch.tensor([len(p[1]) for p in pairs], dtype=torch.int32, device=device)
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        icp.icp_pairs(src, sl, tgt, tl, check_every=0, **KITTI)                       # eager warm-up on this stream
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        res = icp.icp_pairs(src, sl, tgt, tl, check_every=0, **KITTI)                 # grid build, init and 201 rounds: launches only
    for _ in range(2):
        for k in OUT:
            res.dev[k].fill_(-7)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        got = _host(res)
        for k in OUT:
            assert np.array_equal(got[k], eager[k]), k


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_compat_registration_icp_is_the_direct_call(device, gold):
    direct = _run(device, [(gold["src"], gold["tgt"], None)], **KITTI)
    with icp_np.compat_open3d(ROOT) as open3d:
        a, b = open3d.geometry.PointCloud(), open3d.geometry.PointCloud()
        a.points = open3d.utility.Vector3dVector(gold["src"])
        b.points = open3d.utility.Vector3dVector(gold["tgt"])
        reg = open3d.registration
        res = reg.registration_icp(a, b, 0.2, np.eye(4), reg.TransformationEstimationPointToPoint(),
                                   reg.ICPConvergenceCriteria(max_iteration=200))
    assert np.array_equal(res.transformation, direct.transformation[0])
    assert res.fitness == direct.fitness[0] and res.inlier_rmse == direct.inlier_rmse[0]
    assert np.array_equal(np.asarray(res.correspondence_set), direct.correspondences(0))
    assert np.max(np.abs(res.transformation - gold["T"])) <= _tolerance(gold) and res.fitness == float(gold["fitness"])
    assert np.array_equal(np.asarray(res.correspondence_set)[:, 1], gold["nearest"][gold["nearest"] >= 0])
