"""d3f_training_pairs on the GPU against tests/training_pairs_np.py (the header's text in numpy, held against a float64 brute force, a
KD-tree and the reference's rotate() by tests/test_training_pairs_host.py): every integer integer for integer, the rows bit for bit.

The fixtures (tests/training_pairs_cases.py) make fp32 and float64 agree about every match: lattice points in sixty-fourths under quarter
turns (every d2 exact, ties frequent), and one pair under a general rotation with a searched margin of 1e-4.  The sizes are the
smallest that reach each branch: an anchor of 1100 rows (past one workgroup and one scan tile), M = min_matches - 1 / = min_matches /
= keypts_num, an empty anchor, rows without a match at both ends of a cloud, 75 positives inside one radius, an anchor outside the
positive's box, 254 clouds in one call, capacities above the lengths with sentinels behind every output.

.params is compared within one fp32 ulp (the device's float64 cos / sin against libm); .points is then held BIT FOR BIT to the
restatement fed the device's parameters, so the row pass has no tolerance at all.
"""
import os

import numpy as np
import pytest
import torch

import training_pairs_cases as tc
import training_pairs_np as tp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -777.25, -7


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(device, pairs, radius=tc.RADIUS, extra_rows=0, sentinels=True, **kw):
    """One radius-form call on `pairs` -> (result, host dict of every output, points, lens, trans)."""
    from d3feat_amd import training_pairs as T
    pts, lens, trans = tc.stack(pairs)
    if extra_rows:
        pts = np.concatenate([pts, np.full((extra_rows, 3), 1e6, np.float32)])
    N, P, k = len(pts), len(pairs), int(kw["keypts_num"])
    out = T.TrainingPairs(N, P, k, device)
    if sentinels:
        out.points.fill_(SENT_F); out.backup.fill_(SENT_F); out.anc_idx.fill_(SENT_I); out.pos_idx.fill_(SENT_I)
    res = T.training_pairs(_t(pts, device), _t(lens, device), trans=_t(trans, device), radius=radius, out=out, **kw)
    torch.cuda.synchronize(device)
    host = {name: getattr(res, name).cpu().numpy() for name in ("points", "backup", "anc_idx", "pos_idx", "n", "row0", "matches", "status", "params")}
    host["step"] = int(res.step.item())
    return res, host, pts, lens, trans


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all())


def _held(host, pts, lens, trans, pairs, radius, step, **kw):
    """Every output of a radius-form call against the restatement."""
    n_real = int(np.sum(lens))
    want = tp.training_pairs(pts[:n_real], lens, trans, radius=radius, step=step, **kw)
    fed = tp.training_pairs(pts[:n_real], lens, trans, radius=radius, step=step, params=host["params"], **kw)
    P = len(pairs)
    for name in ("n", "matches", "status", "row0"):
        assert np.array_equal(host[name][:len(want[name])], want[name]), (name, host[name], want[name])
    assert host["row0"][P] == n_real
    assert _ulp_close(host["params"], want["params"]), np.abs(host["params"] - want["params"]).max()
    assert np.array_equal(host["params"][:, 13:], want["params"][:, 13:])
    assert np.array_equal(_bits(host["points"][:n_real]), _bits(fed["points"]))
    assert np.array_equal(_bits(host["backup"][:n_real]), _bits(want["backup"]))
    # nothing behind a count: the rows past n, the index rows of a flagged pair
    assert (host["points"][n_real:] == SENT_F).all() and (host["backup"][n_real:] == SENT_F).all()
    for p, (a, b, T) in enumerate(pairs):
        if want["status"][p]:
            assert host["n"][p] == 0 and (host["anc_idx"][p] == SENT_I).all() and (host["pos_idx"][p] == SENT_I).all()
            continue
        assert np.array_equal(host["anc_idx"][p], want["anc_idx"][p]) and np.array_equal(host["pos_idx"][p], want["pos_idx"][p]), p
        true = tp.matches_f64(a, b, T, radius)
        got = list(zip(host["anc_idx"][p].tolist(), (host["pos_idx"][p] - len(a)).tolist()))
        assert len(set(got)) == len(got) and set(got) <= true                   # distinct true matches; pos shifted by len(anchor)
        assert host["matches"][p] == len(true)
    return want


def test_three_pairs_every_output(device):
    pairs = tc.three_pairs()
    kw = dict(keypts_num=16, min_matches=64, seed=5, augment=tp.AUGMENT_KITTI)
    res, host, pts, lens, trans = _run(device, pairs, extra_rows=37, step=3, **kw)
    want = _held(host, pts, lens, trans, pairs, tc.RADIUS, 3, **kw)
    assert (want["status"] == 0).all() and host["step"] == 4
    assert not np.array_equal(host["params"][0, 9], 1.0) and np.array_equal(host["params"][0, 9], host["params"][1, 9])


def test_thresholds_of_the_sample(device):
    """M = min_matches - 1 (flagged, the index row untouched), M = min_matches, M = keypts_num exactly (every match returned)."""
    pair = tc.small_pair()
    lst, _ = tp.matches(*pair, tc.RADIUS)
    M = len(lst)
    assert 16 < M <= 1024
    for k, mm, status in ((8, M + 1, tp.FEW_MATCHES), (8, M, 0), (M, 1, 0), (M, M, 0)):
        kw = dict(keypts_num=k, min_matches=mm, seed=9, augment=tp.AUGMENT_3DMATCH)
        res, host, pts, lens, trans = _run(device, [pair], step=1, **kw)
        _held(host, pts, lens, trans, [pair], tc.RADIUS, 1, **kw)
        assert host["status"][0] == status and host["matches"][0] == M and host["n"][0] == (0 if status else k)
        if k == M:
            got = sorted(zip(host["anc_idx"][0].tolist(), (host["pos_idx"][0] - len(pair[0])).tolist()))
            assert got == sorted(map(tuple, lst.tolist()))
    # more indices asked for than there are matches
    kw = dict(keypts_num=M + 1, min_matches=1, seed=9, augment=tp.AUGMENT_3DMATCH)
    res, host, pts, lens, trans = _run(device, [pair], step=1, **kw)
    _held(host, pts, lens, trans, [pair], tc.RADIUS, 1, **kw)
    assert host["status"][0] == tp.BELOW_KEYPTS


def test_empty_ends_cluster_and_apart(device):
    """An empty anchor, rows without a match at the first and last record of a cloud, 75 positives inside one radius, an anchor outside the
    positive's grown box -- in one call, between ordinary pairs."""
    a, b, T = tc.small_pair()
    empty = (np.zeros((0, 3), np.float32), b, T)
    pairs = [tc.ends_pair(), empty, tc.cluster_pair(), tc.apart_pair(), tc.small_pair(seed=6)]
    kw = dict(keypts_num=64, min_matches=64, seed=21, augment=tp.AUGMENT_KITTI)
    res, host, pts, lens, trans = _run(device, pairs, extra_rows=5, step=0, **kw)
    want = _held(host, pts, lens, trans, pairs, tc.RADIUS, 0, **kw)
    assert want["status"].tolist()[1] == want["status"].tolist()[3] == (tp.FEW_MATCHES | tp.BELOW_KEYPTS)
    assert want["status"][0] == 0 and want["status"][2] == 0 and host["matches"][1] == 0 and host["matches"][3] == 0
    # the cluster's row is sampled past its 8th candidate
    a, b, T = pairs[2]
    lst, start = tp.matches(a, b, T, tc.RADIUS)
    row = int(np.argmax(np.diff(start)))
    d2 = tp.d2_f32(tp.move(T, a[row:row + 1]), b)[0]
    ranks = [lst[start[row]:start[row + 1], 1].tolist().index(j - len(a)) for i, j in zip(host["anc_idx"][2], host["pos_idx"][2]) if i == row]
    assert max(ranks) > 32 and len(set(d2[lst[start[row]:start[row + 1], 1]].tolist())) < 40         # deep ranks, among many ties


def test_general_rotation(device):
    z = np.load(os.path.join(GOLDEN, "training_pairs.npz"))
    pair = (z["general_anchor"], z["general_positive"], z["general_trans"])
    radius = float(z["general_radius"])
    kw = dict(keypts_num=128, min_matches=128, seed=2, augment=dict(tp.AUGMENT_KITTI, augment_rotation=3))
    res, host, pts, lens, trans = _run(device, [pair], radius=radius, step=8, **kw)
    want = _held(host, pts, lens, trans, [pair], radius, 8, **kw)
    assert want["status"][0] == 0


@pytest.mark.parametrize("rotation", [0, 1, 3])
@pytest.mark.parametrize("moved", [True, False], ids=["scale_shift", "plain"])
def test_augmentation_modes(device, rotation, moved):
    aug = dict(tp.AUGMENT_KITTI if moved else tp.AUGMENT_3DMATCH, augment_rotation=rotation)
    pairs = [tc.small_pair(), tc.small_pair(seed=6)]
    kw = dict(keypts_num=8, min_matches=8, seed=13, augment=aug)
    res, host, pts, lens, trans = _run(device, pairs, step=2, **kw)
    _held(host, pts, lens, trans, pairs, tc.RADIUS, 2, **kw)
    q = host["params"]
    assert (q[:, 15] == rotation).all()
    if rotation == 0:
        assert np.array_equal(q[:, :9], np.tile(np.eye(3, dtype=np.float32).reshape(9), (4, 1)))
    else:
        assert not np.array_equal(q[0, :9], q[1, :9])
    if moved:
        assert q[0, 9] == q[1, 9] != q[2, 9] and not np.array_equal(q[0, 10:13], q[1, 10:13])
    else:
        assert (q[:, 9] == 1).all() and not q[:, 10:13].any()


def test_equal_step_equal_bits_and_another_step_moves_everything(device):
    pairs = tc.three_pairs()[1:]
    kw = dict(keypts_num=16, min_matches=16, seed=4, augment=tp.AUGMENT_KITTI)
    _, a, *_ = _run(device, pairs, step=6, **kw)
    _, b, *_ = _run(device, pairs, step=6, **kw)
    _, c, *_ = _run(device, pairs, step=7, **kw)
    for name in ("points", "backup", "anc_idx", "pos_idx", "n", "row0", "matches", "status", "params"):
        assert np.array_equal(_bits(a[name]) if a[name].dtype == np.float32 else a[name], _bits(b[name]) if b[name].dtype == np.float32 else b[name]), name
    for name in ("points", "anc_idx", "pos_idx", "params"):
        assert not np.array_equal(a[name], c[name]), name
    assert not (a["points"] == c["points"]).all(1).any() and not np.array_equal(a["anc_idx"][0], c["anc_idx"][0])
    assert np.array_equal(a["backup"], c["backup"]) and np.array_equal(a["matches"], c["matches"])       # (no draw in these)


def test_254_clouds_in_one_call_equal_the_pairs_run_alone(device):
    from d3feat_amd import training_pairs as T
    pairs = tc.many_pairs(127)
    kw = dict(keypts_num=4, min_matches=4, seed=17, augment=tp.AUGMENT_KITTI)
    res, host, pts, lens, trans = _run(device, pairs, step=5, **kw)
    assert len(lens) == 254
    _held(host, pts, lens, trans, pairs, tc.RADIUS, 5, **kw)
    off = np.concatenate([[0], np.cumsum(lens)])
    for p, pair in enumerate(pairs):
        _, one, *_ = _run(device, [pair], step=5, first_pair=p, **kw)
        r0, r1 = off[2 * p], off[2 * p + 2]
        assert np.array_equal(_bits(one["points"]), _bits(host["points"][r0:r1])) and np.array_equal(_bits(one["backup"]), _bits(host["backup"][r0:r1]))
        assert np.array_equal(one["anc_idx"][0], host["anc_idx"][p]) and np.array_equal(one["pos_idx"][0], host["pos_idx"][p])
        assert np.array_equal(_bits(one["params"]), _bits(host["params"][2 * p:2 * p + 2]))
        assert (one["n"][0], one["matches"][0], one["status"][0]) == (host["n"][p], host["matches"][p], host["status"][p])
    # more pairs than one call takes: chunks, the same bits
    more = pairs + pairs[:3]
    res2, host2, *_ = _run(device, more, step=5, **kw)
    assert np.array_equal(host2["anc_idx"][:127], host["anc_idx"]) and np.array_equal(_bits(host2["points"][:off[-1]]), _bits(host["points"]))
    _, tail, *_ = _run(device, pairs[:3], step=5, first_pair=127, **kw)
    assert np.array_equal(host2["anc_idx"][127:], tail["anc_idx"]) and np.array_equal(host2["row0"][127:], tail["row0"] + off[-1])
    assert host2["step"] == 6


def test_list_form(device):
    """The 3DMatch form on lists of length 1, 5 and 3000 (and an empty one): with replacement, both columns from one row of the list."""
    from d3feat_amd import training_pairs as T
    pairs = [tc.small_pair(seed=s) for s in (5, 6, 7, 8)]
    pts, lens, _ = tc.stack(pairs)
    kp, start = tc.keypts_lists([1, 5, 3000, 0], [(len(a), len(b)) for a, b, _ in pairs])
    pts_cap = np.concatenate([pts, np.full((9, 3), 1e6, np.float32)])
    k = 64
    out = T.TrainingPairs(len(pts_cap), 4, k, device)
    out.points.fill_(SENT_F); out.backup.fill_(SENT_F); out.anc_idx.fill_(SENT_I); out.pos_idx.fill_(SENT_I)
    res = T.training_pairs(_t(pts_cap, device), _t(lens, device), keypts_pairs=_t(kp, device), pair_start=_t(start, device), keypts_num=k,
                           seed=3, augment=T.AUGMENT_3DMATCH, out=out)                                 # the device step: 0
    torch.cuda.synchronize(device)
    want = tp.training_pairs(pts, lens, keypts_pairs=kp, pair_start=start, keypts_num=k, seed=3, step=0, augment=tp.AUGMENT_3DMATCH)
    fed = tp.training_pairs(pts, lens, keypts_pairs=kp, pair_start=start, keypts_num=k, seed=3, step=0, augment=tp.AUGMENT_3DMATCH,
                            params=res.params.cpu().numpy())
    assert res.matches.tolist() == [1, 5, 3000, 0] and res.status.tolist() == [0, 0, 0, tp.BELOW_KEYPTS] and res.n.tolist() == [k, k, k, 0]
    got_a, got_p = res.anc_idx.cpu().numpy(), res.pos_idx.cpu().numpy()
    assert np.array_equal(got_a[:3], want["anc_idx"][:3]) and np.array_equal(got_p[:3], want["pos_idx"][:3])
    assert (got_a[3] == SENT_I).all() and (got_p[3] == SENT_I).all()
    assert len(set(got_a[2].tolist())) > 8 and int(res.step.item()) == 1
    n = len(pts)
    assert np.array_equal(_bits(res.backup.cpu().numpy()[:n]), _bits(pts)) and (res.backup.cpu().numpy()[n:] == SENT_F).all()
    assert np.array_equal(_bits(res.points.cpu().numpy()[:n]), _bits(fed["points"])) and (res.points.cpu().numpy()[n:] == SENT_F).all()
    assert _ulp_close(res.params.cpu().numpy(), want["params"])
    # offsets outside the list
    bad = start.copy(); bad[-1] = len(kp) + 1
    res = T.training_pairs(_t(pts, device), _t(lens, device), keypts_pairs=_t(kp, device), pair_start=_t(bad, device), keypts_num=k, seed=3,
                           step=0, augment=T.AUGMENT_3DMATCH)
    assert res.status.tolist() == [0, 0, 0, tp.LIST_RANGE] and res.n.tolist() == [k, k, k, 0]


def test_capture_once_replay_three_times(device):
    """.step advances on the device: each replay equals the eager call at that step, no two replays are equal."""
    from d3feat_amd import training_pairs as T
    pairs = tc.three_pairs()[1:]
    pts, lens, trans = tc.stack(pairs)
    kw = dict(radius=tc.RADIUS, keypts_num=16, min_matches=16, seed=8, augment=T.AUGMENT_KITTI)
    d_pts, d_lens, d_trans = _t(pts, device), _t(lens, device), _t(trans, device)
    stream, graph = torch.cuda.Stream(device=device), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        res = T.training_pairs(d_pts, d_lens, trans=d_trans, **kw)                    # eager warm-up on this stream: step 0 -> 1
    stream.synchronize()
    assert int(res.step.item()) == 1
    with torch.cuda.graph(graph, stream=stream):
        T.training_pairs(d_pts, d_lens, trans=d_trans, out=res, **kw)                 # builds its grid inside the capture
    seen = []
    for replay in range(3):
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        step = 1 + replay
        assert int(res.step.item()) == step + 1
        eager = T.training_pairs(d_pts, d_lens, trans=d_trans, step=step, **kw)
        torch.cuda.synchronize(device)
        for name in ("points", "backup", "anc_idx", "pos_idx", "n", "row0", "matches", "status", "params"):
            a, b = getattr(res, name), getattr(eager, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (replay, name)
        seen.append((res.points.cpu().numpy().copy(), res.anc_idx.cpu().numpy().copy()))
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(seen[i][0], seen[j][0]) and not np.array_equal(seen[i][1], seen[j][1])


def test_one_pair_trains_the_network(device):
    """training_flat_inputs into the model of the training_network case at dropout_prob = 0.5: a finite loss, status 0, a gradient."""
    import training_network_np as tn
    from d3feat_amd import training_pairs as T
    from d3feat_amd.datasets.common import Dataset
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    cfg, inp = tn.config(True), tn.geometry()
    lens = np.asarray(inp["stack_lengths"], np.int32)
    pts = np.ascontiguousarray(inp["points"][0], np.float32)
    trans = np.eye(4, dtype=np.float32)[None]
    res = T.training_pairs(_t(pts, device), _t(lens, device), trans=_t(trans, device), radius=1.5 * cfg.first_subsampling_dl,
                           keypts_num=cfg.keypts_num, min_matches=cfg.keypts_num, seed=1, step=0,
                           augment=dict(T.AUGMENT_3DMATCH, augment_noise=0.001))
    assert res.status.tolist() == [0] and res.n.tolist() == [cfg.keypts_num]
    ds = Dataset("training_pairs")
    ds.device = device
    ds.neighborhood_limits = tn.LIMITS
    flat = T.training_flat_inputs(ds, cfg, res, 0)
    assert flat[-1] is res.trans[0] or torch.equal(flat[-1], res.trans[0])
    assert torch.equal(flat[4 * cfg.num_layers + 4].cpu(), torch.from_numpy(lens))
    model = KernelPointFCNN(iter(()), cfg, weights=dict(tn.variables(True)), device=device)
    model.dropout_prob = 0.5
    model.run(flat)
    assert np.isfinite(float(model.loss.detach())) and model.validation.status.tolist() == [0]
    params = model.backward()
    g = params["layer_0/simple_0/weights"].grad
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
