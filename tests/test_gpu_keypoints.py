"""Keypoint selection on the device (d3f_topk_records, d3feat_amd.keypoints, FragmentEngine(keypoints=K), register_keypoints).

One definition everywhere, for one cloud with scores s and K >= 1 -- what the reference's testers and consumers compute on the host
(utils/tester.py:208-213 np.argsort(scores); geometric_registration/evaluate.py:45-50 [-num_keypts:]):

    sel = np.argsort(s, kind="stable")[-K:]          # min(n, K) rows
    out = records[sel]                               # ascending score; ties in ascending row index

Results are copies of input rows: every comparison here is on bit patterns, no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expect(rec, K):
    sel = np.argsort(rec[:, -1], kind="stable")[-K:]
    return rec[sel], sel.astype(np.int32)


def _families(rng, n, K):
    """-> {name: scores f32[n]}"""
    fam = {}
    s = rng.standard_normal(n).astype(np.float32)
    fam["normal"] = s
    t = s.copy()
    if n > K:
        v = np.sort(t)[-K]                                   # the K-th largest
        below = np.nonzero(t < v)[0]
        t[rng.permutation(below)[:5]] = v                    # five more rows (all there are when fewer lie below) carry it
        d = np.sort(t)[::-1]
        assert d[K - 1] == d[K], "the threshold must fall inside a run of ties"
    fam["planted"] = t
    fam["thirds"] = (np.round(rng.standard_normal(n) * 3.0) / 3.0).astype(np.float32)
    fam["equal"] = np.full(n, 0.25, np.float32)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 3.5], np.float32)
    m = special[rng.integers(0, len(special), n)]
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]          # a NaN with the sign bit and a payload
    m[rng.random(n) < 0.05] = neg_nan
    fam["special"] = m
    return fam


def _records(rng, s):
    n = len(s)
    rec = rng.standard_normal((n, 36)).astype(np.float32)
    rec[:, 0] = np.arange(n)
    rec[:, -1] = s
    return rec


def _check_cloud(kp, cnt, idx, rec, K, what):
    """kp f32[K, 36], idx i32[K] as the device left them (prefilled with sentinels), cnt int."""
    want, sel = _expect(rec, K)
    assert cnt == len(sel) == min(len(rec), K), what
    assert np.array_equal(idx[:cnt], sel), what
    assert np.array_equal(_bits(kp[:cnt]), _bits(want)), what
    assert np.all(kp[cnt:] == SENTINEL) and np.all(idx[cnt:] == -7), what


@pytest.mark.parametrize("K", [1, 50, 250, 5000, 8192])
@pytest.mark.parametrize("n", [1, 63, 64, 250, 251, 4097, 29369, 40000, 70000])
def test_topk_op_equals_stable_argsort_tail(device, n, K):
    from d3feat_amd import keypoints
    rng = np.random.default_rng(1000 * n + K)
    for name, s in _families(rng, n, K).items():
        rec = _records(rng, s)
        t = torch.from_numpy(rec).to(device)
        # (a) a finished record block (score column: stride 36)
        out = torch.full((1, K, 36), float(SENTINEL), dtype=torch.float32, device=device)
        idx = torch.full((1, K), -7, dtype=torch.int32, device=device)
        cnt = torch.full((1,), -1, dtype=torch.int32, device=device)
        keypoints.topk(t[:, :3], t[:, 3:35], t[:, 35], K, out=out, count=cnt, idx=idx)
        _check_cloud(out[0].cpu().numpy(), int(cnt.item()), idx[0].cpu().numpy(), rec, K, (name, "block"))
        # (b) separate arrays with a contiguous score vector
        xyz, desc, score = t[:, :3].contiguous(), t[:, 3:35].contiguous(), t[:, 35:].contiguous()
        out.fill_(float(SENTINEL))
        idx.fill_(-7)
        cnt.fill_(-1)
        keypoints.topk(xyz, desc, score, K, out=out, count=cnt, idx=idx)
        _check_cloud(out[0].cpu().numpy(), int(cnt.item()), idx[0].cpu().numpy(), rec, K, (name, "arrays"))
    # the allocating front end returns the same rows
    kp, c, ix = keypoints.topk_records(t, K, return_index=True)
    want, sel = _expect(rec, K)
    assert kp.shape == (1, K, 36) and int(c.item()) == len(sel)
    assert np.array_equal(_bits(kp[0, :len(sel)].cpu().numpy()), _bits(want)) and np.array_equal(ix[0, :len(sel)].cpu().numpy(), sel)


@pytest.mark.parametrize("keep", [1, 2])
@pytest.mark.parametrize("K", [250, 5000])
def test_topk_stack_of_fragments_with_and_without_row_map(device, keep, K):
    """12 fragments of two clouds each, different lengths, one cloud empty; keep = 1 keeps the first cloud of every fragment.  With a
    per-cloud row_map permutation (the inputs in an internal order) the call returns the rows and REFERENCE indices of the plain one."""
    from d3feat_amd import keypoints
    rng = np.random.default_rng(77 + keep + K)
    lens = [int(x) for x in rng.integers(100, 9000, 24)]
    lens[6], lens[3], lens[8] = 0, 17, 30000
    s = (np.round(rng.standard_normal(sum(lens)) * 3.0) / 3.0).astype(np.float32)      # many ties: the reference row decides
    rec = _records(rng, s)
    starts = np.concatenate([[0], np.cumsum(lens)])
    row_map = np.concatenate([starts[b] + rng.permutation(lens[b]) for b in range(24)]).astype(np.int32)
    internal = np.empty_like(rec)
    internal[:] = rec[row_map]                       # input row m holds reference row row_map[m]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=device)
    kept = [f * 2 + c for f in range(12) for c in range(keep)]
    results = []
    for arr, rm in ((rec, None), (internal, torch.from_numpy(row_map).to(device))):
        t = torch.from_numpy(arr).to(device)
        out = torch.full((len(kept), K, 36), float(SENTINEL), dtype=torch.float32, device=device)
        idx = torch.full((len(kept), K), -7, dtype=torch.int32, device=device)
        _, cnt, _ = keypoints.topk(t[:, :3].contiguous(), t[:, 3:35].contiguous(), t[:, 35].contiguous(), K, lens=lens_dev, group=2,
                                   keep=keep, row_map=rm, out=out, idx=idx, n_cap=30000)
        results.append((out.cpu().numpy(), cnt.cpu().numpy(), idx.cpu().numpy()))
    for out, cnt, idx in results:
        for j, b in enumerate(kept):
            _check_cloud(out[j], int(cnt[j]), idx[j], rec[starts[b]:starts[b + 1]], K, (j, b))
    # the record-block front end on the same stack
    kp, c = keypoints.topk_records(torch.from_numpy(rec).to(device), K, lens=lens, group=2, keep=keep)
    assert np.array_equal(c.cpu().numpy(), results[0][1])
    for j in range(len(kept)):
        assert np.array_equal(_bits(kp[j, :int(c[j])].cpu().numpy()), _bits(results[0][0][j, :int(c[j])]))


@pytest.mark.parametrize("keep", [1, 5])
def test_topk_stack_of_255_clouds(device, keep):
    """A stack of D3F_MAX_BATCH = 255 clouds: 51 fragments of five clouds of 0 to 40 rows -- shorter than, as long as and longer than
    K = 16 -- with one cloud of 5000 rows among them; keep = 1 keeps the first cloud of every fragment, keep = 5 all of them.  With and
    without a per-cloud row_map; every kept cloud against the stable argsort tail.  0.01 s (keep = 1) and 0.02 s (keep = 5) on an
    MI355X inside the full suite."""
    from d3feat_amd import keypoints
    B, group, K = 255, 5, 16
    rng = np.random.default_rng(255 + keep)
    lens = [int(x) for x in rng.integers(0, 41, B)]
    lens[0], lens[5], lens[10], lens[130], lens[254] = 16, 0, 17, 5000, 40        # (clouds 0, 5, 10, 130 are kept at keep = 1 too)
    assert min(lens) == 0 and sorted(set(lens))[-2] == 40 and lens.count(0) >= 2
    s = (np.round(rng.standard_normal(sum(lens)) * 3.0) / 3.0).astype(np.float32)      # many ties: the reference row decides
    rec = _records(rng, s)
    starts = np.concatenate([[0], np.cumsum(lens)])
    row_map = np.concatenate([starts[b] + rng.permutation(lens[b]) for b in range(B)]).astype(np.int32)
    internal = np.empty_like(rec)
    internal[:] = rec[row_map]                       # input row m holds reference row row_map[m]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=device)
    kept = [f * group + c for f in range(B // group) for c in range(keep)]
    assert len(kept) == 51 * keep and 130 in kept
    results = []
    for arr, rm in ((rec, None), (internal, torch.from_numpy(row_map).to(device))):
        t = torch.from_numpy(arr).to(device)
        out = torch.full((len(kept), K, 36), float(SENTINEL), dtype=torch.float32, device=device)
        idx = torch.full((len(kept), K), -7, dtype=torch.int32, device=device)
        _, cnt, _ = keypoints.topk(t[:, :3].contiguous(), t[:, 3:35].contiguous(), t[:, 35].contiguous(), K, lens=lens_dev, group=group,
                                   keep=keep, row_map=rm, out=out, idx=idx, n_cap=5000)
        results.append((out.cpu().numpy(), cnt.cpu().numpy(), idx.cpu().numpy()))
    for out, cnt, idx in results:
        assert cnt.tolist() == [min(lens[b], K) for b in kept]
        for j, b in enumerate(kept):
            _check_cloud(out[j], int(cnt[j]), idx[j], rec[starts[b]:starts[b + 1]], K, (j, b))
    # the record-block front end on the same stack
    kp, c = keypoints.topk_records(torch.from_numpy(rec).to(device), K, lens=lens, group=group, keep=keep)
    assert np.array_equal(c.cpu().numpy(), results[0][1])
    for j in range(len(kept)):
        assert np.array_equal(_bits(kp[j, :int(c[j])].cpu().numpy()), _bits(results[0][0][j, :int(c[j])]))


@pytest.mark.parametrize("name", ["network_3dmatch_4k.npz", "network_3dmatch.npz", "network_kitti.npz"])
def test_topk_on_the_network_fixtures(device, name):
    """First cloud of the committed network outputs (real duplicated scores): indices equal the stable expression, and the score
    sequence is bit-equal to the reference's own np.argsort(scores_first_pcd, axis=0)[-K:] (utils/tester.py:208-213; its default sort
    leaves the order inside ties open, the score sequence is the same).  The files hold no level-0 points: xyz carries the row number;
    `features` (one column) stands for the descriptor, which makes a 5-float record: the element-wise store path."""
    from d3feat_amd import keypoints
    z = np.load(os.path.join(GOLDEN, name))
    n = int(z["stack_lengths"][0])
    s = z["scores"][:n].astype(np.float32)
    feat = z["features"][:n].astype(np.float32)
    xyz = np.repeat(np.arange(n, dtype=np.float32)[:, None], 3, 1)
    rec = np.concatenate([xyz, feat, s], 1)
    d = np.sort(s[:, 0])[::-1]
    Ks = sorted({50, 250} | {K for K in range(1, min(n, 8192)) if d[K - 1] == d[K]})
    t = torch.from_numpy(rec).to(device)
    for K in Ks:
        kp, cnt, idx = keypoints.topk_records(t, K, return_index=True)
        c = int(cnt.item())
        want, sel = _expect(rec, K)
        assert c == len(sel) and np.array_equal(idx[0, :c].cpu().numpy(), sel), K
        got = kp[0, :c].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), K
        ref_order = np.argsort(s, axis=0)[-K:]                      # the reference's expression, [K, 1]
        assert np.array_equal(_bits(got[:, -1]), _bits(s[ref_order[:, 0], 0])), K


def test_topk_rejects_cpu_tensors_and_bad_k(device):
    from d3feat_amd import _lib, keypoints
    with pytest.raises(_lib.D3FeatLibraryError):
        keypoints.topk_records(torch.zeros(10, 36), 5)
    t = torch.zeros(10, 36, device=device)
    for K in (0, _lib.TOPK_MAX + 1):
        with pytest.raises(ValueError):
            keypoints.topk_records(t, K)


# ---- engine ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup(device):
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    return cfg, W, np.asarray([37, 35, 36, 38, 38], np.int32)


def _frag(seed, n_raw=40000):
    from d3feat_amd.utils.synthetic import room_fragment
    return room_fragment(seed, n_raw=n_raw, edge=1.0)


class _no_device_reads:
    """Inside: any .item() / .cpu() / .tolist() of a device tensor raises (fetch must live on the replay's one status block)."""

    def __enter__(self):
        self.saved = {k: getattr(torch.Tensor, k) for k in ("item", "cpu", "tolist")}
        for k, fn in self.saved.items():
            def guard(t, *a, _fn=fn, _k=k, **kw):
                if t.is_cuda:
                    raise AssertionError("device read-back through Tensor.%s inside fetch" % _k)
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, guard)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)
        return False


def _same_replay(rec_cloud, kp, K):
    """kp (device view) against the numpy selection from the records of the same replay (one cloud)."""
    r = rec_cloud.cpu().numpy()
    want, _ = _expect(r, K)
    got = kp.cpu().numpy()
    assert got.shape == want.shape == (min(len(r), K), 36)
    assert np.array_equal(_bits(got), _bits(want))


def _pair_of_engines(setup, device, **kw):
    from d3feat_amd.engine import FragmentEngine
    cfg, W, limits = setup
    eng = FragmentEngine(cfg, W, limits, device=device, keypoints=250, **kw)
    plain = FragmentEngine(cfg, W, limits, device=device, **kw)
    for a, b in zip(eng.slots, plain.slots):
        assert a.host_stat.numel() == b.host_stat.numel() and a.dev_stat.numel() == b.dev_stat.numel()
    return eng, plain


@pytest.mark.parametrize("internal", [True, False])
def test_engine_keypoints_single_fragment_paths(device, setup, internal):
    """F = 1: a plain replay, a cloud with fewer than 250 voxels, submit(out=...) and an oversize fragment (eager fallback)."""
    eng, plain = _pair_of_engines(setup, device, raw_cap=45000, n0_cap=14000, slots=1, internal_order=internal)
    K = 250
    raw = torch.from_numpy(_frag(301)).to(device)
    eng.submit(0, raw)
    with _no_device_reads():
        rec, kp = eng.fetch(0, packed=True, keypoints=True)
    assert eng.fallbacks == 0
    n = rec.shape[0] // 2
    _same_replay(rec[:n], kp, K)
    plain.submit(0, raw)
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(plain.fetch(0, packed=True).cpu().numpy()))
    rec_keep = rec.clone()
    # keypoints alone
    eng.submit(0, raw)
    only = eng.fetch(0, keypoints=True)
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(_expect(rec_keep[:n].cpu().numpy(), K)[0]))
    # the default forms of fetch are today's
    eng.submit(0, raw)
    assert np.array_equal(_bits(eng.fetch(0, packed=True).cpu().numpy()), _bits(rec_keep.cpu().numpy()))
    # submit(out=...): the full records go to the caller's buffer, the keypoints do not depend on that
    dst = torch.zeros((eng.kept_rows_cap(), 36), dtype=torch.float32, device=device)
    eng.submit(0, raw, out=dst)
    with _no_device_reads():
        rec2, kp2 = eng.fetch(0, packed=True, keypoints=True)
    assert rec2.data_ptr() == dst.data_ptr() and rec2.shape[0] == n
    assert np.array_equal(_bits(rec2.cpu().numpy()), _bits(rec_keep[:n].cpu().numpy()))
    _same_replay(rec2, kp2, K)
    # fewer than 250 voxels
    g = torch.Generator(device="cpu").manual_seed(5)
    tiny = (torch.rand((400, 3), generator=g) * 0.15).to(device)
    eng.submit(0, tiny)
    rec3, kp3 = eng.fetch(0, packed=True, keypoints=True)
    n3 = rec3.shape[0] // 2
    assert 0 < n3 < 250 and kp3.shape[0] == n3
    _same_replay(rec3[:n3], kp3, K)
    plain.submit(0, tiny)
    assert np.array_equal(_bits(rec3.cpu().numpy()), _bits(plain.fetch(0, packed=True).cpu().numpy()))
    # oversize: more raw points than raw_cap, the eager path
    big = torch.from_numpy(_frag(302, 50000)).to(device)
    before = eng.fallbacks
    eng.submit(0, big)
    rec4, kp4 = eng.fetch(0, packed=True, keypoints=True)
    assert eng.fallbacks == before + 1
    _same_replay(rec4[:rec4.shape[0] // 2], kp4, K)
    plain.submit(0, big)
    assert np.array_equal(_bits(rec4.cpu().numpy()), _bits(plain.fetch(0, packed=True).cpu().numpy()))


@pytest.mark.parametrize("internal", [True, False])
def test_engine_keypoints_batched_partial_and_flagged(device, setup, internal):
    """F = 4: a partial batch of three, and a flagged replay (one fragment beyond the voxel capacity: isolation re-submits, the outlier
    goes eager) -- the three result paths return the same rows."""
    eng, plain = _pair_of_engines(setup, device, raw_cap=45000, n0_cap=9000, slots=1, batch=4, internal_order=internal)
    K = 250
    raws = [torch.from_numpy(_frag(310 + i, m)).to(device) for i, m in enumerate((6000, 8000, 4000))]
    eng.submit(0, raws)
    with _no_device_reads():
        outs = eng.fetch(0, packed=True, keypoints=True)
    assert len(outs) == 3 and eng.fallbacks == 0 and eng.isolated == 0
    plain.submit(0, raws)
    for (rec, kp), want in zip(outs, plain.fetch(0, packed=True)):
        _same_replay(rec[:rec.shape[0] // 2], kp, K)
        assert np.array_equal(_bits(rec.cpu().numpy()), _bits(want.cpu().numpy()))
    # flagged: fragment 1 has ~10 k voxels > n0_cap
    mixed = [raws[0], torch.from_numpy(_frag(320, 40000)).to(device), raws[2], raws[1]]
    eng.submit(0, mixed)
    outs = eng.fetch(0, packed=True, keypoints=True)
    assert eng.isolated == 1 and eng.fallbacks == 1
    plain.submit(0, mixed)
    for (rec, kp), want in zip(outs, plain.fetch(0, packed=True)):
        _same_replay(rec[:rec.shape[0] // 2], kp, K)
        assert np.array_equal(_bits(rec.cpu().numpy()), _bits(want.cpu().numpy()))
    eng.submit(0, mixed)
    only = eng.fetch(0, keypoints=True)
    for kv, (_, kp) in zip(only, outs):
        assert torch.equal(kv, kp)


def test_engine_keypoints_mirror_and_no_stage0(device, setup):
    eng, plain = _pair_of_engines(setup, device, raw_cap=45000, n0_cap=14000, slots=1, batch=2, mirror_self_pair=True)
    K = 250
    raws = [torch.from_numpy(_frag(330 + i, m)).to(device) for i, m in enumerate((30000, 20000))]
    eng.submit(0, raws)
    outs = eng.fetch(0, packed=True, keypoints=True)
    plain.submit(0, raws)
    for (rec, kp), want in zip(outs, plain.fetch(0, packed=True)):
        _same_replay(rec[:rec.shape[0] // 2], kp, K)
        assert np.array_equal(_bits(rec.cpu().numpy()), _bits(want.cpu().numpy()))
    assert eng.fallbacks == 0
    # stage0=False: the cloud is already at the first subsampling resolution
    from d3feat_amd import tf_custom_ops as tfo
    sub = tfo.grid_subsampling(raws[0], 0.03)
    eng, plain = _pair_of_engines(setup, device, n0_cap=14000, slots=1, stage0=False)
    eng.submit(0, sub)
    rec, kp = eng.fetch(0, packed=True, keypoints=True)
    assert eng.fallbacks == 0 and rec.shape[0] == 2 * sub.shape[0]
    _same_replay(rec[:sub.shape[0]], kp, K)
    plain.submit(0, sub)
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(plain.fetch(0, packed=True).cpu().numpy()))


def test_engine_keypoints_two_clouds(device):
    from d3feat_amd.engine import FragmentEngine
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import kitti_config
    from d3feat_amd.utils.synthetic import lidar_sweep
    cfg = kitti_config()
    W = build_variables(cfg, seed=7, randomize_bn=True).values
    limits = np.asarray([25, 25, 25, 25, 25], np.int32)
    kw = dict(raw_cap=250000, n0_cap=30000, level_ratio=0.6, slots=1, device=device, two_clouds=True)
    eng = FragmentEngine(cfg, W, limits, keypoints=250, **kw)
    plain = FragmentEngine(cfg, W, limits, **kw)
    assert eng.slots[0].host_stat.numel() == plain.slots[0].host_stat.numel()
    pair = tuple(torch.from_numpy(lidar_sweep(s, 120000)).to(device) for s in (3, 103))
    eng.submit(0, pair)
    with _no_device_reads():
        rec, (kp_a, kp_b) = eng.fetch(0, packed=True, keypoints=True)
    assert eng.fallbacks == 0
    sl = eng.slots[0]
    na, nb = (int(x) for x in sl.host_stat.numpy()[sl.nstat:sl.nstat + 2])
    assert na + nb == rec.shape[0]
    _same_replay(rec[:na], kp_a, 250)
    _same_replay(rec[na:], kp_b, 250)
    plain.submit(0, pair)
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(plain.fetch(0, packed=True).cpu().numpy()))
    with pytest.raises(ValueError):
        plain.submit(0, pair)
        plain.fetch(0, keypoints=True)


def test_engine_rejects_keypoints_out_of_range(device, setup):
    from d3feat_amd import _lib
    from d3feat_amd.engine import FragmentEngine
    cfg, W, limits = setup
    for K in (0, -3, _lib.TOPK_MAX + 1):
        with pytest.raises(ValueError):
            FragmentEngine(cfg, W, limits, raw_cap=4096, n0_cap=4096, slots=1, device=device, keypoints=K)


# ---- registration ---------------------------------------------------------------------------------------------------------------

def _unit(rng, n, c=32):
    x = rng.standard_normal((n, c)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _pair(seed, n=400, outliers=0.3, noise=0.003):
    """target keypoints on a room surface; source = the same points moved by a known rigid motion (+ noise), a share of the
    descriptors replaced by unrelated ones; scores random, the same for both copies of a point.  -> two record blocks, R, t"""
    from d3feat_amd.utils.synthetic import room_fragment
    rng = np.random.default_rng(seed)
    tgt = room_fragment(seed, n_raw=20000, edge=2.0)[rng.permutation(20000)[:n]].astype(np.float32)
    ang = rng.uniform(-0.6, 0.6, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-0.5, 0.5, 3)
    src = ((tgt.astype(np.float64) - t) @ R + rng.normal(scale=noise, size=tgt.shape)).astype(np.float32)   # source -> target is (R, t)
    perm = rng.permutation(n)
    src = src[perm]
    d_t = _unit(rng, n)
    d_s = d_t[perm] + 0.05 * rng.standard_normal((n, 32)).astype(np.float32)
    bad = rng.random(n) < outliers
    d_s[bad] = _unit(rng, int(bad.sum()))
    d_s /= np.linalg.norm(d_s, axis=1, keepdims=True)
    sc_t = rng.random((n, 1)).astype(np.float32)
    rec_s = np.concatenate([src, d_s.astype(np.float32), sc_t[perm]], 1)
    rec_t = np.concatenate([tgt, d_t, sc_t], 1)
    return rec_s, rec_t, R, t


def test_register_keypoints_equals_ransac_on_the_numpy_tails(device):
    from d3feat_amd import keypoints
    from d3feat_amd import registration as reg
    rec_s, rec_t, R, t = _pair(41, n=400)
    K, num = 300, 250
    kw = dict(max_correspondence_distance=0.05, ransac_n=4, edge_similarity=0.9, checker_distance=0.05, max_iteration=50000,
              max_validation=200, seed=5, batch=8192)
    blocks = []
    for rec in (rec_s, rec_t):
        kp, cnt = keypoints.topk_records(torch.from_numpy(rec).to(device), K)
        assert int(cnt.item()) == K
        blocks.append(kp[0, :K])
    got = reg.register_keypoints(blocks[0], blocks[1], num_keypts=num, **kw)
    tail_s, tail_t = _expect(rec_s, num)[0], _expect(rec_t, num)[0]
    want = reg.ransac_feature_matching(tail_s[:, :3], tail_t[:, :3], tail_s[:, 3:35], tail_t[:, 3:35], device=device, **kw)
    for k in ("fitness", "inlier_rmse", "iterations", "validations"):
        assert got[k] == want[k], k
    assert np.array_equal(got["transformation"], want["transformation"])
    assert np.array_equal(got["correspondence_set"], want["correspondence_set"])
    assert np.array_equal(got["correspondences"], reg.build_correspondence(tail_s[:, 3:35], tail_t[:, 3:35], device=device))
    M = got["transformation"]
    assert np.abs(M[:3, :3] - R).max() < 0.03 and np.abs(M[:3, 3] - t).max() < 0.03 and got["fitness"] > 0.9
