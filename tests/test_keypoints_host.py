"""Keypoint selection, the layers that need no GPU: the C ABI of d3f_topk_records (exported, bound, host-side argument checks), the
sharded runner with keep="keypoints" under gloo on CPU tensors (a numpy stand-in engine), and the keypoint result files.

The selection itself, for one cloud with scores s and K >= 1 (utils/tester.py:208-213 + geometric_registration/evaluate.py:45-50):

    sel = np.argsort(s, kind="stable")[-K:]          # min(n, K) rows
    out = records[sel]                               # ascending score; ties in ascending row index
"""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

K = 40
N_FRAG = 9
SIZES = [int(x) for x in np.random.default_rng(5).integers(200, 900, N_FRAG)]
SIZES[2], SIZES[7] = 25, 31                     # fragments with fewer than K rows
IDS = ["scene%d/cloud_bin_%d.ply" % (i % 2, i) for i in range(N_FRAG)]


def _topk(rec, k):
    return rec[np.argsort(rec[:, -1], kind="stable")[-k:]]


# ---- 1. C ABI -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def test_topk_entry_points_are_exported_and_bound(lib):
    from d3feat_amd import _lib
    for name in ("d3f_topk_records", "d3f_topk_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    assert "#define D3F_TOPK_MAX 8192" in hdr and _lib.TOPK_MAX == 8192


def test_topk_host_side_argument_checks_need_no_gpu(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(ldx=3, ldd=32, C=32, lds=1, N=1000, B=2, group=2, keep=1, n_cap=1000, k=250, ldo=36, ws=p, ws_bytes=4096, out=p, lens=p, tickets=None):
        return lib.d3f_topk_records(p, ldx, p, ldd, C, p, lds, N, None, lens, B, group, keep, None, n_cap, k, out, ldo, None, None,
                                    tickets, ws, ws_bytes, None)
    for bad in (dict(k=0), dict(k=-1), dict(k=8193), dict(N=-1), dict(n_cap=-1), dict(n_cap=1 << 24), dict(C=0), dict(ldo=35),
                dict(ldd=31), dict(ldx=2), dict(lds=0), dict(B=0), dict(B=256), dict(group=0), dict(keep=0), dict(keep=3),
                dict(out=None), dict(lens=None)):
        assert call(**bad) == -3, bad
    # a cloud too long for LDS beside 8192 candidates: the keys go through the workspace
    need = lib.d3f_topk_workspace_bytes(140000, 2, 70000, 8192)
    assert need >= 140000 * 4
    assert call(N=140000, n_cap=70000, k=8192, ws=None, ws_bytes=0) == -2
    assert call(N=140000, n_cap=70000, k=8192, ws=p, ws_bytes=4096) == -2
    # 250 of 30000: eight workgroups per cloud (slices of >= 2048 rows) leave at most 250 candidates of 12 bytes (+ a count) each
    assert 2 * 8 * (250 * 12 + 4) <= lib.d3f_topk_workspace_bytes(60000, 2, 30000, 250) <= 2 * 8 * (250 * 12 + 4) + 512
    assert call(N=60000, n_cap=30000, k=250, ws=p, ws_bytes=4096, tickets=p) == -2     # split form: the lists do not fit 4096 bytes


def test_topk_op_rejects_cpu_tensors():
    from d3feat_amd import _lib, keypoints
    with pytest.raises(_lib.D3FeatLibraryError):
        keypoints.topk_records(torch.zeros(10, 36), 5)
    with pytest.raises(_lib.D3FeatLibraryError):
        keypoints.topk(torch.zeros(10, 3), torch.zeros(10, 32), torch.zeros(10), 5)


# ---- 2. sharded runner ----------------------------------------------------------------------------------------------------------

def _load(i):
    return np.random.default_rng(100 + i).random((SIZES[i], 3)).astype(np.float32)


def _records(raw):
    """First cloud's records of a fragment: [xyz | 32 x sum | score], scores quantised so that ties occur."""
    n = min(len(raw), 60)
    p = raw[:n]
    score = np.round(p[:, :1] * 8.0) / 8.0
    return np.concatenate([p, np.repeat(p.sum(1, keepdims=True), 32, 1), score], 1).astype(np.float32)


class _Engine:
    """Stand-in with the FragmentEngine interface run_sharded(keep="keypoints") uses."""
    F = 2
    keypoints = K
    keep_clouds = 1

    def __init__(self):
        self.slots = [None, None]
        self.held = {}
        self.fallbacks = 0

    def submit(self, slot, raws):
        assert slot not in self.held and 1 <= len(raws) <= self.F
        self.held[slot] = [r.numpy() for r in raws]

    def fetch(self, slot, packed=False, keypoints=False):
        assert keypoints and not packed
        return [torch.from_numpy(_topk(_records(r), K)) for r in self.held.pop(slot)]


def _hist(raws, layers=5, bins=905):
    h = np.zeros((layers, bins), np.int64)
    for r in raws:
        g = np.random.default_rng(len(r))
        for l in range(layers):
            h[l] += np.bincount(g.integers(5, 60, 300), minlength=bins)[:bins]
    return h


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, overlap_chunk):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from d3feat_amd import parallel, runner
    try:
        strides = []
        real = parallel.ShardCollector

        class Spy(real):
            def __init__(self, *a, **kw):
                strides.append(int(kw.get("frag_rows", 0)))
                super().__init__(*a, **kw)
        parallel.ShardCollector = Spy
        saved = {}
        res = runner.run_sharded(IDS, SIZES, _load, None, None, lambda c, w, l, r: _Engine(), _hist, torch.device("cpu"),
                                 save=lambda fid, kp: saved.__setitem__(fid, kp.clone()), keep="keypoints", overlap_chunk=overlap_chunk,
                                 dst=0)
        if overlap_chunk > 0:
            assert strides == [K]                      # the stride of the chunk exchange: K rows, not a cloud capacity
        assert sorted(saved) == sorted(IDS[i] for i in res["mine"])
        for i in res["mine"]:
            assert torch.equal(saved[IDS[i]], torch.from_numpy(_topk(_records(_load(i)), K)))      # `save` gets the keypoint block
        assert len(res["shards"]) == world
        for r, (rec, rows) in enumerate(res["shards"]):
            assert rows == [min(K, min(SIZES[i], 60)) for i in res["order"][r]]
            if rank != 0 and r != rank:
                assert rec is None
                continue
            o = 0
            for i, n in zip(res["order"][r], rows):
                want = _topk(_records(_load(i)), K)
                assert n == len(want) and np.array_equal(rec[o:o + n].numpy().view(np.uint32), want.view(np.uint32)), i
                o += n
            assert o == rec.shape[0]
        open(os.path.join(out_dir, "ok_%d" % rank), "w").write(",".join(str(i) for i in res["mine"]))
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("overlap_chunk", [0, 2])
def test_sharded_runner_keeps_keypoints_two_ranks_gloo(tmp_path, overlap_chunk):
    """Rank 0 receives per fragment exactly the stand-in's K rows (fewer for the two short fragments), stride K in the overlapped
    exchange."""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), overlap_chunk), nprocs=world, join=True)
    owned = [open(tmp_path / ("ok_%d" % r)).read().split(",") for r in range(world)]
    assert sorted(int(i) for o in owned for i in o if i) == list(range(N_FRAG))


def test_sharded_runner_keypoints_needs_a_keypoint_engine():
    from d3feat_amd import runner

    class Plain(_Engine):
        keypoints = None
    with pytest.raises(ValueError):
        runner.run_sharded(IDS, SIZES, _load, None, None, lambda c, w, l, r: Plain(), _hist, torch.device("cpu"), keep="keypoints")


# ---- 3. result files ------------------------------------------------------------------------------------------------------------

def test_keypoint_files_hold_the_tail_of_the_full_files(tmp_path):
    """K = 500 with ties planted at the K-th place: the consumer's [-250:] and [-50:] (geometric_registration/evaluate.py:47-50) of
    the three keypoint files are bit-equal to the same slices of the full files save_3dmatch_results writes."""
    from d3feat_amd.utils.results import save_3dmatch_keypoints, save_3dmatch_results
    rng = np.random.default_rng(11)
    n, k = 3000, 500
    s = rng.standard_normal(n).astype(np.float32)
    v = np.sort(s)[-k]
    below = np.nonzero(s < v)[0]
    s[rng.permutation(below)[:5]] = v
    d = np.sort(s)[::-1]
    assert d[k - 1] == d[k]
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    feat = rng.standard_normal((n, 32)).astype(np.float32)
    rec = np.concatenate([pts, feat, s[:, None]], 1)
    stacked = [np.concatenate([a, a]) for a in (pts, feat, s[:, None])]
    full = save_3dmatch_results(str(tmp_path / "full"), "scene/cloud_bin_3.ply", *stacked, n)
    kp = save_3dmatch_keypoints(str(tmp_path / "kp"), "scene/cloud_bin_3.ply", _topk(rec, k))
    assert [os.path.relpath(p, tmp_path / "full") for p in full] == [os.path.relpath(p, tmp_path / "kp") for p in kp]
    for a, b in zip(full, kp):
        A, B = np.load(a), np.load(b)
        assert B.shape == (k,) + A.shape[1:] and A.dtype == B.dtype == np.float32
        for m in (500, 250, 50):
            assert np.array_equal(A[-m:].view(np.uint32), B[-m:].view(np.uint32)), (a, m)
