"""The chained resident contraction (d3f_gemm_x3_chain, csrc/gemm_x3.h): a contraction to 64 / 128 columns whose finished tile is
contracted on to 32 columns from the accumulators, in the same launch.  Claims checked here, at small M (the entry point always
takes the resident form; the routing threshold of 65536 rows is not under test):
  * the first output, where stored, has the bits of d3f_gemm_x3 on the same operands;
  * the second output is (that fp32 first output) @ W2 with the second epilogue: against float64 within the bound
    tests/test_gpu_gemm_x3.py applies to the kernel family, and no worse than the two-launch form beyond a factor of two;
  * the k-permutation of the packed W2 image is the kernel's: integer operands, bit for bit the two-launch result;
  * rows at and beyond a device-resident row count are not written; the argument rules; the network routing and its switch.
Shapes: (K, N) = (256, 64), [ gathered (indices -1 and >= N1 among them) | skip ], first output not stored -- the decoder pair; and
(32 + 64, 128) as [A1 | A2], first output stored -- the encoder pair.  Rows 1, 31, 32, 33 (less than a tile, the tile edge), 257 (more
tiles than one workgroup's first round: waves without a tile beside waves with one), 773 (more than one workgroup); the float64
comparison also at 32 * 8 * CUs * 2 + 33 rows, where every wave walks two or three tiles (the bit-for-bit tests of that regime are
tests/test_gpu_gemm_branches.py::test_x3_chain_walk)."""
import numpy as np
import pytest
import torch

from conftest import surface_cloud

pytestmark = pytest.mark.gpu
ROWS = (1, 31, 32, 33, 257, 773)
SHAPES = {"decoder": (128, 128, 64, False), "encoder": (32, 64, 128, True)}        # C1, C2, N, first output stored
N1 = 97                                                                           # rows of the gather source


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(autouse=True)
def _x3_for_every_width(monkeypatch):
    """The two-launch form beside it runs d3f_gemm_x3 at every width (the host keeps small 32-column layers on the fp32 kernel)."""
    from d3feat_amd import ops
    monkeypatch.setattr(ops, "_x3_ok", lambda C1, C2, N, rows=0: ops.GEMM_X3 and (C1 + C2) % 32 == 0 and (C2 == 0 or C1 % 32 == 0))


def make_case(kind, M, integer=False, seed=0):
    C1, C2, N, _ = SHAPES[kind]
    rng = np.random.default_rng(1000 * seed + M + N)
    if integer:
        # |Y| <= 256 * 6 < 2^11 in quarters after LeakyReLU(0.25), |Y @ W2| <= 128 * 2 * 1536 < 2^19 in quarters, sixteenths after the
        # second LeakyReLU: 23 significant bits at the most -- every product and every partial sum is exact in fp32
        draw = lambda lim, shape: rng.integers(-lim, lim + 1, shape).astype(np.float32)
        c = dict(A=draw(3, (N1 if kind == "decoder" else M, C1)), skip=draw(3, (M, C2)), W=draw(2, (C1 + C2, N)), W2=draw(2, (N, 32)),
                 s1=np.exp2(rng.integers(-1, 2, N)).astype(np.float32), t1=draw(4, N), s2=np.exp2(rng.integers(-1, 2, 32)).astype(np.float32),
                 t2=draw(4, 32), alpha=0.25)
    else:
        f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
        c = dict(A=f(N1 if kind == "decoder" else M, C1), skip=f(M, C2), W=f(C1 + C2, N) / np.float32(np.sqrt(C1 + C2)), W2=f(N, 32) / np.float32(np.sqrt(N)),
                 s1=(1.0 + 0.2 * f(N)), t1=0.1 * f(N), s2=(1.0 + 0.2 * f(32)), t2=0.1 * f(32), alpha=0.2)
    c["idx"] = None
    if kind == "decoder":
        idx = rng.integers(0, N1, (M, 3)).astype(np.int32)
        idx[::7, 0] = -1                  # shadow / out-of-range indices gather the zero row
        idx[3::11, 0] = N1
        idx[5::13, 0] = N1 + 50
        c["idx"] = idx
    return c


def run_chain(device, kind, c, second_epilogue, out=None, out2=None, tags=None):
    from d3feat_amd import ops
    stored = SHAPES[kind][3]
    A, idx = _t(c["A"], device), (_t(c["idx"], device) if c["idx"] is not None else None)
    for t, (n_dev, hint) in (tags or {}).items():
        obj = {"A": A, "idx": idx}[t]
        obj.n_dev, obj.n_hint = n_dev, hint
    e2 = dict(col_scale2=_t(c["s2"], device), col_shift2=_t(c["t2"], device), leaky2=True, alpha2=c["alpha"]) if second_epilogue else {}
    return ops.gemm_chain(A, _t(c["W"], device), _t(c["W2"], device), idx=idx, skip=_t(c["skip"], device), store_first=stored,
                          col_scale=_t(c["s1"], device), col_shift=_t(c["t1"], device), leaky=True, alpha=c["alpha"], out=out, out2=out2, **e2)


def run_two_launches(device, kind, c, second_epilogue):
    """-> (Y, C2) of d3f_gemm_x3 twice on the same operands."""
    from d3feat_amd import ops
    W, s1, t1 = _t(c["W"], device), _t(c["s1"], device), _t(c["t1"], device)
    if kind == "decoder":
        u = ops.UpsampleCat(_t(c["A"], device), _t(c["idx"], device), _t(c["skip"], device))
        Y = ops.gemm_upsample_cat(u, W, col_scale=s1, col_shift=t1, leaky=True, alpha=c["alpha"])
    else:
        Y = ops.gemm_cat2(_t(c["A"], device), _t(c["skip"], device), W, col_scale=s1, col_shift=t1, leaky=True, alpha=c["alpha"])
    e2 = dict(col_scale=_t(c["s2"], device), col_shift=_t(c["t2"], device), leaky=True, alpha=c["alpha"]) if second_epilogue else {}
    return Y, ops.gemm(Y, _t(c["W2"], device), **e2)


def second_reference(c, Y, second_epilogue):
    """float64 of (the fp32 first output) @ W2 with the second epilogue."""
    r = Y.astype(np.float64) @ c["W2"].astype(np.float64)
    if second_epilogue:
        r = r * c["s2"].astype(np.float64) + c["t2"].astype(np.float64)
        r = np.where(r > 0, r, r * np.float64(np.float32(c["alpha"])))
    return r


@pytest.mark.parametrize("second_epilogue", [False, True], ids=["identity", "bn_leaky"])
@pytest.mark.parametrize("M", ROWS + ("walk",))
@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_against_the_two_launch_form_and_float64(device, kind, M, second_epilogue, capsys):
    if M == "walk":       # two full rounds of this device's waves and 33 rows more: every wave walks two tiles or three
        M = 32 * 8 * torch.cuda.get_device_properties(device).multi_processor_count * 2 + 33
    c = make_case(kind, M)
    Y, got = run_chain(device, kind, c, second_epilogue)
    Y2, two = run_two_launches(device, kind, c, second_epilogue)
    assert tuple(got.shape) == (M, 32)
    if SHAPES[kind][3]:
        assert torch.equal(Y.view(torch.int32), Y2.view(torch.int32))      # the stored first output: the bits of d3f_gemm_x3
    else:
        assert Y is None
    ref = second_reference(c, Y2.cpu().numpy(), second_epilogue)
    scale = max(1.0, np.abs(ref).max())
    err, err_two = np.abs(got.cpu().numpy() - ref).max(), np.abs(two.cpu().numpy() - ref).max()
    with capsys.disabled():
        print("\n[gemm_chain %s M=%d %s] max error chained %.3e, two launches %.3e, bound %.3e" %
              (kind, M, "bn_leaky" if second_epilogue else "identity", err, err_two, 4e-6 * scale))
    assert err <= 4e-6 * scale
    assert err <= 2 * err_two + 2.0 ** -23 * scale


@pytest.mark.parametrize("M", [33, 773])
@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_the_k_permutation_of_w2(device, kind, M):
    """Integer-valued operands: every product and sum is exact whatever the order, so a W2 image packed in any other k order than
    the kernel's shows at once."""
    c = make_case(kind, M, integer=True)
    _, got = run_chain(device, kind, c, True)
    Y2, two = run_two_launches(device, kind, c, True)
    want = second_reference(c, Y2.cpu().numpy(), True)
    assert np.array_equal(two.cpu().numpy().astype(np.float64), want)         # (the case really is exact)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_capacity_rows_stay_untouched(device, kind):
    """A capacity of 773 rows with 500 of them live (device-resident count): the rows beyond keep the caller's fill in both outputs."""
    cap, live = 773, 500
    C1, C2, N, stored = SHAPES[kind]
    c = make_case(kind, cap, seed=3)
    n_dev = torch.tensor([live], dtype=torch.int32, device=device)
    out = torch.full((cap, N), 12345.0, device=device) if stored else None
    out2 = torch.full((cap, 32), 54321.0, device=device)
    Y, got = run_chain(device, kind, c, True, out=out, out2=out2, tags={"idx" if kind == "decoder" else "A": (n_dev, live)})
    assert got.data_ptr() == out2.data_ptr() and got.n_dev is n_dev
    Yfull, full = run_chain(device, kind, c, True)
    assert torch.equal(got[:live], full[:live]) and bool((out2[live:] == 54321.0).all())
    if stored:
        assert torch.equal(Y[:live], Yfull[:live]) and bool((out[live:] == 12345.0).all())


def test_predicate_and_argument_rules(device):
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    ok = lib.d3f_gemm_x3_chain_ok
    assert ok(100000, 64, 256, 0, 0) == 1 and ok(100000, 128, 96, 1, 0) == 1
    assert ok(100000, 64, 256, 1, 0) == 0           # W (120 KB) + W2 + the patches: beyond the LDS
    assert ok(100000, 128, 128, 1, 0) == 0 and ok(100000, 32, 64, 1, 0) == 0 and ok(100000, 96, 64, 1, 0) == 0
    assert ok(1000, 64, 256, 0, 0) == 0 and ok(100000, 64, 256, 0, 1000) == 0      # not a call of the resident form
    assert ops.gemm_chain_ok(100000, 64, 256, False) and not ops.gemm_chain_ok(1000, 64, 256, False)
    M = 64
    A, out2 = torch.zeros((M, 256), device=device), torch.full((M, 32), 7.0, device=device)
    wx = torch.zeros(int(lib.d3f_gemm_x3_packed_bytes(256, 128)), dtype=torch.uint8, device=device)
    w2x = torch.zeros(int(lib.d3f_gemm_x3_packed_bytes(128, 32)), dtype=torch.uint8, device=device)
    first = torch.full((M, 128), 7.0, device=device)

    def call(K=256, N=64, C=None, c2=out2.data_ptr(), ldc2=32, w2=w2x.data_ptr()):
        return lib.d3f_gemm_x3_chain(A.data_ptr(), M, 256, K, None, 0, None, 0, 0, wx.data_ptr(), C, N, M, N, None, None, None, None, 0, 1, 0.2,
                                     w2, None, None, 0, 0.2, c2, ldc2, None, None, None)
    assert call(N=32) == -3 and call(N=96) == -3                     # 64 or 128 columns only
    assert call(C=first.data_ptr()) == -3                            # K = 256 with the first output stored: the LDS image does not fit
    assert call(K=128, N=128, C=first.data_ptr()) == -3
    assert call(c2=None) == -3 and call(c2=out2.data_ptr() + 4) == -3 and call(ldc2=30) == -3 and call(w2=None) == -3
    assert call(K=48) == -3                                          # d3f_gemm_x3's own rules
    assert lib.d3f_gemm_pack_x3_chain(A.data_ptr(), 32, 96, 32, w2x.data_ptr(), None) == -3
    torch.cuda.synchronize()
    assert bool((out2 == 7.0).all()) and bool((first == 7.0).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out2 == 0.0).all())


def _forward(device, cfg, W, flat):
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    model = KernelPointFCNN(flat, cfg, weights=W)
    return model.out_features, model.out_scores


def test_network_routing_and_switch(device, monkeypatch):
    """The whole network on one small fragment pair with the row threshold of the predicate overridden: both pairs of launches are
    chained, descriptors and scores stay within the benchmark's 1e-4 of the unchained run; with the switch off no chained launch is
    made and the result has the bits of a run that was never offered the chained form."""
    from d3feat_amd import ops
    from d3feat_amd.datasets.common import FragmentDataset
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    cloud = surface_cloud(43, n_raw=30000)
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    ds = FragmentDataset([cloud], fast=True)
    ds.neighborhood_limits = np.asarray([37, 35, 36, 38, 38], np.int32)
    gen, _, _ = ds.get_batch_gen('test', cfg)
    flat = ds.get_tf_mapping(cfg)(*ds._to_device(next(iter(gen()))))
    calls = []
    chain = ops.gemm_chain
    monkeypatch.setattr(ops, "gemm_chain", lambda *a, **k: (calls.append(k.get("store_first", True)), chain(*a, **k))[1])
    plain_d, plain_s = _forward(device, cfg, W, flat)                # below the threshold: the launches of every run before
    assert calls == []
    monkeypatch.setattr(ops, "CHAIN_MIN_ROWS", 1)
    on_d, on_s = _forward(device, cfg, W, flat)
    assert sorted(calls) == [False, True]                            # the decoder pair and the encoder pair, once each
    assert (on_d - plain_d).abs().max().item() <= 1e-4 and (on_s - plain_s).abs().max().item() <= 1e-4
    assert not torch.equal(on_d, plain_d)                            # (the second sums run in another order)
    del calls[:]
    monkeypatch.setattr(ops, "GEMM_CHAIN", False)
    off_d, off_s = _forward(device, cfg, W, flat)
    assert calls == [] and torch.equal(off_d, plain_d) and torch.equal(off_s, plain_s)
