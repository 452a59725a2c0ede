"""The pair loops `for (p = blockIdx; p < P; p += gridDim)` of the one-call entry points on the MI355X, past the 65535-workgroup cap of
their grids, and calls of 9000 pairs -- more than the Python front ends pass in one entry-point call (PAIRS_PER_CALL = 4096).

tests/pair_limit_cases.py makes, per entry point, seven pair kinds; pair p of a call is kind p % 7.  Each test first holds the call of
the seven kinds (P = 7) against the definition the project already has -- matching_np.match_counts, overlap_np.overlap,
repeatability_np.repeat_counts (integers), validation_np.figures (the rule of test_gpu_validation.py), loss_grad_np.gradients (the
rule and cap of test_gpu_loss_grad.py), registration.register_keypoints(num_keypts=k) per kind and count (bit for bit, as
test_gpu_register_counts.py) -- and then makes ONE entry-point call of P_BIG = 65535 + 301 pairs through the C ABI (validation_pairs
and loss_gradients through their Python entry points, which pass P whole), every output pre-filled with a sentinel: every word must
equal the seven-kind call's word of kind p % 7, integers as integers, floats by their bits.  Workgroups 0 .. 300 of the pair dimension
run a second pair there, the successor kind of their first (tests/test_pair_limit_host.py): LDS reused after a full pair, after a
`continue`, after an early return.  Nothing has a tolerance of its own.

Sizes: C = 16 everywhere, blocks of at most 300 rows, lists of at most 70 entries.  The largest allocations are loss_gradients'
workspace at P_BIG (1.4 GB from d3f_loss_gradients_workspace_bytes, inside ops.private_workspace, so no later call inherits it) with
4.5 million rows of descriptors and gradients (0.3 GB each), validation_pairs' 0.25 GB and register_pairs_counts' 0.26 GB; each is
allocated once in its test and freed there.

Durations on the MI355X (pytest --durations).  The module alone, 3.3 s with the start of the device: the seven kinds against
register_keypoints 0.48 s, the shared keypoint fixture 0.32 s, match_pairs at P_BIG 0.11 s, repeatability_pairs 0.11 s,
validation_pairs 0.08 s, loss_gradients 0.08 and 0.06 s, register_pairs_counts at P_BIG 0.03 s, every other test under 0.03 s.  Inside
the whole suite (384 s): 0.15 s, then loss_gradients 0.05 s each, validation_pairs 0.05 s, register_pairs_counts at P_BIG 0.03 s,
match_pairs at P_BIG 0.01 s, every other test under 0.01 s.

What the module catches (tried once against a library built with the per-pair accumulators of mp_count_kernel, vp_rows_kernel and
nb_overlap_kernel declared in front of the pair loop): the six P_BIG tests fail at pairs 65535 and up, naming the kinds; the calls of
7 and of 9000 pairs, in which no workgroup runs a second pair, pass.
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_grad_np as lg
import matching_np as mnp
import overlap_np as onp
import pair_limit_cases as plc
import repeatability_np as rnp
import validation_np as vnp

pytestmark = pytest.mark.gpu

SENTINEL = -77
RPC_FIELDS = ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers", "nearest")


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _np_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _filled(shape, dtype, device):
    """An output pre-filled with a sentinel: NaN for floats, -77 for integers."""
    return torch.full(shape, float("nan") if dtype.is_floating_point else SENTINEL, dtype=dtype, device=device)


def _assert_cyclic(big, small, what):
    """big [P, ...] equals small [7, ...] repeated: row p is row p % 7, bit for bit; the first differing rows are reported."""
    P = big.shape[0]
    reps = -(-P // plc.M)
    want = _bits(small).repeat(reps, *([1] * (small.dim() - 1)))[:P]
    got = _bits(big)
    if not torch.equal(got, want):
        bad = (got != want).reshape(P, -1).any(1).nonzero().flatten()
        raise AssertionError("%s: %d of %d pairs differ from their kind; the first: %s (kinds %s)" % (
            what, bad.numel(), P, bad[:10].tolist(), (bad[:10] % plc.M).tolist()))


def _counts_host():
    n = len(plc.KP_COUNTS)
    return (ctypes.c_int * n)(*plc.KP_COUNTS), n


@pytest.fixture(scope="module")
def kp(device):
    """The keypoint kinds on the device: (kinds, kp f32[5, 320, 20], count i32[5])"""
    from d3feat_amd import registration as reg
    kinds = plc.keypoint_kinds()
    kpt, count = reg.stack_keypoints(kinds["blocks"], plc.KP_K, device=device)
    assert tuple(kpt.shape) == (len(plc.KP_ROWS), plc.KP_K, plc.KP_C + 4) and count.tolist() == list(plc.KP_ROWS)
    return kinds, kpt, count


def _kp_call(kinds, P, device):
    """pairs i32[P, 2], gt f32[P, 3, 4], gt f64[P, 3, 4] of the cyclic call, on the device"""
    pairs = _dev(plc.cyclic(kinds["pairs"], P), device)
    gt64 = _dev(plc.cyclic(kinds["gts"], P), device)
    return pairs, gt64.to(torch.float32).contiguous(), gt64


# ---- the entry points, P whole in one call, outputs pre-filled ------------------------------------------------------------------------
def _match_pairs(kpt, count, pairs, gt):
    from d3feat_amd import _lib, ops
    lib, dev, P = _lib.load(), kpt.device, pairs.shape[0]
    (n_blocks, K, ld), (ks, n) = kpt.shape, _counts_host()
    ws = torch.empty((lib.d3f_match_pairs_workspace_bytes(P, ctypes.addressof(ks), n),), dtype=torch.uint8, device=dev)
    out = dict(mutual_count=_filled((P, n), torch.int32, dev), gt_inliers=_filled((P, n), torch.int32, dev))
    rc = lib.d3f_match_pairs(kpt.data_ptr(), n_blocks, K, ld, ld - 4, count.data_ptr(), pairs.data_ptr(), P, gt.data_ptr(), plc.KP_THRESHOLD,
                             ctypes.addressof(ks), n, out["mutual_count"].data_ptr(), out["gt_inliers"].data_ptr(), ws.data_ptr(),
                             ws.numel(), ops._stream(dev))
    _lib.check(rc, "match_pairs")
    torch.cuda.synchronize(dev)
    return out


def _register_pairs_counts(kpt, count, pairs, gt):
    from d3feat_amd import _lib, ops
    lib, dev, P = _lib.load(), kpt.device, pairs.shape[0]
    (n_blocks, K, ld), (ks, n), kw = kpt.shape, _counts_host(), plc.RANSAC
    nbytes = lib.d3f_register_pairs_counts_workspace_bytes(P, n_blocks, K, ctypes.addressof(ks), n, kw["max_validation"])
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = dict(T=_filled((P, n, 3, 4), torch.float32, dev), sumd2=_filled((P, n), torch.int64, dev),
               nearest=_filled((P, sum(plc.KP_COUNTS)), torch.int32, dev))
    for f in ("inliers", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers"):
        out[f] = _filled((P, n), torch.int32, dev)
    rc = lib.d3f_register_pairs_counts(
        kpt.data_ptr(), n_blocks, K, ld, ld - 4, count.data_ptr(), pairs.data_ptr(), P, ctypes.addressof(ks), n,
        kw["max_correspondence_distance"], kw["ransac_n"], kw["edge_similarity"], kw["checker_distance"], kw["max_iteration"],
        kw["max_validation"], kw["seed"], gt.data_ptr(), plc.KP_THRESHOLD, out["T"].data_ptr(), out["inliers"].data_ptr(),
        out["sumd2"].data_ptr(), out["validations"].data_ptr(), out["iterations"].data_ptr(), out["best_iteration"].data_ptr(),
        out["mutual_count"].data_ptr(), out["gt_inliers"].data_ptr(), out["nearest"].data_ptr(), ws.data_ptr(), ws.numel(),
        ops._stream(dev))
    _lib.check(rc, "register_pairs_counts")
    torch.cuda.synchronize(dev)
    return out, nbytes


def _register_pairs(kpt, count, pairs, gt, k):
    from d3feat_amd import _lib, ops
    lib, dev, P = _lib.load(), kpt.device, pairs.shape[0]
    (n_blocks, K, ld), kw = kpt.shape, plc.RANSAC
    ws = torch.empty((lib.d3f_register_pairs_workspace_bytes(P, K, k, kw["max_validation"]),), dtype=torch.uint8, device=dev)
    out = dict(T=_filled((P, 3, 4), torch.float32, dev), sumd2=_filled((P,), torch.int64, dev), nearest=_filled((P, k), torch.int32, dev))
    for f in ("inliers", "validations", "iterations", "best_iteration", "mutual_count", "gt_inliers"):
        out[f] = _filled((P,), torch.int32, dev)
    rc = lib.d3f_register_pairs(
        kpt.data_ptr(), n_blocks, K, ld, ld - 4, count.data_ptr(), pairs.data_ptr(), P, k, kw["max_correspondence_distance"],
        kw["ransac_n"], kw["edge_similarity"], kw["checker_distance"], kw["max_iteration"], kw["max_validation"], kw["seed"],
        gt.data_ptr(), plc.KP_THRESHOLD, out["T"].data_ptr(), out["inliers"].data_ptr(), out["sumd2"].data_ptr(),
        out["validations"].data_ptr(), out["iterations"].data_ptr(), out["best_iteration"].data_ptr(), out["mutual_count"].data_ptr(),
        out["nearest"].data_ptr(), None, out["gt_inliers"].data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "register_pairs")
    torch.cuda.synchronize(dev)
    return out


def _repeatability_pairs(kpt, count, pairs, gt64):
    from d3feat_amd import _lib, ops
    lib, dev, P = _lib.load(), kpt.device, pairs.shape[0]
    (n_blocks, K, ld), (ks, n), thr = kpt.shape, _counts_host(), ctypes.c_double(plc.KP_THRESHOLD)
    out = dict(repeat=_filled((P, n), torch.int32, dev), totals=_filled((n,), torch.int64, dev))
    rc = lib.d3f_repeatability_pairs(kpt.data_ptr(), n_blocks, K, ld, count.data_ptr(), pairs.data_ptr(), P, gt64.data_ptr(), 0,
                                     ctypes.addressof(thr), ctypes.addressof(ks), n, out["repeat"].data_ptr(), out["totals"].data_ptr(),
                                     ops._stream(dev))
    _lib.check(rc, "repeatability_pairs")
    torch.cuda.synchronize(dev)
    return out


def _overlap_pairs(grid, N, B, pairs):
    from d3feat_amd import _lib, ops
    lib, dev, P = _lib.load(), pairs.device, pairs.shape[0]
    out = dict(count=_filled((P,), torch.int32, dev), nearest=_filled((P, plc.OV_LD), torch.int32, dev))
    rc = lib.d3f_overlap_pairs(grid.mem.data_ptr(), grid.nbytes, N, B, pairs.data_ptr(), P, plc.OV_THRESHOLD, out["count"].data_ptr(),
                               out["nearest"].data_ptr(), plc.OV_LD, ops._stream(dev))
    _lib.check(rc, "overlap_pairs")
    torch.cuda.synchronize(dev)
    return out


# ---- d3f_match_pairs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def match7(device, kp):
    kinds, kpt, count = kp
    pairs, gt, _ = _kp_call(kinds, plc.M, device)
    return _match_pairs(kpt, count, pairs, gt)


def test_match_pairs_kinds_equal_the_restatement(kp, match7):
    kinds, _, _ = kp
    pairs = [tuple(p) for p in kinds["pairs"].tolist()]
    want_m, want_g = mnp.match_counts(kinds["blocks"], pairs, kinds["gts"], plc.KP_COUNTS, plc.KP_THRESHOLD, C=plc.KP_C)
    assert np.array_equal(match7["mutual_count"].cpu().numpy(), want_m) and np.array_equal(match7["gt_inliers"].cpu().numpy(), want_g)


@pytest.mark.parametrize("P", [plc.P_BIG, plc.P_MID])
def test_match_pairs_in_one_call(device, kp, match7, P):
    kinds, kpt, count = kp
    pairs, gt, _ = _kp_call(kinds, P, device)
    big = _match_pairs(kpt, count, pairs, gt)
    for f in ("mutual_count", "gt_inliers"):
        _assert_cyclic(big[f], match7[f], "match_pairs %s at P = %d" % (f, P))


# ---- d3f_register_pairs_counts -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counts7(device, kp):
    kinds, kpt, count = kp
    pairs, gt, _ = _kp_call(kinds, plc.M, device)
    return _register_pairs_counts(kpt, count, pairs, gt)[0]


def test_register_pairs_counts_kinds_equal_register_keypoints_bit_for_bit(device, kp, counts7, match7):
    from d3feat_amd import registration as reg
    kinds, kpt, count = kp
    pairs, gt, _ = _kp_call(kinds, plc.M, device)
    kw = plc.RANSAC
    res = reg.register_pairs_counts(kpt, count, pairs, num_keypts=plc.KP_COUNTS, gt=gt, distance_threshold=plc.KP_THRESHOLD, nearest=True, **kw)
    for f in RPC_FIELDS:                                           # the entry point called here directly, and through the front end
        assert torch.equal(_bits(counts7[f]), _bits(getattr(res, f))), f
    assert torch.equal(counts7["mutual_count"], match7["mutual_count"]) and torch.equal(counts7["gt_inliers"], match7["gt_inliers"])
    near, rows = res.nearest.cpu().numpy(), kinds["blocks"]
    validated = res.validations.cpu().numpy()
    for p, (a, b) in enumerate(kinds["pairs"].tolist()):
        for c, k in enumerate(plc.KP_COUNTS):
            where = "kind %d = (%d, %d) at count %d" % (p, a, b, k)
            got = res.host(p, c)
            Ns, Nt = (min(len(rows[i]), k) if 0 <= i < len(rows) else 0 for i in (a, b))
            assert np.all(near[p, res.offsets[c] + Ns:res.offsets[c] + k] == -1), where
            if min(Ns, Nt) < kw["ransac_n"]:
                assert got["validations"] == 0 and got["iterations"] == 0 and got["best_iteration"] == -1, where
                assert np.array_equal(got["transformation"], np.eye(4)) and got["fitness"] == 0.0 and got["inlier_rmse"] == 0.0, where
                assert len(got["correspondence_set"]) == 0, where
                if min(Ns, Nt) == 0:
                    assert got["mutual_count"] == 0, where
                    continue
            want = reg.register_keypoints(kpt[a, :len(rows[a])], kpt[b, :len(rows[b])], num_keypts=k, device=device, **kw)
            assert np.array_equal(_np_bits(got["transformation"]), _np_bits(want["transformation"])), where
            assert got["fitness"] == want["fitness"] and got["inlier_rmse"] == want["inlier_rmse"], where
            assert got["validations"] == want["validations"], where
            assert np.array_equal(got["correspondence_set"], want["correspondence_set"]), where
            assert got["mutual_count"] == len(want["correspondences"]), where
    # hypotheses are validated next to kinds with none, in both orders: the `continue`s of rc_score_kernel and rc_select_kernel
    top = len(plc.KP_COUNTS) - 1
    # (kind 2 validated before kind 3 without; kind 5 without before kind 6, or kind 6 without before kind 0)
    assert validated[0, top] == validated[1, top] == validated[2, top] == kw["max_validation"], validated
    assert not validated[list(plc.KP_NO_HYPOTHESES)].any()
    inl = res.inliers.cpu().numpy()
    assert inl[0, top] > 100 and inl[2, top] > 100 and inl[1, top] > 10


@pytest.mark.parametrize("P", [plc.P_BIG, plc.P_MID])
def test_register_pairs_counts_in_one_call(device, kp, counts7, P):
    kinds, kpt, count = kp
    pairs, gt, _ = _kp_call(kinds, P, device)
    big, nbytes = _register_pairs_counts(kpt, count, pairs, gt)
    print("register_pairs_counts: P = %d, workspace %.2f GB" % (P, nbytes / 2.0 ** 30))
    for f in RPC_FIELDS:
        _assert_cyclic(big[f], counts7[f], "register_pairs_counts %s at P = %d" % (f, P))


# ---- d3f_register_pairs, d3f_repeatability_pairs: grids of P workgroups ---------------------------------------------------------------------
def test_register_pairs_of_9000_pairs_in_one_call(device, kp, counts7):
    kinds, kpt, count = kp
    k, c = plc.KP_COUNTS[-1], len(plc.KP_COUNTS) - 1
    pairs, gt, _ = _kp_call(kinds, plc.M, device)
    small = _register_pairs(kpt, count, pairs, gt, k)
    off = sum(plc.KP_COUNTS[:c])
    for f in RPC_FIELDS:                                           # the seven kinds: the figures of register_pairs_counts at that count
        want = counts7[f][:, off:off + k] if f == "nearest" else counts7[f][:, c]
        assert torch.equal(_bits(small[f]), _bits(want.contiguous())), f
    pairs, gt, _ = _kp_call(kinds, plc.P_MID, device)
    big = _register_pairs(kpt, count, pairs, gt, k)
    for f in RPC_FIELDS:
        _assert_cyclic(big[f], small[f], "register_pairs %s at P = %d" % (f, plc.P_MID))


def test_repeatability_pairs_of_9000_pairs_in_one_call(device, kp):
    kinds, kpt, count = kp
    host_pairs = [tuple(p) for p in kinds["pairs"].tolist()]
    pairs, _, gt64 = _kp_call(kinds, plc.M, device)
    small = _repeatability_pairs(kpt, count, pairs, gt64)
    want = rnp.repeat_counts(kinds["blocks"], host_pairs, kinds["gts"], plc.KP_COUNTS, plc.KP_THRESHOLD, "target")
    assert np.array_equal(small["repeat"].cpu().numpy(), want) and np.array_equal(small["totals"].cpu().numpy(), want.sum(0))
    pairs, _, gt64 = _kp_call(kinds, plc.P_MID, device)
    big = _repeatability_pairs(kpt, count, pairs, gt64)
    _assert_cyclic(big["repeat"], small["repeat"], "repeatability_pairs repeat at P = %d" % plc.P_MID)
    total = plc.cyclic(want, plc.P_MID).astype(np.int64).sum(0)
    assert big["totals"].dtype == torch.int64 and np.array_equal(big["totals"].cpu().numpy(), total)
    assert torch.equal(big["totals"], big["repeat"].to(torch.int64).sum(0))


# ---- d3f_overlap_pairs -----------------------------------------------------------------------------------------------------------------
def test_overlap_pairs_in_one_call(device):
    from d3feat_amd import ops, overlap
    kinds = plc.overlap_kinds()
    clouds, host_pairs = kinds["clouds"], [tuple(p) for p in kinds["pairs"].tolist()]
    points, lens = overlap.stack_fragments(clouds, device=device)
    grid = ops.NeighborGrid(points, lens, plc.OV_THRESHOLD)
    N, B = points.shape[0], len(clouds)
    small = _overlap_pairs(grid, N, B, _dev(kinds["pairs"], device))
    count, near = onp.overlap(clouds, host_pairs, plc.OV_THRESHOLD, ld=plc.OV_LD)
    assert np.array_equal(small["count"].cpu().numpy(), count), (small["count"].cpu().numpy(), count)
    got = small["nearest"].cpu().numpy()
    assert np.array_equal(got, near), np.argwhere(got != near)[:10]
    for P in (plc.P_BIG, plc.P_MID):
        big = _overlap_pairs(grid, N, B, _dev(plc.cyclic(kinds["pairs"], P), device))
        for f in ("count", "nearest"):                             # rows no pair owns: -1, as the definition says
            _assert_cyclic(big[f], small[f], "overlap_pairs %s at P = %d" % (f, P))


# ---- d3f_validation_pairs, d3f_loss_gradients -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vp():
    return plc.validation_kinds()


def _vp_args(kinds, P, device):
    """The cyclic call on the device.  n goes as a device tensor: the front end then leaves the range check of n to the kernel."""
    return [_dev(t, device) for t in plc.validation_call(kinds, P)]


KW = dict(safe_radius=plc.VP_RADIUS, keypts_num=plc.VP_KEYPTS_NUM, det_loss_weight=1.0)


def _check_forward(values, status, kinds):
    """values f32[7, 8], status i32[7] of the seven kinds against validation_np.figures and the status rules of the header."""
    from test_gpu_validation import _check
    skip = np.asarray(vnp.SKIP, np.float32)
    assert status.tolist() == list(plc.VP_STATUS)
    for k, (f, s, x, ai, pi) in enumerate(kinds["cases"]):
        if k in plc.VP_EVALUATED:
            want = vnp.figures(f, s, x, ai, pi, plc.VP_RADIUS, plc.VP_KEYPTS_NUM, 1.0)
            _check(values[k], want, plc.VP_C, "kind %d n=%d" % (k, plc.VP_N[k]))
        else:
            assert np.array_equal(values[k, :6], skip) and values[k, 6] == 0.0 and values[k, 7] == float(plc.VP_N[k]), (k, values[k])


def test_validation_pairs_in_one_call(device, vp):
    from d3feat_amd import ops
    from d3feat_amd.validation import PairValidation, validation_pairs
    small = validation_pairs(*_vp_args(vp, plc.M, device), **KW)
    _check_forward(small.values.cpu().numpy(), small.status.cpu().numpy(), vp)
    P = plc.P_BIG
    args = _vp_args(vp, P, device)
    out = PairValidation(P, torch.device(device))
    out.values.fill_(float("nan"))
    out.status.fill_(SENTINEL)
    with ops.private_workspace():
        validation_pairs(*args, out=out, **KW)
        torch.cuda.synchronize(device)
        print("validation_pairs: P = %d, workspace %.2f GB" % (P, out._inputs[-1].numel() / 2.0 ** 30))
        out._inputs = None
    _assert_cyclic(out.values, small.values, "validation_pairs values")
    _assert_cyclic(out.status, small.status, "validation_pairs status")
    # the split totals: the kernel's float64 tree over P pairs against the float64 sum of the same fp32 values
    v = plc.cyclic(small.values.cpu().numpy(), P).astype(np.float64)
    counts = [int(((v[:, k] > 0) if k == 3 else (v[:, k] != 0)).sum()) for k in range(6)]
    assert out.counts.cpu().tolist() == counts
    sums = [float(v[:, k][(v[:, k] > 0) if k == 3 else (v[:, k] != 0)].sum()) for k in range(6)]
    assert np.allclose(out.sums.cpu().numpy(), sums, rtol=1e-12, atol=0)


@pytest.mark.parametrize("loss", ["circle_loss", "desc_loss"])
def test_loss_gradients_in_one_call(device, vp, loss):
    from test_gpu_loss_grad import _check
    from d3feat_amd import ops
    from d3feat_amd.validation import PairGradients, loss_gradients, validation_pairs
    args7 = _vp_args(vp, plc.M, device)
    small = PairGradients(plc.M, args7[0].shape[0], plc.VP_C, torch.device(device))
    for t in (small.features, small.scores, small.values):
        t.fill_(float("nan"))
    loss_gradients(*args7, loss=loss, out=small, **KW)
    fwd = validation_pairs(*args7, **KW)
    assert torch.equal(_bits(small.values), _bits(fwd.values)) and torch.equal(small.status, fwd.status)
    _check_forward(small.values.cpu().numpy(), small.status.cpu().numpy(), vp)
    gf, gs = small.features.cpu().numpy(), small.scores.cpu().numpy()
    for k, case in enumerate(vp["cases"]):
        lo, hi = int(vp["row0"][k]), int(vp["row0"][k + 1])
        if k not in plc.VP_EVALUATED:
            assert not gf[lo:hi].any() and not gs[lo:hi].any(), k      # rows no evaluated pair owns: zeros
            continue
        f, s, x, ai, pi = case
        want = lg.gradients(f, s, x, ai, pi, plc.VP_RADIUS, plc.VP_KEYPTS_NUM, 1.0, loss=loss)
        assert not want["skipped"]
        # (a): float32 torch autograd of the same pair (its skip rule is the forward's: evaluated with keypts_num = 2 there)
        _check(gf[lo:hi], gs[lo:hi], want, ai, pi, plc.VP_C, 1.0, "kind %d %s" % (k, loss), case=case, loss=loss, r=plc.VP_RADIUS)
    P = plc.P_BIG
    args = _vp_args(vp, P, device)
    out = PairGradients(P, args[0].shape[0], plc.VP_C, torch.device(device))
    for t in (out.features, out.scores, out.values):
        t.fill_(float("nan"))
    out.status.fill_(SENTINEL)
    with ops.private_workspace():
        loss_gradients(*args, loss=loss, out=out, **KW)
        torch.cuda.synchronize(device)
        print("loss_gradients: P = %d, %d rows, workspace %.2f GB" % (P, args[0].shape[0], out._inputs[-1].numel() / 2.0 ** 30))
        out._inputs = None
    _assert_cyclic(out.values, small.values, "loss_gradients values")
    _assert_cyclic(out.status, small.status, "loss_gradients status")
    # the gradient rows: the rows of the seven kinds, tiled as the inputs are
    R, reps = int(vp["row0"][-1]), -(-P // plc.M)
    assert out.features.shape[0] == reps * R
    _assert_cyclic(out.features.view(reps, R * plc.VP_C)[:P // plc.M], small.features.view(1, R * plc.VP_C).expand(plc.M, -1).contiguous(),
                   "loss_gradients grad_desc")
    _assert_cyclic(out.scores.view(reps, R)[:P // plc.M], small.scores.view(1, R).expand(plc.M, -1).contiguous(), "loss_gradients grad_score")
    # the last, partial repetition holds the pairs P - P % 7 .. P - 1 and rows no pair owns: zeros there
    tail, last = int(vp["row0"][P % plc.M]), out.features[(reps - 1) * R:]
    assert torch.equal(_bits(last[:tail]), _bits(small.features[:tail])) and not last[tail:].any().item()
    assert torch.equal(_bits(out.scores[(reps - 1) * R:][:tail]), _bits(small.scores[:tail])) and not out.scores[(reps - 1) * R + tail:].any().item()
    del out, args
    torch.cuda.empty_cache()
