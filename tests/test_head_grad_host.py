"""d3feat_amd.ops.detect_head_backward / neighbor_transpose without a GPU.  The reference cannot emit gradients here (TensorFlow is not
installed), so what is pinned is the DEFINITION (include/d3feat_amd.h, tests/head_grad_np.py): against float64 torch autograd of a
line-by-line torch restatement of models/D3Feat.py:65-115, against difference quotients of oracle.network_np.detection_head_f64 (the
forward that existing tests tie to the reference's own Python), the fixture, the transposed table against a brute-force loop, and
the argument errors that come before the device is asked."""
import ctypes
import os

import numpy as np
import pytest
import torch

import head_grad_np as hg
from conftest import GOLDEN
from oracle import head_cases, network_np


def test_restatement_against_torch_float64_autograd():
    """head_grad_np.gradients against autograd of head_grad_np.torch_head in float64: 1e-12 of the path's largest entry.  C in (1, 20,
    32, 33, 64, 128), K in (0, 1, 17), B in (1, 2, 3) with an empty middle cloud, equal-length clouds (pads = 1), a padded
    all-non-positive cloud with two planted exact zeros (pads * C + 2 ties for the maximum 0), the duplicated-column stack, explicit
    pad counts -- and ties of size >= 2 exercised in each of T, W and the cloud maximum."""
    tT = tW = tM = 0
    for name in ("c1", "c20", "c32", "c33", "c64", "c128", "k0", "k1", "b1", "b3empty", "eqlen", "negzero", "negzero_pads", "dup", "pads",
                 "b255", "b255g5", "b129"):
        c = hg.grid_case(name)
        for ev in hg.EVALS:
            gd, gs = hg.seeds_of(c, ev)
            got = hg.gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])
            want = hg.torch_gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])
            big = np.abs(want).max()
            print("%s %s: largest %.3e, difference %.2e" % (name, ev, big, np.abs(got["gx"] - want).max()))
            assert np.abs(got["gx"] - want).max() <= 1e-12 * big, (name, ev)
        tT, tW, tM = max(tT, int(got["T"].sum(1).max())), max(tW, int(got["W"].sum(1).max())), max(tM, int(got["cloud_ties"].max()))
        if name == "negzero":
            assert got["cloud_ties"][1] == 2 + hg.pad_counts(c["lens"])[1] * c["C"] and hg.pad_counts(c["lens"]) == [0, 10]
        if name == "negzero_pads":                          # the explicit vector is a COUNT: neither the derived 10 nor a flag's 1
            assert got["cloud_ties"][1] == 2 + 3 * c["C"]
        if name == "eqlen":
            assert hg.pad_counts(c["lens"]) == [1, 1]
        if name == "dup":                                   # the copied column: every maximum that falls on it is a tie of two
            both = got["T"][:, 3] & got["T"][:, 7]
            assert np.array_equal(got["T"][:, 3], got["T"][:, 7]) and np.array_equal(got["W"][:, 3], got["W"][:, 7]) and both.any()
    assert tT >= 2 and tW >= 2 and tM >= 2
    assert hg.pad_counts([12, 20, 15, 15, 18, 9], 2) == [8, 0, 1, 1, 0, 9] and hg.pad_counts([5, 5, 7], 0) == [2, 2, 0]


def test_restatement_against_difference_quotients_of_the_pinned_forward():
    """Central differences of F(x) = sum gdesc * desc + sum gscore * score with (desc, score) = oracle.network_np.detection_head_f64
    on a few entries of a small stack away from every tie: each cloud's maximum (the path through den_b), entries of a row, of one of
    its neighbours and of a row with shadow slots only.
    Tolerance, from the step h = 1e-6 (the perturbed values are exact in float64), for a stack kept at |x_i| >= 1, w_i >= 0.1 and
    den_b >= 1 (asserted; |y| <= 1 then, since y = x / (max + 1e-6)):
      rounding    F is a sum of n (C + 1) products of magnitude <= 3 max|seed| and carries about 64 * 2^-52 of sum |terms|, divided by
                  2 h;
      truncation  h^2 / 6 |F'''| along one coordinate.  desc = x / |x| is homogeneous of degree 0: its third derivatives are at most
                  15 / |x|^3 <= 15, times sum_c |gdesc|.  score = softplus(d) y / (1e-6 + w): softplus has derivatives <= 1, the
                  quotient's third derivative in y is at most 6 |y| / w^4 <= 6e4, Leibniz over the two factors at most 8 times the
                  larger, d y / d x <= 1 / den <= 1: 8 * 6e4 per row, times the rows one entry reaches (all of its cloud through den_b),
                  times max |gscore|."""
    C, K, lens, h = 8, 5, (12, 9), 1e-6
    for k in range(64):
        x, nb = head_cases.head_case(500 + k, C, K, lens, specials=False)
        P = hg.forward_parts(x, nb, lens)
        try:
            hg.margins(x, nb, lens, parts=P)
        except AssertionError:
            continue
        if (np.sqrt((P["x"] ** 2).sum(1)) >= 1).all() and (P["w"] >= 0.1).all() and (P["den"] >= 1).all():
            break
    else:
        raise AssertionError("no stack found")
    n = sum(lens)
    rng = np.random.default_rng(5)
    gd, gs = rng.normal(size=(n, C)), rng.normal(size=n)
    x = x.astype(np.float64)
    terms = 3 * (np.abs(gd).sum() + np.abs(gs).sum())
    tol = 64 * 2.0 ** -52 * terms / (2 * h) + h * h / 6 * (15 * np.abs(gd).sum(1).max() + 8 * 6e4 * max(lens) * np.abs(gs).max())
    assert tol < 2e-5

    def value(xx):
        desc, score, _ = network_np.detection_head_f64(xx, nb, lens)
        return (desc * gd).sum() + (score * gs).sum()
    got = hg.gradients(x, nb, lens, gd, gs)
    assert got["T"].sum(1).max() == 1 and got["W"].sum(1).max() == 1 and got["cloud_ties"].max() == 1
    entries = [np.unravel_index(np.argmax(x[:12]), (12, C)), tuple(np.add(np.unravel_index(np.argmax(x[12:]), (9, C)), (12, 0)))]
    valid = (nb[3] >= 0) & (nb[3] < n)
    entries += [(3, c) for c in range(C)] + [(int(nb[3][valid][0]), c) for c in (0, 5)] + [(15, 1), (20, 7)]
    worst = 0.0
    for r, c in entries:
        xp, xm = x.copy(), x.copy()
        xp[r, c] += h
        xm[r, c] -= h
        q = (value(xp) - value(xm)) / (xp[r, c] - xm[r, c])
        worst = max(worst, abs(q - got["gx"][r, c]))
    print("largest |quotient - gradient| %.2e (tolerance %.2e, largest entry %.2e)" % (worst, tol, np.abs(got["gx"]).max()))
    assert worst <= tol


def test_fixture_against_the_restatement():
    """tests/golden/head_grad.npz (tools/make_golden_head_grad.py): the stored float64 gradients are what head_grad_np gives today, the
    seeds are the ones grid_case finds, the margins hold, and the recorded float32 deviations are of the size measured when the
    fixture was made (some 1e-7 of the largest entry)."""
    path = os.path.join(GOLDEN, "head_grad.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    names = [str(s) for s in z["names"]]
    assert names == list(hg.GRID) and [str(s) for s in z["evaluations"]] == list(hg.EVALS)
    checked = 0
    for at, name in enumerate(names):
        c = hg.grid_case(name)
        assert c["seed"] == int(z["seeds"][at]), name
        assert np.allclose([min(c["margins"][k], 1e300) for k in z["margin_names"]], z["margins"][at], rtol=1e-12, atol=0), name
        assert (z["margins"][at][:3] >= hg.REL_GAP).all() and z["margins"][at][3] >= 2
        real = z["largest"][at] > 1e-6                     # (C = 1: the (gdesc, 0) gradient of a non-clamp row is identically zero)
        # (at most 3.8e-7 of the largest entry when made; C = 1, both: 1.5e-6 -- the descriptor path's rounding around an exact zero)
        assert (z["err32"][at][real] <= 2e-6 * z["largest"][at][real]).all() and (z["err32_clamp"][at] <= 1e-6 * z["largest_clamp"][at]).all(), name
        if c["C"] > 1:                                     # without the clamp rows an ordinary row's entries are of order 1, not 1e5
            assert (z["largest"][at] < 50).all(), name
            if max(c["lens"]) >= 6:                        # (head_case plants a clamp row in every cloud of six rows or more)
                assert (z["largest_clamp"][at][[0, 2]] > 1e4).all(), name
            else:
                assert not z["largest_clamp"][at].any() and not z["err32_clamp"][at].any(), name
        assert (name in hg.NEGATIVE_ROWS) == bool(np.isfinite(z["err32_rel"][at]).all())
        for e, ev in enumerate(hg.EVALS):
            if "gx_%s_%s" % (name, ev) not in z.files:
                continue
            gd, gs = hg.seeds_of(c, ev)
            got = hg.gradients(c["x"], c["nb"], c["lens"], gd, gs, c["group"], c["pads"])["gx"]
            want = z["gx_%s_%s" % (name, ev)]
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, ev)
            checked += 1
    assert checked == 3 * len(hg.STORED)


def test_transpose_np_against_a_brute_force_loop():
    """transpose_np (argsort, searchsorted) against "who names j": a loop over j, edges in ascending e."""
    rng = np.random.default_rng(3)
    for n, N, K in ((0, 3, 4), (7, 7, 0), (9, 12, 5), (40, 40, 17)):
        nb = rng.integers(-3, n + 4, (N, K)).astype(np.int32)
        if n > 2:
            nb[1, :] = 2                                     # a row that names one neighbour K times
            nb[nb == 0] = 1                                  # a row nobody names
        start, edges = hg.transpose_np(nb, n, N)
        flat = nb[:n].reshape(-1)
        pos = 0
        for j in range(N + 1):
            assert start[j] == pos
            if j < n:
                who = [e for e in range(n * K) if flat[e] == j]
                assert edges[pos:pos + len(who)].tolist() == who
                pos += len(who)
        assert pos == len(edges) == int(((flat >= 0) & (flat < n)).sum())
        if n > 2 and K:
            assert start[1] == start[0] and start[3] - start[2] >= K


def _args(N=20, C=32, K=8, B=2, **over):
    a = dict(x=torch.zeros(N, C), neighbors=torch.zeros(N, K, dtype=torch.int32), stack_lengths_dev=torch.zeros(B, dtype=torch.int32),
             include_zero_dev=None, grad_desc=torch.zeros(N, C), grad_score=torch.zeros(N))
    a.update(over)
    return a


def test_argument_errors():
    """The checks of detect_head_backward and neighbor_transpose, made before the device is asked for."""
    from d3feat_amd import _lib
    from d3feat_amd.models.D3Feat import detection_head_backward
    from d3feat_amd.ops import detect_head_backward, neighbor_transpose
    with pytest.raises(TypeError):
        detect_head_backward(**_args(x=torch.zeros(20, 32, dtype=torch.float64)))
    with pytest.raises(TypeError):
        detect_head_backward(**_args(neighbors=torch.zeros(20, 8, dtype=torch.int64)))
    with pytest.raises(TypeError):
        detect_head_backward(**_args(x=np.zeros((20, 32), np.float32)))
    with pytest.raises(ValueError, match="128"):
        detect_head_backward(**_args(C=129))
    with pytest.raises(ValueError, match="neighbour rows"):
        detect_head_backward(**_args(neighbors=torch.zeros(19, 8, dtype=torch.int32)))
    with pytest.raises(ValueError, match="grad_desc"):
        detect_head_backward(**_args(grad_desc=torch.zeros(19, 32)))
    with pytest.raises(ValueError, match="grad_desc"):
        detect_head_backward(**_args(grad_desc=torch.zeros(20, 31)))
    with pytest.raises(ValueError, match="grad_score"):
        detect_head_backward(**_args(grad_score=torch.zeros(21)))
    with pytest.raises(ValueError, match="grad_score"):
        detect_head_backward(**_args(grad_score=torch.zeros(20, 2)))
    with pytest.raises(ValueError, match="clouds"):
        detect_head_backward(**_args(B=0))
    with pytest.raises(ValueError, match="clouds"):
        neighbor_transpose(torch.zeros(20, 8, dtype=torch.int32), torch.zeros(256, dtype=torch.int32))
    with pytest.raises(ValueError, match="include_zero_dev"):
        detect_head_backward(**_args(include_zero_dev=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="stack_group"):
        detect_head_backward(**_args(), stack_group=-1)
    with pytest.raises(ValueError, match="out"):
        detect_head_backward(**_args(), out=torch.zeros(20, 31))
    with pytest.raises(TypeError):
        neighbor_transpose(torch.zeros(20, 8), torch.zeros(2, dtype=torch.int32))
    # well-formed host tensors: there is no CPU path
    with pytest.raises(_lib.D3FeatLibraryError):
        detect_head_backward(**_args())
    with pytest.raises(_lib.D3FeatLibraryError):
        neighbor_transpose(torch.zeros(20, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.D3FeatLibraryError):
        detection_head_backward(torch.zeros(20, 32), dict(neighbors=[torch.zeros(20, 8, dtype=torch.int32)], stack_lengths=[12, 8]),
                                torch.zeros(20, 32), None)


def test_entry_points_refuse_bad_sizes_before_the_device():
    from d3feat_amd import _lib
    lib = _lib.load()
    for name in ("d3f_neighbor_transpose", "d3f_neighbor_transpose_workspace_bytes", "d3f_detect_head_backward",
                 "d3f_detect_head_backward_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def transpose(N=10, ld=8, K=8, B=2, start=p, edges=p, ws=(p, 1 << 16)):
        return lib.d3f_neighbor_transpose(p, N, ld, K, p, B, start, edges, ws[0], ws[1], None)
    for bad in (dict(N=1 << 20, ld=1 << 11, K=1 << 11), dict(N=524287, ld=4096, K=4096), dict(ld=7), dict(B=0), dict(B=256), dict(start=None),
                dict(edges=None), dict(N=-1),
                dict(K=-1, ld=0)):
        assert transpose(**bad) == -3, bad
    assert transpose(ws=(p, 64)) == -2 and transpose(ws=(None, 0)) == -2
    size = lib.d3f_neighbor_transpose_workspace_bytes
    assert size(-1, 8) == 0 and size(8, -1) == 0 and size(1 << 20, 1 << 11) == 0 and size(524287, 4096) == 0      # 2^31 - 4096 slots
    assert 0 < size(0, 8) <= size(10, 8) <= size(1000, 8) <= size(30000, 40) and size(30000, 40) >= 16 * 30000 * 40

    def backward(N=10, ldx=32, C=32, ld=8, K=8, group=0, B=2, start=p, edges=p, gd=p, ldg=32, gs=p, ldgs=1, gx=p, ldgx=32, ws=(p, 1 << 16)):
        return lib.d3f_detect_head_backward(p, N, ldx, C, p, ld, K, p, None, group, B, start, edges, gd, ldg, gs, ldgs, gx, ldgx, ws[0], ws[1],
                                            None)
    for bad in (dict(N=-1), dict(C=0), dict(C=129, ldx=132, ldg=132, ldgx=132), dict(ldx=31), dict(ld=7), dict(K=-1, ld=0), dict(group=-1),
                dict(B=0), dict(B=256), dict(start=None), dict(edges=None), dict(gx=None), dict(ldg=31), dict(ldgs=0), dict(ldgx=31),
                dict(N=1 << 20, ld=1 << 11, K=1 << 11), dict(N=524287, ld=4096, K=4096)):
        assert backward(**bad) == -3, bad
    assert backward(ws=(p, 64)) == -2 and backward(ws=(None, 0)) == -2
    assert backward(N=0, gx=None, start=None) == 0                                              # nothing to do
    size = lib.d3f_detect_head_backward_workspace_bytes
    assert size(-1, 32, 2) == 0 and size(10, 0, 2) == 0 and size(10, 129, 2) == 0 and size(10, 32, 0) == 0 and size(10, 32, 256) == 0
    assert 0 < size(0, 32, 2) <= size(10, 32, 2) <= size(1000, 32, 2) <= size(30000, 32, 2)
    for C in (1, 32, 128):                                                                       # (8 C + 12) bytes per row of capacity
        assert 60000 * (8 * C + 12) <= size(60000, C, 2) <= 60000 * (8 * C + 12) + 8 * 256
