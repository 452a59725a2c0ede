"""d3feat_amd.ops.ind_max_pool_backward / closest_pool_cat_backward without a GPU.  The reference cannot emit gradients here (TensorFlow
is not installed), so what is pinned is the DEFINITION (include/d3feat_amd.h, tests/pool_grad_np.py): against float64 torch autograd of
line-by-line torch restatements of models/network_blocks.py:51-66 and :69-83 + the concatenation, against difference quotients on a
tie-free case, and the argument errors that come before the device is asked."""
import numpy as np
import pytest
import torch

import pool_grad_np as pg

SHAPES = [(40, 17, K, C) for K in (1, 3, 7) for C in (1, 3, 8)] + [(281, 90, 40, 5)]


def test_amax_and_amin_split_ties_evenly():
    """The premise of the comparison below: torch.amax / amin hand a tie equal shares (torch.max(dim) would pick one index)."""
    for fn in (torch.amax, torch.amin):
        v = torch.tensor([[1.5], [1.5]], dtype=torch.float64, requires_grad=True)
        fn(v, dim=0).sum().backward()
        assert v.grad.tolist() == [[0.5], [0.5]]
    v = torch.tensor([[2.0, 2.0, 1.0, 2.0]], dtype=torch.float64, requires_grad=True)
    torch.amax(v, dim=1).sum().backward()
    assert np.allclose(v.grad.numpy(), [[1 / 3, 1 / 3, 0, 1 / 3]], rtol=1e-15)


def _torch_pool_gradient(x, inds, g):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = pg.torch_ind_max_pool(xt, inds)
    (y * torch.as_tensor(g, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy()


def test_max_pool_restatement_against_torch_float64_autograd():
    """Values quantised to multiples of 1/8 (many ties), with the planted cases of pool_grad_np.pool_case: 1e-12 of the largest entry."""
    seen = dict(T=0, shadow=0, M=0)
    for at, (N1, N2, K, C) in enumerate(SHAPES):
        x, inds, g = pg.pool_case(10 + at, N1, N2, K, C, dtype=np.float64)
        y = pg.max_pool_forward(x, inds)
        want_y, want = _torch_pool_gradient(x, inds, g)
        assert np.array_equal(y, want_y)
        p = pg.max_pool_backward(x, inds, y, g, parts=True)
        big = np.abs(want).max()
        print("N1 %d N2 %d K %d C %d: largest %.3e, difference %.2e" % (N1, N2, K, C, big, np.abs(p["gx"] - want).max()))
        assert np.abs(p["gx"] - want).max() <= 1e-12 * big
        # the planted cases are what they claim to be
        assert (p["shadow_ties"][0] == K).all() and (p["T"][0] == K).all()                    # no valid neighbour
        assert p["colmin"][0] == x[5, 0] and p["M"][0] == 1 and p["T"][1, 0] == K and p["shadow_ties"][1, 0] == K - 1
        if C > 1:
            assert p["M"][1] == 3
        if K > 2:
            assert (inds[2] == 7).sum() >= 2
        assert not (inds == 4).any() and (inds[2:, 0] == 3).all()
        valid = (inds >= 0) & (inds < N1)
        named = np.zeros(N1, bool)
        named[inds[valid]] = True
        unnamed = ~named
        assert unnamed[4] and np.array_equal(p["gx"][unnamed], (x[unnamed] == p["colmin"]) * (p["S"] / p["M"]))
        seen = dict(T=max(seen["T"], int(p["T"].max())), shadow=max(seen["shadow"], int(p["shadow_ties"].max())), M=max(seen["M"], int(p["M"].max())))
    assert seen["T"] >= 3 and seen["shadow"] >= 2 and seen["M"] >= 3


def test_sliced_case_against_torch_float64_autograd():
    """pool_grad_np.sliced_pool_case (the case of the GPU test's runs beyond one slice of pooled rows) is what it claims to be, and on it
    the restatement agrees with float64 torch autograd to 1e-12 -- the zeros of both signs included: torch's amin / amax compare
    values, so +0 and -0 tie."""
    S, N1, N2, K = 256, 3 * 256 + 25, 2 * 256 + 7, 7
    for C, zc in ((3, None), (64, None), (4, 2)):
        x, inds, g = pg.pool_case(70 + C, N1, N2, K, C, dtype=np.float64, slice_rows=S, zero_column=zc)
        y = pg.max_pool_forward(x, inds)
        want_y, want = _torch_pool_gradient(x, inds, g)
        assert np.array_equal(y, want_y)
        p = pg.max_pool_backward(x, inds, y, g, parts=True)
        assert np.abs(p["gx"] - want).max() <= 1e-12 * np.abs(want).max()
        shadow = (inds < 0) | (inds >= N1)
        for a in range(0, N2, S):
            assert shadow[a].all() and (p["shadow_ties"][a] == K).all() and (p["T"][a + 1, 0] == K) and (inds[a + 2] == 7).sum() >= 2
            assert (p["T"][a:a + S] >= 2).any() and (inds[a + 1] == N1 - 2).sum() == 1
            assert ((p["shadow_ties"][a:a + S] * p["gs"][a:a + S]).sum(0) != 0).any()
        assert p["M"][0] == 1 and np.nonzero(x[:, 0] == p["colmin"][0])[0].tolist() == [N1 - 2] and p["M"][1] == 3
        assert pg.longest_segment(inds, N1) <= 90 and not (inds == 4).any() and not (inds == S + 4).any()
        if zc is not None:
            zero = x[:, zc] == 0
            assert p["colmin"][zc] == 0 and p["M"][zc] == zero.sum() and zero[[4, S + 4]].all()
            assert not np.signbit(x[:S, zc][zero[:S]]).any() and np.signbit(x[S:, zc][zero[S:]]).all()
            share = p["S"][zc] / p["M"][zc]
            assert share != 0 and np.allclose(p["gx"][[4, S + 4], zc], share, rtol=1e-15)


def test_upsample_restatement_against_torch_float64_autograd():
    for at, (N1, N2, K, C1, C2) in enumerate([(50, 300, 3, 4, 0), (50, 300, 1, 1, 32), (12, 40, 5, 7, 3)]):
        inds, g = pg.upsample_case(20 + at, N1, N2, K, C1, C2, dtype=np.float64)
        rng = np.random.default_rng(at)
        x = torch.tensor(rng.normal(size=(N1, C1)), dtype=torch.float64, requires_grad=True)
        skip = torch.tensor(rng.normal(size=(N2, C2)), dtype=torch.float64, requires_grad=True) if C2 else None
        out = pg.torch_closest_pool_cat(x, inds, skip)
        assert np.array_equal(out.detach().numpy(), pg.upsample_cat_forward(x.detach().numpy(), inds, None if skip is None else skip.detach().numpy()))
        (out * torch.as_tensor(g)).sum().backward()
        gx, gskip = pg.upsample_cat_backward(g, inds, N1, C1)
        big = np.abs(x.grad.numpy()).max()
        assert np.abs(gx - x.grad.numpy()).max() <= 1e-12 * big
        if C2:
            assert np.array_equal(gskip, skip.grad.numpy())
        first = inds[:, 0]
        assert not gx[2].any() and ((first < 0) | (first >= N1)).sum() >= 2          # a row nobody names; shadow indices present
        assert (first == 1).sum() >= N2 - 10 - N2 // 5


def test_restatements_against_difference_quotients():
    """Central differences of F(x) = sum g * y on a tie-free case (all entries of x distinct, spaced by at least 1 / (N1 C) = 2.5e-3, far
    above the step h = 1e-6): F is piecewise LINEAR in x, so inside one piece the quotient is exact up to rounding -- about
    2^-52 sum |g y| / (2 h) <= 1e-8 here."""
    N1, N2, K, C, h = 40, 17, 5, 10, 1e-6
    x, inds, g = pg.pool_case(3, N1, N2, K, C, quantised=False, ties=False, dtype=np.float64)
    inds[0, :] = N1                                                             # a row of shadow slots only: y = colmin
    assert np.diff(np.sort(x.reshape(-1))).min() > 1e-3
    y = pg.max_pool_forward(x, inds)
    p = pg.max_pool_backward(x, inds, y, g, parts=True)
    assert (p["M"] == 1).all() and (p["shadow_ties"][0] == K).all()
    ups, gu = pg.upsample_case(4, N1, 60, 2, C, 0, dtype=np.float64)
    gux, _ = pg.upsample_cat_backward(gu, ups, N1, C)
    rng = np.random.default_rng(1)
    worst = 0.0
    entries = [(int(np.argmin(x[:, c])), c) for c in range(C)] + [(int(r), int(c)) for r, c in zip(rng.integers(0, N1, 40), rng.integers(0, C, 40))]
    for r, c in entries:
        xp, xm = x.copy(), x.copy()
        xp[r, c] += h
        xm[r, c] -= h
        q = ((pg.max_pool_forward(xp, inds) - pg.max_pool_forward(xm, inds)) * g).sum() / (xp[r, c] - xm[r, c])
        worst = max(worst, abs(q - p["gx"][r, c]))
        q = ((pg.upsample_cat_forward(xp, ups) - pg.upsample_cat_forward(xm, ups)) * gu).sum() / (xp[r, c] - xm[r, c])
        worst = max(worst, abs(q - gux[r, c]))
    print("largest |quotient - gradient| %.2e" % worst)
    assert worst <= 1e-7


def test_transpose_np_against_a_brute_force_loop():
    x, inds, _ = pg.pool_case(5, 30, 12, 6, 2)
    start, edges = pg.transpose_np(inds, 30)
    flat = inds.reshape(-1)
    for j in range(30):
        assert edges[start[j]:start[j + 1]].tolist() == [e for e in range(flat.size) if flat[e] == j]
    assert start[30] == len(edges) and pg.longest_segment(inds, 30) == np.diff(start).max() >= 10


def _pool_args(N1=20, N2=9, K=5, C=8, **over):
    a = dict(x=torch.zeros(N1, C), inds=torch.zeros(N2, K, dtype=torch.int32), y=torch.zeros(N2, C), grad_y=torch.zeros(N2, C))
    a.update(over)
    return a


def test_argument_errors():
    """The checks of the two Python entry points, made before the device is asked for."""
    from d3feat_amd import _lib
    from d3feat_amd.ops import closest_pool_cat_backward, ind_max_pool_backward
    with pytest.raises(TypeError):
        ind_max_pool_backward(**_pool_args(x=torch.zeros(20, 8, dtype=torch.bfloat16)))         # fp32 rows only
    with pytest.raises(TypeError):
        ind_max_pool_backward(**_pool_args(inds=torch.zeros(9, 5, dtype=torch.int64)))
    with pytest.raises(TypeError):
        ind_max_pool_backward(**_pool_args(y=np.zeros((9, 8), np.float32)))
    with pytest.raises(ValueError, match="grad_y"):
        ind_max_pool_backward(**_pool_args(grad_y=torch.zeros(9, 7)))
    with pytest.raises(ValueError, match="y is"):
        ind_max_pool_backward(**_pool_args(y=torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="out"):
        ind_max_pool_backward(**_pool_args(), out=torch.zeros(19, 8))
    with pytest.raises(ValueError, match="transpose"):
        ind_max_pool_backward(**_pool_args(), transpose=(torch.zeros(20, dtype=torch.int32), torch.zeros(45, dtype=torch.int32)))
    with pytest.raises(ValueError, match="transpose"):
        ind_max_pool_backward(**_pool_args(), transpose=(torch.zeros(21, dtype=torch.int32), torch.zeros(44, dtype=torch.int32)))
    with pytest.raises(ValueError, match="contiguous rows"):
        ind_max_pool_backward(**_pool_args(x=torch.zeros(8, 20).t()))
    g, inds = torch.zeros(30, 12), torch.zeros(30, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="C1"):
        closest_pool_cat_backward(g, inds, 10, 13)
    with pytest.raises(ValueError, match="C1"):
        closest_pool_cat_backward(g, inds, 10, 0)
    with pytest.raises(ValueError, match="num_coarse"):
        closest_pool_cat_backward(g, inds, -1, 4)
    with pytest.raises(ValueError, match="inds"):
        closest_pool_cat_backward(g, inds[:29], 10, 4)
    with pytest.raises(ValueError, match="out"):
        closest_pool_cat_backward(g, inds, 10, 4, out=torch.zeros(10, 5))
    with pytest.raises(ValueError, match="transpose"):
        closest_pool_cat_backward(g, inds, 10, 4, transpose=(torch.zeros(10, dtype=torch.int32), torch.zeros(30, dtype=torch.int32)))
    with pytest.raises(TypeError):
        closest_pool_cat_backward(g.double(), inds, 10, 4)
    # well-formed host tensors: there is no CPU path
    with pytest.raises(_lib.D3FeatLibraryError):
        ind_max_pool_backward(**_pool_args())
    with pytest.raises(_lib.D3FeatLibraryError):
        closest_pool_cat_backward(g, inds, 10, 4)
