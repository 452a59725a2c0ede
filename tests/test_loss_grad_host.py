"""d3feat_amd.validation.loss_gradients without a GPU.  The reference cannot emit gradients here (TensorFlow is not installed, the
stand-in oracle/tf_eager has none), so what is pinned is the DEFINITION (include/d3feat_amd.h, tests/loss_grad_np.py), three ways:
against float64 torch autograd of a line-by-line torch restatement of utils/loss.py, against difference quotients of the forward that
tests/golden/validation.npz ties to the reference's own loss.py, and the argument errors that come before the device is asked."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_grad_np as lg
import validation_np as vnp
from conftest import GOLDEN

LOSSES = ("circle_loss", "desc_loss")


def _with_duplicates(case):
    """The lists as the loader draws them (replace=True): the same (ai, pi) three times, a positive named by three entries (exact ties
    in cn), a row named by both lists."""
    f, s, x, ai, pi = case
    ai, pi = ai.copy(), pi.copy()
    ai[5], pi[5] = ai[3], pi[3]
    ai[7], pi[7] = ai[3], pi[3]
    pi[11] = pi[13] = pi[12]
    ai[20] = pi[21]
    return f, s, x, ai, pi


@pytest.mark.parametrize("loss", LOSSES)
def test_restatement_against_torch_float64_autograd(loss):
    """loss_grad_np.gradients against autograd of loss_grad_np.torch_loss in float64: 1e-12 of the pair's largest entry, at n = 1, 2,
    around a tile edge, with duplicated entries (amin's gradient is the equal split among ties, as reduce_min's), a skipped pair,
    every negative masked, and det_loss_weight 0, 1 and 0.5."""
    cases = [(lg.clean_case(100 + n, n, C, 0.1, noise=1.0)[0], 0.1, 2) for n, C in ((1, 16), (2, 16), (40, 32), (65, 64))]
    cases.append((_with_duplicates(lg.clean_case(140, 40, 32, 0.1, noise=1.0)[0]), 0.1, 2))
    cases.append((_with_duplicates(lg.clean_case(165, 65, 16, 0.1, noise=1.6)[0]), 0.1, 2))
    cases.append((lg.clean_case(7, 30, 32, 0.1, cube=0.05, noise=1.6)[0], 0.1, 2))                # all inside the safe radius
    cases.append((lg.clean_case(8, 30, 32, 0.1)[0], 0.1, 64))                                     # 30 < 0.5 * 64: skipped
    ties = 0
    for (f, s, x, ai, pi), r, kn in cases:
        for w in (0.0, 1.0, 0.5):
            got = lg.gradients(f, s, x, ai, pi, r, kn, w, loss=loss)
            gf, gs = lg.torch_gradients(f, s, x, ai, pi, r, kn, w, loss=loss)
            if got["skipped"]:
                assert not gf.any() and not gs.any() and not got["features"].any() and not got["scores"].any()
                continue
            ties = max(ties, int(got["ties"].max()))
            for have, want in ((got["features"], gf), (got["scores"], gs)):
                big = np.abs(want).max()
                print("n=%d C=%d w=%.1f %s: largest %.3e, difference %.2e" % (len(ai), f.shape[1], w, loss, big, np.abs(have - want).max()))
                assert np.abs(have - want).max() <= 1e-12 * big
            assert (w == 0) == (not got["scores"].any())
    assert ties == 3                                                                              # the equal split was exercised


def test_restatement_against_difference_quotients_of_the_pinned_forward():
    """Central differences of validation_np.figures -- the forward that tests/golden/validation.npz ties to the reference's loss.py --
    on a few rows of a small pair.  The contrastive and the detection loss are differentiated as they are.  The circle loss is not
    the derivative of its own value: max(0, m - D) is under stop_gradient, so z = L (m - D)^2 is differentiated as L (m - D) * const;
    the quotient of the forward sees twice that, which gradients(stop_gradient=False) restates -- the two differ in that factor only,
    and the factor itself is pinned by the autograd test above.
    Tolerance, from the step h = 1e-6 (the perturbed values are exact in float64; F is of magnitude 1):
      rounding    the value carries about 64 * 2^-52 |F| (sums of n^2 terms, exp, log) and is divided by 2 h: 64 * 2^-52 / h;
      truncation  h^2 / 6 * |F'''|, and along one coordinate |F'''| <= 2 (2 L m)^3 / L: the third derivative of log-sum-exp is
                  bounded by |z'|^3 with |z'| <= 2 L m, softplus / L divides by L, the factor 2 covers the curvature of D itself
                  (|D''| <= 1 / D, the pair keeps D >= 0.2), and the mean over n rows outweighs the n rows a positive row enters."""
    n, C, h = 12, 16, 1e-6
    (f, s, x, ai, pi), DKD, _ = lg.clean_case(31, n, C, 0.25, noise=1.0)
    f, s = f.astype(np.float64), s.astype(np.float64)
    assert DKD[0].min() >= 0.2
    L, m = vnp.LOG_SCALE, vnp.NEG_MARGIN
    tol = 64 * 2.0 ** -52 / h + h * h / 6 * 2 * (2 * L * m) ** 3 / L
    assert tol < 5e-8

    def value(ff, ss, loss, w):
        v = vnp.figures(ff, ss, x, ai, pi, 0.25, 2, w)
        return v["circle" if loss == "circle_loss" else "contrastive"] + v["det"]
    rows = [int(ai[0]), int(ai[5]), int(pi[0]), int(pi[7]), len(f) - 1]                            # anchors, positives, a row nobody names
    named = set(ai.tolist()) | set(pi.tolist())
    assert rows[-1] not in named
    for loss in LOSSES:
        for w in (0.0, 1.0):
            got = lg.gradients(f, s, x, ai, pi, 0.25, 2, w, loss=loss, stop_gradient=False)
            worst = 0.0
            for r in rows:
                for c in range(C):
                    fp_, fm_ = f.copy(), f.copy()
                    fp_[r, c] += h
                    fm_[r, c] -= h
                    q = (value(fp_, s, loss, w) - value(fm_, s, loss, w)) / (fp_[r, c] - fm_[r, c])
                    worst = max(worst, abs(q - got["features"][r, c]))
                sp_, sm_ = s.copy(), s.copy()
                sp_[r] += h
                sm_[r] -= h
                q = (value(f, sp_, loss, w) - value(f, sm_, loss, w)) / (sp_[r] - sm_[r])
                worst = max(worst, abs(q - got["scores"][r]))
            print("%s w=%.0f: largest |quotient - gradient| %.2e (tolerance %.2e, largest entry %.2e)" % (
                loss, w, worst, tol, np.abs(got["features"]).max()))
            assert worst <= tol
            assert not got["features"][rows[-1]].any() and got["scores"][rows[-1]] == 0
    # the stop_gradient factor: exactly the live part of the circle term, once against twice
    a = lg.gradients(f, s, x, ai, pi, 0.25, 2, 0.0)
    b = lg.gradients(f, s, x, ai, pi, 0.25, 2, 0.0, stop_gradient=False)
    off = ~np.eye(n, dtype=bool)
    assert a["live"].any() and np.allclose(b["G"][off], 2 * a["G"][off], rtol=1e-15, atol=0) and np.array_equal(np.diag(a["G"]), np.diag(b["G"]))


def test_fixture_against_the_restatement():
    """tests/golden/loss_grad.npz (tools/make_golden_loss_grad.py): the stored float64 gradients are what loss_grad_np gives today, the
    seeds are the ones clean_case finds, the margins hold, and the recorded float32 deviations are of the size the issue measured
    (some 1e-7 of the largest entry)."""
    z = np.load(os.path.join(GOLDEN, "loss_grad.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "loss_grad.npz")) < 1 << 20
    keys = [tuple(int(v) for v in k) for k in z["keys"]]
    assert len(keys) == 3 * 7 * 2 * 2 and len(set(keys)) == len(keys)
    r, kn = float(z["safe_radius"]), int(z["keypts_num"])
    checked = 0
    for at, (C, n, li, w) in enumerate(keys):
        tag = "C%d_n%d_%s_w%d" % (C, n, LOSSES[li], w)
        assert (z["err32"][at] <= 1e-6 * np.maximum(z["largest"][at], 1e-30)).all(), tag
        assert (z["margins"][at] > 0).all(), tag
        if "features_" + tag not in z.files:
            continue
        case, DKD, mg = lg.clean_case(100 * C + n, n, C, r, cube=0.4, noise=1.6)
        assert np.allclose([mg[k] for k in z["margin_names"]], z["margins"][at], rtol=1e-12, atol=0)
        f, s, x, ai, pi = case
        assert np.array_equal(vnp.make_case(int(z["seeds"][at]), n, C, cube=0.4, noise=1.6)[0], f)
        got = lg.gradients(f, s, x, ai, pi, r, kn, float(w), loss=LOSSES[li], DKD=DKD)
        for name in ("features", "scores"):
            want = z[name + "_" + tag]
            assert np.abs(got[name] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), tag
        assert np.isclose(np.abs(got["features"]).max(), z["largest"][at][0], rtol=1e-12)
        checked += 1
    assert checked == 12


def _args(C=32, N=50, ld=16, **over):
    a = dict(features=torch.zeros(N, C), scores=torch.zeros(N), points=torch.zeros(N, 3), anc_idx=torch.zeros(ld, dtype=torch.int32),
             pos_idx=torch.zeros(ld, dtype=torch.int32))
    a.update(over)
    return a


def test_argument_errors():
    """The checks of validation_pairs, made before the device is asked for."""
    from d3feat_amd import _lib
    from d3feat_amd.validation import PairGradients, loss_gradients, loss_gradients_records
    with pytest.raises(ValueError, match="16"):
        loss_gradients(**_args(C=8))
    with pytest.raises(ValueError, match="1024"):
        loss_gradients(**_args(ld=1025))
    with pytest.raises(ValueError, match="1024"):
        loss_gradients(**_args(ld=2048), n=1025)
    with pytest.raises(ValueError, match="lists hold 16"):
        loss_gradients(**_args(), n=17)
    with pytest.raises(ValueError):
        loss_gradients(**_args(), n=-1)
    with pytest.raises(ValueError, match="scores"):
        loss_gradients(**_args(scores=torch.zeros(49)))
    with pytest.raises(ValueError, match="points"):
        loss_gradients(**_args(points=torch.zeros(50, 2)))
    with pytest.raises(ValueError, match="index lists"):
        loss_gradients(**_args(pos_idx=torch.zeros(15, dtype=torch.int32)))
    with pytest.raises(TypeError):
        loss_gradients(**_args(features=np.zeros((50, 32), np.float32)))
    with pytest.raises(ValueError, match="loss"):
        loss_gradients(**_args(), loss="triplet")
    with pytest.raises(ValueError, match="loss"):
        PairGradients(1, 50, 32, torch.device("cpu"), loss="triplet")
    with pytest.raises(ValueError, match="features"):
        PairGradients(1, 50, 32, torch.device("cpu"), features=torch.zeros(50, 16))
    # well-formed host tensors: there is no CPU path
    with pytest.raises(_lib.D3FeatLibraryError):
        loss_gradients(**_args())
    with pytest.raises(_lib.D3FeatLibraryError):
        loss_gradients_records(torch.zeros(50, 36), [25, 25], torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32))
    out = PairGradients(2, 50, 32, torch.device("cpu"))
    assert out.features.shape == (50, 32) and out.scores.shape == (50,) and out.values.shape == (2, 8) and out.status.shape == (2,)
    assert len(out.figures(1)) == 5


def test_entry_point_refuses_bad_sizes_before_the_device():
    from d3feat_amd import _lib
    lib = _lib.load()
    assert "d3f_loss_gradients" in _lib.SIGNATURES and "d3f_loss_gradients_workspace_bytes" in _lib.SIGNATURES
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def call(C=32, ldd=32, lds=1, ldp=3, n_rows=10, ld_idx=16, P=1, radius=0.1, kn=16, w=1.0, q=0.1, m=1.4, L=25.0, kind=0, ldg=32, ldgs=1,
             gd=p, ws=(p, 1 << 16)):
        return lib.d3f_loss_gradients(p, ldd, C, p, lds, p, ldp, n_rows, p, p, p, ld_idx, p, P, radius, kn, w, q, m, L, kind, gd, ldg, p, ldgs,
                                      p, p, ws[0], ws[1], None)
    for bad in (dict(C=8), dict(C=48), dict(ldd=31), dict(lds=0), dict(ldp=2), dict(n_rows=-1), dict(ld_idx=0), dict(P=-1), dict(kn=-1),
                dict(radius=float("nan")), dict(m=0.0), dict(L=0.0), dict(L=41.0), dict(kind=2), dict(kind=-1), dict(ldg=31), dict(ldgs=0),
                dict(gd=None)):
        assert call(**bad) == -3, bad
    assert call(ws=(p, 64)) == -2 and call(ws=(None, 0)) == -2
    size = lib.d3f_loss_gradients_workspace_bytes
    assert size(-1, 16, 32) == 0 and size(1, 0, 32) == 0 and size(1, 16, 48) == 0
    # (52 + 8 C) bytes per pair and index, the lists rounded up to whole 64-entry tiles and capped at D3F_VALIDATION_NMAX
    for C in (16, 32, 64):
        assert 128 * (52 + 8 * C) <= size(1, 100, C) <= 128 * (52 + 8 * C) + 6 * 256
        assert size(1, 5000, C) == size(1, 1024, C)
        assert size(500, 256, C) >= 500 * 256 * (52 + 8 * C)
