"""d3feat_amd.validation without a GPU: argument errors, the mean rules and the printed line, and the fixture of the reference
(tests/golden/validation.npz) against the float64 restatement tests/validation_np.py that the GPU tests use as their oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import validation_np as vnp
from conftest import GOLDEN

FIG = ("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg")


def _args(C=32, N=50, ld=16, **over):
    a = dict(features=torch.zeros(N, C), scores=torch.zeros(N), points=torch.zeros(N, 3), anc_idx=torch.zeros(ld, dtype=torch.int32),
             pos_idx=torch.zeros(ld, dtype=torch.int32))
    a.update(over)
    return a


def test_argument_errors():
    from d3feat_amd import _lib
    from d3feat_amd.validation import PairValidation, validation_pairs, validation_records
    with pytest.raises(ValueError, match="16"):
        validation_pairs(**_args(C=8))
    with pytest.raises(ValueError, match="1024"):
        validation_pairs(**_args(ld=1025))
    with pytest.raises(ValueError, match="1024"):
        validation_pairs(**_args(ld=2048), n=1025)
    with pytest.raises(ValueError, match="lists hold 16"):
        validation_pairs(**_args(), n=17)
    with pytest.raises(ValueError):
        validation_pairs(**_args(), n=-1)
    with pytest.raises(ValueError, match="scores"):
        validation_pairs(**_args(scores=torch.zeros(49)))
    with pytest.raises(ValueError, match="points"):
        validation_pairs(**_args(points=torch.zeros(50, 2)))
    with pytest.raises(ValueError, match="index lists"):
        validation_pairs(**_args(pos_idx=torch.zeros(15, dtype=torch.int32)))
    with pytest.raises(TypeError):
        validation_pairs(**_args(features=np.zeros((50, 32), np.float32)))
    with pytest.raises(ValueError, match="loss"):
        PairValidation(1, torch.device("cpu"), loss="triplet")
    # well-formed host tensors: there is no CPU path
    with pytest.raises(_lib.D3FeatLibraryError):
        validation_pairs(**_args())
    with pytest.raises(_lib.D3FeatLibraryError):
        validation_records(torch.zeros(50, 36), [25, 25], torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32))


def test_entry_point_refuses_bad_sizes_before_the_device():
    from d3feat_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(C=32, ldd=32, lds=1, ldp=3, n_rows=10, ld_idx=16, P=1, radius=0.1, kn=16, w=1.0, q=0.1, m=1.4, L=25.0, sums=p, ws=(p, 4096)):
        return lib.d3f_validation_pairs(p, ldd, C, p, lds, p, ldp, n_rows, p, p, p, ld_idx, p, P, radius, kn, w, q, m, L, p, p, sums, p,
                                        ws[0], ws[1], None)
    for bad in (dict(C=8), dict(C=48), dict(ldd=31), dict(lds=0), dict(ldp=2), dict(n_rows=-1), dict(ld_idx=0), dict(P=-1), dict(kn=-1),
                dict(radius=float("nan")), dict(m=0.0), dict(L=0.0), dict(L=41.0), dict(sums=None)):
        assert call(**bad) == -3, bad
    assert call(ws=(p, 64)) == -2 and call(ws=(None, 0)) == -2
    assert lib.d3f_validation_pairs_workspace_bytes(-1, 16) == 0 and lib.d3f_validation_pairs_workspace_bytes(1, 0) == 0
    # 32 bytes per pair and index, the lists rounded up to whole 64-row tiles and capped at D3F_VALIDATION_NMAX
    one = lib.d3f_validation_pairs_workspace_bytes(1, 100)
    assert 128 * 32 <= one <= 128 * 32 + 512
    assert lib.d3f_validation_pairs_workspace_bytes(1, 5000) == lib.d3f_validation_pairs_workspace_bytes(1, 1024)
    assert lib.d3f_validation_pairs_workspace_bytes(500, 256) >= 500 * 256 * 32
    assert _lib.VALIDATION_NMAX == 1024


def test_fixture_of_the_reference_against_float64():
    """What loss.py of the reference computed in float32 for the fixture's pairs is what validation_np computes in float64, within the
    tolerances of validation_np itself; the stored tolerances are 4 x the measured difference; the inputs keep the margins."""
    z = np.load(os.path.join(GOLDEN, "validation.npz"))
    ref = z["reference"].astype(np.float64)
    worst = np.zeros(6)
    kinds = [str(k) for k in z["kinds"]]
    assert {"duplicates", "all_masked", "skipped"} <= set(kinds) and z["features"].shape[1] == 32
    assert os.path.getsize(os.path.join(GOLDEN, "validation.npz")) < 1 << 20
    for p, n in enumerate(z["n"]):
        lo, hi = z["row0"][p], z["row0"][p + 1]
        f, s, x = z["features"][lo:hi], z["scores"][lo:hi], z["points"][lo:hi]
        ai, pi = z["anc_idx"][p, :n], z["pos_idx"][p, :n]
        want = vnp.figures(f, s, x, ai, pi, float(z["safe_radius"]), int(z["keypts_num"][p]), float(z["det_loss_weight"]))
        if kinds[p] == "skipped":
            assert want["skipped"] and ref[p].tolist() == list(vnp.SKIP)
            continue
        planted = [int(r) for r in z["planted_rows"][p] if r >= 0]
        rows = [i for i in range(n) if any(ai[i] == ai[j] and pi[i] == pi[j] for j in planted)]
        vnp.margins(f, x, ai, pi, float(z["safe_radius"]), 32, planted_rows=rows)
        if kinds[p] == "duplicates":
            assert len(rows) == 2 * len(planted) and all(want["fp"][r] == want["cn"][r] for r in rows)
        if kinds[p] == "all_masked":
            assert want["masked"] == 1.0 and np.allclose(want["lse"], np.log(n), rtol=1e-15) and ref[p, 5] == 0
        elif n >= 63:
            assert want["masked"] >= 0.02
        tol = vnp.tolerances(32, want["Dmax"], want["smax"])
        assert int(round(ref[p, 3] * n)) == want["accurate"]
        for k, name in enumerate(FIG):
            if name != "accuracy":
                d = abs(ref[p, k] - want[name])
                assert d <= tol[name], (p, name, ref[p, k], want[name])
                worst[k] = max(worst[k], d)
            assert np.isclose(z["float64"][p, k], want[name] if name != "accuracy" else ref[p, k], rtol=1e-12, atol=0)
    assert np.allclose(z["tolerance"], 4 * worst, rtol=1e-9, atol=0) and (z["tolerance"][[0, 1, 2, 4, 5]] > 0).all()
    assert any(0 < a < 1 for a in ref[:, 3])                           # not every pair is perfectly accurate


def test_mean_rules_and_the_printed_line():
    from d3feat_amd.validation import PairValidation, format_line, split_means
    # per pair (circle, contrastive, det, accuracy, d_pos, d_neg): a skipped pair, a pair with accuracy 0, one with a NaN d_neg, two plain
    rows = np.array([[0, 0, 0, -1, 0, 0], [0.5, 0.7, -0.2, 0.0, 0.9, 1.3], [0.3, 0.2, 0.1, 1.0, 0.2, np.nan], [0.4, 0.6, -0.4, 0.5, 0.3, 1.2],
                     [0.6, 0.8, 0.0, 0.25, 0.4, 1.4]])
    sums, counts = np.zeros(6), np.zeros(6, np.int64)
    for k in range(6):
        sel = rows[:, k] > 0 if k == 3 else rows[:, k] != 0                 # utils/trainer.py:442-452 (NaN != 0 is true)
        sums[k], counts[k] = rows[sel, k].sum(), sel.sum()
    assert counts.tolist() == [4, 4, 3, 3, 4, 4]
    got = split_means(sums, counts)
    want = vnp.split_means(rows[:, [0, 2, 3, 4, 5]])
    assert np.allclose(got, want, rtol=1e-15, atol=0, equal_nan=True) and np.isnan(got[4])
    assert np.isclose(got[0], 0.45) and np.isclose(got[1], -0.5 / 3) and np.isclose(got[2], 1.75 / 3) and np.isclose(got[3], 0.45)
    assert np.isclose(split_means(sums, counts, "desc_loss")[0], 2.3 / 4)
    assert all(np.isnan(v) for v in split_means(np.zeros(6), np.zeros(6, np.int64)))      # np.mean([]) of the trainer
    line = format_line("3DMatch", 7, (0.4567, -0.1234, 0.98765, 0.2, 1.3))
    assert line == "3DMatch Epoch   7: desc_loss = 0.457 det_loss = -0.123 accuracy = 98.77%  d_pos = 0.200 d_neg = 1.300"
    out = PairValidation(5, torch.device("cpu"))
    out.sums.copy_(torch.from_numpy(np.nan_to_num(sums)))
    out.counts.copy_(torch.from_numpy(counts))
    assert out.line("KITTI", 12).startswith("KITTI Epoch  12: desc_loss = 0.450 det_loss = -0.167 accuracy = 58.33%  d_pos = 0.450")
    assert out.means()[:4] == split_means(np.nan_to_num(sums), counts)[:4]


def test_float64_restatement_on_hand_made_pairs():
    """validation_np itself: a three-row pair worked out by hand."""
    e = np.eye(4, 16)
    f = np.concatenate([e[:3], e[:3]]).astype(np.float32)                  # positives identical to their anchors
    x = np.array([[0, 0, 0], [0.05, 0, 0], [1, 0, 0]] * 2, np.float32)
    s = np.full(6, 0.5, np.float32)
    ai, pi = np.arange(3), np.arange(3) + 3
    w = vnp.figures(f, s, x, ai, pi, 0.1, 2)
    assert np.allclose(w["fp"], 1e-6) and np.allclose(w["cn"], np.sqrt(2 + 1e-12)) and w["accuracy"] == 1.0
    # rows 0 and 1 are false negatives of each other: 4 of the 6 off-diagonal distances remain
    assert np.isclose(w["d_neg"], 4 * np.sqrt(2 + 1e-12) / 9 * 3 / 2) and np.isclose(w["masked"], 2 / 6)
    assert np.allclose(w["lse"], np.log(3))                                # sqrt(2) >= 1.4: every z is 0
    assert np.isclose(w["det"], (1e-6 - np.sqrt(2 + 1e-12)) * (1 + 1e-6))
    assert vnp.figures(f, s, x, ai[:1], pi[:1], 0.1, 3)["skipped"] and not vnp.figures(f, s, x, ai[:1], pi[:1], 0.1, 2)["skipped"]
    assert np.isnan(vnp.figures(f, s, x, ai[:1], pi[:1], 0.1, 2)["d_neg"])
    with pytest.raises(AssertionError, match="change the seed"):
        vnp.margins(f, np.array([[0, 0, 0], [0.1, 0, 0], [1, 0, 0]] * 2, np.float32), ai, pi, 0.1, 16)
