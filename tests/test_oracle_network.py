"""Cross-check of the floating-point oracle (oracle/network_np.py, the restatement of the reference's TF graph).

The reference ships no test or golden vector for this part and TensorFlow cannot be installed here:
PARITY UNPINNED by the reference.  What can be done is done here: every op of the restatement is re-derived
independently -- scalar float64 loops written from the formulas in the reference's docstrings/comments
(kernels/convolution_ops.py:161-255, models/D3Feat.py:65-115), not from the vectorised restatement -- on small cases,
and the full forward is checked for the structural properties the reference's graph guarantees."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
import os


def _kpconv_loops(q, s, idx, f, KP, W, extent, influence="linear", mode="sum"):
    n, K = idx.shape
    P, Cin, Cout = W.shape
    out = np.zeros((n, Cout))
    for i in range(n):
        wf = np.zeros((P, Cin))
        cnt = 0
        for k in range(K):
            j = idx[i, k]
            if j >= len(s):                       # shadow neighbour: point at 1e6, zero features
                continue
            rel = s[j].astype(np.float64) - q[i]
            d2 = ((rel[None, :] - KP.astype(np.float64)) ** 2).sum(1)
            if influence == "linear":
                h = np.maximum(1.0 - np.sqrt(d2 + 1e-10) / (2.0 * extent), 0.0)
            elif influence == "constant":
                h = np.ones(P)
            else:
                sig = extent * 0.3
                h = np.exp(-d2 / (2 * sig ** 2 + 1e-9))
            if mode == "closest":
                m = np.zeros(P)
                m[np.argmin(d2)] = 1.0
                h = h * m
            wf += h[:, None] * f[j][None, :]
            cnt += 1 if f[j].astype(np.float64).sum() > 0 else 0
        out[i] = np.einsum("pc,pco->o", wf, W.astype(np.float64)) / max(cnt, 1)
    return out


@pytest.mark.parametrize("influence,mode", [("linear", "sum"), ("constant", "sum"), ("gaussian", "sum"), ("linear", "closest")])
def test_kpconv_ops_restatement_vs_scalar_loops(coracle, influence, mode):
    from oracle import network_np as onp
    rng = np.random.default_rng(0)
    s = np.load(os.path.join(GOLDEN, "demo_bin0_sub003.npy"))[:1500]
    lens = np.asarray([len(s)], np.int32)
    nb = coracle.batch_neighbors(s[:60], s, np.asarray([60], np.int32), lens, np.float32(0.075))[:, :30]
    f = rng.standard_normal((len(s), 6)).astype(np.float32)
    W = rng.standard_normal((15, 6, 5)).astype(np.float32)
    KP = np.load(os.path.join(GOLDEN, "kitti_kernel_points.npz"))["layer_0__simple_0__kernel_points"] * np.float32(0.1)
    want = _kpconv_loops(s[:60], s, nb, f, KP, W, 0.03, influence, mode)
    got = onp.KPConv_ops(s[:60], s, nb, f, KP, W, 0.03, influence, mode).numpy()
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


def test_detection_head_restatement_vs_scalar_loops(coracle):
    from oracle import network_np as onp
    rng = np.random.default_rng(1)
    s = np.load(os.path.join(GOLDEN, "demo_bin0_sub003.npy"))[:400]
    L = np.asarray([250, 150], np.int32)
    nb = coracle.batch_neighbors(s, s, L, L, np.float32(0.09))[:, :12]
    x = rng.standard_normal((400, 8)).astype(np.float32)
    in_b = onp.stack_batch_inds(L)
    got = onp.detection_head(torch.from_numpy(x), nb, in_b, L).numpy()[:, 0]
    xd = x.astype(np.float64)
    m = [max(xd[:250].max(), 0.0 if 400 in in_b[0] else -np.inf), max(xd[250:].max(), 0.0 if 400 in in_b[1] else -np.inf)]
    y = np.concatenate([xd[:250] / (m[0] + 1e-6), xd[250:] / (m[1] + 1e-6)])
    want = np.zeros(400)
    for i in range(400):
        rows = [y[j] for j in nb[i] if j < 400]
        cnt = max(sum(1 for r in rows if np.float32(r.astype(np.float32).sum()) != 0), 1)
        mean = (np.sum(rows, 0) if rows else np.zeros(8)) / cnt
        alpha = np.log1p(np.exp(y[i] - mean))
        beta = y[i] / (1e-6 + y[i].max())
        want[i] = (alpha * beta).max()
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


# two-cloud stacks for the float64 head reference: (C, K, lens, all-negative clouds, include-zero vector or None = length rule)
HEAD_F64_CASES = [(32, 33, (60, 60), (), None), (32, 35, (70, 45), (), None), (20, 7, (45, 70), (), None),
                  (64, 40, (50, 50), (), None), (128, 33, (40, 64), (), None), (1, 16, (30, 50), (), None),
                  (32, 30, (60, 60), (0, 1), None), (32, 30, (70, 45), (1,), None), (32, 30, (70, 45), (0,), None),
                  (33, 17, (70, 45), (0,), (1, 0)), (32, 0, (20, 30), (), None)]
HEAD_F64_MEASURED = 2.79e-7     # largest difference over the cases above on the CPU (scores 7.6e-8 .. 2.8e-7 per case; the descriptors differ by less)
HEAD_F64_BOUND = 2 * HEAD_F64_MEASURED


def test_detection_head_f64_generalisation_vs_oracle():
    """onp.detection_head_f64 (B clouds, stack groups, explicit include-zero: the reference of tests/test_gpu_pool_head.py) restates
    the same lines as onp.detection_head, which is pinned to the reference's Python: on two-cloud stacks (equal / unequal lengths,
    all-negative clouds whose padded maximum is the zero row, shadow slots, all-zero and cancelling rows, K = 0) they differ by the
    float32 rounding of the oracle only.  The bound is twice the largest difference measured here on these inputs, relative to
    max(1, |want|) (a padded all-negative cloud has scores of order 1e7); it stays far below the 1e-5 descriptor bar."""
    from oracle import head_cases as hc
    from oracle import network_np as onp
    worst = 0.0
    for i, (C, K, lens, neg, inc) in enumerate(HEAD_F64_CASES):
        x, nb = hc.head_case(100 + i, C, K, lens, negative=neg)
        assert hc.neighbours_stay_in_cloud(nb, lens)
        n = sum(lens)
        inc_v = onp.include_zero_rule(lens) if inc is None else list(inc)
        in_b = onp.stack_batch_inds(lens) if inc is None else hc.in_batches(lens, inc_v)
        nb_t = np.where((nb < 0) | (nb >= n), n, nb)
        got = onp.detection_head(torch.from_numpy(x), nb_t, in_b, np.asarray(lens)).numpy()[:, 0].astype(np.float64)
        desc, want, _ = onp.detection_head_f64(x, nb, lens, 0, inc)
        assert [int(n in set(in_b[b].tolist())) for b in range(2)] == inc_v
        rel = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print("head f64 vs oracle: C %d K %d lens %s neg %s inc %s: %.3e (|want| max %.3g)" % (C, K, lens, neg, inc, rel, np.abs(want).max()))
        worst = max(worst, rel)
        sq = (torch.from_numpy(x) ** 2).sum(1, keepdim=True)
        d32 = (torch.from_numpy(x) * torch.rsqrt(torch.clamp(sq, min=1e-10))).numpy()     # onp.forward's descriptor line
        worst = max(worst, np.abs(d32 - desc).max())
    print("largest: %.3e" % worst)
    assert worst <= HEAD_F64_BOUND < 1e-5


def test_pools_restatement():
    from oracle import network_np as onp
    x = torch.tensor([[1., -5.], [3., 2.], [-2., 7.]])
    inds = np.asarray([[0, 1, 3], [3, 3, 3], [2, 3, 3]])
    # shadow row (index 3) = per-column minimum (-2, -5): max-pool ignores it unless the row is all-shadow
    assert torch.equal(onp.ind_max_pool(x, inds), torch.tensor([[3., 2.], [-2., -5.], [-2., 7.]]))
    assert torch.equal(onp.closest_pool(x, inds), torch.tensor([[1., -5.], [0., 0.], [-2., 7.]]))


def test_forward_structure_on_reference_geometry(coracle):
    """Full forward of the restatement on a crop of the demo cloud: shapes, unit-norm descriptors, finite positive
    scores, and the self-pair mirror (both halves of a stacked self-pair give identical rows)."""
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import threedmatch_config
    from oracle import network_np as onp
    cfg = threedmatch_config()
    sub = np.load(os.path.join(GOLDEN, "demo_bin0_sub003.npy"))
    c = sub[np.linalg.norm(sub - np.median(sub, axis=0), axis=1) < 0.9]
    assert 500 < len(c) < 5000
    pts = np.concatenate([c, c])
    lens = np.asarray([len(c)] * 2, np.int32)
    inp = onp.descriptor_input(cfg, pts, np.ones((len(pts), 1), np.float32), lens, [37, 35, 36, 38, 38],
                               lambda q, s, ql, sl, r: coracle.batch_neighbors(q, s, ql, sl, r),
                               lambda p, l, dl: coracle.batch_grid_subsampling(p, l, dl))
    W = build_variables(cfg, seed=42, randomize_bn=True).values
    trace = {}
    d, s = onp.forward(cfg, W, inp, trace)
    assert d.shape == (2 * len(c), 32) and s.shape == (2 * len(c), 1)
    assert np.isfinite(d).all() and np.isfinite(s).all()
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-5
    assert (s >= 0).all()
    assert np.abs(d[: len(c)] - d[len(c):]).max() < 1e-6 and np.abs(s[: len(c)] - s[len(c):]).max() < 1e-6
    assert trace["layer_0/simple_0"].shape[1] == 64 and trace["layer_4/resnetb_0"].shape[1] == 2048
    assert trace["uplayer_0/last_unary_1"].shape[1] == 32


def test_kpconv_case_generator_conditions_hold_for_every_shape():
    """oracle/kpconv_cases.py states two conditions on its inputs (row sums decided in any precision; no near-tie of the 'closest'
    arg-min) and meets them by nudging / re-drawing, never by leaving a case out: every shape of tests/test_gpu_kpconv_branches.py
    is generated here by the GPU tests' own helper (with 15 kernel points; the generator asserts both conditions itself on the
    other variants) and both are asserted on it; the stated index patterns are present."""
    from oracle import kpconv_cases as kc
    shapes = kc.all_shapes()
    assert len(shapes) >= 90
    kinds = set()
    for kernel, Cin, Nq, K in shapes:
        for bf16 in ((False, True) if kc.has_bf16(kernel, Cin) or kernel == "errors" else (False,)):
            c = kc.shape_case(kernel, Cin, Nq, K, bf16=bf16)
            f = c.f[:c.Ns]
            assert kc.row_sums_decided(f) and kc.closest_decided(c)
            assert np.isnan(c.f[c.Ns:]).all() and np.isnan(c.q[c.Nq:]).all()
            if bf16:
                assert np.array_equal(f, kc.bf16_values(f))
            sums = f.astype(np.float64).sum(1)
            assert (sums < 0).any() and (sums > 0).any() and (np.abs(f).sum(1) == 0).any()
            if Cin >= 2:
                assert ((sums == 0) & (np.abs(f).sum(1) > 0)).any()
            idx = c.idx[:Nq]
            valid = (idx >= 0) & (idx < c.Ns)
            if Nq >= 4 and K >= 1:
                assert (~valid.any(1)).sum() >= 2
            if Nq * K >= 300:
                assert (idx == c.Ns).any() and (idx > c.Ns).any() and (idx < 0).any() and valid.any()
                assert any(len(set(r[v])) < v.sum() for r, v in zip(idx, valid))          # duplicates within a row
                kinds.add(kernel)
    assert kinds == {"agg_vec4", "fused32", "fused", "c1_sum", "c1_closest", "agg_scalar", "errors"}
    x, want = kc.rowpos_case(1, 77, 20)
    assert 0 < want.sum() < 77 and want[2] == 1 and want[3] == 0 and want[5] == 1 and want[4] == 0 and want[1] == 0


KPCONV_F64_SHAPES = [("agg_vec4", 4, 255, 2), ("agg_vec4", 16, 63, 5), ("agg_scalar", 6, 37, 9), ("fused32", 32, 31, 8),
                     ("fused", 64, 53, 17), ("c1_sum", 1, 15, 65), ("c1_closest", 1, 31, 37), ("agg_vec4", 8, 127, 0)]


@pytest.mark.parametrize("influence,mode", [("constant", "sum"), ("linear", "sum"), ("gaussian", "sum"),
                                            ("constant", "closest"), ("linear", "closest"), ("gaussian", "closest")])
def test_kpconv_f64_vs_restatement_and_scalar_loops(influence, mode):
    """onp.kpconv_f64 (the reference of tests/test_gpu_kpconv_branches.py: float64, shadow = any index outside [0, Ns), epilogue)
    against the float32 restatement of the reference's graph (onp.KPConv_ops, at its float32 rounding) and against the float64
    scalar loops above (at float64 rounding), in all six modes, at the generator's shapes -- capacity rows and every shadow pattern
    included, which the two older forms only take as the index Ns."""
    from oracle import kpconv_cases as kc
    from oracle import network_np as onp
    assert (influence, mode) in kc.MODES and len(kc.MODES) == 6
    shapes = set(kc.all_shapes())
    for kernel, Cin, Nq, K in KPCONV_F64_SHAPES:
        assert (kernel, Cin, Nq, K) in shapes
        num_kp = 15 if Cin != 8 else 4
        c = kc.kpconv_case(kc.shape_seed(kernel, Cin, Nq, K), Cin, K, Nq, num_kp=num_kp, cap_q=2, cap_s=4)
        W = kc.weights(kc.shape_seed(kernel, Cin, Nq, K), num_kp, Cin, 5)
        wf, count, out = onp.kpconv_f64(c.q, c.s, c.idx, c.f, c.KP, W, kc.EXTENT, influence, mode, Nq=c.Nq, Ns=c.Ns)
        assert wf.shape == (Nq, num_kp, Cin) and count.shape == (Nq,) and out.shape == (Nq, 5)
        q, s, f = c.q[:c.Nq], c.s[:c.Ns], c.f[:c.Ns]
        idx = np.where((c.idx[:c.Nq] < 0) | (c.idx[:c.Nq] >= c.Ns), c.Ns, c.idx[:c.Nq])
        loops = _kpconv_loops(q, s, idx, f, c.KP, W, kc.EXTENT, influence, mode)
        scale = max(1.0, np.abs(loops).max())
        assert np.abs(out - loops).max() <= 1e-12 * scale
        o32 = onp.KPConv_ops(q, s, idx, f, c.KP, W, kc.EXTENT, influence, mode).numpy()
        assert np.abs(o32 - out).max() <= 2e-5 * scale
        # the epilogue, restated: act(out * scale + shift + residual)
        rng = np.random.default_rng(K)
        cs, ch, res = rng.random(5) + 0.5, rng.standard_normal(5), rng.standard_normal((Nq + 2, 5))
        _, _, oe = onp.kpconv_f64(c.q, c.s, c.idx, c.f, c.KP, W, kc.EXTENT, influence, mode, Nq=c.Nq, Ns=c.Ns, col_scale=cs,
                                  col_shift=ch, residual=res, leaky=True, alpha=0.125)
        v = out * cs + ch + res[:Nq]
        assert np.array_equal(oe, np.where(v > 0, v, 0.125 * v))
        # the count differs from the number of valid slots (zero / negative rows are present, not counted)
        if Nq * K >= 300:
            assert (count < ((c.idx[:Nq] >= 0) & (c.idx[:Nq] < c.Ns)).sum(1)).any()
