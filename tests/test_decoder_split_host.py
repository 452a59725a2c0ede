"""Host side of the decoder's split form (no GPU): the derived weights of VariableStore.split_decoder, the predicate that chooses
between the split and the one-launch form, and the inputs / float64 reference that tests/test_gpu_decoder_split.py measures against."""
import numpy as np
import pytest
import torch

import test_gpu_decoder_split as gs


def _store(C1, C2, N, seed=1):
    from d3feat_amd.models.variables import VariableStore
    vs = VariableStore(seed=seed, device=torch.device("cpu"))
    with vs.variable_scope('uplayer_2/unary_0'):
        w = vs.weight_variable([C1 + C2, N])
        bn = vs.batch_norm_variables(N)
    rng = np.random.default_rng(seed)
    vs.values[bn[0]] = (1.0 + 0.2 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[1]] = (0.1 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[2]] = (0.1 * rng.standard_normal(N)).astype(np.float32)
    vs.values[bn[3]] = (0.5 + rng.random(N)).astype(np.float32)
    return vs, w, bn


def _want(vs, w, bn, C1, eps=1e-6):
    g, b, m, v = (vs.values[n] for n in bn)
    s = (g / np.sqrt(v + np.float32(eps))).astype(np.float32)
    Ws = (vs.values[w] * s[None, :]).astype(np.float32)
    return Ws[:C1], Ws[C1:], (b - m * s).astype(np.float32)


def test_split_decoder_recipe():
    C1, C2, N = 64, 32, 48
    vs, w, bn = _store(C1, C2, N)
    got = vs.split_decoder(w, bn, C1)
    assert [tuple(t.shape) for t in got] == [(C1, N), (C2, N), (N,)] and all(t.is_contiguous() for t in got)
    for t, a in zip(got, _want(vs, w, bn, C1)):
        assert np.array_equal(t.numpy().view(np.uint32), a.view(np.uint32))
    assert vs.split_decoder(w, bn, C1) is got                        # made once
    # update_in_place rewrites the same tensors from the new host values (a weight, then a batch-norm vector)
    ptrs = [t.data_ptr() for t in got]
    touched = vs.update_in_place({w: vs.values[w] * np.float32(1.5)})
    assert all(any(t is d for d in touched) for t in got)
    touched = vs.update_in_place({bn[0]: vs.values[bn[0]] + np.float32(0.25), bn[2]: vs.values[bn[2]] - np.float32(0.5)})
    assert [t.data_ptr() for t in got] == ptrs
    for t, a in zip(got, _want(vs, w, bn, C1)):
        assert np.array_equal(t.numpy().view(np.uint32), a.view(np.uint32))
    # without batch norm: the plain halves, views of the weight's own device copy
    w1, w2, t = vs.split_decoder(w, None, C1)
    assert t is None and w1._base is vs.tensor(w) and w2._base is vs.tensor(w) and w1.is_contiguous() and w2.is_contiguous()
    assert np.array_equal(w1.numpy(), vs.values[w][:C1]) and np.array_equal(w2.numpy(), vs.values[w][C1:])


def test_predicate(monkeypatch):
    from d3feat_amd import ops
    assert ops.DECODER_SPLIT
    # the decoder of the default run: levels 3 .. 1 split, level 0 (the resident-W form) as it is
    assert ops._split_ok(10860, 2048, 1024, 512) and ops._split_ok(43590, 512, 512, 256) and ops._split_ok(174966, 256, 256, 128)
    assert bool(ops._x3_resident(704868, 64, 256, 0)) and not ops._split_ok(704868, 128, 128, 64)
    assert not ops._split_ok(300000, 128, 128, 64, 171000) and ops._split_ok(300000, 128, 128, 64, 60000)   # by the EXPECTED rows
    assert not ops._split_ok(2500, 128, 0, 64)                       # no skip operand
    assert not ops._split_ok(2500, 16, 48, 64) and not ops._split_ok(2500, 64, 48, 64)      # parts that are no whole k-tiles
    assert not ops._split_ok(2500, 128, 64, 64, f32=False)           # bf16 feature tensors
    assert not ops._split_ok(2500, 128, 64, 64, f32t_ok=False)       # operands d3f_gemm_x3 cannot address
    assert not ops._split_ok(2500, 64, 64, 32)                       # 32 columns below the resident form: the fp32 MFMA kernel
    assert not ops._split_ok(ops.X3_MAX_ROWS + 1, 1024, 512, 512)
    with ops.bf16_contraction():
        assert not ops._split_ok(10860, 2048, 1024, 512)
    assert ops._split_ok(10860, 2048, 1024, 512)
    monkeypatch.setattr(ops, "GEMM_X3", False)
    assert not ops._split_ok(10860, 2048, 1024, 512)
    monkeypatch.setattr(ops, "GEMM_X3", True)
    monkeypatch.setattr(ops, "DECODER_SPLIT", False)
    assert not ops._split_ok(10860, 2048, 1024, 512)


def test_predicate_on_tensors():
    """upsample_split_ok looks at the operands of an UpsampleCat: dtype, the skip, alignment (host tensors: nothing is launched)."""
    from d3feat_amd import ops
    x, skip, idx = torch.zeros((50, 64)), torch.zeros((200, 32)), torch.zeros((200, 3), dtype=torch.int32)
    assert ops.upsample_split_ok(ops.UpsampleCat(x, idx, skip), 64)
    assert not ops.upsample_split_ok(ops.UpsampleCat(x, idx, None), 64)
    assert not ops.upsample_split_ok(ops.UpsampleCat(x.to(torch.bfloat16), idx, skip.to(torch.bfloat16)), 64)
    assert not ops.upsample_split_ok(ops.UpsampleCat(torch.zeros((50, 16)), idx, torch.zeros((200, 48))), 64)
    assert not ops.upsample_split_ok(ops.UpsampleCat(x, idx, torch.zeros((200, 34))[:, 2:]), 64)      # skip rows not 16-byte aligned


def test_inputs_and_reference_of_the_gpu_tests():
    C1, C2, N, m = 64, 32, 48, 1000
    x, skip, idx, W, s, t = gs.make_case(C1, C2, N, m)
    n1 = gs.N1
    assert idx.shape == (m, 3) and idx.dtype == np.int32 and x.shape == (n1, C1)
    i0 = idx[:, 0]
    assert (i0[::17] == n1).all() and (i0 < 0).sum() >= 20 and (i0 > n1).sum() >= 20
    assert ((i0 >= 0) & (i0 < n1)).sum() > m // 2 and i0[(i0 >= 0) & (i0 <= n1)].max() == n1 and i0[i0 >= 0].min() < 10
    ref, live = gs.reference(x, skip, idx, W, s, t)
    assert np.array_equal(live, (i0 >= 0) & (i0 < n1))
    # the same thing the slow way: closest_pool's zero row, row by row
    xz = np.concatenate([x, np.zeros((1, C1), np.float32)]).astype(np.float64)
    for r in (0, 5, 7, 17, 34, 123, m - 1):
        row = np.concatenate([xz[i0[r] if 0 <= i0[r] < n1 else n1], skip[r].astype(np.float64)])
        want = row @ W.astype(np.float64) * s + t
        want = np.where(want > 0, want, 0.2 * want)
        assert np.allclose(ref[r], want, rtol=0, atol=1e-12)
    # the rewrite itself, in float64 on the fp32-folded halves: the folding costs a rounding per weight, far inside the bound
    w1, w2 = gs.halves(W, s, C1)
    Y = np.concatenate([x.astype(np.float64) @ w1.astype(np.float64), np.zeros((1, N))])
    alt = skip.astype(np.float64) @ w2.astype(np.float64) + t + Y[np.where(live, i0, n1)]
    alt = np.where(alt > 0, alt, 0.2 * alt)
    assert np.abs(alt - ref).max() <= 5e-7 * max(1.0, np.abs(ref).max())
    # a coarse row count below the capacity: indices at or above it gather zeros
    ref2, live2 = gs.reference(x, skip, idx, W, s, t, n1=600)
    assert np.array_equal(live2, (i0 >= 0) & (i0 < 600)) and np.array_equal(ref2[live2], ref[live2]) and not np.array_equal(ref2, ref)
