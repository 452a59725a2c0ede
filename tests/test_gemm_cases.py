"""Every statement of every case of oracle/gemm_cases.py, checked from the oracle alone (no GPU, no kernel): the exactness budget
(max(|A| @ |W|) < 2^24, every intermediate of the epilogue equal to its own float32 rounding), the placement of signs, exact zeros
and bfloat16 ties, the shadow indices, what poisoned() poisons, and that the branch a case records (written down from the shape
tables) is what the restated host plans give.  Where libd3feat_amd.so is built, the restated plans are compared with the library's own
(d3f_gemm_x3_plan, d3f_gemm_x3_resident, the S implied by the three *_workspace_bytes functions) over a grid of (M, N, K, hint) that
includes every case.  The host-side refusals of the six entry points are tests/test_cabi.py::test_gemm_entry_points_refuse_*."""
import ctypes
import os

import numpy as np
import pytest

from oracle import gemm_cases as gc


def _check_case(s):
    c = gc.build(s)
    M, N, K = s["M"], s["N"], c["K"]
    it = s["intent"]
    assert (it["kernel"], it["S"], it["tiles"]) == gc.planned_branch(s), gc.case_id(s)
    assert sum(it["tiles"]) == gc.cdiv(K, 32) and len(it["tiles"]) == it["S"]
    assert c["want"].shape == (M, N) and c["exact"], gc.case_id(s)
    if s["kind"] == "lattice":
        assert c["bound"].max() < 2 ** 24, gc.case_id(s)
        amax, wmax = c["amax"], c["wmax"]
        assert K * amax * wmax < 2 ** 24
        lim = max(amax, 127) if s["c_bf16"] else amax             # (the three planted rows hold 64 / 127 and one more entry)
        for op in (c["x"], c["skip"]):
            assert op is None or op.size == 0 or (np.abs(op).max() <= lim and (op == np.rint(op)).all())
        if s["col"] or s["epi"]:
            assert 16 * K * amax * wmax + 2 * 128 + 64 < 2 ** 22
            q = c["pre"] * 4
            assert (q == np.rint(q)).all() and np.abs(c["pre"]).max() < 2 ** 22
        if s["entry"] == "bf16":
            assert amax <= 127 and wmax <= 127 and np.abs(c["W"]).max() <= 127
            for op in (c["x"], c["skip"], c["res"]):
                if op is not None:
                    gc.bf16_bits(op)                                   # (asserts exactness)
    else:
        assert not s["col"] and not s["epi"] and s["entry"] != "bf16"
        assert ((c["W"] == 1).sum(0) == 1).all() and ((c["W"] != 0).sum() == N)
        m = np.abs(c["x"].view(np.uint32) & 0x7FFFFF)
        assert (m & 0xFF).any() and (m & 0xFF00).any()                 # mantissa bits in the second and the third bf16 plane
    if s["leaky"] and s["kind"] == "lattice":
        tiles_ok, last_neg = gc.tile_statements(c)
        assert tiles_ok and last_neg, gc.case_id(s)
        if s["alpha"] != 0.25:
            assert s["alpha"] == 0.2 and (c["pre"] < 0).any()
            neg = c["pre"] < 0
            assert np.array_equal(c["want"][neg], c["pre"][neg].astype(np.float32) * np.float32(0.2))
    if s["c_bf16"]:
        t32 = c["pre"].astype(np.float32)
        post = np.where(c["pre"] > 0, t32, t32 * np.float32(s["alpha"])) if s["leaky"] else t32
        kinds = gc.rounding_kinds(post)
        assert all(k.any() for k in kinds), gc.case_id(s)
        assert sorted(v for _, _, v in c["planted"]) == [257, 259, 515]
        for (m, n, v), w in zip(c["planted"], (256.0, 260.0, 516.0)):
            assert post[m, n] == v and gc.bf16_f32(c["want"][m, n:n + 1])[0] == w
        trunc = (post.view(np.uint32) >> 16).astype(np.uint16)
        assert (trunc != c["want"]).any()
    for idx, rows, live in ((c["idx"], c["n1"], c["n1_dev"]), (c["ridx"], c["rrows"], s.get("res_rows_dev"))):
        if idx is None:
            continue
        col = idx[:, 0]
        for v in (-1, -2 ** 31, rows, rows + 3):
            assert (col == v).any(), (gc.case_id(s), v)
        if live is not None:
            assert live < rows and ((col >= live) & (col < rows)).any()
        assert ((col >= 0) & (col < (rows if live is None else live))).sum() > M // 2
    # poison: only rows the call may not read change, and every one of them becomes non-finite
    for m_dev in (None, M // 2):
        o = gc.poisoned(c, m_dev)
        m = M if m_dev is None else m_dev
        for k, lim in (("x", c["n1_dev"] if s["gather"] else m), ("skip", m), ("rs", m),
                       ("res", s.get("res_rows_dev") if s["gres"] else m)):
            if c[k] is None:
                continue
            lim = len(c[k]) if lim is None else lim
            assert np.array_equal(o[k][:lim], c[k][:lim]) and not np.isfinite(o[k][lim:]).any()
        buf = gc.expected_buffer(c, m_dev)
        assert buf.shape == (M + gc.PAD, N + s["ldc_pad"])
        sent = gc.SENT_H if s["c_bf16"] else gc.SENT
        assert (buf[m:] == sent).all() and (buf[:, N:] == sent).all() and np.array_equal(buf[:m, :N], c["want"][:m])
    return c


FAMILIES = {
    "x3": lambda: [s for N in gc.X3_N for K in gc.X3_SLICES for s in gc.x3_cases(N, K)] + gc.x3_extra_cases(),
    "gres": lambda: [s for s in gc.gres_cases() if s["M"] < 1000],
    "dma": lambda: [s for N in gc.DMA_N for K in gc.DMA_SLICES for s in gc.dma_cases(N, K)] + gc.dma_extra_cases(),
    "f32": gc.f32_cases,
    "bf16": lambda: [s for M in gc.BF16_M for K in gc.BF16_SLICES for N in gc.BF16_N for a in (0, 1) for cb in (0, 1)
                     for s in gc.bf16_cases(M, K, N, a, cb)],
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_statement_of_every_small_case(family):
    specs = FAMILIES[family]()
    assert len(specs) > 3
    assert len({gc.case_id(s) for s in specs}) == len(specs)
    for s in specs:
        _check_case(s)


def test_the_small_families_are_all_the_small_cases():
    assert sum(len(f()) for f in FAMILIES.values()) == len(gc.all_small_specs())


@pytest.mark.parametrize("shape", sorted(gc.X3_BIG))
def test_every_statement_of_the_256_row_tile_cases(shape):
    for s in gc.x3_big_cases(*shape):
        _check_case(s)


@pytest.mark.parametrize("N,K", [(32, 224), (36, 160), (100, 32)])
def test_every_statement_of_the_resident_walk_cases(N, K):
    """(three of the fifteen shapes are built here: the builder is the same for all, and the GPU test builds every one)"""
    for hint in (0, gc.X3R_TILE_HINT):
        for s in gc.x3r_cases(N, K, hint):
            if hint and s["id"] == "raw":
                continue
            _check_case(s)
    M = gc.X3R_M
    ntiles = gc.cdiv(M, 32)
    # every wave of a 256-CU chip walks three or four row tiles; with *M_dev = 33 all but two waves leave after the barrier
    per_wave = [gc.cdiv(ntiles - w, 8 * 256) for w in range(8 * 256)]
    assert set(per_wave) == {3, 4}


def test_every_resident_and_gres_shape_records_its_branch():
    for N, K in gc.X3R_SHAPES:
        assert gc.gemm_x3_resident(gc.X3R_M, N, K, 0) == 1 and gc.gemm_x3_resident(gc.X3R_M, N, K, gc.X3R_TILE_HINT) == 0
        for hint in (0, gc.X3R_TILE_HINT):
            for s in gc.x3r_cases(N, K, hint):
                it = s["intent"]
                assert (it["kernel"], it["S"], it["tiles"]) == gc.planned_branch(s)
    for N in (100, 128):                                 # (what does not fit the LDS there)
        assert gc.gemm_x3_resident(gc.X3R_M, N, 160, 0) == 0
    for s in gc.gres_cases() + gc.x3r_extra_cases():
        it = s["intent"]
        assert (it["kernel"], it["S"], it["tiles"]) == gc.planned_branch(s)
    big = [s for s in gc.gres_cases() if s["M"] >= 1000]
    assert len(big) == 1 and gc.gemm_x3_resident(big[0]["M"], big[0]["N"], big[0]["C1"], 0) == 1


def test_the_rotation_and_the_ring_are_covered():
    """the slice lengths of the shape tables: every step of the six-step rotation is the last one of some slice, unsplit and split,
    and the DMA ring sees slices shorter than, equal to and longer than its three stages"""
    unsplit = {t[0] for t in gc.X3_SLICES.values() if len(t) == 1}
    assert unsplit == set(range(1, 10))
    split = {n for t in gc.X3_SLICES.values() if len(t) > 1 for n in t}
    assert split == {5, 6, 7}
    assert {t[0] for t in gc.DMA_SLICES.values() if len(t) == 1} == {1, 2, 3, 4, 5}
    assert {n % 6 for n in unsplit} == set(range(6))
    # a concatenation boundary on every step of the rotation (tile index of the first k-tile of the second operand)
    cats = {s["C1"] // 32 for s in gc.x3_extra_cases() if s["C2"] and not s["gather"]}
    assert cats == {1, 2, 3, 4, 5}
    # nkt coprime to six in the resident walk: a row-tile boundary on every step
    assert {K // 32 for _, K in gc.X3R_SHAPES} >= {1, 5, 7}


def test_bf16_rounding_of_the_oracle():
    v = np.array([256, 257, 258, 259, 260, 515, 513, -257, -259, 0.5, 1.0], np.float32)
    assert gc.bf16_f32(gc.bf16_rne(v)).tolist() == [256, 256, 258, 260, 260, 516, 512, -256, -260, 0.5, 1.0]
    k = gc.rounding_kinds(np.array([257, 259, 515, 513, 256], np.float32))
    assert [a.tolist() for a in k] == [[False, False, True, False, False], [True, False, False, False, False],
                                       [False, True, False, False, False]]


# ---- against the library's own plans (host code only) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libd3feat_amd.so is not built")
    return _lib.load()


def _grid():
    g = set()
    for M in (1, 100, 130, 200, 777, 4525, 8448, 16640, 22016, 65535, 65536, 70000, gc.X3R_M, 707592):
        for N in (4, 20, 32, 33, 36, 64, 96, 100, 128, 132, 256, 512):
            for K in (4, 32, 36, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 416, 480, 512, 544, 576, 800, 1024, 3072, 7680):
                for hint in (0, 60000, 150):
                    g.add((M, N, K, hint))
    specs = gc.all_small_specs() + gc.gres_cases() + gc.x3r_extra_cases()
    specs += [s for k in gc.X3_BIG for s in gc.x3_big_cases(*k)]
    specs += [s for N, K in gc.X3R_SHAPES for h in (0, gc.X3R_TILE_HINT) for s in gc.x3r_cases(N, K, h)]
    for s in specs:
        if s["C1"] + s["C2"]:
            g.add((s["M"], s["N"], s["C1"] + s["C2"], s["hint"]))
    return sorted(g)


def test_the_restated_plans_are_the_librarys(lib):
    r, c, sl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n = 0
    for M, N, K, hint in _grid():
        _, _, S, _ = gc.gemm_plan(M, N, K, hint)
        assert lib.d3f_gemm_workspace_bytes(M, N, K, hint) == gc.slab_bytes(S, M, N), (M, N, K, hint)
        S, _ = gc.gemm_bf16_split(M, N, K, hint)
        assert lib.d3f_gemm_bf16_workspace_bytes(M, N, K, hint) == gc.slab_bytes(S, M, N), (M, N, K, hint)
        assert lib.d3f_gemm_x3_resident(M, N, K, hint) == gc.gemm_x3_resident(M, N, K, hint), (M, N, K, hint)
        if K % 32 == 0:
            tn, waves, S, _ = gc.gemm_x3_plan(M, N, K, hint)
            assert lib.d3f_gemm_x3_plan(M, N, K, hint, ctypes.byref(r), ctypes.byref(c), ctypes.byref(sl)) == 0
            assert (r.value, c.value, sl.value) == (32 * waves, 32 * tn, S), (M, N, K, hint)
            assert lib.d3f_gemm_x3_workspace_bytes(M, N, K, hint) == gc.slab_bytes(S, M, N), (M, N, K, hint)
            n += 1
    assert n > 3000
