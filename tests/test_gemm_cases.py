"""Every statement of every case of oracle/gemm_cases.py, checked from the oracle alone (no GPU, no kernel): the exactness budget
(max(|A| @ |W|) < 2^24, every intermediate of the epilogue equal to its own float32 rounding), the placement of signs, exact zeros
and bfloat16 ties, the shadow indices, what poisoned() poisons, and that the branch a case records (written down from the shape
tables) is what the restated host plans give.  Where libd3feat_amd.so is built, the restated plans are compared with the library's own
(d3f_gemm_x3_plan, d3f_gemm_x3_resident, d3f_gemm_x3_chain_ok, the S implied by the three *_workspace_bytes functions) over a grid
of (M, N, K, hint) that includes every case.  The chained cases (d3f_gemm_x3_chain) add the second level: exact2 -- the recorded
condition that fp32 arithmetic of the second product and epilogue is exact -- the leaky statements of the second output, the
restated LDS image and the instance a case names.  The host-side refusals of the six entry points are tests/test_cabi.py::test_gemm_entry_points_refuse_*."""
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


def _check_chain_case(s):
    """the first level by _check_case (the case IS an x3 case with its own magnitudes); then every statement of the second level"""
    c = _check_case(s)
    M, N, K, cid = s["M"], s["N"], c["K"], gc.case_id(s)
    f = c["first"]
    assert f["spec"]["entry"] == "x3" and c["want"] is f["want"] and c["x"] is f["x"] and c["W"] is f["W"]
    assert c["exact"] and c["exact2"], cid
    assert c["want2"].shape == (M, 32) and c["want2"].dtype == np.float32 and np.isfinite(c["want2"]).all()
    # the instance and its LDS image
    assert s["intent"]["kernel"] == "gemm_x3r_chain_kernel<%d,%s>" % (N // 32, "true" if s["store"] else "false"), cid
    assert gc.gemm_x3r_chain_lds_bytes(K // 32, N // 32, s["store"]) <= gc.LDS_LIMIT and gc.gemm_x3_chain_accepts(N, K, s["store"])
    assert gc.gemm_x3_resident(M, N, K, 0) == gc.gemm_x3_chain_ok(M, N, K, s["store"])
    W2 = c["W2"]
    assert W2.shape == (N, 32)
    if s["kind"] == "select2":
        assert not (s["cs2"] or s["ch2"] or s["leaky2"] or s["leaky"])
        assert ((W2 == 1).sum(0) == 1).all() and (W2 != 0).sum() == 32
        # every element of the second output is ONE operand of A, bit for bit -- restated from the operands alone
        sel = c["W"].argmax(0)[W2.argmax(0)]
        if s["gather"]:
            rows = c["idx"][:, 0].astype(np.int64)
            ok = (rows >= 0) & (rows < c["n1_dev"])
            a = np.where(ok[:, None], c["x"][np.where(ok, rows, 0)], np.float32(0))
        else:
            a = c["x"][:M]
        a = np.concatenate([a, c["skip"]], 1) if c["skip"] is not None else a
        assert np.array_equal(c["want2"].view(np.uint32), np.ascontiguousarray(a[:, sel]).view(np.uint32)), cid
        low = c["want2"].view(np.uint32) & 0xFF
        assert (low != 0).mean() > 0.9                                  # bits in the third plane of nearly every output
    elif s["w2"] == "select":
        assert s["alpha"] == 0.2 and s["alpha2"] == 0.2 and s["leaky"] and s["leaky2"] and not s["ch2"]
        assert ((W2 == 1).sum(0) <= 1).all() and (W2 != 0).sum() == 31
        neg = c["pre2"] < 0
        assert neg.any() and np.array_equal(c["want2"][neg], c["pre2"][neg].astype(np.float32) * np.float32(0.2))
        assert (c["want"].view(np.uint32) & 0xFF).any()                 # the first output is no lattice: full mantissas
    else:
        assert np.abs(W2).max() <= s["w2max"] == 2 and (W2 == np.rint(W2)).all() and not W2[:, c["zero_cols2"]].any()
        assert c["amax"] == 3 and c["wmax"] == 2 and np.abs(c["W"]).max() <= 2
        # u is 1/16 after a LeakyReLU with alpha 0.25 on multiples of 1/4, 1 on a raw product; the sums keep a margin of 16
        assert c["unit2"] == (1 / 16 if s["leaky"] else 1.0), cid
        assert c["bound2"] < 2 ** 20, (cid, c["bound2"])
        q = c["pre2"] / (c["unit2"] / 2)
        assert (q == np.rint(q)).all() and np.abs(q).max() < 2 ** 22, cid
    if c["ch2"] is not None:
        assert not c["ch2"][c["zero_cols2"]].any()
    if s["leaky2"]:
        assert gc.tile_statements(c, "pre2") == (True, True), cid
        assert s["alpha2"] in (0.25, 0.2)
    # the poison leaves the expectation alone: no operand of the second level depends on a row, W2 keeps its values inside NaN
    for m_dev in (None, 33):
        o = gc.poisoned(c, m_dev)
        w2 = o["W2"].reshape(N, o["ldb2"])
        assert o["ldb2"] == 36 and np.array_equal(w2[:, :32], W2) and np.isnan(w2[:, 32:]).all()
        m = M if m_dev is None else m_dev
        buf = gc.expected_buffer(c, m_dev, second=True)
        assert buf.shape == (M + gc.PAD, 32 + s["ldc2_pad"])
        assert (buf[m:] == gc.SENT).all() and (buf[:, 32:] == gc.SENT).all() and np.array_equal(buf[:m, :32], c["want2"][:m])
    return c


@pytest.mark.parametrize("K,N,store", sorted(gc.CHAIN_SHAPES))
def test_every_statement_of_the_chain_walk_cases(K, N, store):
    raw, full = gc.chain_cases(K, N, store)
    assert raw["M"] == gc.X3R_M and not (raw["epi"] or raw["col"] or raw["cs2"] or raw["ch2"] or raw["leaky2"])
    assert full["epi"] == 3 and full["leaky"] and full["cs2"] and full["ch2"] and full["leaky2"] and full["alpha2"] == 0.25
    assert full["ldr_pad"] == 4 and full["ldc_pad"] == (4 if store else 0) and full["ldc2_pad"] == 4
    for s in (raw, full):
        assert s["C1"] + s["C2"] == K and bool(s["gather"]) == gc.CHAIN_SHAPES[(K, N, store)][2]
        _check_chain_case(s)


@pytest.mark.parametrize("s", gc.chain_extra_cases(), ids=gc.case_id)
def test_every_statement_of_the_other_chain_cases(s):
    _check_chain_case(s)


def test_the_chain_shapes_cover_every_instance_and_both_boundaries():
    shapes = sorted(gc.CHAIN_SHAPES)
    assert len(shapes) == 9 and {(N, st) for _, N, st in shapes} == set(gc.CHAIN_KERNELS)
    for N in (64, 128):
        for st in (False, True):
            Kmax = gc.chain_largest_k(N, st)
            assert (Kmax, N, st) in gc.CHAIN_SHAPES                      # the largest image of every instance is walked
            assert gc.gemm_x3_chain_accepts(N, Kmax, st) and not gc.gemm_x3_chain_accepts(N, Kmax + 32, st)
    assert {(N, st): gc.chain_largest_k(N, st) for N in (64, 128) for st in (False, True)} == \
        {(64, False): 288, (64, True): 224, (128, False): 128, (128, True): 96}
    assert gc.gemm_x3r_chain_lds_bytes(4, 4, False) == 5 * 4 * 7680 + 1280 == 154880
    # the entry point takes K = 288 at 64 columns, the router's predicate does not (d3f_gemm_x3 has no resident form there)
    assert gc.gemm_x3_chain_ok(100000, 64, 288, False) == 0 and gc.gemm_x3_chain_ok(100000, 64, 256, False) == 1
    # every wave of a chip of up to 384 CUs walks three tiles or more
    assert gc.cdiv(gc.X3R_M, 32) > 2 * 8 * 384
    ids = [gc.case_id(s) for k in shapes for s in gc.chain_cases(*k)] + [gc.case_id(s) for s in gc.chain_extra_cases()]
    assert len(set(ids)) == len(ids)
    kinds = [s["id"] for s in gc.chain_extra_cases()]
    assert kinds.count("select2") == 2 and kinds.count("alpha0.2") == 2 and "scale2-only" in kinds and "shift2-only" in kinds
    assert {s["intent"]["kernel"] for s in gc.chain_extra_cases() if s["id"] == "select2"} == \
        {"gemm_x3r_chain_kernel<2,false>", "gemm_x3r_chain_kernel<4,true>"}


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


def test_the_restated_chain_predicate_is_the_librarys(lib):
    n = 0
    for M in (1, 1000, 65535, 65536, 100000, gc.X3R_M, 707592):
        for N in (32, 64, 96, 100, 128, 256):
            for K in list(range(32, 385, 32)) + [0, 16, 48]:
                for store in (0, 1):
                    for hint in (0, 1000, 70000):
                        assert lib.d3f_gemm_x3_chain_ok(M, N, K, store, hint) == gc.gemm_x3_chain_ok(M, N, K, store, hint), (M, N, K, store, hint)
                        n += 1
    for k in gc.CHAIN_SHAPES:
        for s in gc.chain_cases(*k) + gc.chain_extra_cases():
            K = s["C1"] + s["C2"]
            assert lib.d3f_gemm_x3_chain_ok(s["M"], s["N"], K, int(s["store"]), 0) == gc.gemm_x3_resident(s["M"], s["N"], K, 0)
    assert n > 2000
