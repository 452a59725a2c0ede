"""Every kernel instance and pipeline branch of the contraction family -- csrc/gemm_f32.hip, gemm_dma.h, gemm_x3.h and the shared
K-split reduction of gemm_common.h -- bit for bit against integer / float64 expectations that no kernel had a part in
(oracle/gemm_cases.py; tests/test_gemm_cases.py checks every statement of every case on the CPU).  NO TOLERANCE anywhere: the operands
are lattices whose fp32 arithmetic is exact in every summation order (or 0/1 selections of full 24-bit mantissas), so every
comparison is np.array_equal on VALUES over the WHOLE output buffer -- the documented rows, and the sentinel in everything else: the
PAD rows behind the output, the rows from *M_dev on, the columns N .. ldc - 1 of every row.  NaN anywhere fails.

Entry points are called through _lib.load() with a workspace of exactly the advertised size, filled with NaN (every slab element
the reduction reads must have been written); every operand carries NaN / Inf in every float the contract says is not read
(oracle.gemm_cases.poisoned and .widen: rows past *M_dev / *N1_dev / *res_rows_dev, the columns between the rows where a leading
dimension exceeds the width, the floats in front of a shifted base).  Packed weights are made from a column view of a wider matrix
(ldb = N + 4, NaN beside it), so the pack kernels are checked through every product.  Every case first asserts, from the
library's own plan functions, that it lands in the branch it names; no case skips.  Every K-split case runs twice on one workspace,
with other operands the second time (a stale slab).  Where the branch is the Python router (bfloat16 tensors, gemm_upsample_split)
the call goes through d3feat_amd.ops.

Branch -> test
--------------
  gemm_x3_kernel<1,4> (N = 4, 32), <2,4> (N = 36, 64, 96, 100)       test_x3_tile_kernels[N-K]: M = 200 (two row tiles, the last ragged)
    rotation, unsplit: last step 0 .. 5 and the second trip          K = 32 .. 288 (1 .. 9 k-tiles)
    rotation, split: slices of 5, 6, 7 tiles, S = 2 and 3            K = 320 (5+5), 352 (6+5), 416 (7+6), 480 (5+5+5), 544 (6+6+5)
    the clamped over-request ("the last tile again")                 every K above: the request runs two tiles past every slice end
    three column groups, group index clamped to NG - 1               test_x3_tile_kernels[96-*]
    EPI: raw, col only, + row scale, + residual, both (ldc = N + 4)  test_x3_tile_kernels[*-160], [*-352]; raw + full everywhere else
    a_rebase on every rotation step (C1 = 32 .. 160 of K = 192, 224) test_x3_more[*cat*]
    gathered x: shadow indices, ld_idx 1 / 3, *N1_dev < N1           test_x3_more[*gather*]
    selection operands, alpha = 0.2                                  test_x3_more[*select*], [*alpha0.2]
    *M_dev = 0, 1, 127, 128, 129, M (unsplit and split)              test_x3_row_counts[N-K]
  gemm_x3_kernel<4,8>: one k-tile; S 3 (11+11+10); five column       test_x3_256_row_tiles[shape] (each also with *M_dev = M - 100: a ragged
    groups with the last workgroup clamped                           row tile)
  gemm_x3r_kernel<1>, <2>, <4>: nkt 1, 5, 7 (1, 3, 4 at N > 64),     test_x3_resident_walk[N-K]: M = 3 * 65536 + 37, raw + full epilogue,
    a row-tile boundary on every step, three / four tiles per wave   gathered + concatenated operands
    *M_dev = 0 / 1 / 33 (most waves leave after the barrier) / 65535 the same tests, on the full case
    the same shapes with M_hint < 65536: the tile form, same values  the same tests
    selection operands, alpha = 0.2                                  test_x3_resident_more[id]
  gemm_x3r_chain_kernel<2,false>: K 256 (gathered 128 + skip 128:    test_x3_chain_walk[N-K-store] (d3f_gemm_x3_chain): M = 3 * 65536 + 37 and, asserted
    the decoder pair), 288 (the largest image the entry point        first, more than 2 * 8 * CUs row tiles -- EVERY wave walks three tiles or more:
    takes), 32 (one k-tile: a tile boundary on every step)           the accumulators cleared in finish_tile, the fresh acc2, the patch reused for
  gemm_x3r_chain_kernel<2,true>: K 224 (96 + 128: the largest        the N-column and the 32-column stores of consecutive tiles, requests across a
    stored image at 64 columns), 160 (five k-tiles)                  tile boundary (rq_rows of the next tile, gathered indices included), a_rebase at
  gemm_x3r_chain_kernel<4,true>: K 96 (32 + 64: the encoder pair,    K1 inside the walk, c_tile += tstride.  Raw (no epilogue operand at either level)
    a_rebase at k-tile 1), 32                                        and full: row scale, column scale and shift, residual (ldr = N + 4), LeakyReLU,
  gemm_x3r_chain_kernel<4,false>: K 128 (64 + 64: the largest        ldc = N + 4 where stored (C = NULL where not), the second epilogue on, ldc2 = 36.
    image at 128 columns), 64 (gathered 32 + skip 32)                Whole buffers: the second output always, the first where stored -- and that one
    *M_dev = 0 / 1 / 33 / 65535: a walk that ends early              against the expectation of the d3f_gemm_x3 case of the same operands.  The full
                                                                     case at every *M_dev of X3R_MDEV
    both 0/1 selections of full mantissas (select2): the exact       test_x3_chain_more[*select2] on <2,false> and <4,true>
    three-plane split of the finished value, W2's k order
    alpha = alpha2 = 0.2; second epilogue scale only / shift only    test_x3_chain_more[*alpha0.2], [*scale2-only], [*shift2-only], [*ldc2-32] (the
    (NULL pointers); ldc2 = 32                                       last also with *M_dev = 65535)
    the LDS boundary of the entry point and of the predicate         test_x3_chain_lds_boundary[N-store]: the largest K of the restated formula is
                                                                     launched, K + 32 is D3F_ERR_ARG with both outputs untouched,
                                                                     d3f_gemm_x3_chain_ok draws the same line where d3f_gemm_x3 is resident
  d3f_gemm_x3_gres: gemm_residual_row in the direct epilogue (K 64)  test_x3_gathered_residual[id]: ld_res_idx 1 / 3, indices negative, equal
    and in gemm_splitk_reduce_kernel (K 352)                         to and beyond the row count, *res_rows_dev < res_rows, a row scale
    a call for which d3f_gemm_x3_resident answers 1                  test_x3_gathered_residual[*resident-shape]: still the tile form
  ops.gemm_upsample_split (the router of the decoder's split form)   test_upsample_split_router
  gemm_dma_kernel<4,1,EPI>, <2,2,EPI>, EPI 0 .. 3                    test_dma_ring[N-K]: M = 100 (fewer than 8 items: the padded grid)
    ring of three: slices of 1, 2, 3, 4, 5 tiles; K % 32 (4, 36:     K = 4, 32, 36, 64, 96, 128, 160, 544 (9+8), 800 (9+9+7); lda = K + 4 with
    A columns beyond K from the zero line)                           NaN behind every row
    a concatenation boundary inside a k-tile (C1 = 36), gathered x   test_dma_more[*cat36*], [*gather*]
    selection operands, alpha = 0.2, *M_dev                          test_dma_more[*select*], [*alpha0.2], test_dma_row_counts[N-K]
  gemm_fast_kernel<4,1,EPI>, <2,2,EPI>: K = 0, 96, 544 (9+8)         test_f32_entries[fast-*] (d3f_gemm_f32, d3f_gemm_upsample_cat_f32)
  gemm_f32_kernel<4,1>, <2,2> by each single cause, unsplit + split  test_f32_entries[generic-*]: odd K, odd N, odd lda (vecA off alone), odd
                                                                     ldb (vecB off alone), odd ldc, A / B base 4 bytes off
    *M_dev on both kernels                                           test_f32_row_counts[kind-N-K]
  gemm_bf16_kernel<0,0>, <0,1>, <1,0>, <1,1>; res_bf16 / c_bf16 of   test_bf16_kernels[M-K-N]: all four through the C ABI (8-byte aligned
    gemm_splitk_reduce_kernel (K = 544: 9+8, K = 1024: 4 x 8)        bf16 bases), raw / full epilogue with a bf16 residual / gathered +
    RNE of the output: planted 257 (tie down), 259 (tie up), 515     concatenated; <1,1>, <1,0>, <0,0> also through ops.gemm,
                                                                     gemm_upsample_cat and gemm_cat2 under ops.bf16_contraction
  gemm_pack_x3_kernel, gemm_pack_f32t_kernel, gemm_pack_bf16_kernel  every test above: ldb = N + 4, NaN beside the matrix
  gemm_pack_x3_kernel, chain = 1 (d3f_gemm_pack_x3_chain)            every test_x3_chain_* case: W2 from a column view, ldb = 36, NaN beside it
  gemm_splitk_reduce_kernel: stale slab                              every split case above runs twice on one workspace

No defect found: every case passes on the library as it was before this file, and the chained cases on the library as it was before
them (the header comment of d3f_gemm_x3_chain named K <= 96 for N = 128 whatever is stored; the code takes, and
test_x3_chain_walk[128-128-0] runs, K = 128 with the first output not stored: the comment was wrong, not the code).
What the chained cases catch, tried on scratch copies of the library (value-only edits, one at a time): W2 packed in
d3f_gemm_pack_x3's plain k order -- every test_x3_chain_walk and test_x3_chain_more case fails; the accumulators of the first product
not cleared at the end of finish_tile -- every test_x3_chain_walk and test_x3_chain_more case fails (and the walk-size rows of
tests/test_gpu_gemm_chain.py) while every test at one tile per wave still passes; the second epilogue reading the first epilogue's
vectors -- every case fails; the finished value split into two planes only -- the select2 and alpha0.2 cases fail, the lattice cases
(at most 16 significant bits) do not.

Cost, measured on an MI355X: the 338 tests take 38.9 s run alone (pytest's figure; 34.5 s for the 317 before the chained cases).
The nine test_x3_chain_walk cases are the slowest with 0.8 .. 2.0 s each (six launches of 196 645 rows each, operands of up to 57 M
floats, two expectations in float64 on the host), the fifteen test_x3_resident_walk cases take 0.3 .. 1.6 s (eight launches), the
eight test_x3_chain_more cases 0.6 .. 1.1 s, test_x3_chain_lds_boundary under 0.1 s; nothing else reaches 0.5 s.  One complete
`pytest -m gpu tests` run with this file took 331.3 s (1680 passed, 5 skipped); the figure before the chained cases, from an earlier
state of the suite, was 390.8 s (1333 passed, 5 skipped).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gemm_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _x3_plan(lib, M, N, K, hint):
    r, c, s = C.c_int(), C.c_int(), C.c_int()
    assert lib.d3f_gemm_x3_plan(M, N, K, hint, C.byref(r), C.byref(c), C.byref(s)) == 0
    return r.value, c.value, s.value


def workspace_bytes(lib, s):
    M, N, K, hint = s["M"], s["N"], s["C1"] + s["C2"], s["hint"]
    fn = {"x3": lib.d3f_gemm_x3_workspace_bytes, "x3_gres": lib.d3f_gemm_x3_workspace_bytes,
          "bf16": lib.d3f_gemm_bf16_workspace_bytes}.get(s["entry"], lib.d3f_gemm_workspace_bytes)
    return int(fn(M, N, K, hint))


def assert_branch(lib, s, ptrs=None):
    """the case lands in the branch it names, by the library's own plan functions"""
    M, N, K, hint, it = s["M"], s["N"], s["C1"] + s["C2"], s["hint"], s["intent"]
    if s["entry"] == "chain":
        # the instance follows from N and from whether a first output is handed over; the LDS image must fit; no workspace
        stored = bool(ptrs["C"])
        assert stored == bool(s["store"]) and it["kernel"] == gc.CHAIN_KERNELS[(N, stored)] and it["tiles"] == (K // 32,)
        assert gc.gemm_x3r_chain_lds_bytes(K // 32, N // 32, stored) <= gc.LDS_LIMIT
        assert lib.d3f_gemm_x3_chain_ok(M, N, K, int(stored), hint) == lib.d3f_gemm_x3_resident(M, N, K, hint)
        return 0
    wsb = workspace_bytes(lib, s)
    if s["entry"] in ("x3", "x3_gres"):
        resident = lib.d3f_gemm_x3_resident(M, N, K, hint)
        if it["kernel"].startswith("gemm_x3r"):
            assert s["entry"] == "x3" and resident == 1 and it["kernel"] == "gemm_x3r_kernel<%d>" % {1: 1, 2: 2, 4: 4}[gc.cdiv(N, 32)]
            return wsb
        assert resident == 0 or s["entry"] == "x3_gres"
        rows, cols, S = _x3_plan(lib, M, N, K, hint)
        assert it["kernel"] == "gemm_x3_kernel<%d,%d>" % (cols // 32, rows // 32) and it["S"] == S
    elif s["entry"] == "bf16":
        assert it["kernel"] == "gemm_bf16_kernel<%d,%d>" % (s["a_bf16"], s["c_bf16"])
    else:
        shape = "4,1" if N <= 32 else "2,2"
        if s["entry"] == "f32t":
            assert it["kernel"] == "gemm_dma_kernel<%s,%d>" % (shape, s["epi"] & 3)
        else:
            # gemm_run's choice between its two kernels, from the addresses and leading dimensions actually handed over
            fast = all(v % 4 == 0 for v in ptrs["lds"]) and all(p % 16 == 0 for p in ptrs["bases"]) and K % 4 == 0 and N % 4 == 0
            want = "gemm_fast_kernel<%s,%d>" % (shape, s["epi"] & 3) if fast else "gemm_f32_kernel<%s>" % shape
            assert it["kernel"] == want
    assert wsb == gc.slab_bytes(it["S"], M, N)           # the S of the launcher, through its workspace function
    return wsb


class Launch:
    """one call of a case through the C ABI: uploads the poisoned operands, packs the weights, launches, returns the whole output buffer"""

    def __init__(self, lib, dev, c, m_dev=None, ws=None):
        s = c["spec"]
        self.lib, self.dev, self.c, self.s, self.m_dev = lib, dev, c, s, m_dev
        M, N, C1, C2 = s["M"], s["N"], s["C1"], s["C2"]
        K = C1 + C2
        o = gc.poisoned(c, m_dev)
        h, e = s["a_bf16"], s["entry"]
        self.keep = []
        off = 4 if h else s["a_off"]                     # bfloat16 bases: 8-byte, not 16-byte aligned

        def op(a, pad, off=0):
            if a is None or a.shape[1] == 0:
                return None, 0
            flat, ld = gc.widen(a, pad, off=off)
            if h:
                flat = gc.bf16_bits(flat).view(np.int16)
            t = _up(flat, dev)
            self.keep.append(t)
            return t.data_ptr() + off * t.element_size(), ld
        pA, lda = op(o["x"], s["lda_pad"], off)
        pS, lds = op(o["skip"], s["lds_pad"], 4 if h else 0)
        pR, ldr = op(o["res"], s["ldr_pad"], 4 if h else 0)

        def vec(a, dtype=None):
            if a is None:
                return None
            t = _up(a if dtype is None else a.astype(dtype), dev)
            self.keep.append(t)
            return t.data_ptr()
        pidx, pridx = vec(o["idx"]), vec(o["ridx"])
        prs, pcs, pch = vec(o["rs"]), vec(c["cs"]), vec(c["ch"])
        pmd = vec(np.array([m_dev], np.int32)) if m_dev is not None else None
        pn1 = vec(np.array([c["n1_dev"]], np.int32)) if c["n1_dev"] is not None else None
        prr = vec(np.array([s["res_rows_dev"]], np.int32)) if s.get("res_rows_dev") is not None else None
        # the weights: a column view of a wider matrix (packed entries: always ldb = N + 4)
        packed = e in ("x3", "x3_gres", "chain", "f32t", "bf16")
        ldb_pad = 4 if packed else s["ldb_pad"]
        pW = ldb = None
        if K:
            wflat, ldb = gc.widen(c["W"], ldb_pad, off=0 if packed else s["b_off"])
            tw = _up(wflat, dev)
            self.keep.append(tw)
            pW = tw.data_ptr() + (0 if packed else 4 * s["b_off"])
        if packed:
            Kp = gc.cdiv(K, 32) * 32
            if e in ("x3", "x3_gres", "chain"):
                nb = int(lib.d3f_gemm_x3_packed_bytes(K, N))
                assert nb == gc.cdiv(N, 32) * (K // 32) * gc.X3_CHUNK_BYTES
                wp = torch.full((nb,), 0x7F, dtype=torch.uint8, device=dev)
                assert lib.d3f_gemm_pack_x3(pW, ldb, K, N, wp.data_ptr(), None) == 0
            elif e == "f32t":
                wp = torch.full((N * Kp,), float("nan"), dtype=torch.float32, device=dev)
                assert lib.d3f_gemm_pack_f32t(pW, ldb, K, N, wp.data_ptr(), None) == 0
            else:
                wp = torch.full((N * Kp,), 0x7FC0, dtype=torch.int16, device=dev)
                assert lib.d3f_gemm_pack_bf16(pW, ldb, K, N, wp.data_ptr(), None) == 0
            self.keep.append(wp)
            pW = wp.data_ptr()
        ldc = N + s["ldc_pad"]
        if e == "chain":
            # W2 through d3f_gemm_pack_x3_chain from a column view (ldb = 36, NaN beside it); the second output with its own sentinel
            tw2 = _up(o["W2"], dev)
            nb2 = int(lib.d3f_gemm_x3_packed_bytes(N, 32))
            assert o["ldb2"] == 36 and nb2 == (N // 32) * gc.X3_CHUNK_BYTES
            w2p = torch.full((nb2,), 0x7F, dtype=torch.uint8, device=dev)
            assert lib.d3f_gemm_pack_x3_chain(tw2.data_ptr(), o["ldb2"], N, 32, w2p.data_ptr(), None) == 0
            self.keep += [tw2, w2p]
            self.ldc2 = 32 + s["ldc2_pad"]
            self.out2 = torch.full(((M + gc.PAD) * self.ldc2,), float(gc.SENT), dtype=torch.float32, device=dev)
        if e == "chain" and not s["store"]:
            self.out = None                              # C = NULL: the first output is not stored
        elif s["c_bf16"]:
            self.out = torch.full(((M + gc.PAD) * ldc,), int(np.uint16(gc.SENT_H).view(np.int16)), dtype=torch.int16, device=dev)
        else:
            self.out = torch.full(((M + gc.PAD) * ldc,), float(gc.SENT), dtype=torch.float32, device=dev)
        self.wsb = assert_branch(lib, s, dict(lds=[lda, lds, ldb or 0, ldc, ldr], bases=[p or 0 for p in (pA, pS, pW, pR, pcs, pch, self.out.data_ptr() if self.out is not None else 0)],
                                                C=self.out is not None))
        if ws is None:
            ws = torch.full((self.wsb // 4,), float("nan"), dtype=torch.float32, device=dev)
        assert ws.numel() * 4 == self.wsb
        self.ws = ws
        n1 = c["n1"]
        tail = [ws.data_ptr(), C.c_size_t(self.wsb), pmd]
        flags = [1 if s["leaky"] else 0, float(s["alpha"])]
        pC = self.out.data_ptr() if self.out is not None else None
        if e == "chain":
            self.fn = lib.d3f_gemm_x3_chain
            self.args = [pA, n1, lda, C1, pidx, s["ld_idx"], pS, lds, C2, pW, pC, ldc, M, N, prs, pcs, pch, pR, ldr] + flags + \
                        [w2p.data_ptr(), vec(c["cs2"]), vec(c["ch2"]), 1 if s["leaky2"] else 0, float(s["alpha2"]), self.out2.data_ptr(), self.ldc2,
                         pmd, pn1, None]
        elif e == "f32":
            self.fn, self.args = lib.d3f_gemm_f32, [pA, max(lda, K), pW, ldb or N, pC, ldc, M, N, K, prs, pcs, pch, pR, ldr] + flags + tail + [s["hint"], None]
        elif e == "upcat":
            self.fn = lib.d3f_gemm_upsample_cat_f32
            self.args = [pA, n1, lda, C1, pidx, s["ld_idx"], pS, lds, C2, pW, ldb, pC, ldc, M, N, pcs, pch] + flags + tail + [pn1, s["hint"], None]
        else:
            head = [pA, n1, lda, C1, pidx, s["ld_idx"], pS, lds, C2, pW, pC, ldc, M, N, prs, pcs, pch, pR, ldr]
            if e == "x3_gres":
                self.fn = lib.d3f_gemm_x3_gres
                self.args = head + [pridx, s["ld_res_idx"], s["res_rows"], prr] + flags + tail + [pn1, s["hint"], None]
            else:
                self.fn = {"x3": lib.d3f_gemm_x3, "f32t": lib.d3f_gemm_f32t, "bf16": lib.d3f_gemm_bf16}[e]
                self.args = head + flags + tail + [pn1, s["hint"]] + ([h, s["c_bf16"]] if e == "bf16" else []) + [None]

    def run(self):
        rc = self.fn(*self.args)
        assert rc == 0, (gc.case_id(self.s), rc)
        torch.cuda.synchronize()
        s = self.s
        if self.out is None:
            return None
        got = self.out.cpu().numpy().reshape(s["M"] + gc.PAD, s["N"] + s["ldc_pad"])
        return got.view(np.uint16) if s["c_bf16"] else got

    def second(self):
        """(after run) the whole second output buffer of a chained case"""
        return self.out2.cpu().numpy().reshape(self.s["M"] + gc.PAD, self.ldc2)


def _same(c, m_dev, got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        s = c["spec"]
        raise AssertionError("%s%s (*M_dev %s): %d elements differ, first at %s: got %r, want %r; rows %d..%d, columns %d..%d"
                             % (gc.case_id(s), what, m_dev, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])],
                                bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()))


def check(lib, dev, c, m_dev=None, ws=None):
    """launch, compare the WHOLE buffer (expectation + every sentinel); -> the workspace, for a second call on it"""
    L = Launch(lib, dev, c, m_dev, ws)
    _same(c, m_dev, L.run(), gc.expected_buffer(c, m_dev))
    return L.ws


def check_chain(lib, dev, c, m_dev=None):
    """a chained case: the WHOLE second output buffer and, where it is stored, the WHOLE first one -- against the chained case's
    expectation and against what the d3f_gemm_x3 case of the same first-level operands (c["first"]) expects, which must be the same"""
    s = c["spec"]
    assert s["entry"] == "chain" and c["exact"] and c["exact2"], gc.case_id(s)
    L = Launch(lib, dev, c, m_dev)
    got = L.run()
    _same(c, m_dev, L.second(), gc.expected_buffer(c, m_dev, second=True), " second output")
    if s["store"]:
        x3 = c["first"]
        assert x3["spec"]["entry"] == "x3" and lib.d3f_gemm_x3_resident(s["M"], s["N"], c["K"], 0) == 1
        _same(c, m_dev, got, gc.expected_buffer(x3, m_dev), " first output")
        assert np.array_equal(gc.expected_buffer(x3, m_dev), gc.expected_buffer(c, m_dev))
    else:
        assert got is None


def check_twice_if_split(lib, dev, s, c=None):
    """the case; a K-split case a second time on the SAME workspace with other operands (a stale slab must be overwritten whole)"""
    c = c if c is not None else gc.build(s)
    ws = check(lib, dev, c)
    if s["intent"]["S"] > 1:
        check(lib, dev, gc.build(dict(s, seed=s["seed"] + 1)), ws=ws)
    return c


# ---- gemm_x3_kernel, 128-row tiles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted(gc.X3_SLICES))
@pytest.mark.parametrize("N", gc.X3_N)
def test_x3_tile_kernels(lib, device, N, K):
    cases = gc.x3_cases(N, K)
    assert len(cases) == (5 if K in gc.X3_ALL_EPI_K else 2)
    for s in cases:
        check_twice_if_split(lib, device, s)


@pytest.mark.parametrize("s", gc.x3_extra_cases(), ids=gc.case_id)
def test_x3_more(lib, device, s):
    check_twice_if_split(lib, device, s)


@pytest.mark.parametrize("K", gc.X3_ALL_EPI_K)
@pytest.mark.parametrize("N", (32, 100))
def test_x3_row_counts(lib, device, N, K):
    s = gc.x3_cases(N, K)[1]
    c = gc.build(s)
    for m_dev in gc.X3_MDEV:
        check(lib, device, c, m_dev)


@pytest.mark.parametrize("shape", sorted(gc.X3_BIG), ids=lambda t: "%dx%dx%d" % t)
def test_x3_256_row_tiles(lib, device, shape):
    for s in gc.x3_big_cases(*shape):
        c = check_twice_if_split(lib, device, s)
        if s["id"] == "full":
            check(lib, device, c, shape[0] - 100)


# ---- gemm_x3r_kernel: the resident-W walk ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gc.X3R_SHAPES)
def test_x3_resident_walk(lib, device, N, K):
    raw, full = gc.x3r_cases(N, K)
    check(lib, device, gc.build(raw))
    c = gc.build(full)
    for m_dev in gc.X3R_MDEV:
        check(lib, device, c, None if m_dev == gc.X3R_M else m_dev)
    # the same operands with M_hint below 65536: the tile form, the same values
    hinted = gc.x3r_cases(N, K, gc.X3R_TILE_HINT)[1]
    assert {k: v for k, v in hinted.items() if k not in ("hint", "intent")} == {k: v for k, v in full.items() if k not in ("hint", "intent")}
    assert hinted["intent"]["kernel"].startswith("gemm_x3_kernel")
    check(lib, device, dict(c, spec=hinted))
    check(lib, device, dict(c, spec=hinted), 65535)


@pytest.mark.parametrize("s", gc.x3r_extra_cases(), ids=gc.case_id)
def test_x3_resident_more(lib, device, s):
    check(lib, device, gc.build(s))


# ---- gemm_x3r_chain_kernel: the chained form in the multi-tile walk -----------------------------------------------------------------------
@pytest.mark.parametrize("N,K,store", [(N, K, st) for K, N, st in sorted(gc.CHAIN_SHAPES, key=lambda k: (k[1], k[0], k[2]))],
                         ids=lambda v: str(int(v)))
def test_x3_chain_walk(lib, device, N, K, store):
    M = gc.X3R_M
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert gc.cdiv(M, 32) > 2 * 8 * cus                  # every wave of THIS device walks three tiles or more
    raw, full = gc.chain_cases(K, N, store)
    check_chain(lib, device, gc.build(raw))
    c = gc.build(full)
    for m_dev in gc.X3R_MDEV:
        check_chain(lib, device, c, None if m_dev == M else m_dev)


@pytest.mark.parametrize("s", gc.chain_extra_cases(), ids=gc.case_id)
def test_x3_chain_more(lib, device, s):
    c = gc.build(s)
    check_chain(lib, device, c)
    if s["id"] == "ldc2-32":
        assert s["ldc2_pad"] == 0
        check_chain(lib, device, c, 65535)


@pytest.mark.parametrize("store", (0, 1))
@pytest.mark.parametrize("N", (64, 128))
def test_x3_chain_lds_boundary(lib, device, N, store):
    """the largest K the restated LDS formula admits is launched, the next one is refused with nothing written, and the router's
    predicate draws the same line wherever d3f_gemm_x3 has a resident form (the walk test runs the image at that K)"""
    Kmax = gc.chain_largest_k(N, store)
    assert (Kmax, N, bool(store)) in gc.CHAIN_SHAPES
    M, D3F_OK, D3F_ERR_ARG = 70, 0, -3
    for K in (Kmax, Kmax + 32):
        A = torch.zeros((M, K), device=device)
        wx = torch.zeros(int(lib.d3f_gemm_x3_packed_bytes(K, N)), dtype=torch.uint8, device=device)
        w2x = torch.zeros(int(lib.d3f_gemm_x3_packed_bytes(N, 32)), dtype=torch.uint8, device=device)
        first = torch.full((M + gc.PAD, N), float(gc.SENT), device=device)
        out2 = torch.full((M + gc.PAD, 32), float(gc.SENT), device=device)
        rc = lib.d3f_gemm_x3_chain(A.data_ptr(), M, K, K, None, 1, None, 0, 0, wx.data_ptr(), first.data_ptr() if store else None, N, M, N,
                                   None, None, None, None, 0, 0, 0.25, w2x.data_ptr(), None, None, 0, 0.25, out2.data_ptr(), 32, None, None, None)
        torch.cuda.synchronize()
        if K == Kmax:
            assert rc == D3F_OK
            assert bool((out2[:M] == 0).all()) and bool((out2[M:] == float(gc.SENT)).all())
            assert bool((first[:M] == 0).all()) == bool(store) and bool((first[M:] == float(gc.SENT)).all())
        else:
            assert rc == D3F_ERR_ARG
            assert bool((out2 == float(gc.SENT)).all()) and bool((first == float(gc.SENT)).all())
    seen = 0
    for K in range(32, Kmax + 97, 32):
        if lib.d3f_gemm_x3_resident(100000, N, K, 0):
            assert lib.d3f_gemm_x3_chain_ok(100000, N, K, store, 0) == int(K <= Kmax) == gc.gemm_x3_chain_ok(100000, N, K, store)
            seen += 1
        else:
            assert lib.d3f_gemm_x3_chain_ok(100000, N, K, store, 0) == 0
    assert seen >= 3


@pytest.mark.parametrize("s", gc.gres_cases(), ids=gc.case_id)
def test_x3_gathered_residual(lib, device, s):
    c = check_twice_if_split(lib, device, s)
    for m_dev in (0, 129):
        check(lib, device, c, m_dev)


def test_upsample_split_router(device):
    """ops.gemm_upsample_split: Y = x @ W1 over the coarse rows, then act(skip @ W2 + shift + Y[inds[:, 0]]) through d3f_gemm_x3_gres;
    the expectation is the one-launch operator's (integers: the two forms are the same sums)"""
    from d3feat_amd import ops
    s = gc.spec("x3", 200, 64, 64, C2=96, gather=True, n1=150, ld_idx=3, col=True, no_cs=True, leaky=True,
                intent=dict(kernel="gemm_x3_kernel<2,4>", S=1, tiles=(5,)), id="split-router")
    c = gc.build(s)
    assert c["cs"] is None and c["exact"] and gc.tile_statements(c) == (True, True)
    u = ops.UpsampleCat(_up(c["x"], device), _up(c["idx"], device), _up(c["skip"], device))
    assert ops.upsample_split_ok(u, 64)
    W = _up(c["W"], device)
    buf = torch.full((200 + gc.PAD, 64), float(gc.SENT), dtype=torch.float32, device=device)
    got = ops.gemm_upsample_split(u, W[:64].contiguous(), W[64:].contiguous(), col_shift=_up(c["ch"], device), leaky=True, alpha=0.25,
                                  out=buf[:200])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(buf.cpu().numpy(), gc.expected_buffer(c))


# ---- gemm_dma_kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted(gc.DMA_SLICES))
@pytest.mark.parametrize("N", gc.DMA_N)
def test_dma_ring(lib, device, N, K):
    cases = gc.dma_cases(N, K)
    assert [s["epi"] for s in cases] == [0, 1, 2, 3]
    for s in cases:
        check_twice_if_split(lib, device, s)


@pytest.mark.parametrize("s", gc.dma_extra_cases(), ids=gc.case_id)
def test_dma_more(lib, device, s):
    check_twice_if_split(lib, device, s)


@pytest.mark.parametrize("K", (36, 160, 544))
@pytest.mark.parametrize("N", (32, 68))
def test_dma_row_counts(lib, device, N, K):
    c = gc.build(gc.dma_cases(N, K)[3])
    for m_dev in gc.DMA_MDEV:
        check(lib, device, c, m_dev)


# ---- gemm_fast_kernel, gemm_f32_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", gc.f32_cases(), ids=gc.case_id)
def test_f32_entries(lib, device, s):
    check_twice_if_split(lib, device, s)


@pytest.mark.parametrize("K", (96, 544))
@pytest.mark.parametrize("N", (32, 68))
@pytest.mark.parametrize("kind", ("fast", "generic"))
def test_f32_row_counts(lib, device, kind, N, K):
    tag = "fast-N%d-K%d-epi3" % (N, K) if kind == "fast" else "generic-lda-N%d-K%d" % (N, K)
    s, = [s for s in gc.f32_cases() if s["id"] == tag]
    c = gc.build(s)
    for m_dev in gc.F32_MDEV:
        check(lib, device, c, m_dev)


# ---- gemm_bf16_kernel --------------------------------------------------------------------------------------------------------------
def _bf16_view(a, pad, dev, off=4):
    """float32 values exact in bfloat16 -> a torch.bfloat16 [rows, w] view (leading dimension w + pad, base 8 bytes into its buffer)"""
    flat, ld = gc.widen(a, pad, off=off)
    t = _up(gc.bf16_bits(flat).view(np.int16), dev).view(torch.bfloat16)
    return t[off:].view(a.shape[0], ld)[:, :a.shape[1]]


def _through_ops(dev, c, m_dev):
    """the same case through the Python router: bfloat16 (or, a_bf16 = 0, float32) tensors under ops.bf16_contraction"""
    from d3feat_amd import ops
    s = c["spec"]
    M, N, a, cb = s["M"], s["N"], s["a_bf16"], s["c_bf16"]
    o = gc.poisoned(c, m_dev)
    feat = (lambda v, pad: _bf16_view(v, pad, dev)) if a else (lambda v, pad: _up(gc.widen(v, pad)[0], dev).view(v.shape[0], -1)[:, :v.shape[1]])
    vec = lambda v: None if v is None else _up(v, dev)
    W = _up(c["W"], dev)
    count = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=dev)
    kw = dict(col_scale=vec(c["cs"]), col_shift=vec(c["ch"]), leaky=bool(s["leaky"]), alpha=float(s["alpha"]))
    import contextlib
    with ops.bf16_contraction(features=bool(a)), (ops.f32_output() if (a and not cb) else contextlib.nullcontext()):
        assert ops._out_dtype() == (torch.bfloat16 if cb else torch.float32)
        if s["id"] in ("raw", "full"):
            A = feat(o["x"], 4)
            if count is not None:
                A.n_dev = count
            sent = torch.full((M + gc.PAD, N), float(gc.SENT), dtype=torch.float32, device=dev)
            buf = sent.to(torch.bfloat16) if cb else sent
            res = None if o["res"] is None else feat(o["res"], 4 + (-N) % 4)     # (the router wants ldr % 4 == 0)
            ops.gemm(A, W, row_scale=vec(o["rs"]), residual=res, out=buf[:M], **kw)
            got = buf
        else:
            x, skip = feat(o["x"], 4), feat(o["skip"], 4)
            if s["id"] == "upcat":
                idx = _up(o["idx"], dev)
                x.n_dev = torch.tensor([c["n1_dev"]], dtype=torch.int32, device=dev)
                if count is not None:
                    idx.n_dev = count
                got = ops.gemm_upsample_cat(ops.UpsampleCat(x, idx, skip), W, **kw)
            else:
                if count is not None:
                    x.n_dev = count
                got = ops.gemm_cat2(x, skip, W, **kw)
    torch.cuda.synchronize()
    assert got.dtype == (torch.bfloat16 if cb else torch.float32)
    got = got.view(torch.int16).cpu().numpy().view(np.uint16) if cb else got.cpu().numpy()
    m = M if m_dev is None else m_dev
    want = gc.expected_buffer(c, m_dev)
    if got.shape[0] == M:                               # (an output the router allocated: rows from *M_dev on are not defined)
        assert np.array_equal(got[:m], want[:m]), gc.case_id(s)
    else:
        assert np.array_equal(got, want), gc.case_id(s)


@pytest.mark.parametrize("N", gc.BF16_N)
@pytest.mark.parametrize("K", sorted(gc.BF16_SLICES))
@pytest.mark.parametrize("M", gc.BF16_M)
def test_bf16_kernels(lib, device, M, K, N):
    for a in (0, 1):
        for cb in (0, 1):
            for s in gc.bf16_cases(M, K, N, a, cb):
                c = check_twice_if_split(lib, device, s)
                check(lib, device, c, 65)
                if (a, cb) != (0, 1):                   # (float32 features with a bfloat16 output: no such mode in the router)
                    _through_ops(device, c, None)
                    _through_ops(device, c, 65)
