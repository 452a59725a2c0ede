"""TEST INFRASTRUCTURE ONLY.  Seeded operands and integer / float64 expectations for the branch tests of the contraction family
(tests/test_gpu_gemm_branches.py on the GPU, tests/test_gemm_cases.py on the CPU): d3f_gemm_f32, d3f_gemm_upsample_cat_f32,
d3f_gemm_f32t, d3f_gemm_bf16, d3f_gemm_x3, d3f_gemm_x3_gres, d3f_gemm_x3_chain and the four pack entry points (csrc/gemm_f32.hip,
gemm_dma.h, gemm_x3.h, gemm_common.h).  numpy only; no kernel has a part in any expectation, and NO TOLERANCE exists anywhere: the operands are chosen so
that fp32 arithmetic is exact, whatever the order of the sums.

  lattice   A, skip, x, W and the residual hold small integers, row_scale / col_scale come from {0.5, 1, 2, 4}, col_shift holds
            integers and halves, alpha is 0.25 (one case per family: 0.2, one fp32 multiply of an exact value).  ranges() budgets the
            magnitudes per K so that max(|A| @ |W|) < 2^24 (raw) -- every product of the x3 planes, every partial sum in every order is
            exact -- and so that every intermediate of the epilogue is a multiple of 1/4 below 2^22, i.e. an FMA-contracted epilogue
            and a separately rounded one agree.  The expectation is computed in float64 on integers (exact) and cast.
  select    W is a 0/1 selection matrix, A holds full 24-bit mantissas over 2^+-20: every output is ONE operand (fp32 kernels only).
  bf16      operands |v| <= 127 (exact in bfloat16); a bf16 output is the round-to-nearest-even of the exact value, and every such
            case carries planted outputs 257 (a tie that rounds DOWN to even), 259 (a tie that rounds UP to even) and 515 (no tie,
            rounding differs from truncation).
  leaky     every 32 x 32 output tile holds both signs and exact zeros (a zero column of W per column group whose shift is zero; a
            group of one column copies column 0 of the operand, zero in every third row).
  chain     d3f_gemm_x3_chain: a first-level case (built by the x3 builder itself: its expectation IS the x3 expectation) and on top
            of it W2 f32[N, 32] in small integers with one zero column, cs2 from {0.5, 1, 2, 4}, ch2 in integers and halves,
            want2 = act2((Y @ W2) cs2 + ch2) in float64 from the exact first output Y.  |A| <= 3, |W| <= 2, |W2| <= 2 (CHAIN_RANGES):
            the first-level budget of ranges() is for ONE product.  Exactness of the second level is COMPUTED and recorded (exact2):
            with u the finest power of two that divides every Y, max(|Y| @ |W2|) / u < 2^24, and every intermediate of the second
            epilogue equals its own float32 rounding.  select2: W and W2 both 0/1 selections, identity epilogues -- every element
            of the second output is one full-mantissa operand of A, which holds only if the finished value is split into three
            planes without loss and the W2 image's k order is the kernel's.
  poison    poisoned() writes NaN / Inf into every float the contract says is not read: rows of A / skip / residual / row_scale past
            *M_dev, rows of x past *N1_dev, rows of a gathered residual past *res_rows_dev, the columns between the rows of every
            operand whose leading dimension exceeds its width.  Outputs are PAD rows longer than documented, ldc = N + 4 where the
            case says so, pre-filled with SENT.

The host plans are restated below (gemm_plan, gemm_bf16_split, gemm_x3_cost / gemm_x3_plan, gemm_x3_resident,
gemm_x3r_chain_lds_bytes / gemm_x3_chain_ok); every case records the branch it MEANS to exercise (kernel instance, S, k-tiles of
every slice -- written down from the shape tables, not computed by the restatement) and tests/test_gemm_cases.py checks that the
restatement, and where it is built the library, agree."""
import numpy as np

SENT = np.float32(-7.25e9)
SENT_H = np.uint16(0xCFD8)                # the same for a bfloat16 output buffer (-7.25e9 truncated)
PAD = 5                                   # rows every output buffer is longer than its documented extent
GX_BK = 32
X3_CHUNK_BYTES = 7680


def cdiv(a, b):
    return -(-a // b)


# ---- the host plans, restated -------------------------------------------------------------------------------------------------------
def gemm_plan(M, N, K, hint=0):
    """-> (bm, bn, S, tps) of gemm_run / d3f_gemm_f32t (csrc/gemm_common.h)"""
    if 0 < hint < M:
        M = hint
    bm, bn = (128, 32) if N <= 32 else (64, 64)
    blocks, nt, S = cdiv(M, bm) * cdiv(N, bn), cdiv(K, 32), 1
    if blocks < 768 and nt > 16:
        S = max(1, min(cdiv(1536, blocks), nt // 8, 64))
    tps = cdiv(nt, S)
    return bm, bn, cdiv(nt, tps), tps


def gemm_bf16_split(M, N, K, hint=0):
    """-> (S, tps) of d3f_gemm_bf16: the fp32 plan of a 64-column tile"""
    _, _, S, _ = gemm_plan(M, N if N > 32 else 64, K, hint)
    nt = cdiv(K, 32)
    tps = cdiv(nt, min(S, nt))
    return cdiv(nt, tps), tps


def gemm_x3_cost(blocks, slots, nt, per):
    best, S, s = -1, 1, 1
    while s <= 64 and s * 4 <= nt:
        t = cdiv(nt, s)
        if cdiv(nt, t) == s:
            cost = cdiv(blocks * s, slots) * (t + 12) * per + (200 * s if s > 1 else 0)
            if best < 0 or cost < best:
                best, S = cost, s
        s += 1
    if best < 0:
        best = cdiv(blocks, slots) * (nt + 12) * per
    return best, S


def gemm_x3_plan(M, N, K, hint=0):
    """-> (tn, waves, S, tps) of the tile form of d3f_gemm_x3"""
    if 0 < hint < M:
        M = hint
    nt = K // GX_BK
    tn, waves = (1 if N <= 32 else 2), 4
    c_small, S = gemm_x3_cost(cdiv(M, 128) * cdiv(N, 32 * tn), 512, nt, 100)
    if N >= 128:
        c_big, s_big = gemm_x3_cost(cdiv(M, 256) * cdiv(N, 128), 256, nt, 163)
        if c_big < c_small:
            tn, waves, S = 4, 8, s_big
    tps = cdiv(nt, S)
    return tn, waves, cdiv(nt, tps), tps


def gemm_x3_resident(M, N, K, hint=0):
    if N < 1 or K < GX_BK or K % GX_BK:
        return 0
    NG, m_eff = cdiv(N, 32), (hint if 0 < hint < M else M)
    lds = (K // GX_BK) * NG * X3_CHUNK_BYTES + 8 * 32 * 36 * 4 + 2 * 128 * 4
    return int(NG in (1, 2, 4) and lds <= 160 * 1024 and m_eff >= 65536)


LDS_LIMIT = 160 * 1024


def gemm_x3r_chain_lds_bytes(nkt, NG, store_first):
    """LDS of gemm_x3r_chain_kernel: W, the W2 image (one k-tile per column group), the eight output patches when the first output
    is stored, both epilogues' vectors"""
    return (nkt + 1) * NG * X3_CHUNK_BYTES + (8 * 32 * 36 * 4 if store_first else 0) + 2 * 128 * 4 + 2 * 32 * 4


def gemm_x3_chain_accepts(N, K, store_first):
    """what the entry point d3f_gemm_x3_chain launches (whatever M is)"""
    return int(N in (64, 128) and K >= GX_BK and K % GX_BK == 0 and gemm_x3r_chain_lds_bytes(K // GX_BK, N // 32, store_first) <= LDS_LIMIT)


def gemm_x3_chain_ok(M, N, K, store_first, hint=0):
    """d3f_gemm_x3_chain_ok: the router's predicate -- the call is one of d3f_gemm_x3's resident form AND the chained image fits"""
    return int(bool(gemm_x3_resident(M, N, K, hint)) and bool(gemm_x3_chain_accepts(N, K, store_first)))


def chain_largest_k(N, store_first):
    """the largest K whose chained LDS image fits, from the formula"""
    K = GX_BK
    while gemm_x3r_chain_lds_bytes(K // GX_BK + 1, N // 32, store_first) <= LDS_LIMIT:
        K += GX_BK
    return K


# the four instances, written down: (N, first output stored) -> kernel
CHAIN_KERNELS = {(64, False): "gemm_x3r_chain_kernel<2,false>", (64, True): "gemm_x3r_chain_kernel<2,true>",
                 (128, False): "gemm_x3r_chain_kernel<4,false>", (128, True): "gemm_x3r_chain_kernel<4,true>"}


def chain_kernel(N, store_first):
    return CHAIN_KERNELS[(N, bool(store_first))]


def slab_bytes(S, M, N):
    """what a *_workspace_bytes function answers for S slices"""
    return (S * M * N * 4 + 255) // 256 * 256 + 256 if S > 1 else 256


def slices(nt, tps):
    """k-tiles of every K slice"""
    return tuple(min(tps, nt - t) for t in range(0, nt, tps))


def planned_branch(spec):
    """(kernel instance, S, k-tiles per slice) the restated plans give for a case"""
    e, M, N, K, hint = spec["entry"], spec["M"], spec["N"], spec["C1"] + spec["C2"], spec.get("hint", 0)
    if e == "chain":
        if not gemm_x3_chain_accepts(N, K, spec["store"]):
            return None, 0, ()
        return "gemm_x3r_chain_kernel<%d,%s>" % (N // 32, "true" if spec["store"] else "false"), 1, (K // 32,)
    if e in ("x3", "x3_gres"):
        if e == "x3" and gemm_x3_resident(M, N, K, hint):
            return "gemm_x3r_kernel<%d>" % cdiv(N, 32), 1, (K // 32,)
        tn, waves, S, tps = gemm_x3_plan(M, N, K, hint)
        return "gemm_x3_kernel<%d,%d>" % (tn, waves), S, slices(K // 32, tps)
    if e == "bf16":
        S, tps = gemm_bf16_split(M, N, K, hint)
        return "gemm_bf16_kernel<%d,%d>" % (spec["a_bf16"], spec["c_bf16"]), S, slices(cdiv(K, 32), tps)
    bm, bn, S, tps = gemm_plan(M, N, max(K, 1), hint)
    shape = "4,1" if bn == 32 else "2,2"
    sl = slices(cdiv(K, 32), tps) if K else (0,)
    if e == "f32t":
        return "gemm_dma_kernel<%s,%d>" % (shape, spec["epi"] & 3), S, sl
    if spec_is_fast(spec):
        return "gemm_fast_kernel<%s,%d>" % (shape, spec["epi"] & 3), S, sl
    return "gemm_f32_kernel<%s>" % shape, S, sl


def spec_is_fast(spec):
    """gemm_run's `fast` predicate, from the layout a case asks for (every buffer a case hands over is 16-byte aligned but for the
    offsets it names)"""
    K, N = spec["C1"] + spec["C2"], spec["N"]
    odd = [spec.get(k, 0) % 4 for k in ("lda_pad", "ldb_pad", "ldc_pad", "a_off", "b_off")]
    return K % 4 == 0 and N % 4 == 0 and not any(odd) and (not spec["C2"] or spec["C1"] % 4 == 0)


# ---- number formats -------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 values that ARE bfloat16 values -> their uint16 storage"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not exact in bfloat16"
    return (u >> 16).astype(np.uint16)


def bf16_rne(a):
    """float32 -> bfloat16 storage, round to nearest, ties to even: the nearer of the two neighbouring bfloat16 values, decided in
    float64 (finite inputs)"""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32)
    lo = u & np.uint32(0xFFFF0000)                      # towards zero
    hi = lo + np.uint32(0x10000)                        # away from zero (finite inputs far from FLT_MAX)
    dlo = np.abs(a.astype(np.float64) - lo.view(np.float32).astype(np.float64))
    dhi = np.abs(hi.view(np.float32).astype(np.float64) - a.astype(np.float64))
    even_lo = ((lo >> 16) & 1) == 0
    pick_lo = (dlo < dhi) | ((dlo == dhi) & even_lo)
    return (np.where(pick_lo, lo, hi) >> 16).astype(np.uint16)


def bf16_f32(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rounding_kinds(t32):
    """of exact float32 outputs: (RNE differs from truncation and is no tie, tie that rounds down to even, tie that rounds up)"""
    u = np.ascontiguousarray(t32, np.float32).view(np.uint32)
    low, odd = u & 0xFFFF, ((u >> 16) & 1) == 1
    return (low > 0x8000), (low == 0x8000) & ~odd, (low == 0x8000) & odd


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def ranges(K, epilogue, bf16):
    """(amax, wmax) of a lattice case: K amax wmax < 2^24 raw; with an epilogue 16 K amax wmax + 2 * 128 + 64 < 2^22, so that every
    intermediate (a multiple of 1/4) has 24 significant bits at most"""
    K = max(K, 1)
    wmax = 15 if epilogue else (31 if K <= 128 else 63)
    budget = (1 << 18) - 64 if epilogue else (1 << 24) - 1
    amax = min(4095, budget // (K * wmax))
    if bf16:
        amax, wmax = min(amax, 127), min(wmax, 127)
    return int(amax), int(wmax)


def zero_columns(N):
    """one column per 32-column group: W and the shift are zero there"""
    return [32 * g + min(5, min(32, N - 32 * g) - 1) for g in range(cdiv(N, 32))]


SPEC_DEFAULTS = dict(C2=0, gather=False, ld_idx=1, n1=0, epi=0, col=False, leaky=False, alpha=0.25, kind="lattice", hint=0,
                     lda_pad=0, lds_pad=0, ldb_pad=0, ldc_pad=0, ldr_pad=0, a_off=0, b_off=0, a_bf16=0, c_bf16=0,
                     gres=False, ld_res_idx=1, res_rows=0, seed=0, amax=0, wmax=0,
                     store=False, cs2=False, ch2=False, leaky2=False, alpha2=0.25, ldc2_pad=4, w2="lattice", w2max=2)


def spec(entry, M, N, C1, **kw):
    s = dict(SPEC_DEFAULTS, entry=entry, M=M, N=N, C1=C1)
    s.update(kw)
    if s["epi"] or s["leaky"]:
        s["col"] = True
    return s


def shadow_indices(rng, M, n1, n1_dev, ld):
    """gather indices i32[M, ld]: column 0 is used.  Valid rows, and in known places every kind of shadow: -1, a large negative one,
    n1, n1 + 3 and (n1_dev < n1) rows between *N1_dev and N1"""
    live = n1_dev if n1_dev is not None else n1
    idx = rng.integers(-7, 2 ** 20, (M, ld)).astype(np.int32)        # columns past the first: garbage nobody may use
    idx[:, 0] = rng.integers(0, max(live, 1), M)
    sh = [-1, -2 ** 31, n1, n1 + 3] + ([live, n1 - 1] if live < n1 else [])
    for j, v in enumerate(sh):
        idx[3 + 7 * j:M:41, 0] = v
    return idx


def build(s):
    """-> the case of a spec: clean operands (no poison), the expectation and its pre-activation value.
    Effective operand: Aeff[m] = [ x'[idx[m, 0]] (x[m] without a gather) | skip[m] ]; t = (Aeff @ W) rs cs + ch + res; out = act(t)."""
    if s["entry"] == "chain":
        return build_chain(s)
    M, N, C1, C2 = s["M"], s["N"], s["C1"], s["C2"]
    K = C1 + C2
    rng = np.random.default_rng([s["seed"], M, N, C1, C2, s["epi"], len(s["entry"])])
    bf = s["entry"] == "bf16"
    epilogue = bool(s["col"] or s["epi"] or s["leaky"])
    amax, wmax = ranges(K, epilogue, bf)
    if s["amax"]:                                       # (a case that budgets its own magnitudes: the chained ones)
        assert s["amax"] <= amax and s["wmax"] <= wmax
        amax, wmax = s["amax"], s["wmax"]
    c = dict(spec=s, K=K, amax=amax, wmax=wmax)
    n1 = s["n1"] if s["gather"] else M
    n1_dev = s.get("n1_dev")
    if s["kind"] == "select":
        x = (rng.standard_normal((n1, C1)) * np.exp(rng.uniform(-20, 20, (n1, C1)))).astype(np.float32)
        skip = (rng.standard_normal((M, C2)) * np.exp(rng.uniform(-20, 20, (M, C2)))).astype(np.float32) if C2 else None
        sel = rng.integers(0, K, N)
        W = np.zeros((K, N), np.float32)
        W[sel, np.arange(N)] = 1.0
    else:
        x = rng.integers(-amax, amax + 1, (n1, C1)).astype(np.float32)
        skip = rng.integers(-amax, amax + 1, (M, C2)).astype(np.float32) if C2 else None
        W = rng.integers(-wmax, wmax + 1, (K, N)).astype(np.float32)
    idx = shadow_indices(rng, M, n1, n1_dev, s["ld_idx"]) if s["gather"] else None
    rs = rng.choice([0.5, 1.0, 2.0, 4.0], M).astype(np.float32) if s["epi"] & 1 else None
    cs = rng.choice([0.5, 1.0, 2.0, 4.0], N).astype(np.float32) if s["col"] and not s.get("no_cs") else None
    ch = (rng.integers(-255, 256, N) * 0.5).astype(np.float32) if s["col"] else None
    res = ridx = None
    rrows = (s["res_rows"] if s["gres"] else M)
    if s["epi"] & 2:
        res = rng.integers(-100, 101, (rrows, N)).astype(np.float32)
        if s["gres"]:
            ridx = shadow_indices(rng, M, rrows, s.get("res_rows_dev"), s["ld_res_idx"])
    zc = zero_columns(N)
    if s["kind"] == "lattice":
        W[:, zc] = 0.0
        if N % 32 == 1 and K:
            # a column group of ONE column cannot be all zero and hold both signs: it copies column 0 of the operand instead, which
            # is 0, +3, -3 by row modulo three (a gathered row m reads a row of x with the same remainder)
            W[0, N - 1] = 1.0
            x[:, 0] = np.array([0.0, 3.0, -3.0], np.float32)[np.arange(len(x)) % 3]
            if idx is not None:
                live_ = n1_dev if n1_dev is not None else n1
                ok = (idx[:, 0] >= 0) & (idx[:, 0] < live_)
                r = idx[:, 0] // 3 * 3 + np.arange(M) % 3
                r = np.where(r >= live_, r - 3, r)
                idx[:, 0] = np.where(ok, r, idx[:, 0])
            if res is not None:
                res[:, N - 1] = 0.0
        if ch is not None:
            ch[zc] = 0.0
        if res is not None:
            res[::2, zc] = 0.0
    # planted bfloat16 rounding cases: rows 2, 35 and M - 1 of Aeff are 4 a0 + a1 in column nstar
    planted = []
    if s["c_bf16"]:
        nstar = max(n for n in range(N) if n not in zc)
        W[0, nstar], W[1, nstar] = 4.0, 1.0
        for j, (m, a0, a1) in enumerate(((2, 64, 1), (35, 64, 3), (M - 1, 127, 7))):
            r = m
            if idx is not None:
                r = j                                   # a reserved row of x
                idx[m, 0] = r
            x[r] = 0.0
            if C1 >= 2:
                x[r, 0], x[r, 1] = a0, a1
            else:
                raise ValueError("planting needs C1 >= 2")
            if skip is not None:
                skip[m] = 0.0
            if rs is not None:
                rs[m] = 1.0
            if res is not None:
                res[m, nstar] = 0.0
            planted.append((m, nstar, 4 * a0 + a1))
        if cs is not None:
            cs[nstar] = 1.0
        if ch is not None:
            ch[nstar] = 0.0
    # ---- the expectation: float64 on integers (lattice) is exact; a selection picks one operand
    live = n1_dev if n1_dev is not None else n1
    W64 = W.astype(np.float64)
    if K == 0:
        acc, bound = np.zeros((M, N)), np.zeros((M, N))
    else:
        def part(op, Wp, rows=None):
            y = op.astype(np.float64) @ Wp
            if rows is None:
                return y
            ok = (rows >= 0) & (rows < live)
            return np.where(ok[:, None], y[np.where(ok, rows, 0)], 0.0)
        rows = idx[:, 0].astype(np.int64) if idx is not None else None
        with np.errstate(over="ignore", invalid="ignore"):
            acc = part(x, W64[:C1], rows)
            bound = part(np.abs(x), np.abs(W64[:C1]), rows)
            if C2:
                acc = acc + part(skip, W64[C1:])
                bound = bound + part(np.abs(skip), np.abs(W64[C1:]))
    if s["kind"] == "select":
        # one operand per output: taken, not summed (float64 sums of 2^+-20 values would still be exact, but say it directly)
        xz = np.concatenate([x, np.zeros((1, C1), np.float32)])
        g = xz[np.where((rows >= 0) & (rows < live), rows, n1)] if idx is not None else x[:M]
        full = np.concatenate([g, skip], 1) if C2 else g
        acc = full[:, sel].astype(np.float64)
    # every intermediate of the epilogue, in the kernels' order, must be its own float32 rounding (checked as it is made: the
    # large cases would not want five float64 copies kept)
    def is32(v):
        return bool((v.astype(np.float32).astype(np.float64) == v).all())
    t = acc
    exact = is32(t)
    if rs is not None:
        t = t * rs.astype(np.float64)[:, None]
        exact = exact and is32(t)
    if cs is not None:
        t = t * cs.astype(np.float64)
        exact = exact and is32(t)
    if ch is not None:
        t = t + ch.astype(np.float64)
        exact = exact and is32(t)
    if res is not None:
        if ridx is not None:
            rl = s.get("res_rows_dev")
            rl = rrows if rl is None else rl
            rr = ridx[:, 0].astype(np.int64)
            ok = (rr >= 0) & (rr < rl)
            radd = np.where(ok[:, None], res[np.where(ok, rr, 0)], np.float32(0)).astype(np.float64)
        else:
            radd = res.astype(np.float64)
        t = t + radd
        exact = exact and is32(t)
    out = t.astype(np.float32)
    if s["leaky"]:
        neg = np.float32(out) * np.float32(s["alpha"])  # ONE fp32 multiply of the exact pre-activation value
        out = np.where(t > 0, out, neg).astype(np.float32)
    c.update(x=x, idx=idx, skip=skip, W=W, rs=rs, cs=cs, ch=ch, res=res, ridx=ridx, n1=n1, n1_dev=n1_dev, rrows=rrows,
             bound=bound, exact=exact, pre=t, planted=planted, zero_cols=zc,
             want=bf16_rne(out) if s["c_bf16"] else out)
    return c


def first_level_spec(s):
    """the d3f_gemm_x3 case with the first-level operands of a chained case (the resident walk takes it wherever M >= 65536)"""
    return dict(s, entry="x3", kind="select" if s["kind"] == "select2" else s["kind"], intent=None, hint=0)


def lattice_unit(v, finest=12):
    """the largest 2^-k (k = 0 .. finest) of which every element of v is an integer multiple; None: there is none"""
    q = v * float(1 << finest)
    n = q.astype(np.int64)
    if not (n == q).all():
        return None
    bits = int(np.bitwise_or.reduce(np.abs(n), axis=None))
    low = (bits & -bits).bit_length() - 1 if bits else finest          # the lowest bit set anywhere
    return 2.0 ** (min(low, finest) - finest)


def build_chain(s):
    """-> the case of a `chain` spec: the first-level case as build() makes it for d3f_gemm_x3 (c["first"]; every key of it is here
    too, want = Y), and on top W2, cs2, ch2, pre2, want2 = act2((Y @ W2) cs2 + ch2), exact2, unit2 (the lattice unit u of Y),
    bound2 (max(|Y| @ |W2|) / u)"""
    f = build(first_level_spec(s))
    M, N = s["M"], s["N"]
    rng = np.random.default_rng([s["seed"], M, N, s["C1"], s["C2"], s["epi"], 1 + 2 * s["cs2"] + 4 * s["ch2"], 77])
    Y = f["want"].astype(np.float64)                    # the exact first output
    zc2 = zero_columns(32)
    sel2 = None
    if s["kind"] == "select2" or s["w2"] == "select":
        sel2 = rng.integers(0, N, 32)
        W2 = np.zeros((N, 32), np.float32)
        W2[sel2, np.arange(32)] = 1.0
    else:
        W2 = rng.integers(-s["w2max"], s["w2max"] + 1, (N, 32)).astype(np.float32)
    cs2 = rng.choice([0.5, 1.0, 2.0, 4.0], 32).astype(np.float32) if s["cs2"] else None
    ch2 = (rng.integers(-255, 256, 32) * 0.5).astype(np.float32) if s["ch2"] else None
    if s["kind"] != "select2":
        W2[:, zc2] = 0.0
        if ch2 is not None:
            ch2[zc2] = 0.0

    def is32(v):
        return bool((v.astype(np.float32).astype(np.float64) == v).all())
    unit2 = bound2 = None
    if sel2 is not None:
        # one operand per output, taken: the three planes of a value add up to it in the kernel's order (smallest first), the other
        # 32 TN - 1 products of the sum are zeros
        t = np.where((W2 != 0).any(0), Y[:, sel2], 0.0)
        exact2 = f["exact"]
    else:
        t = Y @ W2.astype(np.float64)
        unit2 = lattice_unit(Y)
        bound2 = float((np.abs(Y) @ np.abs(W2).astype(np.float64)).max() / unit2) if unit2 else None
        exact2 = bool(f["exact"] and unit2 and bound2 < 2 ** 24 and is32(t))
    if cs2 is not None:
        t = t * cs2.astype(np.float64)
        exact2 = exact2 and is32(t)
    if ch2 is not None:
        t = t + ch2.astype(np.float64)
        exact2 = exact2 and is32(t)
    out2 = t.astype(np.float32)
    if s["leaky2"]:
        out2 = np.where(t > 0, out2, np.float32(out2) * np.float32(s["alpha2"])).astype(np.float32)
    c = dict(f, spec=s, first=f, W2=W2, cs2=cs2, ch2=ch2, sel2=sel2, pre2=t, want2=out2, exact2=bool(exact2), unit2=unit2,
             bound2=bound2, zero_cols2=zc2)
    return c


# ---- poison and buffers ---------------------------------------------------------------------------------------------------------------
def widen(a, pad, rows_extra=0, off=0, fill=np.nan):
    """[rows, w] -> flat buffer of `off` + (rows + rows_extra) x (w + pad) floats, everything that is not the matrix filled with
    `fill`; -> (flat buffer, leading dimension).  The matrix starts `off` elements into the buffer."""
    r, w = a.shape
    buf = np.full((r + rows_extra, w + pad), fill, a.dtype)
    buf[:r, :w] = a
    flat = np.concatenate([np.full(off, fill, a.dtype), buf.ravel()])
    return flat, w + pad


def poisoned(c, m_dev=None):
    """copies of the operands of case c with NaN / Inf in every float that a call with *M_dev = m_dev (None: M) may not read; the
    rows of x past *N1_dev and of a gathered residual past *res_rows_dev are poisoned whenever the case sets those counts"""
    s = c["spec"]
    M = s["M"]
    m = M if m_dev is None else min(m_dev, M)
    o = {k: (None if c[k] is None else c[k].copy()) for k in ("x", "skip", "rs", "res", "idx", "ridx")}
    bad = np.array([np.nan, np.inf, -np.inf, np.nan], np.float32)

    def rows_from(a, r0):
        if a is not None and r0 < len(a):
            flat = a[r0:].reshape(-1)                   # (a view: the operands are contiguous) bad, repeated in flat order
            flat[:] = np.tile(bad, cdiv(flat.size, len(bad)))[:flat.size]
    if s["gather"]:
        if c["n1_dev"] is not None:
            rows_from(o["x"], c["n1_dev"])
        if o["idx"] is not None:
            o["idx"][m:] = -1                           # (indices past *M_dev are not read; -1 keeps a wrong read harmless)
    else:
        rows_from(o["x"], m)
    rows_from(o["skip"], m)
    rows_from(o["rs"], m)
    if s["gres"]:
        if s.get("res_rows_dev") is not None:
            rows_from(o["res"], s["res_rows_dev"])
        if o["ridx"] is not None:
            o["ridx"][m:] = -1
    else:
        rows_from(o["res"], m)
    if s["entry"] == "chain":
        # nothing of the second level depends on a row; W2 goes to d3f_gemm_pack_x3_chain as a column view of a wider matrix
        o["W2"], o["ldb2"] = widen(c["W2"], 4)
    return o


def expected_buffer(c, m_dev=None, second=False):
    """the whole output buffer [M + PAD, ldc] after the call: rows below *M_dev hold the expectation, every other element the sentinel.
    second: the 32-column output of a chained case, [M + PAD, 32 + ldc2_pad]"""
    s = c["spec"]
    M, N = s["M"], s["N"]
    m = M if m_dev is None else min(m_dev, M)
    if second:
        buf = np.full((M + PAD, 32 + s["ldc2_pad"]), SENT, np.float32)
        buf[:m, :32] = c["want2"][:m]
        return buf
    sent = SENT_H if s["c_bf16"] else SENT
    buf = np.full((M + PAD, N + s["ldc_pad"]), sent, c["want"].dtype)
    buf[:m, :N] = c["want"][:m]
    return buf


def tile_statements(c, key="pre"):
    """leaky coverage of a case: (every 32 x 32 output tile of three rows or more holds a positive, a negative and an exactly zero
    pre-activation value, the last (ragged) tile holds a negative one).  key = "pre2": of the second output of a chained case"""
    t = c[key]
    M, N = t.shape
    ok = True
    for n0 in range(0, N, 32):
        blk = t[:, n0:n0 + 32]
        starts = np.arange(0, M, 32)
        pos = np.add.reduceat((blk > 0).any(1).astype(np.int64), starts)
        neg = np.add.reduceat((blk < 0).any(1).astype(np.int64), starts)
        zer = np.add.reduceat((blk == 0).any(1).astype(np.int64), starts)
        full = np.diff(np.append(starts, M)) >= 3      # (M = 130, N = 33: the corner tile is two rows of one column)
        ok = ok and bool((pos > 0)[full].all() and (neg > 0)[full].all() and (zer > 0)[full].all())
    last = t[(M - 1) // 32 * 32:, (N - 1) // 32 * 32:]
    return ok, bool((last < 0).any())


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# k-tiles of every K slice of gemm_x3_kernel<1,4> / <2,4> at M = 200 (two row tiles, the last one ragged at 72 rows), by K
X3_SLICES = {32: (1,), 64: (2,), 96: (3,), 128: (4,), 160: (5,), 192: (6,), 224: (7,), 256: (8,), 288: (9,),
             320: (5, 5), 352: (6, 5), 416: (7, 6), 480: (5, 5, 5), 544: (6, 6, 5)}
X3_M = 200
X3_N = (4, 32, 36, 64, 96, 100)
X3_ALL_EPI_K = (160, 352)                 # all four EPI combinations there; elsewhere raw + the full epilogue
X3_MDEV = (0, 1, 127, 128, 129, X3_M)
FULL = dict(epi=3, leaky=True, ldc_pad=4, ldr_pad=4, lda_pad=4)


def x3_kernel(N, M=X3_M):
    return "gemm_x3_kernel<%d,4>" % (1 if N <= 32 else 2)


def _intent(kernel, sl):
    return dict(kernel=kernel, S=len(sl), tiles=tuple(sl))


def x3_cases(N, K):
    """the cases of one (N, K) of the 128-row tile kernels"""
    it = _intent(x3_kernel(N), X3_SLICES[K])
    out = [spec("x3", X3_M, N, K, intent=it, id="raw"), spec("x3", X3_M, N, K, intent=it, id="full", **FULL)]
    if K in X3_ALL_EPI_K:
        out += [spec("x3", X3_M, N, K, intent=it, id="epi%d" % e, epi=e, leaky=True, ldc_pad=4, ldr_pad=4) for e in (0, 1, 2)]
    return out


def x3_extra_cases():
    out = []
    for N in (32, 100):
        for K in (192, 224):                            # the concatenation boundary on every step of the rotation
            for C1 in range(32, 161, 32):
                out.append(spec("x3", X3_M, N, C1, C2=K - C1, intent=_intent(x3_kernel(N), X3_SLICES[K]), id="cat%d+%d-N%d" % (C1, K - C1, N),
                                lds_pad=4, **FULL))
        for K, ld in ((96, 1), (96, 3), (352, 3)):      # gathered x, shadow indices, *N1_dev < N1
            out.append(spec("x3", X3_M, N, K, gather=True, n1=150, n1_dev=131, ld_idx=ld, intent=_intent(x3_kernel(N), X3_SLICES[K]),
                            id="gather-K%d-ld%d-N%d" % (K, ld, N), **FULL))
        out.append(spec("x3", X3_M, N, 64, C2=96, gather=True, n1=150, n1_dev=131, ld_idx=3, lds_pad=4,
                        intent=_intent(x3_kernel(N), X3_SLICES[160]), id="gather+cat-N%d" % N, **FULL))
    for N in (32, 64):                                  # one selection and one network-alpha case per kernel instance
        out.append(spec("x3", X3_M, N, 224, kind="select", intent=_intent(x3_kernel(N), X3_SLICES[224]), id="select-N%d" % N))
        out.append(spec("x3", X3_M, N, 352, kind="select", intent=_intent(x3_kernel(N), X3_SLICES[352]), id="select-split-N%d" % N))
    out.append(spec("x3", X3_M, 64, 160, intent=_intent(x3_kernel(64), X3_SLICES[160]), id="alpha0.2", **dict(FULL, alpha=0.2)))
    return out


# gemm_x3_kernel<4,8>: (M, K, N) -> slices
X3_BIG = {(16640, 32, 256): (1,), (8448, 1024, 256): (11, 11, 10), (22016, 160, 132): (5,)}


def x3_big_cases(M, K, N):
    it = _intent("gemm_x3_kernel<4,8>", X3_BIG[(M, K, N)])
    out = [spec("x3", M, N, K, intent=it, id="raw"), spec("x3", M, N, K, intent=it, id="full", **FULL)]
    if K == 32:
        out.append(spec("x3", M, N, K, kind="select", intent=it, id="select"))
    return out


# the resident-W walk: every wave walks three or four row tiles; nkt 1, 5, 7 (1, 3, 4 where only K <= 128 fits the LDS)
X3R_M = 3 * 65536 + 37
X3R_SHAPES = [(N, K) for N in (32, 36, 64) for K in (32, 160, 224)] + [(N, K) for N in (100, 128) for K in (32, 96, 128)]
X3R_MDEV = (0, 1, 33, 65535, X3R_M)
X3R_TILE_HINT = 60000


def x3r_cases(N, K, hint=0):
    """raw and full epilogue; K = 32 raw is the plain operand, everything else gathered (+ concatenated with a 32-column skip)"""
    if hint:
        tn, waves, S, tps = gemm_x3_plan(X3R_M, N, K, hint)       # (the tile form of these shapes: whatever the cost model takes)
        it = _intent("gemm_x3_kernel<%d,%d>" % (tn, waves), slices(K // 32, tps))
    else:
        it = _intent("gemm_x3r_kernel<%d>" % {1: 1, 2: 2, 4: 4}[cdiv(N, 32)], (K // 32,))
    C1, C2 = (K, 0) if K == 32 else (K - 32, 32)
    g = dict(gather=True, n1=700, n1_dev=650, ld_idx=3)
    raw = spec("x3", X3R_M, N, C1, C2=C2, intent=it, hint=hint, id="raw", **(g if C2 else {}))
    full = spec("x3", X3R_M, N, C1, C2=C2, intent=it, hint=hint, id="full", **dict(FULL, lda_pad=4, lds_pad=4 if C2 else 0, **g))
    return [raw, full]


def x3r_extra_cases():
    out = []
    for N in (32, 64, 128):
        out.append(spec("x3", X3R_M, N, 32, kind="select", intent=_intent("gemm_x3r_kernel<%d>" % (N // 32), (1,)), id="select-N%d" % N))
    out.append(spec("x3", X3R_M, 64, 128, C2=32, gather=True, n1=700, n1_dev=650, intent=_intent("gemm_x3r_kernel<2>", (5,)),
                    id="alpha0.2", **dict(FULL, alpha=0.2, lds_pad=4)))
    return out


# d3f_gemm_x3_chain at the walk size: (K, N, first output stored) -> (C1, C2, gathered); every instance, both LDS boundaries
CHAIN_RANGES = dict(amax=3, wmax=2, w2max=2)
CHAIN_SHAPES = {(256, 64, False): (128, 128, True),     # <2,false>  the decoder pair
                (288, 64, False): (288, 0, False),      #            the largest image the entry point accepts
                (32, 64, False): (32, 0, False),        #            one k-tile: every rotation step is a tile boundary
                (224, 64, True): (96, 128, False),      # <2,true>   the largest stored image at 64 columns
                (160, 64, True): (160, 0, False),       #            five k-tiles
                (96, 128, True): (32, 64, False),       # <4,true>   the encoder pair, a_rebase at k-tile 1
                (32, 128, True): (32, 0, False),        #            one k-tile
                (128, 128, False): (64, 64, False),     # <4,false>  the largest image at 128 columns
                (64, 128, False): (32, 32, True)}       #            gathered + skip
CHAIN_GATHER = dict(gather=True, n1=700, n1_dev=650, ld_idx=3)
SECOND = dict(cs2=True, ch2=True, leaky2=True)


def _chain_spec(K, N, store, id, M=None, **kw):
    C1, C2, gathered = CHAIN_SHAPES[(K, N, store)]
    kw = dict(CHAIN_RANGES, **kw)
    if gathered:
        kw.update(CHAIN_GATHER)
    return spec("chain", X3R_M if M is None else M, N, C1, C2=C2, store=store, intent=_intent(chain_kernel(N, store), (K // 32,)), id=id, **kw)


def chain_cases(K, N, store):
    """raw: no epilogue operand at either level; full: row scale, column scale and shift, residual (ldr = N + 4), LeakyReLU, ldc = N + 4
    where the first output is stored, and the second epilogue"""
    C2 = CHAIN_SHAPES[(K, N, store)][1]
    full = dict(FULL, lds_pad=4 if C2 else 0, ldc_pad=4 if store else 0, **SECOND)
    return [_chain_spec(K, N, store, "raw"), _chain_spec(K, N, store, "full", **full)]


def chain_extra_cases():
    out = []
    for K, N, store in ((256, 64, False), (96, 128, True)):
        out.append(_chain_spec(K, N, store, "select2", kind="select2", amax=0, wmax=0))
    full = lambda K, N, store, **kw: dict(FULL, lds_pad=4 if CHAIN_SHAPES[(K, N, store)][1] else 0, ldc_pad=4 if store else 0, **kw)
    # alpha = alpha2 = 0.2: ONE fp32 multiply of an exact value at either level.  The first output then has full mantissas, so W2 is
    # a selection and the second epilogue a scale (a power of two) and the LeakyReLU
    out.append(_chain_spec(160, 64, True, "alpha0.2", **full(160, 64, True, alpha=0.2, alpha2=0.2, w2="select", cs2=True, leaky2=True)))
    out.append(_chain_spec(64, 128, False, "alpha0.2", **full(64, 128, False, alpha=0.2, alpha2=0.2, w2="select", cs2=True, leaky2=True)))
    out.append(_chain_spec(96, 128, True, "scale2-only", **full(96, 128, True, cs2=True, leaky2=True)))
    out.append(_chain_spec(256, 64, False, "shift2-only", **full(256, 64, False, ch2=True, leaky2=True)))
    out.append(_chain_spec(224, 64, True, "ldc2-32", **full(224, 64, True, ldc2_pad=0, **SECOND)))
    out.append(_chain_spec(128, 128, False, "ldc2-32", **full(128, 128, False, ldc2_pad=0, **SECOND)))
    return out


def gres_cases():
    out = []
    for K in (64, 352):
        for ld in (1, 3):
            out.append(spec("x3_gres", X3_M, 64, K, gres=True, res_rows=90, res_rows_dev=77, ld_res_idx=ld, epi=2, leaky=True, ldc_pad=4,
                            ldr_pad=4, intent=_intent("gemm_x3_kernel<2,4>", X3_SLICES[K]), id="gres-K%d-ld%d" % (K, ld)))
    out.append(spec("x3_gres", X3_M, 64, 352, gres=True, res_rows=90, ld_res_idx=1, epi=3, leaky=True,
                    intent=_intent("gemm_x3_kernel<2,4>", X3_SLICES[352]), id="gres-rows-rs"))
    # d3f_gemm_x3_resident answers 1 for this call: with a gathered residual it must still take the tile form
    out.append(spec("x3_gres", 70000, 64, 64, gres=True, res_rows=500, res_rows_dev=420, ld_res_idx=3, epi=2, leaky=True,
                    intent=_intent("gemm_x3_kernel<2,4>", (2,)), id="gres-resident-shape"))
    return out


# d3f_gemm_f32t: M = 100 is fewer than 8 items (the grid is padded to a multiple of 8)
DMA_M = 100
DMA_SLICES = {4: (1,), 32: (1,), 36: (2,), 64: (2,), 96: (3,), 128: (4,), 160: (5,), 544: (9, 8), 800: (9, 9, 7)}
DMA_N = (4, 32, 36, 68)
DMA_MDEV = (0, 1, 63, 64, 65, DMA_M)


def dma_kernel(N, epi):
    return "gemm_dma_kernel<%s,%d>" % ("4,1" if N <= 32 else "2,2", epi)


def dma_cases(N, K):
    out = []
    for e in range(4):
        out.append(spec("f32t", DMA_M, N, K, epi=e, col=e > 0, leaky=e > 0, ldc_pad=4 if e else 0, ldr_pad=4, lda_pad=4 if e else 0,
                        intent=_intent(dma_kernel(N, e), DMA_SLICES[K]), id="epi%d" % e))
    return out


def dma_extra_cases():
    out = []
    for N in (32, 68):
        for C2 in (28, 60, 508):                        # a concatenation boundary inside a k-tile (C1 = 36)
            K = 36 + C2
            out.append(spec("f32t", DMA_M, N, 36, C2=C2, lda_pad=4, lds_pad=4, intent=_intent(dma_kernel(N, 3), DMA_SLICES[K]),
                            id="cat36+%d-N%d" % (C2, N), **{k: v for k, v in FULL.items() if k != "lda_pad"}))
        for K, ld in ((36, 1), (160, 3), (544, 3)):
            out.append(spec("f32t", DMA_M, N, K, gather=True, n1=80, n1_dev=66, ld_idx=ld, intent=_intent(dma_kernel(N, 3), DMA_SLICES[K]),
                            id="gather-K%d-N%d" % (K, N), **FULL))
        out.append(spec("f32t", DMA_M, N, 36, C2=28, gather=True, n1=80, n1_dev=66, ld_idx=3, lds_pad=4,
                        intent=_intent(dma_kernel(N, 3), DMA_SLICES[64]), id="gather+cat-N%d" % N, **FULL))
        out.append(spec("f32t", DMA_M, N, 160, kind="select", intent=_intent(dma_kernel(N, 0), DMA_SLICES[160]), id="select-N%d" % N))
        out.append(spec("f32t", DMA_M, N, 544, kind="select", intent=_intent(dma_kernel(N, 0), DMA_SLICES[544]), id="select-split-N%d" % N))
    out.append(spec("f32t", DMA_M, 68, 96, intent=_intent(dma_kernel(68, 3), DMA_SLICES[96]), id="alpha0.2", **dict(FULL, alpha=0.2)))
    return out


# d3f_gemm_f32 / d3f_gemm_upsample_cat_f32: gemm_fast_kernel and gemm_f32_kernel
F32_M = 100
F32_SLICES = {0: (0,), 96: (3,), 97: (4,), 544: (9, 8), 545: (9, 9)}


def f32_kernel(fast, N, epi):
    shape = "4,1" if N <= 32 else "2,2"
    return "gemm_fast_kernel<%s,%d>" % (shape, epi) if fast else "gemm_f32_kernel<%s>" % shape


def f32_cases():
    out = []
    for N in (32, 68):
        for K in (0, 96, 544):                          # the straight-line kernel: both tiles, EPI 0 .. 3, K = 0, a K split
            for e in range(4):
                out.append(spec("f32", F32_M, N, K, epi=e, col=e > 0, leaky=e > 0, ldc_pad=4 if e else 0, ldr_pad=4, lda_pad=4 if e else 0,
                                ldb_pad=4 if e else 0, intent=_intent(f32_kernel(True, N, e), F32_SLICES[K]), id="fast-N%d-K%d-epi%d" % (N, K, e)))
        for K in (96, 544):
            out.append(spec("f32", F32_M, N, K, kind="select", intent=_intent(f32_kernel(True, N, 0), F32_SLICES[K]), id="fast-select-N%d-K%d" % (N, K)))
            out.append(spec("upcat", F32_M, N, 36, C2=K - 36, gather=True, n1=80, n1_dev=66, ld_idx=3, col=True, leaky=True, ldc_pad=4,
                            lda_pad=4, lds_pad=4, ldb_pad=4, intent=_intent(f32_kernel(True, N, 0), F32_SLICES[K]), id="fast-upcat-N%d-K%d" % (N, K)))
        # the generic kernel, reached by each single cause, unsplit and split
        for tag, kw, dk, dn in (("oddK", {}, 1, 0), ("oddN", {}, 0, 1), ("lda", dict(lda_pad=1), 0, 0), ("ldb", dict(ldb_pad=1), 0, 0),
                                ("ldc", dict(ldc_pad=1), 0, 0), ("baseA", dict(a_off=1), 0, 0), ("baseB", dict(b_off=1), 0, 0)):
            for K in (96, 544):
                n = N + dn if N > 32 else N - dn        # (31 stays on the 128 x 32 tile, 69 on the 64 x 64 one)
                out.append(spec("f32", F32_M, n, K + dk, epi=3, leaky=True, ldr_pad=0, intent=_intent(f32_kernel(False, n, 3), F32_SLICES[K + dk]),
                                id="generic-%s-N%d-K%d" % (tag, n, K + dk), **kw))
        out.append(spec("f32", F32_M, N, 97, kind="select", lda_pad=1, intent=_intent(f32_kernel(False, N, 0), F32_SLICES[97]),
                        id="generic-select-N%d" % N))
        out.append(spec("upcat", F32_M, N + 1, 36, C2=544 - 36, gather=True, n1=80, n1_dev=66, ld_idx=1, col=True, leaky=True, lds_pad=4,
                        intent=_intent(f32_kernel(False, N + 1, 0), F32_SLICES[544]), id="generic-upcat-N%d" % (N + 1)))
    out.append(spec("f32", F32_M, 68, 96, intent=_intent(f32_kernel(True, 68, 3), F32_SLICES[96]), id="fast-alpha0.2", **dict(FULL, alpha=0.2)))
    out.append(spec("f32", F32_M, 68, 97, intent=_intent(f32_kernel(False, 68, 3), F32_SLICES[97]), id="generic-alpha0.2",
                    epi=3, leaky=True, alpha=0.2))
    return out


F32_MDEV = (0, 1, 63, 64, 65, F32_M)

# d3f_gemm_bf16
BF16_M = (100, 130)
BF16_SLICES = {36: (2,), 64: (2,), 544: (9, 8), 1024: (8, 8, 8, 8)}
BF16_N = (20, 33, 64, 100)
BF16_CAT = {36: 20, 64: 32, 544: 512, 1024: 512}      # C1 of the concatenated form of every K


def bf16_cases(M, K, N, a, cb):
    it = _intent("gemm_bf16_kernel<%d,%d>" % (a, cb), BF16_SLICES[K])
    kw = dict(a_bf16=a, c_bf16=cb, intent=it)
    C1 = BF16_CAT[K]
    return [spec("bf16", M, N, K, id="raw", **kw),
            spec("bf16", M, N, K, id="full", epi=3, leaky=True, **kw),
            spec("bf16", M, N, C1, C2=K - C1, gather=True, n1=80, n1_dev=66, ld_idx=3, col=True, leaky=True, id="upcat", **kw),
            spec("bf16", M, N, C1, C2=K - C1, col=True, leaky=True, id="cat2", **kw)]


def all_small_specs():
    """every case but the large ones (x3 256 x 128 tiles, the resident walk), for the CPU checks"""
    out = []
    for N in X3_N:
        for K in X3_SLICES:
            out += x3_cases(N, K)
    out += x3_extra_cases() + [s for s in gres_cases() if s["M"] < 1000]
    for N in DMA_N:
        for K in DMA_SLICES:
            out += dma_cases(N, K)
    out += dma_extra_cases() + f32_cases()
    for M in BF16_M:
        for K in BF16_SLICES:
            for N in BF16_N:
                for a in (0, 1):
                    for cb in (0, 1):
                        out += bf16_cases(M, K, N, a, cb)
    return out


def case_id(s):
    e = s["entry"] + ("%d%d" % (s["a_bf16"], s["c_bf16"]) if s["entry"] == "bf16" else "") + ("-hint%d" % s["hint"] if s["hint"] else "")
    if s["entry"] == "chain":
        e += "-stored" if s["store"] else "-unstored"
    return "%s-M%d-N%d-K%d+%d-%s" % (e, s["M"], s["N"], s["C1"], s["C2"], s["id"])
