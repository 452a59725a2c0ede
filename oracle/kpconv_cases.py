"""TEST INFRASTRUCTURE ONLY.  Seeded synthetic inputs for the KPConv kernel tests (tests/test_gpu_kpconv_branches.py on the GPU,
tests/test_oracle_network.py on the CPU): no room fragment, no neighbour grid -- the smallest shapes at which each kernel of
csrc/kpconv.hip can still go wrong, built so that the two discontinuities of the operator are never decided by rounding:

  1. row sums ("does this neighbour count", sum_c f > 0, kernels/convolution_ops.py:250-251): every feature row's float64 sum is
     exactly 0 or at least 2^-10 * sum|f| away from 0, so every fp32 / fp64 summation order agrees on its sign;
  2. 'closest' (:227-229): for every valid (query, neighbour) pair the two smallest squared distances to the kernel points differ
     by at least 1e-4 relative in float64 (the kernels contract d2 into FMAs, torch does not: a near-tie would flip the arg-min).

Both are CONDITIONS, not exclusions: inputs are nudged / re-drawn until they hold for every row and pair, and features() and
kpconv_case() assert them on whatever they return, so they hold on every input a test computes with.  The CPU test asserts them
again (row_sums_decided, closest_decided) on shape_case() of every shape of all_shapes() with 15 kernel points; the GPU tests build
their inputs with the same shape_case(), also with 4 / 13 kernel points and with the supports as queries."""
import math

import numpy as np

EXTENT = float(np.float32(0.03))      # KP_extent: a float32 value, so the kernels and the float64 reference use the same number
GARBAGE = 0x3fffffff                  # padding columns of an index matrix with ld_idx > K
MODES = [(i, a) for a in ("sum", "closest") for i in ("constant", "linear", "gaussian")]


class Case(dict):
    __getattr__ = dict.__getitem__


def bf16_values(a):
    """float32 array -> the same values rounded to bfloat16 (round to nearest even), still float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def kernel_points(seed, num_kp):
    """num_kp points of norm <= 1.5 * KP_extent = 0.045, KP[0] = 0 (the 'center' disposition's fixed point)."""
    rng = np.random.default_rng(1000 + seed)
    d = rng.standard_normal((num_kp, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kp = (d * (rng.random((num_kp, 1)) ** (1.0 / 3.0)) * 0.045 * 0.999).astype(np.float32)
    kp[0] = 0
    return kp


def row_sums_decided(f):
    """condition 1 for every row of f (float32 or bfloat16 values)."""
    f = np.asarray(f, np.float64)
    s = np.asarray([math.fsum(r) for r in f])
    return bool(np.all((s == 0) | (np.abs(s) >= 2.0 ** -10 * np.abs(f).sum(1))))


def features(rng, Ns, C, bf16=False):
    """N(0, 1) rows; ~20 % with a negative sum; rows i % 11 == 3: +-pairs of multiples of 2^-8 (sum exactly 0
    in fp32 and fp64 in any order, C >= 2); rows i % 13 == 5: all zeros."""
    x = rng.standard_normal((Ns, C)).astype(np.float32)
    neg = rng.random(Ns) < 0.2
    s = x.astype(np.float64).sum(1)
    x[(s < 0) != neg] *= -1
    h = C // 2
    for i in range(Ns):
        if i % 11 == 3 and h:
            x[i] = 0
            x[i, :h] = (np.round(rng.standard_normal(h) * 256) / 256).astype(np.float32)    # multiples of 2^-8: every partial
            x[i, h:2 * h] = -x[i, :h]                                                        # sum is exact in fp32, in any order
        if i % 13 == 5:
            x[i] = 0
    if bf16:
        x = bf16_values(x)
    for _ in range(64):
        xd = x.astype(np.float64)
        s = np.asarray([math.fsum(r) for r in xd])
        bad = (s != 0) & (np.abs(s) < 2.0 ** -10 * np.abs(xd).sum(1))
        if not bad.any():
            break
        x[bad, 0] += np.where(s[bad] >= 0, 0.5, -0.5).astype(np.float32)     # (0.5: a bfloat16 value)
        if bf16:
            x = bf16_values(x)
    assert row_sums_decided(x)
    return x


def _closest_margin(q, s, idx, KP, Ns):
    """[Nq, K] bool: the pair is valid and its two smallest d2 are closer than 1e-4 relative."""
    if KP.shape[0] < 2 or idx.size == 0:
        return np.zeros(idx.shape, bool)
    valid = (idx >= 0) & (idx < Ns)
    rel = s.astype(np.float64)[np.where(valid, idx, 0)] - q.astype(np.float64)[:, None, :]
    d2 = np.sort(((rel[:, :, None, :] - KP.astype(np.float64)[None, None]) ** 2).sum(-1), -1)
    return valid & (d2[..., 1] - d2[..., 0] < 1e-4 * d2[..., 1])


def closest_decided(c):
    """condition 2 for every valid (query, neighbour) pair of a case."""
    return not _closest_margin(c.q[:c.Nq], c.s[:c.Ns], c.idx[:c.Nq], c.KP, c.Ns).any()


def kpconv_case(seed, Cin, K, Nq, Ns=150, num_kp=15, self_queries=False, bf16=False, cap_q=0, cap_s=0, near=28):
    """-> Case(q [Nq + cap_q, 3], s [Ns + cap_s, 3], idx i32[Nq + cap_q, K], f [Ns + cap_s, Cin], KP [num_kp, 3], Nq, Ns).
    Supports: uniform in a box of edge 0.25.  Queries: the supports themselves (self_queries: Nq = Ns) or jittered copies of
    randomly drawn supports.  Index rows: K draws with repetition from the query's `near` nearest supports (so a good part of the
    pairs lies inside the kernel's reach of 2 * KP_extent + |KP|), then 28 % shadow slots: == Ns, > Ns (up to Ns + 1000) and
    negative; with Nq >= 4, rows 1 and Nq // 2 hold no valid slot at all.  Capacity rows (cap_q / cap_s: rows beyond the
    effective counts Nq / Ns, which the kernels are told through Nq_dev / Ns_dev) hold NaN points and features and index rows that
    point at valid supports: a kernel that visits them writes rows it must not write."""
    rng = np.random.default_rng(seed)
    if self_queries:
        Ns = Nq
    s = (rng.random((Ns, 3)) * 0.25).astype(np.float32)
    if self_queries:
        q = s.copy()
    else:
        q = (s[rng.integers(0, Ns, Nq)] + rng.normal(0, 0.004, (Nq, 3))).astype(np.float32)
    KP = kernel_points(seed, num_kp)
    d = ((q.astype(np.float64)[:, None, :] - s.astype(np.float64)[None]) ** 2).sum(-1)
    cand = np.argsort(d, 1, kind="stable")[:, :min(near, Ns)]

    def draw(shape_rows):
        return np.take_along_axis(cand[shape_rows], rng.integers(0, cand.shape[1], (len(shape_rows), K)), 1)
    idx = draw(np.arange(Nq)).astype(np.int64)
    for _ in range(200):                                   # condition 2: re-draw the slots whose arg-min would be a near-tie
        bad = _closest_margin(q, s, idx, KP, Ns)
        if not bad.any():
            break
        idx = np.where(bad, draw(np.arange(Nq)), idx)
    r = rng.random((Nq, K))
    idx = np.where(r < 0.12, Ns, idx)
    idx = np.where((r >= 0.12) & (r < 0.2), Ns + 1 + rng.integers(0, 1000, (Nq, K)), idx)
    idx = np.where((r >= 0.2) & (r < 0.28), -1 - rng.integers(0, 1000, (Nq, K)), idx)
    if Nq >= 4:
        for row in (1, Nq // 2):
            idx[row] = np.where(np.arange(K) % 2 == 0, Ns, -3)
    f = features(rng, Ns, Cin, bf16)
    if cap_q:
        q = np.concatenate([q, np.full((cap_q, 3), np.nan, np.float32)])
        idx = np.concatenate([idx, rng.integers(0, Ns, (cap_q, K))])
    if cap_s:
        s = np.concatenate([s, np.full((cap_s, 3), np.nan, np.float32)])
        f = np.concatenate([f, np.full((cap_s, Cin), np.nan, np.float32)])
    c = Case(q=q, s=s, idx=idx.astype(np.int32), f=f, KP=KP, Nq=Nq, Ns=Ns)
    assert closest_decided(c)
    return c


def weights(seed, num_kp, Cin, Cout):
    """K_values with outputs of order 1 for N(0, 1) features (He scaling over the num_kp * Cin contraction, times 2 for the
    neighbour-count division)."""
    rng = np.random.default_rng(2000 + seed)
    return (rng.standard_normal((num_kp, Cin, Cout)) * (2.0 * np.sqrt(2.0 / (num_kp * Cin)))).astype(np.float32)


def rowpos_case(seed, Ns, Cin, bf16=False):
    """Rows for d3f_row_positive, whose claim is the sign of the EXACT sum: N(0, 1) rows, then (row i % 8, where they fit)
      1: +-pairs, sum exactly 0        2: {2^20, 1, -2^20} (exact in fp32 too) and, every other time, {2^25, 1, -2^25}: positive
      only if accumulated wider than fp32 (2^25 + 1 rounds to 2^25 in fp32: a left-to-right fp32 sum gives 0)
      3: the negative mirror of 2      4: all -0.0          5: a lone subnormal (2^-133: a bfloat16 subnormal too)
      6: all negative                  7: one positive value in the last channel only.
    -> (f float32 [Ns, Cin] (bfloat16 values if bf16), want uint8 [Ns] = math.fsum(row) > 0)."""
    rng = np.random.default_rng(3000 + seed)
    x = rng.standard_normal((Ns, Cin)).astype(np.float32)
    sub = np.asarray([0x00010000], np.uint32).view(np.float32)[0]
    for i in range(Ns):
        k = i % 8
        if k == 1 and Cin >= 2:
            h = Cin // 2
            x[i] = 0
            x[i, :h] = (np.round(rng.standard_normal(h) * 256) / 256).astype(np.float32)    # multiples of 2^-8: every partial sum
            x[i, h:2 * h] = -x[i, :h]                                                        # is exact, in any order and precision
        elif k in (2, 3) and Cin >= 3:
            x[i] = 0
            p = rng.permutation(Cin)[:3] if i >= 8 else np.arange(3)
            big = 2.0 ** (25 if (i // 8) % 2 else 20)
            x[i, np.sort(p)] = np.asarray([big, 1.0, -big], np.float32) * (1 if k == 2 else -1)
        elif k == 4:
            x[i] = -0.0
        elif k == 5:
            x[i] = 0
            x[i, (i // 8) % Cin] = sub
        elif k == 6:
            x[i] = -np.abs(x[i]) - np.float32(0.25)
        elif k == 7:
            x[i] = 0
            x[i, Cin - 1] = np.float32(0.75)
    if bf16:
        x = bf16_values(x)
    want = np.asarray([1 if math.fsum(r) > 0 else 0 for r in x.astype(np.float64)], np.uint8)
    return x, want


# ---- the shapes: queries per workgroup (TQ) and neighbours per chunk of each kernel ---------------------------------------------
FUSED32_K = (1, 7, 8, 9, 37)                  # kpconv_fused32_kernel: chunks of KF_LQ = 8
C1_K = (1, 2, 37, 64, 65, 130)                # the Cin = 1 kernels: passes of 64 neighbours, pairs of two
C1_COUT = (1, 10, 64, 65, 130, 256)


def nq_values(TQ):
    """1, TQ - 1, 3 TQ + 5 queries (TQ = queries per workgroup)."""
    return sorted({1, TQ - 1, 3 * TQ + 5} - {0})


def agg_k_values(LQ):
    """kpconv_agg_vec4<LQ>: around its chunk KC = LQ; LQ <= 8: the PF = 8 prefetch group as well."""
    if LQ == 256:
        return [1, 40, 257]
    ks = {0, 1, LQ - 1, LQ, LQ + 1, 37}
    if LQ <= 8:
        ks |= {7, 8, 9}
    return sorted(ks)


def fused_k_values(LQ):
    """kpconv_fused_kernel<LQ>: around LQ, and (LQ = 64: the chunk is 32 wide) around 32."""
    return sorted({1, LQ - 1, LQ, LQ + 1} | ({31, 33} if LQ == 64 else set()))


def combos(nqs, ks):
    """A sparse (Nq, K) matrix: every K once; Nq = 1 with the second K, the larger Nq values in turn with the others, the last
    (largest) K with the largest Nq."""
    big = nqs[1:] or nqs
    out = [(big[j % len(big)], k) for j, k in enumerate(ks)]
    out[min(1, len(ks) - 1)] = (nqs[0], ks[min(1, len(ks) - 1)])
    out[-1] = (nqs[-1], ks[-1])
    return out


def shape_case(kernel, Cin, Nq, K, num_kp=15, bf16=False, self_queries=False):
    """The case of one entry of all_shapes(), as the CPU and the GPU tests build it: seeded by the shape, 5 capacity query rows and 7
    capacity support rows; self_queries (the supports are the queries, Ns = Nq) only from 30 queries on."""
    return kpconv_case(shape_seed(kernel, Cin, Nq, K), Cin, K, Nq, num_kp=num_kp, bf16=bf16, cap_q=5, cap_s=7,
                       self_queries=self_queries and Nq >= 30)


def has_bf16(kernel, Cin):
    """Does the kernel family have a bfloat16 feature-storage instantiation at this Cin (the case is then generated twice)?"""
    return kernel in ("fused32", "fused") or (kernel == "agg_vec4" and Cin in (256, 512))


def shapes_of(kernel, Cin):
    """The (Nq, K) list of one kernel family and channel count, in the order of all_shapes()."""
    return [(nq, k) for kn, c, nq, k in all_shapes() if (kn, c) == (kernel, Cin)]


def all_shapes():
    """Every (kernel, Cin, Nq, K) the GPU tests generate (agg_scalar Cin = 32, Nq = 3: also the 2^24 index stride case; "errors":
    the operands of the argument-error calls, never computed with)."""
    out = [("errors", 16, 9, 5), ("errors", 128, 7, 9), ("errors", 256, 7, 9), ("errors", 512, 7, 9), ("errors", 32, 9, 5),
           ("errors", 64, 9, 5), ("errors", 1, 31, 37)]
    for LQ in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        out += [("agg_vec4", 4 * LQ, nq, k) for nq, k in combos(nq_values(256 // LQ), agg_k_values(LQ))]
    out += [("agg_scalar", cin, nq, k) for cin in (6, 1, 32) for nq, k in ((37, 9), (3, 5))]
    out += [("fused32", 32, nq, k) for nq, k in combos(nq_values(32), FUSED32_K)]
    for LQ in (16, 32, 64):
        out += [("fused", 4 * LQ, nq, k) for nq, k in combos(nq_values(16), fused_k_values(LQ))]
    out += [("c1_sum", 1, nq, k) for nq, k in combos(nq_values(16), C1_K)]
    out += [("c1_closest", 1, nq, k) for nq, k in combos(nq_values(32), C1_K)]
    return out


def shape_seed(kernel, Cin, Nq, K):
    return (sum(map(ord, kernel)) * 7919 + Cin * 131 + Nq * 17 + K) % (1 << 31)
