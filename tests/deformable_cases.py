"""TEST INFRASTRUCTURE ONLY.  Seeded synthetic inputs for the deformable KPConv kernel tests: oracle.kpconv_cases.kpconv_case (imported,
not edited) plus per-query kernel-point offsets and modulations, built so that the two further discontinuities of the deformable
operator (kernels/convolution_ops.py:379-499) are never decided by rounding -- in the manner of that file's condition 2:

  1. in range (:435, and the 'constant' influence :456): for every valid (query, neighbour, kernel point) the squared distance to the
     DEFORMED kernel point satisfies |d2 / KP_extent^2 - 1| >= 1e-4 in float64, about a hundred times the fp32 rounding of d2;
  2. 'closest' (:473-475): for every valid (query, neighbour) the two smallest d2 to the DEFORMED points differ by at least 1e-4
     relative (and, for the rigid offset convolution that precedes the operator, kpconv_cases' own condition 2 on the rigid points).

Offending index slots are re-drawn until both hold for every slot: no case is left out.  deform_case() asserts both conditions on
what it returns, and that the case holds valid neighbours that are in range AND valid neighbours that are not (otherwise the range
filter is untested): where chance does not provide both, one slot is pointed at the support nearest to a deformed point and one at the farthest.
"""
import numpy as np

from oracle import kpconv_cases as kc

EXTENT = kc.EXTENT
OFF_SIGMA = 0.2           # raw offsets ~ N(0, 0.2) per coordinate, in units of KP_extent: |offset| ~ 0.35, up to ~0.8 KP_extent


def TQ(LQ):
    """queries per workgroup of kpconv_deform_agg_vec4<LQ> (csrc/kpconv_deform.hip)."""
    return min(256 // LQ, 64)


def k_values(LQ):
    """around the neighbour chunk KC = LQ."""
    return sorted({1, LQ - 1, LQ + 1, 2 * LQ + 3} - {0})


def shapes(LQ):
    """(Nq, K): Nq in {1, TQ - 1, 3 TQ + 5} x the K values, sparse (kpconv_cases.combos)."""
    return kc.combos(kc.nq_values(TQ(LQ)), k_values(LQ))


def deformed_d2(q, s, idx, KP, raw, Ns, extent=EXTENT):
    """float64 -> (valid [Nq, K], d2 [Nq, K, P] to the deformed points KP + raw[:, :3P] * extent)."""
    P = KP.shape[0]
    valid = (idx >= 0) & (idx < Ns)
    kpd = KP.astype(np.float64)[None] + raw[:, :3 * P].astype(np.float64).reshape(-1, P, 3) * float(extent)
    rel = s.astype(np.float64)[np.where(valid, idx, 0)] - q.astype(np.float64)[:, None, :]
    return valid, ((rel[:, :, None, :] - kpd[:, None, :, :]) ** 2).sum(-1)


def _undecided(q, s, idx, KP, raw, Ns):
    """[Nq, K] bool: valid slots that break condition 1 or 2 (or kpconv_cases' condition 2 on the rigid points)."""
    if idx.size == 0:
        return np.zeros(idx.shape, bool)
    valid, d2 = deformed_d2(q, s, idx, KP, raw, Ns)
    bad = (np.abs(d2 / EXTENT ** 2 - 1.0) < 1e-4).any(-1)
    if KP.shape[0] >= 2:
        d = np.sort(d2, -1)
        bad |= d[..., 1] - d[..., 0] < 1e-4 * d[..., 1]
    return valid & (bad | kc._closest_margin(q, s, idx, KP, Ns))


def range_decided(c):
    """conditions 1 and 2 for every valid slot of a case."""
    return not _undecided(c.q[:c.Nq], c.s[:c.Ns], c.idx[:c.Nq].astype(np.int64), c.KP, c.raw[:c.Nq], c.Ns).any()


def in_range_counts(c):
    """-> (valid neighbours in range of a deformed point, valid neighbours out of range)."""
    if c.idx[:c.Nq].size == 0:
        return 0, 0
    valid, d2 = deformed_d2(c.q[:c.Nq], c.s[:c.Ns], c.idx[:c.Nq].astype(np.int64), c.KP, c.raw[:c.Nq], c.Ns)
    near = (d2 < EXTENT ** 2).any(-1)
    return int((valid & near).sum()), int((valid & ~near).sum())


def deform_case(seed, Cin, K, Nq, num_kp=15, self_queries=False, cap_q=5, cap_s=7, near=28):
    """kpconv_case(...) + raw f32[Nq + cap_q, 4 num_kp]: columns 0 .. 3 num_kp - 1 the offsets of the kernel points in units of
    KP_extent (what the offset convolution emits), the last num_kp the modulation logits (modulation = 2 sigmoid); capacity rows
    hold NaN.  A test without modulations passes raw[:, :3 num_kp]."""
    c = kc.kpconv_case(seed, Cin, K, Nq, num_kp=num_kp, self_queries=self_queries, cap_q=cap_q, cap_s=cap_s, near=near)
    Nq, Ns, P = c.Nq, c.Ns, num_kp
    assert Nq * K >= 2, "one pair cannot be both in and out of range"
    rng = np.random.default_rng(seed + 7777)
    raw = np.concatenate([rng.normal(0, OFF_SIGMA, (len(c.q), 3 * P)), rng.normal(0, 1.0, (len(c.q), P))], 1).astype(np.float32)
    raw[Nq:] = np.nan
    q, s = c.q[:Nq], c.s[:Ns]
    idx = c.idx.astype(np.int64)
    d = ((q.astype(np.float64)[:, None, :] - s.astype(np.float64)[None]) ** 2).sum(-1)
    order = np.argsort(d, 1, kind="stable")
    cand = order[:, :min(near, Ns)]
    c["raw"] = raw
    # both kinds of valid neighbour: rows that kpconv_case left with valid slots (rows 1 and Nq // 2 hold none from 4 queries on)
    rows = [r for r in range(Nq) if not (Nq >= 4 and r in (1, Nq // 2))]

    def plant(row, slot, want_in):
        """Point idx[row, slot] at a support that is in range (nearest to a deformed point first) / out of range (farthest first)
        and decided."""
        _, d2 = deformed_d2(q[row:row + 1], s, np.arange(Ns)[None, :], c.KP, raw[row:row + 1], Ns)
        dmin = d2[0].min(-1)
        for j in (np.argsort(dmin, kind="stable") if want_in else np.argsort(-dmin, kind="stable")):
            if (dmin[j] < EXTENT ** 2) != want_in:
                return False
            trial = idx[row:row + 1].copy()
            trial[0, slot] = j
            if not _undecided(q[row:row + 1], s, trial, c.KP, raw[row:row + 1], Ns)[0, slot]:
                idx[row, slot] = j
                return True
        return False

    def kinds():
        """[Nq, K]: 0 shadow, 1 valid and in range, 2 valid and out of range."""
        valid, d2 = deformed_d2(q, s, idx[:Nq], c.KP, raw[:Nq], Ns)
        return np.where(valid, np.where((d2 < EXTENT ** 2).any(-1), 1, 2), 0)
    for want_in in (True, False):
        kd = kinds()
        if (kd == (1 if want_in else 2)).any():
            continue
        other = 2 if want_in else 1                  # never overwrite the only neighbour of the other kind
        free = [(r, k) for r in rows for k in range(K) if not (kd[r, k] == other and (kd == other).sum() == 1)]
        assert any(plant(r, k, want_in) for r, k in free), "no support %s range of a free slot" % ("in" if want_in else "out of")
    for _ in range(200):
        bad = _undecided(q, s, idx[:Nq], c.KP, raw[:Nq], Ns)
        if not bad.any():
            break
        redraw = np.take_along_axis(cand, rng.integers(0, cand.shape[1], (Nq, K)), 1)
        idx[:Nq] = np.where(bad, redraw, idx[:Nq])
    c["idx"] = idx.astype(np.int32)
    assert range_decided(c) and kc.closest_decided(c)
    n_in, n_out = in_range_counts(c)
    assert n_in > 0 and n_out > 0, (n_in, n_out)
    return c


def shape_case(kernel, Cin, Nq, K, num_kp=15, self_queries=False):
    """The case of one (kernel family, Cin, Nq, K): seeded by the shape, 5 capacity query rows and 7 capacity support rows."""
    return deform_case(kc.shape_seed("deform_" + kernel, Cin, Nq, K), Cin, K, Nq, num_kp=num_kp, self_queries=self_queries and Nq >= 30)
