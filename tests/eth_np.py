"""float64 / numpy restatement of the ETH test's evaluation (geometric_registration_eth/evaluate_eth.py of the reference), done the
slow way: per pair np.nan_to_num of both descriptor blocks, the last 250 rows, the mutually nearest pairs, the target points moved
with gt, the distances against the threshold, the ratio through the 8 decimals of the result file; per scene the sums of
evaluate_eth.py:153-163 and the closing figures of :168-177.  Plus the integer form of that rounding (ratio_e8) next to Python's own
formatting (ratio_e8_python), and the margin rule of the fixture.

The mutual pairs are tests/matching_np.py's (float64 squared distances); as there, this module does not claim the kernel's bits and is
to be used only on inputs whose margins were asserted first (margins() below).  A helper module (no tests in it)."""
from fractions import Fraction

import numpy as np

import matching_np as mnp

LARGE_B = (1024, 1280, 1536, 2560, 4096, 5120, 7680, 8192)


# ---- the rounding of the result file ----------------------------------------------------------------------------------------------
def ratio_e8_python(a, b):
    """The integer m with m / 1e8 == float("%.8f" % (a / b)), through Python's own formatting; 0 for b == 0."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    out = np.zeros(len(a), np.int64)
    for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        if y > 0:
            text = "%.8f" % (x / y)
            out[i] = int(text.replace(".", ""))
            assert out[i] / 1e8 == float(text)
    return out


def ratio_e8(a, b):
    """The same integer without formatting anything: m = floor((2 a 1e8 + b) / (2 b)) in int64; on a tie ((2 a 1e8) mod 2 b == b) the
    sign of fl(a / b) * b - a, taken exactly, decides (positive: up, negative: down, zero: to the even integer).  0 for b == 0."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ok = b > 0
    bb = np.where(ok, b, 1)
    num, den = 2 * a * 10 ** 8, 2 * bb
    m = (num + bb) // den
    for i in np.nonzero(ok & (num % den == bb))[0]:
        e = Fraction(float(a[i]) / float(b[i])) * int(b[i]) - int(a[i])          # exact: what fma(q, b, -a) returns
        if e < 0 or (e == 0 and m[i] % 2):
            m[i] -= 1
    return np.where(ok, m, 0)


def rounding_cases():
    """(a, b) i32 arrays: every 0 <= a <= b for b <= 599 (b = 0 included) and for the eight b that are multiples of 512 or near."""
    bs = list(range(600)) + list(LARGE_B)
    a = np.concatenate([np.arange(b + 1) for b in bs])
    b = np.concatenate([np.full(b + 1, b) for b in bs])
    return a.astype(np.int32), b.astype(np.int32)


# ---- register2Fragments and the aggregation -----------------------------------------------------------------------------------------
def sanitize(block, C=32):
    out = np.array(block, np.float32)
    out[:, 3:3 + C] = np.nan_to_num(out[:, 3:3 + C])
    return out


def pair_counts(blocks, pairs, gts, gt_flag, num_keypts=(250,), threshold=0.10, C=32, nan_to_num=True):
    """(mutual_count, gt_inliers) i64[P, n] of every pair (listed or not) on the sanitised blocks: matching_np.match_counts."""
    use = [sanitize(b, C) for b in blocks] if nan_to_num else blocks
    return mnp.match_counts(use, pairs, gts, num_keypts, threshold, C)


def rows(mutual_count, gt_inliers, gt_flag):
    """The rows [num_inliers, ratio, gt_flag] of one count as evaluate_eth.py:150-151 reads them back from the files :67-69 write."""
    out = []
    for m, i, g in zip(mutual_count, gt_inliers, gt_flag):
        if not g:
            out.append([0, float("%.8f" % 0), 0])
        else:
            out.append([int(i), float("%.8f" % (int(i) / int(m))) if m else 0.0, 1])
    return out


def scene_figures(rows_, scene_start, inlier_ratio=0.05):
    """i64[S, 4] (ground-truth pairs, pairs above the ratio, sum of inliers, sum of round(ratio * 1e8) over the ground-truth pairs)
    and f64[S] the float sum of the ratios over the ground-truth pairs as evaluate_eth.py:162 adds them."""
    fig, fsum = np.zeros((len(scene_start) - 1, 4), np.int64), np.zeros(len(scene_start) - 1)
    for s in range(len(scene_start) - 1):
        r = np.array(rows_[scene_start[s]:scene_start[s + 1]], dtype=np.float64).reshape(-1, 3)
        gt = r[:, 2] == 1
        fig[s] = [gt.sum(), (r[:, 1] > inlier_ratio).sum(), int(r[gt, 0].sum()), int(np.rint(r[gt, 1] * 1e8).astype(np.int64).sum())]
        fsum[s] = np.sum(np.where(gt, r[:, 1], np.zeros(r.shape[0])))
    return fig, fsum


def lines(rows_, scene_start, inlier_ratio=0.05):
    """The lines evaluate_eth.py:158-177 prints, from the rows: per scene the two counts, the recall in percent and the two sums over the
    listed pairs divided by the number of pairs above the ratio (numpy's float64 sums, as there), then the stars, the list of recalls,
    the pooled recall and the three means over the scenes."""
    out, per_scene, above_all, listed_all = [], [], 0, 0
    for s in range(len(scene_start) - 1):
        r = np.array(rows_[scene_start[s]:scene_start[s + 1]])
        listed, above = np.sum(r[:, 2] == 1), np.sum(r[:, 1] > inlier_ratio)
        nothing = np.zeros(r.shape[0])
        fig = (float(above / listed) * 100, np.sum(np.where(r[:, 2] == 1, r[:, 0], nothing)) / above,
               np.sum(np.where(r[:, 2] == 1, r[:, 1], nothing)) / above)
        out += ["Correct Match %s, ground truth Match %s" % (above, listed), "Recall %s%%" % fig[0], "Average Num Inliners: %s" % fig[1],
                "Average Num Inliner Ratio: %s" % fig[2]]
        per_scene.append(fig)
        above_all, listed_all = above_all + above, listed_all + listed
    mean = lambda k: sum(f[k] for f in per_scene) / len(per_scene)
    return out + ["*" * 40, str([f[0] for f in per_scene]), "Avergae Matching Recall: %s%%" % (above_all / listed_all * 100),
                  "All 8 scene, average recall: %s%%" % mean(0), "All 8 scene, average num inliers: %s" % mean(1),
                  "All 8 scene, average num inliers ratio: %s" % mean(2)]


# ---- the margins of the fixture ---------------------------------------------------------------------------------------------------------
def margins(blocks, pairs, gts, gt_flag, k=250, threshold=0.10, C=32):
    """The margins of tests/matching_np.py on the SANITISED rows of the listed pairs, dict(err, gap, zero_slack, point_err, band).

    A row with a component zeroed is no unit vector any more: the reference's 2 - 2 s.t then differs from the squared distance by the
    squares of the zeroed components, and err (the largest difference between the float64 squared distance and either fp32 form)
    includes that.  An all-zero row (an all-NaN one before) is at distance |t|^2 ~ 1 from every row here and at 2 in the reference's
    form, its own nearest row is decided by rounding alone, so it is left out of err and gap and gets a rule of its own: zero_slack =
    the smallest (distance to a zero row - best distance to a non-zero row) over the non-zero rows, either direction.  With zero_slack
    above the error no row's nearest is a zero row in any arithmetic, so a zero row is in no mutual pair whatever it picks."""
    err = perr = 0.0
    gap = band = slack = np.inf
    for p, (a, b) in enumerate(pairs):
        if not gt_flag[p]:
            continue
        S, T = mnp.tail(sanitize(blocks[a], C), k), mnp.tail(sanitize(blocks[b], C), k)
        s, t = S[:, 3:3 + C], T[:, 3:3 + C]
        D = mnp.d2_f64(s, t)
        ls, lt = np.any(s != 0, 1), np.any(t != 0, 1)                  # the rows that are not all zero
        live = np.ix_(ls, lt)
        err = max(err, float(np.abs(D - mnp.d2_f32_chain(s, t))[live].max()), float(np.abs(D - mnp.d2_reference(s, t))[live].max()))
        gap = min(gap, mnp._gap(D[live]))
        if (~lt).any():
            slack = min(slack, float((D[ls][:, ~lt].min(1) - D[live].min(1)).min()))
        if (~ls).any():
            slack = min(slack, float((D[~ls][:, lt].min(0) - D[live].min(0)).min()))
        m = mnp.mutual_pairs(s, t)
        if len(m):
            d64 = np.sqrt(((S[m[:, 0], :3].astype(np.float64) - mnp.move(gts[p], T[m[:, 1], :3])) ** 2).sum(1))
            d32 = np.sqrt(((S[m[:, 0], :3] - mnp.move_f32(gts[p], T[m[:, 1], :3])) ** 2).sum(1, dtype=np.float32))
            perr = max(perr, float(np.abs(d64 - d32).max()))
            band = min(band, float(np.abs(d64 - threshold).min()))
    return dict(err=err, gap=gap, zero_slack=slack, point_err=perr, band=band)


def margins_ok(m, factor=8.0):
    return m["gap"] >= factor * m["err"] and m["zero_slack"] >= factor * m["err"] and m["band"] >= factor * m["point_err"]
