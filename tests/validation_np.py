"""TEST INFRASTRUCTURE ONLY.  Float64 restatement of the validation figures (d3feat_amd/validation.py; models/KPFCNN_model.py:131-186
and utils/loss.py of the reference): the whole n x n matrices, no tiling, no fp32 anywhere -- the oracle of tests/test_validation_host.py
and tests/test_gpu_validation.py, with the tolerances derived from the case and the margins an input must keep so that the COUNTS
(accuracy, the false-negative mask) are the same in fp32 and float64.
"""
import numpy as np

POS_MARGIN, NEG_MARGIN, LOG_SCALE = 0.1, 1.4, 25.0
SKIP = (0.0, 0.0, 0.0, -1.0, 0.0, 0.0)          # circle, contrastive, det, accuracy, d_pos, d_neg
U = 2.0 ** -24


def matrices(f, x, ai, pi):
    """D (descriptors of ai against pi) and KD (points of ai against ai), float64 [n, n] (64 rows at a time: n n C differences)."""
    f, x = np.asarray(f, np.float64), np.asarray(x, np.float64)
    a, b, k = f[ai], f[pi], x[ai]
    D = np.concatenate([np.sqrt(((a[i:i + 64, None, :] - b[None, :, :]) ** 2).sum(-1) + 1e-12) for i in range(0, len(a), 64)])
    KD = np.sqrt(((k[:, None, :] - k[None, :, :]) ** 2).sum(-1) + 1e-12)
    return D, KD


def softplus(x):
    return np.logaddexp(0.0, x)


def figures(f, s, x, ai, pi, safe_radius, keypts_num, det_loss_weight=1.0, q=POS_MARGIN, m=NEG_MARGIN, L=LOG_SCALE):
    """-> dict(circle, contrastive, det, accuracy, d_pos, d_neg, accurate, n, fp, cn, lse, Dmax, smax): the definition, in float64."""
    ai, pi = np.asarray(ai, np.int64), np.asarray(pi, np.int64)
    n = len(ai)
    if n == 0 or n < 0.5 * keypts_num:
        return dict(zip(("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg"), SKIP), accurate=0, n=n, skipped=True)
    D, KD = matrices(f, x, ai, pi)
    s = np.asarray(s, np.float64).reshape(-1)
    eye = np.eye(n, dtype=bool)
    FN = (KD < np.float64(np.float32(safe_radius))) & ~eye
    fp = np.diag(D).copy()
    cn = (D + 1e5 * eye).min(1)
    z = np.where(eye | FN | (D >= m), 0.0, L * (m - D) ** 2)
    lse = np.log(np.exp(z).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        d_neg = (D * (~eye & ~FN)).mean() * n / (n - 1.0)
    sab = s[ai] + s[pi] + 1e-6
    return dict(circle=(softplus(L * (fp - q) + lse) / L).mean(),
                contrastive=(np.maximum(fp - q, 0) + np.maximum(m - cn, 0)).mean(),
                det=det_loss_weight * ((fp - cn) * sab).mean() if det_loss_weight != 0 else 0.0,
                accuracy=float((fp - cn <= 0).sum()) / n, d_pos=fp.mean(), d_neg=d_neg, accurate=int((fp - cn <= 0).sum()), n=n,
                skipped=False, fp=fp, cn=cn, lse=lse, Dmax=float(D.max()), smax=float(np.abs(sab).max()),
                masked=float(FN.sum()) / max(n * n - n, 1), D=D, KD=KD)


def tolerances(C, Dmax, smax, m=NEG_MARGIN):
    """Absolute bounds of the fp32 evaluation against float64, from the case: gamma = (C + 4) 2^-24 bounds the relative error of a
    C-term squared-difference chain and its root; lse and softplus are 1-Lipschitz and |dz/dD| <= 2 L m."""
    g = (C + 4) * U
    d = 2 * g * Dmax
    return dict(circle=d * (1 + 2 * m), contrastive=d * (1 + 2 * m), det=4 * g * Dmax * smax, d_pos=d, d_neg=d, dist=d)


def margins(f, x, ai, pi, safe_radius, C, planted_rows=(), planted_kd=(), DKD=None):
    """Asserts what makes the counts of a test input the same in fp32 and float64: no row has |fp - cn| inside 4 gamma Dmax (rows with
    a planted exact tie excepted) and no off-diagonal KD lies inside 8 * 7 * 2^-24 r of r (planted entries excepted).  -> (the smallest
    |fp - cn| over the other rows, the smallest |KD - r| / r)."""
    ai, pi = np.asarray(ai, np.int64), np.asarray(pi, np.int64)
    n = len(ai)
    D, KD = DKD if DKD is not None else matrices(f, x, ai, pi)
    eye = np.eye(n, dtype=bool)
    g = (C + 4) * U
    gap = np.abs(np.diag(D) - (D + 1e5 * eye).min(1))
    keep = np.ones(n, bool)
    keep[list(planted_rows)] = False
    band = 4 * g * D.max()
    assert not (gap[keep] <= band).any(), "a row has |fp - cn| = %.3e inside the band %.3e: change the seed" % (gap[keep].min(), band)
    r = float(np.float32(safe_radius))
    off = ~eye
    for (i, j) in planted_kd:
        off[i, j] = off[j, i] = False
    rel = np.abs(KD[off] - r) / r if off.any() else np.asarray([np.inf])
    assert not (rel <= 8 * 7 * U).any(), "an off-diagonal KD lies %.3e r from r: change the seed" % rel.min()
    return float(gap[keep].min()) if keep.any() else np.inf, float(rel.min())


def split_means(rows):
    """rows: per pair (desc, det, accuracy, d_pos, d_neg) -> the means of utils/trainer.py:442-452, 467-471."""
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    out = []
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        for k in range(5):
            v = rows[:, k]
            buf = v[v > 0] if k == 2 else v[v != 0]
            out.append(float(np.mean(buf)) if len(buf) else float("nan"))
    return tuple(out)


def make_case(seed, n, C, cube=0.4, n_anchor=None, n_positive=None, noise=0.3):
    """One pair: unit descriptors, positives b = normalize(a + noise * gaussian) in a shuffled row order, points uniform in a cube of
    `cube` metres, scores in (0.05, 1).  -> f [N, C], s [N], x [N, 3] float32, ai, pi int32 (pi shifted by the anchor's length)."""
    rng = np.random.default_rng(seed)
    na = n_anchor if n_anchor is not None else n + 7
    nb = n_positive if n_positive is not None else n + 5
    fa = rng.standard_normal((na, C))
    fa /= np.linalg.norm(fa, axis=1, keepdims=True)
    fb = rng.standard_normal((nb, C))
    fb /= np.linalg.norm(fb, axis=1, keepdims=True)
    ai = rng.permutation(na)[:n]
    pj = rng.permutation(nb)[:n]
    b = fa[ai] + noise * rng.standard_normal((n, C)) / np.sqrt(C)          # (noise of norm about `noise`)
    fb[pj] = b / np.linalg.norm(b, axis=1, keepdims=True)
    x = rng.uniform(0, cube, (na + nb, 3))
    s = rng.uniform(0.05, 1.0, na + nb)
    f = np.concatenate([fa, fb]).astype(np.float32)
    return f, s.astype(np.float32), x.astype(np.float32), ai.astype(np.int32), (pj + na).astype(np.int32)


def clean_case(seed, n, C, safe_radius, keypts_num=2, det_loss_weight=1.0, **kw):
    """make_case(seed, ...) with the first seed from `seed` on (steps of 1000) whose input keeps the margins: "change the seed, not the
    band".  -> (f, s, x, ai, pi), figures, (smallest |fp - cn|, smallest |KD - r| / r)."""
    for k in range(20):
        case = make_case(seed + 1000 * k, n, C, **kw)
        want = figures(*case, safe_radius, keypts_num, det_loss_weight)
        if want["skipped"] or n < 2:
            return case, want, (np.inf, np.inf)
        try:
            return case, want, margins(case[0], case[2], case[3], case[4], safe_radius, C, DKD=(want["D"], want["KD"]))
        except AssertionError:
            continue
    raise AssertionError("no clean seed found from %d on" % seed)
