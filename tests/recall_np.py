"""The registration recall of the 3DMatch benchmark in numpy, twice (no GPU, no library):

  (a) device(...)    the definition of d3f_registration_recall (include/d3feat_amd.h) in float64, operation by operation: element-wise
                     numpy products, sums, quotients and square roots only, each rounded on its own, in the order the header writes
                     down -- what the kernel must give bit for bit;
  (b) matlab(...)    external/ElasticReconstruction/mrEvaluateRegistration.m of the reference line by line, with np.linalg.inv and @
                     where the .m file has ^ -1 and * -- the figure the papers quote, up to the summation order of a BLAS.

Both take the rows of registration.registration_recall: T f32[P, n, 3, 4] (source -> target, inverted here as evaluate.py:104 logs it)
or, with logged=True, f64[P, n, 4, 4]; gt f64[P, 4, 4]; info f64[P, 6, 6]; gt_flag, result_flag (None: gt_flag), ids [P, 2];
scene_start.  -> dict(error f64[P, n], flags i32[P, n], figures i64[S, n, 5])."""
import numpy as np

GOOD, RESULT, FALSE_POS, GT = 1, 2, 4, 8
ERR2 = 0.04


# ---- (a) the device definition --------------------------------------------------------------------------------------------------------
def invert(a):
    """a f64[..., >= 3, 4] affine rows [A | t] -> f64[..., 3, 4], the inverse [B | u] by cofactors over the determinant."""
    a = np.asarray(a, np.float64)
    e = lambda r, c: a[..., r, c]
    n = lambda x, y, z, w: e(*x) * e(*y) - e(*z) * e(*w)
    num = [[n((1, 1), (2, 2), (1, 2), (2, 1)), n((0, 2), (2, 1), (0, 1), (2, 2)), n((0, 1), (1, 2), (0, 2), (1, 1))],
           [n((1, 2), (2, 0), (1, 0), (2, 2)), n((0, 0), (2, 2), (0, 2), (2, 0)), n((0, 2), (1, 0), (0, 0), (1, 2))],
           [n((1, 0), (2, 1), (1, 1), (2, 0)), n((0, 1), (2, 0), (0, 0), (2, 1)), n((0, 0), (1, 1), (0, 1), (1, 0))]]
    det = (e(0, 0) * num[0][0] + e(0, 1) * num[1][0]) + e(0, 2) * num[2][0]
    out = np.empty(a.shape[:-2] + (3, 4), np.float64)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                out[..., r, c] = num[r][c] / det
            out[..., r, 3] = -((out[..., r, 0] * e(0, 3) + out[..., r, 1] * e(1, 3)) + out[..., r, 2] * e(2, 3))
    return out


def transformation_error(result, gt, info):
    """result f64[N, 3, 4] (the log's matrix), gt f64[N, >= 3, 4], info f64[N, 6, 6] -> p f64[N] of the header, NaN where s > 0 is false."""
    G, R, I = invert(gt), np.asarray(result, np.float64), np.asarray(info, np.float64)
    with np.errstate(all="ignore"):
        E = np.empty(R.shape[:-2] + (3, 4), np.float64)
        for r in range(3):
            for c in range(4):
                v = (G[..., r, 0] * R[..., 0, c] + G[..., r, 1] * R[..., 1, c]) + G[..., r, 2] * R[..., 2, c]
                E[..., r, c] = v + G[..., r, 3] if c == 3 else v
        s = ((1.0 + E[..., 0, 0]) + E[..., 1, 1]) + E[..., 2, 2]
        ok = s > 0.0
        d = 4.0 * (0.5 * np.sqrt(np.where(ok, s, 1.0)))
        er = [E[..., 0, 3], E[..., 1, 3], E[..., 2, 3], (E[..., 2, 1] - E[..., 1, 2]) / d, (E[..., 0, 2] - E[..., 2, 0]) / d,
              (E[..., 1, 0] - E[..., 0, 1]) / d]
        num = None
        for r in range(6):
            v = I[..., r, 0] * er[0]
            for c in range(1, 6):
                v = v + I[..., r, c] * er[c]
            t = er[r] * v
            num = t if num is None else num + t
        p = num / I[..., 0, 0]
    return np.where(ok, p, np.nan)


def _layout(T, logged, gt_flag, result_flag, ids):
    T = np.asarray(T)
    tail = (4, 4) if logged else (3, 4)
    assert T.dtype == (np.float64 if logged else np.float32) and T.shape[-2:] == tail and T.ndim in (3, 4)
    T = T.reshape((T.shape[0], T.shape[1] if T.ndim == 4 else 1) + tail)
    g = np.asarray(gt_flag) != 0
    r = g if result_flag is None else np.asarray(result_flag) != 0
    ids = np.asarray(ids).reshape(-1, 2)
    return T, g, r, (ids[:, 1].astype(np.int64) - ids[:, 0]) > 1


def _finish(p, g, r, apart, scene_start, err2, n):
    P = len(g)
    both = (g & r & apart)[:, None]
    error = np.where(both, p, 0.0)
    with np.errstate(invalid="ignore"):
        good = both & (p <= err2)
    per_pair = (r & apart) * RESULT + (r & apart & ~g) * FALSE_POS + (g & apart) * GT
    flags = (good * GOOD + per_pair[:, None]).astype(np.int32).reshape(P, n)
    S = len(scene_start) - 1
    figures = np.zeros((S, n, 5), np.int64)
    for s in range(S):
        f = flags[int(scene_start[s]):int(scene_start[s + 1])]
        figures[s, :, 0] = ((f & GOOD) != 0).sum(0)
        figures[s, :, 1] = ((f & (GOOD | RESULT | FALSE_POS)) == RESULT).sum(0)
        figures[s, :, 2] = ((f & FALSE_POS) != 0).sum(0)
        figures[s, :, 3] = ((f & GT) != 0).sum(0)
        figures[s, :, 4] = ((f & RESULT) != 0).sum(0)
    return dict(error=error, flags=flags, figures=figures)


def device(T, gt, info, gt_flag, ids, scene_start, err2=ERR2, result_flag=None, logged=False):
    T, g, r, apart = _layout(T, logged, gt_flag, result_flag, ids)
    P, n = T.shape[:2]
    gt, info = np.asarray(gt, np.float64).reshape(P, 4, 4), np.asarray(info, np.float64).reshape(P, 6, 6)
    result = T[:, :, :3] if logged else invert(T.astype(np.float64))
    p = np.stack([transformation_error(result[:, c], gt, info) for c in range(n)], 1) if n else np.zeros((P, 0))
    return _finish(p, g, r, apart, scene_start, err2, n)


# ---- (b) the .m files ------------------------------------------------------------------------------------------------------------------
def dcm2quat(DCM):
    """mrEvaluateRegistration.m:51-59"""
    q = np.zeros(4)
    q[0] = 0.5 * np.sqrt(1 + DCM[0, 0] + DCM[1, 1] + DCM[2, 2])
    q[1] = -(DCM[2, 1] - DCM[1, 2]) / (4 * q[0])
    q[2] = -(DCM[0, 2] - DCM[2, 0]) / (4 * q[0])
    q[3] = -(DCM[1, 0] - DCM[0, 1]) / (4 * q[0])
    return q


def compute_transformation_error(trans, info):
    """mrEvaluateRegistration.m:44-49"""
    te = trans[0:3, 3]
    qt = dcm2quat(trans[0:3, 0:3])
    er = np.concatenate([te, -qt[1:4]])
    return er @ info @ er / info[0, 0]


def matlab(T, gt, info, gt_flag, ids, scene_start, err2=ERR2, result_flag=None, logged=False):
    """Row by row as mrEvaluateRegistration.m:21-37 walks the results; the result matrix of a float32 estimate is np.linalg.inv of its
    float64 4x4, the matrix results.write_registration_log writes."""
    T, g, r, apart = _layout(T, logged, gt_flag, result_flag, ids)
    P, n = T.shape[:2]
    gt, info = np.asarray(gt, np.float64).reshape(P, 4, 4), np.asarray(info, np.float64).reshape(P, 6, 6)
    p = np.zeros((P, n))
    with np.errstate(all="ignore"):
        for i in range(P):
            if not (g[i] and r[i] and apart[i]):
                continue
            for c in range(n):
                if logged:
                    trans = T[i, c]
                else:
                    M = np.eye(4)
                    M[:3] = T[i, c].astype(np.float64)
                    trans = np.linalg.inv(M)
                p[i, c] = compute_transformation_error(np.linalg.inv(gt[i]) @ trans, info[i])
    return _finish(p, g, r, apart, scene_start, err2, n)


def summary(figures):
    """[scene][count] -> dict as registration.SceneRecall.scenes()"""
    out = []
    for per in figures:
        row = []
        for good, bad, fpos, gtn, rsn in per.tolist():
            row.append(dict(good=good, bad=bad, false_pos=fpos, gt_num=gtn, rs_num=rsn, recall=good / gtn if gtn else 0.0,
                            precision=good / rsn if rsn else 0.0))
        out.append(row)
    return out
