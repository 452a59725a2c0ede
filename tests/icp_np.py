"""float64 numpy restatement of d3f_icp_pairs (include/d3feat_amd.h), done the slow way: a brute-force nearest search over every
(source, target) couple, the 16 sums in the header's order (so the integer outputs, sum d2 and the centroid / covariance sums have the
device's bits), and the rigid fit by rg_horn's formulation through numpy.linalg.eigh -- or, alternatively, by SVD (Kabsch).  The fit is
the one step whose bits differ from the device's (LAPACK against 12 Jacobi sweeps): the transform is compared within a tolerance, and
the margins recorded here say that such a last-bit difference cannot flip a correspondence or the stop test.

Not a test module (no test_ prefix); imported by tests/test_icp_host.py, tests/test_gpu_icp.py, tests/test_gpu_icp_branches.py,
tools/make_golden_icp.py and tools/icp_bench.py.
"""
import contextlib
import os
import sys
import types

import numpy as np

CHUNK = 256


def move(T, s):
    """p = ((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r], the rows widened f32 -> f64, every operation rounded on its own."""
    s = np.asarray(s, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def _d2(p, t):
    dx, dy, dz = p[:, None, 0] - t[None, :, 0], p[:, None, 1] - t[None, :, 1], p[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest_brute(p, tgt, r):
    """-> (index i64[Ns] (-1: none), d2 f64[Ns], smallest gap nearest / second nearest among matched rows, smallest |d2 - r r|)."""
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    n = p.shape[0]
    if n == 0 or t.shape[0] == 0:
        return np.full(n, -1, np.int64), np.zeros(n), np.inf, np.inf
    r2 = np.float64(r) * np.float64(r)
    idx, best = np.empty(n, np.int64), np.empty(n)
    gap_nn, gap_r = np.inf, np.inf
    for a in range(0, n, 512):                       # blocks of rows: the matrix of every couple never exceeds a few MB
        D = _d2(p[a:a + 512], t)
        j = np.argmin(D, axis=1)                     # the first minimum = the lowest index among equal d2
        b = D[np.arange(D.shape[0]), j]
        idx[a:a + 512], best[a:a + 512] = j, b
        gap_r = min(gap_r, float(np.min(np.abs(D - r2))))
        if t.shape[0] > 1 and np.any(b < r2):
            D[np.arange(D.shape[0]), j] = np.inf
            gap_nn = min(gap_nn, float(np.min((np.min(D, axis=1) - b)[b < r2])))
    ok = best < r2                                   # STRICT
    return np.where(ok, idx, -1), np.where(ok, best, 0.0), gap_nn, gap_r


def nearest_ckdtree(p, tgt, r):
    """The same correspondences through scipy's k-d tree (the bench's host comparison, and the only search that is affordable at sweep
    size): the tree proposes its two nearest targets, the header's d2 decides between them -- among equal d2 the lower index, as
    nearest_brute.  The margins: margin_nn = the smallest (second d2 - first d2) over matched rows, the same number nearest_brute
    gives as long as the tree's two proposals are the two nearest by the header's d2 (they can only fail to be where the margin is
    within rounding of 0 anyway); margin_r = the smallest |d2 of the nearest - r r| over ALL rows: only the nearest target of a row can
    change whether the row counts, so this is never below nearest_brute's minimum over every couple."""
    from scipy.spatial import cKDTree
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    n = p.shape[0]
    if n == 0 or t.shape[0] == 0:
        return np.full(n, -1, np.int64), np.zeros(n), np.inf, np.inf
    k = min(2, t.shape[0])
    _, j = cKDTree(t).query(p, k=k)
    j = np.asarray(j).reshape(n, k)
    d = p[:, None, :] - t[j]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if k == 2:
        swap = (d2[:, 1] < d2[:, 0]) | ((d2[:, 1] == d2[:, 0]) & (j[:, 1] < j[:, 0]))
        j = np.where(swap[:, None], j[:, ::-1], j)
        d2 = np.where(swap[:, None], d2[:, ::-1], d2)
    r2 = np.float64(r) * np.float64(r)
    ok = d2[:, 0] < r2
    gap_nn = float(np.min((d2[:, 1] - d2[:, 0])[ok])) if k == 2 and ok.any() else np.inf
    gap_r = float(np.min(np.abs(d2[:, 0] - r2)))
    return np.where(ok, j[:, 0], -1), np.where(ok, d2[:, 0], 0.0), gap_nn, gap_r


def _halve(x, s0):
    """the halving tree s = s0, s0 / 2, .. 1 along the last axis: x[t] += x[t + s] for t < s -> x[..., 0]"""
    x = x.copy()
    s = s0
    while s > 0:
        x[..., :s] = x[..., :s] + x[..., s:2 * s]
        s //= 2
    return x[..., 0]


def sums(p, tgt, idx, d2):
    """The 16 sums in the header's order -> (f64[16], count)."""
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    n = p.shape[0]
    ok = idx >= 0
    v = np.zeros((n, 16))
    if n and ok.any():
        x = t[np.where(ok, idx, 0)]
        v[:, 0] = d2
        v[:, 1:4] = p
        v[:, 4:7] = x
        for a in range(3):
            for b in range(3):
                v[:, 7 + 3 * a + b] = p[:, a] * x[:, b]
        v[~ok] = 0.0                                 # a row without a correspondence adds +0.0 to every sum
    nc = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((nc * CHUNK, 16))
    pad[:n] = v
    g = _halve(pad.reshape(nc, 4, 64, 16).transpose(0, 1, 3, 2), 32)          # [nc, 4, 16]
    part = (g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])                           # [nc, 16]
    acc = np.zeros((256, 16))
    for c in range(nc):                               # partial t: chunks t, t + 256, ... in ascending order from 0.0
        acc[c % 256] = acc[c % 256] + part[c]
    return _halve(acc.T, 128), int(ok.sum())


def horn_matrix(S):
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def rotation_eigh(S):
    """rg_horn's formulation: the unit quaternion = the eigenvector of the largest eigenvalue of N(S), by LAPACK."""
    w, V = np.linalg.eigh(horn_matrix(S))
    q = V[:, np.argmax(w)]
    w_, x, y, z = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                     [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                     [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])


def rotation_svd(S):
    """Kabsch: the rotation maximising sum x_i . R p_i for S = sum (p - mp)(x - mt)^T."""
    U, _, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T


def update(T, sm, n, fit="eigh"):
    """T_{k+1} = U T_k from the 16 sums, in the header's operation order."""
    if n == 0:
        return T.copy()
    dn = np.float64(n)
    mp, mt = sm[1:4] / dn, sm[4:7] / dn
    S = np.array([[sm[7 + 3 * a + b] - sm[1 + a] * mt[b] for b in range(3)] for a in range(3)])
    R = rotation_eigh(S) if fit == "eigh" else rotation_svd(S)
    tu = np.array([mt[a] - ((R[a, 0] * mp[0] + R[a, 1] * mp[1]) + R[a, 2] * mp[2]) for a in range(3)])
    O = np.empty((3, 4))
    for a in range(3):
        for c in range(4):
            O[a, c] = (R[a, 0] * T[0, c] + R[a, 1] * T[1, c]) + R[a, 2] * T[2, c]
        O[a, 3] = O[a, 3] + tu[a]
    return O


def icp(src, tgt, init=None, max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6, relative_rmse=1e-6, fit="eigh",
        nearest=nearest_brute):
    """One pair -> namespace(T f64[4,4], count, sumd2, fitness, rmse, iterations, converged, nearest i64[Ns], margin_nn, margin_r,
    margin_stop).  The margins are the smallest, over all rounds, of: the gap between the nearest and the second-nearest d2 of a
    matched row; |d2 - r r| over every couple; and the distance of |rmse_k - rmse_{k-1}| and |fitness_k - fitness_{k-1}| from their
    thresholds."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    T = np.eye(4)[:3].copy() if init is None else np.array(np.asarray(init, np.float64).reshape(-1, 4)[:3])
    ns = src.shape[0]
    m_nn, m_r, m_stop = np.inf, np.inf, np.inf
    fit_prev = rms_prev = np.float64(0.0)
    k = 0
    while True:
        p = move(T, src)
        idx, d2, g_nn, g_r = nearest(p, tgt, max_correspondence_distance)
        m_nn, m_r = min(m_nn, g_nn), min(m_r, g_r)
        sm, n = sums(p, tgt, idx, d2)
        fitness = np.float64(n) / np.float64(ns) if ns > 0 else np.float64(0.0)
        rmse = np.sqrt(sm[0] / np.float64(n)) if n > 0 else np.float64(0.0)
        if k >= 1:
            m_stop = min(m_stop, abs(abs(fitness - fit_prev) - relative_fitness), abs(abs(rmse - rms_prev) - relative_rmse))
        if k >= 1 and abs(fitness - fit_prev) < relative_fitness and abs(rmse - rms_prev) < relative_rmse:
            converged = 1
            break
        if k >= max_iteration:
            converged = 0
            break
        T = update(T, sm, n, fit)
        fit_prev, rms_prev = fitness, rmse
        k += 1
    T4 = np.eye(4)
    T4[:3] = T
    return types.SimpleNamespace(T=T4, count=n, sumd2=float(sm[0]), fitness=float(fitness), rmse=float(rmse), iterations=k,
                                 converged=converged, nearest=idx, margin_nn=m_nn, margin_r=m_r, margin_stop=m_stop)


class PairsNP:
    """What d3feat_amd.icp.icp_pairs returns, computed by the restatement (the host tests put it in the device call's place)."""

    def __init__(self, runs):
        self.runs = runs
        self.transformation = np.stack([r.T for r in runs]) if runs else np.zeros((0, 4, 4))
        self.fitness = np.array([r.fitness for r in runs])
        self.inlier_rmse = np.array([r.rmse for r in runs])
        self.iterations = np.array([r.iterations for r in runs], np.int32)
        self.converged = np.array([r.converged for r in runs], bool)
        self.count = np.array([r.count for r in runs], np.int32)
        self.sumd2 = np.array([r.sumd2 for r in runs])

    def correspondences(self, p):
        nn = self.runs[p].nearest
        i = np.nonzero(nn >= 0)[0]
        return np.stack([i, nn[i]], axis=1).astype(np.int32)


def icp_pairs(src, src_lens, tgt, tgt_lens, init=None, check_every=8, **kw):
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    so, to = np.concatenate([[0], np.cumsum(src_lens)]).astype(int), np.concatenate([[0], np.cumsum(tgt_lens)]).astype(int)
    runs = []
    for p in range(len(src_lens)):
        T0 = None if init is None else np.asarray(init, np.float64)[p]
        runs.append(icp(src[so[p]:so[p + 1]], tgt[to[p]:to[p + 1]], T0, **kw))
    return PairsNP(runs)


@contextlib.contextmanager
def compat_open3d(root):
    """`import open3d` resolving to compat/open3d for the length of a with block (and gone from sys.modules afterwards)."""
    path = os.path.join(root, "compat")
    drop = lambda: [sys.modules.pop(k) for k in list(sys.modules) if k == "open3d" or k.startswith("open3d.")]
    drop()
    sys.path.insert(0, path)
    try:
        import open3d
        yield open3d
    finally:
        sys.path.remove(path)
        drop()
