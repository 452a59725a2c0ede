"""TEST INFRASTRUCTURE ONLY (no tests in it): the calls of tests/test_pair_limit_host.py and tests/test_gpu_pair_limits.py.

Five entry points cap the pair dimension of their grids at CAP = 65535 workgroups and walk the remaining pairs in a loop
`for (p = blockIdx; p < P; p += gridDim)`.  Each builder here returns M = 7 pair KINDS; the call of P pairs made of them is cyclic,
pair p is kind p % 7.  65535 % 7 == 1, so in a call of P_BIG = 65535 + 301 pairs the workgroups 0 .. 300 run a second pair and
the workgroup that ran kind k runs kind (k + 1) % 7 next: every kind is followed by its successor 43 times.  The kinds are ordered
so that the successions the kernels' comments depend on all occur (SUCCESSIONS_* below name them, the host test asserts them), and
so that two successive kinds never have the same result: a workgroup that repeated its first pair would be seen.

Every input keeps the margins of its restatement (matching_np, overlap_np, validation_np, loss_grad_np): asserted by the host test.
"""
import numpy as np

import loss_grad_np as lg
import validation_np as vnp

M = 7
CAP = 65535                   # workgroups in the pair dimension of a grid
P_BIG = CAP + 301             # one entry-point call: 301 workgroups run two pairs
P_MID = 9000                  # more than the Python front ends pass in one call (PAIRS_PER_CALL = 4096), below the cap


def cyclic(rows, P):
    """rows [M, ...] -> [P, ...]: row p is rows[p % M]."""
    rows = np.asarray(rows)
    return np.ascontiguousarray(np.concatenate([rows] * (-(-P // len(rows))))[:P])


def successions(P=P_BIG, m=M, cap=CAP):
    """[(kind of the first pair, kind of the second pair)] of every workgroup of the pair dimension that runs two pairs."""
    return [(w % m, (w + cap) % m) for w in range(max(P - cap, 0))]


# ---- keypoint blocks: d3f_match_pairs, d3f_register_pairs_counts, d3f_register_pairs, d3f_repeatability_pairs ------------------------------
KP_C, KP_K = 16, 320
KP_ROWS = (300, 280, 40, 0, 1)                       # rows of the five blocks: two beyond the 256-rank tile, one inside it, none, one
KP_COUNTS = (5, 300)
KP_THRESHOLD = 0.10
# (source, target) of the seven kinds; -1 and 5 = n_blocks lie outside [0, n_blocks)
KP_PAIRS = ((0, 1), (2, 0), (1, 0), (-1, 5), (4, 4), (0, 3), (0, 2))
KP_FULL, KP_SHORT, KP_OUTSIDE, KP_ONE_ROW, KP_EMPTY = (0, 2, 6), (1,), (3,), (4,), (5,)
# kinds whose source or target has fewer than ransac_n = 3 rows at every count: no hypothesis is drawn, nothing is validated
KP_NO_HYPOTHESES = (3, 4, 5)
SUCCESSIONS_KP = {
    "a full pair before a short one": (0, 1), "a short pair before a full one": (1, 2),
    "rows before a block index outside [0, n_blocks)": (2, 3), "a block index outside before rows": (3, 4),
    "one row before an empty block": (4, 5), "an empty block before rows": (5, 6),
    "hypotheses before none": (2, 3), "none before hypotheses": (5, 6), "the last kind before the first": (6, 0),
}
RANSAC = dict(max_correspondence_distance=0.05, ransac_n=3, edge_similarity=0.9, checker_distance=0.05, max_iteration=300,
              max_validation=5, seed=5)


def _rigid(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-1, 1, 3)
    return T


def keypoint_kinds(seed=0):
    """-> dict(blocks: five f32[n, 3 + 16 + 1] keypoint blocks ([xyz | unit desc | score], ascending score) cut out of one world of
    300 points, each in its own frame; pairs i32[7, 2]; gts f64[7, 3, 4] target -> source (the identity for a pair with an index outside
    the blocks, where it is not read)."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(0, 1, (300, 3))
    wdesc = rng.standard_normal((300, KP_C))
    wdesc /= np.linalg.norm(wdesc, axis=1, keepdims=True)
    blocks, frames = [], []
    for n in KP_ROWS:
        F = _rigid(rng)                                          # the world into the block's frame
        sel = rng.permutation(300)[:n]
        d = wdesc[sel] + 0.05 * rng.standard_normal((n, KP_C))
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
        xyz = world[sel] @ F[:3, :3].T + F[:3, 3] + rng.normal(scale=0.003, size=(n, 3))
        blocks.append(np.concatenate([xyz, d, np.sort(rng.random(n))[:, None]], 1).astype(np.float32))
        frames.append(F)
    gts = []
    for a, b in KP_PAIRS:
        inside = 0 <= a < len(blocks) and 0 <= b < len(blocks)
        gts.append((frames[a] @ np.linalg.inv(frames[b]))[:3] if inside else np.eye(4)[:3])
    return dict(blocks=blocks, pairs=np.asarray(KP_PAIRS, np.int32), gts=np.asarray(gts, np.float64))


# ---- fragments: d3f_overlap_pairs -----------------------------------------------------------------------------------------------------
OV_THRESHOLD = 0.05
OV_LD = 64                                           # shorter than the long source: the kernel keeps to the row
# clouds: 0 the target (300 points), 1 a long source (257), 2 a short source (5), 3 empty, 4 the target 1000 m away
OV_PAIRS = ((1, 0), (2, 0), (4, 0), (0, 1), (3, 0), (0, 2), (-1, 0))
SUCCESSIONS_OV = {
    "a long source before a short one": (0, 1), "overlapping clouds before disjoint boxes": (1, 2), "disjoint boxes before overlapping clouds": (2, 3),
    "overlapping clouds before an empty fragment": (3, 4), "an empty fragment before overlapping clouds": (4, 5),
    "overlapping clouds before an index outside [0, B)": (5, 6), "an index outside before a long source": (6, 0),
}


def overlap_kinds(seed=7):
    """-> dict(clouds: five f32[n, 3], pairs i32[7, 2])"""
    rng = np.random.default_rng(seed)
    tgt = (rng.random((300, 3)) * 0.5).astype(np.float32)
    clouds = [tgt]
    for n in (257, 5):
        clouds.append((tgt[rng.permutation(300)[:n]] + rng.normal(scale=0.02, size=(n, 3))).astype(np.float32))
    clouds.append(np.zeros((0, 3), np.float32))
    clouds.append(tgt + np.float32(1000.0))
    return dict(clouds=clouds, pairs=np.asarray(OV_PAIRS, np.int32))


# ---- training pairs: d3f_validation_pairs, d3f_loss_gradients ------------------------------------------------------------------------------
VP_C, VP_LD = 16, 70                                 # ld_idx = 70: two 64-row tiles, and nmax = 70
VP_RADIUS, VP_KEYPTS_NUM = 0.1, 6                    # the skip rule: n < 3
# n of the seven kinds.  0: both tiles at work, a row named twice (entries 3 and 50 are the same index pair).  1: the second tile has
# nothing to do.  2: n = 70 with an index one past the pair's rows (the rows kernel works on both tiles, the status skips the pair).
# 3: skipped by keypts_num.  4: no entries.  5: n = 71 > nmax.  6: one entry (with keypts_num = 6 the skip rule takes it as well; n = 1
# evaluated as written is tests/test_gpu_validation.py::test_skip_rule_and_tiny_pairs) -- and then the first kind again: 1 before 70.
VP_N = (70, 3, 70, 2, 0, 71, 1)
VP_STATUS = (0, 0, 1, 0, 0, 2, 0)                    # D3F_VP_INDEX_RANGE = 1, D3F_VP_COUNT_RANGE = 2
VP_EVALUATED = (0, 1)                                # the other kinds give the skip tuple and zero gradients
VP_DUPLICATE = (3, 50)                               # entries of kind 0 that are the same (ai, pi)
SUCCESSIONS_VP = {
    "n = 70 before n = 3": (0, 1), "n = 3 before n = 70": (1, 2), "an index outside the rows before a pair under the skip rule": (2, 3),
    "the skip rule before n = 0": (3, 4), "n = 0 before n > nmax": (4, 5), "n > nmax before n = 1": (5, 6), "n = 1 before n = 70": (6, 0),
}


def validation_kinds(seed=300):
    """-> dict(cases: seven (f, s, x, ai, pi) of validation_np.make_case with the lists cut or spoilt as VP_N says; f, s, x: the rows
    of the seven kinds one after the other; anc, pos i32[7, 70]; n i32[7]; row0 i32[8]; planted: per kind (planted_rows, planted_kd)
    for the margins)."""
    cases, planted = [], []
    for k, n in enumerate(VP_N):
        m = min(n, VP_LD) if n >= 3 else 5                           # entries the case is made with (a skipped kind has rows all the same)
        if k == 0:
            for t in range(40):                                      # the first seed that keeps the margins with the duplicate planted
                f, s, x, ai, pi = vnp.make_case(seed + 1000 * t, m, VP_C, noise=0.3, n_anchor=m + 2, n_positive=m + 1)
                i, j = VP_DUPLICATE
                ai[j], pi[j] = ai[i], pi[i]
                try:
                    lg.margins(f, x, ai, pi, VP_RADIUS, VP_C, planted_rows=VP_DUPLICATE, planted_kd=(VP_DUPLICATE,))
                    break
                except AssertionError:
                    continue
            else:
                raise AssertionError("no clean seed")
            case, plant = (f, s, x, ai, pi), (VP_DUPLICATE, (VP_DUPLICATE,))
        else:
            case = lg.clean_case(seed + k, m, VP_C, VP_RADIUS, noise=(1.0 if k == 1 else 0.3), n_anchor=m + 2, n_positive=m + 1)[0]
            plant = ((), ())
        f, s, x, ai, pi = case
        ai, pi = ai[:min(n, m)].copy(), pi[:min(n, m)].copy()
        if VP_STATUS[k] == 1:
            pi[66] = len(f)                                          # one past the pair's rows, in the second tile
        cases.append((f, s, x, ai, pi))
        planted.append(plant)
    anc, pos = np.zeros((M, VP_LD), np.int32), np.zeros((M, VP_LD), np.int32)
    for k, c in enumerate(cases):
        anc[k, :len(c[3])], pos[k, :len(c[3])] = c[3], c[4]
    row0 = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int32)
    f, s, x = (np.ascontiguousarray(np.concatenate([c[i] for c in cases])) for i in range(3))
    return dict(cases=cases, f=f, s=s, x=x, anc=anc, pos=pos, n=np.asarray(VP_N, np.int32), row0=row0, planted=planted)


def validation_call(kinds, P):
    """The cyclic call of P pairs: the rows of the seven kinds tiled, row0 cumulative over them.
    -> (f, s, x, anc, pos, n, row0) as numpy arrays; pair p holds the rows of kind p % 7."""
    reps = -(-P // M)
    R = int(kinds["row0"][-1])
    f, s, x = (np.tile(kinds[k], (reps,) + (1,) * (kinds[k].ndim - 1)) for k in ("f", "s", "x"))
    starts = (np.arange(reps, dtype=np.int64)[:, None] * R + kinds["row0"][None, :M]).reshape(-1)
    row0 = np.concatenate([starts[:P], [starts[P] if P < len(starts) else reps * R]]).astype(np.int32)
    return f, s, x, cyclic(kinds["anc"], P), cyclic(kinds["pos"], P), cyclic(kinds["n"], P), row0
