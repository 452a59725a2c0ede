"""TEST INFRASTRUCTURE ONLY.  Seeded inputs of the ICP tests, the host arithmetic that says which cell edge a grid build realises, and
the body of d3feat_amd.icp.icp_pairs for one chunk with the grid's radius as a parameter.

  rigid, single_pass_pairs, branch_pairs   the input builders of tests/test_gpu_icp.py (moved here unchanged);
  rigid_random, sweep_pairs                the recipe of tools/icp_bench.py at 66 000 points, the inputs of tests/golden/icp_sweep.npz
                                           (tools/make_golden_icp.py --sweep), and their SHA-256;
  cell_edge                                nb_cell_budget and nb_prep (csrc/radius_neighbors.hip) restated: every test that claims a
                                           regime (cells coarser or finer than the radius, the one-cell grid) asserts it with this, so
                                           that no test silently stops exercising its branch when a generator changes;
  run_pairs, run_direct, host, rows        one device call through icp.icp_pairs / straight through the C entry point.

Not a test module (no test_ prefix); imported by tests/test_gpu_icp.py, tests/test_gpu_icp_branches.py, tests/test_icp_host.py and
tools/make_golden_icp.py.  Nothing here needs a GPU at import.
"""
import ctypes
import hashlib
import math

import numpy as np

R = 0.125                                   # r and r r are exact in binary: d2 == r r can be hit on purpose
H = R * (1.0 + 2.0 ** -20)                  # the grid's cell edge for that radius (nb_prep)
OUT = ("T", "count", "sumd2", "fitness", "rmse", "iterations", "converged", "nearest")
MAX_BATCH = 255                             # D3F_MAX_BATCH


def rigid(deg, axis, shift):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = shift
    return T


def single_pass_pairs():
    rng = np.random.default_rng(17)
    f32 = np.float32
    pairs = []
    pairs.append((np.zeros((0, 3), f32), np.array([[1.0, 2.0, 3.0]], f32), None))                          # 0 rows against 1
    pairs.append((np.zeros((1, 3), f32), np.array([[R, 0.0, 0.0]], f32), None))                            # 1 row, d2 == r r: excluded
    # 257 rows: 250 random ones, then  [250] three targets at equal d2 (the lowest index wins, and it is not the first in the stack),
    # [251] a target at exactly the radius (excluded, the next one is farther), [252..256] queries far outside the box of the targets
    src = np.concatenate([rng.uniform(0, 1, (250, 3)), [[3.0, 0.5, 0.5], [3.0, 2.0, 0.5]],
                          [[50, 50, 50], [-40, 0.5, 0.5], [0.5, -3.0, 0.5], [0.5, 0.5, 9.0], [1e6, -1e6, 1e6]]]).astype(f32)
    tgt = np.concatenate([[[0.0, 0.0, 0.0]], rng.uniform(0, 1, (292, 3)),
                          [[3.0, 0.5625, 0.5], [3.0625, 0.5, 0.5], [2.9375, 0.5, 0.5], [3.0, 0.5, 0.4375]],
                          [[3.0 + R, 2.0, 0.5], [3.0, 2.1875, 0.5]], [[0.5, 0.5, 0.5]]]).astype(f32)
    pairs.append((src, tgt, None))
    # 700 rows moved by a pure shift so that row 699 lands EXACTLY on the cell boundary x = 3 h (0.25 + t_x in float64, the box of the
    # targets starts at 0); its only correspondence is a radius (less a hair) below, just above the low edge of the neighbouring cell 2.
    # Row 698 the same one cell up, its correspondence a radius (less a hair) above.
    shift = np.eye(4)
    shift[0, 3] = R + 3 * R * 2.0 ** -20
    lo = np.nextafter(np.nextafter(f32(3 * H - R), f32(9)), f32(9))                        # two float32 steps inside the radius
    hi = np.nextafter(np.nextafter(f32((0.25 + R) + shift[0, 3] + R), f32(-9)), f32(-9))
    src = np.concatenate([rng.uniform(0, 1, (698, 3)), [[0.25 + R, 0.5, 2.5], [0.25, 0.5, 2.5]]]).astype(f32)
    tgt = np.concatenate([[[0.0, 0.0, 0.0]], rng.uniform(0, 1, (600, 3)), [[lo, 0.5, 2.5]], [[hi, 0.5, 3.5]]]).astype(f32)
    src[698] = [0.25 + R, 0.5, 3.5]
    pairs.append((src, tgt, shift))
    pairs.append((rng.uniform(0, 1, (300, 3)).astype(f32), rng.uniform(0, 1, (900, 3)).astype(f32), rigid(5.0, (1, 2, 3), (0.02, -0.01, 0.03))))
    return pairs


def branch_pairs(gold):
    rng = np.random.default_rng(23)
    cloud = rng.uniform(0, 2, (500, 3)).astype(np.float32)
    single_src = np.array([[0, 0, 0], [5, 0, 0], [0, 5, 0]], np.float32)
    single_tgt = np.array([[9, 9, 9], [5.05, 0.02, -0.03], [-7, 0, 0]], np.float32)
    return [(gold["src"], gold["tgt"], None),                                          # the golden pair
            (cloud, cloud.copy(), None),                                               # identical clouds: converged at k = 1
            (np.zeros((0, 3), np.float32), cloud[:50], None),                          # an empty source
            (cloud[:300], cloud[:300] + np.float32(10.0), None),                       # 10 m apart: no correspondence at all
            (single_src, single_tgt, None)]                                            # one correspondence: a pure shift


# ---- the sweep-size fixture's inputs ---------------------------------------------------------------------------------------------------
SWEEP = dict(rng_seed=1, sweep_seed=100, n_raw=66000, n_tgt=20000, motion_deg=2.0, motion_shift=10.0, noise=0.01, init_deg=0.3,
             init_shift=0.1, pairs=2)


def rigid_random(rng, deg, shift):
    """tools/icp_bench.py's rigid(rng, deg, shift): a rotation by deg about a random axis and a shift of that length in a random
    direction, the same draws in the same order.  Spelled in scalar arithmetic (math.sin / math.cos, no matrix product), so that the
    bits do not depend on which BLAS kernel a host picks: the fixture records a SHA-256 of what comes out."""
    axis = rng.normal(size=3)
    axis = axis / math.sqrt(float(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]))
    a = math.radians(deg)
    K = [[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]]
    T = np.eye(4)
    for i in range(3):
        for j in range(3):
            kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
            T[i, j] = ((1.0 if i == j else 0.0) + math.sin(a) * K[i][j]) + (1.0 - math.cos(a)) * kk
    d = rng.normal(size=3)
    n = math.sqrt(float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    for i in range(3):
        T[i, 3] = shift * d[i] / n
    return T


def _compose(A, B):
    """A @ B for two 4 x 4 transforms, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in that order."""
    out = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return out


def sweep_pairs():
    """[(src f32[65984, 3], tgt f32[20000, 3], init f64[4, 4])] x 2: tools/icp_bench.py's workload at 66 000 points with the target
    thinned to 20 000 rows.  65 984 source rows are 258 chunks; the targets span 160 x 160 x 9.6 m."""
    from d3feat_amd.utils.synthetic import lidar_sweep
    rng = np.random.default_rng(SWEEP["rng_seed"])
    pairs = []
    for p in range(SWEEP["pairs"]):
        s = lidar_sweep(SWEEP["sweep_seed"] + p, n_raw=SWEEP["n_raw"])
        G = rigid_random(rng, SWEEP["motion_deg"], SWEEP["motion_shift"])
        s64 = s.astype(np.float64)
        moved = np.stack([((G[r, 0] * s64[:, 0] + G[r, 1] * s64[:, 1]) + G[r, 2] * s64[:, 2]) + G[r, 3] for r in range(3)], axis=1)
        t = (moved + rng.normal(scale=SWEEP["noise"], size=s.shape)).astype(np.float32)
        t = np.ascontiguousarray(t[rng.permutation(len(t))][:SWEEP["n_tgt"]])
        init = _compose(rigid_random(rng, SWEEP["init_deg"], SWEEP["init_shift"]), G)
        pairs.append((s, t, init))
    return pairs


def pair_sha256(pair):
    """hex SHA-256 of the bytes of src (f32), tgt (f32) and init (f64[4, 4]) of one pair, in that order."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pair[0], np.float32).tobytes())
    h.update(np.ascontiguousarray(pair[1], np.float32).tobytes())
    h.update(np.ascontiguousarray(pair[2], np.float64).tobytes())
    return h.hexdigest()


# ---- which cell edge a build realises ----------------------------------------------------------------------------------------------------
def cell_edge(target_clouds, grid_radius):
    """The cell edge d3f_neighbor_grid_build(radius = grid_radius) realises for every element of the stacked target clouds -> f64[B]:
    nb_cell_budget (clamp(4 Ns, 2^16, 2^28) cells for the whole call, an equal share per element) and nb_prep (float32 min and max per
    cloud; h = radius (1 + 2^-20), doubled while prod(floor((mx - mn) / h) + 1) exceeds the share) in the kernel's own float64
    expressions.  An empty element gets edge 1; an element that never fits (non-finite rows) the one-cell grid, inv_h = 0: inf here."""
    clouds = [np.asarray(c, np.float32).reshape(-1, 3) for c in target_clouds]
    B = len(clouds)
    Ns = sum(len(c) for c in clouds)
    per = min(max(4 * max(Ns, 1), 1 << 16), 1 << 28) // B
    edges = np.empty(B)
    for b, c in enumerate(clouds):
        if len(c) == 0:
            edges[b] = 1.0
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            mn, mx = c.min(axis=0).astype(np.float64), c.max(axis=0).astype(np.float64)
            h = float(np.float32(grid_radius)) * (1.0 + 1.0 / 1048576.0)
            if not h > 0.0:
                h = 1.0
            edges[b] = np.inf
            for _ in range(64):
                inv_h = 1.0 / h
                tot = 1.0
                for d in range(3):
                    tot *= np.floor((mx[d] - mn[d]) * inv_h) + 1.0
                if tot <= float(per):
                    edges[b] = h
                    break
                h *= 2.0
    return edges


# ---- device calls ------------------------------------------------------------------------------------------------------------------------
def _stack(pairs):
    src = np.concatenate([np.asarray(p[0], np.float32).reshape(-1, 3) for p in pairs])
    tgt = np.concatenate([np.asarray(p[1], np.float32).reshape(-1, 3) for p in pairs])
    init = np.stack([np.eye(4) if p[2] is None else np.asarray(p[2], np.float64) for p in pairs])
    return src, tgt, init


def run_pairs(device, pairs, **kw):
    """pairs: [(src, tgt, init or None)] -> PairICP of ONE icp.icp_pairs call over all of them (host length lists)"""
    import torch
    from d3feat_amd import icp
    src, tgt, init = _stack(pairs)
    return icp.icp_pairs(torch.from_numpy(src).to(device), [len(p[0]) for p in pairs], torch.from_numpy(tgt).to(device),
                         [len(p[1]) for p in pairs], init=init, **kw)


def host(res):
    return {k: res.dev[k].cpu().numpy() for k in OUT}


def rows(pairs):
    return np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(int)


def run_direct(device, pairs, grid_radius, src_lens=None, max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6,
               relative_rmse=1e-6, check_every=8):
    """The body of icp.icp_pairs for ONE chunk (at most 255 pairs) with the radius of the grid build as a parameter -> the eight
    output arrays on the host.  src_lens: the source lengths as they go to the device (default: the pairs' own); they need not add up
    to the rows of the stack -- N_src is the stack's."""
    import torch
    from d3feat_amd import _lib, ops
    lib = _lib.load()
    src, tgt, init = _stack(pairs)
    B, n_src, n_tgt = len(pairs), src.shape[0], tgt.shape[0]
    assert 1 <= B <= MAX_BATCH
    src_d, tgt_d = torch.from_numpy(src).to(device), torch.from_numpy(tgt).to(device)
    sl = torch.tensor([len(p[0]) for p in pairs] if src_lens is None else list(src_lens), dtype=torch.int32, device=device)
    tl = torch.tensor([len(p[1]) for p in pairs], dtype=torch.int32, device=device)
    T0 = torch.from_numpy(np.ascontiguousarray(init[:, :3, :].reshape(B, 12))).to(device)
    crit = (ctypes.c_double * 3)(float(max_correspondence_distance), float(relative_fitness), float(relative_rmse))
    out = dict(T=torch.empty((B, 12), dtype=torch.float64, device=device), nearest=torch.full((n_src,), -1, dtype=torch.int32, device=device))
    for name, dt in (("count", torch.int32), ("sumd2", torch.float64), ("fitness", torch.float64), ("rmse", torch.float64),
                     ("iterations", torch.int32), ("converged", torch.int32)):
        out[name] = torch.empty((B,), dtype=dt, device=device)
    grid = ops.NeighborGrid(tgt_d, tl, grid_radius)
    wsb = lib.d3f_icp_pairs_workspace_bytes(n_src, B)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=device)
    rc = lib.d3f_icp_pairs(grid.mem.data_ptr(), grid.nbytes, n_tgt, src_d.data_ptr() if n_src else None, n_src, sl.data_ptr(), B,
                           T0.data_ptr(), ctypes.addressof(crit), int(max_iteration), int(check_every), out["T"].data_ptr(),
                           *(out[k].data_ptr() for k in ("count", "sumd2", "fitness", "rmse", "iterations", "converged")),
                           out["nearest"].data_ptr() if n_src else None, ws.data_ptr(), wsb, ops._stream(device))
    _lib.check(rc, "icp_pairs")
    torch.cuda.synchronize(device)
    return {k: out[k].cpu().numpy() for k in OUT}
