"""Seeded synthetic inputs shaped like the reference's workloads -- host-side numpy only.

    room_fragment(seed)       config #2: a 3DMatch-like indoor fragment (surfaces, not volumes): points on the six
                              faces of a box plus three spheres standing on the floor, Gaussian jitter; ~300k raw
                              points that grid-subsample to ~30k at 0.03 m.
    lidar_sweep(seed)         config #4a: a KITTI-like 64-ring sweep over a ground plane with boxes.
"""
import numpy as np


def room_fragment(seed=0, n_raw=300000, edge=1.68, jitter=0.002):
    rng = np.random.Generator(np.random.PCG64(seed))
    ex, ey, ez = edge * (1.0 + 0.05 * rng.random()), edge * (1.0 + 0.05 * rng.random()), edge * 0.8
    n_box = int(n_raw * 0.88)
    face = rng.integers(0, 6, n_box)
    uv = rng.random((n_box, 2))
    pts = np.empty((n_box, 3))
    ax = face // 2
    side = face % 2
    ext = np.array([ex, ey, ez])
    for a in range(3):
        m = ax == a
        o = [d for d in range(3) if d != a]
        pts[m, a] = side[m] * ext[a]
        pts[m, o[0]] = uv[m, 0] * ext[o[0]]
        pts[m, o[1]] = uv[m, 1] * ext[o[1]]
    n_sph = n_raw - n_box
    # sphere centres keep 0.5 m from the walls (rooms narrower than 1 m: on the centre line); same draws for edge >= 1
    centers = np.stack([rng.uniform(min(0.5, ex / 2), max(ex - 0.5, ex / 2), 3),
                        rng.uniform(min(0.5, ey / 2), max(ey - 0.5, ey / 2), 3), np.full(3, 0.3)], 1)
    which = rng.integers(0, 3, n_sph)
    d = rng.standard_normal((n_sph, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sph = centers[which] + 0.3 * d
    allp = np.concatenate([pts, sph], 0)
    allp += rng.normal(scale=jitter, size=allp.shape)
    allp = allp[rng.permutation(allp.shape[0])]
    return allp.astype(np.float32)


def lidar_sweep(seed=0, n_raw=120000, rings=64):
    rng = np.random.Generator(np.random.PCG64(seed))
    per = n_raw // rings
    az = rng.uniform(-np.pi, np.pi, (rings, per))
    el = np.linspace(np.deg2rad(-24.8), np.deg2rad(2.0), rings)[:, None] + np.zeros((1, per))
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    h = 1.73
    t_ground = np.where(dirs[:, 2] < -1e-3, -h / np.minimum(dirs[:, 2], -1e-3), 120.0)
    t = np.minimum(t_ground, 80.0)
    # axis-aligned boxes (cars / walls): slab intersection
    nb = 24
    c = np.stack([rng.uniform(-50, 50, nb), rng.uniform(-50, 50, nb), np.full(nb, -h + 0.8)], 1)
    s = np.stack([rng.uniform(1, 4, nb), rng.uniform(1, 8, nb), rng.uniform(0.7, 2.5, nb)], 1)
    for i in range(nb):
        lo, hi = c[i] - s[i], c[i] + s[i]
        with np.errstate(divide='ignore', invalid='ignore'):
            t1, t2 = lo / dirs, hi / dirs
        tn = np.max(np.minimum(t1, t2), axis=1)
        tf = np.min(np.maximum(t1, t2), axis=1)
        hit = (tn < tf) & (tn > 1.0)
        t = np.where(hit & (tn < t), tn, t)
    pts = dirs * t[:, None]
    pts += rng.normal(scale=0.01, size=pts.shape)
    return pts.astype(np.float32)


def scene(seed, n_frag=8, K=250, edge=3.0, crop=1.1, noise=0.003, dnoise=0.05, outliers=0.3):
    """n_frag keypoint blocks [xyz | 32-d unit desc | score] cut out of ONE room, each in its own frame; poses[f] takes
    fragment f into the world.  gt for pair (a, b), target -> source: inv(poses[a]) @ poses[b]."""
    rng = np.random.default_rng(seed)
    world = room_fragment(seed, n_raw=40000, edge=edge).astype(np.float64)
    wdesc = rng.standard_normal((len(world), 32)); wdesc /= np.linalg.norm(wdesc, axis=1, keepdims=True)
    wscore = rng.random(len(world))
    lo, hi = world.min(0), world.max(0)
    cent = lo + (hi - lo) * (0.25 + 0.5 * rng.random((n_frag, 3)))
    blocks, poses = [], []
    for f in range(n_frag):
        inside = np.nonzero(np.linalg.norm(world - cent[f], axis=1) < crop)[0]
        s = wscore[inside] + 0.15 * rng.random(len(inside))      # detection repeats across fragments, not exactly
        sel = inside[np.argsort(s, kind="stable")[-K:]]
        q, _ = np.linalg.qr(rng.standard_normal((3, 3))); R = q * np.sign(np.linalg.det(q)); t = rng.uniform(-1, 1, 3)
        xyz = (world[sel] - t) @ R + rng.normal(scale=noise, size=(len(sel), 3))
        d = wdesc[sel] + dnoise * rng.standard_normal((len(sel), 32))
        bad = rng.random(len(sel)) < outliers
        d[bad] = rng.standard_normal((int(bad.sum()), 32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        sc = np.sort(rng.random(len(sel)))
        blocks.append(np.concatenate([xyz, d, sc[:, None]], 1).astype(np.float32))
        M = np.eye(4); M[:3, :3] = R; M[:3, 3] = t
        poses.append(M)
    return blocks, poses


def overlap_scene(seed, n_frag=6, n_raw=12000, thr=0.05, edge=3.0, half_width=0.32, keep=0.55):
    """n_frag fragments of ONE room, all in the room's frame, that overlap their neighbours along x (the input of overlap.overlap_pairs):
    fragment f is the slab |x - c_f| < half_width * (x extent) of room_fragment(seed, n_raw, edge), c_f running from 15 % to 85 % of
    the x extent; every point of the slab is kept with probability `keep` and moved by Gaussian noise of 0.3 thr / sqrt(3) per axis (a
    surface sampled again, not the same points), then cast to float32.  -> list of f32[n_f, 3]."""
    rng = np.random.default_rng(seed)
    world = room_fragment(seed, n_raw=n_raw, edge=edge).astype(np.float64)
    lo, ext = world[:, 0].min(), world[:, 0].max() - world[:, 0].min()
    out = []
    for c in lo + ext * np.linspace(0.15, 0.85, n_frag):
        inside = np.nonzero(np.abs(world[:, 0] - c) < half_width * ext)[0]
        sel = inside[rng.random(len(inside)) < keep]
        out.append((world[sel] + rng.normal(scale=0.3 * thr / np.sqrt(3.0), size=(len(sel), 3))).astype(np.float32))
    return out


def keypoint_pairs(seed, n_pairs=3, K=64, C=32, extent=20.0, noise=0.03, dnoise=0.1, outliers=0.2):
    """Keypoint blocks [xyz | C-d unit desc | score] (ascending score) of n_pairs pairs of frames at the scale of a KITTI sweep: block
    2i + 1 is block 2i moved by a known motion of a few metres and degrees, re-noised, a share `outliers` of its rows replaced, its
    rows in another order.  -> (kp f32[2 n_pairs, K, C + 4], gt f32[n_pairs, 3, 4] taking block 2i into the frame of block 2i + 1)."""
    rng = np.random.default_rng(seed)
    kp, gt = np.zeros((2 * n_pairs, K, C + 4), np.float32), np.zeros((n_pairs, 3, 4), np.float32)
    for i in range(n_pairs):
        xyz = rng.uniform(-extent, extent, (K, 3)) * [1, 1, 0.1]
        desc = rng.standard_normal((K, C))
        a = rng.normal(size=3) * [0.1, 0.1, 1]
        a /= np.linalg.norm(a)
        th = np.deg2rad(rng.uniform(1, 15))
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R, t = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx), rng.normal(size=3) * [4, 1, 0.1]
        xyz1, desc1 = xyz @ R.T + t + rng.normal(scale=noise, size=xyz.shape), desc + dnoise * rng.standard_normal(desc.shape)
        out = rng.random(K) < outliers
        xyz1[out], desc1[out] = rng.uniform(-extent, extent, (int(out.sum()), 3)), rng.standard_normal((int(out.sum()), C))
        perm = rng.permutation(K)
        for b, (x, d) in enumerate(((xyz, desc), (xyz1[perm], desc1[perm]))):
            d = d / np.linalg.norm(d, axis=1, keepdims=True)
            kp[2 * i + b] = np.concatenate([x, d, np.sort(rng.random((K, 1)), 0)], 1)
        gt[i] = np.hstack([R, t.reshape(3, 1)])
    return kp, gt
