#!/usr/bin/env python3
"""What does the front of a KITTI training step cost on the device?  (One process, one GPU; not bench.py.)

Workload: two pairs of 16 k-point clouds at KITTI's settings (training_pairs.MATCHING_KITTI: radius 0.45, 1024 distinct matches of at
least 1024; AUGMENT_KITTI).  The clouds are height fields on a 20/64 lattice with coordinates in sixty-fourths under a quarter turn, so
that fp32, float64 and a KD-tree agree about every match (tests/training_pairs_cases.py says why).  Three forms are alternated inside the
same run, nine windows each (a window: 50 device calls, each followed by a synchronise; the host loop once), the clouds on the device:

  (a) the call, eager (grid build included);
  (b) the call captured once in a graph and replayed (the device step advances by itself);
  (c) the host: the restatement's procedure per pair with scipy.spatial.cKDTree -- one radius query per anchor point as
      get_matching_indices loops, the (d2, j) order, Floyd's sample, the float32 row pass of tests/training_pairs_np.py.

Before any timing the integers of (a) and (c) are compared (M, n, status, both index lists) and the rows of (a) are compared bit for bit
with the restatement fed the device's parameters.  No time is a pass / fail condition.

    python tools/training_pairs_bench.py [--out profiles/training_pairs_bench.json] [--pairs 2] [--points 16000] [--windows 9]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import training_pairs_cases as tc
import training_pairs_np as tp
from d3feat_amd import training_pairs as T

STEP = 20.0 / 64.0


def cloud(rng, n):
    side = int(np.ceil(np.sqrt(n * 1.15)))
    pick = rng.choice(side * side, size=n, replace=False)
    ij = np.stack(np.unravel_index(pick, (side, side)), 1).astype(np.float64)
    xy = ij * STEP + rng.integers(-3, 4, size=(n, 2)) / 64.0
    z = np.round(64.0 * 1.5 * np.sin(xy[:, 0] / 7.0) * np.cos(xy[:, 1] / 5.0)) / 64.0
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def host_pair(pair, anchor, positive, trans, step, seed, k, min_matches, augment, params):
    """One pair on the host -> (M, status, anc, pos, augmented rows)."""
    from scipy.spatial import cKDTree
    q = tp.move(trans, anchor)
    tree = cKDTree(positive.astype(np.float64))
    r2 = np.float32(T.MATCHING_KITTI["radius"]) * np.float32(T.MATCHING_KITTI["radius"])
    rows = []
    for i in range(len(q)):                                                  # get_matching_indices: one radius query per anchor point
        js = np.asarray(tree.query_ball_point(q[i].astype(np.float64), T.MATCHING_KITTI["radius"]), np.int64)
        d2 = tp.d2_f32(q[i:i + 1], positive[js])[0] if len(js) else np.zeros(0, np.float32)
        js, d2 = js[d2 < r2], d2[d2 < r2]                                    # strict, in the header's metric
        js = js[np.lexsort((js, d2))]
        rows += [(i, int(j)) for j in js]
    M = len(rows)
    st = (tp.FEW_MATCHES if M < min_matches else 0) | (tp.BELOW_KEYPTS if M < k else 0)
    lst = np.asarray(rows, np.int64).reshape(-1, 2)
    anc = pos = None
    if not st:
        sel = tp.floyd(seed, step, pair, M, k)
        anc, pos = lst[sel, 0], lst[sel, 1] + len(anchor)
    out = [tp.augment_rows(seed, step, pair, side, augment["augment_noise"], params[side], c) for side, c in enumerate((anchor, positive))]
    return M, st, anc, pos, np.concatenate(out)


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(float(t.min()) * 1e3, 3), "max_ms": round(float(t.max()) * 1e3, 3),
            "ms_per_pair_median": round(float(np.median(t)) * 1e3 / pairs, 3), "windows_ms": [round(float(x) * 1e3, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training_pairs_bench.json"))
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--points", type=int, default=16000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50, help="device calls per window (each followed by a synchronise); the host loop runs once")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    pairs = []
    for p in range(a.pairs):
        Tm = tc.quarter_turn(1 + p, (640 * (p + 1), -320, 64))
        Ti = tc.inverse(Tm)
        base = cloud(rng, a.points)
        anchor = (base @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        pairs.append((anchor, cloud(rng, a.points), Tm))
    pts, lens, trans = tc.stack(pairs)
    d_pts, d_lens, d_trans = (torch.from_numpy(x).to(dev) for x in (pts, lens, trans))
    d_lens.host_lens = [int(x) for x in lens]
    kw = dict(seed=1, augment=T.AUGMENT_KITTI, **T.MATCHING_KITTI)
    k, mm = T.MATCHING_KITTI["keypts_num"], T.MATCHING_KITTI["min_matches"]

    first = T.training_pairs(d_pts, d_lens, trans=d_trans, step=0, **kw)
    torch.cuda.synchronize(dev)
    h = first.host()
    params = h["params"]
    off = np.concatenate([[0], np.cumsum(lens)])
    agree, rows_equal, host_t = True, True, []
    dev_points = first.points.cpu().numpy()
    for p, (anchor, positive, Tm) in enumerate(pairs):
        M, st, anc, pos, rows = host_pair(p, anchor, positive, Tm, 0, 1, k, mm, T.AUGMENT_KITTI, params[2 * p:2 * p + 2])
        agree = agree and M == int(h["matches"][p]) and st == int(h["status"][p]) and int(h["n"][p]) == (0 if st else k)
        if not st:
            agree = agree and np.array_equal(anc, h["anc_idx"][p]) and np.array_equal(pos, h["pos_idx"][p])
        rows_equal = rows_equal and np.array_equal(rows.view(np.uint32), dev_points[off[2 * p]:off[2 * p + 2]].view(np.uint32))

    res = T.training_pairs(d_pts, d_lens, trans=d_trans, **kw)                  # the device step from here on
    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        T.training_pairs(d_pts, d_lens, trans=d_trans, out=res, **kw)
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        T.training_pairs(d_pts, d_lens, trans=d_trans, out=res, **kw)

    def eager():
        T.training_pairs(d_pts, d_lens, trans=d_trans, step=0, **kw)
        torch.cuda.synchronize(dev)

    def replay():
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()

    def host():
        for p, (anchor, positive, Tm) in enumerate(pairs):
            host_pair(p, anchor, positive, Tm, 0, 1, k, mm, T.AUGMENT_KITTI, params[2 * p:2 * p + 2])

    def wall(fn, reps=1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps

    eager(); replay()
    times = {"eager": [], "replayed": [], "host_ckdtree": []}
    for w in range(a.windows):
        times["eager"].append(wall(eager, a.reps))
        times["replayed"].append(wall(replay, a.reps))
        times["host_ckdtree"].append(wall(host))
        print("window %d: eager %.3f ms, replayed %.3f ms, host %.1f ms" % (w, *(times[n][-1] * 1e3 for n in times)), file=sys.stderr, flush=True)
    out = {"pairs": a.pairs, "points_per_cloud": a.points, "settings": dict(T.MATCHING_KITTI, **T.AUGMENT_KITTI), "windows": a.windows,
           "timing": "the three forms alternated, %d windows each; a window is %d device calls, each followed by a synchronise (the host loop "
                     "once), wall clock per call; clouds on the device; eager includes the grid build, replayed is one graph launch" % (a.windows, a.reps),
           "matches": [int(x) for x in h["matches"]], "status": [int(x) for x in h["status"]],
           "integers_equal_host": bool(agree), "rows_bit_equal_host": bool(rows_equal), "device_step_after": int(res.step.item()),
           "host": "the restatement's procedure with scipy.spatial.cKDTree, one radius query per anchor point, one core"}
    for n, t in times.items():
        out[n] = stats(t, a.pairs)
    out["host_over_replayed"] = round(out["host_ckdtree"]["median_ms"] / max(out["replayed"]["median_ms"], 1e-9), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if not (agree and rows_equal):
        raise SystemExit("the device and the host restatement differ")


if __name__ == "__main__":
    main()
