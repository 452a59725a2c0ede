#!/usr/bin/env python3
"""What do the registration and the metric of the KITTI test cost in one device call, against the only way the tree offered before
it?  (One process, one GPU; not bench.py.)

Workload: utils.synthetic.keypoint_pairs(5, n_pairs=555, K=250) -- 555 pairs (the size of the reference's test split) of 250 keypoints
with 32-d descriptors -- with registration.EVALUATE_KITTI(0.3).  Variants are alternated inside the same run, nine windows each:

  (a) one registration.register_kitti_pairs call, then a device synchronise (wall clock);
  (b) the same call captured in a HIP graph, HIP events around a replay;
  (c) the loop that was the only way before: registration.register_keypoints per pair (several launches and read-backs each), then
      rte / rre / the flags in numpy on the host (tester.py:329-338 in float64).  It is the baseline.

Before any timing the transforms of (a) and (b) are compared with those of (c), bit for bit, and the flags of all three are compared:
equal, or the run fails.  No time is a pass / fail condition.

    python tools/kitti_test_bench.py [--out profiles/kitti_test_bench.json] [--pairs 555] [--windows 9]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from d3feat_amd import ops
from d3feat_amd import registration as reg
from d3feat_amd.utils.synthetic import keypoint_pairs

VOXEL, SEED, K = 0.3, 5, 250


def stats(times, pairs):
    t = np.asarray(times, np.float64)
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4),
            "pairs_per_s_median": round(pairs / float(np.median(t)), 1), "windows_ms": [round(float(x) * 1e3, 4) for x in t]}


def host_errors(T, gt):
    """tester.py:329-338 on the host in float64 -> (rte, rre, flags)"""
    rte = np.linalg.norm(T[:, :, 3] - gt[:, :, 3], axis=1)
    with np.errstate(invalid="ignore"):
        rre = np.arccos((np.einsum("pki,pki->p", T[:, :, :3], gt[:, :, :3]) - 1) / 2)
        a, b = rte < 2, ~np.isnan(rre) & (rre < np.pi / 180 * 5)
    return rte, rre, a.astype(np.int32) | (b.astype(np.int32) << 1) | ((a & b).astype(np.int32) << 2)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "kitti_test_bench.json"))
    ap.add_argument("--pairs", type=int, default=555)
    ap.add_argument("--windows", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    kp_h, gt_h = keypoint_pairs(5, n_pairs=a.pairs, K=K)
    kp, gt = torch.from_numpy(kp_h).to(dev), torch.from_numpy(gt_h).to(dev)
    count = torch.full((2 * a.pairs,), K, dtype=torch.int32, device=dev)
    P, kw = a.pairs, dict(reg.EVALUATE_KITTI(VOXEL), seed=SEED)
    res = reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED)
    torch.cuda.synchronize(dev)

    def call():
        reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED, out=res)
        torch.cuda.synchronize(dev)

    def loop():
        T = np.stack([reg.register_keypoints(kp[2 * p], kp[2 * p + 1], device=dev, **kw)["transformation"][:3] for p in range(P)])
        return T, host_errors(T, gt_h.astype(np.float64))

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    with ops.private_workspace() as pw:
        with torch.cuda.stream(stream):
            gres = reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED)           # warm-up on this stream (scratch)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            reg.register_kitti_pairs(kp, count, gt, VOXEL, seed=SEED, out=gres)
    keep = pw.kept

    def replay():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            graph.replay()
            e1.record()
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    # the results first
    T_loop, (_, _, flags_loop) = loop()
    call()
    gres.T.fill_(-7)
    gres.errors.flags.fill_(-7)
    replay()
    T_call, T_graph = res.T.cpu().numpy(), gres.T.cpu().numpy()
    f_call, f_graph = res.errors.flags.cpu().numpy(), gres.errors.flags.cpu().numpy()
    same_T = bool(np.array_equal(T_call.astype(np.float64), T_loop) and np.array_equal(T_call, T_graph))
    same_flags = bool(np.array_equal(f_call, flags_loop) and np.array_equal(f_call, f_graph))
    times = {"device_call": [], "device_call_graph": [], "pair_loop": []}
    for w in range(a.windows):
        times["device_call"].append(wall(call))
        times["device_call_graph"].append(replay())
        times["pair_loop"].append(wall(loop))
        print("window %d: call %.1f ms, graph %.1f ms, loop %.1f ms" % (w, *(times[k][-1] * 1e3 for k in times)), file=sys.stderr, flush=True)
    m = res.errors.meters()
    out = {"pairs": P, "K": K, "C": 32, "parameters": dict(kw), "voxel_size": VOXEL, "windows": a.windows,
           "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, pair_loop), HIP events around "
                     "the graph replay" % a.windows,
           "baseline": "pair_loop: registration.register_keypoints per pair, then rte / rre / flags in numpy on the host",
           "transforms_equal": same_T, "flags_equal": same_flags, "success": [m["success"]["sum"], m["success"]["count"]],
           "validations": int(res.registration.validations.sum().item()), "iterations": int(res.registration.iterations.sum().item())}
    for k, t in times.items():
        out[k] = stats(t, P)
    h = np.median(times["pair_loop"])
    out["loop_over_device_call"] = round(float(h / np.median(times["device_call"])), 2)
    out["loop_over_device_call_graph"] = round(float(h / np.median(times["device_call_graph"])), 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    del keep
    if not (same_T and same_flags):
        raise SystemExit("results differ")


if __name__ == "__main__":
    main()
