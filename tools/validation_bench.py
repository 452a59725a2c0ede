#!/usr/bin/env python3
"""What do the validation figures of a split cost in one device call, against a loop that materialises the distance matrices as the
reference's TensorFlow graph does?  (One process, one GPU; not bench.py.)

Workloads (seeded where the tool runs): 500 pairs of n = 256 correspondences (3DMatch: keypts_num 256, safe radius 0.1, validation_size
500 in training_3DMatch.py) and 100 pairs of n = 1024 (KITTI: 1024, 1.0), C = 32, stacks of 2 x 2048 rows per pair.
Variants are alternated inside the same run, nine windows each:

  (a) one validation.validation_pairs call over all pairs: eager (wall clock around call + synchronise), and replayed from a HIP
      graph (HIP events around the replay);
  (b) torch_loop below: per pair the gathers, the [n, n, C] differences of loss.cdist (twice: descriptors and points), the masks,
      logsumexp, softplus and the means as utils/loss.py writes them, in float32 torch ops on the same device (wall clock).

Before any timing the figures of (a) and (b) are compared pair by pair (the accurate-row counts equal, the five figures within 1e-5:
two float32 evaluations in different summation orders).  Medians and ranges go to profiles/validation_bench.json; (a) counts as
faster only when the ranges of the nine windows do not overlap.

    python tools/validation_bench.py [--out profiles/validation_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/validation_bench.py --profile-call      (one call of each workload only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

WINDOWS = 9
C, ROWS = 32, 2048
WORKLOADS = (("3dmatch", 500, 256, dict(safe_radius=0.1, keypts_num=256, det_loss_weight=1.0), 0.4),
             ("kitti", 100, 1024, dict(safe_radius=1.0, keypts_num=1024, det_loss_weight=1.0), 4.0))


def make(seed, P, n, cube, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = torch.nn.functional.normalize(torch.randn((P, 2 * ROWS, C), generator=g), dim=-1)
    ai = torch.stack([torch.randperm(ROWS, generator=g)[:n] for _ in range(P)])
    pj = torch.stack([torch.randperm(ROWS, generator=g)[:n] for _ in range(P)])
    b = torch.nn.functional.normalize(torch.gather(f, 1, ai[:, :, None].expand(-1, -1, C)) + 1.6 * torch.randn((P, n, C), generator=g)
                                      / C ** 0.5, dim=-1)
    f.scatter_(1, (pj + ROWS)[:, :, None].expand(-1, -1, C), b)
    x = torch.rand((P, 2 * ROWS, 3), generator=g) * cube
    s = torch.rand((P, 2 * ROWS), generator=g) * 0.95 + 0.05
    row0 = torch.arange(P + 1, dtype=torch.int32) * (2 * ROWS)
    return [t.to(dev) for t in (f.reshape(-1, C), s.reshape(-1), x.reshape(-1, 3), ai.to(torch.int32), (pj + ROWS).to(torch.int32),
                                torch.full((P,), n, dtype=torch.int32), row0)]


def torch_loop(f, s, x, anc, pos, row0, safe_radius, keypts_num, det_loss_weight):
    """utils/loss.py (cdist, circle_loss, det_loss) and KPFCNN_model.py:131-186 with torch ops, one pair at a time -> f32[P, 6]
    (circle, det, accuracy, d_pos, d_neg, accurate rows)."""
    out = []
    for p in range(anc.shape[0]):
        o = int(row0[p])
        a, b = (o + anc[p]).long(), (o + pos[p]).long()
        n = a.numel()

        def cdist(u, v):
            d = u[:, None, :] - v[None, :, :]                     # all n x n x C differences, as loss.all_diffs
            return torch.sqrt((d * d).sum(-1) + 1e-12)
        kd = cdist(x[a], x[a])
        D = cdist(f[a], f[b])
        eye = torch.eye(n, dtype=torch.bool, device=f.device)
        fn = (kd < safe_radius) & ~eye
        fp = (D * eye).max(1).values
        cn = (D + 1e5 * eye).min(1).values
        d_neg = (D * (~eye & ~fn)).mean() * n / (n - 1.0)
        diff = fp - cn
        acc = (diff <= 0).float().sum()
        neg = D + 1e8 * fn + 1e8 * eye
        lse = torch.logsumexp(25.0 * (1.4 - neg) * torch.clamp(1.4 - neg, min=0.0), -1)
        circle = (torch.nn.functional.softplus(25.0 * (fp - 0.1) + lse) / 25.0).mean()
        det = det_loss_weight * (diff[:, None] * (s[a][:, None] + s[b][:, None] + 1e-6)).mean()
        out.append(torch.stack([circle, det, acc / n, fp.mean(), d_neg, acc]))
    return torch.stack(out)


def stats(times):
    t = np.asarray(times, np.float64) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
            "windows_ms": [round(float(v), 4) for v in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "validation_bench.json"))
    ap.add_argument("--profile-call", action="store_true", help="one validation_pairs call per workload and nothing else")
    a = ap.parse_args()
    from d3feat_amd import ops, validation
    dev = torch.device("cuda", 0)
    report = {"windows": WINDOWS, "descriptor_dim": C, "rows_per_pair": 2 * ROWS,
              "timing": "variants alternated, %d windows each; wall clock around call + synchronise (device_call, torch_loop), HIP events "
                        "around the graph replay" % WINDOWS,
              "baseline": "torch_loop: per pair the n x n x C differences of loss.cdist for descriptors and points, masks, logsumexp, "
                          "softplus, means -- float32 torch ops on the same device"}
    failed = False
    for name, P, n, par, cube in WORKLOADS:
        f, s, x, anc, pos, nd, row0 = make(1, P, n, cube, dev)
        res = validation.validation_pairs(f, s, x, anc, pos, nd, row0, **par)
        torch.cuda.synchronize(dev)
        if a.profile_call:
            report[name] = {"pairs": P, "n": n, "means": res.means()}
            continue
        host_row0 = row0.cpu().tolist()

        def call():
            validation.validation_pairs(f, s, x, anc, pos, nd, row0, out=res, **par)
            torch.cuda.synchronize(dev)

        def loop():
            r = torch_loop(f, s, x, anc, pos, host_row0, **par)
            torch.cuda.synchronize(dev)
            return r
        base = loop().cpu().numpy().astype(np.float64)
        got = res.values.cpu().numpy().astype(np.float64)
        err = np.abs(got[:, [0, 2, 3, 4, 5]] - base[:, :5]).max(0)
        counts_equal = bool(np.array_equal(got[:, 6], base[:, 5]))
        stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
        gres = validation.PairValidation(P, dev)
        with torch.cuda.stream(stream):
            with ops.private_workspace() as pw:
                validation.validation_pairs(f, s, x, anc, pos, nd, row0, out=gres, **par)          # warm-up on this stream
                stream.synchronize()
                with torch.cuda.graph(graph, stream=stream):
                    validation.validation_pairs(f, s, x, anc, pos, nd, row0, out=gres, **par)

        def replay():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                graph.replay()
                e1.record()
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        def wall(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        gres.values.fill_(-7.0)
        replay()
        graph_equal = bool(torch.equal(gres.values.view(torch.int32), res.values.view(torch.int32)) and torch.equal(gres.sums, res.sums))
        times = {"device_call": [], "device_call_graph": [], "torch_loop": []}
        for _ in range(WINDOWS):
            times["device_call"].append(wall(call))
            times["device_call_graph"].append(replay())
            times["torch_loop"].append(wall(loop))
        w = {"pairs": P, "n": n, "parameters": par, "means": res.means(), "accurate_rows_equal_to_torch_loop": counts_equal,
             "largest_difference_to_torch_loop": dict(zip(("circle", "det", "accuracy", "d_pos", "d_neg"), [float(v) for v in err])),
             "graph_replay_equal_to_eager": graph_equal,
             "bytes_the_loop_materialises_per_pair": int(n) * int(n) * (C + 3) * 4}
        for k, t in times.items():
            w[k] = stats(t)
        b = np.median(times["torch_loop"])
        w["torch_loop_over_device_call"] = round(float(b / np.median(times["device_call"])), 2)
        w["torch_loop_over_device_call_graph"] = round(float(b / np.median(times["device_call_graph"])), 2)
        w["ranges_disjoint"] = bool(max(times["device_call"]) < min(times["torch_loop"]))
        report[name] = w
        failed = failed or not counts_equal or not graph_equal or float(err.max()) > 1e-5
        del pw
    if not a.profile_call:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))
    if failed:
        raise SystemExit("the device call and the torch loop disagree")


if __name__ == "__main__":
    main()
