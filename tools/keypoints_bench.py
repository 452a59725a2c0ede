#!/usr/bin/env python3
"""What does the keypoint selection on the device cost, and what does it save?  (One process, one GPU; not bench.py.)

Workload: the config-#2 fragment (utils.synthetic.room_fragment with bench.py's default arguments: 300 k raw points, ~29 k voxels per
cloud), K = 250.  Variants are alternated inside the same run, every figure is the median of nine windows.

  (a) the selection launch alone (HIP events) at F = 1 and F = 12 fragments per stack, contiguous-score form and record-block form,
      beside its algorithmic bytes (4 B per row read + 144 B per kept row read and written) and the record packing launch of the
      same stack (launches captured into a HIP graph, as they run inside a replay);
  (b) FragmentEngine(batch=12, slots=4, keypoints=250) against the same engine without keypoints, fragments/s (records stay on the
      device in both); single-fragment latency (F = 1, one slot) with and without;
  (c) fragment -> 250 keypoint records in HOST memory: fetch(keypoints=True) + a copy of K rows, against the way without the selection
      kernel (fetch(packed=True) -> .cpu() -> utils.results.select_first_cloud -> [-250:]), fragments/s;
  and the bytes one fragment contributes to the shard exchange, from the shapes.

    python tools/keypoints_bench.py [--out profiles/keypoints_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from d3feat_amd import keypoints, ops
from d3feat_amd import tf_custom_ops as tfo
from d3feat_amd.engine import FragmentEngine
from d3feat_amd.models.variables import build_variables
from d3feat_amd.utils.config import threedmatch_config
from d3feat_amd.utils.results import select_first_cloud
from d3feat_amd.utils.synthetic import room_fragment

K = 250
WINDOWS = 9


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


class LaunchTimer:
    """GPU time of one call of fn as it runs inside a replay: `reps` calls captured back to back into a HIP graph, HIP events around
    a replay of it (calls issued one by one from Python are bound by the host below ~30 us)."""

    def __init__(self, fn, dev, reps=20):
        self.reps, self.stream, self.graph = reps, torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
        self.out = []                                   # results stay alive: the graph owns their addresses
        with ops.private_workspace() as pw:
            with torch.cuda.stream(self.stream):
                fn()                                    # warm-up on this stream (scratch, ticket counters)
            self.stream.synchronize()
            with torch.cuda.graph(self.graph, stream=self.stream):
                for _ in range(reps):
                    self.out.append(fn())
        self.keep = pw.kept

    def __call__(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            self.graph.replay()
            e1.record()
        self.stream.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.reps


def selection_alone(rec_pair, dev):
    """rec_pair: the records f32[2n, 36] of one stacked self-pair (a real replay's scores)."""
    n = rec_pair.shape[0] // 2
    out = {}
    variants = {}
    for F in (1, 12):
        rec = torch.cat([rec_pair] * F).contiguous()
        lens = ops.as_lens([n, n] * F, dev)
        xyz, desc, score = rec[:, :3].contiguous(), rec[:, 3:35].contiguous(), rec[:, 35].contiguous()
        ident = torch.arange(rec.shape[0], dtype=torch.int32, device=dev)
        kp = torch.zeros((F, K, 36), dtype=torch.float32, device=dev)
        cnt = torch.zeros((F,), dtype=torch.int32, device=dev)
        variants[("contiguous_score", F)] = (lambda a=(xyz, desc, score, lens, kp, cnt):
                                             keypoints.topk(a[0], a[1], a[2], K, lens=a[3], group=2, keep=1, out=a[4], count=a[5], n_cap=n))
        variants[("record_block", F)] = (lambda a=(rec, lens, kp, cnt):
                                         keypoints.topk(a[0][:, :3], a[0][:, 3:35], a[0][:, 35], K, lens=a[1], group=2, keep=1, out=a[2],
                                                        count=a[3], n_cap=n))
        variants[("pack_descriptors_to", F)] = (lambda a=(xyz, desc, score, lens, ident):
                                                ops.pack_descriptors(a[0], a[1], a[2], lens=a[3], group=2, keep=1, row_map=a[4]))
    timers = {k: LaunchTimer(fn, dev) for k, fn in variants.items()}
    for t in timers.values():
        t()
    times = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, t in timers.items():
            times[k].append(t())
    for (name, F), ts in times.items():
        e = out.setdefault(name, {})
        e["F=%d" % F] = {"launch_us": round(median(ts), 2)}
        if name != "pack_descriptors_to":
            b = F * (4 * n + 2 * 144 * K)
            e["F=%d" % F]["algorithmic_bytes"] = b
            e["F=%d" % F]["GB_per_s"] = round(b / median(ts) / 1e3, 2)
    out["rows_per_cloud"] = n
    out["bound"] = ("latency: a chain of dependent steps inside one launch (slice keys -> 1-4 digit histograms -> candidates to the "
                    "workspace -> ticket -> the last workgroup's select over <= G * K candidates -> rank order -> record rows), each a "
                    "few barriers or one memory round trip long; the bytes (4 per row + 288 per kept row) are far below any "
                    "bandwidth limit, and the F clouds of a stack run side by side on F * G compute units")
    return out


def pipelined(eng, pool, rounds, consume):
    """rounds submits of eng.F fragments over all slots; consume(list of fetched results) per replay.  -> fragments/s"""
    S, F = len(eng.slots), eng.F
    busy = [False] * S
    torch.cuda.synchronize(eng.device)
    t0 = time.perf_counter()
    for i in range(rounds):
        k = i % S
        if busy[k]:
            consume(k)
        eng.submit(k, [pool[(i * F + j) % len(pool)] for j in range(F)])
        busy[k] = True
    for i in range(rounds, rounds + S):
        if busy[i % S]:
            consume(i % S)
            busy[i % S] = False
    torch.cuda.synchronize(eng.device)
    return rounds * F / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "keypoints_bench.json"))
    ap.add_argument("--rounds", type=int, default=16, help="replays per window of the engine measurements")
    ap.add_argument("--pool", type=int, default=12, help="different fragments in the pool")
    ap.add_argument("--keypoints-first", action="store_true",
                    help="build the keypoint engine before the plain one: an A/B of the build order itself")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = threedmatch_config()
    W = build_variables(cfg, seed=42).values
    limits = np.asarray([42, 42, 46, 51, 49], np.int32)            # fixed (tools/engine_timing.py): both engines of a pair share them
    pool = [torch.from_numpy(room_fragment(s)).to(dev) for s in range(a.pool)]
    n0 = [int(tfo.grid_subsampling(p, cfg.first_subsampling_dl).shape[0]) for p in pool]
    raw_cap = int(max(p.shape[0] for p in pool) * 1.05) + 1024
    n0_cap = (int(max(n0) * 1.1) + 1023) // 1024 * 1024            # bench.py's default capacities (--cap-factor 1.1, --level-ratio 0.32)
    kw = dict(raw_cap=raw_cap, n0_cap=n0_cap, level_ratio=0.32, device=dev, n0_hint=int(np.mean(n0)))
    res = {"K": K, "voxels_per_cloud": n0, "n0_cap": n0_cap, "windows": WINDOWS, "timing": "median of %d windows, variants alternated" % WINDOWS}

    # ---- (b), (c): engines
    # both engines replay on the SAME four streams: the runtime maps streams onto a few hardware queues in creation order, and an
    # engine on its own, later streams measured ~4 % faster than the one built first, whichever of the two it was
    streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
    if a.keypoints_first:
        kpe = FragmentEngine(cfg, W, limits, batch=12, slots=4, keypoints=K, streams=streams, **kw)
        plain = FragmentEngine(cfg, W, limits, batch=12, slots=4, streams=streams, **kw)
    else:
        plain = FragmentEngine(cfg, W, limits, batch=12, slots=4, streams=streams, **kw)
        kpe = FragmentEngine(cfg, W, limits, batch=12, slots=4, keypoints=K, streams=streams, **kw)
    res["built_first"] = "keypoints_engine" if a.keypoints_first else "plain_engine"
    host = torch.zeros((12, K, 36), dtype=torch.float32).pin_memory()
    sink = {}

    def keep_on_device(eng):
        return lambda k: eng.fetch(k, packed=True)

    def new_path(k):
        outs = kpe.fetch(k, keypoints=True)
        for j, kp in enumerate(outs):
            host[j, :kp.shape[0]].copy_(kp, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        sink["new"] = host[len(outs) - 1, -1, -1].item()

    def parent_path(k):
        for rec in plain.fetch(k, packed=True):
            r = rec.cpu().numpy()
            kp, feat, sc = select_first_cloud(r[:, :3], r[:, 3:-1], r[:, -1:], r.shape[0] // 2)
            sink["parent"] = (kp[-K:], feat[-K:], sc[-K:])

    runs = {"plain_engine": (plain, keep_on_device(plain)), "keypoints_engine": (kpe, keep_on_device(kpe)),
            "keypoints_to_host": (kpe, new_path), "parent_path_to_host": (plain, parent_path)}
    for eng, consume in runs.values():
        pipelined(eng, pool, 8, consume)
    fps = {k: [] for k in runs}
    for _ in range(WINDOWS):
        for name, (eng, consume) in runs.items():
            fps[name].append(pipelined(eng, pool, a.rounds if name != "parent_path_to_host" else max(a.rounds // 4, 4), consume))
    assert plain.fallbacks == 0 and kpe.fallbacks == 0
    med = {k: median(v) for k, v in fps.items()}
    res["engine_batch12_slots4"] = {
        "fragments_per_s": {k: round(v, 1) for k, v in med.items()},
        "windows_fragments_per_s": {k: [round(x, 1) for x in v] for k, v in fps.items()},
        "keypoints_engine_over_plain": round(med["keypoints_engine"] / med["plain_engine"], 4),
        "keypoints_to_host_over_plain": round(med["keypoints_to_host"] / med["plain_engine"], 4),
        "parent_path_to_host_over_plain": round(med["parent_path_to_host"] / med["plain_engine"], 4),
        "required": "both keypoint ratios >= 0.97"}
    # the keypoints of a replay are the stable-sort tail of that fragment's records
    plain.submit(0, pool[:12])
    recs = plain.fetch(0, packed=True)
    kpe.submit(0, pool[:12])
    kps = kpe.fetch(0, keypoints=True)
    r = recs[11].cpu().numpy()
    want = r[: r.shape[0] // 2][np.argsort(r[: r.shape[0] // 2, -1], kind="stable")[-K:]]
    res["host_results_agree"] = bool(np.array_equal(kps[11].cpu().numpy().view(np.uint32), want.view(np.uint32)))
    rec_pair = recs[0].clone()

    # ---- single-fragment latency
    one_plain = FragmentEngine(cfg, W, limits, batch=1, slots=1, **kw)
    one_kp = FragmentEngine(cfg, W, limits, batch=1, slots=1, keypoints=K, **kw)
    lat = {"plain": [], "keypoints": []}
    for eng in (one_plain, one_kp):
        for _ in range(5):
            eng.submit(0, pool[0])
            eng.fetch(0, packed=True)
    for _ in range(WINDOWS):
        for name, eng in (("plain", one_plain), ("keypoints", one_kp)):
            ts = []
            for i in range(10):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.submit(0, pool[i % len(pool)])
                eng.fetch(0, packed=True)
                ts.append(time.perf_counter() - t0)
            lat[name].append(median(ts) * 1e3)
    res["single_fragment_latency_ms"] = {k: round(median(v), 4) for k, v in lat.items()}

    # ---- (a): the launch alone
    res["selection_launch"] = selection_alone(rec_pair, dev)

    # ---- shard exchange, from the shapes
    res["shard_bytes_per_fragment"] = {"records_stride_n0_cap": n0_cap * 144, "keypoints_stride_K": K * 144,
                                       "multi_gpu_time": "not measured (one GPU)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("engine_batch12_slots4", "single_fragment_latency_ms", "selection_launch", "host_results_agree")}))


if __name__ == "__main__":
    main()
