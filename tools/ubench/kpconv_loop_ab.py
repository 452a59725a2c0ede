"""Time per launch of the KPConv kernels that share the neighbour loop of csrc/kp_shared.h, HIP-graph timed (10 launches per replay,
`timed` as tools/ubench/kpconv32_bench.py), on level-0 .. level-3 shapes of the default run (F = 4 fragments, each stacked with itself):
fused32 (Cin 32), fused (Cin 64 / 128 / 256), fp32 and bf16 feature rows, both contraction forms; the aggregate at Cin 512 with bf16
rows (level-3 shape); the deformable aggregate at the widths of resnetb_deformable (32 / 64 / 128 / 256 at levels 0 .. 3).

    python tools/ubench/kpconv_loop_ab.py run OUT.json [LEVELS]   one process = one round of one library (D3FEAT_AMD_LIB is read at
                                                                  import); LEVELS: comma list of the levels to time (default all)
    python tools/ubench/kpconv_loop_ab.py combine DIR OUT.json   DIR holds parent_<r>.json / new_<r>.json of alternated rounds

combine: per kernel the parent's median and min .. max over its rounds, this build's median, and `position`: does the new median lie within
the parent's own range, below it or above it -- the noise of this method on that day is the margin."""
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(path, levels=(0, 1, 2, 3), F=4):
    import numpy as np
    import torch
    from d3feat_amd import ops, tf_custom_ops as tfo
    from d3feat_amd.kernels.kernel_points import create_kernel_points
    from d3feat_amd.utils.synthetic import room_fragment
    dev = torch.device("cuda", 0)
    LIMITS = (37, 35, 36, 38)
    g = torch.Generator(device="cpu").manual_seed(0)

    def timed(fn, iters=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(gr, stream=st):
                for _ in range(iters):
                    fn()
            gr.replay()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            gr.replay()
            e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters * 1e3

    res = {}
    clouds = [tfo.grid_subsampling(torch.from_numpy(room_fragment(i, 300000, 1.68)).to(dev), 0.03) for i in range(F)]
    for level in range(4):
        dl = 0.03 * 2 ** level
        if level:
            clouds = [tfo.grid_subsampling(c, dl) for c in clouds]
        pts = torch.cat([x for c in clouds for x in (c, c)], 0).contiguous()
        lens = ops.as_lens([int(c.shape[0]) for c in clouds for _ in (0, 1)], dev)
        grid = ops.NeighborGrid(pts, lens, 2.5 * dl)
        nb, _ = grid.search(pts, lens, LIMITS[level], query_grid=grid, internal=True)
        P = grid.xyz.contiguous()
        Cin = 32 << level
        KP = create_kernel_points(1.5 * dl, 15, 1, 3, "center", rng=np.random.default_rng(1)).reshape(15, 3).astype(np.float32)
        f = torch.randn((P.shape[0], Cin), generator=g).to(dev)
        fh = f.to(torch.bfloat16)
        W = (torch.randn((15, Cin, Cin), generator=g) * 0.05).to(dev)
        raw = (torch.randn((P.shape[0], 60), generator=g) * 0.2).to(dev)
        fused = ops.kpconv_fused32 if level == 0 else ops.kpconv_fused
        cases = {}
        for x3 in (False, True):
            for name, feat in (("f32", f), ("bf16", fh)):
                def call(feat=feat, x3=x3):
                    ops.KP_X3 = x3
                    return fused(P, P, nb, feat, KP, W, dl, leaky=True)
                cases["level%d/%s Cin %d %s %s" % (level, "fused32" if level == 0 else "fused", Cin, name, "x3" if x3 else "mfma")] = call
        cases["level%d/deform_aggregate Cin %d f32" % (level, Cin)] = lambda: ops.kpconv_deform_aggregate(P, P, nb, f, KP, raw, dl, raw=True)
        if level == 3:
            f512 = torch.randn((P.shape[0], 512), generator=g).to(dev).to(torch.bfloat16)
            cases["level3/aggregate Cin 512 bf16"] = lambda: ops.kpconv_aggregate(P, P, nb, f512, KP, dl)
        for name, fn in cases.items() if level in levels else ():
            ops.KP_X3 = True
            res[name] = round(timed(fn), 3)
            print("%-48s rows %7d  %9.2f us" % (name, P.shape[0], res[name]), flush=True)
    with open(path, "w") as fh_:
        json.dump(res, fh_, indent=0)


def write_compact(obj, path):
    """JSON with one line per entry of the top level and of every `kernels` table below it."""
    def enc(k, v, ind):
        if isinstance(v, dict) and (k == "kernels" or "kernels" in v):
            return "%s%s: {\n%s\n%s}" % (ind, json.dumps(k), ",\n".join(enc(a, b, ind + " ") for a, b in v.items()), ind)
        return "%s%s: %s" % (ind, json.dumps(k), json.dumps(v))
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(enc(k, v, " ") for k, v in obj.items()) + "\n}\n")


def combine(d, path):
    rounds = {k: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, k + "_*.json")))] for k in ("parent", "new")}
    table, ok = {}, True
    for name in rounds["parent"][0]:
        p = [r[name] for r in rounds["parent"]]
        n = [r[name] for r in rounds["new"]]
        inside = min(p) <= statistics.median(n) <= max(p)
        ok = ok and inside
        pos = "inside" if inside else "below parent_min (faster)" if statistics.median(n) < min(p) else "above parent_max (slower)"
        table[name] = {"parent_us": p, "new_us": n, "parent_median": statistics.median(p), "new_median": statistics.median(n), "position": pos}
    out = {"what": "us per launch, HIP-graph timed, parent and new library alternated in fresh processes (tools/ubench/kpconv_loop_ab.py)",
           "rule": "new_median within [parent_min, parent_max] of the parent's own rounds",
           "rounds": {k: len(v) for k, v in rounds.items()}, "kernels": table, "all_inside_parent_spread": ok}
    if os.path.exists(path):                       # keep what another step recorded in the same file (bench_py)
        out.update({k: v for k, v in json.load(open(path)).items() if k not in out})
    write_compact(out, path)
    for name, t in table.items():
        print("%-48s parent %8.2f [%8.2f .. %8.2f]  new %8.2f  %s" % (name, t["parent_median"], min(t["parent_us"]), max(t["parent_us"]),
                                                                   t["new_median"], t["position"]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], *([tuple(int(x) for x in sys.argv[3].split(","))] if len(sys.argv) > 3 else []))
    else:
        combine(sys.argv[2], sys.argv[3])
