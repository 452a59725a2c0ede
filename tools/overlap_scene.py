#!/usr/bin/env python3
"""The overlap and correspondence tables of one scene on the GPU, as datasets/cal_overlap.py makes them pair by pair with a
brute-force matcher on the host.

Reads <root>/<scene>/seq-*/cloud_bin_<k>.ply with its cloud_bin_<k>.pose.npy (4 x 4, fragment to world) in the order of
cal_overlap.py:32-47 (sequences sorted by name, fragments by number), subsamples every fragment at --downsample, moves it into the
world frame (:53-59), then calls overlap.overlap_pairs for ALL pairs a < b and once more with nearest=True for the pairs above 0.30
only, and writes the two dictionaries of :128-131 -- '<anc>@<pos>' -> ratio and -> int32[M, 2] -- under the reference's file names
into --out.  Prints one JSON line: fragments, pairs, selected pairs.

    python tools/overlap_scene.py --root data/3DMatch/fragments --scene 7-scenes-chess --out data/3DMatch

The subsampling is this project's grid subsampler (ops.batch_grid_subsample: the barycentre of every occupied voxel of a grid
whose origin is the cloud's minimum corner rounded down to a multiple of the voxel size).  open3d.voxel_down_sample, which the reference calls, anchors its voxels at another origin
(the minimum bound minus half a voxel) and is not installed where this project is developed, so its output cannot be pinned here:
the tables agree with the reference's in definition, not point for point.  Hand in clouds subsampled by Open3D (--downsample 0
takes the .ply files as they are) where the same points are needed.
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def scene_ids(root, scene):
    """The fragment ids of cal_overlap.py:39-46: '<scene>/<seq>/cloud_bin_<k>', sequences sorted by name, fragments by number."""
    ids = []
    for seq in sorted(os.listdir(os.path.join(root, scene))):
        if not seq.startswith("seq"):
            continue
        names = [f.split(".")[0] for f in os.listdir(os.path.join(root, scene, seq)) if f.endswith("ply")]
        ids += ["%s/%s/%s" % (scene, seq, n) for n in sorted(names, key=lambda x: int(x.split("_")[-1]))]
    return ids


def load_fragments(root, ids):
    """-> (list of f32[n, 3] clouds in their own frames, list of f64[4, 4] poses)."""
    from d3feat_amd.utils.ply import read_ply_xyz
    return [read_ply_xyz(os.path.join(root, i + ".ply")) for i in ids], [np.load(os.path.join(root, i + ".pose.npy")) for i in ids]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--downsample", type=float, default=0.025, help="voxel size, and the matching threshold (0: no subsampling, "
                    "threshold --threshold)")
    ap.add_argument("--threshold", type=float, default=None, help="matching distance when it is not the voxel size")
    ap.add_argument("--split", default="train")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from d3feat_amd import _lib, ops, overlap
    from d3feat_amd.utils import results
    dev = torch.device("cuda", 0)
    ids = scene_ids(a.root, a.scene)
    if not 1 <= len(ids) <= _lib.MAX_BATCH:
        raise SystemExit("%s: %d fragments (1 to %d)" % (os.path.join(a.root, a.scene), len(ids), _lib.MAX_BATCH))
    clouds, poses = load_fragments(a.root, ids)
    thr = a.threshold if a.threshold is not None else a.downsample
    if a.downsample > 0:
        raw, raw_lens = overlap.stack_fragments(clouds, device=dev)
        sub, sub_lens, _, _ = ops.batch_grid_subsample(raw, raw_lens, a.downsample)
        clouds = [c.cpu().numpy() for c in torch.split(sub, ops.host_lens(sub_lens))]
    points, lens = overlap.stack_fragments(clouds, poses, device=dev)
    first = overlap.overlap_pairs(points, lens, threshold=thr)
    pairs = torch.from_numpy(np.stack(np.triu_indices(len(ids), 1), 1).astype(np.int32))
    keep = first.selected(overlap.OVERLAP_3DMATCH["min_ratio"])
    chosen = pairs[keep].contiguous()
    ratios = first.ratios()[keep]
    matches = []
    if len(keep):
        second = overlap.overlap_pairs(points, lens, chosen.to(dev), threshold=thr, nearest=True, grid=first.grid)
        assert np.array_equal(second.ratios(), ratios)
        matches = [second.matches(p) for p in range(len(keep))]
    paths = results.save_overlap_tables(a.out, ids, chosen.tolist(), ratios, matches, split=a.split, downsample=a.downsample)
    print(json.dumps(dict(scene=a.scene, fragments=len(ids), pairs=int(pairs.shape[0]), selected=int(len(keep)), threshold=thr,
                          points=[int(n) for n in ops.host_lens(lens)], files=paths)))


if __name__ == "__main__":
    main()
