"""The host side of the ETH generalisation test (test_eth.py, datasets/ETH.py and geometric_registration_eth/evaluate_eth.py of the
reference): the four outdoor scenes, what the test changes in a 3DMatch-trained configuration, the order of a scene's scans, and the
pair list with its ground truth in the layout registration.match_scenes takes.  Pure numpy apart from read_scan, whose voxel grid runs
on the device.

    <root>/<scene>/Hokuyo_<k>.ply       the scans of a scene (any name that ends in _<k>.ply)
    <root>/<scene>/gt.log               blocks of `id1 \\t id2 \\t n` + a 4x4 matrix, target -> source, for the pairs that overlap
"""
import os

import numpy as np

from ..utils.results import read_gt_log

SCENES = ('gazebo_summer', 'gazebo_winter', 'wood_autmn', 'wood_summer')       # ETH.py:153-158 (its spelling)
FIRST_SUBSAMPLING_DL, KP_EXTENT, VOXEL_SIZE = 0.05, 2, 0.0625                  # test_eth.py:37,39, ETH.py:169


def apply_config(config):
    """test_eth.py:37-39: what the test changes in the configuration of a 3DMatch-trained model.  -> config"""
    config.first_subsampling_dl = FIRST_SUBSAMPLING_DL
    config.dataset = 'ETH'
    config.KP_extent = KP_EXTENT
    return config


def scene_scans(root, scene):
    """The .ply files of <root>/<scene> sorted by the trailing integer of their names (ETH.py:163-166: Hokuyo_10 after Hokuyo_9)
    -> list of paths."""
    d = os.path.join(root, scene)
    names = [f for f in os.listdir(d) if f.endswith('ply')]
    return [os.path.join(d, f) for f in sorted(names, key=lambda x: int(x[:-4].split("_")[-1]))]


def read_scan(path, voxel_size=VOXEL_SIZE):
    """One scan, voxelised at 0.0625 m (ETH.py:168-169) -> f32[n, 3].  The grid is THIS project's grid subsampler (barycentres of the
    reference's own grid_subsampling.cpp, on the device), as everywhere else here; Open3D's voxel grid, which the reference calls at
    this place, is third-party arithmetic that nothing pins and is not reproduced."""
    import torch
    from .. import tf_custom_ops as tfo
    from ..utils.ply import read_ply_xyz
    pts = np.ascontiguousarray(read_ply_xyz(path), dtype=np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return pts
    dev = torch.device("cuda", torch.cuda.current_device())
    return tfo.grid_subsampling(torch.from_numpy(pts).to(dev), float(voxel_size)).cpu().numpy()


def benchmark(root_or_counts, gt_logs=None, scenes=SCENES):
    """The pair list of evaluate_eth.py:104-109 for all scenes at once -> (pairs i32[P, 2], gt f32[P, 3, 4], gt_flag i32[P],
    scene_start i64[S + 1]), the arguments of registration.match_scenes (host arrays).

    root_or_counts: the data root (scenes `scenes`, the scans counted on disk, gt.log read from <root>/<scene>/gt.log) or a list of
    scan counts, one per scene; gt_logs: then one per scene, a path or a dict as results.read_gt_log returns it (None: no pair listed).
    pairs hold GLOBAL block indices -- scene s starts at the sum of the counts before it --, every id1 < id2 of a scene in the
    reference's order, the scenes one after the other; scene_start[s] is the first pair of scene s.  gt[p] is the target -> source
    matrix of gt.log, the identity where gt.log does not list the pair (gt_flag 0: the pair counts nowhere)."""
    if isinstance(root_or_counts, (str, os.PathLike)):
        root = os.fspath(root_or_counts)
        counts = [len(scene_scans(root, s)) for s in scenes]
        if gt_logs is None:
            gt_logs = [os.path.join(root, s, "gt.log") for s in scenes]
    else:
        counts = [int(c) for c in root_or_counts]
        if gt_logs is None:
            gt_logs = [None] * len(counts)
    if len(gt_logs) != len(counts):
        raise ValueError("benchmark: %d scenes, %d gt logs" % (len(counts), len(gt_logs)))
    pairs, gt, flag, scene_start, base = [], [], [], [0], 0
    for n, log in zip(counts, gt_logs):
        log = {} if log is None else (log if isinstance(log, dict) else read_gt_log(os.fspath(log)))
        for id1 in range(n):
            for id2 in range(id1 + 1, n):
                M = log.get("%d_%d" % (id1, id2))
                pairs.append((base + id1, base + id2))
                gt.append(np.eye(4)[:3] if M is None else np.asarray(M, np.float64)[:3])
                flag.append(0 if M is None else 1)
        base += n
        scene_start.append(len(pairs))
    return (np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(gt, np.float64).reshape(-1, 3, 4).astype(np.float32),
            np.asarray(flag, np.int32), np.asarray(scene_start, np.int64))
