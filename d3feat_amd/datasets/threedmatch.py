"""The host side of the 3DMatch registration benchmark (geometric_registration/evaluate.py and geometric_registration/3dmatch/evaluate.m
of the reference): the eight test scenes, and the pair list with its ground truth in the layout registration.register_scenes and
registration.registration_recall take.  Pure numpy.

    <gt_root>/<scene>-evaluation/gt.log     blocks of `id1 \\t id2 \\t n` + a 4x4 matrix, target -> source, for the pairs that overlap
    <gt_root>/<scene>-evaluation/gt.info    blocks of `id1 \\t id2 \\t n` + the 6x6 information matrix of the same pairs
"""
import collections
import os

import numpy as np

from ..utils.results import _blocks, read_gt_info, read_gt_log

SCENES = ('7-scenes-redkitchen', 'sun3d-home_at-home_at_scan1_2013_jan_1', 'sun3d-home_md-home_md_scan9_2012_sep_30',
          'sun3d-hotel_uc-scan3', 'sun3d-hotel_umd-maryland_hotel1', 'sun3d-hotel_umd-maryland_hotel3',
          'sun3d-mit_76_studyroom-76-1studyroom2', 'sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika')   # evaluate.py:161-170, evaluate.m:14-23

Benchmark = collections.namedtuple("Benchmark", "pairs ids gt info gt_flag scene_start")


def gt_paths(gt_root, scene):
    """-> (gt.log, gt.info) of a scene under the reference's gt_result layout (evaluate.py:142, evaluate.m:34-38)."""
    d = os.path.join(os.fspath(gt_root), scene + "-evaluation")
    return os.path.join(d, "gt.log"), os.path.join(d, "gt.info")


def _ground_truth(log, info):
    """(path or dict or None) x 2 -> (dict of 4x4, dict of 6x6) with the same keys; a duplicate entry is an error."""
    if log is None:
        log = {}
    elif not isinstance(log, dict):
        path = os.fspath(log)
        log = read_gt_log(path)
        if len(log) != len(_blocks(path, 4)):
            raise ValueError("%s: two entries for one pair" % path)
    if info is None:
        info = {}
    elif not isinstance(info, dict):
        info = read_gt_info(os.fspath(info))
    if set(log) != set(info):
        raise ValueError("gt.log and gt.info list different pairs: %s" % sorted(set(log) ^ set(info))[:5])
    return log, info


def benchmark(gt_root, fragments_per_scene, scenes=SCENES, gt_logs=None, gt_infos=None):
    """The pair list of evaluate.py:150-156 for all scenes at once -> Benchmark(pairs i32[P, 2], ids i32[P, 2], gt f64[P, 4, 4],
    info f64[P, 6, 6], gt_flag i32[P], scene_start i64[S + 1]), the arguments of registration.register_scenes /
    registration_recall (host arrays).

    gt_root: the folder of the <scene>-evaluation folders (gt.log and gt.info read from there), or None with gt_logs / gt_infos: one
    per scene, a path or a dict as results.read_gt_log / read_gt_info return it (None: no pair listed).  fragments_per_scene: the
    number of fragments of every scene.  pairs hold GLOBAL block indices -- scene s starts at the sum of the counts before it --, ids
    the fragment numbers inside the scene; every id1 < id2 of a scene in the reference's order, the scenes one after the other;
    scene_start[s] is the first pair of scene s.  gt[p] / info[p] are the matrices of gt.log / gt.info, the identity where they do not
    list the pair (gt_flag 0).  An entry for a fragment the scene does not have, a pair listed twice, or a pair in only one of the
    two files is an error."""
    counts = [int(c) for c in fragments_per_scene]
    if gt_root is not None:
        if gt_logs is not None or gt_infos is not None:
            raise ValueError("benchmark: gt_root or gt_logs / gt_infos, not both")
        if len(counts) != len(scenes):
            raise ValueError("benchmark: %d scenes, %d fragment counts" % (len(scenes), len(counts)))
        gt_logs, gt_infos = zip(*(gt_paths(gt_root, s) for s in scenes)) if counts else ((), ())
    gt_logs = [None] * len(counts) if gt_logs is None else list(gt_logs)
    gt_infos = [None] * len(counts) if gt_infos is None else list(gt_infos)
    if len(gt_logs) != len(counts) or len(gt_infos) != len(counts):
        raise ValueError("benchmark: %d scenes, %d gt logs, %d gt infos" % (len(counts), len(gt_logs), len(gt_infos)))
    pairs, ids, gt, info, flag, scene_start, base = [], [], [], [], [], [0], 0
    for n, log, inf in zip(counts, gt_logs, gt_infos):
        log, inf = _ground_truth(log, inf)
        known = {"%d_%d" % (a, b) for a in range(n) for b in range(a + 1, n)}
        if not set(log) <= known:
            raise ValueError("benchmark: gt.log lists %s, the scene has %d fragments" % (sorted(set(log) - known)[:5], n))
        for id1 in range(n):
            for id2 in range(id1 + 1, n):
                key = "%d_%d" % (id1, id2)
                M = log.get(key)
                pairs.append((base + id1, base + id2))
                ids.append((id1, id2))
                gt.append(np.eye(4) if M is None else np.asarray(M, np.float64))
                info.append(np.eye(6) if M is None else np.asarray(inf[key], np.float64))
                flag.append(0 if M is None else 1)
        base += n
        scene_start.append(len(pairs))
    return Benchmark(np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(ids, np.int32).reshape(-1, 2),
                     np.asarray(gt, np.float64).reshape(-1, 4, 4), np.asarray(info, np.float64).reshape(-1, 6, 6),
                     np.asarray(flag, np.int32), np.asarray(scene_start, np.int64))
