#!/usr/bin/env python3
"""Registration recall of .log files that are already written: what geometric_registration/3dmatch/evaluate.m prints, without MATLAB.

    python tools/registration_recall.py --gt-root geometric_registration/gt_result --log-root geometric_registration/log_result [--name D3Feat_]

Reads `<gt-root>/<scene>-evaluation/gt.log` and `gt.info` and `<log-root>/<scene>-evaluation/<name>.log` (evaluate.m:31-38) of the
eight test scenes -- those whose result file exists --, puts every result row of every scene into ONE registration.registration_recall
call (logged=True: the matrices are in the .log convention already; result_flag 1 for every row, so a row for a pair gt.log does not
list is a false positive and a pair without a row only counts in gt_num) and prints the lines of mrEvaluateRegistration.m:40 and
evaluate.m:47-48, then one JSON line with the figures, the false positives among them.  A pair that appears twice in a result file is
two rows, as in MATLAB.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def load(gt_root, log_root, scenes, name="D3Feat_"):
    """-> (rows of registration_recall as host arrays: T f64[P, 4, 4], gt, info, gt_flag, result_flag, ids, scene_start): per scene
    first the rows of the result file in file order, then one row without a result for every listed pair the file does not hold."""
    from d3feat_amd.datasets import threedmatch
    from d3feat_amd.utils import results
    T, gt, info, flag, res, ids, scene_start = [], [], [], [], [], [], [0]
    for scene in scenes:
        log_p, info_p = threedmatch.gt_paths(gt_root, scene)
        log, inf = threedmatch._ground_truth(log_p, info_p)
        seen = set()
        for id1, id2, M in results.read_result_log(os.path.join(log_root, scene + "-evaluation", name + ".log")):
            key = "%d_%d" % (id1, id2)
            seen.add(key)
            T.append(M)
            gt.append(log.get(key, np.eye(4)))
            info.append(inf.get(key, np.eye(6)))
            flag.append(1 if key in log else 0)
            res.append(1)
            ids.append((id1, id2))
        for key in log:
            if key not in seen:
                T.append(np.eye(4)); gt.append(log[key]); info.append(inf[key]); flag.append(1); res.append(0)
                ids.append(tuple(int(v) for v in key.split("_")))
        scene_start.append(len(T))
    f64 = lambda a, *s: np.asarray(a, np.float64).reshape(-1, *s)
    i32 = lambda a, *s: np.asarray(a, np.int32).reshape(-1, *s)
    return f64(T, 4, 4), f64(gt, 4, 4), f64(info, 6, 6), i32(flag), i32(res), i32(ids, 2), scene_start


def evaluate(gt_root, log_root, scenes, name="D3Feat_", err2=0.04, device=None):
    """-> registration.SceneRecall of ONE registration_recall call over the result files of `scenes`."""
    import torch
    from d3feat_amd import registration as reg
    dev = device if device is not None else torch.device("cuda", 0)
    T, gt, info, flag, res, ids, scene_start = load(gt_root, log_root, scenes, name)
    d = lambda a: torch.from_numpy(a).to(dev)
    return reg.registration_recall(d(T), d(gt), d(info), d(flag), d(ids), scene_start, err2=err2, result_flag=d(res), logged=True)


def report(scenes, recall, c=0, **extra):
    from d3feat_amd.utils import results
    print("\n".join(results.registration_recall_lines(scenes, recall, c)))
    print(json.dumps(dict(scenes=list(scenes), figures=[per[c] for per in recall.scenes()], overall=recall.overall(c), **extra)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt-root", required=True)
    ap.add_argument("--log-root", required=True)
    ap.add_argument("--name", default="D3Feat_", help="the result files are <name>.log (descriptorName of evaluate.m)")
    ap.add_argument("--err2", type=float, default=0.04)
    a = ap.parse_args()
    from d3feat_amd.datasets import threedmatch
    scenes = [s for s in threedmatch.SCENES if os.path.isfile(os.path.join(a.log_root, s + "-evaluation", a.name + ".log"))]
    if not scenes:
        raise SystemExit("%s holds no <scene>-evaluation/%s.log of the 3DMatch test scenes" % (a.log_root, a.name))
    report(scenes, evaluate(a.gt_root, a.log_root, scenes, a.name, a.err2))


if __name__ == "__main__":
    main()
