"""tools/evaluate_3dmatch.py and tools/registration_recall.py end to end on a toy tree: two of the eight scenes with four and three
synthetic fragments, the files utils.results.save_3dmatch_keypoints writes, a gt.log / gt.info per scene.  The first tool registers
everything in one call and writes the .log files; the second evaluates those files -- MATLAB's job in the reference -- and must arrive
at the same figures; tools/register_scene.py --info prints the same recall line for one scene.  Each tool runs in a fresh child process,
with a time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTS = (32, 64)


def _block_text(entries, n):
    return "".join("%d\t %d\t %d\n" % (a, b, n) + "".join("\t".join(repr(float(v)) for v in row) + "\t\n" for row in M) for a, b, M in entries)


def _toy_tree(tmp_path, seed=23):
    from d3feat_amd.datasets import threedmatch
    from d3feat_amd.utils import results
    from d3feat_amd.utils.synthetic import scene
    rng = np.random.default_rng(seed)
    scenes = (threedmatch.SCENES[0], threedmatch.SCENES[5])
    root, gt_root = tmp_path / "D3Feat_toy", tmp_path / "gt_result"
    for k, (sc, n) in enumerate(zip(scenes, (4, 3))):
        blocks, poses = scene(seed + k, n_frag=n, K=64)
        blocks[1][7, 9] = np.nan                                                                  # evaluate.py:43-44 has work
        for f, b in enumerate(blocks):
            results.save_3dmatch_keypoints(str(root), "%s/seq-01/cloud_bin_%d.ply" % (sc, f), b)
        keys = [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) != (0, 1)]
        A = rng.normal(size=(len(keys), 6, 6))
        d = gt_root / (sc + "-evaluation")
        d.mkdir(parents=True)
        (d / "gt.log").write_text(_block_text([(i, j, np.linalg.inv(poses[i]) @ poses[j]) for i, j in keys], n))
        (d / "gt.info").write_text(_block_text([(i, j, a @ a.T * 50 + 5000 * np.eye(6)) for (i, j), a in zip(keys, A)], n))
    return scenes, root, gt_root


def _tool(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in args], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdin=subprocess.DEVNULL, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


INTS = ("good", "bad", "false_pos", "gt_num", "rs_num")


def test_evaluate_3dmatch_writes_logs_that_registration_recall_evaluates_to_the_same_figures(device, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import registration_recall as rr_tool
    from d3feat_amd.utils import results
    scenes, root, gt_root = _toy_tree(tmp_path)
    out = tmp_path / "out"
    lines = _tool("evaluate_3dmatch.py", "--root", root, "--gt-root", gt_root, "--counts", ",".join(str(k) for k in COUNTS), "--out", out, "--seed", 4)
    first = json.loads(lines[-1])
    assert first["scenes"] == list(scenes) and first["pairs"] == 9 and first["num_keypts"] == list(COUNTS)
    assert [l for l in lines if l.startswith("num_keypts = ")] == ["num_keypts = 32", "num_keypts = 64"] * 3           # per scene, then per count
    assert sum(l.startswith("recall : ") for l in lines) == 4 and sum(l.startswith("True average recall: ") for l in lines) == 2
    assert sum(l.startswith("Correct Match ") for l in lines) == 4
    # gt.log lists every pair but (0, 1); (0, 2), (0, 3), (1, 3) and (0, 2) are the non-consecutive ones
    assert [[r["gt_num"] for r in per] for per in first["registration"]] == [[3, 3], [1, 1]]
    assert [[r["rs_num"] for r in per] for per in first["registration"]] == [[3, 3], [1, 1]]
    assert [[r["gt"] for r in per] for per in first["matching"]] == [[5, 5], [2, 2]]
    for c, k in enumerate(COUNTS):
        base = out / ("num_keypts_%d" % k)
        for s, (sc, n) in enumerate(zip(scenes, (4, 3))):
            rows = results.read_result_log(str(base / "log_result" / (sc + "-evaluation") / "D3Feat_.log"))
            assert [(a, b) for a, b, _ in rows] == [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) != (0, 1)]
            assert len(os.listdir(base / "pred_result" / sc)) == n * (n - 1) // 2
            assert (base / "pred_result" / sc / "cloud_bin_0_cloud_bin_1.rt.txt").read_text() == "cloud_bin_0\tcloud_bin_1\t0\t0.00000000\t0"
    # the largest count through the second tool in a child process, the other through its function
    lines2 = _tool("registration_recall.py", "--gt-root", gt_root, "--log-root", out / "num_keypts_64" / "log_result")
    second = json.loads(lines2[-1])
    assert second["scenes"] == list(scenes)
    want = [per[1] for per in first["registration"]]
    assert [{k: r[k] for k in INTS} for r in second["figures"]] == [{k: r[k] for k in INTS} for r in want]
    assert [r["recall"] for r in second["figures"]] == [r["recall"] for r in want] and second["overall"] == first["overall"][1]
    assert lines[-6] == "num_keypts = 64" and lines2[:-1] == lines[-5:-1]                         # the same printed lines
    # tools/register_scene.py --info on the first scene alone: the same recall lines, each before its JSON line
    gt_dir = gt_root / (scenes[0] + "-evaluation")
    lines3 = _tool("register_scene.py", "--root", root, "--scene", scenes[0], "--gt", gt_dir / "gt.log", "--info", gt_dir / "gt.info",
                   "--counts", "32,64", "--seed", 4, "--out", tmp_path / "out_scene")
    assert lines[-11] == "num_keypts = 32" and [l for l in lines3 if l.startswith("recall : ")] == [lines[-10], lines[-5]]
    assert [l.startswith("recall : ") for l in lines3] == [True, False, True, False] and json.loads(lines3[-1])["num_keypts"] == 64
    other = rr_tool.evaluate(str(gt_root), str(out / "num_keypts_32" / "log_result"), scenes, device=device)
    assert [{k: r[0][k] for k in INTS} for r in other.scenes()] == [{k: per[0][k] for k in INTS} for per in first["registration"]]
    assert other.logged and other.figures.shape == (2, 1, 5)
