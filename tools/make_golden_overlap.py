#!/usr/bin/env python3
"""tests/golden/overlap.npz: what the REFERENCE'S OWN PYTHON computes for the overlap of a scene's fragments (build machine only).

datasets/cal_overlap.py is imported UNMODIFIED from the reference tree.  It imports open3d (only to read and transform .ply files:
not used here, the points are handed over in memory) and cv2, for cv2.BFMatcher(cv2.NORM_L2).match(a, b); neither is installed, so
this script provides stub modules of its own.  The BFMatcher stand-in is a float64 brute force over the float32 inputs that takes the
first minimum and returns objects with queryIdx, trainIdx and distance.  So THE NEAREST-NEIGHBOUR SEARCH ITSELF IS THE STUB'S; what
the reference contributes is the filter (distance < voxel size, get_matching_indices :78-85), the ratio (len(matches) / len(anchor),
:116) and the selection (> 0.30, :121-123) with the two dictionaries it pickles (:128-131).

The ThreeDMatch object is made with object.__new__ (its __init__ reads a dataset from disk) and given pts, scene_to_ids, savepath (a
temporary directory), split, downsample and the two empty dictionaries.  get_matching_indices runs for every DIRECTED pair (every
count and every match list); then cal_overlap itself runs, and its pickles give the selection of the pairs i < j and their arrays.

Scene: utils.synthetic.overlap_scene(SEED): six slabs of one room, 3.0-4.1 k points each, thr = 0.05.  Only arrays go into the
fixture (the inputs, per directed pair the count and the nearest row, the selected flags and ratios of the pairs i < j) plus the
sha256 of the script; none of its text does.

The fixture is to be reproduced EXACTLY by an fp32 search, so the generator refuses to write it unless, in float64,
    every query's nearest d2 keeps |d2 / r2 - 1| >= BAND from the threshold, and
    every query whose nearest d2 is below 1.5 r2 has (d2_second - d2_first) / d2_second >= BAND,
BAND = 2^-18: 64 units of fp32 round-off, about 8 x the rounding bound of the d2 expression plus that of r2.  Under these conditions
the fp32 kernel and the float64 reference cannot disagree on a count or an index.  The first seed that meets both is used; if none
does, change the seeds -- never BAND.
"""
import hashlib
import importlib.util
import os
import pickle
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import overlap_np as onp
from d3feat_amd.utils.synthetic import overlap_scene

REF = "/root/reference"
REL = "datasets/cal_overlap.py"
SEEDS, N_FRAG, THR = range(8), 6, 0.05
SCENE = "synthetic-room"
OUT = os.path.join(ROOT, "tests", "golden", "overlap.npz")


class DMatch:
    def __init__(self, q, t, d):
        self.queryIdx, self.trainIdx, self.distance = int(q), int(t), float(d)


class BFMatcher:
    def __init__(self, norm):
        assert norm == "NORM_L2"

    def match(self, a, b):
        assert a.dtype == np.float32 and b.dtype == np.float32
        a64, b64, out = a.astype(np.float64), b.astype(np.float64), []
        for i0 in range(0, len(a64), 512):
            d = a64[i0:i0 + 512, None, :] - b64[None, :, :]
            d2 = (d * d).sum(-1)
            j = np.argmin(d2, axis=1)                             # the first minimum
            out += [DMatch(i0 + i, j[i], np.sqrt(d2[i, j[i]])) for i in range(len(j))]
        return out


def stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.NORM_L2, cv2.BFMatcher = "NORM_L2", BFMatcher
    sys.modules.update({"open3d": types.ModuleType("open3d"), "cv2": cv2})


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s: the reference tree is needed" % REF)
    stub_modules()
    spec = importlib.util.spec_from_file_location("cal_overlap", os.path.join(REF, REL))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for seed in SEEDS:
        clouds = overlap_scene(seed, n_frag=N_FRAG, thr=THR)
        directed = [(a, b) for a in range(N_FRAG) for b in range(N_FRAG) if a != b]
        m = [onp.margins(clouds[a], clouds[b], THR) for a, b in directed]
        m_thr, m_run = min(x[0] for x in m), min(x[1] for x in m)
        print("seed %d: fragments %s, threshold margin %.3e, runner-up margin %.3e" % (seed, [len(c) for c in clouds], m_thr, m_run))
        if m_thr >= onp.BAND and m_run >= onp.BAND:
            break
    else:
        raise SystemExit("no seed of %s keeps both margins >= 2^-18: change the seeds" % (list(SEEDS),))
    ids = ["%s/seq-01/cloud_bin_%d" % (SCENE, f) for f in range(N_FRAG)]
    ld = max(len(c) for c in clouds)
    with tempfile.TemporaryDirectory() as tmp:
        obj = object.__new__(mod.ThreeDMatch)
        obj.pts = {i: c.astype(np.float64) for i, c in zip(ids, clouds)}      # np.array(pcd.points) is float64; :108-109 cast it back
        obj.scene_to_ids, obj.savepath, obj.split, obj.downsample = {SCENE: ids}, tmp, "golden", THR
        obj.overlap_ratio, obj.keypts_pairs = {}, {}
        count, nearest = np.zeros((len(directed),), np.int32), np.full((len(directed), ld), -1, np.int16)
        for p, (a, b) in enumerate(directed):
            match = obj.get_matching_indices(clouds[a], clouds[b], obj.downsample)
            count[p] = len(match)
            if len(match):
                assert np.all(np.diff(match[:, 0]) > 0)
                nearest[p, match[:, 0]] = match[:, 1]
        obj.cal_overlap(THR)
        with open(os.path.join(tmp, "3DMatch_golden_%.3f_overlap.pkl" % THR), "rb") as f:
            ratio = pickle.load(f)
        with open(os.path.join(tmp, "3DMatch_golden_%.3f_keypts.pkl" % THR), "rb") as f:
            keypts = pickle.load(f)
    upper = [(a, b) for a in range(N_FRAG) for b in range(a + 1, N_FRAG)]
    key = lambda a, b: "%s@%s" % (ids[a], ids[b])
    selected = np.array([key(a, b) in ratio for a, b in upper])
    assert set(ratio) == set(keypts) and len(ratio) == int(selected.sum())
    sel_ratio = np.array([ratio.get(key(a, b), np.nan) for a, b in upper], np.float64)
    # the arrays cal_overlap pickled are the match lists of the directed calls above
    for a, b in upper:
        if key(a, b) in keypts:
            arr, row = keypts[key(a, b)], nearest[directed.index((a, b))].astype(np.int32)
            assert arr.dtype == np.int32 and np.array_equal(arr[:, 1], row[arr[:, 0]]) and len(arr) == int((row >= 0).sum())
    all_ratio = np.array([count[directed.index(p)] / len(clouds[p[0]]) for p in upper])
    print("ratios of the pairs i < j: %s; selected %d" % (np.round(all_ratio, 3).tolist(), int(selected.sum())))
    assert 0 < selected.sum() < len(upper) and all_ratio.min() == 0.0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, points=np.concatenate(clouds, 0), lens=np.array([len(c) for c in clouds], np.int32),
                        threshold=np.float64(THR), seed=np.int32(seed), directed=np.array(directed, np.int32), count=count,
                        nearest=nearest, pairs=np.array(upper, np.int32), selected=selected, selected_ratio=sel_ratio,
                        sha256_cal_overlap=np.array(hashlib.sha256(open(os.path.join(REF, REL), "rb").read()).hexdigest()))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
