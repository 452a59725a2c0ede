"""The host side of the KITTI odometry TEST split (datasets/KITTI.py of the reference): which frame pairs are tested, the ground-truth
transform of a pair, and its two sweeps.  Pure numpy, except the ICP refinement of the ground truth (KITTI.py:293-303), which runs on
the device (d3feat_amd.icp) and only when asked for: refine_pairs / pair_transform(refine=True) write the cache files the reference
would.  By default the refined transforms are read from the cache, or the unrefined odometry is used when the caller says so.

    <root>/sequences/<drive:02d>/velodyne/<frame:06d>.bin      float32 records x, y, z, reflectance
    <root>/poses/<drive:02d>.txt                               one 3x4 camera pose per frame, row-major
    <icp_dir>/<drive>_<t0>_<t1>.npy                            f64[4,4], source (t0) -> target (t1), ICP-refined by the reference
                                                               (or by refine_pairs: the same file name, the same content rule)
"""
import glob
import os

import numpy as np

from ..utils.results import read_kitti_bin

TEST_SEQUENCES = (8, 9, 10)                     # data/kitti/config/test_kitti.txt
WRONG_PAIR = (8, 15, 58)                        # KITTI.py:123-124: "pair (8, 15, 58) is wrong"
MIN_DISTANCE, WINDOW = 10.0, 100                # KITTI.py:96,99

# KITTI.py:350-356 (the odometry benchmark's velodyne -> camera calibration, one for every sequence there)
VELO2CAM = np.vstack([np.hstack([
    np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03,
              1.480755e-02]).reshape(3, 3),
    np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01]).reshape(3, 1)]), [0, 0, 0, 1]])

_poses = {}


def velodyne_file(root, drive, t):
    return os.path.join(root, "sequences", "%02d" % drive, "velodyne", "%06d.bin" % t)


def read_poses(root, drive):
    """<root>/poses/<drive>.txt -> f64[n, 4, 4] camera poses (KITTI.py:359-367, 385-389); cached per file."""
    path = os.path.join(root, "poses", "%02d.txt" % drive)
    if path not in _poses:
        odo = np.genfromtxt(path).reshape(-1, 12)
        pos = np.zeros((odo.shape[0], 4, 4))
        pos[:, :3] = odo.reshape(-1, 3, 4)
        pos[:, 3, 3] = 1.0
        _poses[path] = pos
    return _poses[path]


def frame_numbers(root, drive):
    fnames = glob.glob(os.path.join(root, "sequences", "%02d" % drive, "velodyne", "*.bin"))
    if not fnames:
        raise FileNotFoundError("%s holds no sweeps of sequence %02d" % (root, drive))
    return sorted(int(os.path.split(f)[-1][:-4]) for f in fnames)


def test_pairs(root, sequences=TEST_SEQUENCES):
    """The pair list of KITTI.py:82-126 -> [(drive, t0, t1)]: from the first frame of a sequence, t1 is the frame before the first one
    of the next WINDOW that lies more than 10 m from t0 (camera positions of poses/<drive>.txt); the walk goes on at t1 + 1; a frame
    without such a successor is skipped (`curr_time += 1`).  (8, 15, 58) is removed if present.  The reference's loop never ends when
    frame numbers have a gap (its t1 is then no frame and t0 does not advance): that is a ValueError here."""
    files = []
    for drive in sequences:
        drive = int(drive)
        inames = frame_numbers(root, drive)
        if inames != list(range(inames[0], inames[0] + len(inames))):
            missing = sorted(set(range(inames[0], inames[-1] + 1)) - set(inames))
            raise ValueError("sequence %02d: frame numbers with gaps (frame %06d is missing): the pair list is undefined"
                             % (drive, missing[0]))
        Ts = read_poses(root, drive)[:, :3, 3]
        if Ts.shape[0] <= inames[-1]:
            raise ValueError("sequence %02d: %d poses for frames up to %06d" % (drive, Ts.shape[0], inames[-1]))
        curr, last = inames[0], inames[-1]
        while curr <= last:
            d = Ts[curr:curr + WINDOW] - Ts[curr]
            far = np.where(np.sqrt((d ** 2).sum(-1)) > MIN_DISTANCE)[0]
            if len(far) == 0:
                curr += 1
                continue
            nxt = int(far[0]) + curr - 1
            if nxt > last:                                            # more poses than sweeps: the reference would not end either
                raise ValueError("sequence %02d: frame %06d pairs with %06d, beyond the last sweep %06d" % (drive, curr, nxt, last))
            files.append((drive, curr, nxt))
            curr = nxt + 1
    if WRONG_PAIR in files:
        files.remove(WRONG_PAIR)
    return files


test_pairs.__test__ = False                     # (a function of the package, not a test)


def odometry_transform(root, drive, t0, t1):
    """The unrefined M of KITTI.py:288-289: source (t0) -> target (t1) velodyne frames from the two camera poses, f64[4,4]."""
    pos = read_poses(root, drive)
    v2c = VELO2CAM.T                                                  # the reference keeps the transpose (:356)
    return (v2c @ pos[t0].T @ np.linalg.inv(pos[t1].T) @ np.linalg.inv(v2c)).T


def cache_file(root, drive, t0, t1, icp_dir=None):
    icp_dir = icp_dir if icp_dir is not None else os.path.join(root, "icp")
    return os.path.join(icp_dir, "%d_%d_%d.npy" % (drive, t0, t1))


def refine_pairs(root, pairs, icp_dir=None, batch=16, check_every=8):
    """For every (drive, t0, t1) of `pairs` without a cache file: the ICP-refined ground truth of KITTI.py:288-303, computed on the
    device `batch` pairs per call (d3feat_amd.icp.icp_pairs with ICP_KITTI) and np.save'd where the reference would -> the number of
    files written.  The file holds WHAT THE REFERENCE WRITES: M2 = M @ T_icp (KITTI.py:300, in that order), M the odometry transform and
    T_icp the ICP from the identity on the sweep pre-moved by M.

    The one deliberate difference: the reference moves the sweep by M once (apply_transform), hands the moved points to Open3D, and
    Open3D accumulates its updates on those moved points.  Here the device call gets init = M and the RAW float32 rows, and moves them
    by the accumulated float64 transform T in every round; T_icp = T M^-1 is recovered on the host in float64.  The same algebra, one
    rounding of the moved points less."""
    from .. import icp as _icp
    todo = [(int(d), int(t0), int(t1)) for d, t0, t1 in pairs if not os.path.exists(cache_file(root, int(d), int(t0), int(t1), icp_dir))]
    todo = list(dict.fromkeys(todo))
    for a in range(0, len(todo), max(int(batch), 1)):
        part = todo[a:a + max(int(batch), 1)]
        sweeps = [read_pair(root, d, t0, t1) for d, t0, t1 in part]
        M = np.stack([odometry_transform(root, d, t0, t1) for d, t0, t1 in part])
        src = np.concatenate([np.ascontiguousarray(s[0], np.float32).reshape(-1, 3) for s in sweeps])
        tgt = np.concatenate([np.ascontiguousarray(s[1], np.float32).reshape(-1, 3) for s in sweeps])
        res = _icp.icp_pairs(src, [len(s[0]) for s in sweeps], tgt, [len(s[1]) for s in sweeps], init=M, check_every=check_every,
                             **_icp.ICP_KITTI)
        T = np.asarray(res.transformation, np.float64)
        for (d, t0, t1), Mi, Ti in zip(part, M, T):
            T_icp = Ti @ np.linalg.inv(Mi)
            path = cache_file(root, d, t0, t1, icp_dir)
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            np.save(path, Mi @ T_icp)
    return len(todo)


def pair_transform(root, drive, t0, t1, icp_dir=None, odometry_gt=False, refine=False):
    """Ground truth of a test pair, source (t0) -> target (t1), f64[4,4] (KITTI.py:283-310): <icp_dir>/<drive>_<t0>_<t1>.npy when it
    exists -- the ICP-refined cache, the reference's or refine_pairs'.  Without it: FileNotFoundError naming the file, unless
    refine=True computes and caches it (refine_pairs; needs the GPU), or odometry_gt=True asks for the unrefined odometry transform
    (:288-289), which is never written to the cache.  A missing cache never silently changes the metric."""
    path = cache_file(root, drive, t0, t1, icp_dir)
    if not os.path.exists(path) and refine:
        refine_pairs(root, [(drive, t0, t1)], icp_dir=icp_dir)
    if os.path.exists(path):
        M = np.load(path)
        if M.shape != (4, 4):
            raise ValueError("%s: a transform of shape %s" % (path, M.shape))
        return M
    if not odometry_gt:
        raise FileNotFoundError("%s: no ICP-refined ground truth for pair (%d, %d, %d) -- copy the reference's cache, compute it with "
                                "refine=True (tools/kitti_icp.py), or pass odometry_gt=True for the unrefined odometry"
                                % (path, drive, t0, t1))
    return odometry_transform(root, drive, t0, t1)


def read_pair(root, drive, t0, t1):
    """The two sweeps of a pair -> (xyz0 f32[n0,3], xyz1 f32[n1,3])  (KITTI.py:273-281)."""
    return read_kitti_bin(velodyne_file(root, drive, t0)), read_kitti_bin(velodyne_file(root, drive, t1))
