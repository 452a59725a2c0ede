#!/usr/bin/env python3
"""Fills the ICP-refined ground-truth cache of the KITTI test split on the device (datasets/KITTI.py:283-306 of the reference does it
pair by pair with Open3D on one CPU core, the first time a pair is read), and optionally goes straight on to the KITTI test:

    python tools/kitti_icp.py --root data/kitti [--icp-dir DIR] [--sequences 8,9,10] [--batch 16]
    python tools/kitti_icp.py --root data/kitti --weights results_kitti/Log_xxx [--out DIR] [... any option of tools/kitti_test.py]

Every test pair (datasets/kitti.test_pairs) without <icp-dir>/<drive>_<t0>_<t1>.npy gets one: kitti.refine_pairs, `batch` pairs per
device call.  Existing files are left alone.  With --weights the KITTI test (tools/kitti_test.py, in this process, with the same
--root / --icp-dir / --sequences and every option this tool does not know) runs afterwards: one command from a plain KITTI download
to the reference's figures.  tools/kitti_test.py itself has no such switch; started on its own it reads the cache this tool writes.
"""
import argparse
import importlib.util
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from d3feat_amd.datasets import kitti  # noqa: E402


def kitti_test_module():
    spec = importlib.util.spec_from_file_location("kitti_test", os.path.join(HERE, "kitti_test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="data/kitti")
    ap.add_argument("--icp-dir", default=None, help="default: <root>/icp")
    ap.add_argument("--sequences", default=",".join(str(s) for s in kitti.TEST_SEQUENCES))
    ap.add_argument("--batch", type=int, default=16, help="pairs per device call")
    ap.add_argument("--weights", default=None, help="then run tools/kitti_test.py with these weights and the remaining options")
    args, rest = ap.parse_known_args(argv)
    if rest and args.weights is None:
        ap.error("unknown options %s (options of tools/kitti_test.py need --weights)" % rest)
    pairs = kitti.test_pairs(args.root, [int(s) for s in args.sequences.split(",")])
    t0 = time.time()
    n = kitti.refine_pairs(args.root, pairs, icp_dir=args.icp_dir, batch=args.batch)
    print("%d test pairs, %d cache files written in %.1f s" % (len(pairs), n, time.time() - t0))
    if args.weights is not None:
        test_argv = ["--root", args.root, "--weights", args.weights, "--sequences", args.sequences]
        test_argv += ["--icp-dir", args.icp_dir] if args.icp_dir is not None else []
        old = sys.argv
        sys.argv = [os.path.join(HERE, "kitti_test.py")] + test_argv + rest
        try:
            kitti_test_module().main()
        finally:
            sys.argv = old
    return n


if __name__ == "__main__":
    main()
