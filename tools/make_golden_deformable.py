#!/usr/bin/env python3
"""tests/golden/deformable.npz: what the REFERENCE'S OWN PYTHON computes for the deformable KPConv.

Works like tools/make_golden_network.py: /root/reference and oracle/tf_eager (the numpy float32 eager stand-in named `tensorflow`)
go on sys.path and the reference's kernels/convolution_ops.py and models/network_blocks.py run UNMODIFIED (their sha256 are stored
in the fixture).  The stand-in lacks four things the deformable code touches; they are supplied here, at run time, without editing
anything under oracle/ or in the reference:

  * tf.add(x, y, name=...)                                                         (convolution_ops.py:424)
  * tf.batch_gather with trailing dimensions: params of rank 3, indices of rank 2  (:447)
  * tf.Variable returning an array whose .shape has as_list()                      (:325)
  * a working directory where kernels/kernel_points.py may write its disposition file

Recorded:
  (a) ops/<influence>/<aggregation>/<mod|plain>: KPConv_deform_ops on one synthetic case (tests/deformable_cases.py: 40 queries,
      12 neighbour slots, Cin 8, Cout 12, non-zero offsets; shadow slots point at the shadow row, as the reference requires);
  (b) block/<name>/<mod|plain>: resnetb_deformable_block and resnetb_deformable_strided_block on a crop of a demo cloud, with every
      variable the block created (in creation order), its inputs, its output and the raw output of the offset convolution.  The
      offset weights are seeded non-zero and scaled (from a first pass) so that the largest |offset| is 0.3 KP_extent.

    python tools/make_golden_deformable.py        # needs /root/reference
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_network as mgn      # noqa: E402  (setup_imports, crop: the same import discipline)

REF = mgn.REF
OUT = os.path.join(ROOT, "tests", "golden")
SEED = 20261019
REF_FILES = ["kernels/convolution_ops.py", "kernels/kernel_points.py", "models/network_blocks.py", "utils/config.py"]
LIMIT = 40          # neighbour columns kept (the nearest: the searches return them in order of distance)
TARGET = 0.3        # largest |offset| / KP_extent of the block fixtures


class _Shape(tuple):
    def as_list(self):
        return list(self)


class _Var(np.ndarray):
    """An ndarray whose .shape answers as_list(), as a tf.Variable's TensorShape does."""
    @property
    def shape(self):
        return _Shape(np.ndarray.shape.__get__(self))


def install_shims(tf):
    orig_variable = tf.Variable

    def Variable(*a, **k):
        return np.asarray(orig_variable(*a, **k)).view(_Var)

    def add(x, y, name=None):
        return np.asarray(x) + y

    def batch_gather(params, indices):
        p, i = np.asarray(params), np.asarray(indices).astype(np.int64)
        assert i.ndim == 2 and p.ndim in (2, 3)
        return p[np.arange(p.shape[0])[:, None], i]
    tf.Variable, tf.add, tf.batch_gather = Variable, add, batch_gather


def run_ops(conv_ops, out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deformable_cases as dc
    from oracle import kpconv_cases as kc
    c = dc.deform_case(SEED % 100000, 8, 12, 40, cap_q=0, cap_s=0)
    idx = np.where((c.idx >= 0) & (c.idx < c.Ns), c.idx, c.Ns).astype(np.int32)      # the reference gathers row Ns for a shadow
    P = c.KP.shape[0]
    e = np.float32(dc.EXTENT)
    offsets = (c.raw[:, :3 * P].reshape(-1, P, 3) * e).astype(np.float32)
    mods = (2.0 / (1.0 + np.exp(-c.raw[:, 3 * P:].astype(np.float64)))).astype(np.float32)
    W = kc.weights(SEED % 1000, P, 8, 12)
    out.update({"ops/q": c.q, "ops/s": c.s, "ops/idx": idx, "ops/f": c.f, "ops/kp": c.KP, "ops/offsets": offsets, "ops/modulations": mods,
                "ops/raw": c.raw, "ops/w": W, "ops/extent": e})
    for infl, agg in kc.MODES:
        for tag, m in (("plain", None), ("mod", mods)):
            got = conv_ops.KPConv_deform_ops(c.q, c.s, idx, c.f, c.KP, offsets, m, W, float(e), infl, agg)
            out["ops/%s/%s/%s" % (infl, agg, tag)] = np.asarray(got, np.float32)


def run_block(tf, conv_ops, network_blocks, cfg, name, modulated, inputs, features, out):
    cfg.modulated = modulated
    tag = "block/%s/%s" % (name, "mod" if modulated else "plain")
    fn = getattr(network_blocks, name + "_block")
    fdim, radius = 32, cfg.first_subsampling_dl * cfg.density_parameter
    rng = np.random.default_rng(SEED + (1 if modulated else 0) + (2 if "strided" in name else 0))
    drawn = {}

    def run(scale):
        created, raw = [], {}

        def hook(full, default):
            leaf = full.rsplit("/", 1)[-1]
            if full not in drawn:
                if leaf == "weights":
                    drawn[full] = (rng.standard_normal(default.shape) * np.sqrt(2.0 / default.shape[-1])).astype(np.float32)
                elif leaf == "offset_conv_weights":
                    drawn[full] = (rng.standard_normal(default.shape) / np.sqrt(default.shape[0] * default.shape[1])).astype(np.float32)
                elif leaf == "offset_conv_bias":
                    drawn[full] = (0.2 * rng.standard_normal(default.shape)).astype(np.float32)
                elif leaf == "gamma":
                    drawn[full] = (1.0 + 0.2 * rng.standard_normal(default.shape)).astype(np.float32)
                elif leaf in ("beta", "moving_mean"):
                    drawn[full] = (0.1 * rng.standard_normal(default.shape)).astype(np.float32)
                elif leaf == "moving_variance":
                    drawn[full] = (0.5 + rng.random(default.shape)).astype(np.float32)
                else:                                       # kernel_points: what the reference's own load_kernels created
                    drawn[full] = np.ascontiguousarray(default, np.float32)
            v = drawn[full]
            if leaf in ("offset_conv_weights", "offset_conv_bias"):
                assert not np.any(default), "the reference initialises %s with zeros" % full
                v = (v * np.float32(scale)).astype(np.float32)
            created.append((full, v))
            return v
        orig = conv_ops.KPConv_ops

        def KPConv_ops(*a, **k):
            r = orig(*a, **k)
            raw["x"] = np.asarray(r, np.float32)
            return r
        tf.reset_default_graph()
        tf.set_variable_hook(hook)
        np.random.seed(SEED % (2 ** 31))
        conv_ops.KPConv_ops = KPConv_ops
        try:
            with tf.variable_scope("b"):
                y = fn(0, inputs, features, radius, fdim, cfg, False)
        finally:
            conv_ops.KPConv_ops = orig
            tf.set_variable_hook(None)
        bias = dict(created)["b/conv2/offset_conv_bias"]
        return np.asarray(y, np.float32), created, raw["x"] + bias

    _, _, raw = run(1.0)
    P = cfg.num_kernel_points
    big = np.linalg.norm(raw[:, :3 * P].reshape(-1, P, 3), axis=-1).max()
    y, created, raw = run(TARGET / big)
    reach = np.linalg.norm(raw[:, :3 * P].reshape(-1, P, 3), axis=-1).max()
    assert abs(reach - TARGET) < 1e-3, reach
    out[tag + "/out"] = y
    out[tag + "/raw"] = raw.astype(np.float32)
    out[tag + "/varlist"] = np.asarray(json.dumps([[n[2:], list(v.shape)] for n, v in created]))
    for n, v in created:
        out[tag + "/var/" + n[2:]] = v
    print("%-52s out %s  max |offset| / KP_extent %.3f" % (tag, y.shape, reach))


def main():
    tf = mgn.setup_imports()
    install_shims(tf)
    from oracle.clib import COracle
    work = tempfile.mkdtemp(prefix="d3f_golden_deform_")
    os.chdir(work)                                # kernels/kernel_points.py writes kernels/dispositions/ under the cwd
    import kernels.convolution_ops as conv_ops
    import models.network_blocks as network_blocks
    from utils.config import Config
    for m in (conv_ops, network_blocks):
        assert os.path.realpath(m.__file__).startswith(REF + "/"), m.__file__
    out = {}
    run_ops(conv_ops, out)

    cfg = Config()
    cfg.load(os.path.join(REF, "results", "Log_contraloss"))
    co = COracle()
    p0 = mgn.crop(np.load(os.path.join(OUT, "demo_bin0_sub003.npy")), 4000, 300)
    l0 = np.asarray([len(p0)], np.int32)
    dl = cfg.first_subsampling_dl
    p1, l1 = co.batch_grid_subsampling(p0, l0, np.float32(2 * dl))
    r = np.float32(dl * cfg.density_parameter)    # datasets/common.py:1344,1363: the search radius of a layer with a deformable block
    nb = co.batch_neighbors(p0, p0, l0, l0, r)[:, :LIMIT]
    pool = co.batch_neighbors(p1, p0, l1, l0, r)[:, :LIMIT]
    inputs = dict(points=[p0, np.ascontiguousarray(p1, np.float32)], neighbors=[nb.astype(np.int32)], pools=[pool.astype(np.int32)])
    rng = np.random.default_rng(SEED + 99)
    feats = np.maximum(rng.standard_normal((len(p0), 32)), 0.2 * rng.standard_normal((len(p0), 32))).astype(np.float32)
    out.update({"block/points_0": p0, "block/points_1": inputs["points"][1], "block/neighbors_0": inputs["neighbors"][0],
                "block/pools_0": inputs["pools"][0], "block/features": feats, "block/fdim": np.int32(32),
                "block/radius": np.float64(dl * cfg.density_parameter)})
    for name in ("resnetb_deformable", "resnetb_deformable_strided"):
        for modulated in (False, True):
            run_block(tf, conv_ops, network_blocks, cfg, name, modulated, inputs, feats, out)
    out["reference_sources"] = np.asarray(json.dumps({f: hashlib.sha256(open(os.path.join(REF, f), "rb").read()).hexdigest()
                                                      for f in REF_FILES}))
    out["generated_with"] = np.asarray("oracle/tf_eager (numpy %s float32 eager stand-in for tensorflow 1.12)" % np.__version__)
    fn = os.path.join(OUT, "deformable.npz")
    np.savez_compressed(fn, **out)
    # (tests/golden/MANIFEST.json lists the fixtures of the geometry and network generators; this one carries the hashes of the
    # reference sources it ran inside itself and is left out of that file)
    print("deformable.npz %.2f MB" % (os.path.getsize(fn) / 1e6))


if __name__ == "__main__":
    main()
