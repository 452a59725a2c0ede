"""The deformable KPConv on the host: tests/deformable_np.py (the float64 restatement every GPU test of the operator compares with)
against what the reference's own Python computed (tests/golden/deformable.npz, tools/make_golden_deformable.py), and the model-side
plumbing that needs no GPU: variable names / shapes / order, a checkpoint round trip with the two new names, the block table.

Bars.  The fixture holds float32 results of numpy kernels (oracle/tf_eager), the restatement is float64: the bar is what float32
arithmetic can differ by, derived in deformable_np (c_h, out_bound, block_bound) from K, Cin, the offsets' size and the magnitudes
in the file -- never from a measured difference.  Each test prints the largest error / bound it saw.
Seen: operator 0.005 .. 0.013 of the bound over the twelve mode combinations (the bound takes a 120-term contraction with
absolute values); blocks 1e-4 .. 4e-4 of theirs, 3.8e-6 absolute at outputs of up to 15."""
import json
import os

import numpy as np
import pytest

import deformable_np as dn
from conftest import GOLDEN, write_tf_bundle


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "deformable.npz"))


def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max())


def _cfg(modulated):
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    cfg.modulated = bool(modulated)
    return cfg


@pytest.mark.parametrize("tag", ["plain", "mod"])
@pytest.mark.parametrize("agg", ["sum", "closest"])
@pytest.mark.parametrize("infl", ["constant", "linear", "gaussian"])
def test_operator_restatement_matches_the_reference(gold, infl, agg, tag):
    """KPConv_deform_ops, six modes x with / without modulations: the mask form equals the reference's compaction."""
    g = gold
    a = (g["ops/q"], g["ops/s"], g["ops/idx"], g["ops/f"], g["ops/kp"], g["ops/offsets"], g["ops/modulations"] if tag == "mod" else None,
         g["ops/w"], float(g["ops/extent"]), infl, agg)
    r = dn.kpconv_deform_f64(*a)
    want = g["ops/%s/%s/%s" % (infl, agg, tag)]
    ratio = _ratio(r["out"], want, dn.out_bound(*a))
    print("KPConv_deform_ops %s / %s / %s: error / bound %.3f" % (infl, agg, tag, ratio))
    assert ratio <= 1.0
    kept, valid = r["in_range"].sum(), r["valid"].sum()
    assert 0 < kept < valid                                  # the range filter dropped some neighbours and kept some


def _block_inputs(g):
    return dict(points=[g["block/points_0"], g["block/points_1"]], neighbors=[g["block/neighbors_0"]], pools=[g["block/pools_0"]])


def _block_vars(g, tag):
    return {"b/" + n: g["%s/var/%s" % (tag, n)] for n, _ in json.loads(str(g[tag + "/varlist"]))}


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "mod"])
@pytest.mark.parametrize("name", ["resnetb_deformable", "resnetb_deformable_strided"])
def test_block_restatement_matches_the_reference(gold, name, modulated):
    tag = "block/%s/%s" % (name, "mod" if modulated else "plain")
    cfg = _cfg(modulated)
    out, bound = dn.block_bound(0, _block_inputs(gold), gold["block/features"], float(gold["block/radius"]), int(gold["block/fdim"]), cfg,
                                _block_vars(gold, tag), "b", strided="strided" in name)
    plain = dn.resnetb_deformable_f64(0, _block_inputs(gold), gold["block/features"], float(gold["block/radius"]), int(gold["block/fdim"]),
                                      cfg, _block_vars(gold, tag), "b", strided="strided" in name)
    assert np.array_equal(out, plain)                        # (the bound's own forward is the restatement)
    ratio = _ratio(out, gold[tag + "/out"], bound)
    print("%s: error / bound %.4f, largest bound %.2e, largest |out| %.2f" % (tag, ratio, bound.max(), np.abs(out).max()))
    assert ratio <= 1.0
    # the worst-case bound takes every sum of three chained contractions with absolute values and is loose (0.1 .. 0.4 here); the
    # project's parity bar (BASELINE.json: 1e-4) is what the GPU tests of the blocks hold, and the float32 reference meets it too
    assert np.abs(out - gold[tag + "/out"]).max() <= 1e-4
    reach = np.linalg.norm(gold[tag + "/raw"][:, :45].reshape(-1, 15, 3), axis=-1).max()
    assert 0.29 < reach < 0.31                               # the fixture's offsets are not small


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "mod"])
def test_build_variables_creates_the_reference_variables_in_its_order(gold, modulated):
    """One deformable block as a whole architecture stage: names, shapes and creation order of its variables equal the list the
    reference's block created (conv2: weights, kernel_points, offset_conv_weights, offset_conv_bias, the batch-norm quartet)."""
    from d3feat_amd.models.variables import build_variables
    cfg = _cfg(modulated)
    cfg.architecture = ["resnetb_deformable", "resnetb_deformable_strided", "resnetb", "nearest_upsample", "unary", "last_unary"]
    cfg.num_layers = 2
    cfg.first_features_dim = 32
    for block, scope in (("resnetb_deformable", "layer_0/resnetb_0"), ("resnetb_deformable_strided", "layer_0/resnetb_strided_1")):
        vs = build_variables(cfg, in_features_dim=32)
        want = json.loads(str(gold["block/%s/%s/varlist" % (block, "mod" if modulated else "plain")]))
        got = [[n[len(scope) + 1:], list(v.shape)] for n, v in vs.values.items() if n.startswith(scope + "/")]
        if block.endswith("strided"):      # the fixture's block saw 32 input channels, this one the 64 of the block before it
            want = [[n, ([64] + s[1:]) if n in ("conv1/weights", "shortcut/weights") else s] for n, s in want if not n.startswith("shortcut")]
            got = [e for e in got if not e[0].startswith("shortcut")]
        assert got == want
    conv2 = [n.rsplit("/", 1)[-1] for n in vs.values if n.startswith("layer_0/resnetb_0/conv2/") and "batch_norm" not in n]
    assert conv2 == ["weights", "kernel_points", "offset_conv_weights", "offset_conv_bias"]
    D = 60 if modulated else 45
    assert vs.values["layer_0/resnetb_0/conv2/offset_conv_weights"].shape == (15, 16, D)
    assert not vs.values["layer_0/resnetb_0/conv2/offset_conv_weights"].any() and not vs.values["layer_0/resnetb_0/conv2/offset_conv_bias"].any()
    rnd = build_variables(cfg, in_features_dim=32, randomize_offsets=True)
    assert list(rnd.values) == list(vs.values)
    assert rnd.values["layer_0/resnetb_0/conv2/offset_conv_weights"].any() and rnd.values["layer_0/resnetb_0/conv2/offset_conv_bias"].any()
    # a rigid architecture draws exactly what it drew before the option existed
    rigid = _cfg(False)
    a, b = build_variables(rigid, seed=3), build_variables(rigid, seed=3, randomize_offsets=True)
    assert all(np.array_equal(a.values[k], b.values[k]) for k in a.values) and list(a.values) == list(b.values)


def test_checkpoint_round_trip_with_the_offset_variables(tmp_path):
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils import tf_checkpoint as tc
    cfg = _cfg(True)
    cfg.architecture = ["simple", "resnetb_deformable", "resnetb_deformable_strided", "resnetb_deformable", "nearest_upsample", "unary",
                        "last_unary"]
    cfg.num_layers = 2
    cfg.first_features_dim = 16
    vs = build_variables(cfg, seed=5, randomize_bn=True, randomize_offsets=True)
    names = [n for n in vs.values if n.endswith(("offset_conv_weights", "offset_conv_bias"))]
    assert len(names) == 6
    prefix = str(tmp_path / "snap-1")
    write_tf_bundle(prefix, {"KernelPointNetwork/" + n: v for n, v in vs.values.items()})
    back = tc.load_checkpoint(prefix, verify_crc=True)
    assert set(back) == set(vs.values)
    for n in vs.values:
        assert np.array_equal(back[n], vs.values[n]), n


def test_block_table():
    from d3feat_amd.models import network_blocks as nb
    assert nb.get_block_ops("resnetb_deformable").__name__ == "resnetb_deformable_block"
    assert nb.get_block_ops("resnetb_deformable_strided").__name__ == "resnetb_deformable_strided_block"
    for name in ("inception_deformable", "inception_deformable_strided"):
        with pytest.raises(NotImplementedError):
            nb.get_block_ops(name)
    from compat.kernels import convolution_ops as cc
    from d3feat_amd.kernels import convolution_ops as co
    assert cc.KPConv_deformable is co.KPConv_deformable and cc.KPConv_deform_ops is co.KPConv_deform_ops


def test_parameters_file_with_deformable_blocks_builds(tmp_path):
    """A run's parameters.txt whose architecture lists the deformable blocks: Config.load reads it back (`modulated` included), every
    block name resolves and the variables of the whole network can be created."""
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import build_variables
    from d3feat_amd.utils.config import Config
    cfg = _cfg(True)
    arch = list(cfg.architecture)
    arch[7:10] = ["resnetb_deformable", "resnetb_deformable_strided", "resnetb_deformable"]
    cfg.architecture = arch
    cfg.save(str(tmp_path))
    back = Config()
    back.load(str(tmp_path))
    assert list(back.architecture) == arch and back.modulated is True
    for block in arch:
        assert callable(nb.get_block_ops(block))
    vs = build_variables(back)
    for scope, ci in (("layer_3/resnetb_0", 256), ("layer_3/resnetb_strided_1", 256), ("layer_4/resnetb_0", 512)):
        assert vs.values[scope + "/conv2/offset_conv_weights"].shape == (15, ci, 60)
        assert vs.values[scope + "/conv2/offset_conv_bias"].shape == (60,)
