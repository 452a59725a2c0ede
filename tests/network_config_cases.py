"""TEST INFRASTRUCTURE ONLY: no tests in here.

The configurations at which tests/test_network_config_host.py (CPU) and tests/test_gpu_network_configs.py (MI355X) run the whole
network, with their inputs, weights and float64 reference (tests/network_f64_np.py).  Every case changes one thing from
threedmatch_config() unless its line says otherwise; `shipped` is the control, the only point the rest of the suite runs.

Inputs: room_fragment(5, n_raw=3000, edge=1.0) subsampled at 0.03 by the C oracle and stacked with itself (5192 / 3442 / 1190 / 324 /
80 rows at the five levels: the smallest cloud whose level 4 still has a few tiles), the pyramid from oracle.network_np.descriptor_input
over the C oracle's search and subsampling -- only the network is under test.

Weights: build_variables(cfg, seed, randomize_bn=True), then
  * without batch norm every `offset` is drawn N(0, 0.1) (zeros would hide a dropped offset);
  * kernel points of a count other than 15 are drawn directly (as oracle/kpconv_cases.kernel_points: random directions, radii uniform
    in the ball of 1.5 * extent, the first point at the centre) -- create_kernel_points would optimise and cache a new disposition;
  * the `beta` (without batch norm: the `offset`) of every conv1 and of layer_0/simple_0 is shifted DOWN by the case's `shift`, so
    that the row sums entering the KPConvs have mixed signs: with the unshifted weights no neighbour is ever left uncounted
    (kernels/convolution_ops.py:250-251) and the plumbing of that rule between blocks could be wrong unnoticed.

CONDITIONS, asserted by check_conditions() on what this module returns (they are not exclusions from any comparison):
  1. 'closest' cases: in the neighbour and pool matrix of every level, a valid slot whose two smallest squared distances to the kernel
     points of a KPConv that reads the matrix differ by less than 1e-4 relative (oracle.kpconv_cases._closest_margin) is replaced by
     the shadow index -- the same matrices go to the reference and to the device; none is left, and at most 0.1 % of a matrix's valid
     slots are replaced;
  2. no row entering a KPConv has |sum f| < 1e-5 * sum |f| in the float64 reference, and the float32 CPU evaluation of the same
     network (oracle.network_np.forward) gives every row sum the same sign;
  3. at least three KPConv inputs have a share of non-positive row sums between 5 % and 95 %.
`seed` and `shift` are constants of each case, chosen (by search, on the CPU, against the float64 reference alone) so that 2 and 3 hold.
"""
import contextlib
import copy
import functools

import numpy as np

LIMITS = np.asarray([37, 35, 36, 38, 38], np.int32)
CLOUD_SEED, N_RAW, DL = 5, 3000, 0.03
BAR = 1e-4                   # BASELINE.json north star, TOL of the existing network tests
MARGIN = 1e-5                # condition 2
MAX_REPLACED = 1e-3          # condition 1
ENGINE_MARGIN = 2.0 ** -18   # condition 1 on index matrices that cannot be edited (engine_inputs)

_THREE_LAYERS = ["simple", "resnetb", "resnetb_strided", "resnetb", "resnetb_strided", "resnetb", "nearest_upsample", "unary",
                 "nearest_upsample", "unary", "last_unary"]

# id -> (what changes from threedmatch_config(), weight seed, beta shift)
CASES = {
    "shipped": (dict(), 0, 1.0),
    "constant": (dict(KP_influence="constant"), 1, 0.32),
    "gaussian": (dict(KP_influence="gaussian"), 0, 1.0),
    "closest": (dict(convolution_mode="closest"), 0, 0.64),
    "class_defaults": (dict(KP_influence="gaussian", convolution_mode="closest"), 0, 1.0),
    "no_bn": (dict(use_batch_norm=False), 0, 0.64),
    "w32": (dict(first_features_dim=32), 0, 0.64),
    "w128": (dict(first_features_dim=128), 0, 0.64),
    "w18": (dict(first_features_dim=18), 1, 0.64),
    "kp13": (dict(num_kernel_points=13), 0, 1.5),
    "kp4": (dict(num_kernel_points=4), 0, 0.64),
    "cin4": (dict(in_features_dim=4), 1, 0.64),
    "geometry": (dict(KP_extent=1.2, density_parameter=3.0), 0, 2.5),
    "three_layers": (dict(architecture=_THREE_LAYERS), 0, 1.0),
    "mixed": (dict(use_batch_norm=False, KP_influence="gaussian", convolution_mode="closest", first_features_dim=32,
                   num_kernel_points=13), 4, 0.64),
}
# Input features are ones (in_features_dim = 1), except: cin4 (the issue's N(0, 1) columns), and constant -- with ones, KP_influence =
# 'constant' makes every row of every block the SAME vector (each kernel point weighs every neighbour 1, and the sum is divided by
# the neighbour count), so no shift can mix the signs of its row sums (condition 3) and an error that permutes rows could not show:
# this case feeds one N(0, 1) column, which also makes the Cin = 1 kernel count by the sign of its feature.
RANDOM_FEATURES = ("cin4", "constant")
# max deviation of the float32 CPU oracle from the float64 definition (deviation() below), as tests/test_network_config_host.py
# prints it, rounded up to two digits: what bar() rests on.  None reaches 2.5e-5 -- not even no_bn, whose activations nothing renormalises
# -- so every case's bar is the project's 1e-4.
CPU_DEVIATION = {"shipped": 2.3e-6, "constant": 2.8e-6, "gaussian": 2.4e-6, "closest": 1.5e-6, "class_defaults": 3.2e-6, "no_bn": 2.6e-6,
                 "w32": 1.7e-6, "w128": 1.9e-6, "w18": 7.3e-6, "kp13": 1.6e-6, "kp4": 1.6e-6, "cin4": 1.6e-6, "geometry": 2.3e-6,
                 "three_layers": 1.3e-6, "mixed": 2.0e-6}


def bar(case):
    """The bound of the GPU comparison: 1e-4, or four times the case's float32-CPU-against-float64 figure where that exceeds 2.5e-5
    (another summation order and FMA contraction on the device: a factor of four over one float32 evaluation's own error)."""
    cpu = CPU_DEVIATION[case]
    return BAR if cpu <= BAR / 4 else 4 * cpu


def config(case):
    from d3feat_amd.utils.config import threedmatch_config
    cfg = threedmatch_config()
    for k, v in CASES[case][0].items():
        setattr(cfg, k, copy.copy(v))
    cfg.__init__()
    return cfg


@functools.lru_cache(maxsize=None)
def raw_cloud():
    from d3feat_amd.utils.synthetic import room_fragment
    return room_fragment(CLOUD_SEED, n_raw=N_RAW, edge=1.0)


@functools.lru_cache(maxsize=None)
def cloud():
    from oracle.clib import COracle
    return COracle().grid_subsampling(raw_cloud(), DL)


def limits(cfg):
    return LIMITS[:cfg.num_layers].copy()


@functools.lru_cache(maxsize=None)
def _pyramid(KP_extent, arch):
    """The oracle pyramid of the self-pair: it depends on the search radii (KP_extent) and on the architecture only."""
    from d3feat_amd.utils.config import threedmatch_config
    from oracle import network_np as onp
    from oracle.clib import COracle
    co = COracle()
    cfg = threedmatch_config()
    cfg.KP_extent, cfg.architecture = KP_extent, list(arch)
    cfg.__init__()
    c = cloud()
    pts = np.concatenate([c, c])
    lens = np.asarray([len(c)] * 2, np.int32)
    return onp.descriptor_input(cfg, pts, np.ones((len(pts), 1), np.float32), lens, limits(cfg),
                                lambda q, s, ql, sl, r: co.batch_neighbors(q, s, ql, sl, r),
                                lambda p, l, dl: co.batch_grid_subsampling(p, l, dl))


def drawn_kernel_points(radius, num_kp, rng):
    d = rng.standard_normal((num_kp, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kp = (d * (rng.random((num_kp, 1)) ** (1.0 / 3.0)) * radius * 0.999).astype(np.float32)
    kp[0] = 0
    return kp


def _shifted_names(W):
    tails = ("conv1/batch_normalization/beta", "conv1/offset")
    heads = ("layer_0/simple_0/batch_normalization/beta", "layer_0/simple_0/offset")
    return [n for n in W if n.endswith(tails) or n in heads]


def build_weights(cfg, seed, shift):
    from d3feat_amd.models.variables import build_variables
    kp = None if cfg.num_kernel_points == 15 else drawn_kernel_points
    W = dict(build_variables(cfg, seed, randomize_bn=True, kernel_points=kp).values)
    rng = np.random.default_rng(10000 + seed)
    for n in W:
        if n.endswith("/offset"):
            W[n] = (0.1 * rng.standard_normal(W[n].shape)).astype(np.float32)
    for n in _shifted_names(W):
        W[n] = (W[n] - np.float32(shift)).astype(np.float32)
    return W


@functools.lru_cache(maxsize=None)
def weights(case, shifted=True):
    _, seed, shift = CASES[case]
    return build_weights(config(case), seed, shift if shifted else 0.0)


def kpconv_readers(cfg):
    """-> {("neighbors" | "pools", level): [variable scopes of the KPConvs that read that matrix]}."""
    out, layer, bil = {}, 0, 0
    for block in cfg.architecture:
        if "upsample" in block:
            break
        scope = "layer_%d/%s_%d" % (layer, block, bil)
        if block == "simple":
            out.setdefault(("neighbors", layer), []).append(scope)
        elif block == "resnetb":
            out.setdefault(("neighbors", layer), []).append(scope + "/conv2")
        elif block == "resnetb_strided":
            out.setdefault(("pools", layer), []).append(scope + "/conv2")
        bil += 1
        if "strided" in block:
            layer, bil = layer + 1, 0
    return out


def near_ties(cfg, W, inp):
    """-> {(matrix, level): bool [rows, K], the slots of condition 1}."""
    from oracle.kpconv_cases import _closest_margin
    out = {}
    for (key, l), scopes in kpconv_readers(cfg).items():
        idx = inp[key][l]
        q, s = inp["points"][l + 1 if key == "pools" else l], inp["points"][l]
        bad = np.zeros(idx.shape, bool)
        for scope in scopes:
            bad |= _closest_margin(q, s, idx, W[scope + "/kernel_points"], len(s))
        out[(key, l)] = bad
    return out


def build_inputs(cfg, W, seed, random_features=False):
    """-> (inputs, {(matrix, level): (replaced slots, valid slots)}).  random_features: N(0, 1) input features, not ones."""
    base = _pyramid(cfg.KP_extent, tuple(cfg.architecture))
    inp = dict(base)
    for key in ("neighbors", "pools"):
        inp[key] = [m.copy() for m in base[key]]
    n = len(inp["points"][0])
    if random_features or cfg.in_features_dim != 1:
        inp["features"] = np.random.default_rng(20000 + seed).standard_normal((n, cfg.in_features_dim)).astype(np.float32)
    replaced = {}
    if cfg.convolution_mode == "closest":
        for (key, l), bad in near_ties(cfg, W, inp).items():
            m = inp[key][l]
            replaced[(key, l)] = (int(bad.sum()), int((m < len(inp["points"][l])).sum()))
            m[bad] = len(inp["points"][l])
    return inp, replaced


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return build_inputs(config(case), weights(case), CASES[case][1], case in RANDOM_FEATURES)


def inputs(case):
    return _inputs(case)[0]


@functools.lru_cache(maxsize=None)
def reference(case, shifted=True):
    """-> (descriptors, scores, trace, report) of tests/network_f64_np.forward: computed once, shared, never written to."""
    import network_f64_np as f64
    return f64.forward(config(case), weights(case, shifted), inputs(case))


def oracle32_forward(cfg, W, inp):
    """The float32 CPU oracle on the same network -> (descriptors, scores, trace, [sum_c f > 0 of every KPConv's input, as :250
    computes it in float32])."""
    from oracle import network_np as onp
    signs, trace = [], {}
    orig = onp.KPConv_ops

    def rec(q, s, idx, features, *a, **k):
        signs.append((onp.torch.as_tensor(features, dtype=onp.torch.float32).sum(-1) > 0).numpy())
        return orig(q, s, idx, features, *a, **k)
    onp.KPConv_ops = rec
    try:
        d, s = onp.forward(cfg, W, inp, trace=trace)
    finally:
        onp.KPConv_ops = orig
    return d, s, {k: v.numpy() for k, v in trace.items()}, signs


@functools.lru_cache(maxsize=None)
def oracle32(case):
    return oracle32_forward(config(case), weights(case), inputs(case))


def deviation(got_d, got_s, got_trace, ref, bound=None):
    """The figure every comparison of these modules uses: max over the block outputs present in got_trace of max |diff| / max(1, max
    |want|), and the absolute max |diff| of descriptors and scores.  -> (figure, {what: figure}); bound: assert each one against it."""
    want_d, want_s, want_trace, _ = ref
    figs = {}
    for scope, want in want_trace.items():
        if scope in got_trace:
            have = np.asarray(got_trace[scope], np.float64)
            assert have.shape == want.shape, (scope, have.shape, want.shape)
            figs[scope] = float(np.abs(have - want).max() / max(1.0, np.abs(want).max()))
    for what, have, want in (("descriptors", got_d, want_d), ("scores", got_s, want_s)):
        have = np.asarray(have, np.float64)
        assert have.shape == want.shape, (what, have.shape, want.shape)
        figs[what] = float(np.abs(have - want).max())
    if bound is not None:
        over = {k: v for k, v in figs.items() if not v <= bound}
        assert not over, (bound, over)
    return max(figs.values()), figs


def condition_figures(cfg, W, inp, replaced, ref, signs32):
    """-> dict of the figures conditions 1-3 are about (see check_conditions)."""
    report = ref[3]
    left = 0
    if cfg.convolution_mode == "closest":
        left = sum(int(b.sum()) for b in near_ties(cfg, W, inp).values())
    return dict(replaced=replaced, ties_left=left, margins=[r["margin"] for r in report], shares=[r["share"] for r in report],
                sign_flips=[int((r["positive"] != s).sum()) for r, s in zip(report, signs32)], kpconvs=len(report), signs=len(signs32))


def conditions_hold(fig):
    ok1 = fig["ties_left"] == 0 and all(r <= MAX_REPLACED * v for r, v in fig["replaced"].values())
    ok2 = min(fig["margins"]) >= MARGIN and fig["kpconvs"] == fig["signs"] and not any(fig["sign_flips"])
    ok3 = sum(1 for s in fig["shares"] if 0.05 <= s <= 0.95) >= 3
    return ok1, ok2, ok3


def check_conditions(case):
    """Assert conditions 1-3 of the module docstring on what inputs() / weights() / reference() return -> the figures."""
    fig = condition_figures(config(case), weights(case), inputs(case), _inputs(case)[1], reference(case), oracle32(case)[3])
    ok1, ok2, ok3 = conditions_hold(fig)
    assert ok1, ("near ties of 'closest'", case, fig["replaced"], fig["ties_left"])
    assert ok2, ("row sums undecided", case, fig["margins"], fig["sign_flips"])
    assert ok3, ("row-sum signs not mixed", case, fig["shares"])
    return fig


# ---- the engine's inputs ---------------------------------------------------------------------------------------------------------------
# FragmentEngine builds its own pyramid from the raw cloud, so no slot of it can be replaced.  Its reference is the float64 definition on
# the UNEDITED oracle pyramid (which the device pyramid equals bit for bit: tests/test_gpu_network.py::test_pyramid_vs_oracle), and
# condition 1 becomes a condition on the case's kernel points: no valid slot's two smallest squared distances are closer than
# ENGINE_MARGIN = 2^-18 (3.8e-6) relative.  That is what float32 can decide: s - q is at most half an ulp of the search radius off
# (coordinates below 1, |s - q| <= 2.5 dl 2^level), so is (s - q) - kp, and a slot near a tie is at least a third of the kernel-point
# spacing (>= extent / 3) from both points: 2 * 2^-25 * 2.5 / (1 / 3) = 4.5e-7 relative per distance plus 3 * 2^-24 for the three
# fused multiply-adds, under 1.3e-6 for the difference of two -- a third of the margin.  The weight seeds of the two engine cases are
# chosen so that it holds.

def closest_gap(cfg, W, inp):
    """min over the valid slots of every matrix a KPConv reads of (d2[1] - d2[0]) / d2[1], the two smallest squared distances to the
    kernel points of that KPConv, in float64."""
    out = 1.0
    for (key, l), scopes in kpconv_readers(cfg).items():
        idx = inp[key][l]
        q, s = inp["points"][l + 1 if key == "pools" else l].astype(np.float64), inp["points"][l].astype(np.float64)
        valid = (idx >= 0) & (idx < len(s))
        rel = s[np.where(valid, idx, 0)] - q[:, None, :]
        for scope in scopes:
            KP = W[scope + "/kernel_points"].astype(np.float64)
            d2 = np.sort(((rel[:, :, None, :] - KP[None, None]) ** 2).sum(-1), -1)
            out = min(out, float(((d2[..., 1] - d2[..., 0]) / d2[..., 1])[valid].min()))
    return out


@functools.lru_cache(maxsize=None)
def engine_inputs(case):
    cfg = config(case)
    assert case not in RANDOM_FEATURES
    return _pyramid(cfg.KP_extent, tuple(cfg.architecture))


@functools.lru_cache(maxsize=None)
def engine_reference(case):
    import network_f64_np as f64
    return f64.forward(config(case), weights(case), engine_inputs(case))


def check_engine_conditions(case):
    cfg, W, inp = config(case), weights(case), engine_inputs(case)
    gap = closest_gap(cfg, W, inp) if cfg.convolution_mode == "closest" else 1.0
    assert gap >= ENGINE_MARGIN, (case, gap)
    fig = condition_figures(cfg, W, inp, {}, engine_reference(case), oracle32_forward(cfg, W, inp)[3])
    assert conditions_hold(fig)[1], ("row sums undecided", case, fig["margins"], fig["sign_flips"])
    return dict(fig, gap=gap)


# ---- which kernels a run really takes -------------------------------------------------------------------------------------------------
SPIED = ("kpconv_fused_c1", "kpconv_fused32", "kpconv_fused", "kpconv_aggregate", "gemm_cat2", "gemm_upsample_split", "gemm_upsample_cat",
         "ind_max_pool", "gemm")
KPCONV_ROUTES = SPIED[:4]


@contextlib.contextmanager
def spy_ops(calls, stubs=None):
    """Wrap the entry points of d3feat_amd.ops that the network's Python chooses between: every call appends its name to `calls` (a
    gemm with a residual operand as "gemm+residual").  stubs {name: callable}: run these in place of the kernels (host runs)."""
    from d3feat_amd import ops
    orig = {n: getattr(ops, n) for n in SPIED}

    def wrap(name):
        fn = (stubs or orig)[name]

        def run(*a, **k):
            res = name == "gemm" and (k.get("residual") is not None or (len(a) > 5 and a[5] is not None))
            calls.append(name + ("+residual" if res else ""))
            return fn(*a, **k)
        return run
    for n in SPIED:
        setattr(ops, n, wrap(n))
    try:
        yield calls
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)


def expected_block_forms(cfg):
    """-> (resnet blocks whose two unary branches run as ONE contraction (gemm_cat2), contractions with a residual operand): a block's
    conv3 takes its shortcut as a residual when the shortcut is the identity / the max pooling (same width), or when the shortcut is a
    contraction of its own -- without batch norm, or with a conv2 width that is no multiple of 4 (models/network_blocks._resnetb)."""
    cat2 = res = 0
    fdim, cin = cfg.first_features_dim, cfg.in_features_dim
    for block in cfg.architecture:
        if "upsample" in block:
            break
        if block == "simple":
            cin = fdim
            continue
        if cin != 2 * fdim and cfg.use_batch_norm and (fdim // 2) % 4 == 0:
            cat2 += 1
        else:
            res += 1
        cin = 2 * fdim
        if "strided" in block:
            fdim *= 2
    return cat2, res


def assert_routes(calls):
    """calls {case: [entry points taken]} over ALL cases: every KPConv route ran in at least two cases, the resnet blocks took the
    fused / residual forms expected_block_forms() names (the non-fused shortcut among them), both decoder forms ran."""
    assert set(calls) == set(CASES)
    for route in KPCONV_ROUTES:
        ran = [c for c in CASES if route in calls[c]]
        assert len(ran) >= 2, (route, ran)
    for c in CASES:
        cfg = config(c)
        kp = sum(calls[c].count(r) for r in KPCONV_ROUTES)
        assert kp == sum(len(v) for v in kpconv_readers(cfg).values()), (c, kp)
        assert (calls[c].count("gemm_cat2"), calls[c].count("gemm+residual")) == expected_block_forms(cfg), c
        assert calls[c].count("ind_max_pool") == cfg.num_layers - 1, c
        assert calls[c].count("gemm_upsample_split") + calls[c].count("gemm_upsample_cat") == cfg.num_layers - 1, c
    assert expected_block_forms(config("shipped")) == (5, 4) and expected_block_forms(config("w18")) == (3, 6)      # the non-fused
    assert expected_block_forms(config("no_bn")) == (0, 9)                                                          # shortcut, twice
    for form in ("gemm_upsample_split", "gemm_upsample_cat"):
        assert any(form in calls[c] for c in CASES), form
