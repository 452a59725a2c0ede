"""TEST INFRASTRUCTURE ONLY.  Float64 restatement of the backward of the descriptor / detection head (d3feat_amd.ops.
detect_head_backward, d3f_detect_head_backward of include/d3feat_amd.h): from the gradients with respect to the rows of desc and score
to the gradient with respect to the un-normalised features x -- the oracle of tests/test_head_grad_host.py and
tests/test_gpu_head_backward.py -- with the transposed neighbour table (transpose_np), the margins a test input must keep (the
gradient is discontinuous where the argmax of a row's score channels, of a row's y or of a cloud's entries changes, and at the
descriptor clamp) and first-order tolerances derived from a case.

torch_head() is the second statement of the same thing: models/D3Feat.py:65-115 of the reference written line by line in torch for B
clouds with pad counts, differentiated by autograd (torch_gradients) -- in float64 it pins gradients() (host test), in float32 on the
CPU it is the yardstick "float32 run the plain way" of the device's error (err32 of tests/golden/head_grad.npz).
"""
import numpy as np

from oracle import head_cases

U = 2.0 ** -24
BAR = 1e-4          # the project's bar: no tolerance exceeds this fraction of an evaluation's largest entry
REL_GAP = 1e-3      # clean_case: a maximum and its runner-up differ by this relative gap, or are bit-equal


def pad_counts(lens, group=0):
    """datasets/common.py:453-496: shadow slots of every cloud's row of in_batches -- longest - len, plus 1 when all clouds of the
    stack (of every `group` consecutive clouds) are equally long."""
    lens = [int(l) for l in lens]
    g = group if group > 0 else max(len(lens), 1)
    out = []
    for g0 in range(0, len(lens), g):
        part = lens[g0:g0 + g]
        longest = max(part)
        eq = 1 if all(l == longest for l in part) else 0
        out += [longest - l + eq for l in part]
    return out


def forward_parts(x, nb, lens, group=0, pads=None):
    """The forward's quantities in float64 (the names of include/d3feat_amd.h)."""
    lens = [int(l) for l in lens]
    n = sum(lens)
    x = np.asarray(x, np.float64)[:n]
    C = x.shape[1]
    pads = pad_counts(lens, group) if pads is None else [int(p) for p in pads]
    m, cloud = np.zeros(len(lens)), np.zeros(n, np.int64)
    a = 0
    for b, (l, p) in enumerate(zip(lens, pads)):
        if l:
            m[b] = x[a:a + l].max()
            if p > 0:
                m[b] = max(m[b], 0.0)
            cloud[a:a + l] = b
        a += l
    den = (m + 1e-6)[cloud][:, None] if n else np.zeros((0, 1))
    y = x / den
    nbv = np.asarray(nb, np.int64)[:n]
    nbv = np.where((nbv < 0) | (nbv >= n), n, nbv)
    nf = np.concatenate([y, np.zeros((1, C))], 0)[nbv]
    num = np.maximum((nf.sum(-1) != 0).sum(-1), 1).astype(np.float64)
    S = nf.sum(1)
    d = y - S / num[:, None]
    alpha = np.logaddexp(0.0, d)
    w = y.max(1)
    w1 = (1e-6 + w)[:, None]
    beta = y / w1
    av = alpha * beta
    s = av.max(1)
    return dict(n=n, C=C, K=nbv.shape[1], x=x, lens=lens, pads=pads, m=m, cloud=cloud, den=den, y=y, nbv=nbv, num=num, S=S, d=d,
                alpha=alpha, w=w, w1=w1, beta=beta, a=av, s=s, absS=np.abs(nf).sum(1))


def gradients(x, nb, lens, gdesc=None, gscore=None, group=0, pads=None, parts=None):
    """-> dict(gx f64[n, C], and what the tests and tolerances() need: T, W (the tie sets), cloud_ties (the tie count of every cloud),
    ss, clamp (rows under the descriptor clamp), the intermediate gradients)."""
    P = parts if parts is not None else forward_parts(x, nb, lens, group, pads)
    n, C, xx, y, den = P["n"], P["C"], P["x"], P["y"], P["den"]
    gsc = np.zeros(n) if gscore is None else np.asarray(gscore, np.float64).reshape(-1)[:n]
    T = P["a"] == P["s"][:, None]
    ga = gsc[:, None] * T / np.maximum(T.sum(1, keepdims=True), 1)                     # 1
    sig = np.exp(-np.logaddexp(0.0, -P["d"]))                                          # sigmoid(d), no overflow
    g_d = ga * P["beta"] * sig                                                         # 2
    g_beta = ga * P["alpha"]
    W = y == P["w"][:, None]
    gw = -(g_beta * y).sum(1, keepdims=True) / P["w1"] ** 2                            # 3
    own = g_d + g_beta / P["w1"] + W * (gw / np.maximum(W.sum(1, keepdims=True), 1))
    gS = -g_d / P["num"][:, None]                                                      # 4
    sc = np.zeros((n + 1, C))
    absc = np.zeros((n + 1, C))
    if P["K"]:
        np.add.at(sc, P["nbv"].reshape(-1), np.repeat(gS, P["K"], 0))
        np.add.at(absc, P["nbv"].reshape(-1), np.repeat(np.abs(gS), P["K"], 0))
    gy = own + sc[:n]
    gx = gy / den                                                                      # 5
    cloud_ties = np.zeros(len(P["lens"]), np.int64)
    shares = np.zeros(len(P["lens"]))
    a = 0
    for b, (l, p) in enumerate(zip(P["lens"], P["pads"])):                             # 6
        if l:
            r = slice(a, a + l)
            gden = -(gy[r] * y[r]).sum() / (P["m"][b] + 1e-6)
            tie = xx[r] == P["m"][b]
            cnt = int(tie.sum()) + (p * C if (p > 0 and P["m"][b] == 0) else 0)
            cloud_ties[b] = cnt
            if cnt:
                shares[b] = gden / cnt
                gx[r] += tie * shares[b]
        a += l
    ss = (xx * xx).sum(1)
    clamp = ss < 1e-10
    if gdesc is not None:                                                              # 7
        g = np.asarray(gdesc, np.float64)[:n]
        inv = 1.0 / np.sqrt(np.maximum(ss, 1e-10))[:, None]
        desc = xx * inv
        gx += np.where(clamp[:, None], g * inv, inv * (g - desc * (desc * g).sum(1, keepdims=True)))
    return dict(gx=gx, T=T, W=W, cloud_ties=cloud_ties, shares=shares, ss=ss, clamp=clamp, g_d=g_d, g_beta=g_beta, gw=gw, own=own,
                gS=gS, gy=gy, scatter_abs=absc[:n], sig=sig, parts=P)


def transpose_np(nb, n, N=None):
    """The transposed neighbour table of include/d3feat_amd.h (d3f_neighbor_transpose) -> (start i32[N + 1], edges i32[valid edges]):
    np.argsort(kind="stable") of the valid edges' keys -- the whole definition."""
    nb = np.asarray(nb, np.int64)[:n]
    N = n if N is None else int(N)
    keys = nb.reshape(-1)
    e = np.arange(keys.size, dtype=np.int64)
    valid = (keys >= 0) & (keys < n)
    kv, ev = keys[valid], e[valid]
    order = np.argsort(kv, kind="stable")
    start = np.searchsorted(kv[order], np.minimum(np.arange(N + 1), n), side="left")
    return start.astype(np.int32), ev[order].astype(np.int32)


def _runner_up_gap(v):
    """rows of v: (largest - the largest value strictly below it) / max(|both|); inf where the row holds one distinct value"""
    v = np.asarray(v, np.float64)
    if v.ndim == 1:
        v = v[None]
    out = np.full(v.shape[0], np.inf)
    if v.shape[1] == 0:
        return out
    best = v.max(1)
    below = np.where(v < best[:, None], v, -np.inf).max(1)
    ok = np.isfinite(below)
    scale = np.maximum(np.abs(best), np.abs(below))
    out[ok] = (best[ok] - below[ok]) / np.maximum(scale[ok], 1e-300)
    return out


def margins(x, nb, lens, group=0, pads=None, parts=None):
    """Asserts what makes the gradient of a test input the same function in fp32 and float64: per row the best and the second-best
    DISTINCT a[i, :], the two largest distinct y[i, :], per cloud the two largest distinct entries (the zero of a padded cloud among
    them) differ by REL_GAP relative -- bit-equal entries are one value: planted ties stay --, and ss is a factor 2 away from 1e-10.
    -> dict(a, y, cloud, ss): the smallest of each."""
    P = parts if parts is not None else forward_parts(x, nb, lens, group, pads)
    ga, gyy = _runner_up_gap(P["a"]), _runner_up_gap(P["y"])
    gc = []
    a = 0
    for l, p in zip(P["lens"], P["pads"]):
        if l:
            v = P["x"][a:a + l].reshape(-1)
            gc.append(_runner_up_gap(np.concatenate([v, [0.0]]) if p > 0 else v)[0])
        a += l
    gc = np.asarray(gc if gc else [np.inf])
    ss = (P["x"] * P["x"]).sum(1)
    ssr = np.where(ss > 0, np.maximum(ss / 1e-10, 1e-10 / np.maximum(ss, 1e-300)), np.inf) if len(ss) else np.asarray([np.inf])
    assert not (ga < REL_GAP).any(), "a row's two best distinct score channels are %.3e apart (relative): change the seed" % ga.min()
    assert not (gyy < REL_GAP).any(), "a row's two largest distinct y are %.3e apart (relative): change the seed" % gyy.min()
    assert not (gc < REL_GAP).any(), "a cloud's two largest distinct entries are %.3e apart (relative): change the seed" % gc.min()
    assert not (ssr < 2).any(), "a row's squared norm is within a factor %.3f of the clamp 1e-10: change the seed" % ssr.min()
    return dict(a=float(ga.min()) if len(ga) else np.inf, y=float(gyy.min()) if len(gyy) else np.inf, cloud=float(gc.min()),
                ss=float(ssr.min()))


def clean_case(seed, C, K, lens, group=0, pads=None, dup=None, plant=(), tries=64, **kw):
    """oracle.head_cases.head_case with the first seed from `seed` on (steps of 1000) that keeps margins(): "change the seed, not the
    gap".  dup = (src, dst): column src of x is copied onto column dst AFTER the draw -- every lane then does the same arithmetic on
    both, so the ties of T, W and of the cloud maximum survive in fp32; plant = ((row, column, value), ...) is written after that (exact
    zeros in an all-non-positive cloud).  -> (x, nb), the margins, the seed used."""
    for k in range(tries):
        sd = seed + 1000 * k
        x, nb = head_cases.head_case(sd, C, K, lens, **kw)
        if dup is not None:
            x[:, dup[1]] = x[:, dup[0]]
        for r, c, v in plant:
            x[r, c] = v
        try:
            return (x, nb), margins(x, nb, lens, group, pads), sd
        except AssertionError:
            continue
    raise AssertionError("no clean seed found from %d on in %d tries" % (seed, tries))


def tolerances(res, K):
    """Absolute first-order bounds of the fp32 evaluation of d3f_detect_head_backward against float64, per entry, derived from the
    case (res = gradients(...)) -- worst case, in the manner of loss_grad_np.tolerances.  u = 2^-24.
      y = x / den: 2u.  S: a chain of K additions of rounded quotients, (K + 4) u sum_k |y_nbr|; so d carries the ABSOLUTE error
        dd_i = 2u max_c |y| + (K + 4) u max_c sum_k |y_nbr| / num_i.
      alpha = softplus(d): d alpha = sigmoid(d) dd, relative sigmoid / alpha;  sigmoid: relative (1 - sigmoid) dd.  Both matter on the
        channels of T_i only (ga is zero elsewhere).  beta, the quotients by (1e-6 + w) and |T|, the products: a few u each; the
        channel sum of gw: C u.  Together rel_i = (C + 16) u + max_{c in T_i} (sigmoid / alpha + 1 - sigmoid) dd_i, applied to the
        sum of the ABSOLUTE values of the terms of gy's own part (g_d, g_beta / (1e-6 + w) and gw / |W| cancel almost entirely
        when T_i = W_i: the bound does not rely on it) and to gS.
      the segment chain of row j: the terms' own errors plus (in-degree + 2) u times the sum of their absolute values.
      gx = gy / den: 3u.  The cloud term: the float64 tree adds nothing visible; the errors of gy enter times |y| / den_b / ties,
        the rounding of gy y to the product 3u, the share rounded to fp32 2u.
      descriptor: rsqrt(ss) with ss a C-term sum, the dot product another: (C + 16) u of inv (|gdesc| + |desc| sum_c |desc gdesc|);
        a clamp row 4u |gdesc| rsqrt(1e-10).
    -> dict(score f64[n, C]: the bound of the score path per entry, rel f64[n, 1]: rel_i); desc_tolerances() is the descriptor's
    part.  The caller adds the two, takes the maximum over the entries it compares, and caps it with cap()."""
    P = res["parts"]
    n, C, y, den = P["n"], P["C"], P["y"], P["den"]
    dd = 2 * U * np.abs(y).max(1) + (K + 4) * U * P["absS"].max(1) / P["num"] if n else np.zeros(0)
    sens = np.where(res["T"], res["sig"] / np.maximum(P["alpha"], 1e-300) + 1 - res["sig"], 0.0).max(1) if n else np.zeros(0)
    rel = ((C + 16) * U + sens * dd)[:, None]
    own_abs = np.abs(res["g_d"]) + np.abs(res["g_beta"] / P["w1"]) + res["W"] * np.abs(res["gw"]) / np.maximum(res["W"].sum(1, keepdims=True), 1)
    e_gS = rel * np.abs(res["gS"])
    sc_err = np.zeros((n + 1, C))
    indeg = np.zeros(n + 1)
    if K:
        np.add.at(sc_err, P["nbv"].reshape(-1), np.repeat(e_gS, K, 0))
        np.add.at(indeg, P["nbv"].reshape(-1), 1)
    e_gy = rel * own_abs + sc_err[:n] + ((indeg[:n] + 2) * U)[:, None] * res["scatter_abs"] + U * np.abs(res["gy"])
    e = e_gy / np.abs(den) + 3 * U * np.abs(res["gy"] / den)
    a = 0
    for b, l in enumerate(P["lens"]):
        if l and res["cloud_ties"][b]:
            r = slice(a, a + l)
            db = abs(P["m"][b] + 1e-6)
            e_sh = ((e_gy[r] * np.abs(y[r])).sum() + 3 * U * np.abs(res["gy"][r] * y[r]).sum()) / db / res["cloud_ties"][b] \
                + 2 * U * abs(res["shares"][b])
            e[r] += (P["x"][r] == P["m"][b]) * e_sh
        a += l
    return dict(score=e, rel=rel)


def desc_tolerances(x, gdesc):
    """the descriptor part of tolerances(): f64[n, C]"""
    x, g = np.asarray(x, np.float64), np.asarray(gdesc, np.float64)
    C = x.shape[1]
    ss = (x * x).sum(1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(ss, 1e-10))
    desc = x * inv
    e = (C + 16) * U * inv * (np.abs(g) + np.abs(desc) * np.abs(desc * g).sum(1, keepdims=True))
    return np.where(ss < 1e-10, 4 * U * np.abs(g) * inv, e)


def cap(bound, largest):
    return min(bound, BAR * largest)


# ---- the second statement: autograd of a torch restatement of models/D3Feat.py:65-115 ---------------------------------------------------
def torch_head(features, neighbor, lens, pads):
    """(backup_features, score) of torch tensors as models/D3Feat.py:65-115 computes them, for B clouds: cloud b's row of in_batches
    is its own rows followed by pads[b] shadow slots (datasets/common.py:453-496).  reduce_max is amax (the equal split among ties;
    Tensor.max(dim)[0] would send the gradient to one index)."""
    import torch
    lens = [int(l) for l in lens]
    n = sum(lens)
    dt, dev = features.dtype, features.device
    features = features[:n]
    backup_features = features * torch.rsqrt(torch.clamp_min((features * features).sum(1, keepdim=True), 1e-10))   # :65
    neighbor = neighbor[:n].long()
    neighbor = torch.where((neighbor < 0) | (neighbor >= n), torch.full_like(neighbor, n), neighbor)
    shadow_features = torch.zeros_like(features[:1, :])                                                          # :77
    features = torch.cat([features, shadow_features], 0)                                                         # :78
    shadow_neighbor = torch.ones_like(neighbor[:1, :]) * n                                                       # :79
    neighbor = torch.cat([neighbor, shadow_neighbor], 0)                                                         # :80
    rows, a = [], 0
    last = torch.ones((), dtype=dt, device=dev)
    for l, p in zip(lens, pads):
        if l:
            indices = torch.cat([torch.arange(a, a + l, device=dev), torch.full((int(p),), n, dtype=torch.long, device=dev)])            # in_batches[b]
            last = features[indices].amax()                                                                       # :84-85
            rows.append(torch.ones((l, 1), dtype=dt, device=dev) * last)                                                     # :87
        a += l
    rows.append(torch.ones((1, 1), dtype=dt, device=dev) * last)                                                             # :88 (the shadow row)
    max_per_sample = torch.cat(rows, 0)                                                                           # :86-89
    features = features / (max_per_sample + 1e-6)                                                                 # :90
    neighbor_features = features[neighbor]                                                                        # :93
    neighbor_features_sum = neighbor_features.sum(-1)                                                             # :94
    neighbor_num = torch.count_nonzero(neighbor_features_sum, dim=-1).reshape(-1, 1)                              # :95
    neighbor_num = torch.clamp_min(neighbor_num, 1)                                                               # :96
    mean_features = neighbor_features.sum(1) / neighbor_num.to(dt)                                                # :97
    d = features - mean_features
    local_max_score = torch.logaddexp(d, torch.zeros_like(d))                                                     # :98 (tf softplus)
    depth_wise_max = features.amax(1, keepdim=True)                                                               # :101
    depth_wise_max_score = features / (1e-6 + depth_wise_max)                                                     # :102
    all_score = local_max_score * depth_wise_max_score                                                            # :104
    score = all_score.amax(1, keepdim=True)                                                                       # :106
    return backup_features, score[:-1, :]                                                                         # :115


def torch_gradients(x, nb, lens, gdesc=None, gscore=None, group=0, pads=None, dtype="float64"):
    """autograd of torch_head on the CPU in `dtype`, seeded with (gdesc, gscore) -> gx [n, C] as float64 numpy."""
    import torch
    dt = getattr(torch, dtype)
    lens = [int(l) for l in lens]
    n = sum(lens)
    pads = pad_counts(lens, group) if pads is None else [int(p) for p in pads]
    xt = torch.tensor(np.asarray(x)[:n], dtype=dt, requires_grad=True)
    desc, score = torch_head(xt, torch.tensor(np.asarray(nb, np.int64)[:n]), lens, pads)
    val = torch.zeros((), dtype=dt)
    if gdesc is not None:
        val = val + (desc * torch.tensor(np.asarray(gdesc)[:n], dtype=dt)).sum()
    if gscore is not None:
        val = val + (score.reshape(-1) * torch.tensor(np.asarray(gscore).reshape(-1)[:n], dtype=dt)).sum()
    if not val.requires_grad:
        return np.zeros((n, xt.shape[1]))
    val.backward()
    return xt.grad.double().numpy()


# ---- the case grid shared by tools/make_golden_head_grad.py and the two test files ------------------------------------------------------
# name: (seed, C, K, lens, group, pads, dup, plant, head_case keywords).  At most about a hundred rows each (the 129- and 255-cloud
# stacks: some 300 to 600).
LENS_B255 = tuple(1 + i % 3 for i in range(254)) + (0,)                          # 255 clouds of 1 to 3 rows, the last empty: 507 rows
# 255 clouds of 0 to 3 rows, half of them empty, clouds 100 .. 104 -- one whole group of five -- among them
LENS_B255G5 = tuple(0 if (i % 3 == 0 or 100 <= i < 105) else (7 * i) % 4 for i in range(255))
LENS_B129 = tuple(1 + (5 * i) % 8 for i in range(129))                           # 129 clouds of 1 to 8 rows: 577 rows
GRID = {
    "c1": (11, 1, 17, (40, 30), 0, None, None, (), {}),
    "c20": (12, 20, 17, (40, 30), 0, None, None, (), {}),
    "c32": (13, 32, 17, (40, 30), 0, None, None, (), {}),
    "c33": (14, 33, 17, (40, 30), 0, None, None, (), {}),
    "c64": (15, 64, 17, (40, 30), 0, None, None, (), {}),
    "c100": (16, 100, 17, (30, 20), 0, None, None, (), {}),
    "c128": (17, 128, 17, (30, 20), 0, None, None, (), {}),
    "k0": (18, 32, 0, (30, 20), 0, None, None, (), {}),
    "k1": (19, 32, 1, (30, 20), 0, None, None, (), {}),
    "k33": (20, 32, 33, (30, 20), 0, None, None, (), {}),
    "k65": (21, 20, 65, (30, 20), 0, None, None, (), {}),
    "b1": (22, 32, 17, (50,), 0, None, None, (), {}),
    "b3g1": (23, 32, 17, (20, 25, 30), 1, None, None, (), {}),
    "b3empty": (24, 20, 17, (30, 0, 25), 0, None, None, (), {}),
    "b6g2": (25, 32, 17, (12, 20, 15, 15, 18, 9), 2, None, None, (), {}),
    "b6g3": (26, 33, 17, (12, 20, 15, 15, 18, 9), 3, None, None, (), {}),
    "eqlen": (27, 32, 17, (25, 25), 0, None, None, (), {}),
    "pads": (28, 32, 17, (30, 20), 0, (2, 0), None, (), {}),
    "dup": (29, 33, 17, (25, 25), 0, None, (3, 7), (), {}),
    "neg": (30, 32, 17, (30, 20), 0, None, None, (), dict(negative=(1,))),
    "negzero": (31, 20, 17, (30, 20), 0, None, None, ((33, 2, 0.0), (41, 7, 0.0)), dict(negative=(1,))),
    # explicit pad counts where the COUNT matters: the maximum of cloud 1 is the zero row, 3 C + 2 ties (derived: 10 C + 2; as a flag: C + 2)
    "negzero_pads": (31, 20, 17, (30, 20), 0, (0, 3), None, ((33, 2, 0.0), (41, 7, 0.0)), dict(negative=(1,))),
    # stacks of D3F_MAX_BATCH = 255 clouds (one thread per cloud in the maximum's first kernel, d3f_find_elem's steps of 128 / 64 / 32
    # from 129 / 65 / 33 clouds on); the clouds are kept this short: stacks of some 1100 rows find no clean seed in 64 tries
    "b255": (32, 20, 5, LENS_B255, 0, None, None, (), {}),
    "b255g5": (33, 32, 5, LENS_B255G5, 5, None, None, (), {}),
    "b129": (34, 20, 9, LENS_B129, 0, None, None, (), {}),
}
STORED = ("c1", "c20", "c32", "dup", "negzero", "b6g2")       # cases whose float64 gradients the fixture holds
EVALS = ("desc", "score", "both")                              # (gdesc, 0), (0, gscore), (gdesc, gscore)
NEGATIVE_ROWS = {"neg": slice(30, 50), "negzero": slice(30, 50), "negzero_pads": slice(30, 50)}   # the all-non-positive padded cloud: compared per entry, relatively
_grid = {}


def grid_case(name):
    """-> dict(x, nb, lens, group, pads, gd, gs, seed, margins, C, K): the case and its two seeds (float32), computed once."""
    if name not in _grid:
        seed, C, K, lens, group, pads, dup, plant, kw = GRID[name]
        (x, nb), mg, sd = clean_case(seed, C, K, lens, group, pads, dup, plant, **kw)
        rng = np.random.default_rng(seed + 7)
        n = sum(lens)
        _grid[name] = dict(x=x, nb=nb, lens=list(lens), group=group, pads=pads, gd=rng.normal(size=(n, C)).astype(np.float32),
                           gs=rng.normal(size=n).astype(np.float32), seed=sd, margins=mg, C=C, K=K, n=n)
    return _grid[name]


def seeds_of(case, ev):
    return (case["gd"] if ev in ("desc", "both") else None), (case["gs"] if ev in ("score", "both") else None)


def deviations(have, want, ev, clamp, neg=None):
    """How an evaluation is compared -> dict(main=(largest deviation, largest entry) over the rows compared absolutely, clamp=(...) over
    the clamp rows (ss < 1e-10) in EVERY evaluation -- in the descriptor path their entries are some 1e5 times the rest, and the same
    rows have w_i of about 1e-6, so they dominate the score path by as much: under one 'largest entry' bar they would hide every error
    of an ordinary row --, rel = the largest per-entry relative deviation over the rows `neg` (entries whose float64 value is zero
    must be zero))."""
    have, want = np.asarray(have, np.float64), np.asarray(want, np.float64)
    rows = np.ones(len(want), bool)
    if neg is not None:
        rows[neg] = False
    out = {}
    if clamp.any():
        c = clamp & rows
        out["clamp"] = (float(np.abs(have[c] - want[c]).max()), float(np.abs(want[c]).max()))
        rows = rows & ~clamp
    out["main"] = (float(np.abs(have[rows] - want[rows]).max()), float(np.abs(want[rows]).max())) if rows.any() else (0.0, 0.0)
    if neg is not None:
        h, w = have[neg], want[neg]
        nz = w != 0
        out["rel"] = float((np.abs(h - w)[nz] / np.abs(w[nz])).max()) if nz.any() else 0.0
        out["rel_zero_ok"] = bool((h[~nz] == 0).all())
    return out
