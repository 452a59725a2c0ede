"""The KITTI test metric of d3f_pose_errors in float64 numpy, in the operation and summation order include/d3feat_amd.h defines:
every operation below is one IEEE rounding (numpy never contracts), so rte, tr, c and the sums have the device's bits; arccos is
the C library's, which may differ from the device's by a few ulp."""
import numpy as np

RTE_MAX, RRE_MAX = 2.0, np.pi / 180 * 5


def rows(T, gt, per_pair=1):
    """T f32[P * per_pair, 12] (or [..., 3, 4]), gt f32[P, 12] -> dict of f64 arrays rte, tr, c, rre, rre_deg over the rows."""
    T = np.ascontiguousarray(T, np.float32).reshape(-1, 12).astype(np.float64)
    G = np.repeat(np.ascontiguousarray(gt, np.float32).reshape(-1, 12).astype(np.float64), per_pair, axis=0)
    assert T.shape == G.shape, (T.shape, G.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        d0, d1, d2 = T[:, 3] - G[:, 3], T[:, 7] - G[:, 7], T[:, 11] - G[:, 11]
        rte = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
        tr = T[:, 0] * G[:, 0]
        for k in (1, 2, 4, 5, 6, 8, 9, 10):
            tr = tr + T[:, k] * G[:, k]
        c = (tr - 1.0) / 2.0
        rre = np.arccos(c)
        rre_deg = (rre * 180.0) / np.pi
    return dict(rte=rte, tr=tr, c=c, rre=rre, rre_deg=rre_deg)


def flags(rte, rre, rte_max=RTE_MAX, rre_max=RRE_MAX):
    with np.errstate(invalid="ignore"):
        a = rte < rte_max
        b = ~np.isnan(rre) & (rre < rre_max)
    return a.astype(np.int32) | (b.astype(np.int32) << 1) | ((a & b).astype(np.int32) << 2)


def tree_sum(v, mask):
    """256 partial sums (partial t: rows t, t + 256, ... in ascending order; rows outside the mask skipped), then the halving tree."""
    v = np.where(mask, np.asarray(v, np.float64), 0.0)             # x + 0.0 has the bits of x: skipping and adding zero agree
    pad = (-len(v)) % 256
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, 256)
    part = np.zeros(256)
    for chunk in v:
        part = part + chunk
    s = 128
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def meters(rte, rre_deg, flg, per_pair=1):
    """The f64[per_pair, 8] sums of d3f_pose_errors from per-row values (the device's own, or rows()'s)."""
    rte, rre_deg, flg = (np.asarray(a).reshape(-1, per_pair) for a in (rte, rre_deg, flg))
    out = np.zeros((per_pair, 8))
    for c in range(per_pair):
        t, r, f = rte[:, c], rre_deg[:, c], flg[:, c]
        a, b, ok = (f & 1) != 0, (f & 2) != 0, (f & 4) != 0
        one = np.ones(len(f))
        with np.errstate(invalid="ignore", over="ignore"):
            out[c] = [tree_sum(t, a), tree_sum(t * t, a), tree_sum(one, a), tree_sum(r, b), tree_sum(r * r, b), tree_sum(one, b),
                      tree_sum(one, ok), float(len(f))]
    return out


def pose_errors(T, gt, per_pair=1, rte_max=RTE_MAX, rre_max=RRE_MAX):
    r = rows(T, gt, per_pair)
    r["flags"] = flags(r["rte"], r["rre"], rte_max, rre_max)
    r["meters"] = meters(r["rte"], r["rre_deg"], r["flags"], per_pair)
    return r


# ---- the log lines of ModelTester.test_kitti: text skeleton and figures ------------------------------------------------------------
import re

_NUM = re.compile(r"(?<![\w.'@])[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|nan|inf)(?![\w'@])")
_PERIODIC = ("count", "count", None, None, "count", "avg_rte", "avg_rre", "success", "count", "percent")     # None: a timer
_FINAL = ("count", "avg_rte", "var_rte", "avg_rre", "var_rre", "success", "count", "percent")


def split_line(line):
    """-> (the line with its id and every number cut out, [the numbers as floats], the id of a 'Failed with' line or None)"""
    m = re.match(r"b'([^']*)' ", line)
    ident = m.group(1) if m else None
    body = line[m.end():] if m else line
    return _NUM.sub("#", body), [float(x) for x in _NUM.findall(body)], ident


def figure_names(line):
    """What each number of a line is, in order (None: a timer, not compared)."""
    if "Failed with" in line:
        return ("printed_rte", "printed_rre_deg")
    return _FINAL if line.startswith("Total loss") else _PERIODIC


def check_against_golden(gold, rte, rre_deg, flags, sums):
    from d3feat_amd.utils import results
    """The assertions test_kitti_host.py and test_gpu_kitti.py share against tests/golden/kitti.npz: per-pair figures, flags, failed ids, the lines (skeleton and figures)."""
    n = len(gold["T"])
    assert rte.shape == rre_deg.shape == flags.shape == (n,)
    assert np.array_equal(flags, gold["flags"])
    assert np.max(np.abs(rte - gold["rte"].astype(np.float64))) <= gold["tol_rte"]
    assert np.array_equal(np.isnan(rre_deg), np.isnan(gold["rre_deg"]))
    assert np.nanmax(np.abs(rre_deg - gold["rre_deg"].astype(np.float64))) <= gold["tol_rre_deg"]
    ids = [str(s) for s in gold["anc_ids"]]
    assert [ids[i] for i in range(n) if not flags[i] & 4] == [str(s) for s in gold["failed_ids"]]
    lines = results.kitti_lines(ids, rte, rre_deg, flags, final=results.kitti_meters_from_sums(sums))
    want = [str(l) for l in gold["lines"]]
    assert len(lines) == len(want)
    compared = set()
    for a, b in zip(want, lines):
        (ska, na, ida), (skb, nb, idb) = split_line(a), split_line(b)
        assert ska == skb and ida == idb and len(na) == len(nb), (a, b)
        for name, x, y in zip(figure_names(a), na, nb):
            if name is None:
                continue
            compared.add(name)
            if np.isnan(x) or np.isnan(y):
                assert np.isnan(x) and np.isnan(y), (a, b)
            elif name in ("count", "success"):
                assert x == y, (a, b)
            else:
                assert abs(x - y) <= gold["tol_" + name], (name, a, b)
    assert compared == {"count", "success", "percent", "printed_rte", "printed_rre_deg", "avg_rte", "avg_rre", "var_rte", "var_rre"}
    return lines
