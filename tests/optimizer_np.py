"""numpy restatements of d3f_momentum_sgd (include/d3feat_amd.h): the optimiser's step of every variable.

    g1 = g  |  fl(g + fl(wd v))  (decayed);   S = sum (double)g1^2;   n = (float)sqrt(S);   s = clip > 0 ? fl(clip / max(n, clip)) : 1
    g2 = fl(g1 s);   a' = fl(fl(mom a) + g2);   v' = fl(v - fl(lr a'));   R = sum over decayed of 0.5 (double)v^2;  reg = (float)(wd R)

step32: every rounding the device call makes, as float32 numpy array operations (numpy neither fuses nor reorders them).  The float64
sums S and R are taken in numpy's own order: where every square and partial sum is exact -- inputs that are multiples of 2^-6 with
|.| <= 4, up to 2^20 entries -- any order gives the same bits, and so does the device.  Elsewhere another order may move n by one
float32 ulp, which reaches the variables whose norm exceeds the clip only: `bounds`.
step64: the same formulas in float64 on the widened inputs and the widened float32 hyper-parameters.
Variables are dicts name -> array (any shape); G[name] None: the variable is skipped whole.  hyper = (lr, mom, clip, wd)."""
import numpy as np

U = 2.0 ** -24


def _step(V, G, A, hyper, decay, dt):
    wide = dt is np.float64
    lr, mom, clip, wd = (dt(np.float32(h)) for h in hyper)
    V2, A2, info, R = {}, {}, {}, 0.0
    with np.errstate(all="ignore"):
        for k, v in V.items():
            g, a = G.get(k), A[k]
            if g is None:
                V2[k], A2[k] = v.copy(), a.copy()
                continue
            v, g, a = v.astype(dt), g.astype(dt), a.astype(dt)
            g1 = g + wd * v if decay.get(k) else g
            S = np.sum(g1.astype(np.float64) * g1.astype(np.float64))
            n = np.sqrt(S) if wide else np.float32(np.sqrt(S))
            s = dt(clip / np.maximum(n, clip)) if clip > 0 else dt(1)
            g2 = g1 * s
            a2 = mom * a + g2
            step = lr * a2
            V2[k], A2[k] = v - step, a2
            if decay.get(k):
                R += float(np.sum(0.5 * v.astype(np.float64) * v.astype(np.float64)))
            info[k] = dict(g1=g1, g2=g2, n=n, s=s, step=step, clipped=bool(clip > 0 and not n <= clip), mom_a=mom * a)
            assert V2[k].dtype == dt and a2.dtype == dt
    reg = np.float64(wd) * R
    return V2, A2, (reg if wide else np.float32(reg)), info


def step32(V, G, A, hyper, decay=()):
    """-> (V', A', regularization loss f32, info): info[name] = g1, g2, n, s, step = fl(lr a'), clipped, mom_a of the live variables."""
    return _step(V, G, A, hyper, dict.fromkeys(decay, True) if not isinstance(decay, dict) else decay, np.float32)


def step64(V, G, A, hyper, decay=()):
    return _step(V, G, A, hyper, dict.fromkeys(decay, True) if not isinstance(decay, dict) else decay, np.float64)


def zeros_like(V):
    return {k: np.zeros_like(v) for k, v in V.items()}


def run32(V, steps, decay=()):
    """steps: [(G, hyper), ...] with the accumulators carried from zeros -> [(V', A', reg, info), ...]."""
    A, out = zeros_like(V), []
    for G, hyper in steps:
        V, A, reg, info = step32(V, G, A, hyper, decay)
        out.append((V, A, reg, info))
    return out


def bounds(case, hyper):
    """How far a' and v' of ONE step may lie from step32's when S was added in another order (inputs equal): n moves by at most one
    float32 ulp, 2u relative, and s and g2 = fl(g1 s) follow with a rounding each.  case: step32's result.
    -> {name: (|da| <= 8u (|g2| + |a'|),  |dv| <= lr |da| + 2u (|lr a'| + |v'|))}, arrays."""
    V2, A2, _, info = case
    lr = float(np.float32(hyper[0]))
    out = {}
    for k, i in info.items():
        ba = 8 * U * (np.abs(i["g2"]).astype(np.float64) + np.abs(A2[k]))
        out[k] = (ba, lr * ba + 2 * U * (np.abs(i["step"]).astype(np.float64) + np.abs(V2[k])))
    return out


def bounds64(case, V, hyper, decay=(), ea=None, ev=None):
    """First-order bound of step32 against step64 on the same inputs, with incoming deviations ea (accumulators) and ev (variables) of
    earlier steps carried: one term u |x| per float32 rounding x = wd v, g1, g2, mom a, a', lr a', v'; n carries its own rounding and
    the 2-norm of the deviations of g1 (Cauchy-Schwarz), s one more rounding where a norm exceeds the clip:
        e_g1 = u (|wd v| + |g1|) + wd ev;   dn = u n + |e_g1|_2;   ds = s (dn / max(n, clip) + u)  (clipped)  |  0
        e_g2 = s e_g1 + |g1| ds + u |g2|;   ea' = mom ea + u |mom a| + e_g2 + u |a'|;   ev' = ev + lr ea' + u (|lr a'| + |v'|)
    times 1 + 2^-10 for the second-order terms.  -> ({name: ea'}, {name: ev'})."""
    V2, A2, _, info = case
    lr, mom, clip, wd = (float(np.float32(h)) for h in hyper)
    ea = ea or {}
    ev = ev or {}
    oa, ov = {}, {}
    for k in V2:
        a0, v0 = ea.get(k, 0.0), ev.get(k, 0.0)
        if k not in info:
            oa[k], ov[k] = a0, v0
            continue
        i = info[k]
        g1, g2 = np.abs(i["g1"]).astype(np.float64), np.abs(i["g2"]).astype(np.float64)
        e1 = (U * (np.abs(wd * V[k].astype(np.float64)) + g1) + wd * v0) if k in decay else np.zeros_like(g1)
        n, s = float(i["n"]), float(i["s"])
        ds = s * ((U * n + np.sqrt(np.sum(e1 * e1))) / max(n, clip, 1e-300) + U) if (clip > 0 and n * (1 + 4 * U) > clip) else 0.0
        e2 = s * e1 + g1 * ds + U * g2
        oa[k] = (mom * a0 + U * np.abs(i["mom_a"]) + e2 + U * np.abs(A2[k])) * (1 + 2.0 ** -10)
        ov[k] = (v0 + lr * oa[k] + U * (np.abs(i["step"]).astype(np.float64) + np.abs(V2[k]))) * (1 + 2.0 ** -10)
    return oa, ov


def quantised(rng, shape, scale=4.0):
    """Multiples of 2^-6 in [-scale, scale]: every square (a multiple of 2^-12 below 2^4) and every sum of up to 2^20 of them (below
    2^24, 36 bits) is exact in float64."""
    return (np.round(rng.uniform(-scale, scale, shape) * 64) / 64).astype(np.float32)
