#!/usr/bin/env python3
"""tests/golden/validation.npz: what the REFERENCE'S OWN PYTHON computes for the validation figures (build machine only).

utils/loss.py is imported UNMODIFIED from the reference tree with the numpy stand-in for TensorFlow (oracle/tf_eager) on the path.
The stand-in lacks two symbols loss.py needs and one method; they are added HERE, to the imported module object, never to oracle/:

    tf.greater_equal                x >= y
    tf.math.reduce_logsumexp        log(sum(exp(x - max))) + max, float32
    tf.logical_and                  wrapped so that its result accepts .set_shape (a no-op: loss.py:102,147)

The lines of models/KPFCNN_model.py that join them (:131-132 keypoint distances, :145-170 masks and the three LOSS_CHOICES calls,
:172-186 the skip rule) cannot be imported without building the whole graph; run_model() restates them line by line on the stand-in.

Per pair the fixture holds the inputs, the reference's float32 figures (circle = LOSS_CHOICES['circle_loss'], contrastive =
LOSS_CHOICES['desc_loss'], det, accuracy, d_pos, d_neg after the skip rule), and per figure the tolerance 4 x the largest difference
between the reference's float32 value and the float64 restatement (tests/validation_np.py) over the fixture's pairs -- the kernel's
fp32 error is of the kind and size of the reference's own, so two of them add and a factor 2 is spare.  Only arrays go into the
fixture (and the sha256 of loss.py); none of the reference's text does.

Accuracy is a count, so the generator refuses to write unless validation_np.margins holds on every evaluated pair: no row with
|fp - cn| inside 4 gamma Dmax (planted ties excepted), no keypoint distance inside 8 * 7 * 2^-24 r of the safe radius.  If that
fails, change a seed -- not the band.
"""
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tf_eager"))
import numpy as np

import validation_np as vnp

REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "validation.npz")
C, LD, SAFE_RADIUS, DET_WEIGHT = 32, 256, 0.1, 1.0
# (seed, n, keypts_num, cube edge, kind, descriptor noise: 0.3 leaves every row accurate, 1.6 about half of them)
PAIRS = ((11, 2, 4, 0.4, "", 0.3), (12, 3, 4, 0.4, "", 1.0), (13, 63, 64, 0.4, "", 1.6), (14, 64, 64, 0.4, "duplicates", 0.3),
         (15, 65, 128, 0.05, "all_masked", 0.6), (16, 255, 256, 0.4, "", 1.6), (17, 256, 256, 0.4, "", 0.3),
         (18, 100, 256, 0.4, "skipped", 0.3))
DUPLICATES = ((5, 40), (17, 18))            # rows (i, i'): entry i' of both lists is made a copy of entry i
FIGURES = ("circle", "contrastive", "det", "accuracy", "d_pos", "d_neg")


class _Mask(np.ndarray):
    def set_shape(self, shape):
        pass


def patch_stand_in():
    import tensorflow as tf
    tf.greater_equal = lambda x, y: np.asarray(x) >= y

    def reduce_logsumexp(x, axis=None, keepdims=False):
        x = np.asarray(x, np.float32)
        mx = np.max(x, axis=axis, keepdims=True)
        out = np.log(np.sum(np.exp(x - mx), axis=axis, keepdims=True, dtype=np.float32)) + mx
        return (out if keepdims else np.squeeze(out, axis=axis)).astype(np.float32)
    tf.math.reduce_logsumexp = reduce_logsumexp
    plain_and = tf.logical_and
    tf.logical_and = lambda x, y: np.asarray(plain_and(x, y)).view(_Mask)
    return tf


def load_loss():
    spec = importlib.util.spec_from_file_location("loss", os.path.join(REF, "utils", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_model(tf, loss, out_features, out_scores, backup_points, anc_inds, pos_inds, safe_radius, keypts_num, det_loss_weight):
    """models/KPFCNN_model.py:131-132, 145-186 on the stand-in; -> (circle, contrastive, det, accuracy, d_pos, d_neg) float32."""
    anc_keypts = tf.gather(backup_points, anc_inds)                                        # :131
    keypts_distance = loss.cdist(anc_keypts, anc_keypts, metric='euclidean')               # :132
    positiveIDS = tf.range(tf.size(anc_inds))                                              # :145
    positiveIDS = tf.reshape(positiveIDS, [tf.size(anc_inds)])                             # :146
    anc_features = tf.gather(out_features, anc_inds)                                       # :147
    pos_features = tf.gather(out_features, pos_inds)                                       # :148
    dists = loss.cdist(anc_features, pos_features, metric='euclidean')                     # :149
    same_identity_mask = tf.equal(tf.expand_dims(positiveIDS, axis=1), tf.expand_dims(positiveIDS, axis=0))       # :152
    distance_lessthan_threshold_mask = tf.less(keypts_distance, np.float32(safe_radius))   # :153
    false_negative_mask = tf.logical_and(distance_lessthan_threshold_mask, tf.logical_not(same_identity_mask))    # :154
    circle, accuracy, d_pos, d_neg = loss.LOSS_CHOICES['circle_loss'](dists, positiveIDS, pos_margin=0.1, neg_margin=1.4,
                                                                      false_negative_mask=false_negative_mask)   # :157-161
    contrastive, acc2, _, _ = loss.LOSS_CHOICES['desc_loss'](dists, positiveIDS, pos_margin=0.1, neg_margin=1.4,
                                                             false_negative_mask=false_negative_mask)
    assert float(acc2) == float(accuracy)
    if det_loss_weight != 0:                                                               # :164-170
        anc_scores = tf.gather(out_scores, anc_inds)
        pos_scores = tf.gather(out_scores, pos_inds)
        det = loss.LOSS_CHOICES['det_loss'](dists, anc_scores, pos_scores, positiveIDS)
        det = tf.scalar_mul(np.float32(det_loss_weight), det)
    else:
        det = tf.constant(0, dtype=np.float32)
    enough = tf.constant(0.5 * keypts_num)                                                 # :173-174
    condition = tf.less_equal(enough, tf.cast(tf.size(anc_inds), tf.float32))
    keep = lambda: (circle, contrastive, det, accuracy, d_pos, d_neg)
    skip = lambda: tuple(tf.constant(v, dtype=np.float32) for v in (0, 0, 0, -1, 0, 0))    # :179-184
    return np.asarray([np.float32(v) for v in tf.cond(condition, keep, skip)], np.float32)  # :186


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s: the reference tree is needed" % REF)
    tf = patch_stand_in()
    loss = load_loss()
    feats, scores, points, row0 = [], [], [], [0]
    anc, pos = np.zeros((len(PAIRS), LD), np.int32), np.zeros((len(PAIRS), LD), np.int32)
    ns, kns, ref, f64 = [], [], [], []
    planted = np.full((len(PAIRS), len(DUPLICATES)), -1, np.int32)
    for k, (seed, n, kn, cube, kind, noise) in enumerate(PAIRS):
        f, s, x, ai, pi = vnp.make_case(seed, n, C, cube=cube, noise=noise)
        rows = ()
        if kind == "duplicates":
            for (i, j) in DUPLICATES:
                ai[j], pi[j] = ai[i], pi[i]
            rows = tuple(r for d in DUPLICATES for r in d)
            planted[k] = [j for (_, j) in DUPLICATES]
        r32 = run_model(tf, loss, f, s[:, None], x, ai, pi, SAFE_RADIUS, kn, DET_WEIGHT)
        want = vnp.figures(f, s, x, ai, pi, SAFE_RADIUS, kn, DET_WEIGHT)
        if not want["skipped"]:
            # (the duplicated rows sit on each other: their points coincide, which the keypoint-distance margin is not about)
            gap, rel = vnp.margins(f, x, ai, pi, SAFE_RADIUS, C, planted_rows=rows,
                                   planted_kd=DUPLICATES if kind == "duplicates" else ())
            assert int(round(float(r32[3]) * n)) == want["accurate"], (k, r32[3] * n, want["accurate"])
            if kind == "all_masked":
                assert want["masked"] == 1.0 and np.allclose(want["lse"], np.log(n))
            if kind == "duplicates":
                assert all(want["fp"][j] == want["cn"][j] for (_, j) in DUPLICATES)
            print("pair %d n=%3d %-10s masked %.3f  smallest |fp-cn| %.2e  KD margin %.2e  ref %s" % (
                k, n, kind, want["masked"], gap, rel, np.round(r32, 5).tolist()))
        else:
            assert kind == "skipped" and r32.tolist() == [0, 0, 0, -1, 0, 0]
        feats.append(f), scores.append(s), points.append(x), row0.append(row0[-1] + len(f))
        anc[k, :n], pos[k, :n] = ai, pi
        row = [want[name] for name in FIGURES]
        if not want["skipped"]:
            row[3] = float(np.float32(want["accurate"]) / np.float32(n))      # a count over n: the float32 quotient of the reference
        ns.append(n), kns.append(kn), ref.append(r32), f64.append(row)
    ref, f64 = np.asarray(ref, np.float32), np.asarray(f64, np.float64)
    tol = 4.0 * np.abs(ref.astype(np.float64) - f64).max(0)
    print("reference float32 against float64, largest difference per figure:", (tol / 4).tolist())
    assert tol[3] == 0.0                                        # accuracy is a count over n: the same float32 quotient
    sha = hashlib.sha256(open(os.path.join(REF, "utils", "loss.py"), "rb").read()).hexdigest()
    np.savez_compressed(OUT, features=np.concatenate(feats), scores=np.concatenate(scores), points=np.concatenate(points),
                        row0=np.asarray(row0, np.int32), anc_idx=anc, pos_idx=pos, n=np.asarray(ns, np.int32),
                        keypts_num=np.asarray(kns, np.int32), safe_radius=np.float32(SAFE_RADIUS), det_loss_weight=np.float32(DET_WEIGHT),
                        reference=ref, float64=f64, tolerance=tol, planted_rows=planted,
                        kinds=np.asarray([p[4] for p in PAIRS]), sha256_loss=np.array(sha))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
