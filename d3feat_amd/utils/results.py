"""Data formats on either side of the hot path: the KITTI velodyne reader the reference's test
generators use, and the per-fragment result files its testers write.  Pure numpy; no device work here.
"""
import os

import numpy as np


def read_kitti_bin(path):
    """One velodyne sweep: float32 records (x, y, z, reflectance) -> xyz f32[n,3]  (datasets/KITTI.py:131, 277-278)."""
    raw = np.fromfile(path, dtype=np.float32)
    if raw.size % 4 != 0:
        raise ValueError("%s: %d float32 values, not a multiple of 4" % (path, raw.size))
    return np.ascontiguousarray(raw.reshape(-1, 4)[:, :3])


def read_kitti_records(path):
    """One velodyne sweep as RAW bytes + record layout for ops.decode_xyz_records (16-byte records x, y, z, reflectance)."""
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 16 != 0:
        raise ValueError("%s: %d bytes, not a multiple of 16" % (path, raw.size))
    return raw, dict(n=raw.size // 16, stride=16, offsets=(0, 4, 8), dtype='f4', big_endian=False)


def select_first_cloud(points, features, scores, first_len):
    """The keypoint selection of utils/tester.py:208-213 / demo_registration.py:158-164 for a stacked self-pair: rows of the
    FIRST cloud (the reference indexes them through in_batches[0][:-1]), in ASCENDING score order as its np.argsort leaves
    them (ties in index order: numpy's default quicksort is not stable, the reference's order among exactly equal scores is
    therefore unspecified -- a stable sort is used here).  -> (keypts [n,3], features [n,C], scores [n,1])"""
    points, features, scores = (np.asarray(a) for a in (points, features, scores))
    n = int(first_len)
    if not 0 <= n <= scores.shape[0]:
        raise ValueError("first_len %d outside [0, %d]" % (n, scores.shape[0]))
    s = scores[:n].reshape(n, -1)
    order = np.argsort(s[:, 0], kind="stable")
    return points[:n][order].astype(np.float32), features[:n][order].astype(np.float32), s[order].astype(np.float32)


def save_3dmatch_results(root, anc_id, points, features, scores, first_len):
    """The three files utils/tester.py:215-229 writes per fragment under `root` (its <path>/<descriptors|keypoints|scores>/
    <scene>/ layout): anc_id is the generator's id string '<scene>/.../cloud_bin_<k>.ply'.  Returns the three paths."""
    if isinstance(anc_id, bytes):
        anc_id = anc_id.decode("utf-8")
    scene = anc_id.split("/")[0]
    num_frag = int(anc_id.split("_")[-1][:-4])
    kp, feat, sc = select_first_cloud(points, features, scores, first_len)
    out = []
    for sub, name, arr in (("descriptors", "cloud_bin_%d.D3Feat" % num_frag, feat), ("keypoints", "cloud_bin_%d" % num_frag, kp),
                           ("scores", "cloud_bin_%d" % num_frag, sc)):
        d = os.path.join(root, sub, scene)
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, name)
        np.save(p, arr)
        out.append(p + ".npy")
    return out


def save_3dmatch_keypoints(root, anc_id, kp_records):
    """The three files of utils/tester.py:215-229 for a fragment of which only the K highest-scoring rows were kept: kp_records
    f32[k, 3 + C + 1] rows [xyz | desc | score] in ascending score order (keypoints.topk_records / FragmentEngine.fetch(keypoints=True),
    brought to the host by the caller).  The files hold those k rows: for any num_keypts <= k the consumer's [-num_keypts:]
    (geometric_registration/evaluate.py:47-50) reads the same rows as from the full files save_3dmatch_results writes.
    Returns the three paths."""
    if isinstance(anc_id, bytes):
        anc_id = anc_id.decode("utf-8")
    r = np.asarray(kp_records, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] < 5:
        raise ValueError("save_3dmatch_keypoints: records of shape %s" % (r.shape,))
    scene = anc_id.split("/")[0]
    num_frag = int(anc_id.split("_")[-1][:-4])
    out = []
    for sub, name, arr in (("descriptors", "cloud_bin_%d.D3Feat" % num_frag, r[:, 3:-1]), ("keypoints", "cloud_bin_%d" % num_frag, r[:, :3]),
                           ("scores", "cloud_bin_%d" % num_frag, r[:, -1:])):
        d = os.path.join(root, sub, scene)
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, name)
        np.save(p, np.ascontiguousarray(arr))
        out.append(p + ".npy")
    return out


# ---- the files of geometric_registration/evaluate.py -------------------------------------------------------------------------
def read_gt_log(path):
    """A gt.log (blocks of `id1 \\t id2 \\t n` + four rows of a 4x4 matrix) -> {"id1_id2": f64[4,4]}  (geometric_registration/
    utils.py:20-35).  The blocks write_registration_log writes parse the same way."""
    with open(path) as f:
        content = f.readlines()
    result = {}
    for i in range(0, len(content) - 4, 5):
        head = content[i].replace("\n", "").split("\t")[0:3]
        trans = np.zeros([4, 4])
        for r in range(4):
            trans[r] = [float(x) for x in content[i + 1 + r].replace("\n", "").split("\t")[0:4]]
        result["%d_%d" % (int(head[0]), int(head[1]))] = trans
    return result


def write_registration_log(path, pairs, transformations):
    """Appends the .log blocks of evaluate.py:101-110: per pair (id1, id2) the header `id1 \\t id2 \\t  37` and the four rows of the
    INVERSE of the estimated transformation (source -> target as register_pairs / register_keypoints return it)."""
    with open(path, "a+") as f:
        for (id1, id2), T in zip(pairs, transformations):
            trans = np.linalg.inv(np.asarray(T, dtype=np.float64))
            f.write(f'{int(id1)}\t {int(id2)}\t  37\n')
            for r in range(4):
                f.write(f"{trans[r, 0]}\t {trans[r, 1]}\t {trans[r, 2]}\t {trans[r, 3]}\t \n")


def write_pair_results(directory, pairs, num_inliers, inlier_ratio, gt_flag):
    """The cloud_bin_<s>_cloud_bin_<t>.rt.txt files of evaluate.py:113-115, one per pair.  Returns the rows
    [num_inliers, inlier_ratio, gt_flag] as evaluate.py:203-204 reads them back (the ratio at the 8 decimals of the file)."""
    os.makedirs(directory, exist_ok=True)
    rows = []
    for (id1, id2), n, r, g in zip(pairs, num_inliers, inlier_ratio, gt_flag):
        s, t = "cloud_bin_%d" % int(id1), "cloud_bin_%d" % int(id2)
        line = f"{s}\t{t}\t{int(n)}\t{float(r):.8f}\t{int(g)}"
        with open(os.path.join(directory, f"{s}_{t}.rt.txt"), "w+") as f:
            f.write(line)
        nums = line.split("\t")[2:5]
        rows.append([int(nums[0]), float(nums[1]), int(nums[2])])
    return rows


def feature_matching_recall(rows, inlier_ratio=0.05):
    """Per-scene figures of evaluate.py:200-219 from rows [num_inliers, inlier_ratio, gt_flag]: -> dict(correct, gt, recall in
    percent, ave_num_inliers, ave_inlier_ratio) -- as there, the averages divide the sums over the ground-truth pairs by the
    number of pairs above the ratio."""
    result = np.array(rows, dtype=np.float64).reshape(-1, 3)
    gt_results = int(np.sum(result[:, 2] == 1))
    pred_results = int(np.sum(result[:, 1] > inlier_ratio))
    zeros = np.zeros(result.shape[0])
    div = lambda a: float(a / pred_results) if pred_results else 0.0
    return dict(correct=pred_results, gt=gt_results, recall=float(pred_results / gt_results) * 100 if gt_results else 0.0,
                ave_num_inliers=div(np.sum(np.where(result[:, 2] == 1, result[:, 0], zeros))),
                ave_inlier_ratio=div(np.sum(np.where(result[:, 2] == 1, result[:, 1], zeros))))


def matching_table(num_keypts, rows_per_count, inlier_ratio=0.05):
    """The per-scene lines of evaluate.py:211-216 for a sweep of keypoint counts (evaluate.py:46 edited by hand, one run per count):
    rows_per_count[c] = the rows [num_inliers, inlier_ratio, gt_flag] of count num_keypts[c] (registration.PairMatching.rows).
    -> (lines, {K: feature_matching_recall dict})."""
    ks, rows_per_count = [int(k) for k in num_keypts], list(rows_per_count)
    if len(ks) != len(rows_per_count):
        raise ValueError("matching_table: %d counts, %d row lists" % (len(ks), len(rows_per_count)))
    lines, table = [], {}
    for k, rows in zip(ks, rows_per_count):
        r = table[k] = feature_matching_recall(rows, inlier_ratio)
        lines += [f"num_keypts = {k}", f"Correct Match {r['correct']}, ground truth Match {r['gt']}", f"Recall {r['recall']}%",
                  f"Average Num Inliners: {r['ave_num_inliers']}", f"Average Num Inliner Ratio: {r['ave_inlier_ratio']}"]
    return lines, table


def eth_lines(scene_names, summary, c=0):
    """The lines geometric_registration_eth/evaluate_eth.py:158-177 prints, in its order and with its wording (its typos too): four per
    scene, the row of stars, the list of recalls and the four closing figures.  summary: registration.SceneMatching (or anything with
    its .scenes() / .overall()), one scene per name; c: the column of the keypoint count (the script has one, 250)."""
    scenes = summary.scenes()
    if len(scene_names) != len(scenes):
        raise ValueError("eth_lines: %d names, %d scenes" % (len(scene_names), len(scenes)))
    lines = []
    for per_count in scenes:
        r = per_count[c]
        lines += [f"Correct Match {r['correct']}, ground truth Match {r['gt']}", f"Recall {r['recall']}%",
                  f"Average Num Inliners: {r['ave_num_inliers']}", f"Average Num Inliner Ratio: {r['ave_inlier_ratio']}"]
    o = summary.overall(c)
    lines += ["*" * 40, str(o["recall_list"]), f"Avergae Matching Recall: {o['matching_recall']}%",
              f"All 8 scene, average recall: {o['average_recall']}%", f"All 8 scene, average num inliers: {o['average_inliers']}",
              f"All 8 scene, average num inliers ratio: {o['average_inliers_ratio']}"]
    return lines


# ---- the files and lines of geometric_registration/3dmatch/evaluate.m --------------------------------------------------------------
def _blocks(path, width):
    """The whitespace-separated numbers of a .log / .info file as fscanf reads them (mrLoadLog.m, mrLoadInfo.m): blocks of three
    integers and width * width floats -> [((id1, id2, n), f64[width, width])]; a trailing partial block is an error."""
    with open(path) as f:
        tok = f.read().split()
    per = 3 + width * width
    if len(tok) % per:
        raise ValueError("%s: %d numbers, not a multiple of %d" % (path, len(tok), per))
    out = []
    for i in range(0, len(tok), per):
        head = tuple(int(t) for t in tok[i:i + 3])
        out.append((head, np.array([float(t) for t in tok[i + 3:i + per]], np.float64).reshape(width, width)))
    return out


def read_gt_info(path):
    """A gt.info (blocks of `id1 \\t id2 \\t n` + six rows of a 6x6 information matrix, mrLoadInfo.m) -> {"id1_id2": f64[6,6]}, the
    keys of read_gt_log.  Two entries for one pair are an error: mrEvaluateRegistration.m:9-14 would keep the last and count both, the
    benchmark's files hold none."""
    result = {}
    for (id1, id2, _), mat in _blocks(path, 6):
        key = "%d_%d" % (id1, id2)
        if key in result:
            raise ValueError("%s: two entries for the pair %s" % (path, key))
        result[key] = mat
    return result


def read_result_log(path):
    """A .log of results as write_registration_log / evaluate.py:101-110 write it (mrLoadLog.m) -> the ordered list
    [(id1, id2, f64[4,4])]; a pair that appears twice appears twice here, and counts twice, as in mrEvaluateRegistration.m:21-37."""
    return [(id1, id2, mat) for (id1, id2, _), mat in _blocks(path, 4)]


def _num2str(x):
    """MATLAB's num2str of a scalar in [0, 1]: '%d' for an integer, otherwise sprintf('%.5g') (max(floor(log10(x)) + 5, 5) significant
    digits), which drops trailing zeros."""
    return "%d" % x if float(x) == int(x) else "%.5g" % x


def registration_recall_lines(scene_names, summary, c=0):
    """The lines geometric_registration/3dmatch/evaluate.m prints for count c, with the .m files' own wording: per scene
    `recall : R ( good / gt_num )` (mrEvaluateRegistration.m:40, MATLAB's disp of num2str = %.5g with trailing zeros dropped), then
    evaluate.m:47-48 (`%f`, `%d`).  The `totalRecall` column MATLAB echoes in between is its console format, not reproduced.  summary:
    registration.SceneRecall (or anything with its .scenes() / .overall()), one scene per name.  Where MATLAB would print NaN (a scene
    without a non-consecutive ground-truth pair) the ratio is 0."""
    scenes = summary.scenes()
    if len(scene_names) != len(scenes):
        raise ValueError("registration_recall_lines: %d names, %d scenes" % (len(scene_names), len(scenes)))
    lines = ["recall : %s ( %s / %s )" % (_num2str(per[c]["recall"]), _num2str(per[c]["good"]), _num2str(per[c]["gt_num"])) for per in scenes]
    o = summary.overall(c)
    lines += ["Mean registration recall: %f precision: %f" % (o["mean_recall"], o["mean_precision"]),
              "True average recall: %f (%d/%d)" % (o["true_recall"], o["total_tp"], o["total_gt"])]
    return lines


# ---- the lines of repeatability/evaluate_3dmatch_our.py / evaluate_kitti_our.py -------------------------------------------------
def repeatability_table(num_keypts, scene_values):
    """The lines both scripts print, one per keypoint count (evaluate_3dmatch_our.py:66, evaluate_kitti_our.py:44), from values
    computed elsewhere (registration.repeatability_pairs(...).scene(), or an average of several scenes' values): ->
    (["Average Repeatability at num_keypts = K: v", ...], {K: v})."""
    ks, vs = [int(k) for k in num_keypts], [float(v) for v in np.asarray(scene_values, dtype=np.float64).reshape(-1)]
    if len(ks) != len(vs):
        raise ValueError("repeatability_table: %d counts, %d values" % (len(ks), len(vs)))
    return [f"Average Repeatability at num_keypts = {k}: {v}" for k, v in zip(ks, vs)], dict(zip(ks, vs))


# ---- the tables of datasets/cal_overlap.py ------------------------------------------------------------------------------------------
def save_overlap_tables(savepath, ids, pairs, ratios, matches, split="train", downsample=0.025):
    """The two pickles of cal_overlap.py:128-131 under `savepath`, by the reference's file names (:88-89): for every pair handed over --
    the reference keeps those with a ratio above 0.30, :121-123 -- '<anc id>@<pos id>' -> overlap ratio (a Python float) in
    3DMatch_<split>_<downsample>_overlap.pkl and -> int32[M, 2] rows [anchor index, positive index] in ..._keypts.pkl.  ids: the
    fragments' id strings ('<scene>/<seq>/cloud_bin_<k>'); pairs: (anchor, positive) positions in ids; matches: one array per pair
    (overlap.PairOverlap.matches).  Returns the two paths."""
    import pickle
    pairs, ratios, matches = list(pairs), list(ratios), list(matches)
    if not len(pairs) == len(ratios) == len(matches):
        raise ValueError("save_overlap_tables: %d pairs, %d ratios, %d match arrays" % (len(pairs), len(ratios), len(matches)))
    overlap_ratio, keypts_pairs = {}, {}
    for (a, b), r, m in zip(pairs, ratios, matches):
        m = np.asarray(m)
        if m.ndim != 2 or m.shape[1] != 2:
            raise ValueError("save_overlap_tables: matches of shape %s for pair (%d, %d)" % (m.shape, a, b))
        key = f'{ids[int(a)]}@{ids[int(b)]}'
        keypts_pairs[key] = np.ascontiguousarray(m, dtype=np.int32)
        overlap_ratio[key] = float(r)
    os.makedirs(savepath, exist_ok=True)
    out = []
    for name, table in (("overlap", overlap_ratio), ("keypts", keypts_pairs)):
        path = os.path.join(savepath, f'3DMatch_{split}_{downsample:.3f}_{name}.pkl')
        with open(path, "wb") as f:
            pickle.dump(table, f)
        out.append(path)
    return out


# ---- the files and log lines of ModelTester.test_kitti (utils/tester.py:235-360) ----------------------------------------------------
def kitti_pair_filename(anc_id, pos_id):
    """tester.py:298: '<drive>@<t0>-<t1>.npz' from the generator's ids '<drive>@<t0>' and '<drive>@<t1>' (str or bytes)."""
    a, p = (s.decode("utf-8") if isinstance(s, bytes) else str(s) for s in (anc_id, pos_id))
    return a + "-" + p.split("@")[-1] + ".npz"


def save_kitti_pair(directory, anc_id, pos_id, T, anc_pts, pos_pts, anc_scores, pos_scores):
    """The per-pair file of tester.py:317-323 under `directory`: trans f32[4,4] (T as [3,4] or [4,4], source -> target) and the
    keypoints and scores of both clouds.  Returns the path."""
    T = np.asarray(T, dtype=np.float32)
    if T.shape == (3, 4):
        T = np.vstack([T, np.array([[0, 0, 0, 1]], np.float32)])
    if T.shape != (4, 4):
        raise ValueError("save_kitti_pair: T of shape %s" % (T.shape,))
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, kitti_pair_filename(anc_id, pos_id))
    np.savez(path, trans=T, anc_pts=np.asarray(anc_pts), pos_pts=np.asarray(pos_pts), anc_scores=np.asarray(anc_scores),
             pos_scores=np.asarray(pos_scores))
    return path


def _meter(s, sq, n):
    n = int(n)
    avg = float(s) / n if n else 0                       # AverageMeter.reset: avg = 0 until the first update
    return dict(sum=float(s), count=n, avg=avg, var=float(sq) / n - avg ** 2 if n else float("nan"))


def kitti_meters_from_sums(sums):
    """The three AverageMeters of tester.py:252 from the eight sums of d3f_pose_errors (rte sum, square sum, number; the same of
    rre in degrees; successes; pairs) -> {"rte" | "rre" | "success": dict(sum, count, avg, var)}; var is NaN for a meter without an
    update (the reference has no such attribute then)."""
    s = [float(v) for v in np.asarray(sums, dtype=np.float64).reshape(8)]
    return dict(rte=_meter(s[0], s[1], s[2]), rre=_meter(s[3], s[4], s[5]), success=_meter(s[6], s[6], s[7]))


def kitti_meters(rte, rre_deg, flags):
    """kitti_meters_from_sums of per-pair arrays (flags: bit 0 rte under its threshold, bit 1 rre, bit 2 success), summed in pair
    order in float64 as the reference's loop updates its meters (tester.py:332-341)."""
    rte, rre_deg, flags = np.asarray(rte, np.float64), np.asarray(rre_deg, np.float64), np.asarray(flags)
    s = [0.0] * 8
    for t, r, f in zip(rte, rre_deg, flags):
        if f & 1:
            s[0] += t; s[1] += t * t; s[2] += 1
        if f & 2:
            s[3] += r; s[4] += r * r; s[5] += 1
        s[6] += 1 if f & 4 else 0
        s[7] += 1
    return kitti_meters_from_sums(s)


def kitti_lines(anc_ids, rte, rre_deg, flags, every=10, feat_times=None, reg_times=None, final=None):
    """The log lines of ModelTester.test_kitti without their time stamps, in its order: per failed pair
    "b'<id>' Failed with RTE: .., RRE: .." (tester.py:342), after every `every` pairs the running line (:347-352, the two timers averaged
    since the last such line and then reset), and the closing "Total loss" line (:356-360).  anc_ids: str or bytes per pair; rte /
    rre_deg / flags: the per-pair arrays of registration.pose_errors(...).host() (one column); feat_times / reg_times: seconds per
    pair (None: 0.0); final: the meters of the closing line (PairPoseErrors.meters(); None: from the arrays).  The loss is the
    constant 0 the reference sets (:328), Success is the float sum over the integer count."""
    rte, rre_deg, flags = (np.asarray(a).reshape(-1) for a in (rte, rre_deg, flags))
    n = len(anc_ids)
    if not (rte.shape[0] == rre_deg.shape[0] == flags.shape[0] == n):
        raise ValueError("kitti_lines: %d ids, %d / %d / %d figures" % (n, rte.shape[0], rre_deg.shape[0], flags.shape[0]))
    every = int(every)
    ft = np.zeros(n) if feat_times is None else np.asarray(feat_times, np.float64)
    rt = np.zeros(n) if reg_times is None else np.asarray(reg_times, np.float64)
    lines = []
    for i in range(n):
        if not flags[i] & 4:
            a = anc_ids[i] if isinstance(anc_ids[i], bytes) else str(anc_ids[i]).encode("utf-8")
            lines.append(f"{a} Failed with RTE: {float(rte[i])}, RRE: {float(rre_deg[i])}")
        if (i + 1) % every == 0:
            m = kitti_meters(rte[:i + 1], rre_deg[:i + 1], flags[:i + 1])
            w = slice(i + 1 - every, i + 1)
            lines.append(f"{i+1} / {n}: Feat time: {float(np.mean(ft[w]))}, Reg time: {float(np.mean(rt[w]))}, Loss: {0.0},"
                         f" RTE: {m['rte']['avg']}, RRE: {m['rre']['avg']}, Success: {m['success']['sum']} / {m['success']['count']}"
                         f" ({m['success']['avg'] * 100} %)")
    m = final if final is not None else kitti_meters(rte, rre_deg, flags)
    lines.append(f"Total loss: {0.0}, RTE: {m['rte']['avg']}, var: {m['rte']['var']}, RRE: {m['rre']['avg']}, var: {m['rre']['var']},"
                 f" Success: {m['success']['sum']} / {m['success']['count']} ({m['success']['avg'] * 100} %)")
    return lines
