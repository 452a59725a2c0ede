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
