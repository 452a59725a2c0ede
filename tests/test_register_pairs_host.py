"""Batched registration (d3f_register_pairs / registration.register_pairs), the part that needs no GPU: the two entry points are
exported and bound, every size is refused on the host before a launch, and the result files of
geometric_registration/evaluate.py (gt.log reader, .log blocks, .rt.txt files, recall figures) are written and read as there."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def test_entry_points_are_exported_and_bound(lib):
    from d3feat_amd import _lib
    for name in ("d3f_register_pairs", "d3f_register_pairs_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "d3feat_amd.h")).read()
    m = re.search(r"#define\s+D3F_PAIRS_KMAX\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.PAIRS_KMAX == 1024


def _args(lib, P=4, n_blocks=3, K=250, ld=36, C=32, num_keypts=0, radius=0.05, ransac_n=3, max_iteration=50000, max_validation=1000,
          null=(), gt=False, short=0):
    """Argument list of d3f_register_pairs over one dummy host buffer (nothing is launched: every call here is refused first)."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    need = lib.d3f_register_pairs_workspace_bytes(P, K, num_keypts, max_validation)
    outs = ["T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "nearest", "mutual", "gt_inliers"]
    ptrs = [None if o in null else p for o in outs]
    return ([p, n_blocks, K, ld, C, p, p, P, num_keypts, radius, ransac_n, 0.9, 0.05, max_iteration, max_validation, 5,
             p if gt else None, 0.10] + ptrs + [p, need - short, None]), buf


def test_host_side_argument_checks(lib):
    call = lambda **kw: lib.d3f_register_pairs(*_args(lib, **kw)[0])
    assert call(K=1025) == -3                                   # more rows than D3F_PAIRS_KMAX
    assert call(K=4096, num_keypts=1025) == -3
    assert call(ransac_n=2) == -3 and call(ransac_n=9) == -3
    assert call(C=24, ld=28) == -3
    assert call(ld=35) == -3                                    # ld < C + 4
    assert call(P=-1) == -3
    for out in ("T", "inliers", "sumd2", "validations", "iterations", "best_iteration", "mutual_count", "nearest"):
        assert call(null=(out,)) == -3, out
    assert call(gt=True, null=("gt_inliers",)) == -3            # gt without a place for its count
    assert call(max_validation=0) == -3 and call(max_iteration=-1) == -3
    assert call(short=1) == -2                                  # workspace one byte short
    assert call(P=0) == 0                                       # nothing to do: no launch


def test_workspace_size_grows_with_pairs_and_validations(lib):
    w = lib.d3f_register_pairs_workspace_bytes
    assert w(4096, 250, 0, 1000) >= 4096 * 1000 * 64
    assert w(8, 250, 0, 100) < w(16, 250, 0, 100) < w(16, 250, 0, 200)
    assert w(8, 1024, 250, 100) == w(8, 250, 0, 100)            # only the rows used count


def test_cpu_tensors_are_rejected():
    import torch
    from d3feat_amd import _lib, registration as reg
    kp, count, pairs = torch.zeros(2, 8, 36), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(_lib.D3FeatLibraryError):
        reg.register_pairs(kp, count, pairs, **reg.EVALUATE_3DMATCH)


def test_evaluate_3dmatch_is_the_reference_call():
    from d3feat_amd import registration as reg
    assert reg.EVALUATE_3DMATCH == dict(max_correspondence_distance=0.05, ransac_n=3, edge_similarity=0.9, checker_distance=0.05,
                                        max_iteration=50000, max_validation=1000)


def test_scene_pairs_order():
    import torch
    from d3feat_amd import registration as reg
    got = reg.scene_pairs(5, device=torch.device("cpu"))         # (the default is the current GPU)
    assert got.dtype == torch.int32 and tuple(got.shape) == (10, 2)
    assert [tuple(r) for r in got.tolist()] == [(i, j) for i in range(5) for j in range(i + 1, 5)]
    assert tuple(reg.scene_pairs(1, device=torch.device("cpu")).shape) == (0, 2)


def test_scene_is_deterministic_and_shaped():
    from d3feat_amd.utils.synthetic import scene
    blocks, poses = scene(3, n_frag=3, K=50)
    again, _ = scene(3, n_frag=3, K=50)
    assert len(blocks) == len(poses) == 3
    for b, a, M in zip(blocks, again, poses):
        assert b.shape == (50, 36) and b.dtype == np.float32 and np.array_equal(b, a)
        assert np.all(np.diff(b[:, 35]) >= 0)                                        # ascending score order
        assert np.allclose(np.linalg.norm(b[:, 3:35], axis=1), 1.0, atol=1e-5)
        assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-12) and np.linalg.det(M[:3, :3]) > 0


# ---- result files ----------------------------------------------------------------------------------------------------
FIXTURE = os.path.join(GOLDEN, "gt_log_hotel3.log")
# geometric_registration/gt_result/sun3d-hotel_umd-maryland_hotel3-evaluation/gt.log of the reference, 15 316 bytes, as it is
FIXTURE_SHA256 = "44b48a5d72d69fbba5b3c3b90aa487c588d5e73eedf0d1df10a9aac011c2a078"


def test_read_gt_log_fixture():
    from d3feat_amd.utils.results import read_gt_log
    assert hashlib.sha256(open(FIXTURE, "rb").read()).hexdigest() == FIXTURE_SHA256
    gt = read_gt_log(FIXTURE)
    n_lines = len(open(FIXTURE).readlines())
    assert n_lines % 5 == 0 and len(gt) == n_lines // 5 and len(gt) > 10
    assert list(gt)[0] == "0_1"
    assert np.array_equal(gt["0_1"][0], [9.68286000e-01, 2.75396785e-02, 2.48319350e-01, -5.10998423e-02])
    for key, M in gt.items():
        a, b = (int(x) for x in key.split("_"))
        assert a < b and M.shape == (4, 4) and np.array_equal(M[3], [0, 0, 0, 1])
        assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-5)


def test_registration_log_round_trip(tmp_path):
    from d3feat_amd.utils.results import read_gt_log, write_registration_log
    rng = np.random.default_rng(0)
    pairs, Ts = [(0, 1), (0, 7), (12, 31)], []
    for _ in pairs:
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-2, 2, 3)
        Ts.append(M)
    path = str(tmp_path / "D3Feat.log")
    write_registration_log(path, pairs[:2], Ts[:2])
    write_registration_log(path, pairs[2:], Ts[2:])               # appends, as the reference's 'a+'
    lines = open(path).readlines()
    assert lines[0] == "0\t 1\t  37\n" and lines[5] == f'{0}\t {7}\t  37\n' and len(lines) == 15
    inv = np.linalg.inv(Ts[0])
    assert lines[1] == f"{inv[0,0]}\t {inv[0,1]}\t {inv[0,2]}\t {inv[0,3]}\t \n"
    back = read_gt_log(path)
    assert list(back) == ["0_1", "0_7", "12_31"]
    for (a, b), M in zip(pairs, Ts):
        assert np.array_equal(back["%d_%d" % (a, b)], np.linalg.inv(M))      # repr precision: the very same doubles


def test_pair_results_and_recall(tmp_path):
    from d3feat_amd.utils.results import feature_matching_recall, write_pair_results
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    num = [40, 0, 3, 25, 7]
    ratio = [0.4, 0.0, 0.04999999, 0.123456789, 0.0500001]
    flag = [1, 0, 1, 1, 1]
    rows = write_pair_results(str(tmp_path / "res"), pairs, num, ratio, flag)
    assert sorted(os.listdir(tmp_path / "res")) == sorted("cloud_bin_%d_cloud_bin_%d.rt.txt" % p for p in pairs)
    assert open(tmp_path / "res" / "cloud_bin_1_cloud_bin_3.rt.txt").read() == "cloud_bin_1\tcloud_bin_3\t25\t0.12345679\t1"
    assert rows[3] == [25, 0.12345679, 1] and rows[1] == [0, 0.0, 0]
    # evaluate.py:200-219 on the rows as the files hold them
    result = np.array(rows)
    gt_results, pred_results = np.sum(result[:, 2] == 1), np.sum(result[:, 1] > 0.05)
    assert (gt_results, pred_results) == (4, 3)
    got = feature_matching_recall(rows, inlier_ratio=0.05)
    assert got["correct"] == 3 and got["gt"] == 4 and got["recall"] == float(pred_results / gt_results) * 100 == 75.0
    assert got["ave_num_inliers"] == np.sum(np.where(result[:, 2] == 1, result[:, 0], 0.0)) / pred_results == 25.0
    assert got["ave_inlier_ratio"] == np.sum(np.where(result[:, 2] == 1, result[:, 1], 0.0)) / pred_results
