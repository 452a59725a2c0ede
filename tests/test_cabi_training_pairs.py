"""d3f_training_pairs checks its arguments on the host before anything touches the device: every D3F_ERR_ARG condition of
include/d3feat_amd.h, the workspace rule and the size function, without a GPU.  Every case is a valid call with ONE argument spoilt (a
valid call is never made: it would launch)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def _call(lib, a):
    return lib.d3f_training_pairs(a["grid"], a["grid_bytes"], a["points"], a["N"], a["lens"], a["P"], a["trans"], a["keypts_pairs"], a["L"],
                                  a["pair_start"], a["radius"], a["keypts_num"], a["min_matches"], 7, a["step_dev"], a["use_host_step"], 3,
                                  a["pair0"], a["noise"], a["rotation"], a["scale_min"], a["scale_max"], a["shift"], a["out"], a["backup"],
                                  a["anc"], a["pos"], a["ld_idx"], a["n"], a["row0"], a["matches"], a["status"], a["params"], a["ws"],
                                  a["wsb"], None)


def test_training_pairs_refuses_bad_arguments_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    nan = float("nan")
    common = dict(points=p, N=1000, lens=p, P=2, radius=0.45, keypts_num=64, min_matches=64, step_dev=p, use_host_step=0, pair0=0,
                  noise=0.01, rotation=1, scale_min=0.8, scale_max=1.2, shift=2.0, out=p, backup=p, anc=p, pos=p, ld_idx=64, n=p, row0=p,
                  matches=p, status=p, params=p, ws=p, wsb=1 << 30)
    radius_form = dict(common, grid=p, grid_bytes=1 << 30, trans=p, keypts_pairs=None, L=0, pair_start=None)
    list_form = dict(common, grid=None, grid_bytes=0, trans=None, keypts_pairs=p, L=100, pair_start=p)
    bad = [("N", -1), ("P", 0), ("P", -3), ("P", 128), ("keypts_num", 0), ("keypts_num", -1), ("keypts_num", 1025), ("ld_idx", 63),
           ("pair0", -1), ("rotation", 2), ("rotation", -1), ("rotation", 4), ("noise", nan), ("scale_min", nan), ("scale_max", nan),
           ("shift", nan), ("step_dev", None), ("lens", None), ("points", None), ("out", None), ("backup", None), ("anc", None),
           ("pos", None), ("n", None), ("row0", None), ("matches", None), ("status", None), ("params", None)]
    for form, extra in ((radius_form, [("radius", 0.0), ("radius", -0.45), ("radius", nan), ("radius", float("inf")), ("trans", None)]),
                        (list_form, [("keypts_pairs", None), ("pair_start", None), ("L", -1)])):
        for name, value in bad + extra:
            assert _call(lib, dict(form, **{name: value})) == -3, (name, value)
        # 2 P = 254 clouds are the most one call takes; the workspace: none, or one byte short
        need = lib.d3f_training_pairs_workspace_bytes(1000, 2, 64)
        assert need > 0
        assert _call(lib, dict(form, ws=None)) == -2 and _call(lib, dict(form, wsb=need - 1)) == -2
    # a grid object smaller than d3f_neighbor_grid_bytes(N, 2 P)
    assert _call(lib, dict(radius_form, grid_bytes=lib.d3f_neighbor_grid_bytes(1000, 4) - 1)) == -2
    # the radius is not read in the list form
    assert _call(lib, dict(list_form, radius=0.0, wsb=0)) == -2


def test_training_pairs_workspace_bytes(lib):
    f = lib.d3f_training_pairs_workspace_bytes
    assert f(-1, 2, 64) == 0 and f(1000, 0, 64) == 0 and f(1000, 128, 64) == 0 and f(1000, 2, 0) == 0 and f(1000, 2, 1025) == 0
    assert f(1000, 127, 1024) > 0 and f(0, 1, 1) > 0
    # 8 bytes per row, 4 per sample entry, and the per-call words: linear in each
    assert 0 < f(200000, 2, 64) - f(100000, 2, 64) - 8 * 100000 <= 1024
    assert f(1000, 2, 1024) - f(1000, 2, 512) == 4 * 2 * 512
    assert f(1000, 2, 64) >= 8 * 1001 + 4 * 128


def test_training_draw_refuses_bad_arguments(lib):
    out = ctypes.c_uint64()
    assert lib.d3f_training_draw(1, 2, 3, 4, 5, None) == -3
    assert lib.d3f_training_draw(1, 2, -1, 4, 5, ctypes.byref(out)) == -3
    assert lib.d3f_training_draw(1, 2, 3, 256, 5, ctypes.byref(out)) == -3 and lib.d3f_training_draw(1, 2, 3, -1, 5, ctypes.byref(out)) == -3
    assert lib.d3f_training_draw(1, 2, 3, 255, 5, ctypes.byref(out)) == 0
