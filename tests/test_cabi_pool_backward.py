"""d3f_ind_max_pool_backward and d3f_closest_pool_cat_backward check their arguments on the host: every case is a valid call with ONE
argument spoilt and comes back as D3F_ERR_ARG before anything touches the device (a valid call is never made: it would launch)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def test_max_pool_backward_refuses_bad_arguments_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(x=p, N1=20, ldx=8, C=8, idx=p, N2=9, ld_idx=5, K=5, y=p, ldy=8, gy=p, ldg=8, start=p, edges=p, gx=p, ldgx=8, bf16=0,
                ws=p, wsb=1 << 15)

    def call(**over):
        a = dict(good, **over)
        return lib.d3f_ind_max_pool_backward(a["x"], a["N1"], a["ldx"], a["C"], a["idx"], a["N2"], a["ld_idx"], a["K"], a["y"], a["ldy"],
                                             a["gy"], a["ldg"], a["start"], a["edges"], a["gx"], a["ldgx"], None, None, a["bf16"], a["ws"],
                                             a["wsb"], None)
    for bad in (dict(bf16=1), dict(N1=-1), dict(N2=-1), dict(K=-1, ld_idx=0), dict(C=0), dict(C=(1 << 20) + 1, ldx=1 << 21, ldy=1 << 21, ldg=1 << 21, ldgx=1 << 21),
                dict(ldx=7), dict(ldy=7), dict(ldg=7), dict(ldgx=7), dict(ld_idx=4), dict(x=None), dict(gx=None), dict(start=None),
                dict(y=None), dict(gy=None), dict(idx=None), dict(edges=None), dict(N2=1 << 20, K=1 << 11, ld_idx=1 << 11),
                dict(N2=524287, K=4096, ld_idx=4096)):
        assert call(**bad) == -3, bad
    assert call(wsb=64) == -2 and call(ws=None) == -2
    assert call(N1=0, x=None, gx=None, start=None) == 0                                         # nothing to write
    size = lib.d3f_ind_max_pool_backward_workspace_bytes
    assert size(-1, 9, 5, 8) == 0 and size(20, -1, 5, 8) == 0 and size(20, 9, -1, 8) == 0 and size(20, 9, 5, 0) == 0
    assert size(20, 1 << 20, 1 << 11, 8) == 0 and size(20, 9, 5, (1 << 20) + 1) == 0
    assert 0 < size(0, 0, 0, 1) <= size(20, 9, 5, 8) <= size(30000, 9000, 40, 64) <= size(30000, 9000, 40, 130)
    # gs: one padded row of quads per pooled row; the rest is slice partials and column vectors
    for C in (1, 64, 130):
        quads = (C + 3) // 4 * 16
        assert 9000 * quads <= size(30000, 9000, 40, C) <= 9000 * quads + (118 + 36) * C * 8 + 8 * 256 + 2 * C * 4


def test_upsample_backward_refuses_bad_arguments_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    good = dict(g=p, N2=30, ldg=12, C1=4, idx=p, ld_idx=3, N1=10, start=p, edges=p, gx=p, ldgx=4)

    def call(**over):
        a = dict(good, **over)
        return lib.d3f_closest_pool_cat_backward(a["g"], a["N2"], a["ldg"], a["C1"], a["idx"], a["ld_idx"], a["N1"], a["start"], a["edges"],
                                                 a["gx"], a["ldgx"], None, None, None)
    for bad in (dict(N1=-1), dict(N2=-1), dict(C1=0), dict(C1=(1 << 20) + 1, ldg=1 << 21, ldgx=1 << 21), dict(ldg=3), dict(ldgx=3), dict(ld_idx=0),
                dict(gx=None), dict(start=None), dict(g=None), dict(idx=None), dict(edges=None), dict(N2=(1 << 31) - 8191)):
        assert call(**bad) == -3, bad
    assert call(N1=0, gx=None, start=None) == 0
