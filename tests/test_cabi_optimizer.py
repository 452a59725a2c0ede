"""d3f_momentum_sgd checks its arguments on the host: every case is a valid call with ONE argument spoilt and comes back with its code
before anything touches the device (a valid call is never made: it would launch)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    return _lib.load()


def test_momentum_sgd_refuses_bad_arguments_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    size = lib.d3f_momentum_sgd_workspace_bytes
    good = dict(desc=p, T=7, chunks=p, nchunks=12, hyper=p, zero=0, reg=p, ws=p, wsb=size(7, 12))

    def call(**over):
        a = dict(good, **over)
        return lib.d3f_momentum_sgd(a["desc"], a["T"], a["chunks"], a["nchunks"], a["hyper"], a["zero"], a["reg"], a["ws"], a["wsb"], None)
    for bad in (dict(T=-1), dict(nchunks=-1), dict(desc=None), dict(chunks=None), dict(hyper=None)):
        assert call(**bad) == -3, bad
    assert call(wsb=size(7, 12) - 1) == -2 and call(ws=None) == -2 and call(wsb=0) == -2
    assert call(T=0, nchunks=0, desc=None, chunks=None, ws=None, wsb=0) == 0                   # nothing to launch
    assert call(T=0, nchunks=0, hyper=None) == -3
    assert size(-1, 12) == 0 and size(7, -1) == 0
    assert 0 < size(0, 0) <= size(1, 1) <= size(7, 12) <= size(7, 6000) <= size(300, 6000) <= size(300, 1 << 20)
    for n in (12, 6000, 1 << 20):                                                              # two float64 partials per chunk
        assert 16 * n <= size(7, n) <= 16 * n + 2 * 256
