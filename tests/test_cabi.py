"""The drop-in boundary: libd3feat_amd.so loads on a machine without a GPU and exports exactly the entry points that
include/d3feat_amd.h declares, with the argument lists the ctypes binding (d3feat_amd/_lib.py) assumes.
No compute call is made here (no GPU in the CPU test tier)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "d3feat_amd.h")

_C2CT = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}


def _declarations():
    """-> {name: (return type, [argument C types])} parsed from the header."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(d3f_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        types = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    types.append("ptr")
                else:
                    types.append(a.replace("const ", "").split()[0])
        out[name] = (ret, types)
    return out


@pytest.fixture(scope="module")
def lib():
    from d3feat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "d3feat_amd", "csrc")])
    return _lib.load()


def test_header_declares_the_expected_entry_points():
    decl = _declarations()
    for must in ("d3f_batch_grid_subsample", "d3f_batch_radius_neighbors", "d3f_neighbor_grid_build",
                 "d3f_neighbor_grid_search", "d3f_kpconv_aggregate", "d3f_kpconv_fused_c1", "d3f_gemm_f32",
                 "d3f_ind_max_pool", "d3f_closest_pool_cat", "d3f_detect_head", "d3f_affine_act", "d3f_version"):
        assert must in decl, must
    # plain C ABI: no torch / HIP types anywhere in the signatures
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "torch" not in code and "hipStream_t" not in code and "#include <hip" not in code


def test_library_exports_every_declared_symbol(lib):
    for name in _declarations():
        assert hasattr(lib, name), "libd3feat_amd.so does not export %s" % name


def test_binding_matches_header():
    from d3feat_amd import _lib
    decl = _declarations()
    assert set(decl) == set(_lib.SIGNATURES), set(decl) ^ set(_lib.SIGNATURES)
    for name, (ret, types) in decl.items():
        res, args = _lib.SIGNATURES[name]
        assert res is _C2CT[ret], name
        assert len(args) == len(types), "%s: header has %d arguments, binding %d" % (name, len(types), len(args))
        for i, (t, a) in enumerate(zip(types, args)):
            want = ctypes.c_void_p if t == "ptr" else _C2CT[t]
            assert a is want, "%s argument %d: header %s, binding %s" % (name, i, t, a)


def test_exports_are_unmangled_c_symbols(lib):
    from d3feat_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (d3f_[a-z0-9_]+)\b", nm))
    assert set(_declarations()) <= exported


def test_host_side_argument_checks_need_no_gpu(lib):
    """Entry points validate sizes before touching the device: invalid arguments come back as D3F_ERR_ARG."""
    assert lib.d3f_version() >= 100
    assert lib.d3f_gemm_f32(None, 0, None, 0, None, 0, -1, 4, 4, None, None, None, None, 0, 0, 0.2, None, 0, None, 0, None) == -3
    assert lib.d3f_batch_grid_subsample(None, 10, None, 1, 0.1, None, 0, None, 0, None, None, None, None, None, None, 0, None) == -3
    assert lib.d3f_neighbor_grid_build(None, 5, None, 0, 0.1, None, 0, None) == -3
    assert lib.d3f_grid_subsample_workspace_bytes(30000, 2, 0, 0) > 30000 * 4 * 14
    assert lib.d3f_gemm_workspace_bytes(390, 512, 7680, 0) >= 256
    assert lib.d3f_neighbor_grid_bytes(60000, 2) > 60000 * 16
    # the one-kernel KPConv forms address rows with 24-bit multiplies: row counts / leading dimensions beyond that are refused
    # before anything is launched (include/d3feat_amd.h; the two-kernel form has no such limit)
    import ctypes
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    kp = (ctypes.c_float * 45)()
    args = lambda Nq, Ns, ld_idx, ldf: (p, Nq, p, Ns, p, ld_idx, 8, p, ldf, p, ctypes.addressof(kp), 15, 0.05, 1, 0, p, None, None, None, 0, 1, 0.2,
                                        p, 32, None, None, None, 0, None)
    assert lib.d3f_kpconv_fused32(*args(100, 1 << 24, 8, 32)) == -3
    assert lib.d3f_kpconv_fused32(*args(100, 1 << 20, 8, 1 << 12)) == -3        # Ns * ldf >= 2^31
    assert lib.d3f_kpconv_fused32(*args(1 << 24, 100, 8, 32)) == -3


def test_registration_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """d3f_feature_nn, d3f_ransac_hypotheses, d3f_neighbor_grid_score and d3f_mutual_matches check their arguments on the host before
    anything touches the device."""
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.d3f_feature_nn(p, 4, 48, p, 4, 48, 48, p, None, p, 4096, None) == -3            # C = 48
    assert lib.d3f_feature_nn(p, 4, 31, p, 4, 32, 32, p, None, p, 4096, None) == -3            # lda < C
    assert lib.d3f_feature_nn(p, 4, 32, p, 4, 31, 32, p, None, p, 4096, None) == -3            # ldb < C
    for n in (2, 9):
        assert lib.d3f_ransac_hypotheses(p, 10, p, 10, p, n, 0.9, 0.05, 1, 0, 8, p, p, None) == -3
    assert lib.d3f_ransac_hypotheses(p, 0, p, 10, p, 4, 0.9, 0.05, 1, 0, 8, p, p, None) == -3  # Ns = 0
    assert lib.d3f_neighbor_grid_score(p, 4096, 10, p, 10, p, 1, float("nan"), p, p, None, None) == -3
    assert lib.d3f_neighbor_grid_score(p, 4096, 10, p, 10, p, -1, 0.05, p, p, None, None) == -3
    assert lib.d3f_mutual_matches(p, 10, p, 10, p, None, p, 4096, None) == -3                  # count_dev == NULL


def test_capacity_mode_subsample_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """d3f_batch_grid_subsample_async, _async_inplace and _async_boxed share one argument check: each of them answers D3F_ERR_ARG
    for every argument it rejects, before anything touches the device.  Every case is a valid call with ONE argument spoilt (a
    valid call is never made: it would launch)."""
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    good = dict(points=p, clouds=None, N_cap=1000, lens=p, B=2, dl=0.05, sub=p, M_cap=500, elem_cap=300, elem_points_cap=600,
                sub_lens=p, status=p, bbox_in=None, bbox_out=None)

    def stacked(a):
        return lib.d3f_batch_grid_subsample_async(a["points"], a["N_cap"], a["lens"], a["B"], a["dl"], a["sub"], a["M_cap"],
                                                  a["elem_cap"], a["elem_points_cap"], a["sub_lens"], a["status"], p, 4096, None)

    def inplace(a):
        return lib.d3f_batch_grid_subsample_async_inplace(a["points"], a["N_cap"], a["lens"], a["B"], a["dl"], a["sub"], a["M_cap"],
                                                          a["elem_cap"], a["sub_lens"], a["status"], p, 4096, None)

    def boxed(a):
        return lib.d3f_batch_grid_subsample_async_boxed(a["points"], a["clouds"], a["N_cap"], a["lens"], a["B"], a["dl"], a["sub"],
                                                        a["M_cap"], a["elem_cap"], a["elem_points_cap"], a["sub_lens"], a["status"],
                                                        a["bbox_in"], a["bbox_out"], p, 4096, None)

    common = [("N_cap", 0), ("N_cap", -5), ("N_cap", (1 << 30) + 1), ("M_cap", 0), ("M_cap", -1), ("elem_cap", -1), ("B", 0),
              ("B", 256), ("dl", 0.0), ("dl", -0.05), ("dl", float("nan")), ("points", None), ("lens", None), ("sub", None),
              ("sub_lens", None), ("status", None)]
    for entry, extra in ((stacked, [("elem_points_cap", -1)]), (inplace, []), (boxed, [("elem_points_cap", -1)])):
        for name, bad in common + extra:      # (`points` is the first argument: the pointer table of the in-place entry)
            assert entry(dict(good, **{name: bad})) == -3, (entry.__name__, name, bad)
    # the boxed entry takes the stacked clouds or the pointer table: exactly one of the two
    assert boxed(dict(good, clouds=p)) == -3
    assert boxed(dict(good, points=None, clouds=None)) == -3
    for name, bad in common:
        if name != "points":
            assert boxed(dict(good, points=None, clouds=p, **{name: bad})) == -3, ("boxed, in place", name, bad)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from d3feat_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.D3FeatLibraryError):
        _lib.load()


def test_cpu_tensors_are_rejected():
    """There is no CPU fallback: handing a host tensor to an op raises instead of computing somewhere else."""
    import torch
    from d3feat_amd import _lib, ops
    with pytest.raises(_lib.D3FeatLibraryError):
        ops.gemm(torch.zeros(4, 4), torch.zeros(4, 4))


def _plan(M, N, K, hint=0):
    from d3feat_amd import _lib
    r, c, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.load().d3f_gemm_x3_plan(M, N, K, hint, ctypes.byref(r), ctypes.byref(c), ctypes.byref(s)) == 0
    return r.value, c.value, s.value


def test_gemm_x3_plans():
    """The cost model of the launcher (rounds of resident workgroups x k-tiles per slice): which of tests/test_gpu_gemm_x3.py's problems run as
    128 x 32, 128 x 64 and 256 x 128 workgroups, split in K or not -- so that every kernel instantiation is exercised there.  Host code only: no GPU."""
    assert _plan(20000, 32, 64) == (128, 32, 1) and _plan(20000, 64, 128) == (128, 64, 1)
    assert _plan(20001, 256, 1024)[:2] == (256, 128) and _plan(20001, 200, 1024)[:2] == (256, 128) and _plan(30000, 256, 256)[:2] == (256, 128)
    assert _plan(4525, 512, 3072) == (256, 128, 3)                        # the network's level-3 decoder contraction at F = 5
    rows, cols, s = _plan(900, 256, 3840)
    assert (rows, cols) == (128, 64) and s > 1                            # skinny deep layer: split in K
    assert _plan(300000, 64, 256, 171000)[:2] == (128, 64)
    from d3feat_amd import _lib
    assert _lib.load().d3f_gemm_x3_plan(100, 64, 48, 0, None, None, None) == -3


def _gemm_call(lib, entry, A, W, Cp, M=100, N=64, C1=64, skip=None, C2=0, res=None, cs=None, ws=None, wsb=0, res_idx=None, ld_res_idx=1,
               a_bf16=0):
    """one call of a composite-operand contraction entry point (d3f_gemm_f32t / _x3 / _x3_gres / _bf16) with host-side arguments only"""
    head = [A, M, C1, C1, None, 0, skip, C2, C2, W, Cp, N, M, N, None, cs, None, res, N if res else 0]
    tail = [0, 0.2, ws, wsb, None, None, 0]
    if entry == "d3f_gemm_x3_gres":
        head += [res_idx, ld_res_idx, 50, None]
    if entry == "d3f_gemm_bf16":
        tail += [a_bf16, 0]
    return getattr(lib, entry)(*(head + tail + [None]))


def test_gemm_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """The six contraction entry points check addressing rules, the gathered-residual arguments and the workspace of a K-split plan on
    the host, before anything is launched; M = 0 is D3F_OK whatever the pointers are (tests/test_gpu_gemm_branches.py runs what they
    accept)."""
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    composite = ("d3f_gemm_f32t", "d3f_gemm_x3", "d3f_gemm_x3_gres", "d3f_gemm_bf16")
    for e in composite:
        # misaligned bases: A, the packed weights, the skip operand
        assert _gemm_call(lib, e, p + 4, p, p) == -3, e
        assert _gemm_call(lib, e, p, p + 8, p) == -3, e
        assert _gemm_call(lib, e, p, p, p, C1=32, skip=p + 4, C2=32) == -3, e
        assert _gemm_call(lib, e, None, p, p) == -3 and _gemm_call(lib, e, p, None, p) == -3 and _gemm_call(lib, e, p, p, None) == -3, e
        if e != "d3f_gemm_bf16":                        # fp32 in and out: the output, the residual and the column vectors too
            assert _gemm_call(lib, e, p, p, p + 4) == -3, e
            assert _gemm_call(lib, e, p, p, p, res=p + 8) == -3, e
            assert _gemm_call(lib, e, p, p, p, cs=p + 4) == -3, e
        # M = 0: nothing to launch, pointers are not looked at
        assert _gemm_call(lib, e, None, None, None, M=0) == 0, e
    assert _gemm_call(lib, "d3f_gemm_bf16", p + 4, p, p, a_bf16=1) == -3          # bfloat16 features: 8-byte aligned rows
    # x3: a concatenation whose first part is no whole k-tile (K = 64 itself is fine), K no multiple of 32
    for e in ("d3f_gemm_x3", "d3f_gemm_x3_gres"):
        assert _gemm_call(lib, e, p, p, p, C1=48, skip=p, C2=16) == -3, e
        assert _gemm_call(lib, e, p, p, p, C1=48) == -3, e
    # the gathered residual: an index without a residual, a leading dimension below 1
    assert _gemm_call(lib, "d3f_gemm_x3_gres", p, p, p, res=None, res_idx=p) == -3
    assert _gemm_call(lib, "d3f_gemm_x3_gres", p, p, p, res=p, res_idx=p, ld_res_idx=0) == -3
    # a K-split plan (S = 2 at these shapes) with a workspace one byte short, or none
    for e, M, K in (("d3f_gemm_f32t", 100, 544), ("d3f_gemm_bf16", 100, 544), ("d3f_gemm_x3", 200, 352), ("d3f_gemm_x3_gres", 200, 352)):
        ws_fn = {"d3f_gemm_f32t": lib.d3f_gemm_workspace_bytes, "d3f_gemm_bf16": lib.d3f_gemm_bf16_workspace_bytes}.get(e, lib.d3f_gemm_x3_workspace_bytes)
        need = 2 * M * 64 * 4
        assert ws_fn(M, 64, K, 0) == need + 256, e
        assert _gemm_call(lib, e, p, p, p, M=M, C1=K, ws=p, wsb=need - 1) == -2, e
        assert _gemm_call(lib, e, p, p, p, M=M, C1=K, ws=None, wsb=need) == -2, e
    # d3f_gemm_f32 / d3f_gemm_upsample_cat_f32 take any alignment; what they refuse: short leading dimensions, a skip operand that is
    # not float4-addressable, a short workspace
    f32 = lambda M=100, N=64, K=544, lda=544, ldb=64, ldc=64, ws=None, wsb=0, A=p: lib.d3f_gemm_f32(
        A, lda, p, ldb, p, ldc, M, N, K, None, None, None, None, 0, 0, 0.2, ws, wsb, None, 0, None)
    assert f32(lda=543) == -3 and f32(ldb=63) == -3 and f32(ldc=63) == -3 and f32(A=None) == -3
    assert f32(ws=p, wsb=2 * 100 * 64 * 4 - 1) == -2 and f32(ws=None, wsb=1 << 20) == -2
    assert lib.d3f_gemm_f32(None, 64, None, 64, None, 64, 0, 64, 64, None, None, None, None, 0, 0, 0.2, None, 0, None, 0, None) == 0
    cat = lambda M=100, skip=p, lds=508, C1=36, C2=508, idx=p, ld_idx=1, ws=None, wsb=0: lib.d3f_gemm_upsample_cat_f32(
        p, 50, C1, C1, idx, ld_idx, skip, lds, C2, p, 64, p, 64, M, 64, None, None, 0, 0.2, ws, wsb, None, None, 0, None)
    assert cat(skip=p + 4) == -3 and cat(lds=509) == -3 and cat(C1=34, C2=510, lds=512) == -3 and cat(ld_idx=0) == -3
    assert cat(idx=None) == -3                                                    # rows in place need N1 >= M
    assert cat(ws=p, wsb=2 * 100 * 64 * 4 - 1) == -2
    assert cat(M=0, skip=None, idx=None) == 0
