"""torch-tensor front end of the C ABI (include/d3feat_amd.h).

PyTorch is used for three things only: device allocations (torch.empty on a CUDA/HIP device), the current
HIP stream, and torch.distributed.  Every computation below is a call into libd3feat_amd.so; nothing here
computes with torch ops and nothing falls back to the CPU.
"""
import ctypes

import os

import numpy as np
import torch

from . import _lib

_WS = {}

# Optional per-call HIP-event timing (bench.py): set PROFILE to a list to collect (name, info, start, end) records
# for the kpconv_aggregate / gemm_f32 launches issued on the current stream.
PROFILE = None


class _timed:
    def __init__(self, name, info, device):
        self.on = PROFILE is not None
        self.name, self.info, self.device = name, info, device

    def __enter__(self):
        if self.on:
            self.start = torch.cuda.Event(enable_timing=True)
            self.end = torch.cuda.Event(enable_timing=True)
            self.start.record(torch.cuda.current_stream(self.device))
        return self

    def __exit__(self, *exc):
        if self.on:
            self.end.record(torch.cuda.current_stream(self.device))
            PROFILE.append((self.name, self.info, self.start, self.end))
        return False


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def trace_marker(ident, device):
    """One named one-thread kernel on the current stream: cuts a rocprofv3 kernel trace at the ends of a timed region."""
    _lib.check(_lib.load().d3f_trace_marker(int(ident), _stream(device)), "trace_marker")


# ---- device-resident sizes ------------------------------------------------------------------------------------------
# A tensor whose row count is only an upper bound carries the real count as the attribute `n_dev` (int32[1] on the
# device); every op forwards it to the kernels (the `*_dev` arguments of include/d3feat_amd.h) and tags its outputs.
def _order(t):
    """Spatially coherent visiting order attached to a point / index tensor (attribute `order`, int32), or None."""
    o = getattr(t, "order", None) if t is not None else None
    return _ptr(o)


def _nd(t):
    return _ptr(getattr(t, "n_dev", None) if t is not None else None)


def _ptr(t):
    """Device address of an optional tensor (None -> NULL)."""
    return t.data_ptr() if t is not None else None


def _tag(out, src):
    d = getattr(src, "n_dev", None)
    if d is not None:
        out.n_dev = d
        out.n_hint = getattr(src, "n_hint", 0)   # expected row count (host int): plans launches, never bounds them
    return out


class private_workspace:
    """Scratch buffers allocated inside this context are not shared with (or resized by) later eager calls: used while
    a HIP graph is being captured, so that the graph keeps its own scratch alive."""

    def __enter__(self):
        global _WS
        self.prev, _WS = _WS, {}
        return self

    def __exit__(self, *exc):
        global _WS
        self.kept, _WS = _WS, self.prev
        return False


def workspace(nbytes, device):
    """Stream-ordered scratch: one growable byte buffer per (device, stream)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _req(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor on a GPU (got %s)" % (name, type(t)))
    if not t.is_cuda:
        raise _lib.D3FeatLibraryError("%s is on %s: d3feat_amd has no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must be %d-D (got shape %s)" % (name, ndim, tuple(t.shape)))
    return t


def _rows(t, name):
    """2-D tensor whose rows are contiguous -> (tensor, leading dimension in elements)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s must be 2-D with contiguous rows (shape %s strides %s)" % (name, tuple(t.shape), t.stride()))
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:
        raise ValueError("%s has overlapping rows" % name)
    return t, int(max(ld, 1))


def as_lens(lens, device):
    """Batch lengths as a device int32 tensor.  When the values are known on the host they ride along as the
    attribute `host_lens` (saves a device read-back wherever host logic needs them)."""
    if isinstance(lens, torch.Tensor):
        out = lens.to(device=device, dtype=torch.int32).contiguous()
        if out is not lens and hasattr(lens, "host_lens"):
            out.host_lens = lens.host_lens
        return out
    host = np.asarray(lens, dtype=np.int32).reshape(-1)
    out = torch.as_tensor(host, device=device)
    out.host_lens = [int(x) for x in host]
    return out


def host_lens(lens):
    """Python list of the batch lengths (reads the device tensor back only when no host copy rides along)."""
    if isinstance(lens, torch.Tensor):
        h = getattr(lens, "host_lens", None)
        return list(h) if h is not None else [int(x) for x in lens.tolist()]
    return [int(x) for x in np.asarray(lens).reshape(-1)]


def _raise_flags(flags, what):
    if flags:
        msgs = []
        if flags & _lib.ST_EMPTY_ELEMENT:
            msgs.append("a batch element is empty")
        if flags & _lib.ST_NEG_CELL:
            msgs.append("negative voxel index (origin above a point after fp32 rounding)")
        if flags & _lib.ST_KEY_RANGE:
            msgs.append("voxel key exceeds 2^56")
        if flags & _lib.ST_HIT_OVERFLOW:
            msgs.append("a query has more than %d in-radius supports" % _lib.NEIGHBOR_CAP)
        if flags & _lib.ST_OUT_OVERFLOW:
            msgs.append("more output rows than the capacity of the output buffer")
        if flags & _lib.ST_KEY_WIDTH:
            msgs.append("(element, voxel key) wider than the 32-bit sort key of the capacity-mode subsampling")
        raise _lib.D3FeatLibraryError("d3feat_amd.%s: %s" % (what, "; ".join(msgs)))
    return 0


def check_status(status, what):
    """status: int32[2] device tensor written by a kernel; raises on any D3F_ST_* flag. Synchronises."""
    st = status.tolist()
    _raise_flags(st[1], what)
    return st[0]


# ----------------------------------------------------------------------------------------------------------
def batch_grid_subsample(points, lens, dl, features=None, classes=None):
    """-> (sub_points f32[M,3], sub_lens i32[B] (device), sub_features | None, sub_classes | None).
    One host synchronisation (M is data dependent)."""
    lib = _lib.load()
    points = _req(points, torch.float32, "points", 2).contiguous()
    dev = points.device
    N = points.shape[0]
    lens_t = as_lens(lens, dev)
    B = lens_t.numel()
    fdim = ldim = 0
    if features is not None:
        features = _req(features, torch.float32, "features", 2).contiguous()
        fdim = features.shape[1]
    if classes is not None:
        classes = _req(classes, torch.int32, "classes", 2).contiguous()
        ldim = classes.shape[1]
    sub_p = torch.empty((max(N, 1), 3), dtype=torch.float32, device=dev)
    sub_f = torch.empty((max(N, 1), fdim), dtype=torch.float32, device=dev) if fdim else None
    sub_c = torch.empty((max(N, 1), ldim), dtype=torch.int32, device=dev) if ldim else None
    sub_l = torch.empty((B,), dtype=torch.int32, device=dev)
    status = (ctypes.c_int * (B + 2))()
    nbytes = lib.d3f_grid_subsample_workspace_bytes(N, B, fdim, ldim)
    ws = workspace(nbytes, dev)
    with _timed("grid_subsample", dict(N=N, M=None), dev) as tm:
        rc = lib.d3f_batch_grid_subsample(points.data_ptr(), N, lens_t.data_ptr(), B, float(dl),
                                          features.data_ptr() if fdim else None, fdim,
                                          classes.data_ptr() if ldim else None, ldim,
                                          sub_p.data_ptr(), sub_f.data_ptr() if fdim else None,
                                          sub_c.data_ptr() if ldim else None, sub_l.data_ptr(),
                                          ctypes.addressof(status), ws.data_ptr(), ws.numel(), _stream(dev))
        tm.info["M"] = int(status[0])
    _lib.check(rc, "batch_grid_subsample")
    M = _raise_flags(status[1], "batch_grid_subsample") or status[0]
    sub_l.host_lens = [int(status[2 + b]) for b in range(B)]
    return sub_p[:M], sub_l, (sub_f[:M] if fdim else None), (sub_c[:M] if ldim else None)


def batch_grid_subsample_async(points, lens, dl, m_cap, status=None, m_hint=0, elem_cap=0, elem_points=0, clouds=None, n_cap=0,
                               bbox_in=None, bbox_out=None):
    """Capacity mode of batch_grid_subsample (points only): no host synchronisation.
    clouds (device int64[B]: the ADDRESS of every cloud's own f32[len, 3] array) with points=None and n_cap = bound of sum(lens):
    the clouds are read in place, nothing is stacked (d3f_batch_grid_subsample_async_inplace).
    points f32[N_cap,3] (sum(lens) rows valid) -> (sub_points f32[m_cap,3] tagged with n_dev, sub_lens i32[B] device,
    status i32[2] device = [M, flags]).  elem_cap: capacity of ONE cloud of the stack (0: m_cap); a cloud above it raises
    the overflow flag like a stack above m_cap does.  elem_points: capacity of one cloud in POINTS (0: all rows of `points`);
    at most 16384 selects the one-workgroup-per-cloud form (the coarse pyramid levels: 2 launches instead of ~25).
    bbox_in / bbox_out (device i32[B, 6], GridChain.box): finished boxes of the input clouds (the sort form then skips its boxing
    pass) / where the boxes of the written clouds are accumulated (d3f_batch_grid_subsample_async_boxed)."""
    lib = _lib.load()
    if clouds is not None:
        assert points is None and clouds.dtype == torch.int64 and clouds.is_contiguous() and int(n_cap) > 0
        dev, N = clouds.device, int(n_cap)
    else:
        points = _req(points, torch.float32, "points", 2).contiguous()
        dev = points.device
        N = points.shape[0]
    lens_t = as_lens(lens, dev)
    B = lens_t.numel()
    sub_p = torch.empty((int(m_cap), 3), dtype=torch.float32, device=dev)
    sub_l = torch.empty((B,), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((2,), dtype=torch.int32, device=dev)
    nbytes = lib.d3f_grid_subsample_workspace_bytes(N, B, 0, 0)
    ws = workspace(nbytes, dev)
    with _timed("grid_subsample", dict(N=N, M=int(m_cap)), dev):
        if bbox_in is not None or bbox_out is not None:
            assert all(b is None or (b.dtype == torch.int32 and b.is_contiguous() and b.numel() == 6 * B) for b in (bbox_in, bbox_out))
            assert clouds is None or clouds.numel() == B
            rc = lib.d3f_batch_grid_subsample_async_boxed(_ptr(points), _ptr(clouds), N, lens_t.data_ptr(), B, float(dl),
                                                          sub_p.data_ptr(), int(m_cap), int(elem_cap), int(elem_points),
                                                          sub_l.data_ptr(), status.data_ptr(), _ptr(bbox_in), _ptr(bbox_out),
                                                          ws.data_ptr(), ws.numel(), _stream(dev))
        elif clouds is not None:
            assert clouds.numel() == B
            rc = lib.d3f_batch_grid_subsample_async_inplace(clouds.data_ptr(), N, lens_t.data_ptr(), B, float(dl), sub_p.data_ptr(),
                                                            int(m_cap), int(elem_cap), sub_l.data_ptr(), status.data_ptr(),
                                                            ws.data_ptr(), ws.numel(), _stream(dev))
        else:
            rc = lib.d3f_batch_grid_subsample_async(points.data_ptr(), N, lens_t.data_ptr(), B, float(dl), sub_p.data_ptr(),
                                                    int(m_cap), int(elem_cap), int(elem_points), sub_l.data_ptr(), status.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "batch_grid_subsample_async")
    sub_p.n_dev = status[0:1]
    sub_p.n_hint = int(m_hint)
    return sub_p, sub_l, status


def pack_status(dst, blocks, clear=None):
    """dst i32[>= sum of the blocks' sizes] <- the (up to four) device int32 blocks one after the other, then the FLAG column of
    `clear` (a device int32 [k, 2] tensor of [kmax-or-size | flags] pairs, may be one of the blocks) zeroed -- the size words stay
    readable after the replay: one launch (d3f_pack_status) instead of a copy node per block and a fill."""
    lib = _lib.load()
    # contiguity is checked on the CALLER's tensors: the launch may be captured in a HIP graph with these addresses, and a silent
    # copy (reshape of a strided view) would hand the graph a temporary that is freed when this call returns
    assert 1 <= len(blocks) <= 4 and all(b.dtype == torch.int32 and b.is_contiguous() for b in blocks) and dst.dtype == torch.int32
    assert dst.is_contiguous()
    blocks = [b.view(-1) for b in blocks]
    assert dst.numel() >= sum(b.numel() for b in blocks)
    args = []
    for i in range(4):
        args += [blocks[i].data_ptr(), blocks[i].numel()] if i < len(blocks) else [None, 0]
    if clear is not None:
        assert clear.dtype == torch.int32 and clear.is_contiguous() and clear.dim() == 2 and clear.shape[1] == 2
    _lib.check(lib.d3f_pack_status(dst.data_ptr(), *args, _ptr(clear),
                                   clear.shape[0] if clear is not None else 0, 1, 2, _stream(dst.device)), "pack_status")
    return dst


def stack_self_pair(pts, lens=None, bbox_in=None, bbox_out=None):
    """np.concatenate([c, c]) for every cloud c of a stack whose row counts live on the device:
    pts f32[cap,3] holding B clouds (lens i32[B] on the device; default: one cloud of pts.n_dev rows)
    -> (out f32[2*cap,3] = [c_0; c_0; c_1; c_1; ...] tagged with n_dev, lens_out i32[2B]).
    bbox_in (device i32[B, 6]: the finished boxes of the input clouds) -> bbox_out (device i32[2B, 6]): a box per written cloud."""
    lib = _lib.load()
    pts = _req(pts, torch.float32, "pts", 2).contiguous()
    dev = pts.device
    cap = pts.shape[0]
    if lens is None:
        lens = getattr(pts, "n_dev", None)
        if lens is None:
            lens = torch.full((1,), cap, dtype=torch.int32, device=dev)
    B = lens.numel()
    out = torch.empty((2 * cap, 3), dtype=torch.float32, device=dev)
    lens_out = torch.empty((2 * B,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    if bbox_out is not None:
        assert bbox_out.dtype == torch.int32 and bbox_out.is_contiguous() and bbox_out.numel() == 12 * B
        assert bbox_in is not None and bbox_in.dtype == torch.int32 and bbox_in.is_contiguous() and bbox_in.numel() == 6 * B
        rc = lib.d3f_stack_self_pair_boxed(pts.data_ptr(), cap, lens.data_ptr(), B, out.data_ptr(), lens_out.data_ptr(),
                                           total.data_ptr(), bbox_in.data_ptr(), bbox_out.data_ptr(), _stream(dev))
    else:
        rc = lib.d3f_stack_self_pair(pts.data_ptr(), cap, lens.data_ptr(), B, out.data_ptr(), lens_out.data_ptr(),
                                     total.data_ptr(), _stream(dev))
    _lib.check(rc, "stack_self_pair")
    out.n_dev = total
    out.n_hint = 2 * int(getattr(pts, "n_hint", 0) or 0)
    return out, lens_out


# Neighbour grids built from boxes that the kernels writing the clouds gathered (D3F_GRID_BOXED=0: every grid boxes its cloud
# itself, d3f_neighbor_grid_build -- the five-launch build throughout).
GRID_BOXED = os.environ.get("D3F_GRID_BOXED", "1") != "0"


class GridChain:
    """The static memory of one replay's boxed grid builds: a box block i32[B, 6] and a grid object per pyramid level (rows[l]
    support rows, B clouds), one more box block for the clouds a self-pair is stacked from (`pre`), and the ONE reset launch that precedes the geometry chain (d3f_geometry_reset): initial values of
    every box, cleared counters of every large-form grid.  boxed[l] False: level l's cloud has no producer in the sequence, its
    grid is built by d3f_neighbor_grid_build."""

    def __init__(self, rows, B, device, boxed=None):
        lib = _lib.load()
        self.rows, self.B = [int(r) for r in rows], int(B)
        self.boxed = list(boxed) if boxed is not None else [True] * len(self.rows)
        assert len(self.rows) <= _lib.GRID_RESET_MAX and len(self.boxed) == len(self.rows)
        self.boxes = torch.zeros((len(self.rows) + 1, self.B, 6), dtype=torch.int32, device=device)
        self.pre = self.boxes[len(self.rows)]
        self.nbytes = [lib.d3f_neighbor_grid_bytes(r, self.B) for r in self.rows]
        self.mems = [torch.empty((n,), dtype=torch.uint8, device=device) for n in self.nbytes]
        self.forms = [lib.d3f_neighbor_grid_boxed_form(r, self.B) if on else 0 for r, on in zip(self.rows, self.boxed)]

    def box(self, level):
        return self.boxes[level]

    def reset(self):
        import ctypes
        lib = _lib.load()
        ks = [k for k, on in enumerate(self.boxed) if on]
        n = len(ks)
        grids = (ctypes.c_void_p * max(n, 1))(*[self.mems[k].data_ptr() for k in ks])
        nbytes = (ctypes.c_size_t * max(n, 1))(*[self.nbytes[k] for k in ks])
        rows = (ctypes.c_int * max(n, 1))(*[self.rows[k] for k in ks])
        Bs = (ctypes.c_int * max(n, 1))(*([self.B] * n))
        rc = lib.d3f_geometry_reset(self.boxes.data_ptr(), self.boxes.numel() // 6, ctypes.addressof(grids), ctypes.addressof(nbytes),
                                    ctypes.addressof(rows), ctypes.addressof(Bs), n, _stream(self.boxes.device))
        _lib.check(rc, "geometry_reset")


class NeighborGrid:
    """Cell grid over a stacked support cloud (see d3f_neighbor_grid_build); owns its device memory.
    chain / level: build from the finished boxes of GridChain level `level`, inside the chain's memory
    (d3f_neighbor_grid_build_boxed; the chain's reset launch and the producer of `supports` have run on this stream)."""

    def __init__(self, supports, s_lens, radius, chain=None, level=0):
        lib = _lib.load()
        if chain is not None and chain.boxed[level]:
            self._init_boxed(lib, supports, s_lens, radius, chain, level)
            self._views(lib)
            return
        self.supports = _tag(_req(supports, torch.float32, "supports", 2).contiguous(), supports)
        dev = self.supports.device
        self.Ns = self.supports.shape[0]
        self.s_lens = as_lens(s_lens, dev)
        self.B = self.s_lens.numel()
        self.radius = float(radius)
        self.nbytes = lib.d3f_neighbor_grid_bytes(self.Ns, self.B)
        self.mem = torch.empty((self.nbytes,), dtype=torch.uint8, device=dev)
        with _timed("nb_grid_build", dict(Ns=self.Ns), dev):
            rc = lib.d3f_neighbor_grid_build(self.supports.data_ptr(), self.Ns, self.s_lens.data_ptr(), self.B, self.radius,
                                             self.mem.data_ptr(), self.nbytes, _stream(dev))
        _lib.check(rc, "neighbor_grid_build")
        self._views(lib)

    def _init_boxed(self, lib, supports, s_lens, radius, chain, level):
        self.supports = _tag(_req(supports, torch.float32, "supports", 2).contiguous(), supports)
        dev = self.supports.device
        self.Ns = self.supports.shape[0]
        self.s_lens = as_lens(s_lens, dev)
        self.B = self.s_lens.numel()
        self.radius = float(radius)
        if self.Ns != chain.rows[level] or self.B != chain.B:
            raise ValueError("grid chain level %d was laid out for %d rows / %d clouds, not %d / %d"
                             % (level, chain.rows[level], chain.B, self.Ns, self.B))
        self.nbytes, self.mem = chain.nbytes[level], chain.mems[level]
        self.form = chain.forms[level]
        with _timed("nb_grid_build", dict(Ns=self.Ns), dev):
            rc = lib.d3f_neighbor_grid_build_boxed(self.supports.data_ptr(), self.Ns, self.s_lens.data_ptr(), self.B, self.radius,
                                                   chain.box(level).data_ptr(), self.mem.data_ptr(), self.nbytes, _stream(dev))
        _lib.check(rc, "neighbor_grid_build_boxed")

    def _views(self, lib):
        dev = self.supports.device
        # support indices sorted by cell (a view into the grid object): a spatially coherent visiting order
        off = lib.d3f_neighbor_grid_order_offset(self.Ns, self.B)
        self.order = self.mem[off: off + 4 * max(self.Ns, 1)].view(torch.int32)
        # the level in the INTERNAL (cell-sorted) numbering: position of every support in cell order, and the supports in that order
        off = lib.d3f_neighbor_grid_inv_offset(self.Ns, self.B)
        self.inv = self.mem[off: off + 4 * max(self.Ns, 1)].view(torch.int32)
        off = lib.d3f_neighbor_grid_xyz_offset(self.Ns, self.B)
        self.xyz = self.mem[off: off + 12 * max(self.Ns, 1)].view(torch.float32).view(-1, 3)
        for a in ("n_dev", "n_hint"):
            if getattr(self.supports, a, None) is not None:
                setattr(self.xyz, a, getattr(self.supports, a))

    def search(self, queries, q_lens, width, ld=None, pad_value=None, cap=192, first_only=False, out=None, status=None,
               reset_status=True, want_kmax=True, nn_hint=0.0, query_grid=None, internal=False):
        """-> (out i32[Nq, ld], status i32[2] device tensor); no synchronisation.  reset_status=False: the caller has
        zeroed `status` (saves one launch per search).  want_kmax=False: status[0] (largest neighbour count) is not maintained
        (callers that allocate a fixed number of columns do not need it; see D3F_NB_NO_KMAX).  nn_hint (first_only): the distance
        within which the caller expects the nearest support -- a speed hint only, see include/d3feat_amd.h.
        query_grid: a NeighborGrid built over `queries` themselves (or this grid when the queries are its supports) -- its cell order
        becomes the visiting order (d3f_neighbor_grid_search_ordered); results do not depend on it.
        internal=True (needs query_grid): the INTERNAL numbering -- row j belongs to the j-th query of query_grid's cell order and
        the entries are positions in this grid's cell order (self.inv) instead of indices; pad_value is written as is."""
        lib = _lib.load()
        queries = _req(queries, torch.float32, "queries", 2).contiguous()
        dev = queries.device
        Nq = queries.shape[0]
        ql = as_lens(q_lens, dev)
        if ql.numel() != self.B:
            raise ValueError("q_batches and s_batches must have the same number of elements")
        ld = int(ld if ld is not None else width)
        if out is None:
            out = torch.empty((Nq, ld), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty((2,), dtype=torch.int32, device=dev)
        same = 1 if (queries.data_ptr() == self.supports.data_ptr() and Nq == self.Ns) else 0
        if pad_value is None:
            # BatchOrderedNeighbors pads with the number of supports: known only on the device in capacity mode
            pad_value = _lib.PAD_NUM_SUPPORTS if getattr(self.supports, "n_dev", None) is not None else self.Ns
        if query_grid is not None:
            if query_grid.Ns != Nq or query_grid.B != self.B or query_grid.supports.data_ptr() != queries.data_ptr():
                raise ValueError("query_grid was not built over these queries")
            with _timed("nb_search", dict(Nq=Nq, Ns=self.Ns, width=int(width), first_only=int(bool(first_only))), dev):
                rc = lib.d3f_neighbor_grid_search_ordered(self.mem.data_ptr(), self.nbytes, self.Ns, queries.data_ptr(), Nq, ql.data_ptr(),
                                                          self.B, self.radius, query_grid.mem.data_ptr(), query_grid.nbytes,
                                                          out.data_ptr(), ld, int(width), int(pad_value), int(cap),
                                                          1 if first_only else 0, float(nn_hint),
                                                          (1 if reset_status else 0) | (0 if want_kmax else 2) | (4 if internal else 0),
                                                          status.data_ptr(), _stream(dev))
            _lib.check(rc, "neighbor_grid_search_ordered")
            o = getattr(queries, "order", None)
            if o is not None and not internal:
                out.order = o
            return _tag(out, queries), status
        if internal:
            raise ValueError("internal numbering needs the queries' grid")
        with _timed("nb_search", dict(Nq=Nq, Ns=self.Ns, width=int(width), first_only=int(bool(first_only))), dev):
            rc = lib.d3f_neighbor_grid_search(self.mem.data_ptr(), self.nbytes, self.Ns, queries.data_ptr(), Nq,
                                              ql.data_ptr(), self.B, self.radius, same, out.data_ptr(), ld, int(width),
                                              int(pad_value), int(cap),
                                              1 if first_only else 0, float(nn_hint),
                                              (1 if reset_status else 0) | (0 if want_kmax else 2),
                                              status.data_ptr(),
                                              _stream(dev))
        _lib.check(rc, "neighbor_grid_search")
        o = getattr(queries, "order", None)
        if o is not None:
            out.order = o         # rows of the index matrix = the queries: same visiting order
        return _tag(out, queries), status


def batch_radius_neighbors(queries, supports, q_lens, s_lens, radius, width, ld=None, out=None, pad_value=None, cap=192,
                           first_only=False):
    """Build + search; -> (out i32[Nq, ld] with `width` valid columns, status i32[2] device tensor).
    No synchronisation: status[0] = Kmax, status[1] = flags (see check_status)."""
    grid = NeighborGrid(supports, s_lens, radius)
    return grid.search(queries, q_lens, width, ld=ld, pad_value=pad_value, cap=cap, first_only=first_only, out=out)


class StackGroups:
    """Stands in for the `in_batches` matrix (datasets/common.py:453-496) on the fast path, where the head kernel works from
    the stack lengths: `group` = clouds per reference stack inside a batched stack (see d3f_detect_head)."""

    def __init__(self, group=0):
        self.group = int(group)


_KP_HOST = {}


def _kp_host(K_points):
    """Kernel points as a contiguous host float32 array (they ride in the kernel arguments).  The model keeps them on the
    host; a caller-supplied device tensor is read back once per (storage, version), not once per call."""
    if isinstance(K_points, torch.Tensor):
        key = (K_points.data_ptr(), K_points._version, tuple(K_points.shape))
        hit = _KP_HOST.get(key)
        if hit is None:
            if len(_KP_HOST) > 256:
                _KP_HOST.clear()
            # the entry keeps the tensor alive: its address cannot be handed to another tensor while the key is in use
            hit = _KP_HOST[key] = (K_points, np.ascontiguousarray(K_points.detach().cpu().numpy(), dtype=np.float32))
        return hit[1]
    return np.ascontiguousarray(K_points, dtype=np.float32)


_INFLUENCE = {"constant": 0, "linear": 1, "gaussian": 2}
_AGGREGATION = {"sum": 0, "closest": 1}


# ---- bf16-operand contractions (BASELINE configs[4]) -------------------------------------------------------------------------
# Off by default: the fp32 path is the parity path.  `with bf16_contraction():` routes every contraction issued inside it (the
# engine wraps its capture in it when built with bf16=True) through d3f_gemm_bf16.
BF16_CONTRACTION = False


BF16_FEATURES = False     # bf16 feature STORAGE (needs BF16_CONTRACTION): activations live in HBM as torch.bfloat16
F32_OUTPUT = False        # inside bf16 feature storage: the next contractions write float32 (the descriptor head's input)


class bf16_contraction:
    """BASELINE configs[4].  on: every unary / unfused KPConv contraction multiplies bf16 operands (fp32 accumulate).
    features=True additionally STORES the activations between the layers as bfloat16 (KPConv gathers, max pooling, the
    decoder gather and every contraction then move half the bytes; arithmetic inside the kernels stays fp32)."""

    def __init__(self, on=True, features=False):
        self.on, self.features = bool(on), bool(on) and bool(features)

    def __enter__(self):
        global BF16_CONTRACTION, BF16_FEATURES
        self.prev, BF16_CONTRACTION = BF16_CONTRACTION, self.on
        self.prevf, BF16_FEATURES = BF16_FEATURES, self.features
        return self

    def __exit__(self, *exc):
        global BF16_CONTRACTION, BF16_FEATURES
        BF16_CONTRACTION, BF16_FEATURES = self.prev, self.prevf
        return False


class f32_output:
    """Contractions inside this context write float32 even under bf16 feature storage (last_unary: descriptors / scores are
    computed from fp32 values)."""

    def __enter__(self):
        global F32_OUTPUT
        self.prev, F32_OUTPUT = F32_OUTPUT, True
        return self

    def __exit__(self, *exc):
        global F32_OUTPUT
        F32_OUTPUT = self.prev
        return False


def _feat(t, name, ndim=None):
    """A feature tensor: float32, or bfloat16 under bf16 feature storage."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
        return _req(t, torch.bfloat16, name, ndim)
    return _req(t, torch.float32, name, ndim)


def _h(t):
    return 1 if (t is not None and t.dtype == torch.bfloat16) else 0


def _out_dtype():
    """dtype of a contraction's output."""
    return torch.bfloat16 if (BF16_CONTRACTION and BF16_FEATURES and not F32_OUTPUT) else torch.float32


def _packed_on_tensor(W, slot, make):
    """A packed copy of a weight tensor that LIVES AND DIES WITH THE WEIGHT TENSOR: the copy rides on the tensor object that owns
    the storage (the view's base), keyed by the view's offset / shape / strides and the tensor's version.  (A global cache with
    eviction would free copies that captured graphs still read: round 4 found exactly that -- an engine's replays computed with
    another model's packed weights once 512 entries had gone through the cache.)"""
    base = W._base if W._base is not None else W
    store = getattr(base, slot, None)
    if store is None:
        store = {}
        setattr(base, slot, store)
    key = (W.storage_offset(), tuple(W.shape), tuple(W.stride()))
    hit = store.get(key)
    if hit is None:
        hit = store[key] = [base._version, make(None)]
    elif hit[0] != base._version:
        # the weight was updated in place: re-pack INTO THE SAME BUFFER.  A captured graph holds the packed copy's address; a fresh
        # allocation here would free memory that its replays still read (ADVICE r04 / VERDICT r05 item 8a) -- this way the replays
        # simply see the new values (tests/test_gpu_engine.py::test_in_place_weight_update_reaches_a_captured_engine)
        make(hit[1])
        hit[0] = base._version
    return hit[1]


def refresh_packed_weights(tensors):
    """Re-pack (in place, same addresses) every packed copy that rides on one of `tensors` and is older than its tensor.
    The packed copies are made by the EAGER ops; a caller that updates weights in place and then only REPLAYS captured graphs
    calls this once after the update (FragmentEngine.refresh_weights does)."""
    n = 0
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            continue
        base = t._base if t._base is not None else t
        for slot, fn in _PACKERS:
            for (off, shape, strides), hit in list((getattr(base, slot, None) or {}).items()):
                if hit[0] != base._version:
                    fn(base.as_strided(shape, strides, off))
                    n += 1
    return n


def _packed_weights(W, slot, alloc, pack, what):
    """W f32[K,N] (contiguous rows) -> its packed copy: alloc(K, N) makes the buffer, pack(W, ldb, K, N, buffer, stream) fills it."""
    def make(t):
        K, N = W.shape
        if t is None:
            t = alloc(K, N)
        _lib.check(pack(W.data_ptr(), int(W.stride(0)), K, N, t.data_ptr(), _stream(W.device)), what)
        return t
    return _packed_on_tensor(W, slot, make)


def packed_bf16_weights(W):
    """W f32[K,N] (contiguous rows) -> the bf16 [N][Kp] copy d3f_gemm_bf16 reads; made once per (weight tensor, view, version)."""
    return _packed_weights(W, "_d3f_bf16t", lambda K, N: torch.empty((N, (K + 31) // 32 * 32), dtype=torch.int16, device=W.device),
                           _lib.load().d3f_gemm_pack_bf16, "gemm_pack_bf16")


def packed_f32t_weights(W):
    """W f32[K,N] (contiguous rows) -> the transposed, K-padded f32 [N][Kp] copy d3f_gemm_f32t reads (LDS-DMA copies 16
    contiguous bytes per lane: it cannot transpose); made once per (weight tensor, view, version) -- at a model's first eager
    use, i.e. the engine's warm-up, never inside a captured graph."""
    return _packed_weights(W, "_d3f_f32t", lambda K, N: torch.empty((N, (K + 31) // 32 * 32), dtype=torch.float32, device=W.device),
                           _lib.load().d3f_gemm_pack_f32t, "gemm_pack_f32t")


# The operand-split form (d3f_gemm_x3: exact 3 x bf16 split of both fp32 operands, six bf16 MFMA products per fp32 product, fp32
# accumulate -- fp32 in, fp32 out, fp32-grade error; csrc/gemm_x3.h) takes every contraction it can address; D3F_GEMM_X3=0 keeps
# them all on the fp32 MFMA kernel.
GEMM_X3 = os.environ.get("D3F_GEMM_X3", "1") != "0"


def packed_x3_weights(W):
    """W f32[K,N] (contiguous rows) -> the pre-split bf16 planes d3f_gemm_x3 stages ([column group][k-tile][plane][32][40]); made
    once per (weight tensor, view, version), like the transposed fp32 copy."""
    lib = _lib.load()
    return _packed_weights(W, "_d3f_x3", lambda K, N: torch.empty((int(lib.d3f_gemm_x3_packed_bytes(K, N)) // 2,), dtype=torch.int16,
                                                                  device=W.device), lib.d3f_gemm_pack_x3, "gemm_pack_x3")


X3_MAX_ROWS = 65535 * 128      # d3f_gemm_x3's grid holds 65535 row tiles of (at least) 128 rows; beyond: the fp32 kernel


def _x3_resident(M, N, K, hint):
    """Does d3f_gemm_x3 take its resident-W persistent form for this call?  (The library's own predicate.)"""
    return bool(_lib.load().d3f_gemm_x3_resident(M, N, K, hint))


def _x3_ok(C1, C2, N, rows=0):
    """d3f_gemm_x3 can address the call (K and a concatenation's first part multiples of 32) and is the faster kernel for it.  The
    32-column layers (level-0 unary blocks, memory bound) are slower on its tile form than on the fp32 MFMA kernel (70.9 against
    83.6 us at M = 707592, K = 64: r04 x6) but faster on the resident-W persistent form of round 5, which the library takes when
    d3f_gemm_x3_resident says so for `rows` (70.6 / 105.8 us against 72-82 / 118.6 at M = 707592, 23 / 31 against 28 / 39 at
    M = 235864: r05 g3)."""
    fits = GEMM_X3 and (C1 + C2) % 32 == 0 and (C2 == 0 or C1 % 32 == 0)
    return fits and (N > 32 or _x3_resident(rows, N, C1 + C2, 0))


def _route(M, plain, bf16, bf16_ok, f32t_ok, x3, resident):
    """-> (entry point, record name) of a contraction of M rows.  plain: no gathered or concatenated operand; bf16: BF16_CONTRACTION;
    bf16_ok / f32t_ok: d3f_gemm_bf16 / d3f_gemm_f32t can address the operands (alignment, leading dimensions); x3: _x3_ok of the
    call; resident: d3f_gemm_x3_resident of the call.  The record name tells bench.py's per-family tables which form of d3f_gemm_x3
    runs: the resident form is a streaming kernel, bound by HBM, not by the matrix pipe."""
    if bf16 and bf16_ok:
        return "d3f_gemm_bf16", "gemm_bf16"
    if not f32t_ok:
        return ("d3f_gemm_f32" if plain else "d3f_gemm_upsample_cat_f32"), "gemm_f32"
    if x3 and M <= X3_MAX_ROWS:
        return "d3f_gemm_x3", "gemm_x3r" if resident else "gemm_x3"
    return "d3f_gemm_f32t", "gemm_f32"


def _f32t_ok(N, ldc, out, residual, ldr, vectors, *operands):
    """Can d3f_gemm_f32t address this call?  (every shape of the network can)"""
    if N % 4 or ldc % 4 or out.data_ptr() % 16:
        return False
    if residual is not None and (ldr % 4 or residual.data_ptr() % 16):
        return False
    if any(v is not None and v.data_ptr() % 16 for v in vectors):
        return False
    for t, ld, cols in operands:
        if t is not None and (cols % 4 or ld % 4 or t.data_ptr() % 16 or cols < 4):
            return False
    return True


def _bf16_ok(*operands):
    """(tensor, leading dimension, columns) triples: float4-addressable?"""
    for t, ld, cols in operands:
        if t is None:
            continue
        if cols % 4 or ld % 4 or t.data_ptr() % (8 if t.dtype == torch.bfloat16 else 16):
            return False
    return True


def _contract(what, A, N1, lda, C1, idx, ld_idx, skip, lds, C2, W, ldb, out, ldc, m_dev, n1_dev, hint, row_scale=None, col_scale=None,
              col_shift=None, residual=None, ldr=0, leaky=False, alpha=0.2):
    """out = act(([ A[idx[:,0]] (A itself when idx is None) | skip ] @ W) * row_scale[:,None] * col_scale + col_shift + residual):
    picks the kernel (_route) and launches it.  W f32[C1 + C2, N] with contiguous rows (ldb)."""
    lib = _lib.load()
    (M, N), K, dev = out.shape, C1 + C2, out.device
    operands = ((A, lda, C1), (skip, lds, C2))
    entry, name = _route(M, idx is None and skip is None, BF16_CONTRACTION,
                         K >= 4 and ldc == N and W.is_contiguous() and _bf16_ok(*operands),
                         W.is_contiguous() and _f32t_ok(N, ldc, out, residual, ldr, (col_scale, col_shift), *operands),
                         _x3_ok(C1, C2, N, hint if 0 < hint < M else M), _x3_resident(M, N, K, hint))
    if entry != "d3f_gemm_bf16" and (_h(A) or _h(skip) or _h(out)):
        raise TypeError("%s: bfloat16 operands that the bf16 contraction cannot address (K %d, lda %d)" % (what, K, lda))
    flags = [1 if leaky else 0, float(alpha)]
    if entry == "d3f_gemm_f32":
        ws = workspace(lib.d3f_gemm_workspace_bytes(M, N, K, hint), dev)
        args = [A.data_ptr(), lda, W.data_ptr(), ldb, out.data_ptr(), ldc, M, N, K, _ptr(row_scale), _ptr(col_scale), _ptr(col_shift),
                _ptr(residual), ldr] + flags + [ws.data_ptr(), ws.numel(), m_dev, hint]
    else:
        head = [A.data_ptr(), N1, lda, C1, _ptr(idx), ld_idx, _ptr(skip), lds, C2]
        if entry == "d3f_gemm_upsample_cat_f32":
            ws = workspace(lib.d3f_gemm_workspace_bytes(M, N, K, hint), dev)
            args = head + [W.data_ptr(), ldb, out.data_ptr(), ldc, M, N, _ptr(col_scale), _ptr(col_shift)] + flags
        else:
            pack, ws_bytes = {"d3f_gemm_bf16": (packed_bf16_weights, lib.d3f_gemm_bf16_workspace_bytes),
                              "d3f_gemm_f32t": (packed_f32t_weights, lib.d3f_gemm_workspace_bytes),
                              "d3f_gemm_x3": (packed_x3_weights, lib.d3f_gemm_x3_workspace_bytes)}[entry]
            Wp = pack(W)
            # (the bf16 launcher plans its K split for a 64-column tile even when N <= 32: its own function sizes the slab)
            ws = workspace(ws_bytes(M, N, K, hint), dev)
            args = head + [Wp.data_ptr(), out.data_ptr(), ldc, M, N, _ptr(row_scale), _ptr(col_scale), _ptr(col_shift), _ptr(residual),
                           ldr] + flags
        args += [ws.data_ptr(), ws.numel(), m_dev, n1_dev, hint]
    if entry == "d3f_gemm_bf16":
        if out.data_ptr() % 16 or (residual is not None and (residual.data_ptr() % 8 or ldr % 4)):
            raise ValueError("gemm (bf16): output / residual must be 16 / 8-byte aligned with a leading dimension of 4 k")
        args += [_h(A), _h(out)]
    with _timed(name, dict(M=M, N=N, K=K), dev):
        rc = getattr(lib, entry)(*args, _stream(dev))
    _lib.check(rc, entry[4:])


def gemm(A, Bm, row_scale=None, col_scale=None, col_shift=None, residual=None, leaky=False, alpha=0.2, out=None):
    """out = act((A @ Bm) * row_scale[:,None] * col_scale + col_shift + residual) on the matrix cores."""
    A, lda = _rows(_feat(A, "A"), "A")
    Bm, ldb = _rows(_req(Bm, torch.float32, "B"), "B")
    M, K = A.shape
    if Bm.shape[0] != K:
        raise ValueError("gemm: A is %s, B is %s" % (tuple(A.shape), tuple(Bm.shape)))
    N = Bm.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=_out_dtype(), device=A.device)
    out, ldc = _rows(out, "out")
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(_feat(residual, "residual"), "residual")
    if (_h(A) or _h(out) or _h(residual)) and not (BF16_CONTRACTION and (residual is None or _h(residual) == _h(A))):
        raise TypeError("gemm: bfloat16 feature tensors need ops.bf16_contraction(features=True)")
    for v, n, name in ((row_scale, M, "row_scale"), (col_scale, N, "col_scale"), (col_shift, N, "col_shift")):
        if v is not None:
            _req(v, torch.float32, name)
            if v.numel() != n or not v.is_contiguous():
                raise ValueError("%s must be a contiguous vector of %d" % (name, n))
    _contract("gemm", A, M, lda, K, None, 0, None, 0, 0, Bm, ldb, out, ldc, _nd(A), None, int(getattr(A, "n_hint", 0) or 0),
              row_scale, col_scale, col_shift, residual, ldr, leaky, alpha)
    return _tag(out, A)


class UpsampleCat:
    """The not-yet-materialised result of nearest_upsample + skip concatenation (models/D3Feat.py:55-63):
    rows [ x'[inds[n,0]] | skip[n] ].  The unary block that follows consumes it through gemm_upsample_cat (one launch, no
    intermediate tensor); anything else calls .materialize()."""

    def __init__(self, x, inds, skip=None):
        self.x, self.inds, self.skip = x, inds, skip
        self.shape = (inds.shape[0], x.shape[1] + (skip.shape[1] if skip is not None else 0))
        self.device = x.device
        _tag(self, inds)

    def materialize(self):
        return closest_pool_cat(self.x, self.inds, self.skip)


def gemm_upsample_cat(u, W, col_scale=None, col_shift=None, leaky=False, alpha=0.2):
    """out = act(([ x'[inds[:,0]] | skip ] @ W) * col_scale + col_shift) without building the concatenation."""
    x, ldx = _rows(_feat(u.x, "x"), "x")
    inds, ldi = _rows(_req(u.inds, torch.int32, "inds"), "inds")
    W, ldb = _rows(_req(W, torch.float32, "W"), "W")
    C1, C2, lds, skip = x.shape[1], 0, 0, None
    if u.skip is not None:
        skip, lds = _rows(_feat(u.skip, "skip"), "skip")
        C2 = skip.shape[1]
    M, N = inds.shape[0], W.shape[1]
    if W.shape[0] != C1 + C2:
        raise ValueError("gemm_upsample_cat: W has %d rows, operands %d + %d columns" % (W.shape[0], C1, C2))
    if C2 and (C1 % 4 or lds % 4 or skip.data_ptr() % 16) and not _h(x):
        return gemm(u.materialize(), W, col_scale=col_scale, col_shift=col_shift, leaky=leaky, alpha=alpha)
    out = torch.empty((M, N), dtype=_out_dtype(), device=x.device)
    _contract("gemm_upsample_cat", x, x.shape[0], ldx, C1, inds, ldi, skip, lds, C2, W, ldb, out, N, _nd(inds), _nd(x),
              int(getattr(inds, "n_hint", 0) or 0), col_scale=col_scale, col_shift=col_shift, leaky=leaky, alpha=alpha)
    return _tag(out, inds)


# The decoder's unary blocks in split form (D3F_DECODER_SPLIT=0: the one-launch form above throughout).  The upsampled half of
# [ x'[inds[:,0]] | skip ] is a nearest-neighbour gather from a level with about a quarter of the rows, so the one-launch form
# multiplies -- and splits into bf16 planes -- every coarse row about four times.  The split form contracts it ONCE per coarse row,
# Y = x @ W[:C1], and the fine level computes skip @ W[C1:] and adds the gathered row Y[inds[m, 0]] in its epilogue (d3f_gemm_x3_gres).
DECODER_SPLIT = os.environ.get("D3F_DECODER_SPLIT", "1") != "0"


def _split_ok(M, C1, C2, N, hint=0, f32=True, f32t_ok=True):
    """Is a decoder contraction of M rows ([C1 gathered | C2 skip] columns -> N) taken in the split form?  fp32 only, with a skip
    operand, both parts whole k-tiles, and only where the one-launch call would run gemm_x3_kernel: the resident form's launch (level
    0) is bound by HBM, and halving its K does not change its bytes."""
    if not DECODER_SPLIT or BF16_CONTRACTION or not f32 or C2 <= 0 or C1 <= 0 or C1 % 32 or C2 % 32:
        return False
    resident = _x3_resident(M, N, C1 + C2, hint)
    entry, _ = _route(M, False, False, False, f32t_ok, _x3_ok(C1, C2, N, hint if 0 < hint < M else M), resident)
    return entry == "d3f_gemm_x3" and not resident


def upsample_split_ok(u, N):
    """_split_ok of the decoder block that consumes the UpsampleCat `u` with N output columns."""
    if u.skip is None or u.x.dim() != 2 or u.skip.dim() != 2 or u.inds.dim() != 2:
        return False
    f32 = u.x.dtype == torch.float32 and u.skip.dtype == torch.float32
    aligned = all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (u.x, u.skip))
    return _split_ok(u.inds.shape[0], u.x.shape[1], u.skip.shape[1], N, int(getattr(u.inds, "n_hint", 0) or 0), f32, aligned and N % 4 == 0)


def gemm_upsample_split(u, W1, W2, col_shift=None, leaky=False, alpha=0.2, out=None):
    """out = act(x'[inds[:,0]] @ W1 + skip @ W2 + col_shift) in two launches: Y = x @ W1 over the COARSE rows, then
    act(skip @ W2 + col_shift + Y[inds[:,0]]) over the fine ones (an index outside x's rows adds zeros: the zero row of x').  A
    per-column scale is folded into W1 / W2 by the caller (VariableStore.split_decoder).  Only where upsample_split_ok holds."""
    lib = _lib.load()
    x, _ = _rows(_req(u.x, torch.float32, "x"), "x")
    inds, ldi = _rows(_req(u.inds, torch.int32, "inds"), "inds")
    if u.skip is None:
        raise ValueError("gemm_upsample_split: no skip operand (use gemm_upsample_cat)")
    skip, lds = _rows(_req(u.skip, torch.float32, "skip"), "skip")
    W1, _ = _rows(_req(W1, torch.float32, "W1"), "W1")
    W2, _ = _rows(_req(W2, torch.float32, "W2"), "W2")
    C1, C2, M, N = x.shape[1], skip.shape[1], inds.shape[0], W2.shape[1]
    if W1.shape != (C1, N) or W2.shape[0] != C2 or skip.shape[0] != M or not (W1.is_contiguous() and W2.is_contiguous()):
        raise ValueError("gemm_upsample_split: operands %s | %s, W1 %s, W2 %s" % (tuple(x.shape), tuple(skip.shape), tuple(W1.shape),
                                                                                   tuple(W2.shape)))
    if not upsample_split_ok(u, N):
        raise ValueError("gemm_upsample_split: not a call of the split form (ops.upsample_split_ok): use gemm_upsample_cat")
    Y = gemm(x, W1)
    dev, hint = x.device, int(getattr(inds, "n_hint", 0) or 0)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("gemm_upsample_split: out must be a contiguous, 16-byte aligned float32 [%d, %d]" % (M, N))
    if col_shift is not None and (col_shift.data_ptr() % 16 or col_shift.numel() != N):
        raise ValueError("gemm_upsample_split: col_shift must be a 16-byte aligned vector of %d" % N)
    Wp = packed_x3_weights(W2)
    ws = workspace(lib.d3f_gemm_x3_workspace_bytes(M, N, C2, hint), dev)
    with _timed("gemm_x3", dict(M=M, N=N, K=C2), dev):
        rc = lib.d3f_gemm_x3_gres(skip.data_ptr(), M, lds, C2, None, 0, None, 0, 0, Wp.data_ptr(), out.data_ptr(), N, M, N, None, None,
                                  _ptr(col_shift), Y.data_ptr(), N, inds.data_ptr(), ldi, x.shape[0], _nd(x), 1 if leaky else 0,
                                  float(alpha), ws.data_ptr(), ws.numel(), _nd(inds), None, hint, _stream(dev))
    _lib.check(rc, "gemm_x3_gres")
    return _tag(out, inds)


def gemm_cat2(A1, A2, W, col_scale=None, col_shift=None, leaky=False, alpha=0.2):
    """out = act(([A1 | A2] @ W) * col_scale + col_shift) without building the concatenation (same rows in A1 and A2)."""
    A1, ld1 = _rows(_feat(A1, "A1"), "A1")
    A2, ld2 = _rows(_feat(A2, "A2"), "A2")
    W, ldb = _rows(_req(W, torch.float32, "W"), "W")
    M, C1, C2, N = A1.shape[0], A1.shape[1], A2.shape[1], W.shape[1]
    if A2.shape[0] != M or W.shape[0] != C1 + C2:
        raise ValueError("gemm_cat2: operands %s | %s, W %s" % (tuple(A1.shape), tuple(A2.shape), tuple(W.shape)))
    if (C1 % 4 or ld2 % 4 or A2.data_ptr() % 16) and not _h(A1):
        return gemm(torch.cat([A1, A2], 1), W, col_scale=col_scale, col_shift=col_shift, leaky=leaky, alpha=alpha)
    out = torch.empty((M, N), dtype=_out_dtype(), device=A1.device)
    _contract("gemm_cat2", A1, M, ld1, C1, None, 0, A2, ld2, C2, W, ldb, out, N, _nd(A1), _nd(A1), int(getattr(A1, "n_hint", 0) or 0),
              col_scale=col_scale, col_shift=col_shift, leaky=leaky, alpha=alpha)
    return _tag(out, A1)


# Chained contractions (D3F_GEMM_CHAIN=0: every launch as before).  Two level-0 launches of the resident form write a tall tensor that
# the very next launch reads back and contracts to 32 columns: the decoder's last unary block before `last_unary` (its 64-column
# output has no other consumer) and a resnetb block's conv3 + shortcut before the next block's conv1.  d3f_gemm_x3_chain computes the
# second product from the first one's accumulators (csrc/gemm_x3.h): one launch, the tall tensor not written / not read back.
GEMM_CHAIN = os.environ.get("D3F_GEMM_CHAIN", "1") != "0"
CHAIN_MIN_ROWS = None       # tests only: expected rows from which gemm_chain_ok answers as if the call were a tall (resident) one


def packed_x3_chain_weights(W2):
    """W2 f32[64 or 128, 32] (contiguous rows) -> the pre-split planes d3f_gemm_x3_chain stages for its SECOND product: the layout of
    packed_x3_weights with the k rows of every 16-block in the kernel's accumulator order; made once per (weight tensor, view, version)."""
    lib = _lib.load()
    return _packed_weights(W2, "_d3f_x3c", lambda K, N: torch.empty((int(lib.d3f_gemm_x3_packed_bytes(K, N)) // 2,), dtype=torch.int16,
                                                                    device=W2.device), lib.d3f_gemm_pack_x3_chain, "gemm_pack_x3_chain")


def gemm_chain_ok(M, N, K, store_first, hint=0):
    """Is a contraction of M rows, K -> N columns, followed by one to 32 columns, taken as ONE chained launch?  fp32 only, and only
    where the first contraction alone would run the resident form of d3f_gemm_x3 (the library's predicate d3f_gemm_x3_chain_ok)."""
    if not (GEMM_CHAIN and GEMM_X3) or BF16_CONTRACTION or BF16_FEATURES or M > X3_MAX_ROWS:
        return False
    rows = hint if 0 < hint < M else M
    if CHAIN_MIN_ROWS is not None and rows >= CHAIN_MIN_ROWS:
        M, hint = max(M, 65536), 0
    return bool(_lib.load().d3f_gemm_x3_chain_ok(M, N, K, 1 if store_first else 0, hint))


def _chain_addressable(N, *operands):
    """float4-addressable fp32 operands ((tensor, leading dimension, columns) triples) with whole k-tiles: what _route asks of a call
    before it hands it to d3f_gemm_x3."""
    for t, ld, cols in operands:
        if t is not None and (t.dtype != torch.float32 or cols % 32 or ld % 4 or t.data_ptr() % 16):
            return False
    return N % 4 == 0


def gemm_chain(A, W, W2, idx=None, skip=None, store_first=True, col_scale=None, col_shift=None, leaky=False, alpha=0.2,
               col_scale2=None, col_shift2=None, leaky2=False, alpha2=0.2, out=None, out2=None):
    """Y = act(([ A[idx[:,0]] (A itself when idx is None) | skip ] @ W) * col_scale + col_shift), out2 = act2((Y @ W2) * col_scale2 +
    col_shift2) in ONE launch of the resident form, whatever the row count.  W f32[K, N] with N = 64 or 128, W2 f32[N, 32].
    -> (Y, out2); Y is None -- and never written -- with store_first=False.  Rows at and beyond the device-resident row count of a
    capacity-sized operand are not written."""
    lib = _lib.load()
    A, lda = _rows(_req(A, torch.float32, "A"), "A")
    W, _ = _rows(_req(W, torch.float32, "W"), "W")
    W2, _ = _rows(_req(W2, torch.float32, "W2"), "W2")
    C1, C2, lds, ldi = A.shape[1], 0, 0, 0
    src = A
    if idx is not None:
        idx, ldi = _rows(_req(idx, torch.int32, "idx"), "idx")
        src = idx
    if skip is not None:
        skip, lds = _rows(_req(skip, torch.float32, "skip"), "skip")
        C2 = skip.shape[1]
    M, K, N, dev = src.shape[0], C1 + C2, W.shape[1], A.device
    if W.shape[0] != K or tuple(W2.shape) != (N, 32) or not (W.is_contiguous() and W2.is_contiguous()) or (skip is not None and skip.shape[0] != M):
        raise ValueError("gemm_chain: operands %d + %d columns, W %s, W2 %s" % (C1, C2, tuple(W.shape), tuple(W2.shape)))
    if not _chain_addressable(N, (A, lda, C1), (skip, lds, C2)):
        raise ValueError("gemm_chain: operands must be float32, 16-byte aligned, with whole k-tiles of 32 columns")
    for v, n, name in ((col_scale, N, "col_scale"), (col_shift, N, "col_shift"), (col_scale2, 32, "col_scale2"), (col_shift2, 32, "col_shift2")):
        if v is not None and (_req(v, torch.float32, name).numel() != n or not v.is_contiguous() or v.data_ptr() % 16):
            raise ValueError("gemm_chain: %s must be a contiguous, 16-byte aligned vector of %d" % (name, n))
    Y, ldc = None, N
    if store_first:
        Y = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else out
        Y, ldc = _rows(_req(Y, torch.float32, "out"), "out")
        if tuple(Y.shape) != (M, N):
            raise ValueError("gemm_chain: out must be [%d, %d]" % (M, N))
    out2 = torch.empty((M, 32), dtype=torch.float32, device=dev) if out2 is None else out2
    out2, ldc2 = _rows(_req(out2, torch.float32, "out2"), "out2")
    if tuple(out2.shape) != (M, 32):
        raise ValueError("gemm_chain: out2 must be [%d, 32]" % M)
    Wp, W2p = packed_x3_weights(W), packed_x3_chain_weights(W2)
    # (recorded under the resident family with the FIRST contraction's shape: the chained product is not in the record's flops)
    with _timed("gemm_x3r", dict(M=M, N=N, K=K), dev):
        rc = lib.d3f_gemm_x3_chain(A.data_ptr(), A.shape[0], lda, C1, _ptr(idx), ldi, _ptr(skip), lds, C2, Wp.data_ptr(), _ptr(Y), ldc, M, N,
                                   None, _ptr(col_scale), _ptr(col_shift), None, 0, 1 if leaky else 0, float(alpha), W2p.data_ptr(),
                                   _ptr(col_scale2), _ptr(col_shift2), 1 if leaky2 else 0, float(alpha2), out2.data_ptr(), ldc2,
                                   _nd(src), _nd(A), _stream(dev))
    _lib.check(rc, "gemm_x3_chain")
    return (_tag(Y, src) if Y is not None else None), _tag(out2, src)


class PendingUnary(UpsampleCat):
    """The not-yet-launched unary block act(([ x'[inds[:,0]] | skip ] @ W) * col_scale + col_shift) over a pending concatenation `u`
    (the level-0 decoder block, 64 columns).  `last_unary` consumes it with one chained launch (chain) and the 64-column tensor is
    never written; every other consumer calls .materialize(), the ordinary launch, and sees the tensor it always saw."""

    def __init__(self, u, W, col_scale, col_shift, leaky, alpha):
        self.u, self.W, self.col_scale, self.col_shift, self.leaky, self.alpha = u, W, col_scale, col_shift, leaky, alpha
        self.shape = (u.shape[0], W.shape[1])
        self.device = u.device
        self.dtype = torch.float32
        _tag(self, u.inds)

    def materialize(self):
        return gemm_upsample_cat(self.u, self.W, col_scale=self.col_scale, col_shift=self.col_shift, leaky=self.leaky, alpha=self.alpha)

    def chain(self, W2):
        u = self.u
        return gemm_chain(u.x, self.W, W2, idx=u.inds, skip=u.skip, store_first=False, col_scale=self.col_scale,
                          col_shift=self.col_shift, leaky=self.leaky, alpha=self.alpha)[1]


def pending_unary_ok(u, N):
    """Does the unary block (N columns) over the pending concatenation `u` stay pending for a chained `last_unary`?"""
    if not isinstance(u, UpsampleCat) or isinstance(u, PendingUnary) or u.x.dim() != 2 or u.inds.dim() != 2:
        return False
    C1, C2 = u.x.shape[1], (u.skip.shape[1] if u.skip is not None else 0)
    if u.skip is not None and (u.skip.dim() != 2 or u.skip.stride(1) != 1):
        return False
    if u.x.stride(1) != 1 or u.inds.dtype != torch.int32 or not _chain_addressable(N, (u.x, u.x.stride(0), C1), (u.skip, u.skip.stride(0) if C2 else 0, C2)):
        return False
    return gemm_chain_ok(u.inds.shape[0], N, C1 + C2, False, int(getattr(u.inds, "n_hint", 0) or 0))


def _kp_front(what, query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent, KP_influence,
              aggregation_mode, col_scale=None, col_shift=None, residual=None, leaky=False, alpha=0.2, row_pos=True, feat=_feat):
    """The operand preparation every KPConv wrapper shares -> (gather, kpar, row_pos, epi, tail, f): the argument groups of the
    entry points of csrc/kpconv.hip, tensors and host arrays as objects (they must outlive the launch: pass them through _arg) --
      gather = q, Nq, s, Ns, idx, ld_idx, K, f, ldf     kpar = kernel points (host), num_kp, extent, influence, aggregation
      epi = col_scale, col_shift, residual, ldr, leaky, alpha     tail = Nq_dev, Ns_dev, q_order
    row_pos: the row-positive flags of the features (d3f_row_positive, launched here), or None when the form does not read them."""
    lib = _lib.load()
    q = _req(query_points, torch.float32, "query_points", 2).contiguous()
    s = _req(support_points, torch.float32, "support_points", 2).contiguous()
    idx, ld_idx = _rows(_req(neighbors_indices, torch.int32, "neighbors_indices"), "neighbors_indices")
    f, ldf = _rows(feat(features, "features"), "features")
    if KP_influence not in _INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation_mode not in _AGGREGATION:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    if K_values is not None and f.shape[1] != K_values.shape[1]:
        raise ValueError("%s: features have %d channels, K_values expects %d" % (what, f.shape[1], K_values.shape[1]))
    kp = _kp_host(K_points)
    Nq, Ns = q.shape[0], s.shape[0]
    nq_dev, ns_dev = _nd(query_points), _nd(support_points)
    if ns_dev is None:
        ns_dev = _nd(features)
    rpos = None
    if row_pos:
        rpos = torch.empty((max(Ns, 1),), dtype=torch.uint8, device=q.device)
        _lib.check(lib.d3f_row_positive(f.data_ptr(), Ns, ldf, f.shape[1], rpos.data_ptr(), ns_dev, _h(f), _stream(q.device)),
                   "row_positive")
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(_req(residual, torch.float32, "residual"), "residual")
    return ((q, Nq, s, Ns, idx, ld_idx, idx.shape[1], f, ldf),
            (kp, kp.shape[0], float(KP_extent), _INFLUENCE[KP_influence], _AGGREGATION[aggregation_mode]), rpos,
            (col_scale, col_shift, residual, ldr, 1 if leaky else 0, float(alpha)), (nq_dev, ns_dev, _order(query_points)), f)


def _arg(v):
    """A kernel argument: a tensor's device address, a host array's address, anything else as it is."""
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return v.ctypes.data if isinstance(v, np.ndarray) else v


def kpconv_aggregate(query_points, support_points, neighbors_indices, features, K_points, KP_extent,
                     KP_influence="linear", aggregation_mode="sum"):
    """-> (wf f32[Nq, num_kp*Cin], inv_cnt f32[Nq])   (phase 1 of KPConv_ops)."""
    lib = _lib.load()
    if neighbors_indices.shape[0] != query_points.shape[0] or features.shape[0] != support_points.shape[0]:
        raise ValueError("KPConv: %d queries / %d index rows, %d supports / %d feature rows" %
                         (query_points.shape[0], neighbors_indices.shape[0], support_points.shape[0], features.shape[0]))
    gather, kpar, row_pos, _, tail, f = _kp_front("KPConv", query_points, support_points, neighbors_indices, features, K_points, None,
                                                  KP_extent, KP_influence, aggregation_mode)
    Nq, Ns, K, Cin = gather[1], gather[3], gather[6], f.shape[1]
    wf = torch.empty((Nq, kpar[1] * Cin), dtype=torch.float32, device=f.device)
    inv_cnt = torch.empty((Nq,), dtype=torch.float32, device=f.device)
    with _timed("kpconv_aggregate", dict(Nq=Nq, Ns=Ns, K=K, Cin=Cin), f.device):
        rc = lib.d3f_kpconv_aggregate(*map(_arg, (*gather, Cin, row_pos, *kpar, wf, inv_cnt, *tail, _h(f), _stream(f.device))))
    _lib.check(rc, "kpconv_aggregate")
    return _tag(wf, query_points), _tag(inv_cnt, query_points)


def kpconv_deform_aggregate(query_points, support_points, neighbors_indices, features, K_points, offsets, KP_extent,
                            KP_influence="linear", aggregation_mode="sum", modulations=None, raw=False):
    """Phase 1 of KPConv_deform_ops (kernels/convolution_ops.py:379-490) -> wf f32[Nq, num_kp*Cin], modulations applied.
    raw=False: the operator's own arguments -- offsets f32[Nq, num_kp, 3] (or [Nq, 3*num_kp]) in the units of the points,
    modulations f32[Nq, num_kp] or None.
    raw=True: offsets f32[Nq, 3*num_kp] or [Nq, 4*num_kp] is the RAW output of the offset convolution (:331-339) -- the kernel scales
    the first 3*num_kp columns by KP_extent and turns the remaining num_kp, if any, into 2*sigmoid modulations (:344-359)."""
    lib = _lib.load()
    if neighbors_indices.shape[0] != query_points.shape[0] or features.shape[0] != support_points.shape[0]:
        raise ValueError("KPConv_deformable: %d queries / %d index rows, %d supports / %d feature rows" %
                         (query_points.shape[0], neighbors_indices.shape[0], support_points.shape[0], features.shape[0]))
    if isinstance(features, torch.Tensor) and features.dtype == torch.bfloat16:
        raise TypeError("KPConv_deformable reads float32 feature rows only: d3f_kpconv_deform_aggregate has no bfloat16 "
                        "feature-storage form")
    gather, kpar, _, _, tail, f = _kp_front("KPConv_deformable", query_points, support_points, neighbors_indices, features, K_points,
                                            None, KP_extent, KP_influence, aggregation_mode, row_pos=False,
                                            feat=lambda t, name: _req(t, torch.float32, name))
    Nq, Ns, K, Cin, num_kp = gather[1], gather[3], gather[6], f.shape[1], kpar[1]
    _req(offsets, torch.float32, "offsets")
    if offsets.dim() == 3:
        offsets = offsets.reshape(offsets.shape[0], -1)
    off, ld_off = _rows(offsets, "offsets")
    mod, ld_mod = None, 0
    if raw:
        if modulations is not None or tuple(off.shape) not in ((Nq, 3 * num_kp), (Nq, 4 * num_kp)):
            raise ValueError("KPConv_deformable: raw offsets are %s, expected (%d, %d) or (%d, %d) and no modulations"
                             % (tuple(off.shape), Nq, 3 * num_kp, Nq, 4 * num_kp))
        if off.shape[1] == 4 * num_kp:
            mod, ld_mod = off[:, 3 * num_kp:], ld_off
    else:
        if tuple(off.shape) != (Nq, 3 * num_kp):
            raise ValueError("KPConv_deformable: offsets are %s, expected (%d, %d, 3)" % (tuple(offsets.shape), Nq, num_kp))
        if modulations is not None:
            mod, ld_mod = _rows(_req(modulations, torch.float32, "modulations"), "modulations")
            if tuple(mod.shape) != (Nq, num_kp):
                raise ValueError("KPConv_deformable: modulations are %s, expected (%d, %d)" % (tuple(mod.shape), Nq, num_kp))
    wf = torch.empty((Nq, num_kp * Cin), dtype=torch.float32, device=f.device)
    with _timed("kpconv_deform_aggregate", dict(Nq=Nq, Ns=Ns, K=K, Cin=Cin), f.device):
        rc = lib.d3f_kpconv_deform_aggregate(*map(_arg, (*gather, Cin, off, ld_off, float(KP_extent) if raw else 1.0, mod, ld_mod,
                                                         1 if raw else 0, *kpar, wf, *tail, 0, _stream(f.device))))
    _lib.check(rc, "kpconv_deform_aggregate")
    return _tag(wf, query_points)


def kpconv_deformable(query_points, support_points, neighbors_indices, features, K_points, K_values, offset_weights, offset_bias,
                      KP_extent, KP_influence="linear", aggregation_mode="sum", modulated=False, col_scale=None, col_shift=None,
                      residual=None, leaky=False, alpha=0.2):
    """Whole deformable KPConv (kernels/convolution_ops.py:258-499) + epilogue, four launches and the row flags:
      1. the offset convolution: the rigid operator (aggregation, neighbour-count normalisation, contraction) with
         offset_weights f32[num_kp, Cin, D] and col_shift = offset_bias f32[D], D = 3*num_kp (4*num_kp when modulated);
      2. kpconv_deform_aggregate with its raw output (raw=True: the scaling by KP_extent and the sigmoid happen in the kernel);
      3. the contraction with K_values f32[num_kp, Cin, Cout] and the caller's epilogue (no row_scale: no normalisation)."""
    num_kp, cin, cout = K_values.shape
    D = (4 if modulated else 3) * num_kp
    if tuple(offset_weights.shape) != (num_kp, cin, D) or tuple(offset_bias.shape) != (D,):
        raise ValueError("KPConv_deformable: offset_conv_weights %s / offset_conv_bias %s, expected (%d, %d, %d) / (%d,)" %
                         (tuple(offset_weights.shape), tuple(offset_bias.shape), num_kp, cin, D, D))
    if features.shape[1] != cin:
        raise ValueError("KPConv_deformable: features have %d channels, K_values expects %d" % (features.shape[1], cin))
    with f32_output():
        wf0, inv_cnt = kpconv_aggregate(query_points, support_points, neighbors_indices, features, K_points, KP_extent, KP_influence,
                                        aggregation_mode)
        offsets = gemm(wf0, offset_weights.reshape(num_kp * cin, D), row_scale=inv_cnt, col_shift=offset_bias)
    wf = kpconv_deform_aggregate(query_points, support_points, neighbors_indices, features, K_points, offsets, KP_extent,
                                 KP_influence, aggregation_mode, raw=True)
    return gemm(wf, K_values.reshape(num_kp * cin, cout), col_scale=col_scale, col_shift=col_shift, residual=residual, leaky=leaky,
                alpha=alpha)


def kpconv_fused_supported(cin, cout, num_kp, KP_influence, aggregation_mode, available=False):
    """Should KPConv_ops use the one-kernel form for this shape?  available=True: does the form exist at all (Cin = 256 exists
    but measured no faster than aggregation + contraction: see d3f_kpconv_fused_supported)."""
    r = _lib.load().d3f_kpconv_fused_supported(int(cin), int(cout), int(num_kp), _INFLUENCE.get(KP_influence, -1),
                                               _AGGREGATION.get(aggregation_mode, -1))
    return r >= 1 if available else r == 1


def _packed_kpconv(K_values, slot, alloc, pack, what):
    """K_values f32[num_kp, Cin, Cout] -> a packed copy of the [num_kp*Cin, Cout] matrix, riding on the tensor like the contraction
    weights' copies (made at a model's first eager use -- the engine's warm-up -- never inside a captured graph)."""
    def make(t):
        num_kp, cin, cout = K_values.shape
        W = _req(K_values, torch.float32, "K_values").reshape(num_kp * cin, cout).contiguous()
        if t is None:
            t = alloc(W)
        _lib.check(pack(W.data_ptr(), num_kp * cin, cout, t.data_ptr(), _stream(W.device)), what)
        return t
    return _packed_on_tensor(K_values, slot, make)


def packed_kpconv_weights(K_values):
    """-> the k-block-packed copy d3f_kpconv_fused reads."""
    return _packed_kpconv(K_values, "_d3f_packed", torch.empty_like, _lib.load().d3f_kpconv_pack_weights, "kpconv_pack_weights")


def packed_kpconv_weights_x3(K_values):
    """-> the pre-split bf16 planes d3f_kpconv_fused_x3 / d3f_kpconv_fused32_x3 read."""
    lib = _lib.load()
    return _packed_kpconv(K_values, "_d3f_packed_x3",
                          lambda W: torch.empty((int(lib.d3f_kpconv_packed_x3_bytes(*W.shape)) // 2,), dtype=torch.int16, device=W.device),
                          lib.d3f_kpconv_pack_weights_x3, "kpconv_pack_weights_x3")


# every packed copy that can ride on a weight tensor: its slot and the packer that (re-)makes it
_PACKERS = (("_d3f_bf16t", packed_bf16_weights), ("_d3f_f32t", packed_f32t_weights), ("_d3f_x3", packed_x3_weights),
            ("_d3f_x3c", packed_x3_chain_weights),
            ("_d3f_packed", packed_kpconv_weights), ("_d3f_packed_x3", packed_kpconv_weights_x3))


# The fused KPConv kernels of levels 0 to 2 contract their LDS tile in the operand-split form (csrc/kpconv.hip, round 5: three exact
# bf16 planes per operand, six exact products per fp32 product, fp32 accumulate -- fp32 in, fp32 out); D3F_KP_X3=0 keeps the
# fp32 MFMA form.
KP_X3 = os.environ.get("D3F_KP_X3", "1") != "0"


def _kpconv_fused(what, query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent, KP_influence,
                  aggregation_mode, col_scale, col_shift, residual, leaky, alpha):
    lib = _lib.load()
    num_kp, cin, cout = K_values.shape
    gather, kpar, row_pos, epi, tail, f = _kp_front(what, query_points, support_points, neighbors_indices, features, K_points, K_values,
                                                    KP_extent, KP_influence, aggregation_mode, col_scale, col_shift, residual, leaky,
                                                    alpha)
    level0 = what == "kpconv_fused32"
    x3 = KP_X3 and (num_kp * cin) % 32 == 0 and (level0 or cout % 16 == 0)
    if x3:
        W = packed_kpconv_weights_x3(K_values)
    elif level0:
        W = _req(K_values, torch.float32, "K_values").reshape(num_kp * cin, cout).contiguous()
    else:
        W = packed_kpconv_weights(K_values)
    out = torch.empty((gather[1], cout), dtype=f.dtype, device=f.device)
    with _timed(what, dict(Nq=gather[1], Ns=gather[3], K=gather[6], Cin=cin, Cout=cout), f.device):
        if level0:
            rc = (lib.d3f_kpconv_fused32_x3 if x3 else lib.d3f_kpconv_fused32)(
                *map(_arg, (*gather, row_pos, *kpar, W, *epi, out, cout, *tail, _h(f), _stream(f.device))))
        else:
            rc = (lib.d3f_kpconv_fused_x3 if x3 else lib.d3f_kpconv_fused)(
                *map(_arg, (*gather, cin, row_pos, *kpar, W, cout, *epi, out, cout, *tail, _h(f), _stream(f.device))))
    _lib.check(rc, what)
    return _tag(out, query_points)


def kpconv_fused32(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                   KP_influence="linear", aggregation_mode="sum", col_scale=None, col_shift=None, residual=None,
                   leaky=False, alpha=0.2):
    """Whole KPConv (+ epilogue) for Cin = Cout = 32 in one kernel (the aggregation tile is contracted from LDS)."""
    if tuple(K_values.shape[1:]) != (32, 32):
        raise ValueError("kpconv_fused32 needs Cin == Cout == 32")
    return _kpconv_fused("kpconv_fused32", query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                         KP_influence, aggregation_mode, col_scale, col_shift, residual, leaky, alpha)


def kpconv_fused(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                 KP_influence="linear", aggregation_mode="sum", col_scale=None, col_shift=None, residual=None,
                 leaky=False, alpha=0.2):
    """Whole KPConv (+ epilogue) for Cin == Cout in {64, 128} in one kernel (kpconv_fused_supported says when)."""
    return _kpconv_fused("kpconv_fused", query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                         KP_influence, aggregation_mode, col_scale, col_shift, residual, leaky, alpha)


def kpconv_fused_c1(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
                    KP_influence="linear", aggregation_mode="sum", col_scale=None, col_shift=None, residual=None,
                    leaky=False, alpha=0.2):
    """Whole KPConv (+ epilogue) for Cin = 1 in one kernel.  K_values f32[num_kp, 1, Cout]."""
    lib = _lib.load()
    num_kp, cin, cout = K_values.shape
    if cin != 1:
        raise ValueError("kpconv_fused_c1 needs Cin == 1")
    gather, kpar, _, epi, tail, f = _kp_front("kpconv_fused_c1", query_points, support_points, neighbors_indices, features, K_points,
                                              K_values, KP_extent, KP_influence, aggregation_mode, col_scale, col_shift, residual,
                                              leaky, alpha, row_pos=False, feat=lambda t, name: _req(t, torch.float32, name))
    W = _req(K_values, torch.float32, "K_values").reshape(num_kp, cout).contiguous()
    out = torch.empty((gather[1], cout), dtype=torch.bfloat16 if BF16_FEATURES else torch.float32, device=f.device)
    with _timed("kpconv_fused_c1", dict(Nq=gather[1], Ns=gather[3], K=gather[6], Cin=1, Cout=cout), f.device):
        rc = lib.d3f_kpconv_fused_c1(*map(_arg, (*gather, *kpar, W, cout, *epi, out, cout, *tail, _h(out), _stream(f.device))))
    _lib.check(rc, "kpconv_fused_c1")
    return _tag(out, query_points)


def ind_max_pool(x, inds):
    lib = _lib.load()
    x, ldx = _rows(_feat(x, "x"), "x")
    inds, ldi = _rows(_req(inds, torch.int32, "inds"), "inds")
    dev = x.device
    out = torch.empty((inds.shape[0], x.shape[1]), dtype=x.dtype, device=dev)
    with _timed("ind_max_pool", dict(N1=x.shape[0], N2=inds.shape[0], K=inds.shape[1], C=x.shape[1]), dev):
        rc = lib.d3f_ind_max_pool(x.data_ptr(), x.shape[0], ldx, x.shape[1], inds.data_ptr(), inds.shape[0], ldi,
                                  inds.shape[1], out.data_ptr(), x.shape[1], None, _nd(x), _nd(inds), _order(inds),
                                  _h(x), _stream(dev))
    _lib.check(rc, "ind_max_pool")
    return _tag(out, inds)


def closest_pool_cat(x, inds, skip=None):
    lib = _lib.load()
    x, ldx = _rows(_req(x, torch.float32, "x"), "x")
    inds, ldi = _rows(_req(inds, torch.int32, "inds"), "inds")
    dev = x.device
    C1 = x.shape[1]
    C2 = lds = 0
    if skip is not None:
        skip, lds = _rows(_req(skip, torch.float32, "skip"), "skip")
        C2 = skip.shape[1]
        if skip.shape[0] != inds.shape[0]:
            raise ValueError("closest_pool_cat: %d index rows, %d skip rows" % (inds.shape[0], skip.shape[0]))
    out = torch.empty((inds.shape[0], C1 + C2), dtype=torch.float32, device=dev)
    rc = lib.d3f_closest_pool_cat(x.data_ptr(), x.shape[0], ldx, C1, inds.data_ptr(), inds.shape[0], ldi,
                                  _ptr(skip), lds, C2, out.data_ptr(), C1 + C2,
                                  _nd(x), _nd(inds), _stream(dev))
    _lib.check(rc, "closest_pool_cat")
    return _tag(out, inds)


def detect_head(x, neighbors, stack_lengths_dev, include_zero_dev, stack_group=0):
    """-> (desc f32[N,C], score f32[N,1]).  stack_group: clouds per reference stack inside a batched stack (0: the whole
    stack is one reference stack), see include/d3feat_amd.h."""
    lib = _lib.load()
    x, ldx = _rows(_req(x, torch.float32, "x"), "x")
    nb, ldi = _rows(_req(neighbors, torch.int32, "neighbors"), "neighbors")
    dev = x.device
    N, Cc = x.shape
    B = stack_lengths_dev.numel()
    desc = torch.empty((N, Cc), dtype=torch.float32, device=dev)
    score = torch.empty((N, 1), dtype=torch.float32, device=dev)
    scratch = torch.empty((2 * B + 2 + (N + 3) // 4,), dtype=torch.int32, device=dev)
    with _timed("detect_head", dict(N=N, K=nb.shape[1], C=Cc), dev):
        rc = lib.d3f_detect_head(x.data_ptr(), N, ldx, Cc, nb.data_ptr(), ldi, nb.shape[1],
                                 stack_lengths_dev.data_ptr(),
                                 _ptr(include_zero_dev),
                                 int(stack_group), B, desc.data_ptr(), Cc, score.data_ptr(), scratch.data_ptr(), _order(nb),
                                 _stream(dev))
    _lib.check(rc, "detect_head")
    return _tag(desc, x), _tag(score, x)


def _typed(t, dtype, name, ndim=None):
    """_req without the device check: the shape checks of an entry point come before "there is no CPU path"."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor on a GPU (got %s)" % (name, type(t)))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must be %d-D (got shape %s)" % (name, ndim, tuple(t.shape)))
    return t


def _head_arguments(what, x, neighbors, stack_lengths_dev):
    """The checks detect_head_backward and neighbor_transpose share, before the device is asked -> (nb, ldi, lens)."""
    nb, ldi = _rows(_typed(neighbors, torch.int32, "neighbors"), "neighbors")
    lens = _typed(stack_lengths_dev, torch.int32, "stack_lengths_dev", 1)
    if not lens.is_contiguous():
        raise ValueError("%s: stack_lengths_dev must be contiguous" % what)
    if not 1 <= lens.numel() <= 255:
        raise ValueError("%s: %d clouds (1 .. 255)" % (what, lens.numel()))
    if nb.shape[0] * nb.shape[1] > (1 << 31) - 8192:
        raise ValueError("%s: %d x %d neighbour slots (at most 2^31 - 8192)" % (what, nb.shape[0], nb.shape[1]))
    if x is not None and x.shape[0] != nb.shape[0]:
        raise ValueError("%s: %d feature rows, %d neighbour rows" % (what, x.shape[0], nb.shape[0]))
    return nb, ldi, lens


def _on_device(what, **tensors):
    """There is no CPU path: after the shape checks, before the library is asked."""
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise _lib.D3FeatLibraryError("%s: %s is on %s: d3feat_amd has no CPU path" % (what, name, t.device))


def neighbor_transpose(neighbors, stack_lengths_dev):
    """The transposed neighbour table (d3f_neighbor_transpose, include/d3feat_amd.h) -> (start i32[N + 1], edges i32[N * K]) on the
    device: row j's segment edges[start[j] : start[j + 1]] holds the edges e = i * K + k with neighbors[i, k] == j in ascending e --
    np.argsort(kind="stable") of the valid edges.  Nine launches, no read-back, capturable."""
    lib = _lib.load()
    nb, ldi, lens = _head_arguments("neighbor_transpose", None, neighbors, stack_lengths_dev)
    _on_device("neighbor_transpose", neighbors=nb, stack_lengths_dev=lens)
    dev = nb.device
    N, K = nb.shape
    start = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    edges = torch.empty((max(N * K, 1),), dtype=torch.int32, device=dev)
    nbytes = lib.d3f_neighbor_transpose_workspace_bytes(N, K)
    ws = workspace(nbytes, dev)
    with _timed("neighbor_transpose", dict(N=N, K=K), dev):
        rc = lib.d3f_neighbor_transpose(nb.data_ptr(), N, ldi, K, lens.data_ptr(), lens.numel(), start.data_ptr(), edges.data_ptr(),
                                        ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "neighbor_transpose")
    return start, edges[:N * K]


def detect_head_backward(x, neighbors, stack_lengths_dev, include_zero_dev, grad_desc, grad_score, stack_group=0, transpose=None,
                         out=None):
    """Backward of detect_head -> gx f32[N, C], the gradient with respect to x, from the gradients with respect to the rows of desc
    (grad_desc f32[N, C]) and of score (grad_score f32[N] or [N, 1]); either may be None (zero), both may be strided column views of
    a record block (validation.loss_gradients_records(out_records=...)).  transpose: (start, edges) of neighbor_transpose for the
    same `neighbors`; built here when None.  include_zero_dev, when given, is read as the NUMBER of pad slots of every cloud's row of
    in_batches.  The definition, the tie rules and the summation orders: include/d3feat_amd.h (d3f_detect_head_backward).  Rows at
    or beyond sum(stack_lengths_dev) of `out` are left alone.  Six launches, no read-back, capturable."""
    lib = _lib.load()
    x, ldx = _rows(_typed(x, torch.float32, "x"), "x")
    nb, ldi, lens = _head_arguments("detect_head_backward", x, neighbors, stack_lengths_dev)
    dev = x.device
    N, Cc = x.shape
    if not 1 <= Cc <= 128:
        raise ValueError("detect_head_backward: C = %d (1 .. 128)" % Cc)
    if int(stack_group) < 0:
        raise ValueError("detect_head_backward: stack_group = %r" % (stack_group,))
    gd = ldg = gs = ldgs = None
    if grad_desc is not None:
        gd, ldg = _rows(_typed(grad_desc, torch.float32, "grad_desc"), "grad_desc")
        if tuple(gd.shape) != (N, Cc):
            raise ValueError("detect_head_backward: grad_desc is %s, x %s" % (tuple(gd.shape), (N, Cc)))
    if grad_score is not None:
        gs = _typed(grad_score, torch.float32, "grad_score")
        if gs.dim() == 1:
            gs = gs.unsqueeze(1)
        if gs.dim() != 2 or tuple(gs.shape) != (N, 1):
            raise ValueError("detect_head_backward: grad_score is %s, wanted %d rows of one column" % (tuple(grad_score.shape), N))
        ldgs = int(max(gs.stride(0), 1)) if N > 1 else 1
    if include_zero_dev is not None:
        include_zero_dev = _typed(include_zero_dev, torch.int32, "include_zero_dev", 1)
        if include_zero_dev.numel() != lens.numel() or not include_zero_dev.is_contiguous():
            raise ValueError("detect_head_backward: include_zero_dev must be contiguous, one entry per cloud")
    if out is not None:
        out, ldo = _rows(_typed(out, torch.float32, "out"), "out")
        if tuple(out.shape) != (N, Cc):
            raise ValueError("detect_head_backward: out is %s, x %s" % (tuple(out.shape), (N, Cc)))
    _on_device("detect_head_backward", x=x, neighbors=nb, stack_lengths_dev=lens, include_zero_dev=include_zero_dev, grad_desc=gd,
               grad_score=gs, out=out)
    if transpose is None:
        transpose = neighbor_transpose(nb, lens)
    start = _typed(transpose[0], torch.int32, "transpose[0]", 1)
    edges = _typed(transpose[1], torch.int32, "transpose[1]", 1)
    if start.numel() != N + 1 or edges.numel() < N * nb.shape[1] or not (start.is_contiguous() and edges.is_contiguous()):
        raise ValueError("detect_head_backward: transpose must be (start i32[N + 1], edges i32[N * K]) of the same neighbours")
    _on_device("detect_head_backward", start=start, edges=edges)
    if out is None:
        out, ldo = torch.empty((N, Cc), dtype=torch.float32, device=dev), Cc
    B = lens.numel()
    nbytes = lib.d3f_detect_head_backward_workspace_bytes(N, Cc, B)
    ws = workspace(nbytes, dev)
    with _timed("detect_head_backward", dict(N=N, K=nb.shape[1], C=Cc), dev):
        rc = lib.d3f_detect_head_backward(x.data_ptr(), N, ldx, Cc, nb.data_ptr(), ldi, nb.shape[1], lens.data_ptr(), _ptr(include_zero_dev),
                                          int(stack_group), B, start.data_ptr(), edges.data_ptr(), _ptr(gd), ldg or 0, _ptr(gs), ldgs or 0,
                                          out.data_ptr(), ldo, ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "detect_head_backward")
    return _tag(out, x)


def _count(t, name):
    """An optional device-resident row count: int32, one element."""
    if t is not None:
        _typed(t, torch.int32, name)
        if t.numel() != 1:
            raise ValueError("%s must hold one int32 (got shape %s)" % (name, tuple(t.shape)))
    return t


def neighbor_transpose_supports(neighbors, num_supports, nq_dev=None, ns_dev=None):
    """The transposed table of a neighbour matrix whose rows (queries) differ from the rows it names (num_supports supports):
    d3f_neighbor_transpose_qs -> (start i32[num_supports + 1], edges i32[Nq * K]).  nq_dev / ns_dev: device-resident real counts
    (int32[1]) when the shapes are capacities; nq_dev defaults to the tag of `neighbors`.  Nine launches, no read-back, capturable."""
    lib = _lib.load()
    nb, ldi = _rows(_typed(neighbors, torch.int32, "neighbors"), "neighbors")
    Ns = int(num_supports)
    if Ns < 0:
        raise ValueError("neighbor_transpose_supports: num_supports = %d" % Ns)
    Nq, K = nb.shape
    if Nq * K > (1 << 31) - 8192:
        raise ValueError("neighbor_transpose_supports: %d x %d neighbour slots (at most 2^31 - 8192)" % (Nq, K))
    if nq_dev is None:
        nq_dev = getattr(neighbors, "n_dev", None)
    nq_dev, ns_dev = _count(nq_dev, "nq_dev"), _count(ns_dev, "ns_dev")
    _on_device("neighbor_transpose_supports", neighbors=nb, nq_dev=nq_dev, ns_dev=ns_dev)
    dev = nb.device
    start = torch.empty((Ns + 1,), dtype=torch.int32, device=dev)
    edges = torch.empty((max(Nq * K, 1),), dtype=torch.int32, device=dev)
    nbytes = lib.d3f_neighbor_transpose_workspace_bytes(Nq, K)
    ws = workspace(nbytes, dev)
    with _timed("neighbor_transpose_supports", dict(Nq=Nq, Ns=Ns, K=K), dev):
        rc = lib.d3f_neighbor_transpose_qs(nb.data_ptr(), Nq, ldi, K, _ptr(nq_dev), Ns, _ptr(ns_dev), start.data_ptr(), edges.data_ptr(),
                                           ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "neighbor_transpose_supports")
    return start, edges[:Nq * K]


def kpconv_backward(query_points, support_points, neighbors_indices, features, K_points, K_values, grad_out, KP_extent,
                    KP_influence="linear", aggregation_mode="sum", transpose=None, need_features=True, need_weights=True,
                    out_features=None, out_weights=None):
    """Backward of KPConv_ops (kernels/convolution_ops.py:161-255) -> (gf f32[Ns, Cin] or None, gW f32[num_kp, Cin, Cout] or None): the
    gradients with respect to the support feature rows and to K_values, from grad_out f32[Nq, Cout] (rows may be strided).  The
    definition and the summation orders: include/d3feat_amd.h (d3f_kpconv_backward).  transpose: (start, edges) of
    neighbor_transpose_supports for the same `neighbors_indices`; built here when None and gf is wanted.  Device-resident counts ride
    on the tensors' tags as in the forward; rows of out_features at or beyond the support count are left alone.  No read-back,
    capturable."""
    lib = _lib.load()
    q = _typed(query_points, torch.float32, "query_points", 2)
    s = _typed(support_points, torch.float32, "support_points", 2)
    idx, ld_idx = _rows(_typed(neighbors_indices, torch.int32, "neighbors_indices"), "neighbors_indices")
    f, ldf = _rows(_typed(features, torch.float32, "features"), "features")
    W = _typed(K_values, torch.float32, "K_values", 3)
    g, ldg = _rows(_typed(grad_out, torch.float32, "grad_out"), "grad_out")
    if KP_influence not in _INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation_mode not in _AGGREGATION:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    if q.shape[1] != 3 or s.shape[1] != 3:
        raise ValueError("kpconv_backward: points must be [n, 3] (got %s, %s)" % (tuple(q.shape), tuple(s.shape)))
    Nq, Ns, K = q.shape[0], s.shape[0], idx.shape[1]
    num_kp, Cin, Cout = W.shape
    kp = _kp_host(K_points)
    if kp.ndim != 2 or kp.shape != (num_kp, 3) or not 1 <= num_kp <= 15:
        raise ValueError("kpconv_backward: K_points is %s, K_values %s (1 .. 15 kernel points)" % (tuple(kp.shape), tuple(W.shape)))
    if Cin < 1 or Cout < 1:
        raise ValueError("kpconv_backward: K_values is %s" % (tuple(W.shape),))
    if idx.shape[0] != Nq or f.shape[0] != Ns:
        raise ValueError("kpconv_backward: %d queries / %d index rows, %d supports / %d feature rows" % (Nq, idx.shape[0], Ns, f.shape[0]))
    if f.shape[1] != Cin:
        raise ValueError("kpconv_backward: features have %d channels, K_values expects %d" % (f.shape[1], Cin))
    if tuple(g.shape) != (Nq, Cout):
        raise ValueError("kpconv_backward: grad_out is %s, wanted %s" % (tuple(g.shape), (Nq, Cout)))
    if not (need_features or need_weights):
        raise ValueError("kpconv_backward: neither gradient is wanted")
    if Nq * K > (1 << 31) - 8192:
        raise ValueError("kpconv_backward: %d x %d neighbour slots (at most 2^31 - 8192)" % (Nq, K))
    if Ns == 0 and Nq > 0:
        raise ValueError("kpconv_backward: %d queries and no support" % Nq)
    if not float(KP_extent) > 0:
        raise ValueError("kpconv_backward: KP_extent = %r" % (KP_extent,))
    gf = ldgf = gW = None
    if need_features and out_features is not None:
        gf, ldgf = _rows(_typed(out_features, torch.float32, "out_features"), "out_features")
        if tuple(gf.shape) != (Ns, Cin):
            raise ValueError("kpconv_backward: out_features is %s, wanted %s" % (tuple(gf.shape), (Ns, Cin)))
    if need_weights and out_weights is not None:
        gW = _typed(out_weights, torch.float32, "out_weights", 3)
        if tuple(gW.shape) != (num_kp, Cin, Cout) or not gW.is_contiguous():
            raise ValueError("kpconv_backward: out_weights must be contiguous %s" % ((num_kp, Cin, Cout),))
    start = edges = None
    if need_features and transpose is not None:
        start = _typed(transpose[0], torch.int32, "transpose[0]", 1)
        edges = _typed(transpose[1], torch.int32, "transpose[1]", 1)
        if start.numel() != Ns + 1 or edges.numel() < Nq * K or not (start.is_contiguous() and edges.is_contiguous()):
            raise ValueError("kpconv_backward: transpose must be (start i32[Ns + 1], edges i32[Nq * K]) of the same neighbours")
    nq_t = getattr(query_points, "n_dev", None)
    ns_t = getattr(support_points, "n_dev", None)
    if ns_t is None:
        ns_t = getattr(features, "n_dev", None)
    _on_device("kpconv_backward", query_points=q, support_points=s, neighbors_indices=idx, features=f, K_values=W, grad_out=g,
               out_features=gf, out_weights=gW, start=start, edges=edges, nq_dev=nq_t, ns_dev=ns_t)
    dev = f.device
    q, s, W = q.contiguous(), s.contiguous(), W.contiguous()
    if need_features and start is None:
        start, edges = neighbor_transpose_supports(idx, Ns, nq_t, ns_t)
    if need_features and gf is None:
        gf, ldgf = torch.empty((Ns, Cin), dtype=torch.float32, device=dev), Cin
    if need_weights and gW is None:
        gW = torch.empty((num_kp, Cin, Cout), dtype=torch.float32, device=dev)
    nbytes = lib.d3f_kpconv_backward_workspace_bytes(Nq, Ns, K, Cin, Cout, num_kp)
    ws = workspace(nbytes, dev)
    with _timed("kpconv_backward", dict(Nq=Nq, Ns=Ns, K=K, Cin=Cin, Cout=Cout), dev):
        rc = lib.d3f_kpconv_backward(q.data_ptr(), Nq, s.data_ptr(), Ns, idx.data_ptr(), ld_idx, K, f.data_ptr(), ldf, Cin, kp.ctypes.data,
                                     num_kp, float(KP_extent), _INFLUENCE[KP_influence], _AGGREGATION[aggregation_mode], W.data_ptr(),
                                     g.data_ptr(), ldg, Cout, _ptr(start), _ptr(edges), _ptr(gf), ldgf or 0, _ptr(gW), _ptr(nq_t), _ptr(ns_t),
                                     _order(query_points), 0, ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "kpconv_backward")
    if gf is not None and ns_t is not None:
        gf.n_dev = ns_t
        gf.n_hint = getattr(support_points, "n_hint", 0) or getattr(features, "n_hint", 0)
    return gf, gW


def _table(what, transpose, rows, items):
    """(start i32[rows + 1], edges i32[>= items]) of a passed transposed table, checked."""
    start = _typed(transpose[0], torch.int32, "transpose[0]", 1)
    edges = _typed(transpose[1], torch.int32, "transpose[1]", 1)
    if start.numel() != rows + 1 or edges.numel() < items or not (start.is_contiguous() and edges.is_contiguous()):
        raise ValueError("%s: transpose must be (start i32[%d], edges i32[%d]) of the same indices" % (what, rows + 1, items))
    return start, edges


def ind_max_pool_backward(x, inds, y, grad_y, transpose=None, out=None):
    """Backward of ind_max_pool -> gx f32[N1, C], the gradient with respect to x, from y (the STORED forward output) and grad_y f32[N2, C];
    x, y, grad_y and out may be column views.  Ties split evenly, the shadow row's column minima included: the definition and the
    summation orders are in include/d3feat_amd.h (d3f_ind_max_pool_backward).  transpose: (start, edges) of
    neighbor_transpose_supports(inds, N1); built here when None.  Device-resident counts ride on the tags of x and inds; rows of out at
    or beyond the count of x are left alone.  fp32 rows only.  Three launches, no read-back, capturable."""
    lib = _lib.load()
    x, ldx = _rows(_typed(x, torch.float32, "x"), "x")
    idx, ldi = _rows(_typed(inds, torch.int32, "inds"), "inds")
    y, ldy = _rows(_typed(y, torch.float32, "y"), "y")
    g, ldg = _rows(_typed(grad_y, torch.float32, "grad_y"), "grad_y")
    (N1, C), (N2, K) = x.shape, idx.shape
    if C < 1:
        raise ValueError("ind_max_pool_backward: x is %s" % (tuple(x.shape),))
    if tuple(y.shape) != (N2, C) or tuple(g.shape) != (N2, C):
        raise ValueError("ind_max_pool_backward: y is %s, grad_y %s, wanted %s" % (tuple(y.shape), tuple(g.shape), (N2, C)))
    if N2 * K > (1 << 31) - 8192:
        raise ValueError("ind_max_pool_backward: %d x %d neighbour slots (at most 2^31 - 8192)" % (N2, K))
    if out is not None:
        out, ldo = _rows(_typed(out, torch.float32, "out"), "out")
        if tuple(out.shape) != (N1, C):
            raise ValueError("ind_max_pool_backward: out is %s, x %s" % (tuple(out.shape), (N1, C)))
    start = edges = None
    if transpose is not None:
        start, edges = _table("ind_max_pool_backward", transpose, N1, N2 * K)
    n1_t = getattr(x, "n_dev", None)
    n2_t = _row_count(inds, y, grad_y)
    _on_device("ind_max_pool_backward", x=x, inds=idx, y=y, grad_y=g, out=out, start=start, edges=edges, n1_dev=n1_t, n2_dev=n2_t)
    dev = x.device
    if start is None:
        start, edges = neighbor_transpose_supports(idx, N1, n2_t, n1_t)
    if out is None:
        out, ldo = torch.empty((N1, C), dtype=torch.float32, device=dev), C
    nbytes = lib.d3f_ind_max_pool_backward_workspace_bytes(N1, N2, K, C)
    ws = workspace(nbytes, dev)
    with _timed("ind_max_pool_backward", dict(N1=N1, N2=N2, K=K, C=C), dev):
        rc = lib.d3f_ind_max_pool_backward(x.data_ptr(), N1, ldx, C, idx.data_ptr(), N2, ldi, K, y.data_ptr(), ldy, g.data_ptr(), ldg,
                                           start.data_ptr(), edges.data_ptr(), out.data_ptr(), ldo, _ptr(n1_t), _ptr(n2_t), 0,
                                           ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "ind_max_pool_backward")
    return _tag(out, x)


def closest_pool_cat_backward(grad_out, inds, num_coarse, C1, transpose=None, out=None):
    """Backward of closest_pool_cat with respect to x -> gx f32[num_coarse, C1]: the rows grad_out[n, :C1] added, in ascending n, into
    the coarse row inds[n, 0] names; a shadow index carries nothing (include/d3feat_amd.h, d3f_closest_pool_cat_backward).  The skip's
    gradient is the view grad_out[:, C1:].  transpose: (start, edges) of neighbor_transpose_supports(inds[:, :1], num_coarse); built
    here when None.  The device-resident counts ride on the tags of inds / grad_out (fine rows) and of `out` (coarse rows).  One launch,
    no read-back, capturable."""
    lib = _lib.load()
    g, ldg = _rows(_typed(grad_out, torch.float32, "grad_out"), "grad_out")
    idx, ldi = _rows(_typed(inds, torch.int32, "inds"), "inds")
    N1, C1 = int(num_coarse), int(C1)
    N2 = idx.shape[0]
    if N1 < 0 or C1 < 1 or g.shape[1] < C1:
        raise ValueError("closest_pool_cat_backward: num_coarse = %d, C1 = %d, grad_out is %s" % (N1, C1, tuple(g.shape)))
    if idx.shape[1] < 1 or g.shape[0] != N2:
        raise ValueError("closest_pool_cat_backward: inds is %s, grad_out %s" % (tuple(idx.shape), tuple(g.shape)))
    if out is not None:
        out, ldo = _rows(_typed(out, torch.float32, "out"), "out")
        if tuple(out.shape) != (N1, C1):
            raise ValueError("closest_pool_cat_backward: out is %s, wanted %s" % (tuple(out.shape), (N1, C1)))
    start = edges = None
    if transpose is not None:
        start, edges = _table("closest_pool_cat_backward", transpose, N1, N2)
    n1_t = getattr(out, "n_dev", None) if out is not None else None
    n2_t = _row_count(inds, grad_out)
    _on_device("closest_pool_cat_backward", grad_out=g, inds=idx, out=out, start=start, edges=edges, n1_dev=n1_t, n2_dev=n2_t)
    dev = g.device
    if start is None:
        start, edges = neighbor_transpose_supports(_tag(idx[:, :1], inds), N1, n2_t, n1_t)
    if out is None:
        out, ldo = torch.empty((N1, C1), dtype=torch.float32, device=dev), C1
    with _timed("closest_pool_cat_backward", dict(N1=N1, N2=N2, C1=C1), dev):
        rc = lib.d3f_closest_pool_cat_backward(g.data_ptr(), N2, ldg, C1, idx.data_ptr(), ldi, N1, start.data_ptr(), edges.data_ptr(),
                                               out.data_ptr(), ldo, _ptr(n1_t), _ptr(n2_t), _stream(dev))
    _lib.check(rc, "closest_pool_cat_backward")
    return out


class RawRecords:
    """A cloud still in its file encoding (utils.ply.read_ply_records / utils.results.read_kitti_records): raw bytes + record
    layout.  FragmentEngine.submit takes it wherever it takes a float32 [n,3] cloud and decodes it on the GPU, straight into
    the slot's stage-0 input buffer."""

    def __init__(self, raw, layout, pin=True):
        if not isinstance(raw, torch.Tensor):
            raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.uint8))
        if pin and not raw.is_cuda and torch.cuda.is_available():
            raw = raw.pin_memory()
        self.raw, self.layout = raw, dict(layout)
        self.shape = (int(layout["n"]), 3)
        self.is_cuda = raw.is_cuda

    def decode(self, device=None, out=None):
        return decode_xyz_records(self.raw if device is None or self.raw.is_cuda else self.raw.to(device, non_blocking=True),
                                  self.layout, out=out)


def decode_xyz_records(raw, layout, out=None):
    """Raw file records (uint8 tensor on the device, or pinned / plain host bytes that are copied there asynchronously) ->
    float32 [n,3] on the device.  layout: utils.ply.read_ply_records / utils.results.read_kitti_records."""
    lib = _lib.load()
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    if not isinstance(raw, torch.Tensor):
        raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.uint8))
    if not raw.is_cuda:
        raw = raw.to(dev, non_blocking=True)
    raw = raw.contiguous()
    n, stride = int(layout["n"]), int(layout["stride"])
    if raw.dtype != torch.uint8 or raw.numel() < n * stride:
        raise ValueError("decode_xyz_records: %d bytes for %d records of %d bytes" % (raw.numel(), n, stride))
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    elif out.shape[0] < n or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("decode_xyz_records: output buffer too small or not contiguous float32")
    ox, oy, oz = (int(v) for v in layout["offsets"])
    rc = lib.d3f_decode_xyz_records(raw.data_ptr(), n, stride, ox, oy, oz, 1 if layout["dtype"] == "f8" else 0,
                                    1 if layout.get("big_endian") else 0, out.data_ptr(), _stream(dev))
    _lib.check(rc, "decode_xyz_records")
    return out[:n]


def pack_descriptors(xyz, desc, score, lens=None, group=1, keep=0, dst=None, row_map=None):
    """-> f32[N, 3 + C + 1] records [xyz | desc | score] (one contiguous block per fragment of a stack).
    dst (device int64[fragments] of ADDRESSES, 0 = none) with lens (device i32[B], the stack's clouds), group clouds per fragment:
    the rows of the first `keep` clouds of fragment f are written to the address dst[f] instead (d3f_pack_descriptors_to).
    row_map (device i32[N]): the inputs are in an internal row order, record n is written at row row_map[n]."""
    lib = _lib.load()
    xyz = _req(xyz, torch.float32, "xyz", 2).contiguous()
    desc, ldd = _rows(_req(desc, torch.float32, "desc"), "desc")
    score = _req(score, torch.float32, "score").contiguous()
    N, Cc = desc.shape
    if xyz.shape[0] != N or xyz.shape[1] != 3 or score.numel() != N:
        raise ValueError("pack_descriptors: %s points, %s descriptors, %s scores" % (tuple(xyz.shape), tuple(desc.shape),
                                                                                     tuple(score.shape)))
    out = torch.empty((N, Cc + 4), dtype=torch.float32, device=desc.device)
    if dst is not None or row_map is not None:
        if dst is not None:
            assert dst.dtype == torch.int64 and dst.is_contiguous() and lens is not None and lens.dtype == torch.int32
            assert lens.numel() == dst.numel() * int(group)
        if row_map is not None:
            assert row_map.dtype == torch.int32 and row_map.is_contiguous() and row_map.numel() >= N
        rc = lib.d3f_pack_descriptors_to(xyz.data_ptr(), desc.data_ptr(), ldd, Cc, score.data_ptr(), N, out.data_ptr(), Cc + 4,
                                         _nd(xyz) or _nd(desc), _ptr(lens),
                                         lens.numel() if lens is not None else 0, int(group), int(keep),
                                         _ptr(dst),
                                         _ptr(row_map), _stream(desc.device))
    else:
        rc = lib.d3f_pack_descriptors(xyz.data_ptr(), desc.data_ptr(), ldd, Cc, score.data_ptr(), N, out.data_ptr(), Cc + 4,
                                      _nd(xyz) or _nd(desc), _stream(desc.device))
    _lib.check(rc, "pack_descriptors")
    return _tag(out, desc)


def affine_act(x, col_scale=None, col_shift=None, residual=None, leaky=False, alpha=0.2):
    """out = act(x * col_scale + col_shift + residual): the stand-alone form of the GEMM epilogue."""
    lib = _lib.load()
    x, ldx = _rows(_req(x, torch.float32, "x"), "x")
    M, N = x.shape
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(_req(residual, torch.float32, "residual"), "residual")
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    rc = lib.d3f_affine_act(x.data_ptr(), ldx, M, N, _ptr(col_scale),
                            _ptr(col_shift),
                            _ptr(residual), ldr, 1 if leaky else 0, float(alpha),
                            out.data_ptr(), N, _nd(x), _stream(x.device))
    _lib.check(rc, "affine_act")
    return _tag(out, x)


# ---- training: batch norm with batch statistics, the unary convolution's backward -----------------------------------------
def _col(v, n, name):
    """An optional float32 vector of n columns, contiguous."""
    if v is not None:
        _typed(v, torch.float32, name)
        if v.numel() != n or not v.is_contiguous():
            raise ValueError("%s must be a contiguous vector of %d" % (name, n))
    return v


def _row_count(*tensors):
    """The device-resident row count that rides on the first tagged tensor, or None."""
    for t in tensors:
        d = getattr(t, "n_dev", None) if t is not None else None
        if d is not None:
            return d
    return None


def batch_norm_train(x, gamma, beta, eps=1e-6, residual=None, leaky=False, alpha=0.2, moving_mean=None, moving_variance=None,
                     momentum=0.99, out=None):
    """tf.layers.batch_normalization(training=True) on rows (models/network_blocks.py:149-165) with the block's epilogue ->
    (y, mean f32[2, C], rstd f32[C]): y = act((x - mean) rstd gamma + beta + residual) with the statistics of the real rows, and the
    moving statistics updated in place when both are given.  mean[0] is the batch mean, mean[1] its rounding remainder (the float64
    mean is mean[0] + mean[1]); batch_norm_backward takes the pair as it is.  gamma=None: the form without batch norm, y = act(x + beta + residual),
    mean and rstd are None.  The definition and the summation order: include/d3feat_amd.h (d3f_batch_norm_train).  out may be the
    residual.  Three launches, no read-back, capturable."""
    lib = _lib.load()
    x, ldx = _rows(_typed(x, torch.float32, "x"), "x")
    M, C = x.shape
    if C < 1:
        raise ValueError("batch_norm_train: x is %s" % (tuple(x.shape),))
    gamma, beta = _col(gamma, C, "gamma"), _col(beta, C, "beta")
    if beta is None:
        raise ValueError("batch_norm_train: beta (the offset) is required")
    if (moving_mean is None) != (moving_variance is None):
        raise ValueError("batch_norm_train: moving_mean and moving_variance come together")
    moving_mean, moving_variance = _col(moving_mean, C, "moving_mean"), _col(moving_variance, C, "moving_variance")
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(_typed(residual, torch.float32, "residual"), "residual")
        if tuple(residual.shape) != (M, C):
            raise ValueError("batch_norm_train: residual is %s, wanted %s" % (tuple(residual.shape), (M, C)))
    if out is not None:
        out, ldy = _rows(_typed(out, torch.float32, "out"), "out")
        if tuple(out.shape) != (M, C):
            raise ValueError("batch_norm_train: out is %s, wanted %s" % (tuple(out.shape), (M, C)))
    if gamma is not None and not float(eps) > 0:
        raise ValueError("batch_norm_train: eps = %r" % (eps,))
    n_dev = _row_count(x, residual)
    _on_device("batch_norm_train", x=x, gamma=gamma, beta=beta, residual=residual, out=out, moving_mean=moving_mean,
               moving_variance=moving_variance, n_dev=n_dev)
    dev = x.device
    if out is None:
        out, ldy = torch.empty((M, C), dtype=torch.float32, device=dev), C
    mean = rstd = None
    if gamma is not None:
        mean = torch.empty((2, C), dtype=torch.float32, device=dev)
        rstd = torch.empty((C,), dtype=torch.float32, device=dev)
    else:
        moving_mean = moving_variance = None
    nbytes = lib.d3f_batch_norm_workspace_bytes(M, C)
    ws = workspace(nbytes, dev)
    with _timed("batch_norm_train", dict(M=M, C=C), dev):
        rc = lib.d3f_batch_norm_train(x.data_ptr(), ldx, M, C, _ptr(gamma), beta.data_ptr(), float(eps), float(momentum),
                                      _ptr(moving_mean), _ptr(moving_variance), _ptr(residual), ldr, 1 if leaky else 0, float(alpha),
                                      out.data_ptr(), ldy, _ptr(mean), _ptr(rstd), _ptr(n_dev), ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "batch_norm_train")
    if n_dev is not None and getattr(out, "n_dev", None) is None:
        _tag(out, x if getattr(x, "n_dev", None) is not None else residual)
    return out, mean, rstd


def batch_norm_backward(x, y, grad_y, gamma, mean, rstd, leaky=False, alpha=0.2, need_residual=False, out=None, out_residual=None):
    """Backward of batch_norm_train -> (gx, ggamma, gbeta, gres): from grad_y and the stored y (the LeakyReLU mask is taken from it),
    the gradients with respect to x, gamma, beta and -- need_residual -- the residual (None otherwise).  gamma=None: the form without
    batch norm, ggamma is None and gx is the masked gradient.  out (for gx) may be grad_y; out_residual (for gres) may be grad_y when
    out is not.  The definition: include/d3feat_amd.h
    (d3f_batch_norm_backward).  Two launches, no read-back, capturable."""
    lib = _lib.load()
    g, ldg = _rows(_typed(grad_y, torch.float32, "grad_y"), "grad_y")
    M, C = g.shape
    if C < 1:
        raise ValueError("batch_norm_backward: grad_y is %s" % (tuple(g.shape),))
    ldx = ldy = 0
    if gamma is not None:
        x, ldx = _rows(_typed(x, torch.float32, "x"), "x")
        gamma, mean, rstd = _col(gamma, C, "gamma"), _col(mean, 2 * C, "mean"), _col(rstd, C, "rstd")
        if mean is None or rstd is None:
            raise ValueError("batch_norm_backward: mean and rstd of the forward are required with gamma")
    else:
        x = mean = rstd = None
    if leaky:
        y, ldy = _rows(_typed(y, torch.float32, "y"), "y")
    else:
        y = None
    for t, name in ((x, "x"), (y, "y")):
        if t is not None and tuple(t.shape) != (M, C):
            raise ValueError("batch_norm_backward: %s is %s, grad_y %s" % (name, tuple(t.shape), (M, C)))
    if out is not None:
        out, ldgx = _rows(_typed(out, torch.float32, "out"), "out")
        if tuple(out.shape) != (M, C):
            raise ValueError("batch_norm_backward: out is %s, wanted %s" % (tuple(out.shape), (M, C)))
    gres, ldgr = None, C
    if need_residual and out_residual is not None:
        gres, ldgr = _rows(_typed(out_residual, torch.float32, "out_residual"), "out_residual")
        if tuple(gres.shape) != (M, C):
            raise ValueError("batch_norm_backward: out_residual is %s, wanted %s" % (tuple(gres.shape), (M, C)))
    n_dev = _row_count(grad_y, x, y)
    _on_device("batch_norm_backward", x=x, y=y, grad_y=g, gamma=gamma, mean=mean, rstd=rstd, out=out, out_residual=gres, n_dev=n_dev)
    dev = g.device
    if out is None:
        out, ldgx = torch.empty((M, C), dtype=torch.float32, device=dev), C
    gbeta = torch.empty((C,), dtype=torch.float32, device=dev)
    ggamma = torch.empty((C,), dtype=torch.float32, device=dev) if gamma is not None else None
    if need_residual and gres is None:
        gres = torch.empty((M, C), dtype=torch.float32, device=dev)
    nbytes = lib.d3f_batch_norm_workspace_bytes(M, C)
    ws = workspace(nbytes, dev)
    with _timed("batch_norm_backward", dict(M=M, C=C), dev):
        rc = lib.d3f_batch_norm_backward(_ptr(x), ldx, _ptr(y), ldy, g.data_ptr(), ldg, M, C, _ptr(gamma), _ptr(mean), _ptr(rstd),
                                         1 if leaky else 0, float(alpha), out.data_ptr(), ldgx, _ptr(ggamma), gbeta.data_ptr(), _ptr(gres),
                                         ldgr, _ptr(n_dev), ws.data_ptr(), nbytes, _stream(dev))
    _lib.check(rc, "batch_norm_backward")
    if n_dev is not None:
        for t in (out, gres):
            if t is not None and getattr(t, "n_dev", None) is None:
                t.n_dev = n_dev
                t.n_hint = max(int(getattr(s, "n_hint", 0) or 0) for s in (grad_y, x, y) if s is not None)
    return out, ggamma, gbeta, gres


def gemm_tn(A, B, out=None):
    """A^T B f32[Ca, Cb] over the real rows of A f32[n, Ca] and B f32[n, Cb] (rows may be strided): the contraction of
    kpconv_backward's gW -- slices of rows in order, equal bits from call to call (include/d3feat_amd.h, d3f_gemm_tn_f32)."""
    lib = _lib.load()
    A, lda = _rows(_typed(A, torch.float32, "A"), "A")
    B, ldb = _rows(_typed(B, torch.float32, "B"), "B")
    if A.shape[0] != B.shape[0] or A.shape[1] < 1 or B.shape[1] < 1:
        raise ValueError("gemm_tn: A is %s, B is %s" % (tuple(A.shape), tuple(B.shape)))
    (M, Ca), Cb = A.shape, B.shape[1]
    if out is not None:
        _typed(out, torch.float32, "out", 2)
        if tuple(out.shape) != (Ca, Cb) or not out.is_contiguous():
            raise ValueError("gemm_tn: out must be contiguous %s" % ((Ca, Cb),))
    n_dev = _row_count(A, B)
    _on_device("gemm_tn", A=A, B=B, out=out, n_dev=n_dev)
    dev = A.device
    if out is None:
        out = torch.empty((Ca, Cb), dtype=torch.float32, device=dev)
    nbytes = lib.d3f_gemm_tn_workspace_bytes(M, Ca, Cb)
    ws = workspace(nbytes, dev)
    with _timed("gemm_tn", dict(M=M, Ca=Ca, Cb=Cb), dev):
        rc = lib.d3f_gemm_tn_f32(A.data_ptr(), lda, B.data_ptr(), ldb, M, Ca, Cb, out.data_ptr(), _ptr(n_dev), ws.data_ptr(), nbytes,
                                 _stream(dev))
    _lib.check(rc, "gemm_tn")
    return out


def unary_backward(x, W, grad_y, need_input=True, need_weights=True):
    """Backward of the unary convolution y = x W (W f32[Cin, Cout]) -> (gx = grad_y W^T or None, gW = x^T grad_y or None).  gx is
    ops.gemm on a transposed copy of W (its packed copies are keyed on the tensor and its version, so a fresh transpose per call is
    safe); gW is gemm_tn."""
    _typed(W, torch.float32, "W", 2)
    if tuple(grad_y.shape) != (x.shape[0], W.shape[1]) or x.shape[1] != W.shape[0]:
        raise ValueError("unary_backward: x is %s, W %s, grad_y %s" % (tuple(x.shape), tuple(W.shape), tuple(grad_y.shape)))
    if not (need_input or need_weights):
        raise ValueError("unary_backward: neither gradient is wanted")
    gx = gW = None
    if need_input:
        g = grad_y if getattr(grad_y, "n_dev", None) is not None else _tag(grad_y.detach(), x)
        with f32_output():
            gx = gemm(g, W.detach().t().contiguous())
    if need_weights:
        gW = gemm_tn(x, grad_y)
    return gx, gW


def momentum_sgd_plan(counts):
    """The chunk table of momentum_sgd_step for variables of `counts` elements -> i32[nchunks, 2] on the HOST, (variable, first element)
    per chunk of _lib.SGD_CHUNK elements: a variable's chunks are contiguous and in element order (d3f_momentum_sgd_plan).  Host only."""
    lib = _lib.load()
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    n = lib.d3f_momentum_sgd_plan(counts.ctypes.data, counts.size, None, 0)
    if n < 0:
        _lib.check(n, "momentum_sgd_plan")
    table = np.zeros((n, 2), np.int32)
    rc = lib.d3f_momentum_sgd_plan(counts.ctypes.data, counts.size, table.ctypes.data, n)
    if rc != n:
        _lib.check(min(rc, -3), "momentum_sgd_plan")
    return table


def momentum_sgd_workspace_bytes(num_variables, num_chunks):
    return int(_lib.load().d3f_momentum_sgd_workspace_bytes(int(num_variables), int(num_chunks)))


def momentum_sgd_step(desc, chunks, hyper, zero_grad=False, reg_loss=None, ws=None):
    """One optimiser step of every variable in one call (include/d3feat_amd.h, d3f_momentum_sgd): desc i64[T, 4] on the device, one
    descriptor per variable (the addresses of v, g -- 0: skipped -- and a, then count + (decay << 32)); chunks i32[nchunks, 2] on the
    device (momentum_sgd_plan of the same counts); hyper f32[4] on the device, {lr, mom, clip, wd}; reg_loss f32[1] or None; ws: a byte
    buffer of momentum_sgd_workspace_bytes(T, nchunks) that the caller owns (a captured call keeps its own), else the shared scratch.
    Two launches, no read-back, capturable.  Nothing is returned: v, a (and g with zero_grad) are rewritten in place."""
    lib = _lib.load()
    _typed(desc, torch.int64, "desc", 2)
    _typed(chunks, torch.int32, "chunks", 2)
    _typed(hyper, torch.float32, "hyper", 1)
    if desc.shape[1] != 4 or chunks.shape[1] != 2 or hyper.numel() != 4 or not (desc.is_contiguous() and chunks.is_contiguous() and hyper.is_contiguous()):
        raise ValueError("momentum_sgd_step: desc is %s, chunks %s, hyper %s" % (tuple(desc.shape), tuple(chunks.shape), tuple(hyper.shape)))
    if reg_loss is not None and _typed(reg_loss, torch.float32, "reg_loss").numel() != 1:
        raise ValueError("momentum_sgd_step: reg_loss must hold one float")
    _on_device("momentum_sgd_step", desc=desc, chunks=chunks, hyper=hyper, reg_loss=reg_loss, ws=ws)
    dev = desc.device
    T, nchunks = desc.shape[0], chunks.shape[0]
    nbytes = lib.d3f_momentum_sgd_workspace_bytes(T, nchunks)
    if ws is None:
        ws = workspace(nbytes, dev)
    elif ws.dtype != torch.uint8 or ws.numel() < nbytes:
        raise ValueError("momentum_sgd_step: ws must be a uint8 buffer of at least %d bytes" % nbytes)
    with _timed("momentum_sgd_step", dict(T=T, nchunks=nchunks), dev):
        rc = lib.d3f_momentum_sgd(desc.data_ptr(), T, chunks.data_ptr(), nchunks, hyper.data_ptr(), 1 if zero_grad else 0, _ptr(reg_loss),
                                  ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "momentum_sgd_step")
