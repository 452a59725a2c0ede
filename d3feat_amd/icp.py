"""Point-to-point ICP of many (source, target) pairs, run to convergence on the device in one call (d3f_icp_pairs).

The definition is in include/d3feat_amd.h: Open3D's registration_icp with TransformationEstimationPointToPoint(False) and
ICPConvergenceCriteria, restated (tests/icp_np.py is the same text in numpy).  The reference refines the KITTI ground truth with it
(datasets/KITTI.py:293-297); d3feat_amd.datasets.kitti.refine_pairs is that use.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops

# datasets/KITTI.py:295-297: registration_icp(pcd0, pcd1, 0.2, eye(4), PointToPoint(), ICPConvergenceCriteria(max_iteration=200))
ICP_KITTI = dict(max_correspondence_distance=0.2, max_iteration=200, relative_fitness=1e-6, relative_rmse=1e-6)


class PairICP:
    """Results of icp_pairs for P pairs.  The device tensors are in `.dev` (T f64[P,12], count, sumd2, fitness, rmse, iterations,
    converged, nearest i32[N_src]); the properties copy them to the host."""

    def __init__(self, dev, src_lens):
        self.dev = dev
        self._src_lens = src_lens           # device i32[P]

    def __len__(self):
        return self.dev["T"].shape[0]

    @property
    def transformation(self):
        """f64[P, 4, 4], source -> target."""
        T = self.dev["T"].cpu().numpy().reshape(-1, 3, 4)
        out = np.zeros((T.shape[0], 4, 4))
        out[:, :3] = T
        out[:, 3, 3] = 1.0
        return out

    fitness = property(lambda self: self.dev["fitness"].cpu().numpy())
    inlier_rmse = property(lambda self: self.dev["rmse"].cpu().numpy())
    iterations = property(lambda self: self.dev["iterations"].cpu().numpy())
    converged = property(lambda self: self.dev["converged"].cpu().numpy().astype(bool))
    count = property(lambda self: self.dev["count"].cpu().numpy())
    sumd2 = property(lambda self: self.dev["sumd2"].cpu().numpy())

    def correspondences(self, p):
        """i32[n, 2]: rows (source index, target index), both inside pair p's clouds, ascending by source index -- Open3D's
        correspondence_set under the returned transformation."""
        lens = np.maximum(np.asarray(ops.host_lens(self._src_lens), np.int64), 0)
        off = int(lens[:p].sum())
        nn = self.dev["nearest"][off: off + int(lens[p])].cpu().numpy()
        i = np.nonzero(nn >= 0)[0]
        return np.stack([i, nn[i]], axis=1).astype(np.int32)


def _points(a, name, device):
    if isinstance(a, torch.Tensor):
        return ops._req(a, torch.float32, name, 2).contiguous()
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    return torch.from_numpy(a).to(device)


def _init(init, P, device):
    if init is None:
        return torch.eye(4, dtype=torch.float64, device=device)[:3].reshape(1, 12).repeat(P, 1).contiguous()
    if isinstance(init, torch.Tensor):
        t = ops._req(init, torch.float64, "init")
    else:
        t = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).to(device)
    if t.dim() == 3 and tuple(t.shape[1:]) == (4, 4):
        t = t[:, :3, :]
    t = t.reshape(-1, 12).contiguous()
    if t.shape[0] != P:
        raise ValueError("init: %d transforms for %d pairs" % (t.shape[0], P))
    return t


def grid_radius(r):
    """The smallest float32 that is >= r: a grid built with it has cells wider than the float64 radius (include/d3feat_amd.h)."""
    f = np.float32(r)
    return float(f if float(f) >= float(r) else np.nextafter(f, np.float32(np.inf)))


def icp_pairs(src, src_lens, tgt, tgt_lens, init=None, check_every=8, max_correspondence_distance=0.2, max_iteration=200,
              relative_fitness=1e-6, relative_rmse=1e-6, device=None):
    """ICP of pair p = (source cloud p, target cloud p) for every p, all on the device -> PairICP.

    src f32[N_src, 3] / tgt f32[N_tgt, 3]: the stacked clouds (numpy, or torch tensors on the GPU); src_lens / tgt_lens: P lengths each.
    Lengths given on the host must be non-negative and add up to the rows of their stack (ValueError); lengths that only exist on the
    device are taken as they are, a length running past the stack is cut there.  init: None (identity), or f64[P, 4, 4] / [P, 3, 4] / [P, 12].  More than 255 pairs are run in chunks (the lengths are then needed on
    the host).  check_every=n > 0: the host looks every n rounds whether every pair has stopped; 0: max_iteration + 1 rounds are
    enqueued without any read-back -- with device tensors for every input the call can then be captured in a graph.  Same bits either way.
    """
    lib = _lib.load()
    # lengths known on the host are checked against the rows before anything touches the device: the kernel would cut a length that
    # runs past the stack, and correspondences(p) would then slice by lengths that are not the ones used
    for what, pts, lens in (("src", src, src_lens), ("tgt", tgt, tgt_lens)):
        host = getattr(lens, "host_lens", None) if isinstance(lens, torch.Tensor) else [int(x) for x in np.asarray(lens).reshape(-1)]
        rows = pts.shape[0] if isinstance(pts, torch.Tensor) else np.asarray(pts).reshape(-1, 3).shape[0]
        if host is not None and (min(host, default=0) < 0 or sum(host) != rows):
            raise ValueError("icp_pairs: %s_lens %s do not add up to the %d rows of %s" % (what, "sum to %d" % sum(host), rows, what))
    dev = device
    if dev is None:
        dev = src.device if isinstance(src, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    src, tgt = _points(src, "src", dev), _points(tgt, "tgt", dev)
    sl, tl = ops.as_lens(src_lens, dev), ops.as_lens(tgt_lens, dev)
    P = sl.numel()
    if tl.numel() != P:
        raise ValueError("icp_pairs: %d source and %d target clouds" % (P, tl.numel()))
    r = float(max_correspondence_distance)
    if not r > 0.0 or int(max_iteration) < 0 or int(check_every) < 0:
        raise ValueError("icp_pairs: max_correspondence_distance > 0, max_iteration >= 0 and check_every >= 0 are required")
    T0 = _init(init, P, dev)
    crit = (ctypes.c_double * 3)(r, float(relative_fitness), float(relative_rmse))
    out = dict(T=torch.empty((P, 12), dtype=torch.float64, device=dev), nearest=torch.full((src.shape[0],), -1, dtype=torch.int32, device=dev))
    for name, dt in (("count", torch.int32), ("sumd2", torch.float64), ("fitness", torch.float64), ("rmse", torch.float64),
                     ("iterations", torch.int32), ("converged", torch.int32)):
        out[name] = torch.empty((P,), dtype=dt, device=dev)
    if P == 0:
        return PairICP(out, sl)
    if P <= _lib.MAX_BATCH:
        chunks = [(0, P, 0, src.shape[0], 0, tgt.shape[0])]
    else:
        hs, ht = np.asarray(ops.host_lens(sl), np.int64), np.asarray(ops.host_lens(tl), np.int64)
        os_, ot = np.concatenate([[0], np.cumsum(hs)]), np.concatenate([[0], np.cumsum(ht)])
        chunks = [(a, min(a + _lib.MAX_BATCH, P)) for a in range(0, P, _lib.MAX_BATCH)]
        chunks = [(a, b, int(os_[a]), int(os_[b]), int(ot[a]), int(ot[b])) for a, b in chunks]
    stream = ops._stream(dev)
    for a, b, s0, s1, t0, t1 in chunks:
        B, n_src, n_tgt = b - a, s1 - s0, t1 - t0
        grid = ops.NeighborGrid(tgt[t0:t1], tl[a:b], grid_radius(r))
        wsb = lib.d3f_icp_pairs_workspace_bytes(n_src, B)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        s_rows = src[s0:s1]
        rc = lib.d3f_icp_pairs(grid.mem.data_ptr(), grid.nbytes, n_tgt, s_rows.data_ptr() if n_src else None, n_src, sl[a:b].data_ptr(), B,
                               T0[a:b].data_ptr(), ctypes.addressof(crit), int(max_iteration), int(check_every), out["T"][a:b].data_ptr(),
                               *(out[k][a:b].data_ptr() for k in ("count", "sumd2", "fitness", "rmse", "iterations", "converged")),
                               out["nearest"][s0:s1].data_ptr() if n_src else None, ws.data_ptr(), wsb, stream)
        _lib.check(rc, "icp_pairs")
    return PairICP(out, sl)
