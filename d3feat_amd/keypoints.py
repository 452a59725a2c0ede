"""Keypoint selection on the device: the K records of a cloud with the highest detection scores, in ascending score order.

The reference's testers order a fragment's rows by score (utils/tester.py:208-213, demo_registration.py:159-163:
np.argsort(scores)) and every consumer keeps the tail (geometric_registration/evaluate.py:45-50 [-num_keypts:],
utils/tester.py:283-284, demo_registration.py:249,261).  One definition, for one cloud with scores s and K >= 1:

    sel = np.argsort(s, kind="stable")[-K:]          # min(n, K) rows
    out = records[sel]                               # ascending score; ties in ascending row index

    topk(xyz, desc, score, K, ...)        separate arrays (the form the fragment engine captures into its replay)
    topk_records(records, K, ...)         a finished [xyz | desc | score] block, or a stack of blocks with `lens`

Both are ONE launch of d3f_topk_records (csrc/keypoints.hip) for all kept clouds of the stack; nothing is read back here.
"""
import torch

from . import _lib, ops


_TICKETS = {}


def _tickets(device):
    """Ticket counters of the multi-workgroup form (d3f_topk_records: zero before the first call, left zero by every call), one
    block per (device, stream): calls on one stream run one after the other, calls on different streams never share a counter.
    Made by the first eager call on a stream -- the fragment engine's warm-up -- so a capture only ever finds it."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), ops._stream(device))
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros((_lib.MAX_BATCH + 1,), dtype=torch.int32, device=device)
    return t


def _clouds(B, group, keep):
    return -(-int(B) // int(group)) * int(keep)


def topk(xyz, desc, score, K, lens=None, group=1, keep=None, row_map=None, out=None, count=None, idx=None, return_index=False,
         n_cap=None):
    """xyz f32[N,3], desc f32[N,C], score f32[N] / [N,1] (any row strides: column views of a record block are fine) of a stack of
    B clouds, lens device i32[B] (None: one cloud of N rows).  A fragment is `group` consecutive clouds, its first `keep` (default:
    all) are kept.  row_map (device i32[N]): the inputs are in an internal row order, input row n is reference row row_map[n]
    (ops.pack_descriptors' meaning); ties and the returned indices follow the reference rows.
    -> (kp f32[clouds, K, C + 4], count i32[clouds]) device tensors (+ idx i32[clouds, K], the reference row inside the cloud, with
    return_index or idx=): kp[j, :count[j]] are cloud j's min(n_j, K) records, rows beyond are not written.
    out / count / idx: caller-owned static buffers (the capturable form); n_cap: upper bound of one cloud's rows (default N).
    The scratch comes from ops.workspace (inside ops.private_workspace: the capture's own)."""
    lib = _lib.load()
    xyz, ldx = ops._rows(ops._req(xyz, torch.float32, "xyz", 2), "xyz")
    desc, ldd = ops._rows(ops._req(desc, torch.float32, "desc", 2), "desc")
    score = ops._req(score, torch.float32, "score")
    dev = desc.device
    N, C = desc.shape
    if score.dim() == 2 and score.shape[1] == 1:
        score = score[:, 0]
    if xyz.shape[0] != N or xyz.shape[1] != 3 or score.dim() != 1 or score.shape[0] != N:
        raise ValueError("topk: %s points, %s descriptors, %s scores" % (tuple(xyz.shape), tuple(desc.shape), tuple(score.shape)))
    lds = int(score.stride(0)) if N > 1 else 1
    if lds < 1:
        raise ValueError("topk: score has overlapping rows")
    K = int(K)
    if not 1 <= K <= _lib.TOPK_MAX:
        raise ValueError("topk: K = %d outside 1..%d" % (K, _lib.TOPK_MAX))
    if lens is None:
        lens = ops.as_lens([N], dev)
    lens = ops._req(lens, torch.int32, "lens", 1).contiguous()
    B, group = int(lens.numel()), int(group)
    keep = group if keep is None else int(keep)
    if group < 1 or not 1 <= keep <= group:
        raise ValueError("topk: group %d keep %d" % (group, keep))
    nc = _clouds(B, group, keep)
    W = C + 4
    if out is None:
        out = torch.empty((nc, K, W), dtype=torch.float32, device=dev)
    else:
        ops._req(out, torch.float32, "out", 3)
        if out.shape[0] < nc or out.shape[1] != K or out.shape[2] < W or out.stride(2) != 1 or out.stride(0) != K * out.stride(1):
            raise ValueError("topk: out %s strides %s for %d clouds of %d records of %d floats" % (tuple(out.shape), out.stride(), nc, K, W))
    ldo = int(out.stride(1))
    if count is None:
        count = torch.empty((nc,), dtype=torch.int32, device=dev)
    else:
        ops._req(count, torch.int32, "count", 1)
        assert count.is_contiguous() and count.numel() >= nc
    if idx is None and return_index:
        idx = torch.empty((nc, K), dtype=torch.int32, device=dev)
    if idx is not None:
        ops._req(idx, torch.int32, "idx", 2)
        assert idx.is_contiguous() and idx.shape[0] >= nc and idx.shape[1] == K
    if row_map is not None:
        ops._req(row_map, torch.int32, "row_map", 1)
        assert row_map.is_contiguous() and row_map.numel() >= N
    n_cap = int(N if n_cap is None else n_cap)
    ws = ops.workspace(lib.d3f_topk_workspace_bytes(N, B, n_cap, K), dev)
    rc = lib.d3f_topk_records(xyz.data_ptr(), ldx, desc.data_ptr(), ldd, C, score.data_ptr(), lds, N, ops._nd(xyz) or ops._nd(desc),
                              lens.data_ptr(), B, group, keep, ops._ptr(row_map), n_cap, K, out.data_ptr(), ldo, ops._ptr(idx),
                              count.data_ptr(), _tickets(dev).data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(dev))
    _lib.check(rc, "topk_records")
    return (out, count, idx) if (return_index or idx is not None) else (out, count)


def topk_records(records, K, lens=None, group=1, keep=None, return_index=False):
    """records: a device f32[N, 3 + C + 1] block of [xyz | desc | score] rows (ops.pack_descriptors, FragmentEngine.fetch(packed=True)),
    or a stack of such blocks with `lens` (device i32[B] or a host list).  -> (kp f32[clouds, K, ld], count i32[clouds]) device tensors
    (and idx i32[clouds, K] with return_index): see topk.  No host read-back."""
    rec, _ = ops._rows(ops._req(records, torch.float32, "records", 2), "records")
    if rec.shape[1] < 5:
        raise ValueError("topk_records: records of %d floats" % rec.shape[1])
    if lens is not None and not isinstance(lens, torch.Tensor):
        lens = ops.as_lens(lens, rec.device)
    w = rec.shape[1]
    return topk(rec[:, :3], rec[:, 3:w - 1], rec[:, w - 1], K, lens=lens, group=group, keep=keep, return_index=return_index)
