"""Pairwise feature distances and the validation metric (interface of lib/metrics.py:13-29).

``pdist`` keeps the reference's signature and returns the full [M, M'] matrix (torch ops, compatibility only);
the hot path never materialises it: ``pdist_min`` returns the row minimum and arg-minimum from one HIP kernel
(the only way the reference consumes pdist on the hot path: lib/colocation_trainer.py:510-512, lib/eval.py:25-29).
"""
import ctypes

import torch

from gcl_amd import _lib


def corr_dist(est, gth, xyz0, xyz1, weight=None, max_dist=1):
    """Mean (clamped) distance between the points moved by the estimated and by the true transformation
    (lib/metrics.py:13-19; the validation step's "loss", lib/colocation_trainer.py:343).  ``xyz1`` is unused, as there."""
    moved_est = xyz0 @ est[:3, :3].t() + est[:3, 3]
    moved_gth = xyz0 @ gth[:3, :3].t() + gth[:3, 3]
    dists = torch.clamp(torch.sqrt(((moved_est - moved_gth) ** 2).sum(1)), max=max_dist)
    if weight is not None:
        dists = weight * dists
    return dists.mean()


def pdist(A, B, dist_type="L2"):
    if dist_type not in ("L2", "SquareL2"):
        raise NotImplementedError("Not implemented")
    out = torch.empty((A.shape[0], B.shape[0]), dtype=A.dtype, device=A.device)
    step = max(1, (1 << 26) // max(1, B.shape[0] * A.shape[1]))        # bound the broadcast temp to 256 MB
    for i in range(0, A.shape[0], step):
        out[i:i + step] = torch.sum((A[i:i + step].unsqueeze(1) - B.unsqueeze(0)).pow(2), 2)
    return torch.sqrt(out + 1e-7) if dist_type == "L2" else out


def pdist_min(A, B, dist_type="L2", rows_a=None, rows_b=None):
    """Row-wise (min, argmin) of pdist(A[rows_a], B[rows_b]) without forming the matrix.  Ties -> lowest index."""
    lib = _lib.require_gpu()
    if dist_type not in ("L2", "SquareL2"):
        raise NotImplementedError("Not implemented")
    A, B = A.detach().contiguous(), B.detach().contiguous()
    ma = A.shape[0] if rows_a is None else rows_a.shape[0]
    mb = B.shape[0] if rows_b is None else rows_b.shape[0]
    dmin = torch.empty(ma, dtype=torch.float32, device=A.device)
    arg = torch.empty(ma, dtype=torch.int32, device=A.device)
    c = A.shape[1]
    if c in (16, 32, 64):                      # the widths of the networks: the kernel instantiated for exactly that width
        ns, fn, name = lib.gcl_nn_rowmin_scratch_len(ma, mb), lib.gcl_nn_rowmin, "gcl_nn_rowmin"
    else:                                      # any other width up to 128 (an FPFH descriptor has 33 channels)
        ns, fn, name = lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c), lib.gcl_nn_rowmin_any, "gcl_nn_rowmin_any"
    scratch = torch.empty(ns, dtype=torch.int32, device=A.device) if ns else None
    _lib.check(fn(_lib.ptr(A, torch.float32), _lib.ptr(rows_a, torch.int64), ma,
                  _lib.ptr(B, torch.float32), _lib.ptr(rows_b, torch.int64), mb, c,
                  1 if dist_type == "L2" else 0, _lib.ptr(scratch), _lib.ptr(dmin), _lib.ptr(arg),
                  _lib.stream()), name)
    return dmin, arg


def device_table(records, device):
    """A ctypes array of records (``_lib.NnSearch`` / ``_lib.MutualJob``) on ``device``, through the pinned staging helper
    (no pageable copy, the enqueuing thread does not stop); the bytes are taken when this is called."""
    import numpy as np
    from gcl_amd.lib.eval import host_to_device          # lib/eval.py imports this module
    return host_to_device(np.frombuffer(records, dtype=np.uint8), device)


def mutual_jobs(pairs, device):
    """The ``gcl_mutual_job`` table of ``pairs`` (dicts of tensors / sizes, missing = NULL) on the host and on ``device``."""
    recs = (_lib.MutualJob * len(pairs))()
    for r, job in zip(recs, pairs):
        for name, value in job.items():
            setattr(r, name, value if isinstance(value, int) else _lib.ptr(value))
    return recs, device_table(recs, device)


def pdist_min_batch(problems, dist_type="L2"):
    """``pdist_min`` for a ragged batch of searches in the launches of one (``gcl_nn_rowmin_batch``): one scratch
    allocation, one table copy, one native call, nothing read back.  ``problems``: a sequence of ``(A, B)``,
    ``(A, B, rows_a, rows_b)`` (either may be None) or ``(A, B, rows_a, rows_b, pts_a, pts_b, src_out, tgt_out)`` -- the fused
    gather ``src_out[r] = pts_a[rows_a[r]]``, ``tgt_out[r] = pts_b[rows_b[argmin[r]]]`` into contiguous float32 [ma, 3]
    tensors of the caller's (slices of a batch's padded buffers; None: allocated here).  All searches share the width.
    Returns per search ``(dmin, argmin)`` -- views of one allocation each -- or ``(dmin, argmin, src, tgt)``; every search's
    result is bitwise ``pdist_min``'s."""
    lib = _lib.require_gpu()
    if dist_type not in ("L2", "SquareL2"):
        raise NotImplementedError("Not implemented")
    P = len(problems)
    if P < 1:
        raise ValueError("pdist_min_batch needs at least one search")
    recs = (_lib.NnSearch * P)()
    keep, sizes, c, dev = [], [], None, None          # keep: contiguous copies made here stay alive until the call is enqueued
    f32, i64 = torch.float32, torch.int64
    for i, prob in enumerate(problems):
        if len(prob) not in (2, 4, 8):
            raise ValueError(f"search {i}: expected (A, B), (A, B, rows_a, rows_b) or (A, B, rows_a, rows_b, pts_a, pts_b, "
                             f"src_out, tgt_out), got {len(prob)} entries")
        A, B = prob[0].detach().contiguous(), prob[1].detach().contiguous()
        rows_a, rows_b = (prob[2], prob[3]) if len(prob) > 2 else (None, None)
        if c is None:
            c, dev = A.shape[1], A.device
        if A.shape[1] != c or B.shape[1] != c:
            raise ValueError(f"search {i}: all searches of a call share the width ({c}), got {A.shape[1]} and {B.shape[1]}")
        ma = A.shape[0] if rows_a is None else rows_a.shape[0]
        mb = B.shape[0] if rows_b is None else rows_b.shape[0]
        r = recs[i]
        r.a, r.rows_a, r.ma = _lib.ptr(A, f32), _lib.ptr(rows_a, i64), ma
        r.b, r.rows_b, r.mb = _lib.ptr(B, f32), _lib.ptr(rows_b, i64), mb
        src = tgt = None
        if len(prob) == 8:
            pts_a, pts_b = prob[4].detach().contiguous(), prob[5].detach().contiguous()
            src = torch.empty((ma, 3), dtype=f32, device=dev) if prob[6] is None else prob[6]
            tgt = torch.empty((ma, 3), dtype=f32, device=dev) if prob[7] is None else prob[7]
            if tuple(src.shape) != (ma, 3) or tuple(tgt.shape) != (ma, 3):
                raise ValueError(f"search {i}: src_out / tgt_out must be [{ma}, 3]")
            r.pts_a, r.pts_b, r.src, r.tgt = _lib.ptr(pts_a, f32), _lib.ptr(pts_b, f32), _lib.ptr(src, f32), _lib.ptr(tgt, f32)
            keep += [pts_a, pts_b]
        keep += [A, B]
        sizes.append((ma, src, tgt))
    total = sum(max(ma, 0) for ma, _, _ in sizes)
    dmin = torch.empty(total, dtype=f32, device=dev)
    arg = torch.empty(total, dtype=torch.int32, device=dev)
    out, off = [], 0
    for i, (ma, src, tgt) in enumerate(sizes):
        d, a = dmin[off:off + ma], arg[off:off + ma]
        recs[i].dmin, recs[i].argmin = d.data_ptr(), a.data_ptr()
        out.append((d, a) if src is None else (d, a, src, tgt))
        off += ma
    ns = lib.gcl_nn_rowmin_batch_scratch_len(ctypes.addressof(recs), P, c)      # fills the records' scratch offsets
    scratch = torch.empty(ns, dtype=torch.int32, device=dev) if ns else None
    table = device_table(recs, dev)
    _lib.check(lib.gcl_nn_rowmin_batch(ctypes.addressof(recs), _lib.ptr(table), P, c, 1 if dist_type == "L2" else 0,
                                       _lib.ptr(scratch), _lib.stream()), "gcl_nn_rowmin_batch")
    return out


def nn3_min(Q, P, feats=None):
    """Nearest row of ``P`` [n, 3] for every row of ``Q`` [m, 3]: ``(d2min float32 [m], argmin int32 [m])`` on the device,
    squared distances in the difference form, ties -> lowest index (generalization_ETH/evaluate.py:110-122: pytorch3d's
    knn_points with K = 1).  With ``feats`` [n, c] the same native call also returns ``desc = feats[argmin]`` [m, c]."""
    lib = _lib.require_gpu()
    Q, P = Q.detach().to(torch.float32).contiguous(), P.detach().to(torch.float32).contiguous()
    if Q.dim() != 2 or P.dim() != 2 or Q.shape[1] != 3 or P.shape[1] != 3:
        raise ValueError(f"nn3_min takes [m, 3] and [n, 3] points, got {tuple(Q.shape)} and {tuple(P.shape)}")
    m, n = Q.shape[0], P.shape[0]
    d2 = torch.empty(m, dtype=torch.float32, device=Q.device)
    arg = torch.empty(m, dtype=torch.int32, device=Q.device)
    desc, c = None, 0
    if feats is not None:
        feats = feats.detach().contiguous()
        if feats.dim() != 2 or feats.shape[0] != n:
            raise ValueError(f"nn3_min: feats must be [n = {n}, c], got {tuple(feats.shape)}")
        c = feats.shape[1]
        desc = torch.empty((m, c), dtype=torch.float32, device=Q.device)
    if m == 0:
        return (d2, arg) if feats is None else (d2, arg, desc)
    ns = lib.gcl_nn3_scratch_len(m, n)
    scratch = torch.empty(ns, dtype=torch.int32, device=Q.device) if ns else None
    _lib.check(lib.gcl_nn3_rowmin(_lib.ptr(Q), m, _lib.ptr(P), n, _lib.ptr(feats, torch.float32), c, _lib.ptr(scratch),
                                  _lib.ptr(d2), _lib.ptr(arg), _lib.ptr(desc), _lib.stream()), "gcl_nn3_rowmin")
    return (d2, arg) if feats is None else (d2, arg, desc)
