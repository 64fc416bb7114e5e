"""``util/pointcloud.py`` of the reference, on the device: ``get_matching_indices`` (:53-66), the ground-truth
correspondences every pair dataset hands to the pair trainers (lib/data_loaders.py:256, :506).

The reference moves the source cloud by ``trans`` and runs one open3d KD-tree radius query per point.  Here the target cloud
is a VOXELISED cloud -- one point per voxel of edge ``voxel_size``, which is what the datasets pass (lib/data_loaders.py:498-503)
-- and its coordinate hash table answers a radius query by a scan of the voxels around the query point
(csrc/pairmatch.hip).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.colocation_data_gpu import _cap

STATUS_TEXT = {1: "offsets are not 0 <= o[b] <= o[b+1] <= total", 2: "a radius is not in (0, radius_max]"}


def pack_params(offsets0, offsets1, trans, radii, table_row0=None):
    """The small per-batch arrays of the kernels in ONE pinned block of 8-byte words, so that they travel in one copy:
    offsets0 [B+1], offsets1 [B+1], table_row0 [B], trans [B, 12] (fp64, row-major 3 x 4), radii [B].
    Returns (pinned int64 tensor, {name: (first word, words)})."""
    B = len(radii)
    T = np.asarray(trans, dtype=np.float64).reshape(B, -1, 4)[:, :3, :].reshape(B, 12)
    lay, at = {}, 0
    for name, words in (("offsets0", B + 1), ("offsets1", B + 1), ("table_row0", B), ("trans", 12 * B), ("radii", B)):
        lay[name] = (at, words)
        at += words
    host = torch.empty(at, dtype=torch.int64, pin_memory=True)
    hi = host.numpy()
    hf = hi.view(np.float64)
    a, w = lay["offsets0"]
    hi[a:a + w] = np.asarray(offsets0, dtype=np.int64)
    a, w = lay["offsets1"]
    hi[a:a + w] = np.asarray(offsets1, dtype=np.int64)
    a, w = lay["table_row0"]
    hi[a:a + w] = np.asarray(offsets1 if table_row0 is None else table_row0, dtype=np.int64)[:B]
    a, w = lay["trans"]
    hf[a:a + w] = T.reshape(-1)
    a, w = lay["radii"]
    hf[a:a + w] = np.asarray(radii, dtype=np.float64)
    return host, lay


def matches_on_device(xyz0, xyz1, params, layout, n_pairs, table, cap, voxel_size, radius_max, K=None, cloud0=0,
                      cloud_stride=1, absolute=False):
    """Count, one host read of the totals (through a pinned copy), emit.  ``params``: the DEVICE copy of ``pack_params``'
    block.  Returns (pairs int64 [P, 2] on the device, matches per pair as a list, cnt int32 [total0])."""
    lib = _lib.require_gpu()
    dev = xyz0.device
    total0, total1 = int(xyz0.shape[0]), int(xyz1.shape[0])
    st = _lib.stream()
    at = lambda name: ctypes.c_void_p(params.data_ptr() + 8 * layout[name][0])
    k = 0 if K is None else int(K)
    if K is not None and k < 1:
        raise ValueError("K must be None or >= 1")
    cnt = torch.empty(total0, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.gcl_pair_matches_scratch_len(total0), dtype=torch.int32, device=dev)
    meta = torch.empty(2 + n_pairs, dtype=torch.int64, device=dev)
    common = (_lib.ptr(xyz0, torch.float32) if total0 else None, total0, at("offsets0"),
              _lib.ptr(xyz1, torch.float32) if total1 else None, total1, at("offsets1"), at("table_row0"), n_pairs,
              _lib.ptr(table, torch.int64), cap, int(cloud0), int(cloud_stride), float(voxel_size), at("trans"), at("radii"),
              float(radius_max), k)
    _lib.check(lib.gcl_pair_matches_count(*common, _lib.ptr(cnt) if total0 else None, _lib.ptr(scratch), _lib.ptr(meta), st),
               "gcl_pair_matches_count")
    host = torch.empty(2 + n_pairs, dtype=torch.int64, pin_memory=True)
    host.copy_(meta, non_blocking=True)
    torch.cuda.current_stream().synchronize()                # the host read: P, status, the totals per pair
    m = host.tolist()
    if m[1]:
        raise ValueError(f"gcl_pair_matches_count refused the batch: {STATUS_TEXT.get(m[1], m[1])}")
    P = m[0]
    pairs = torch.empty((P, 2), dtype=torch.int64, device=dev)
    _lib.check(lib.gcl_pair_matches_emit(*common, 1 if absolute else 0, _lib.ptr(scratch), _lib.ptr(meta),
                                         _lib.ptr(pairs) if P else None, P, st), "gcl_pair_matches_emit")
    return pairs, m[2:], cnt


def target_table(xyz1, offsets1, voxel_size):
    """The coordinate table of the target clouds of a batch (cloud b = rows offsets1[b] .. offsets1[b+1], batch id b); its
    values are rows of ``xyz1``.  Raises ValueError when a voxel holds more than one point."""
    lib = _lib.require_gpu()
    total1 = int(xyz1.shape[0])
    B = len(offsets1) - 1
    if B > 64:
        raise ValueError("more than 64 target clouds: pass the table they were voxelised through")
    offs = np.ascontiguousarray(offsets1, dtype=np.int64)
    if offs[0] != 0 or offs[-1] != total1 or (np.diff(offs) < 0).any():
        raise ValueError("offsets1 must run from 0 to len(target_xyz)")
    dev = xyz1.device
    raw = torch.empty((total1, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.gcl_voxel_coords_multi(_lib.ptr(xyz1, torch.float32), total1, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          B, float(voxel_size), _lib.ptr(raw), _lib.stream()), "gcl_voxel_coords_multi")
    cap = _cap(total1)
    table = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.gcl_scan_scratch_len(total1), dtype=torch.int32, device=dev)
    coords = torch.empty((total1, 4), dtype=torch.int32, device=dev)
    index = torch.empty(total1, dtype=torch.int64, device=dev)
    meta = torch.empty(8, dtype=torch.int32, device=dev)
    off = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * t.element_size())
    _lib.check(lib.gcl_unique_coords(_lib.ptr(raw), total1, _lib.ptr(table), cap, _lib.ptr(scratch), _lib.ptr(coords),
                                     _lib.ptr(index), off(meta, 0), off(meta, 4), _lib.stream()), "gcl_unique_coords")
    m = meta.tolist()
    if m[4]:
        raise ValueError(f"{m[4]} target points outside the packable voxel range")
    if m[0] != total1:
        raise ValueError(f"{total1 - m[0]} target points share a voxel of edge {voxel_size} with an earlier one: the matcher "
                         "needs a voxelised target (one point per voxel)")
    return table, cap


def get_matching_indices_batch(xyz0, offsets0, xyz1, offsets1, trans, radii, voxel_size, K=None, table=None, cloud0=0,
                               cloud_stride=1, table_row0=None, absolute=False, return_counts=False):
    """``get_matching_indices`` for a ragged batch of B pairs in one count and one emit.

    ``xyz0`` / ``xyz1``: float32 [total, 3] device tensors, pair b = rows offsets[b] .. offsets[b+1] (host int sequences of
    B + 1 entries); ``trans``: B host transforms (4 x 4 or 3 x 4, source -> target frame); ``radii``: B host floats;
    ``voxel_size``: the edge of the grid on which every target cloud has one point per voxel.  ``table``: ``(table, cap)`` of
    the targets when the caller has voxelised them already (batch id of target b = cloud0 + b * cloud_stride, ``table_row0[b]``
    = the table's value of its first row, default offsets1[b]); without it the table is built here and duplicates raise
    ValueError.  Returns int64 [P, 2] on the device, ordered by pair, source row, then (distance, target row); rows are
    relative to the pair's clouds, or rows of ``xyz0`` / ``xyz1`` with ``absolute=True``.  ``return_counts``: also the
    matches per pair (list) and per source row (int32 device tensor)."""
    _lib.require_gpu()
    if voxel_size is None or not voxel_size > 0:
        raise ValueError("voxel_size: the edge of the grid on which the target has one point per voxel")
    B = len(radii)
    if B < 1 or len(offsets0) != B + 1 or len(offsets1) != B + 1 or len(trans) != B:
        raise ValueError("need B >= 1 pairs: B transforms, B radii and B + 1 offsets per side")
    xyz0, xyz1 = xyz0.contiguous(), xyz1.contiguous()
    if table is None:
        if xyz1.shape[0] == 0:
            table = (torch.full((64, 2), -1, dtype=torch.int64, device=xyz1.device), 64)
        else:
            table = target_table(xyz1, offsets1, voxel_size)
        cloud0, cloud_stride, table_row0 = 0, 1, None
    tbl, cap = table
    host, lay = pack_params(offsets0, offsets1, trans, radii, table_row0)
    params = torch.empty(host.numel(), dtype=torch.int64, device=xyz0.device)
    params.copy_(host, non_blocking=True)
    pairs, totals, cnt = matches_on_device(xyz0, xyz1, params, lay, B, tbl, cap, voxel_size, float(np.max(radii)), K, cloud0,
                                           cloud_stride, absolute)
    return (pairs, totals, cnt) if return_counts else pairs


def get_matching_indices(source_xyz, target_xyz, trans, search_voxel_size, K=None, voxel_size=None, table=None):
    """``get_matching_indices`` (util/pointcloud.py:53-66) of one pair on device tensors: every (i, j) with
    |trans(source[i]) - target[j]| < search_voxel_size, per source row nearest first, the first K of a row when K is given.

    ``voxel_size`` is required: the target must have one point per voxel of that edge (the datasets pass voxelised clouds).  A
    grid of edge ``search_voxel_size`` would NOT do -- a voxel may then hold several points.  ``table``: the ``(table, cap)``
    that ``sparse_quantize_gpu(target_xyz, voxel_size, return_table=True)`` returned (batch id 0), if the caller has it;
    otherwise it is built here and a ValueError names the duplicates.  Returns int64 [P, 2] on the device."""
    if voxel_size is None:
        raise ValueError("get_matching_indices needs voxel_size (with or without a table): the target's voxels are its search "
                         "structure, and a grid of edge search_voxel_size may hold several points per voxel")
    n0, n1 = int(source_xyz.shape[0]), int(target_xyz.shape[0])
    return get_matching_indices_batch(source_xyz, [0, n0], target_xyz, [0, n1], [trans], [float(search_voxel_size)], voxel_size,
                                      K=K, table=table)
