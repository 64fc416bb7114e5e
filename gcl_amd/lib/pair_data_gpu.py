"""Pair batches from raw scans on the GPU: what ``KITTIPairDataset.__getitem__`` (lib/data_loaders.py:494-536) x batch size +
``collate_pair_fn`` (:26-79) produce after the loader's rotation / scale -- voxelisation of both clouds, the ground-truth
correspondences (``get_matching_indices``, util/pointcloud.py:53-66) and the batch dict the four pair trainers and
``validate_pairs`` consume -- with every tensor resident on the device.

All 2 B clouds of a batch go through ONE coordinate table (cloud id 2 b + k, as ``build_batch_gpu`` does for the co-location
batches), the matches of the whole batch are one count and one emit (csrc/pairmatch.hip), and the host reads twice: the row
counts of the clouds, then the match totals.  The file readers, the ICP cache and the rotation / scale draws stay with the
caller, as they do for ``build_batch_gpu``.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.colocation_data_gpu import _cap
from gcl_amd.util.pointcloud import matches_on_device, pack_params


def build_pair_batch_gpu(raw_pairs, voxel_size, device, K=None, stream=None):
    """``raw_pairs``: list of ``{"xyz0", "xyz1": float32 [P, 3] host arrays (after the loader's rotation / scale), "trans":
    4 x 4 (cloud 0 -> cloud 1), "radius": the pair's matching radius (:486-490)}``.  Returns the dict of ``collate_pair_fn``
    with device tensors: ``sinput0_C / sinput1_C`` int32 [N, 4] (batch id = pair number), ``sinput0_F / sinput1_F`` ones,
    ``correspondences`` int64 [P, 2] with the running start indices added (int64: the repository's convention),
    ``pcd0``, ``pcd1``, ``T_gt`` float32 [4 B', 4], ``len_batch``.  The reference's quirk is kept: a pair WITHOUT a match is
    left out of ``pcd0``, ``pcd1``, ``T_gt``, ``len_batch`` (B' pairs remain) and contributes no correspondence, but its rows
    stay in ``sinput*_C`` and the start indices move past it (:46-57).  ``K``: as ``get_matching_indices``' (None = all).
    Work is enqueued on ``stream`` (default: the current one); the two host reads wait for that stream only."""
    lib = _lib.require_gpu()
    dev = torch.device(device)
    B = len(raw_pairs)
    n_clouds = 2 * B
    if B < 1 or n_clouds > 64:
        raise ValueError("1 .. 32 pairs per batch (64 clouds share the table)")
    clouds = [np.asarray(p[k], dtype=np.float32).reshape(-1, 3) for p in raw_pairs for k in ("xyz0", "xyz1")]
    offs = np.zeros(n_clouds + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    P = int(offs[-1])
    if P == 0:
        raise ValueError("a batch without points")
    trans = [np.asarray(p["trans"], dtype=np.float64).reshape(4, 4) for p in raw_pairs]
    radii = [float(p["radius"]) for p in raw_pairs]
    # one pinned block, one copy: identity frames for gcl_loader_points (doubles first: they stay 8-byte aligned), T_gt as the
    # reference's .float() makes it, then the points of the 2 B clouds
    head, tg = n_clouds * 24, B * 16
    host = torch.empty(head + tg + 3 * P, dtype=torch.float32, pin_memory=True)
    host[:head].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.eye(4)[:3].reshape(-1)
    host[head:head + tg].view(B, 4, 4).numpy()[:] = np.stack(trans).astype(np.float32)
    hp = host[head + tg:].view(P, 3).numpy()
    for c, x in enumerate(clouds):
        hp[offs[c]:offs[c + 1]] = x
    st_ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(dev), st_ctx:
        st = _lib.stream()
        d = torch.empty(host.numel(), dtype=torch.float32, device=dev)
        d.copy_(host, non_blocking=True)
        frames, T_all, xyz_raw = d[:head], d[head:head + tg].view(4 * B, 4), d[head + tg:]
        raw = torch.empty((P, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.gcl_voxel_coords_multi(_lib.ptr(xyz_raw), P, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                              n_clouds, float(voxel_size), _lib.ptr(raw), st), "gcl_voxel_coords_multi")
        cap = _cap(P)
        table = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        scratch = torch.empty(lib.gcl_scan_scratch_len(P), dtype=torch.int32, device=dev)
        coords = torch.empty((P, 4), dtype=torch.int32, device=dev)
        index = torch.empty(P, dtype=torch.int64, device=dev)
        meta = torch.empty(8 + n_clouds + 1, dtype=torch.int32, device=dev)
        off = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * t.element_size())
        _lib.check(lib.gcl_unique_coords(_lib.ptr(raw), P, _lib.ptr(table), cap, _lib.ptr(scratch), _lib.ptr(coords),
                                         _lib.ptr(index), off(meta, 0), off(meta, 4), st), "gcl_unique_coords")
        _lib.check(lib.gcl_cloud_row_starts(_lib.ptr(coords), P, off(meta, 0), n_clouds, off(meta, 8), st),
                   "gcl_cloud_row_starts")
        xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        xyz_cf = torch.empty((P, 3), dtype=torch.float32, device=dev)      # identity frames: a second copy nobody reads
        _lib.check(lib.gcl_loader_points(_lib.ptr(xyz_raw), _lib.ptr(index), _lib.ptr(coords), P, off(meta, 0),
                                         _lib.ptr(frames), _lib.ptr(xyz), _lib.ptr(xyz_cf), st), "gcl_loader_points")
        m = meta.tolist()                                        # host read 1: rows, status, the clouds' first rows
        if m[4]:
            raise ValueError(f"{m[4]} points outside the packable voxel range")
        starts = m[8:8 + n_clouds + 1]
        for c in range(n_clouds - 1, -1, -1):                    # a cloud without rows starts where the next one does
            if starts[c] < 0:
                starts[c] = starts[c + 1]
        # the table numbers the rows of all 2 B clouds, pair-major; the trainers want the sources and the targets apart
        side = lambda t, k: torch.cat([t[starts[2 * b + k]:starts[2 * b + k + 1]] for b in range(B)])
        xyz0, xyz1, C0, C1 = side(xyz, 0), side(xyz, 1), side(coords, 0), side(coords, 1)
        C0[:, 0] >>= 1                                           # cloud id 2 b + k -> pair number b
        C1[:, 0] >>= 1
        n0 = [starts[2 * b + 1] - starts[2 * b] for b in range(B)]
        n1 = [starts[2 * b + 2] - starts[2 * b + 1] for b in range(B)]
        o0, o1 = np.concatenate([[0], np.cumsum(n0)]), np.concatenate([[0], np.cumsum(n1)])
        ph, lay = pack_params(o0, o1, trans, radii, table_row0=[starts[2 * b + 1] for b in range(B)])
        params = torch.empty(ph.numel(), dtype=torch.int64, device=dev)
        params.copy_(ph, non_blocking=True)
        pairs, totals, _ = matches_on_device(xyz0, xyz1, params, lay, B, table, cap, voxel_size, max(radii), K, cloud0=1,
                                             cloud_stride=2, absolute=True)          # host read 2: the match totals
        keep = [b for b in range(B) if totals[b] > 0]
        if len(keep) == B:
            pcd0, pcd1, T_gt = xyz0, xyz1, T_all
        elif keep:
            pcd0 = torch.cat([xyz0[o0[b]:o0[b + 1]] for b in keep])
            pcd1 = torch.cat([xyz1[o1[b]:o1[b + 1]] for b in keep])
            T_gt = torch.cat([T_all[4 * b:4 * b + 4] for b in keep])
        else:
            pcd0, pcd1, T_gt = xyz0[:0], xyz1[:0], T_all[:0]
        ones = lambda n: torch.ones((n, 1), dtype=torch.float32, device=dev)
        return {"pcd0": pcd0, "pcd1": pcd1, "sinput0_C": C0, "sinput0_F": ones(len(C0)), "sinput1_C": C1,
                "sinput1_F": ones(len(C1)), "correspondences": pairs, "T_gt": T_gt,
                "len_batch": [[n0[b], n1[b]] for b in keep]}
