"""Pair batches from raw scans on the GPU: what ``KITTIPairDataset.__getitem__`` (lib/data_loaders.py:494-536) x batch size +
``collate_pair_fn`` (:26-79) produce after the loader's rotation / scale -- voxelisation of both clouds, the ground-truth
correspondences (``get_matching_indices``, util/pointcloud.py:53-66) and the batch dict the four pair trainers and
``validate_pairs`` consume -- with every tensor resident on the device.

All 2 B clouds of a batch go through ONE coordinate table (cloud id 2 b + k, as ``build_batch_gpu`` does for the co-location
batches), the matches of the whole batch are one count and one emit (csrc/pairmatch.hip), and the host reads twice: the row
counts of the clouds, then the match totals.  The loader's random rotations and scale (:476-492) are applied on the device when
a pair carries the draws (``"rotation0"``, ``"rotation1"``, ``"scale"``; gcl_amd/lib/augment.py makes them), in the float64
arithmetic the pair loaders keep through ``sparse_quantize``.  The file readers and the ICP cache files stay with the caller, as
they do for ``build_batch_gpu``; the ICP refinement that makes a pair's ``"trans"`` is ``gcl_amd.lib.icp.refine_pair_poses``.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib import augment
from gcl_amd.lib.colocation_data_gpu import AUG_F64, _cap
from gcl_amd.util.pointcloud import matches_on_device, pack_params


def filled_starts(starts):
    """``gcl_cloud_row_starts``' list with the -1 of a cloud without rows replaced: it starts where the next one does."""
    starts = list(starts)
    for c in range(len(starts) - 2, -1, -1):
        if starts[c] < 0:
            starts[c] = starts[c + 1]
    return starts


def sides_and_matches(xyz, coords, starts, B, trans, radii, table, cap, voxel_size, K):
    """The tail the pair builders share.  ``xyz`` / ``coords``: the voxel representatives and coordinates of a table whose
    clouds 2 b and 2 b + 1 are pair b's source and target (further clouds may follow them); ``starts``: their first rows.  The
    table numbers the rows pair-major; the trainers want the sources and the targets apart, the batch id = the pair's number,
    and the matches of the whole batch in one count and one emit (one host read: the totals).  Returns
    ``(xyz0, xyz1, C0, C1, n0, n1, o0, o1, pairs, totals)``."""
    dev = xyz.device
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
                                         cloud_stride=2, absolute=True)
    return xyz0, xyz1, C0, C1, n0, n1, o0, o1, pairs, totals


def build_pair_batch_gpu(raw_pairs, voxel_size, device, K=None, stream=None):
    """``raw_pairs``: list of ``{"xyz0", "xyz1": float32 [P, 3] host arrays (after the loader's rotation / scale), "trans":
    4 x 4 (cloud 0 -> cloud 1), "radius": the pair's matching radius (:486-490)}``.  Returns the dict of ``collate_pair_fn``
    with device tensors: ``sinput0_C / sinput1_C`` int32 [N, 4] (batch id = pair number), ``sinput0_F / sinput1_F`` ones,
    ``correspondences`` int64 [P, 2] with the running start indices added (int64: the repository's convention),
    ``pcd0``, ``pcd1``, ``T_gt`` float32 [4 B', 4], ``len_batch``.  The reference's quirk is kept: a pair WITHOUT a match is
    left out of ``pcd0``, ``pcd1``, ``T_gt``, ``len_batch`` (B' pairs remain) and contributes no correspondence, but its rows
    stay in ``sinput*_C`` and the start indices move past it (:46-57).  ``K``: as ``get_matching_indices``' (None = all).
    A pair may carry the loader's DRAWS instead of augmented clouds (:476-492): ``"rotation0"`` / ``"rotation1"`` (3 x 3, each
    cloud turned about its own centroid: ``T_k = [R_k | R_k (-centroid_k)]``) and / or ``"scale"``.  The device then evaluates
    ``scale * (x @ R.T + t)`` and ``floor(y / voxel_size)`` in float64 as the pair loaders do (lib/data_loaders.py:125-129;
    csrc/data.hip, AUG_F64), ``pcd0`` / ``pcd1`` and the matching read the float32 of those points, ``trans`` becomes
    ``T1 @ trans @ inv(T0)`` with its translation scaled (:479, lib/colocation_data_loader.py:369,
    lib/complement_data_loader.py:662), ``T_gt`` is the float32 of that and ``radius`` becomes ``radius * scale`` (:490).
    ``KITTIPairDataset`` itself leaves the translation unscaled, which puts its ground truth off by (1 - scale) |t|: that quirk
    is NOT reproduced.  A cloud without a rotation stays float32 (``x * fp32(scale)``), as in the reference.  ValueError before
    any GPU work: a rotation with |R^T R - I| above 1e-6, a scale <= 0, an empty cloud that has a rotation.
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
    # the augmentation keys, checked before any GPU work; a batch without them takes the path it always took
    rots = [augment.checked_rotation(p[k], k) if p.get(k) is not None else None for p in raw_pairs
            for k in ("rotation0", "rotation1")]
    scales = [augment.checked_scale(p["scale"]) if p.get("scale") is not None else None for p in raw_pairs]
    device_aug = any(r is not None for r in rots) or any(v is not None for v in scales)
    if any(r is not None and len(x) == 0 for r, x in zip(rots, clouds)):
        raise ValueError("an empty cloud has no centroid to rotate about")
    # one pinned block, one copy: identity frames for gcl_loader_points (doubles first: they stay 8-byte aligned), T_gt as the
    # reference's .float() makes it, then the points of the 2 B clouds
    n_fr, tg = n_clouds * 24, B * 16
    head = n_fr * (2 if device_aug else 1)      # + the per-cloud table of the device's augmentation (augment.affine_rows)
    host = torch.empty(head + tg + 3 * P, dtype=torch.float32, pin_memory=True)
    host[:n_fr].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.eye(4)[:3].reshape(-1)
    if device_aug:
        host[n_fr:head].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.stack(
            [augment.affine_rows(rots[c], scales[c // 2]) for c in range(n_clouds)])
    host[head:head + tg].view(B, 4, 4).numpy()[:] = np.stack(trans).astype(np.float32)
    hp = host[head + tg:].view(P, 3).numpy()
    for c, x in enumerate(clouds):
        hp[offs[c]:offs[c + 1]] = x
    st_ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(dev), st_ctx:
        st = _lib.stream()
        d = torch.empty(host.numel(), dtype=torch.float32, device=dev)
        d.copy_(host, non_blocking=True)
        frames, aug_dev, T_all, xyz_raw = d[:n_fr], d[n_fr:head], d[head:head + tg].view(4 * B, 4), d[head + tg:]
        raw = torch.empty((P, 4), dtype=torch.int32, device=dev)
        off = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * t.element_size())
        offs_p = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        # meta: rows, status, the clouds' first rows and, behind them (8-byte aligned), the device's affines T_c as doubles
        a0 = (8 + n_clouds + 1 + 1) // 2 * 2
        meta = torch.empty(a0 + (24 * n_clouds if device_aug else 0), dtype=torch.int32, device=dev)
        if device_aug:
            cent = torch.empty(3 * n_clouds, dtype=torch.float64, device=dev)
            cscr = torch.empty(lib.gcl_cloud_centroids_scratch_len(P, n_clouds), dtype=torch.float64, device=dev)
            _lib.check(lib.gcl_cloud_centroids(_lib.ptr(xyz_raw), P, offs_p, n_clouds, _lib.ptr(cscr), _lib.ptr(cent), st),
                       "gcl_cloud_centroids")
            _lib.check(lib.gcl_cloud_affines(_lib.ptr(aug_dev), _lib.ptr(cent), n_clouds, off(meta, a0), st), "gcl_cloud_affines")
            _lib.check(lib.gcl_voxel_coords_aug(_lib.ptr(xyz_raw), P, offs_p, n_clouds, float(voxel_size), _lib.ptr(aug_dev),
                                                off(meta, a0), AUG_F64, _lib.ptr(raw), st), "gcl_voxel_coords_aug")
        else:
            _lib.check(lib.gcl_voxel_coords_multi(_lib.ptr(xyz_raw), P, offs_p, n_clouds, float(voxel_size), _lib.ptr(raw), st),
                       "gcl_voxel_coords_multi")
        cap = _cap(P)
        table = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        scratch = torch.empty(lib.gcl_scan_scratch_len(P), dtype=torch.int32, device=dev)
        coords = torch.empty((P, 4), dtype=torch.int32, device=dev)
        index = torch.empty(P, dtype=torch.int64, device=dev)
        _lib.check(lib.gcl_unique_coords(_lib.ptr(raw), P, _lib.ptr(table), cap, _lib.ptr(scratch), _lib.ptr(coords),
                                         _lib.ptr(index), off(meta, 0), off(meta, 4), st), "gcl_unique_coords")
        _lib.check(lib.gcl_cloud_row_starts(_lib.ptr(coords), P, off(meta, 0), n_clouds, off(meta, 8), st),
                   "gcl_cloud_row_starts")
        xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        xyz_cf = torch.empty((P, 3), dtype=torch.float32, device=dev)      # identity frames: a second copy nobody reads
        if not device_aug:
            _lib.check(lib.gcl_loader_points(_lib.ptr(xyz_raw), _lib.ptr(index), _lib.ptr(coords), P, off(meta, 0),
                                             _lib.ptr(frames), _lib.ptr(xyz), _lib.ptr(xyz_cf), st), "gcl_loader_points")
            m = meta.tolist()                                    # host read 1: rows, status, the clouds' first rows
        else:
            _lib.check(lib.gcl_loader_points_aug(_lib.ptr(xyz_raw), _lib.ptr(index), _lib.ptr(coords), P, off(meta, 0),
                                                 _lib.ptr(frames), _lib.ptr(aug_dev), off(meta, a0), AUG_F64, _lib.ptr(xyz),
                                                 _lib.ptr(xyz_cf), st), "gcl_loader_points_aug")
            mh = meta.cpu().numpy()                              # host read 1: the same + the clouds' affines T_c
            m = mh[:a0].tolist()
            T = [augment.affine4(r) for r in mh[a0:].view(np.float64).reshape(n_clouds, 12)]
            for b in range(B):
                trans[b] = augment.follow_pair_trans(T[2 * b], T[2 * b + 1], trans[b], scales[b])
                if scales[b] is not None:
                    radii[b] = radii[b] * scales[b]
            # T_gt of the augmented pairs: the pinned block's first copy has long left it
            host[head:head + tg].view(B, 4, 4).numpy()[:] = np.stack(trans).astype(np.float32)
            d[head:head + tg].copy_(host[head:head + tg], non_blocking=True)
        if m[4]:
            raise ValueError(f"{m[4]} points outside the packable voxel range")
        starts = filled_starts(m[8:8 + n_clouds + 1])
        xyz0, xyz1, C0, C1, n0, n1, o0, o1, pairs, totals = sides_and_matches(xyz, coords, starts, B, trans, radii, table, cap,
                                                                              voxel_size, K)      # host read 2: the match totals
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
