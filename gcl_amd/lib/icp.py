"""Point-to-point ICP on the MI355X kernels (csrc/icp.hip): open3d's ``registration_icp`` with
``TransformationEstimationPointToPoint`` for a ragged batch of scan pairs in one call.

The reference needs it in two places: the pair loaders refine the odometry pose of every pair with it before the pair can
serve as ground truth (lib/data_loaders.py:447-474 ``KITTIPairDataset``, lib/complement_data_loader.py:369-399 ``_get_icp``
and its nuScenes twin) -> ``refine_pair_poses``; and scripts/SC2_PCR/benchmark_utils.py:40-56 offers ``icp_refine``.

The semantics are RESTATED from open3d's published source (open3d is not a dependency), in DESIGN.md "ICP" and in numpy in
tests/icp_oracle.py.  Everything is fp64 on the device from the fp32 points.  Two things differ from open3d on purpose:

- the point of source row i at iteration k is ``T_k x_i`` with the COMPOSED transformation; open3d moves its double points
  by every update in turn.  The two differ by rounding only.
- one or two correspondences stop the pair with ``status`` 2 (open3d's answer there is a rank-deficient SVD, not unique).

The target's neighbour grid is the one of the FPFH lists (``gcl_fpfh_cell_keys`` + a sort, the "cloud" of a key being the
pair); the Kabsch solve is the one of the registration back-ends.  Results stay on the device and no call waits for the host;
a pair's result is bitwise the same alone, anywhere in any batch and on every run.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device
from gcl_amd.lib.fpfh import _offsets_host, _points


class BatchICPResult:
    """Device tensors of a batch of ICP runs: ``transformation`` float64 [B, 4, 4], ``stats`` float64 [B, 4] (fitness,
    inlier rmse, correspondences, updates applied), ``status`` int32 [B] (0; 1: empty cloud or no correspondence; 2: one or
    two correspondences) and ``corr`` int32 [total0] (the target row within the pair's own target under the final
    transformation, -1: none; None unless asked for)."""

    def __init__(self, transformation, stats, status, corr):
        self.transformation, self.stats, self.status, self.corr = transformation, stats, status, corr

    @property
    def fitness(self):
        return self.stats[:, 0]

    @property
    def inlier_rmse(self):
        return self.stats[:, 1]


class ICPResult:
    """Device tensors of one ICP run: ``transformation`` float64 [4, 4], ``fitness``, ``inlier_rmse`` (0-d views),
    ``stats`` float64 [4], ``status`` (0-d int32) and ``correspondence_set`` int64 [n_corr, 2] (source row, target row),
    which is built from the kernels' per-row answer when it is first asked for."""

    def __init__(self, transformation, stats, status, corr):
        self.transformation, self.stats, self.status, self.corr = transformation, stats, status, corr
        self._set = None

    @property
    def fitness(self):
        return self.stats[0]

    @property
    def inlier_rmse(self):
        return self.stats[1]

    @property
    def correspondence_set(self):
        if self._set is None:
            rows = torch.nonzero(self.corr >= 0).flatten()
            self._set = torch.stack([rows, self.corr[rows].long()], dim=1)
        return self._set


def _distance(d):
    d = float(d)
    if not (0.0 < d < 3.0e38) or not np.float32(d) > 0:           # the grid's edge is the float32 of it
        raise ValueError(f"max_correspondence_distance must be positive and finite, got {d}")
    return d


def _criteria(max_iteration, relative_fitness, relative_rmse):
    if int(max_iteration) != max_iteration or not 0 <= int(max_iteration) <= 1000000:
        raise ValueError(f"max_iteration must be an integer in 0 .. 1000000, got {max_iteration}")
    rf, rr = float(relative_fitness), float(relative_rmse)
    if rf != rf or rr != rr:
        raise ValueError("relative_fitness and relative_rmse must be numbers")
    return int(max_iteration), rf, rr


def _init(init, B):
    """The validated [B, 16] float64 start (host numpy, or a device tensor as given); None: identities."""
    if init is None:
        return np.tile(np.eye(4).reshape(1, 16), (B, 1))
    if torch.is_tensor(init):
        if tuple(init.shape) == (4, 4):
            init = init[None]
        if tuple(init.shape) != (B, 4, 4):
            raise ValueError(f"init must be [4, 4] or [B, 4, 4] with B = {B}, got {tuple(init.shape)}")
        return init.detach().to(torch.float64).reshape(B, 16).contiguous()
    a = np.asarray(init, dtype=np.float64)
    if a.shape == (4, 4):
        a = a[None]
    if a.shape != (B, 4, 4):
        raise ValueError(f"init must be [4, 4] or [B, 4, 4] with B = {B}, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("init must be finite")
    return np.ascontiguousarray(a.reshape(B, 16))


def registration_icp_batch(xyz0, offsets0, xyz1, offsets1, max_correspondence_distance, init=None, max_iteration=30,
                           relative_fitness=1e-6, relative_rmse=1e-6, want_corr=False):
    """ICP of B pairs in one call: pair b moves the rows ``offsets0[b] .. offsets0[b + 1]`` of ``xyz0`` [total0, 3] onto the
    rows ``offsets1[b] .. offsets1[b + 1]`` of ``xyz1`` [total1, 3] (offsets: host integers [B + 1], ascending from 0 to the
    row count; None: one pair).  ``init``: [B, 4, 4] (or one [4, 4] when B = 1; host array or device tensor; None:
    identities).  The criteria are open3d's ``ICPConvergenceCriteria``.  Returns a ``BatchICPResult`` of device tensors;
    nothing is read back (``corr`` only with ``want_corr``)."""
    xyz0, xyz1 = _points(xyz0, "xyz0"), _points(xyz1, "xyz1")
    d = _distance(max_correspondence_distance)
    max_iteration, rf, rr = _criteria(max_iteration, relative_fitness, relative_rmse)
    off0, off1 = _offsets_host(offsets0, xyz0.shape[0]), _offsets_host(offsets1, xyz1.shape[0])
    if off0.size != off1.size:
        raise ValueError(f"{off0.size - 1} sources but {off1.size - 1} targets")
    B = off0.size - 1
    init = _init(init, B)
    if xyz0.device != xyz1.device:
        raise ValueError(f"xyz0 on {xyz0.device} but xyz1 on {xyz1.device}")
    lib = _lib.require_gpu()
    dev = xyz0.device
    n0, n1 = xyz0.shape[0], xyz1.shape[0]
    init = init.to(dev) if torch.is_tensor(init) else host_to_device(init, dev)
    off_dev = host_to_device(np.concatenate([off0, off1]), dev)
    off0_dev, off1_dev = off_dev[:B + 1], off_dev[B + 1:]
    skeys = order = None
    if n1:
        keys = torch.empty(n1, dtype=torch.int64, device=dev)
        _lib.check(lib.gcl_fpfh_cell_keys(_lib.ptr(xyz1), n1, _lib.ptr(off1_dev), B, d, _lib.ptr(keys), _lib.stream()),
                   "gcl_fpfh_cell_keys")
        skeys, order = torch.sort(keys)              # plumbing: the kernels need the runs of equal cells, in any inner order
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    corr = torch.empty(n0, dtype=torch.int32, device=dev) if want_corr else None
    scratch = torch.empty(max(lib.gcl_icp_scratch_bytes(n0, n1, B), 1), dtype=torch.uint8, device=dev)
    i64p = ctypes.POINTER(ctypes.c_int64)
    _lib.check(lib.gcl_icp_register_batch(_lib.ptr(xyz0) if n0 else None, off0.ctypes.data_as(i64p), _lib.ptr(off0_dev),
                                          _lib.ptr(xyz1) if n1 else None, off1.ctypes.data_as(i64p), _lib.ptr(off1_dev), B,
                                          _lib.ptr(skeys), _lib.ptr(order), d, _lib.ptr(init), max_iteration, rf, rr,
                                          _lib.ptr(scratch), _lib.ptr(T), _lib.ptr(stats),
                                          _lib.ptr(status), _lib.ptr(corr) if n0 else None, _lib.stream()),
               "gcl_icp_register_batch")
    return BatchICPResult(T, stats, status, corr)


def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6):
    """open3d's ``registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))`` for
    two device clouds [N, 3] and [M, 3]: an ``ICPResult``."""
    r = registration_icp_batch(source, None, target, None, max_correspondence_distance, init, max_iteration,
                               relative_fitness, relative_rmse, want_corr=True)
    return ICPResult(r.transformation[0], r.stats[0], r.status[0], r.corr)


def icp_refine(src_keypts, tgt_keypts, pred_trans):
    """scripts/SC2_PCR/benchmark_utils.py:40-56: ``src_keypts`` / ``tgt_keypts`` [1, n, 3], ``pred_trans`` [1, 4, 4] ->
    the refined transformation float32 [1, 4, 4] on ``pred_trans``' device (threshold 0.10, open3d's default criteria)."""
    if not (torch.is_tensor(src_keypts) and torch.is_tensor(tgt_keypts) and torch.is_tensor(pred_trans)):
        raise ValueError("src_keypts, tgt_keypts and pred_trans must be tensors")
    if src_keypts.dim() != 3 or src_keypts.shape[0] != 1 or tgt_keypts.dim() != 3 or tgt_keypts.shape[0] != 1:
        raise ValueError(f"keypoints must be [1, n, 3], got {tuple(src_keypts.shape)} and {tuple(tgt_keypts.shape)}")
    if tuple(pred_trans.shape) != (1, 4, 4):
        raise ValueError(f"pred_trans must be [1, 4, 4], got {tuple(pred_trans.shape)}")
    r = registration_icp_batch(src_keypts[0], None, tgt_keypts[0], None, 0.10, pred_trans[0])
    return r.transformation.to(pred_trans.device).float()


def voxelise_clouds(clouds, voxel):
    """The loader's device voxeliser over 1 .. 64 raw host clouds (float32 [P_c, 3]) in one pass: the first point of every
    ``voxel`` voxel of every cloud (``sparse_quantize(xyz / voxel, return_index=True)``).  Returns (xyz float32 [P, 3] on the
    device, whose first rows are the selected points cloud after cloud; starts: host list [n_clouds + 1] of the clouds'
    first rows).  One host read: the row counts."""
    n_clouds = len(clouds)
    if not 1 <= n_clouds <= 64:
        raise ValueError(f"1 .. 64 clouds per call (they share the voxeliser's table), got {n_clouds}")
    clouds = [np.asarray(x, dtype=np.float32) for x in clouds]
    for x in clouds:
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"a cloud must be [P, 3], got {x.shape}")
    voxel = float(voxel)
    if not (0.0 < voxel < 3.0e38):
        raise ValueError(f"the voxel size must be positive and finite, got {voxel}")
    offs = np.zeros(n_clouds + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    P = int(offs[-1])
    if P == 0:
        raise ValueError("a batch without points")
    lib = _lib.require_gpu()
    from gcl_amd.lib.colocation_data_gpu import _cap
    dev = torch.device("cuda", torch.cuda.current_device())
    # one pinned block, one copy: identity frames for gcl_loader_points (doubles first: 8-byte aligned), then the points
    n_fr = n_clouds * 24
    host = torch.empty(n_fr + 3 * P, dtype=torch.float32, pin_memory=True)
    host[:n_fr].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.eye(4)[:3].reshape(-1)
    hp = host[n_fr:].view(P, 3).numpy()
    for c, x in enumerate(clouds):
        hp[offs[c]:offs[c + 1]] = x
    st = _lib.stream()
    dbuf = torch.empty(host.numel(), dtype=torch.float32, device=dev)
    dbuf.copy_(host, non_blocking=True)
    frames, xyz_raw = dbuf[:n_fr], dbuf[n_fr:]
    off = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * t.element_size())
    raw = torch.empty((P, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.gcl_voxel_coords_multi(_lib.ptr(xyz_raw), P, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_clouds,
                                          voxel, _lib.ptr(raw), st), "gcl_voxel_coords_multi")
    meta = torch.empty(8 + n_clouds + 1, dtype=torch.int32, device=dev)      # rows, status, the clouds' first rows
    cap = _cap(P)
    table = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.gcl_scan_scratch_len(P), dtype=torch.int32, device=dev)
    coords = torch.empty((P, 4), dtype=torch.int32, device=dev)
    index = torch.empty(P, dtype=torch.int64, device=dev)
    _lib.check(lib.gcl_unique_coords(_lib.ptr(raw), P, _lib.ptr(table), cap, _lib.ptr(scratch), _lib.ptr(coords),
                                     _lib.ptr(index), off(meta, 0), off(meta, 4), st), "gcl_unique_coords")
    _lib.check(lib.gcl_cloud_row_starts(_lib.ptr(coords), P, off(meta, 0), n_clouds, off(meta, 8), st), "gcl_cloud_row_starts")
    xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
    xyz_cf = torch.empty((P, 3), dtype=torch.float32, device=dev)            # identity frames: a second copy nobody reads
    _lib.check(lib.gcl_loader_points(_lib.ptr(xyz_raw), _lib.ptr(index), _lib.ptr(coords), P, off(meta, 0), _lib.ptr(frames),
                                     _lib.ptr(xyz), _lib.ptr(xyz_cf), st), "gcl_loader_points")
    m = meta.tolist()                                                        # host read 1: rows, status, first rows
    if m[4]:
        raise ValueError(f"{m[4]} points outside the packable voxel range")
    starts = m[8:8 + n_clouds + 1]
    for c in range(n_clouds - 1, -1, -1):                                    # a cloud without rows starts where the next does
        if starts[c] < 0:
            starts[c] = starts[c + 1]
    return xyz, starts


def refine_pair_poses(pairs, icp_voxel_size=0.05, max_distance=0.2, max_iteration=200):
    """The batch form of the pair loaders' ``_get_icp``.  ``pairs``: 1 .. 32 dicts ``{"xyz0", "xyz1": raw float32 [P, 3]
    host arrays, "M": 4 x 4, the odometry pose that moves xyz0 into xyz1's frame}``.  Both scans are downsampled to the first
    point of every ``icp_voxel_size`` voxel (``sparse_quantize(xyz / voxel, return_index=True)``, the loader's device
    voxeliser as ``build_pair_batch_gpu`` calls it), the selected xyz0 is registered onto the selected xyz1 from ``init = M``
    -- the iterates of the reference's "move by M, start at the identity" -- and the answer is the reference's
    ``M2 = M @ T_icp`` with ``T_icp = T_total inv(M)`` (its multiplication order is kept as it is): float64 [B, 4, 4] on the
    host, ready to be a pair's ``"trans"``.  Host reads: the voxeliser's row counts, then the [B, 16] transformations."""
    B = len(pairs)
    if not 1 <= B <= 32:
        raise ValueError("1 .. 32 pairs per call (64 clouds share the voxeliser's table)")
    voxel = float(icp_voxel_size)
    if not (0.0 < voxel < 3.0e38):
        raise ValueError(f"icp_voxel_size must be positive and finite, got {voxel}")
    d = _distance(max_distance)
    max_iteration, _, _ = _criteria(max_iteration, 1e-6, 1e-6)
    clouds, Ms = [], []
    for p in pairs:
        for k in ("xyz0", "xyz1"):
            x = np.asarray(p[k], dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != 3:
                raise ValueError(f"{k} must be [P, 3], got {x.shape}")
            clouds.append(x)
        M = np.asarray(p["M"], dtype=np.float64)
        if M.shape != (4, 4) or not np.isfinite(M).all():
            raise ValueError("M must be a finite 4 x 4 matrix")
        Ms.append(M)
    Ms = np.stack(Ms)
    xyz, starts = voxelise_clouds(clouds, voxel)
    side = lambda k: torch.cat([xyz[starts[2 * b + k]:starts[2 * b + k + 1]] for b in range(B)])
    count = lambda k: np.concatenate([[0], np.cumsum([starts[2 * b + k + 1] - starts[2 * b + k] for b in range(B)])])
    r = registration_icp_batch(side(0), count(0), side(1), count(1), d, Ms, max_iteration)
    T = r.transformation.cpu().numpy()                                       # host read 2: [B, 16]
    return np.stack([Ms[b] @ (T[b] @ np.linalg.inv(Ms[b])) for b in range(B)])
