"""FPFH descriptors on the MI355X kernels (csrc/fpfh.hip): radius neighbour lists, surface normals, SPFH and FPFH, as
open3d's ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`` and ``compute_fpfh_feature`` make them.

The reference's SC2-PCR benchmark offers ``descriptor: fpfh`` but only LOADS the descriptors from files that were made with
open3d (scripts/SC2_PCR/dataset.py:66-74, 220-228).  ``fpfh_descriptors`` makes them here, so that the 33-channel arm of
``pdist_min``, ``Matcher``, ``BatchMatcher``, ``FeatureRansac`` and ``SC2_PCR_bench.eval_per_pair`` can be fed from a raw
point cloud.

Everything is fp64 on the device from the fp32 points; the semantics are restated in numpy in tests/fpfh_oracle.py
(neighbour lists, normals' sign and SPFH agree with it bit for bit).  Two things differ from bare open3d on purpose:

- the SIGN of a normal is defined: it is turned towards ``viewpoint`` (open3d leaves the eigen-solver's sign unless
  ``orient_normals_towards_camera_location`` is called, and the third FPFH feature is odd in it).  Pass the SENSOR POSITION
  of each scan, in the scan's own frame, as ``viewpoint``; the default is the origin of each cloud's frame, which is the
  sensor for an untransformed scan.
- a batch: ``offsets`` (host integers [B + 1], ascending from 0 to N) makes ``xyz`` a concatenation of B clouds; a point's
  neighbours come from its own cloud only and ``idx`` holds rows of the concatenation.

Results stay on the device and every call runs on the current stream without waiting for the host (``offsets`` and
``viewpoint`` given on the host are small non-blocking copies).
"""
import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device

BINS = _lib.FPFH_BINS


def _points(xyz, name="xyz"):
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{name} must be a [N, 3] tensor, got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz)}")
    if xyz.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{name}: {xyz.shape[0]} rows do not fit the int32 neighbour lists")
    return xyz.detach().to(torch.float32).contiguous()


def _radius(radius):
    radius = float(radius)
    if not (0.0 < radius < 3.0e38):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    return radius


def _max_nn(max_nn):
    if int(max_nn) != max_nn or not 1 <= int(max_nn) <= _lib.FPFH_MAX_NN:
        raise ValueError(f"max_nn must be an integer in 1 .. {_lib.FPFH_MAX_NN}, got {max_nn}")
    return int(max_nn)


def _offsets_host(offsets, n):
    """The validated host int64 [B + 1] offsets (None: one cloud)."""
    if offsets is None:
        return np.array([0, n], dtype=np.int64)
    if torch.is_tensor(offsets):
        if offsets.is_cuda:
            raise ValueError("offsets must be host integers (they are validated before anything is launched)")
        offsets = offsets.numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError(f"offsets must be [B + 1] integers with B >= 1, got shape {off.shape} of {off.dtype}")
    off = off.astype(np.int64)
    if off.size - 1 > _lib.FPFH_MAX_CLOUDS:
        raise ValueError(f"at most {_lib.FPFH_MAX_CLOUDS} clouds per call, got {off.size - 1}")
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must ascend from 0 to N = {n}, got {off.tolist() if off.size <= 16 else off}")
    return off


def _offsets_dev(off, dev):
    return host_to_device(off, dev)


def _lists(idx, cnt, n):
    if (not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n
            or not 1 <= idx.shape[1] <= _lib.FPFH_MAX_NN):
        raise ValueError(f"idx must be an int32 [{n}, max_nn] tensor with max_nn in 1 .. {_lib.FPFH_MAX_NN}")
    if not torch.is_tensor(cnt) or cnt.dtype != torch.int32 or tuple(cnt.shape) != (n,):
        raise ValueError(f"cnt must be an int32 [{n}] tensor")
    return idx.contiguous(), cnt.contiguous()


def _neighbours(lib, xyz, radius, max_nn, off_dev, n_clouds):
    n, dev = xyz.shape[0], xyz.device
    idx = torch.empty((n, max_nn), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return idx, cnt
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.gcl_fpfh_cell_keys(_lib.ptr(xyz), n, _lib.ptr(off_dev), n_clouds, radius, _lib.ptr(keys), _lib.stream()),
               "gcl_fpfh_cell_keys")
    skeys, order = torch.sort(keys)                  # plumbing: the kernels need the runs of equal cells, in any inner order
    _lib.check(lib.gcl_fpfh_neighbours(_lib.ptr(xyz), n, _lib.ptr(off_dev), n_clouds, _lib.ptr(skeys, torch.int64),
                                       _lib.ptr(order, torch.int64), radius, max_nn, _lib.ptr(idx), _lib.ptr(cnt),
                                       _lib.stream()), "gcl_fpfh_neighbours")
    return idx, cnt


def radius_neighbours(xyz, radius, max_nn, offsets=None):
    """open3d's ``KDTreeSearchParamHybrid(radius, max_nn)`` for every point of ``xyz`` [N, 3] against its own cloud:
    ``(idx int32 [N, max_nn], cnt int32 [N])``, the ``max_nn`` nearest points with d2 <= r2 (the point itself included) in
    ascending (d2, row) order, -1 in unused entries.  Exact for any density: a uniform grid with the radius as its edge, one
    wave per query, a streaming top-``max_nn`` in LDS."""
    xyz, radius, max_nn = _points(xyz), _radius(radius), _max_nn(max_nn)
    off = _offsets_host(offsets, xyz.shape[0])
    lib = _lib.require_gpu()
    return _neighbours(lib, xyz, radius, max_nn, _offsets_dev(off, xyz.device), off.size - 1)


def _viewpoint(viewpoint, n_clouds):
    """The validated float32 [B, 3] viewpoint (host or device tensor), None: the origin."""
    if viewpoint is None:
        return None
    vp = viewpoint.detach().to(torch.float32) if torch.is_tensor(viewpoint) else torch.as_tensor(
        np.asarray(viewpoint, dtype=np.float32))
    if tuple(vp.shape) == (3,):
        vp = vp[None].expand(n_clouds, 3)
    if tuple(vp.shape) != (n_clouds, 3):
        raise ValueError(f"viewpoint must be [3] or [B, 3] with B = {n_clouds}, got {tuple(vp.shape)}")
    return vp.contiguous()


def normals_from_neighbours(xyz, idx, cnt, viewpoint=None, offsets=None):
    """The normals of ``estimate_normals`` from given neighbour lists (``radius_neighbours``' result)."""
    xyz = _points(xyz)
    n = xyz.shape[0]
    idx, cnt = _lists(idx, cnt, n)
    off = _offsets_host(offsets, n)
    vp = _viewpoint(viewpoint, off.size - 1)
    lib = _lib.require_gpu()
    if vp is not None:
        vp = vp.to(xyz.device) if vp.is_cuda else host_to_device(vp, xyz.device)
    normals = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.gcl_fpfh_normals(_lib.ptr(xyz), n, _lib.ptr(idx), _lib.ptr(cnt), idx.shape[1], _lib.ptr(vp),
                                    _lib.ptr(_offsets_dev(off, xyz.device)), off.size - 1, _lib.ptr(normals), _lib.stream()),
               "gcl_fpfh_normals")
    return normals


def estimate_normals(xyz, radius, max_nn=30, viewpoint=None, offsets=None):
    """Surface normals float32 [N, 3]: the unit eigenvector of the smallest eigenvalue of the covariance of each point's
    ``radius_neighbours(xyz, radius, max_nn)`` (fp64 Jacobi), turned towards ``viewpoint`` ([3], or [B, 3] with ``offsets``;
    default: the origin of each cloud's frame) -- pass the sensor position of each scan.  Fewer than 3 neighbours: (0, 0, 1)."""
    xyz, radius, max_nn = _points(xyz), _radius(radius), _max_nn(max_nn)
    off = _offsets_host(offsets, xyz.shape[0])
    vp = _viewpoint(viewpoint, off.size - 1)                                   # shape errors before any launch
    idx, cnt = radius_neighbours(xyz, radius, max_nn, off)
    return normals_from_neighbours(xyz, idx, cnt, vp, off)


def _normals(normals, xyz):
    if not torch.is_tensor(normals) or tuple(normals.shape) != tuple(xyz.shape):
        raise ValueError(f"normals must be a {list(xyz.shape)} tensor like xyz, got "
                         f"{tuple(normals.shape) if torch.is_tensor(normals) else type(normals)}")
    if normals.device != xyz.device:
        raise ValueError(f"normals on {normals.device} but xyz on {xyz.device}")
    return normals.detach().to(torch.float32).contiguous()


def spfh_from_neighbours(xyz, normals, idx, cnt):
    """SPFH float32 [N, 33] of every point over the entries 1 .. cnt - 1 of its list: integer bin counts of open3d's pair
    features times 100 / (cnt - 1)."""
    xyz = _points(xyz)
    normals = _normals(normals, xyz)
    n = xyz.shape[0]
    idx, cnt = _lists(idx, cnt, n)
    lib = _lib.require_gpu()
    spfh = torch.empty((n, BINS), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.gcl_fpfh_spfh(_lib.ptr(xyz), _lib.ptr(normals), n, _lib.ptr(idx), _lib.ptr(cnt), idx.shape[1],
                                 _lib.ptr(spfh), _lib.stream()), "gcl_fpfh_spfh")
    return spfh


def fpfh_from_spfh(xyz, spfh, idx, cnt, normalize=False):
    """FPFH float32 [N, 33] from the SPFH rows of each point's neighbours (weights 1 / d2, open3d's choice)."""
    xyz = _points(xyz)
    n = xyz.shape[0]
    if not torch.is_tensor(spfh) or spfh.dtype != torch.float32 or tuple(spfh.shape) != (n, BINS):
        raise ValueError(f"spfh must be a float32 [{n}, {BINS}] tensor")
    idx, cnt = _lists(idx, cnt, n)
    lib = _lib.require_gpu()
    out = torch.empty((n, BINS), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.gcl_fpfh_combine(_lib.ptr(xyz), _lib.ptr(spfh.contiguous()), n, _lib.ptr(idx), _lib.ptr(cnt),
                                    idx.shape[1], int(bool(normalize)), _lib.ptr(out), _lib.stream()), "gcl_fpfh_combine")
    return out


def compute_fpfh_feature(xyz, normals, radius, max_nn=100, offsets=None, normalize=False):
    """open3d's ``compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn))``: float32 [N, 33].  ``normalize=True``
    applies what the reference's loaders apply to FPFH, f / (|f|_2 + 1e-6) (scripts/SC2_PCR/dataset.py:73-74, 227-228)."""
    xyz, radius, max_nn = _points(xyz), _radius(radius), _max_nn(max_nn)
    normals = _normals(normals, xyz)
    off = _offsets_host(offsets, xyz.shape[0])
    idx, cnt = radius_neighbours(xyz, radius, max_nn, off)
    return fpfh_from_spfh(xyz, spfh_from_neighbours(xyz, normals, idx, cnt), idx, cnt, normalize)


def fpfh_descriptors(xyz, voxel_size, viewpoint=None, offsets=None, normalize=True):
    """The usual recipe for a cloud downsampled at ``voxel_size``: normals at radius 2 voxels / 30 neighbours, FPFH at
    radius 5 voxels / 100 neighbours.  Returns ``(normals [N, 3], features [N, 33])``."""
    voxel_size = _radius(voxel_size)
    normals = estimate_normals(xyz, 2.0 * voxel_size, 30, viewpoint, offsets)
    return normals, compute_fpfh_feature(xyz, normals, 5.0 * voxel_size, 100, offsets, normalize)
