"""The raw-scan loaders' augmentation restated in numpy, element by element (no BLAS on the points), in the two arithmetics the
reference has -- what csrc/data.hip's AUG_F32 / AUG_F64 must reproduce bit for bit.

* ``affine``      T_c = [R | R (-centroid)] (sample_random_trans / follow_presampled_trans, lib/colocation_data_loader.py:38-50),
                  every dot product ((a b + c d) + e f) in fp64.
* ``apply_f32``   the co-location loaders (apply_transform casts the transform to float32, :80-85; ``scale * xyz`` stays float32):
                  y = (((x0 r0 + x1 r1) + x2 r2) + t) * fp32(scale), every operation rounded to float32.
* ``apply_f64``   the pair loaders (lib/data_loaders.py:125-129 keeps float64): y = scale * (((x0 r0 + x1 r1) + x2 r2) + t).
A cloud that is not rotated stays float32 in both loaders: y = x * fp32(scale).
numpy rounds every elementwise operation on its own (no fused multiply-add across two ufunc calls).
"""
import numpy as np


def affine(R, centroid):
    R = np.asarray(R, dtype=np.float64)
    c = [float(v) for v in centroid]
    T = np.eye(4)
    T[:3, :3] = R
    for i in range(3):
        T[i, 3] = (float(R[i, 0]) * -c[0] + float(R[i, 1]) * -c[1]) + float(R[i, 2]) * -c[2]
    return T


def _rows(x, T, dtype):
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    T = np.asarray(T, dtype=np.float64).astype(dtype)
    x0, x1, x2 = x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy()
    return np.stack([((x0 * T[k, 0] + x1 * T[k, 1]) + x2 * T[k, 2]) + T[k, 3] for k in range(3)], axis=1)


def apply_f32(x, T=None, scale=None):
    """float32 [P, 3]."""
    y = np.asarray(x, dtype=np.float32) if T is None else _rows(x, T, np.float32)
    if scale is not None:
        y = y * np.float32(scale)
    assert y.dtype == np.float32
    return y


def apply_f64(x, T=None, scale=None):
    """float64 [P, 3] of a rotated cloud; a cloud without a rotation stays float32 (returned as the float64 of that)."""
    if T is None:
        return apply_f32(x, None, scale).astype(np.float64)
    y = _rows(x, T, np.float64)
    if scale is not None:
        y = np.float64(scale) * y
    return y


def coords_f32(y, voxel):
    """floor(y / fp32(voxel)) as the co-location loaders voxelise float32 points."""
    return np.floor(np.asarray(y, dtype=np.float32) / np.float32(voxel)).astype(np.int32)


def coords_f64(y, voxel):
    """floor(y / voxel) in float64, as the pair loaders' sparse_quantize sees float64 points."""
    return np.floor(np.asarray(y, dtype=np.float64) / float(voxel)).astype(np.int32)


def first_of_every_voxel(coords):
    """Rows of the first point of every voxel, ascending (sparse_quantize's ``return_index``)."""
    _, first = np.unique(coords, axis=0, return_index=True)
    return np.sort(first)


def follow_list_M(T0, M, Tc, scale=None):
    """lib/colocation_data_loader.py:358 and :369."""
    out = T0 @ np.asarray(M, dtype=np.float64) @ np.linalg.inv(Tc)
    if scale is not None:
        out[:3, 3] = scale * out[:3, 3]
    return out


def augment_sample_f32(sample, centroids):
    """A ``build_batch_gpu`` sample with ``"rotation"`` / ``"scale"`` keys -> the key-less sample a host loader would hand over:
    clouds through ``apply_f32``, ``list_M`` followed, ``radius`` scaled.  ``centroids``: [n_clouds, 3] fp64 of the clouds."""
    R, scale = sample.get("rotation"), sample.get("scale")
    out = {k: v for k, v in sample.items() if k not in ("rotation", "scale")}
    Ts = [affine(R, c) if R is not None else None for c in centroids]
    out["xyz"] = [apply_f32(x, T, scale) for x, T in zip(sample["xyz"], Ts)]
    eye = np.eye(4)
    out["list_M"] = [follow_list_M(eye if R is None else Ts[0], M, eye if R is None else Ts[j + 1], scale)
                     for j, M in enumerate(sample["list_M"])]
    out["radius"] = float(sample["radius"]) * scale if scale is not None else float(sample["radius"])
    return out
