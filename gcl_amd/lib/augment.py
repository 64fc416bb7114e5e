"""The raw-scan loaders' augmentation: what is drawn on the host, and the host's share of what the device applies.

The reference's datasets turn every cloud about its centroid and scale the sample right before voxelisation
(``ColocationKittiDataset.__getitem__``, lib/colocation_data_loader.py:349-370; ``KITTIPairDataset.__getitem__``,
lib/data_loaders.py:476-492).  ``build_batch_gpu`` / ``build_pair_batch_gpu`` do the per-point work on the device (csrc/data.hip:
the centroids, ``T_c = [R_c | R_c (-centroid_c)]``, the transformed points); this module holds

* the DRAWS, which consume the same generators in the same order as the reference: ``sample_rotation`` (the rotation half of
  ``sample_random_trans``, :38-43) and ``draw_scale`` (the two ``random.random()`` calls of :362-364);
* the checks a sample's ``"rotation"`` / ``"scale"`` keys pass before any GPU work;
* the 4 x 4 compositions of the ground truth with the affines the device returns, in fp64 with the reference's expressions.
"""
import numpy as np


def sample_rotation(randg, rotation_range=360):
    """R (3 x 3, fp64) of ``sample_random_trans(pcd, randg, rotation_range)``: the draws ``randg.rand(3)`` then ``randg.rand(1)``,
    the angle ``rotation_range * pi / 180 * (u - 0.5)`` kept literally (the reference's datasets pass ``np.pi / 4`` here, i.e.
    less than half a degree), about the drawn axis.  Rodrigues' formula instead of the reference's ``scipy.linalg.expm`` of the
    same skew matrix: two fp64 evaluations of one rotation."""
    axis = randg.rand(3) - 0.5
    theta = float((rotation_range * np.pi / 180.0 * (randg.rand(1) - 0.5))[0])
    n = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def draw_scale(pyrandom, min_scale, max_scale):
    """The scale of lib/colocation_data_loader.py:362-364 from ``pyrandom`` (the ``random`` module or a ``random.Random``):
    ``random() < 0.95`` decides, a second ``random()`` places it in [min_scale, max_scale).  None: this sample is not scaled
    (the second draw is then not made, as in the reference)."""
    if pyrandom.random() < 0.95:
        return min_scale + (max_scale - min_scale) * pyrandom.random()
    return None


def draw_complement_pair(randg, pyrandom, rotation_range, random_rotation, random_scale, min_scale, max_scale):
    """The draws of one ``PairComplement*Dataset.__getitem__`` in the reference's order (lib/complement_data_loader.py:598-605,
    :656-658; the nuScenes twin :1040-1044, :1089-1091): the T0 draws, then the T1 draws -- each ``sample_rotation``'s
    ``rand(3)``, ``rand(1)`` from ``randg`` -- then the scale's one or two ``random()`` calls from ``pyrandom``.
    ``rotation_range`` is passed on literally: the KITTI loader passes ``2 * np.pi`` under its hard-coded
    ``test_augmentation`` (which also switches the rotation on, so pass ``random_rotation=True`` for it), ``np.pi / 4``
    otherwise, as the nuScenes loader always does.  Without ``random_rotation`` / ``random_scale`` the respective generator
    is not touched.  Returns ``{"rotation0", "rotation1", "scale"}`` (None: not drawn), the keys
    ``build_complement_pair_batch_gpu`` reads."""
    R0 = R1 = None
    if random_rotation:
        R0 = sample_rotation(randg, rotation_range)
        R1 = sample_rotation(randg, rotation_range)
    return {"rotation0": R0, "rotation1": R1, "scale": draw_scale(pyrandom, min_scale, max_scale) if random_scale else None}


def checked_rotation(R, what="rotation"):
    """``R`` as a 3 x 3 fp64 array; ValueError unless max|R^T R - I| <= 1e-6."""
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-6:
        raise ValueError(f"{what}: not a 3 x 3 rotation (|R^T R - I| above 1e-6)")
    return R


def checked_scale(scale):
    scale = float(scale)
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError(f"scale: {scale} is not a positive number")
    return scale


def affine_rows(R, scale):
    """One row of the device's per-cloud table: R (9, row-major; identity if None), the scale (1.0 if None), rotated (0 / 1), 0."""
    row = np.zeros(12, dtype=np.float64)
    row[:9] = (np.eye(3) if R is None else R).reshape(-1)
    row[9] = 1.0 if scale is None else scale
    row[10] = 0.0 if R is None else 1.0
    return row


def affine4(rows12):
    """4 x 4 of one row-major 3 x 4 affine."""
    T = np.eye(4)
    T[:3] = np.asarray(rows12, dtype=np.float64).reshape(3, 4)
    return T


def follow_list_M(T0, M, Tc, scale=None):
    """``list_M[i] = T0 @ list_M[i] @ inv(Tc)`` (lib/colocation_data_loader.py:358), then the translation scaled (:369)."""
    out = T0 @ np.asarray(M, dtype=np.float64) @ np.linalg.inv(Tc)
    if scale is not None:
        out[:3, 3] = scale * out[:3, 3]
    return out


def follow_pair_trans(T0, T1, trans, scale=None):
    """``trans = T1 @ trans @ inv(T0)`` (lib/data_loaders.py:479), its translation scaled with the clouds as the co-location and
    complement loaders do (lib/colocation_data_loader.py:369)."""
    out = T1 @ np.asarray(trans, dtype=np.float64) @ np.linalg.inv(T0)
    if scale is not None:
        out[:3, 3] = scale * out[:3, 3]
    return out
