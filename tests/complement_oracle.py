"""The complement pair loaders (``PairComplement*Dataset.__getitem__`` with ``load_neighbourhood``,
lib/complement_data_loader.py:576-716, and ``collate_complement_pair_fn`` / ``collate_debug_pair_fn``, :1224-1333) restated in
numpy, element by element in float32 in the written-out order -- what ``build_complement_pair_batch_gpu`` must reproduce bit for
bit.  Built from tests/augment_oracle.py (``apply_f32``: y = ((x0 r0 + x1 r1) + x2 r2) + t with the transform rounded to
float32, no BLAS on the points) and tests/pair_matches_oracle.py (the brute-force matcher).

    c_k   = f32(M_k) x                         every complement scan                                    (:576-579)
    c_k   = f32(T_s) c_k,  centre = f32(T_s) x  with a rotation, T_s = [R | R (-centroid)]; the second transform acts on the
                                               rounded result of the first                              (:600-612)
    max_s = max (x^2 + y^2) + z^2              float32, over the moved centre scan, before the scale     (:623-624)
    nghb  = the c_k in scan order, then point order, where (x^2 + y^2) + z^2 < max_s (strictly)        (:625-628)
    centre *= fp32(scale); trans[:3, 3] *= scale; radius *= scale; the neighbourhood stays unscaled     (:656-662)
    first point of every voxel floor(y / fp32(voxel)) of all four clouds; matches; placeholders         (:671-685)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as AO           # noqa: E402
import pair_matches_oracle as MO      # noqa: E402

PLACEHOLDER = ((1, 1), (2, 2), (3, 3))


def range2(y):
    """float32 [P]: (x^2 + y^2) + z^2, every operation rounded to float32 (``(xyz ** 2).sum(-1)`` of a float32 array)."""
    y = np.asarray(y, dtype=np.float32)
    r = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    assert r.dtype == np.float32
    return r


def moved_complements(cmpl, list_M, T=None):
    """The complement scans after ``f32(M_k)`` and, with a rotation, ``f32(T)`` on the result: a list of float32 [P_k, 3]."""
    out = []
    for x, M in zip(cmpl, list_M):
        c = AO.apply_f32(np.asarray(x, dtype=np.float32).reshape(-1, 3), M)
        out.append(c if T is None else AO.apply_f32(c, T))
    return out


def crop(moved, max_s):
    """(all moved points concatenated in scan order, the mask of those strictly inside ``max_s``)."""
    cat = np.concatenate(moved) if moved else np.zeros((0, 3), dtype=np.float32)
    return cat, range2(cat) < np.float32(max_s)


def voxelise(y, voxel):
    """(representative points float32 [n, 3], coordinates int32 [n, 3], selected rows): the first point of every voxel."""
    y = np.asarray(y, dtype=np.float32).reshape(-1, 3)
    c = AO.coords_f32(y, voxel)
    sel = AO.first_of_every_voxel(c) if len(y) else np.zeros(0, dtype=np.int64)
    return y[sel], c[sel], sel


def build_sample(s, centroids, voxel, K=None, scale_neighbourhood=False):
    """One ``__getitem__``.  ``s``: a raw sample of ``build_complement_pair_batch_gpu``; ``centroids``: fp64 [2, 3] of the two
    raw centre scans.  Returns a dict: ``pcd0, pcd1, coords0, coords1, matches, trans, radius`` and, when the sample carries
    ``cmpl*``, ``pcd_nghb0, pcd_nghb1`` plus ``max`` (the two float32 maxima) and ``kept`` (the two crop masks)."""
    scale = s.get("scale")
    Ts = [AO.affine(s[k], c) if s.get(k) is not None else None for k, c in zip(("rotation0", "rotation1"), centroids)]
    centre = [AO.apply_f32(s[k], T) for k, T in zip(("xyz0", "xyz1"), Ts)]
    out = {}
    if s.get("cmpl0") is not None:
        out["max"], out["kept"] = [], []
        for k in (0, 1):
            max_s = range2(centre[k]).max()
            cat, keep = crop(moved_complements(s[f"cmpl{k}"], s[f"list_M{k}"], Ts[k]), max_s)
            ng = cat[keep]
            if scale_neighbourhood and scale is not None:
                ng = ng * np.float32(scale)
            out[f"pcd_nghb{k}"] = voxelise(ng, voxel)[0]
            out["max"].append(max_s)
            out["kept"].append(keep)
    eye = np.eye(4)
    trans = (Ts[1] if Ts[1] is not None else eye) @ np.asarray(s["trans"], dtype=np.float64) @ np.linalg.inv(
        Ts[0] if Ts[0] is not None else eye)
    radius = float(s["radius"])
    if scale is not None:
        centre = [y * np.float32(scale) for y in centre]
        trans[:3, 3] = scale * trans[:3, 3]
        radius = radius * scale
    for k in (0, 1):
        out[f"pcd{k}"], out[f"coords{k}"], _ = voxelise(centre[k], voxel)
    out["matches"], _ = MO.matches(out["pcd0"], out["pcd1"], trans, radius, K)
    out["trans"], out["radius"] = trans, radius
    return out


def collate(items, placeholder_matches=True):
    """``collate_complement_pair_fn`` (``collate_debug_pair_fn`` when the items have no neighbourhood) on ``build_sample``
    dicts, with the placeholder rows of :681-685 for a pair without a match -- or, ``placeholder_matches=False``, that pair
    left out as ``collate_pair_fn`` leaves it out.  ``correspondences`` stays int64."""
    nghb = "pcd_nghb0" in items[0]
    keys = ("pcd0", "pcd1") + (("pcd_nghb0", "pcd_nghb1") if nghb else ())
    out = {k: [] for k in keys}
    mb, tb, lb, placeholders, lm = [], [], [], [], []
    C, F = ([], []), ([], [])
    s0 = s1 = 0
    for b, it in enumerate(items):
        n0, n1 = len(it["coords0"]), len(it["coords1"])
        m = np.asarray(it["matches"], dtype=np.int64).reshape(-1, 2)
        if len(m) == 0 and placeholder_matches:
            if n0 < 4 or n1 < 4:
                raise ValueError("placeholder matches need 4 rows in each cloud")
            m = np.asarray(PLACEHOLDER, dtype=np.int64)
            placeholders.append(b)
        if len(m):
            for k in keys:
                out[k].append(np.asarray(it[k], dtype=np.float32))
            tb.append(np.asarray(it["trans"], dtype=np.float64).astype(np.float32))
            mb.append(m + np.array([[s0, s1]], dtype=np.int64))
            lb.append([n0, n1])
            lm.append(len(m))
        s0 += n0
        s1 += n1
        for k in (0, 1):
            c = np.asarray(it[f"coords{k}"], dtype=np.int32).reshape(-1, 3)
            C[k].append(np.concatenate([np.full((len(c), 1), b, dtype=np.int32), c], axis=1))
            F[k].append(np.ones((len(c), 1), dtype=np.float32))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    out.update({"sinput0_C": np.concatenate(C[0]), "sinput0_F": np.concatenate(F[0]), "sinput1_C": np.concatenate(C[1]),
                "sinput1_F": np.concatenate(F[1]), "correspondences": cat(mb, (0, 2), np.int64),
                "T_gt": cat(tb, (0, 4), np.float32), "len_batch": lb, "placeholder_pairs": placeholders, "len_matches": lm})
    return out


# ---- the same chain as ONE composed fp64 transform: what the scenes must tell apart from the loaders' arithmetic ----------
def composed_f64(cmpl, list_M, T, max_s, voxel):
    """(keep mask, voxel coordinates) of the complement points when ``T @ M_k`` is composed in fp64 and applied once."""
    pts = []
    for x, M in zip(cmpl, list_M):
        G = (np.eye(4) if T is None else T) @ np.asarray(M, dtype=np.float64)
        pts.append(MO.transform(np.asarray(x, dtype=np.float32).reshape(-1, 3), G))
    y = np.concatenate(pts) if pts else np.zeros((0, 3))
    r2 = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    return r2 < np.float64(max_s), np.floor(y / float(voxel)).astype(np.int32)


# ---- how far another evaluation order of the same float32 chain (BLAS's ``pts @ R.T + T``) may land ------------------------
U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)


def stage_bound(x, T, b_in=None, dT=None):
    """fp64 [P, 3]: per point and output coordinate, the largest distance between two float32 evaluations of
    ``f32(T) x`` in any order -- each is within gamma_4 (|x0 r0| + |x1 r1| + |x2 r2| + |t|) of the exact value, gamma_4 =
    4u / (1 - 4u), u = 2^-24 -- plus what the inputs' own distance ``b_in`` [P, 3] becomes through |R|, plus the transforms'
    distance ``dT`` ([3, 4], entrywise, before the cast to float32; the cast adds 2u |T|)."""
    x = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    A = np.abs(np.asarray(T, dtype=np.float64)[:3].astype(np.float32).astype(np.float64))
    b = 2 * GAMMA4 * (x @ A[:, :3].T + A[:, 3])
    if b_in is not None:
        b = b + (np.asarray(b_in) + 0.0) @ A[:, :3].T
    if dT is not None:
        d = np.asarray(dT, dtype=np.float64) + 2 * U * A
        b = b + (x + (0.0 if b_in is None else b_in)) @ d[:, :3].T + d[:, 3]
    return b


def range_bound(y, b):
    """fp64 [P]: how far the float32 squared ranges of two points within ``b`` of each other may lie apart, about the fp64
    squared range of ``y``: sum 2 |y_i| b_i + b_i^2, and three float32 roundings of either evaluation."""
    y = np.abs(np.asarray(y, dtype=np.float32).astype(np.float64))
    r2 = (y * y).sum(axis=1)
    return (2 * y * b + b * b).sum(axis=1) + 2 * 3 * U * (r2 + (2 * y * b + b * b).sum(axis=1))


def range2_f64(y):
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    return (y * y).sum(axis=1)
