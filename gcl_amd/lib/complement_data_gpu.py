"""The complement pair loaders on the GPU: what ``PairComplementKittiDataset.__getitem__`` / ``PairComplementNuscenesDataset
.__getitem__`` (lib/complement_data_loader.py:576-716, :1028-1130) x batch size + ``collate_complement_pair_fn`` (:1224-1279)
produce from raw scans and poses -- the validation loader of every GCL run and the test loader of scripts/test_kitti.py --
with every tensor resident on the device, without open3d and without per-point host work.

Unlike ``build_pair_batch_gpu`` (``KITTIPairDataset``, float64) these loaders cast every transform to float32
(``apply_transform``, :65-70) and voxelise by float32 division, and they also hand over the NEIGHBOURHOOD clouds
``pcd_nghb0`` / ``pcd_nghb1``: each of the 2 x 2 k complement scans moved by its pose, then by the centre cloud's rotation,
cropped to the centre scan's range, concatenated in order and voxelised (csrc/nghb.hip).

The 2 B centre clouds of a batch are the coordinate table's clouds 2 b + s, as in ``build_pair_batch_gpu``; the 2 B
neighbourhood clouds follow them as clouds 2 B + 2 b + s, so the shared tail (``pair_data_gpu.sides_and_matches``) finds the
targets where it always did.  The file readers, the ICP cache files, ``mutate_neighbour``, ``downsample_single`` and the choice of
pairs stay with the caller; ``complement_pairs_from_scans`` assembles the poses from ``refine_pair_poses`` and
``multiway_registration``.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib import augment
from gcl_amd.lib.colocation_data_gpu import AUG_F32, _cap
from gcl_amd.lib.pair_data_gpu import filled_starts, sides_and_matches

MAX_SAMPLES = 16          # the voxeliser's table holds 64 clouds, a sample uses 4
PLACEHOLDER = ((1, 1), (2, 2), (3, 3))          # lib/complement_data_loader.py:685


def _scan(x, what):
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [P, 3], got {x.shape}")
    return x


def _mat4(M, what):
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"{what} must be a finite 4 x 4 matrix")
    return M


def build_complement_pair_batch_gpu(raw_samples, voxel_size, device, K=None, stream=None, scale_neighbourhood=False,
                                    placeholder_matches=True):
    """``raw_samples``: 1 .. 16 dicts ``{"xyz0", "xyz1": raw float32 [P, 3] host scans, "cmpl0", "cmpl1": lists of raw complement
    scans, "list_M0", "list_M1": their 4 x 4 transforms complement -> centre, "trans": 4 x 4 (cloud 0 -> cloud 1), "radius",
    optionally the draws "rotation0", "rotation1" (3 x 3), "scale"}`` (``augment.draw_complement_pair`` makes them; they pass
    ``augment.checked_*`` before any GPU work).  One sample is one ``__getitem__`` with ``load_neighbourhood``, in the loaders'
    float32 arithmetic, every product and sum rounded on its own, ``y = ((x0 r0 + x1 r1) + x2 r2) + t``:

    1. complement scan k is moved by ``f32(M_k)``;
    2. with a rotation, ``T_s = [R_s | R_s (-centroid_s)]`` (the centroid of the raw centre scan, ``gcl_cloud_centroids``): the
       centre scan is moved by ``f32(T_s)``, the moved complement points AGAIN by ``f32(T_s)`` (on the rounded result of step 1,
       the two are not composed), ``trans = T1 @ trans @ inv(T0)`` in fp64 on the host;
    3. ``max_s`` = the largest float32 ``(x^2 + y^2) + z^2`` of the moved centre scan, before any scale;
    4. the neighbourhood of side s = its complement points in scan order, then point order, where ``(x^2 + y^2) + z^2 < max_s``
       (strictly).  It is NOT scaled, as in the reference; ``scale_neighbourhood=True`` multiplies it by ``fp32(scale)`` too;
    5. with a scale the centre clouds are multiplied by ``fp32(scale)``, ``trans[:3, 3]`` and ``radius`` by ``scale`` (the
       nuScenes loader leaves the translation unscaled, which puts its ground truth off; that is not reproduced);
    6. all four clouds are voxelised: the first point of every voxel ``floor(y / fp32(voxel_size))`` (float32 division);
    7. ``correspondences = get_matching_indices(pcd0, pcd1, trans, radius)`` by the device matcher; a pair without any match gets
       the loaders' three placeholder rows (1, 1), (2, 2), (3, 3) and is listed under ``"placeholder_pairs"`` -- ValueError if
       one of its clouds has fewer than 4 rows.  ``placeholder_matches=False``: such a pair is left out instead, exactly as
       ``build_pair_batch_gpu`` leaves it out.

    Returns the dict of ``collate_complement_pair_fn`` with device tensors: ``pcd0`` / ``pcd1`` / ``pcd_nghb0`` / ``pcd_nghb1``
    LISTS of per-pair float32 [n, 3] tensors (an empty tensor for a side whose complement points are all cropped, or that has
    none), ``sinput{0,1}_C`` int32 [N, 4] with the pair's number in column 0, ``sinput{0,1}_F`` ones, ``correspondences``
    int64 [P, 2] with the running start indices added, ``T_gt`` float32 [4 B, 4], ``len_batch``; and two keys of this
    repository: ``"placeholder_pairs"`` and ``"len_matches"`` (rows of ``correspondences`` per listed pair).  Samples WITHOUT
    ``"cmpl0"`` / ``"cmpl1"`` (the test phase, :717-) give the dict of ``collate_debug_pair_fn``: no ``pcd_nghb*`` keys; a
    batch may not mix the two kinds.

    Host reads per batch, each waiting for ``stream`` (default: the current one) only -- THREE: the kept points per side
    (with the centre clouds' affines), the rows per cloud, the match totals.  A batch without any complement point makes two."""
    lib = _lib.require_gpu()
    dev = torch.device(device)
    B = len(raw_samples)
    if not 1 <= B <= MAX_SAMPLES:
        raise ValueError(f"1 .. {MAX_SAMPLES} samples per batch (64 clouds share the table, a sample uses 4)")
    voxel = float(voxel_size)
    if not (0.0 < voxel < 3.0e38):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    with_cmpl = [s.get("cmpl0") is not None and s.get("cmpl1") is not None for s in raw_samples]
    if any(with_cmpl) != all(with_cmpl) or any((s.get("cmpl0") is None) != (s.get("cmpl1") is None) for s in raw_samples):
        raise ValueError("either every sample carries cmpl0 and cmpl1 (validation) or none does (the test phase)")
    nghb = all(with_cmpl)
    n_sides = 2 * B
    n_clouds = 4 * B if nghb else 2 * B
    clouds = [_scan(s[k], k) for s in raw_samples for k in ("xyz0", "xyz1")]
    if any(len(x) == 0 for x in clouds):
        raise ValueError("an empty centre scan has neither a centroid nor a range to crop to")
    offs_c = np.zeros(n_sides + 1, dtype=np.int64)
    offs_c[1:] = np.cumsum([len(x) for x in clouds])
    P = int(offs_c[-1])
    trans = [_mat4(s["trans"], "trans") for s in raw_samples]
    radii = [float(s["radius"]) for s in raw_samples]
    rots = [augment.checked_rotation(s[k], k) if s.get(k) is not None else None for s in raw_samples
            for k in ("rotation0", "rotation1")]
    scales = [augment.checked_scale(s["scale"]) if s.get("scale") is not None else None for s in raw_samples]
    scans, scan_M, scan_side = [], [], []
    if nghb:
        for b, s in enumerate(raw_samples):
            for k in (0, 1):
                xs, Ms = list(s[f"cmpl{k}"]), list(s.get(f"list_M{k}") or [])
                if len(xs) != len(Ms):
                    raise ValueError(f"sample {b}: {len(xs)} scans in cmpl{k} but {len(Ms)} transforms in list_M{k}")
                scans += [_scan(x, f"cmpl{k}") for x in xs]
                scan_M += [_mat4(M, f"list_M{k}") for M in Ms]
                scan_side += [2 * b + k] * len(xs)
    n_scans = len(scans)
    if n_scans > _lib.NGHB_MAX_SCANS:
        raise ValueError(f"at most {_lib.NGHB_MAX_SCANS} complement scans per batch, got {n_scans}")
    scan_off = np.zeros(n_scans + 1, dtype=np.int64)
    scan_off[1:] = np.cumsum([len(x) for x in scans])
    Pc = int(scan_off[-1])
    side_arr = np.asarray(scan_side, dtype=np.int32)
    side_off = scan_off[np.searchsorted(side_arr, np.arange(n_sides + 1))]      # first scan of every side -> its point offset
    # one pinned block, one copy (doubles first: they stay 8-byte aligned): identity frames for gcl_loader_points_aug, the
    # per-cloud augmentation table, the scans' transforms, then the complement points and the centre points -- the centre
    # points last, so that the kept complement points can be written right behind them: gcl_voxel_coords_aug wants one array
    n_fr, n_sa = n_clouds * 24, n_scans * 24
    a_at, s_at = n_fr, 2 * n_fr
    c_at = s_at + n_sa
    x_at = c_at + 3 * Pc
    host = torch.empty(x_at + 3 * P, dtype=torch.float32, pin_memory=True)
    host[:n_fr].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.eye(4)[:3].reshape(-1)
    rows = [augment.affine_rows(rots[c], scales[c // 2]) for c in range(n_sides)]
    if nghb:          # a neighbourhood cloud arrives moved; all that is left to apply is the scale, if it is asked for
        rows += [augment.affine_rows(None, scales[c // 2] if scale_neighbourhood else None) for c in range(n_sides)]
    host[a_at:s_at].view(torch.float64).view(n_clouds, 12).numpy()[:] = np.stack(rows)
    if n_scans:
        host[s_at:c_at].view(torch.float64).view(n_scans, 12).numpy()[:] = np.stack([M[:3].reshape(-1) for M in scan_M])
    hc = host[c_at:x_at].view(Pc, 3).numpy()
    for k, x in enumerate(scans):
        hc[scan_off[k]:scan_off[k + 1]] = x
    hx = host[x_at:].view(P, 3).numpy()
    for c, x in enumerate(clouds):
        hx[offs_c[c]:offs_c[c + 1]] = x
    st_ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(dev), st_ctx:
        st = _lib.stream()
        d = torch.empty(host.numel() + 3 * Pc, dtype=torch.float32, device=dev)
        d[:host.numel()].copy_(host, non_blocking=True)
        frames, aug_dev, scan_aff, cmpl, xyz_raw = d[:n_fr], d[a_at:s_at], d[s_at:c_at], d[c_at:x_at], d[x_at:]
        off = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * t.element_size())
        i64p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        # meta: rows, status, the clouds' first rows; behind them (8-byte aligned) the affines T_c as doubles; behind those
        # the kept complement points per side and their total
        a0 = (8 + n_clouds + 1 + 1) // 2 * 2
        k0 = a0 + 24 * n_clouds
        meta = torch.zeros(k0 + n_sides + 1, dtype=torch.int32, device=dev)
        cent = torch.zeros(3 * n_clouds, dtype=torch.float64, device=dev)       # a neighbourhood cloud is never rotated
        cscr = torch.empty(lib.gcl_cloud_centroids_scratch_len(P, n_sides), dtype=torch.float64, device=dev)
        _lib.check(lib.gcl_cloud_centroids(_lib.ptr(xyz_raw), P, i64p(offs_c), n_sides, _lib.ptr(cscr), _lib.ptr(cent), st),
                   "gcl_cloud_centroids")
        _lib.check(lib.gcl_cloud_affines(_lib.ptr(aug_dev), _lib.ptr(cent), n_clouds, off(meta, a0), st), "gcl_cloud_affines")
        kept = [0] * (n_sides + 1)
        if Pc:
            maxv = torch.empty(n_sides, dtype=torch.float32, device=dev)
            moved = torch.empty(3 * Pc, dtype=torch.float32, device=dev)
            flags = torch.empty(Pc, dtype=torch.int32, device=dev)
            nscr = torch.empty(lib.gcl_nghb_scratch_len(Pc), dtype=torch.int32, device=dev)
            _lib.check(lib.gcl_nghb_range_max(_lib.ptr(xyz_raw), P, i64p(offs_c), n_sides, _lib.ptr(aug_dev), off(meta, a0),
                                              _lib.ptr(maxv), st), "gcl_nghb_range_max")
            _lib.check(lib.gcl_nghb_flags(_lib.ptr(cmpl), Pc, i64p(scan_off), side_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          n_scans, n_sides, _lib.ptr(scan_aff), _lib.ptr(aug_dev), off(meta, a0), _lib.ptr(maxv),
                                          _lib.ptr(moved), _lib.ptr(flags), st), "gcl_nghb_flags")
            _lib.check(lib.gcl_nghb_compact(_lib.ptr(moved), _lib.ptr(flags), Pc, i64p(side_off), n_sides, _lib.ptr(nscr),
                                            off(xyz_raw, 3 * P), off(meta, k0), st), "gcl_nghb_compact")
            kept = meta.cpu().numpy()[k0:].tolist()              # host read 1: the kept complement points per side
        offs = np.concatenate([offs_c, P + np.cumsum(kept[:n_sides])]).astype(np.int64) if nghb else offs_c
        Pt = int(offs[-1])
        raw = torch.empty((Pt, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.gcl_voxel_coords_aug(_lib.ptr(xyz_raw), Pt, i64p(offs), n_clouds, voxel, _lib.ptr(aug_dev),
                                            off(meta, a0), AUG_F32, _lib.ptr(raw), st), "gcl_voxel_coords_aug")
        cap = _cap(Pt)
        table = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        scratch = torch.empty(lib.gcl_scan_scratch_len(Pt), dtype=torch.int32, device=dev)
        coords = torch.empty((Pt, 4), dtype=torch.int32, device=dev)
        index = torch.empty(Pt, dtype=torch.int64, device=dev)
        _lib.check(lib.gcl_unique_coords(_lib.ptr(raw), Pt, _lib.ptr(table), cap, _lib.ptr(scratch), _lib.ptr(coords),
                                         _lib.ptr(index), off(meta, 0), off(meta, 4), st), "gcl_unique_coords")
        _lib.check(lib.gcl_cloud_row_starts(_lib.ptr(coords), Pt, off(meta, 0), n_clouds, off(meta, 8), st),
                   "gcl_cloud_row_starts")
        xyz = torch.empty((Pt, 3), dtype=torch.float32, device=dev)
        xyz_cf = torch.empty((Pt, 3), dtype=torch.float32, device=dev)          # identity frames: a second copy nobody reads
        _lib.check(lib.gcl_loader_points_aug(_lib.ptr(xyz_raw), _lib.ptr(index), _lib.ptr(coords), Pt, off(meta, 0),
                                             _lib.ptr(frames), _lib.ptr(aug_dev), off(meta, a0), AUG_F32, _lib.ptr(xyz),
                                             _lib.ptr(xyz_cf), st), "gcl_loader_points_aug")
        mh = meta.cpu().numpy()                                  # host read 2: rows, status, first rows, the affines T_c
        m = mh[:a0].tolist()
        if m[4]:
            raise ValueError(f"{m[4]} points outside the packable voxel range")
        T = [augment.affine4(r) for r in mh[a0:k0].view(np.float64).reshape(n_clouds, 12)[:n_sides]]
        for b in range(B):
            trans[b] = augment.follow_pair_trans(T[2 * b], T[2 * b + 1], trans[b], scales[b])
            if scales[b] is not None:
                radii[b] = radii[b] * scales[b]
        tg = torch.empty(16 * B, dtype=torch.float32, pin_memory=True)
        tg.view(B, 4, 4).numpy()[:] = np.stack(trans).astype(np.float32)          # the reference's .float()
        T_all = torch.empty((4 * B, 4), dtype=torch.float32, device=dev)
        T_all.view(-1).copy_(tg, non_blocking=True)
        starts = filled_starts(m[8:8 + n_clouds + 1])
        xyz0, xyz1, C0, C1, n0, n1, o0, o1, pairs, totals = sides_and_matches(xyz, coords, starts, B, trans, radii, table, cap,
                                                                              voxel, K)      # host read 3: the match totals
        cum = np.concatenate([[0], np.cumsum(totals)]).astype(np.int64)
        keep, chunks, placeholders = [], [], []
        for b in range(B):
            if totals[b] > 0:
                chunks.append(pairs[cum[b]:cum[b + 1]])
            elif placeholder_matches:
                if n0[b] < 4 or n1[b] < 4:
                    raise ValueError(f"pair {b} has no match and its clouds have {n0[b]} and {n1[b]} rows: the placeholder "
                                     "matches (1, 1), (2, 2), (3, 3) need 4 rows in each")
                rows_b = np.asarray(PLACEHOLDER, dtype=np.int64) + np.array([[o0[b], o1[b]]], dtype=np.int64)
                chunks.append(torch.from_numpy(rows_b).to(dev))
                placeholders.append(b)
            else:
                continue
            keep.append(b)
        corr = pairs if not placeholders else torch.cat(chunks)
        ones = lambda n: torch.ones((n, 1), dtype=torch.float32, device=dev)
        out = {"pcd0": [xyz0[o0[b]:o0[b + 1]] for b in keep], "pcd1": [xyz1[o1[b]:o1[b + 1]] for b in keep]}
        if nghb:
            for k in (0, 1):
                out[f"pcd_nghb{k}"] = [xyz[starts[n_sides + 2 * b + k]:starts[n_sides + 2 * b + k + 1]] for b in keep]
        out.update({"sinput0_C": C0, "sinput0_F": ones(len(C0)), "sinput1_C": C1, "sinput1_F": ones(len(C1)),
                    "correspondences": corr,
                    "T_gt": T_all if len(keep) == B else (torch.cat([T_all[4 * b:4 * b + 4] for b in keep]) if keep else T_all[:0]),
                    "len_batch": [[n0[b], n1[b]] for b in keep], "placeholder_pairs": placeholders,
                    "len_matches": [int(c.shape[0]) for c in chunks]})
        return out


def pair_dicts(batch):
    """A B-sample batch of ``build_complement_pair_batch_gpu`` as B one-pair dicts -- batch id 0, ``correspondences`` re-based
    to the pair's own rows, ``T_gt`` [4, 4], the ``pcd*`` lists of one tensor -- so that one build feeds B iterations of
    ``validate_pairs`` / ``eval_pairs``, which read ``d["pcd0"][0]``.  No host read.  ValueError for a batch that left pairs
    out (``placeholder_matches=False`` and a pair without a match): its rows cannot be told apart here."""
    lens = batch["len_batch"]
    if sum(n for n, _ in lens) != len(batch["sinput0_C"]) or sum(n for _, n in lens) != len(batch["sinput1_C"]):
        raise ValueError("the batch left pairs out; build it with placeholder_matches=True")
    out, a0, a1, am = [], 0, 0, 0
    for b, ((n0, n1), nm) in enumerate(zip(lens, batch["len_matches"])):
        d = {k: [batch[k][b]] for k in ("pcd0", "pcd1", "pcd_nghb0", "pcd_nghb1") if k in batch}
        for k, a, n in ((0, a0, n0), (1, a1, n1)):
            C = batch[f"sinput{k}_C"][a:a + n].clone()
            C[:, 0] = 0
            d[f"sinput{k}_C"], d[f"sinput{k}_F"] = C, batch[f"sinput{k}_F"][a:a + n]
        d["correspondences"] = batch["correspondences"][am:am + nm] - torch.tensor([[a0, a1]], dtype=torch.int64).to(
            batch["correspondences"].device)
        d["T_gt"] = batch["T_gt"][4 * b:4 * b + 4]
        d["len_batch"], d["len_matches"] = [[n0, n1]], [nm]
        d["placeholder_pairs"] = [0] if b in batch["placeholder_pairs"] else []
        out.append(d)
        a0, a1, am = a0 + n0, a1 + n1, am + nm
    return out


def complement_pairs_from_scans(samples, velo2cam, num_complement_one_side, voxel_size, device, poses="old", icp_voxel_size=0.05,
                                **build_kw):
    """Raw scans and poses -> the batch dict: the pose half of the loaders (``refine_pair_poses`` = their ``_get_icp``,
    ``multiway_registration`` = theirs), then ``build_complement_pair_batch_gpu``.

    ``samples``: 1 .. 16 dicts ``{"xyz0", "xyz1": raw scans, "pos0", "pos1": their 4 x 4 poses, "cmpl0", "cmpl1": the
    ``2 * num_complement_one_side`` raw complement scans of either centre, "pos_cmpl0", "pos_cmpl1": their poses, "radius",
    optionally "rotation0" / "rotation1" / "scale"}``; without ``cmpl*`` (the test phase) only the pair's pose is made.
    ``poses="old"`` (``use_old_pose``): ``trans`` of all pairs from ONE ``refine_pair_poses`` call whose ``M`` is
    ``_pair_init(velo2cam, pos0, pos1)`` -- the loaders' ``_get_icp(drive, t_1, t_0, ...)``, :583 -- and ``list_M*`` from
    batched ``multiway_registration`` calls (one, as long as the voxeliser's 64-cloud table holds the batch's scans).
    ``poses="given"``: ``inv(pos1) @ pos0`` and ``inv(pos_core) @ pos_k`` (:561-565, :1035).  ``build_kw`` goes to the
    builder."""
    from gcl_amd.lib.icp import refine_pair_poses
    from gcl_amd.lib.multiway import _pair_init, multiway_registration
    if poses not in ("old", "given"):
        raise ValueError(f'poses is "old" or "given", got {poses!r}')
    k = int(num_complement_one_side)
    velo2cam = _mat4(velo2cam, "velo2cam")
    nghb = [s.get("cmpl0") is not None for s in samples]
    pos = [[_mat4(s[f"pos{j}"], f"pos{j}") for j in (0, 1)] for s in samples]
    for s, has in zip(samples, nghb):
        for j in (0, 1):
            if has and (len(s[f"cmpl{j}"]) != 2 * k or len(s[f"pos_cmpl{j}"]) != 2 * k):
                raise ValueError(f"{2 * k} complement scans and poses a side, got {len(s[f'cmpl{j}'])} and {len(s[f'pos_cmpl{j}'])}")
    if poses == "given":
        trans = [np.linalg.inv(p1) @ p0 for p0, p1 in pos]
        list_M = [[[np.linalg.inv(pos[i][j]) @ _mat4(p, "pos_cmpl") for p in s[f"pos_cmpl{j}"]] for j in (0, 1)] if has else None
                  for i, (s, has) in enumerate(zip(samples, nghb))]
    else:
        trans = list(refine_pair_poses([{"xyz0": s["xyz0"], "xyz1": s["xyz1"], "M": _pair_init(velo2cam, p0, p1)}
                                        for s, (p0, p1) in zip(samples, pos)], icp_voxel_size))
        sides = [(i, j) for i, has in enumerate(nghb) if has for j in (0, 1)]
        per_call = max(1, 64 // (1 + 2 * k))
        got = {}
        for a in range(0, len(sides), per_call):
            part = sides[a:a + per_call]
            Ms = multiway_registration([samples[i][f"xyz{j}"] for i, j in part], [list(samples[i][f"cmpl{j}"]) for i, j in part],
                                       [pos[i][j] for i, j in part], [list(samples[i][f"pos_cmpl{j}"]) for i, j in part],
                                       velo2cam, k, icp_voxel_size)
            got.update(dict(zip(part, Ms)))
        list_M = [[got[(i, 0)], got[(i, 1)]] if has else None for i, has in enumerate(nghb)]
    raw = []
    for s, T, Ms in zip(samples, trans, list_M):
        r = {key: s[key] for key in ("xyz0", "xyz1", "radius", "rotation0", "rotation1", "scale") if s.get(key) is not None}
        r["trans"] = T
        if Ms is not None:
            r.update(cmpl0=list(s["cmpl0"]), cmpl1=list(s["cmpl1"]), list_M0=Ms[0], list_M1=Ms[1])
        raw.append(r)
    return build_complement_pair_batch_gpu(raw, voxel_size, device, **build_kw)
