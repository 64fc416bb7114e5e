"""Ground-truth correspondences of scan pairs on the GPU (csrc/pairmatch.hip, gcl_amd/util/pointcloud.py,
gcl_amd/lib/pair_data_gpu.py) against the brute-force fp64 oracle tests/pair_matches_oracle.py.

Every comparison is exact (``torch.equal`` / ``np.array_equal``): indices have no tolerance, and the floats of a batch dict are
copies of the input points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_matches_oracle as MO      # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_matches(xyz0, xyz1, T, radius, voxel, K=None):
    from gcl_amd.util.pointcloud import get_matching_indices_batch
    pairs, totals, cnt = get_matching_indices_batch(dev(xyz0), [0, len(xyz0)], dev(xyz1), [0, len(xyz1)], [T], [radius], voxel,
                                                    K=K, return_counts=True)
    return pairs.cpu().numpy(), totals, cnt.cpu().numpy()


def check(got, want):
    (pairs, totals, cnt), (wp, wc) = got, want
    assert np.array_equal(cnt, wc)
    assert totals == [len(wp)]
    assert pairs.dtype == np.int64 and np.array_equal(pairs, wp)


# ---- 1. natural pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [None, 1, 5])
@pytest.mark.parametrize("radius", MO.RADII_A)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_natural_pairs(seed, radius, K):
    xyz0, xyz1, T = MO.scene_a(seed)
    assert len(xyz0) > 4 * 256          # several workgroups of the kernels and of the scan
    check(gpu_matches(xyz0, xyz1, T, radius, 0.3, K), MO.scene_a_matches(seed, radius, K))


def test_single_pair_wrapper_and_caller_table():
    from gcl_amd.lib.colocation_data_gpu import sparse_quantize_gpu
    from gcl_amd.util.pointcloud import get_matching_indices
    xyz0, xyz1, T = MO.scene_a(0)
    want, _ = MO.scene_a_matches(0, 0.45, 5)
    s, t = dev(xyz0), dev(xyz1)
    assert np.array_equal(get_matching_indices(s, t, T, 0.45, K=5, voxel_size=0.3).cpu().numpy(), want)
    _, index, table = sparse_quantize_gpu(t, 0.3, batch_id=0, return_table=True)
    assert len(index) == len(xyz1)
    assert np.array_equal(get_matching_indices(s, t, T, 0.45, K=5, voxel_size=0.3, table=table).cpu().numpy(), want)
    with pytest.raises(ValueError, match="voxel_size"):
        get_matching_indices(s, t, T, 0.45)


# ---- 2. lattice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turned", [False, True])
@pytest.mark.parametrize("radius,K", [(2.0, None), (3.9, None), (3.9, 100)])
def test_lattice(radius, K, turned):
    """r = 2: the strict boundary (d2 = 4 excluded) and six-way ties ordered by row; r = 3.9: 9^3 candidate voxels and 251 hits
    per interior query, so the order inside a query goes past one wave's width."""
    xyz0, xyz1, T, interior = MO.lattice(turned)
    got = gpu_matches(xyz0, xyz1, T, radius, 1.0, K)
    full = {2.0: 27, 3.9: 251}[radius]
    assert (got[2][interior] == (full if K is None else min(full, K))).all()
    check(got, MO.matches(xyz0, xyz1, T, radius, K))


def test_radius_of_four_voxels_is_refused():
    xyz0, xyz1, T, _ = MO.lattice(False)
    with pytest.raises(RuntimeError, match="supported below 4"):
        gpu_matches(xyz0, xyz1, T, 4.0, 1.0)


# ---- 3. frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.45, 1.17])
def test_moved_and_rotated_frames(radius):
    xyz0, xyz1, T = MO.scene_a_moved(0)
    want = MO.matches(xyz0, xyz1, T, radius)
    assert len(want[0]) > 5000
    check(gpu_matches(xyz0, xyz1, T, radius, 0.3), want)


@pytest.mark.parametrize("rv", [1.5, 3.9])
def test_edge_of_the_packable_range(rv):
    """Voxel 0.025 m, coordinates to +-32767 voxels: no hit is lost to the rounding of the query's voxel, negative coordinates
    floor towards -inf."""
    xyz0, xyz1, T, v = MO.scene_far()
    want = MO.matches(xyz0, xyz1, T, rv * v)
    assert len(want[0]) > 1000
    check(gpu_matches(xyz0, xyz1, T, rv * v, v), want)


# ---- 4. ragged batch ----------------------------------------------------------------------------------------------------
def _ragged():
    a0, a1, Ta = MO.scene_a(1)
    Tfar = np.eye(4)
    Tfar[0, 3] = 50.0
    T1 = MO.rotation((0, 0, 1), 3.0)
    return [(a0, a1, Ta, 0.54), (a0[:1], (a0[:1].astype(np.float64) @ T1[:3, :3].T).astype(np.float32), T1, 0.36),
            (a0[:0], a1[:700], Ta, 0.45), (a0[:900], a1[:900], Tfar @ Ta, 1.17)]


@pytest.mark.parametrize("K", [None, 3])
def test_ragged_batch_equals_single_calls_and_oracle(K):
    from gcl_amd.util.pointcloud import get_matching_indices_batch
    items = _ragged()
    o0 = np.concatenate([[0], np.cumsum([len(i[0]) for i in items])])
    o1 = np.concatenate([[0], np.cumsum([len(i[1]) for i in items])])
    X0, X1 = dev(np.concatenate([i[0] for i in items])), dev(np.concatenate([i[1] for i in items]))
    args = (X0, o0, X1, o1, [i[2] for i in items], [i[3] for i in items], 0.3)
    runs = [get_matching_indices_batch(*args, K=K, return_counts=True) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and torch.equal(runs[0][2], runs[1][2])
    pairs, totals, cnt = runs[0]
    singles = [gpu_matches(*i, 0.3, K) for i in items]
    oracle = [MO.matches(*i, K) for i in items]
    assert totals == [len(o[0]) for o in oracle] and totals[1] == 1 and totals[2] == 0 and totals[3] == 0 and totals[0] > 5000
    assert np.array_equal(cnt.cpu().numpy(), np.concatenate([o[1] for o in oracle]))
    for s, o in zip(singles, oracle):
        check(s, o)
    assert np.array_equal(pairs.cpu().numpy(), np.concatenate([s[0] for s in singles]))
    absolute = get_matching_indices_batch(*args, K=K, absolute=True)
    shift = np.concatenate([np.tile([[o0[b], o1[b]]], (totals[b], 1)) for b in range(4)])
    assert np.array_equal(absolute.cpu().numpy(), pairs.cpu().numpy() + shift)


# ---- 5. bad input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["offsets", "radius"])
def test_bad_offsets_or_radius_set_the_status_and_write_nothing(bad):
    from gcl_amd import _lib
    from gcl_amd.util.pointcloud import pack_params, target_table
    lib = _lib.require_gpu()
    xyz0, xyz1, T = MO.scene_a(2)
    n0, n1 = len(xyz0), len(xyz1)
    s, t = dev(xyz0), dev(xyz1)
    table, cap = target_table(t, [0, n1], 0.3)
    o0 = [0, n0 + 1] if bad == "offsets" else [0, n0]
    radii = [0.45] if bad == "offsets" else [0.6]              # 0.6 > radius_max = 0.45
    host, lay = pack_params(o0, [0, n1], [T], radii)
    params = host.to(DEV)
    at = lambda name: ctypes.c_void_p(params.data_ptr() + 8 * lay[name][0])
    cnt = torch.full((n0,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.empty(lib.gcl_pair_matches_scratch_len(n0), dtype=torch.int32, device=DEV)
    meta = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    pairs = torch.full((1000, 2), -7, dtype=torch.int64, device=DEV)
    common = (_lib.ptr(s), n0, at("offsets0"), _lib.ptr(t), n1, at("offsets1"), at("table_row0"), 1, _lib.ptr(table), cap, 0, 1,
              0.3, at("trans"), at("radii"), 0.45, 0)
    st = _lib.stream()
    _lib.check(lib.gcl_pair_matches_count(*common, _lib.ptr(cnt), _lib.ptr(scratch), _lib.ptr(meta), st))
    _lib.check(lib.gcl_pair_matches_emit(*common, 0, _lib.ptr(scratch), _lib.ptr(meta), _lib.ptr(pairs), 1000, st))
    assert meta.tolist() == [-7, 1 if bad == "offsets" else 2, -7]
    assert (cnt == -7).all() and (pairs == -7).all()
    if bad == "offsets":
        from gcl_amd.util.pointcloud import get_matching_indices_batch
        with pytest.raises(ValueError, match="refused"):
            get_matching_indices_batch(s, o0, t, [0, n1], [T], [0.45], 0.3, table=(table, cap))


def test_target_with_two_points_in_a_voxel_raises():
    from gcl_amd.util.pointcloud import get_matching_indices
    xyz0, xyz1, T = MO.scene_a(0)
    twice = np.concatenate([xyz1, xyz1[5:6] + np.float32(1e-3)])
    assert (np.floor(twice[-1] / np.float32(0.3)) == np.floor(xyz1[5] / np.float32(0.3))).all()
    with pytest.raises(ValueError, match="share a voxel"):
        get_matching_indices(dev(xyz0), dev(twice), T, 0.45, voxel_size=0.3)


# ---- 6. the batch builder -----------------------------------------------------------------------------------------------
_RAW = {}


def raw_pairs():
    """Four raw pairs as a pair dataset holds them before voxelisation: ray-cast scans of one scene from two poses 10 m apart
    (cropped to 11 m around the point half way, to keep the brute-force oracle quick), each cloud under its own random
    rotation, the pair's scale applied; the third pair's transform is off by 50 m (no match)."""
    if _RAW:
        return _RAW["pairs"]
    from gcl_amd import synthetic
    out = []
    for b in range(4):
        rng = np.random.RandomState(40 + b)
        scene = synthetic.make_scene(20 + b, n_boxes=12)
        M = np.eye(4)
        M[0, 3] = -10.0
        clouds = []
        for k, (x, mid) in enumerate(((0.0, 5.0), (10.0, -5.0))):
            p = synthetic.raycast(scene, np.array([x, 0.0, 0.0]), 300 + 2 * b + k)
            clouds.append(p[np.linalg.norm(p - np.array([mid, 0.0, 0.0], dtype=np.float32), axis=1) < 11.0])
        T0, T1 = synthetic._random_rotation(rng, np.pi / 4), synthetic._random_rotation(rng, np.pi / 4)
        if b == 2:
            M[1, 3] = 50.0
        scale = 0.8 + 0.4 * rng.rand()
        trans = T1 @ M @ np.linalg.inv(T0)
        trans[:3, 3] *= scale
        out.append({"xyz0": (scale * synthetic._apply(T0, clouds[0])).astype(np.float32),
                    "xyz1": (scale * synthetic._apply(T1, clouds[1])).astype(np.float32), "trans": trans,
                    "radius": 0.45 * scale})
    _RAW["pairs"] = out
    return out


def host_batch(pairs, voxel, K=None):
    """KITTIPairDataset.__getitem__ :494-536 per pair + collate_pair_fn, restated on the host."""
    from gcl_amd.MinkowskiEngine import utils as me_utils
    items = []
    for p in pairs:
        kept = []
        for k in ("xyz0", "xyz1"):
            _, sel = me_utils.sparse_quantize(p[k] / np.float32(voxel), return_index=True)
            kept.append(p[k][sel])
        m, _ = MO.matches(kept[0], kept[1], p["trans"], p["radius"], K)
        c = [np.floor(x / np.float32(voxel)).astype(np.int32) for x in kept]
        items.append((kept[0], kept[1], c[0], c[1], np.ones((len(c[0]), 1), np.float32), np.ones((len(c[1]), 1), np.float32), m,
                      p["trans"]))
    return MO.collate_pairs(items)


def test_build_pair_batch_gpu_equals_the_host_restatement():
    from gcl_amd.lib.pair_data_gpu import build_pair_batch_gpu
    pairs = raw_pairs()
    want = host_batch(pairs, 0.3)
    got = build_pair_batch_gpu(pairs, 0.3, DEV)
    assert len(want["len_batch"]) == 3 and len(want["correspondences"]) > 3000
    assert set(got) == set(want)
    for k, w in want.items():
        if k == "len_batch":
            assert got[k] == w
            continue
        g = got[k]
        assert g.is_cuda and str(g.dtype) == "torch." + str(w.dtype), k
        assert np.array_equal(g.cpu().numpy(), w), k
    again = build_pair_batch_gpu(pairs, 0.3, DEV)
    assert all(torch.equal(again[k], got[k]) for k in got if k != "len_batch")
    k2 = build_pair_batch_gpu(pairs[:2], 0.3, DEV, K=2, stream=torch.cuda.Stream(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(k2["correspondences"].cpu().numpy(), host_batch(pairs[:2], 0.3, K=2)["correspondences"])


# ---- 7. it trains -------------------------------------------------------------------------------------------------------
def test_contrastive_step_on_the_device_made_batch_equals_the_host_batch():
    """One seed, one set of draws: the step on the device-made dict and on the same content as host tensors return the same
    loss and parts bit for bit (the forward path has no atomics).  Parameters after the step are not
    compared: the loss backward's float atomics differ in the last bit by design."""
    from gcl_amd.lib import trainer as T
    from gcl_amd.lib.colocation_trainer import make_config
    from gcl_amd.lib.pair_data_gpu import build_pair_batch_gpu
    from gcl_amd.model import load_model
    batch = build_pair_batch_gpu(raw_pairs(), 0.3, DEV)
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}
    results = []
    for b in (batch, host):
        torch.manual_seed(4)
        model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV)
        tr = T.ContrastiveLossTrainer(make_config(batch_size=4, lr=0.1, momentum=0.8, weight_decay=1e-4), model=model, device=DEV)
        np.random.seed(9)
        draws = tr.draw_for(b)
        loss, parts, n_rows = tr.train_step(b, draws)
        assert n_rows == len(b["sinput0_C"]) + len(b["sinput1_C"])
        results.append([float(loss)] + [float(p) for p in parts])
    assert np.isfinite(results[0]).all() and results[0][1] > 0 and results[0][2] > 0
    assert results[0] == results[1]
