"""The raw-scan loaders' rotation, centring and scale on the GPU (csrc/data.hip: gcl_cloud_centroids, gcl_cloud_affines,
gcl_voxel_coords_aug, gcl_loader_points_aug; the ``"rotation"`` / ``"scale"`` keys of ``build_batch_gpu`` and
``build_pair_batch_gpu``) against the numpy restatement tests/augment_oracle.py.

Every comparison of a batch is exact: the device must reproduce the reference's two arithmetics bit for bit.  The oracle takes
the clouds' centroids from ``cloud_centroids_gpu``; that function has its own test against ``math.fsum``."""
import ctypes
import functools
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as AO           # noqa: E402
import pair_matches_oracle as MO      # noqa: E402

DEV = "cuda:0"
VOXEL = 0.3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def centroids_of(clouds):
    from gcl_amd.lib.colocation_data_gpu import cloud_centroids_gpu
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    return cloud_centroids_gpu(dev(np.concatenate(clouds).astype(np.float32)), offs).cpu().numpy()


# ---- 1. centroids -------------------------------------------------------------------------------------------------------
# one point; either side of a wave and of a block's 256 running sums; several chunks of 1024 points with a ragged last one;
# more than 256 chunks, so that the second level's own 256 running sums take more than one chunk sum each
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 300001)


def test_centroids_are_bitwise_reproducible_and_within_the_fp64_summation_bound():
    rng = np.random.RandomState(7)
    clouds = [(rng.normal(size=(n, 3)) * 30.0 + np.array([40.0, -25.0, 3.0])).astype(np.float32) for n in SIZES]
    assert len(clouds) == 9
    batch = centroids_of(clouds)
    assert batch.shape == (9, 3) and batch.dtype == np.float64
    assert np.array_equal(bits(batch), bits(centroids_of(clouds)))                       # twice
    alone = np.concatenate([centroids_of([c]) for c in clouds])
    assert np.array_equal(bits(batch), bits(alone))                                      # each alone
    # in another batch: the other way round, an empty cloud in between
    other = centroids_of([clouds[8], clouds[3], clouds[3][:0], clouds[7]])
    assert np.array_equal(bits(other[[0, 1, 3]]), bits(batch[[8, 3, 7]])) and (other[2] == 0).all()
    for c, got in zip(clouds, batch):
        P = len(c)
        for k in range(3):
            x = [float(v) for v in c[:, k]]
            want = math.fsum(x) / P
            bound = (P - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in x) / P        # any fp64 summation order's worst case
            print(f"P = {P} axis {k}: |centroid - fsum / P| = {abs(got[k] - want):.3e}, bound {bound:.3e}")
            assert abs(got[k] - want) <= bound


def test_bad_arguments_set_the_status_and_write_nothing():
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    assert lib.gcl_cloud_centroids_scratch_len(-1, 2) == 0 and lib.gcl_cloud_centroids_scratch_len(4097, 2) == 3 * (4 + 2)
    P, n = 10, 2
    xyz = torch.zeros((P, 3), dtype=torch.float32, device=DEV)
    f64 = lambda k: torch.full((k,), -7.0, dtype=torch.float64, device=DEV)
    scratch, cent, aug, aff = f64(64), f64(3 * n), f64(12 * n), f64(12 * n)
    coords = torch.full((P, 4), -7, dtype=torch.int32, device=DEV)
    index = torch.zeros(P, dtype=torch.int64, device=DEV)
    n_dev = torch.full((1,), P, dtype=torch.int32, device=DEV)
    own, cf = (torch.full((P, 3), -7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    offs = lambda *v: (ctypes.c_int64 * len(v))(*v)
    good, st, p = offs(0, 4, 10), _lib.stream(), _lib.ptr

    def refused(rc, word):
        assert rc == -1 and word in lib.gcl_last_error(), (rc, lib.gcl_last_error())

    refused(lib.gcl_cloud_centroids(None, P, good, n, p(scratch), p(cent), st), b"null")
    refused(lib.gcl_cloud_centroids(p(xyz), P, good, n, None, p(cent), st), b"null")
    refused(lib.gcl_cloud_centroids(p(xyz), P, good, n, p(scratch), None, st), b"null")
    refused(lib.gcl_cloud_centroids(p(xyz), P, offs(0, 4, 9), n, p(scratch), p(cent), st), b"offsets")
    refused(lib.gcl_cloud_centroids(p(xyz), P, offs(1, 4, 10), n, p(scratch), p(cent), st), b"offsets")
    refused(lib.gcl_cloud_centroids(p(xyz), P, offs(0, 11, 10), n, p(scratch), p(cent), st), b"offsets")
    refused(lib.gcl_cloud_centroids(p(xyz), 0, offs(0, 0, 0), n, p(scratch), p(cent), st), b"offsets")
    refused(lib.gcl_cloud_centroids(p(xyz), P, good, 0, p(scratch), p(cent), st), b"clouds")
    refused(lib.gcl_cloud_centroids(p(xyz), P, offs(*([0] * 65 + [10])), 65, p(scratch), p(cent), st), b"clouds")
    refused(lib.gcl_cloud_affines(None, p(cent), n, p(aff), st), b"null")
    refused(lib.gcl_cloud_affines(p(aug), None, n, p(aff), st), b"null")
    refused(lib.gcl_cloud_affines(p(aug), p(cent), n, None, st), b"null")
    refused(lib.gcl_cloud_affines(p(aug), p(cent), 0, p(aff), st), b"clouds")
    refused(lib.gcl_cloud_affines(p(aug), p(cent), 65, p(aff), st), b"clouds")
    for mode in (0, 3):
        refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, n, VOXEL, p(aug), p(aff), mode, p(coords), st), b"mode")
        refused(lib.gcl_loader_points_aug(p(xyz), p(index), p(coords), P, p(n_dev), p(aff), p(aug), p(aff), mode, p(own), p(cf),
                                          st), b"mode")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, n, VOXEL, None, p(aff), 1, p(coords), st), b"null")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, n, VOXEL, p(aug), None, 1, p(coords), st), b"null")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, n, VOXEL, p(aug), p(aff), 1, None, st), b"null")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, n, 0.0, p(aug), p(aff), 1, p(coords), st), b"voxel")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, offs(0, 4, 9), n, VOXEL, p(aug), p(aff), 2, p(coords), st), b"offsets")
    refused(lib.gcl_voxel_coords_aug(p(xyz), P, good, 65, VOXEL, p(aug), p(aff), 2, p(coords), st), b"clouds")
    refused(lib.gcl_loader_points_aug(p(xyz), p(index), p(coords), P, p(n_dev), p(aff), None, p(aff), 1, p(own), p(cf), st),
            b"null")
    refused(lib.gcl_loader_points_aug(p(xyz), p(index), p(coords), P, p(n_dev), p(aff), p(aug), p(aff), 1, None, p(cf), st),
            b"null")
    refused(lib.gcl_loader_points_aug(p(xyz), p(index), p(coords), 0, p(n_dev), p(aff), p(aug), p(aff), 1, p(own), p(cf), st),
            b"rows")
    torch.cuda.synchronize()
    for t in (scratch, cent, aug, aff, coords, own, cf):
        assert (t == -7).all()


# ---- 2. the co-location batch: the loaders' float32 arithmetic ----------------------------------------------------------------
CASES = ("rotation + scale", "rotation", "scale")
TENSORS = ("sinput_C", "sinput_F", "group", "index", "finest_flag", "xyz_own", "xyz_cf")


@functools.lru_cache(maxsize=None)
def plain_samples():
    """The scenes of test_build_batch_gpu_equals_the_cpu_loader, 2 x 3 clouds, as the scan files hold them: no rotation, no scale."""
    from gcl_amd import synthetic
    return tuple(synthetic.make_raw_sample(s, VOXEL, num_neighborhood=2, n_boxes=20, random_rotation=False, random_scale=False)
                 for s in (61, 62))


def keyed_samples(case):
    from gcl_amd.lib import augment
    out = []
    for si, s in enumerate(plain_samples()):
        s = dict(s)
        if "rotation" in case:
            s["rotation"] = augment.sample_rotation(np.random.RandomState(100 + si), 360 if si == 0 else 90)
        if "scale" in case:
            s["scale"] = augment.draw_scale(random.Random(3 + si), 0.8, 1.2)
            assert s["scale"] is not None and s["scale"] != 1.0
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def batches(case):
    """(the batch the device augments, the key-less batch of the same samples augmented on the host by the oracle)."""
    from gcl_amd import synthetic
    from gcl_amd.lib.colocation_data_gpu import build_batch_gpu
    keyed = keyed_samples(case)
    hosted = [AO.augment_sample_f32(s, centroids_of(s["xyz"])) for s in keyed]
    assert not any("rotation" in s or "scale" in s for s in hosted)
    with torch.cuda.device(DEV):
        got = build_batch_gpu(keyed, VOXEL, DEV, jitter=synthetic.raw_sample_jitter(keyed))
        want = build_batch_gpu(hosted, VOXEL, DEV, jitter=synthetic.raw_sample_jitter(hosted))
        torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize("case", CASES)
def test_f32_batch_equals_the_host_augmented_batch_bit_for_bit(case):
    got, want = batches(case)
    assert set(got) == set(want) and set(TENSORS) < set(got)
    for k in TENSORS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert got["batch_lengths"] == want["batch_lengths"] and got["cloud_rows"] == want["cloud_rows"]
    assert got["index_hash"] is None and len(got["cloud_rows"]) == 6 and len(got["group"]) > 200
    # and it is another batch than the scans voxelised as they are
    from gcl_amd.lib.colocation_data_gpu import build_batch_gpu
    plain = build_batch_gpu(list(plain_samples()), VOXEL, DEV)
    assert plain["cloud_rows"] != got["cloud_rows"]


def test_a_batch_may_mix_samples_with_and_without_keys():
    from gcl_amd.lib.colocation_data_gpu import build_batch_gpu
    keyed = keyed_samples("rotation + scale")
    mixed = [keyed[0], plain_samples()[1]]
    hosted = [AO.augment_sample_f32(keyed[0], centroids_of(keyed[0]["xyz"])), plain_samples()[1]]
    got, want = build_batch_gpu(mixed, VOXEL, DEV), build_batch_gpu(hosted, VOXEL, DEV)
    for k in TENSORS:
        assert torch.equal(got[k], want[k]), k
    assert got["cloud_rows"] == want["cloud_rows"]


def test_one_train_step_on_the_device_augmented_batch_gives_the_same_loss():
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    cfg = make_config(batch_size=2, num_pos_per_batch=64, num_hn_samples_per_batch=128, lr=0.0, weight_decay=0.0)
    losses = []
    for batch in batches("rotation + scale"):
        torch.manual_seed(3)
        np.random.seed(3)
        tr = FinestContrastiveLossTrainer(cfg, device=DEV)
        loss, parts, n = tr.train_step(batch)
        assert n == len(batch["sinput_C"])
        losses.append([loss.item()] + [float(v) for v in parts])
    assert np.isfinite(losses[0]).all() and losses[0][0] > 0
    assert losses[0] == losses[1]


def test_train_from_scans_passes_the_keys_through():
    """The loader threads' path: persistent workspaces, their own streams, the second upload from the pinned block."""
    from gcl_amd import synthetic
    from gcl_amd.lib.colocation_data_gpu import train_from_scans
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    cfg = make_config(batch_size=2, num_pos_per_batch=64, num_hn_samples_per_batch=128, lr=0.0, weight_decay=0.0)
    keyed = [keyed_samples(c) for c in CASES]
    hosted = [[AO.augment_sample_f32(s, centroids_of(s["xyz"])) for s in ks] for ks in keyed]
    runs = []
    for raw_batches in (keyed, hosted):
        torch.manual_seed(3)
        np.random.seed(3)
        tr = FinestContrastiveLossTrainer(cfg, device=DEV)
        steps = train_from_scans(tr, [raw_batches[i] for i in (0, 1, 2, 0)], voxel_size=VOXEL, jitter=synthetic.raw_sample_jitter)
        runs.append([l.item() for l, _, _ in steps])
        torch.cuda.synchronize()
    assert runs[0] == runs[1] and len(set(runs[0])) >= 3, runs


# ---- 3. the pair batch: the pair loaders' float64 arithmetic ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_pairs():
    """Three raw pairs as the scan files hold them: ray-cast scans of one scene from two poses 10 m apart (cropped to 11 m around
    the point half way and thinned, to keep the brute-force oracle quick), in sensor frames that lie some hundred metres from
    the origin -- the rounding of a float32 transform then moves points across voxel faces.  Pair 0 carries both rotations and
    a scale, pair 1 the rotations, pair 2 the scale alone."""
    from gcl_amd import synthetic
    from gcl_amd.lib import augment
    shift = np.array([300.0, -200.0, 10.0])
    out = []
    for b in range(3):
        scene = synthetic.make_scene(20 + b, n_boxes=12)
        clouds = []
        for k, (x, mid) in enumerate(((0.0, 5.0), (10.0, -5.0))):
            p = synthetic.raycast(scene, np.array([x, 0.0, 0.0]), 300 + 2 * b + k)
            p = p[np.linalg.norm(p - np.array([mid, 0.0, 0.0], dtype=np.float32), axis=1) < 11.0][::2]
            clouds.append((p + shift).astype(np.float32))
        M = np.eye(4)                               # cloud 0 -> cloud 1 in the shifted frames: x1 = (x0 - shift) + (-10, 0, 0) + shift
        M[0, 3] = -10.0
        pair = {"xyz0": clouds[0], "xyz1": clouds[1], "trans": M, "radius": 0.45}
        if b < 2:
            pair["rotation0"] = augment.sample_rotation(np.random.RandomState(50 + 2 * b), 360)
            pair["rotation1"] = augment.sample_rotation(np.random.RandomState(51 + 2 * b), 360)
        if b != 1:
            pair["scale"] = 0.87 + 0.1 * b
        out.append(pair)
    return tuple(out)


def host_pair_batch(pairs, K=None):
    """KITTIPairDataset.__getitem__ :476-536 per pair + collate_pair_fn on the host: the oracle's fp64 points, numpy floor /
    unique in float64, the float32 representatives matched by the brute-force oracle.  Also returns how many points fall into
    another voxel when the same transform is evaluated in the co-location loaders' float32."""
    items, other_voxel = [], 0
    for p in pairs:
        scale = p.get("scale")
        cents = centroids_of([p["xyz0"], p["xyz1"]])
        Ts = [AO.affine(p[k], c) if p.get(k) is not None else None for k, c in zip(("rotation0", "rotation1"), cents)]
        kept, coords = [], []
        for x, T in zip((p["xyz0"], p["xyz1"]), Ts):
            y = AO.apply_f64(x, T, scale)
            if T is not None:
                c = AO.coords_f64(y, VOXEL)
                other_voxel += int((AO.coords_f32(AO.apply_f32(x, T, scale), VOXEL) != c).any(axis=1).sum())
            else:                               # a cloud that is not rotated is float32 up to and through sparse_quantize
                c = AO.coords_f32(y.astype(np.float32), VOXEL)
            sel = AO.first_of_every_voxel(c)
            kept.append(y[sel].astype(np.float32))
            coords.append(c[sel])
        eye = np.eye(4)
        trans = (Ts[1] if Ts[1] is not None else eye) @ p["trans"] @ np.linalg.inv(Ts[0] if Ts[0] is not None else eye)
        radius = p["radius"]
        if scale is not None:
            trans[:3, 3] = scale * trans[:3, 3]
            radius = radius * scale
        m, _ = MO.matches(kept[0], kept[1], trans, radius, K)
        items.append((kept[0], kept[1], coords[0], coords[1], np.ones((len(kept[0]), 1), np.float32),
                      np.ones((len(kept[1]), 1), np.float32), m, trans))
    return MO.collate_pairs(items), other_voxel


def test_f64_pair_batch_equals_the_host_restatement():
    from gcl_amd.lib.pair_data_gpu import build_pair_batch_gpu
    pairs = list(plain_pairs())
    want, other_voxel = host_pair_batch(pairs)
    print("points in another voxel under float32 evaluation:", other_voxel)
    assert other_voxel >= 1                 # the mode matters on these inputs
    assert len(want["len_batch"]) == 3 and len(want["correspondences"]) > 3000
    got = build_pair_batch_gpu(pairs, VOXEL, DEV)
    assert set(got) == set(want)
    assert got["len_batch"] == want["len_batch"]
    bad = []
    for k, w in want.items():
        if k == "len_batch":
            continue
        g = got[k]
        assert g.is_cuda and str(g.dtype) == "torch." + str(w.dtype), k
        g = g.cpu().numpy()
        if g.shape != w.shape or not np.array_equal(g, w):
            print(k, "differs:", g.shape, w.shape, int((g != w).any(axis=1).sum()) if g.shape == w.shape else "")
            bad.append(k)
    assert not bad, bad
    again = build_pair_batch_gpu(pairs, VOXEL, DEV, stream=torch.cuda.Stream(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(again[k], got[k]) for k in got if k != "len_batch")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_bad_keys_are_refused():
    from gcl_amd.lib.colocation_data_gpu import build_batch_gpu
    from gcl_amd.lib.pair_data_gpu import build_pair_batch_gpu
    keyed, pairs = keyed_samples("rotation + scale"), list(plain_pairs())
    skew = np.eye(3)
    skew[0, 1] = 1e-5

    def sample(**kw):
        s = dict(keyed[0])
        s.update(kw)
        return [s, keyed[1]]

    def pair(**kw):
        p = dict(pairs[0])
        p.update(kw)
        return [p, pairs[1]]

    with pytest.raises(ValueError, match="rotation"):
        build_batch_gpu(sample(rotation=skew), VOXEL, DEV)
    for bad in (0.0, -0.9):
        with pytest.raises(ValueError, match="scale"):
            build_batch_gpu(sample(scale=bad), VOXEL, DEV)
        with pytest.raises(ValueError, match="scale"):
            build_pair_batch_gpu(pair(scale=bad), VOXEL, DEV)
    with pytest.raises(ValueError, match="empty cloud"):
        build_batch_gpu(sample(xyz=[keyed[0]["xyz"][0], keyed[0]["xyz"][1][:0], keyed[0]["xyz"][2]]), VOXEL, DEV)
    with pytest.raises(ValueError, match="rotation1"):
        build_pair_batch_gpu(pair(rotation1=skew), VOXEL, DEV)
    with pytest.raises(ValueError, match="empty cloud"):
        build_pair_batch_gpu(pair(xyz0=pairs[0]["xyz0"][:0]), VOXEL, DEV)
