"""``build_complement_pair_batch_gpu`` (gcl_amd/lib/complement_data_gpu.py, csrc/nghb.hip) against the numpy restatement
tests/complement_oracle.py, bit for bit: every point, coordinate, correspondence, ``T_gt`` as float32 and ``len_batch``, on the
scenes of tests/complement_scenes.py (tests/test_oracle_complement.py proves without a GPU what each of them exercises).  The
oracle takes the centre scans' centroids from ``cloud_centroids_gpu``, which has its own test (tests/test_gpu_augment.py)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import complement_oracle as CO         # noqa: E402
import complement_scenes as CS         # noqa: E402

DEV = "cuda:0"
LISTS = ("pcd0", "pcd1", "pcd_nghb0", "pcd_nghb1")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def centroids_of(s):
    from gcl_amd.lib.colocation_data_gpu import cloud_centroids_gpu
    clouds = [np.asarray(s[k], dtype=np.float32) for k in ("xyz0", "xyz1")]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    return cloud_centroids_gpu(dev(np.concatenate(clouds)), offs).cpu().numpy()


@functools.lru_cache(maxsize=None)
def items(name, scale_neighbourhood=False):
    """The oracle's ``__getitem__`` of every sample of a scene, computed once."""
    return tuple(CO.build_sample(s, centroids_of(s), CS.VOXEL, scale_neighbourhood=scale_neighbourhood) for s in CS.scene(name))


def build(samples, **kw):
    from gcl_amd.lib.complement_data_gpu import build_complement_pair_batch_gpu
    out = build_complement_pair_batch_gpu(list(samples), CS.VOXEL, DEV, **kw)
    torch.cuda.synchronize()
    return out


def same(got, want):
    """Names of the entries of a device batch that are not bit for bit the oracle's."""
    bad = [] if set(got) == set(want) else ["keys: " + " ".join(sorted(set(got) ^ set(want)))]
    for k, w in want.items():
        g = got.get(k)
        if g is None:
            continue
        if k in LISTS:
            ok = len(g) == len(w) and all(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == a.shape and
                                           np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32)) for t, a in zip(g, w))
        elif isinstance(w, list):
            ok = g == w
        else:
            ok = g.is_cuda and str(g.dtype) == "torch." + str(w.dtype) and tuple(g.shape) == w.shape and np.array_equal(
                g.cpu().numpy().view(np.int32 if w.dtype == np.float32 else w.dtype), w.view(np.int32 if w.dtype == np.float32 else w.dtype))
        if not ok:
            print(k, "differs")
            bad.append(k)
    return bad


def equal_batches(a, b):
    return set(a) == set(b) and all(
        (len(a[k]) == len(b[k]) and all(torch.equal(x, y) for x, y in zip(a[k], b[k]))) if k in LISTS else
        (a[k] == b[k] if isinstance(a[k], list) else torch.equal(a[k], b[k])) for k in a)


# k = 3 with neither draw, the rotations, the scale, both; k = 1; the points at the maximum; a side cropped to nothing and one
# cropped of nothing; an empty complement scan and an empty complement list; a pair without a match; B = 3; the test phase
@pytest.mark.parametrize("name", CS.NAMES)
def test_batch_is_the_oracles_bit_for_bit(name):
    want = CO.collate(items(name))
    got = build(CS.scene(name))
    assert not same(got, want)
    if name.startswith("k3_"):
        assert len(want["correspondences"]) > 2500 and all(len(p) > 3000 for k in (2, 3) for p in want[LISTS[k]])
    if name == "all_none":
        assert tuple(got["pcd_nghb0"][0].shape) == (0, 3) and got["pcd_nghb0"][0].is_cuda
    if name in ("no_match", "batch3"):
        assert got["placeholder_pairs"] == [0 if name == "no_match" else 1]
    if name == "test_phase":
        assert "pcd_nghb0" not in got and len(got["pcd0"]) == 2


def test_scaled_neighbourhood_and_a_capped_k():
    for name in ("k1", "boundary"):
        want = CO.collate(items(name, True))
        assert not same(build(CS.scene(name), scale_neighbourhood=True), want)
        plain = CO.collate(items(name))
        assert not np.array_equal(want["pcd_nghb0"][0], plain["pcd_nghb0"][0])           # the keyword matters here
    s = CS.scene("k1")
    want = CO.collate([CO.build_sample(x, centroids_of(x), CS.VOXEL, K=1) for x in s])
    assert len(want["correspondences"]) < len(CO.collate(items("k1"))["correspondences"])
    assert not same(build(s, K=1), want)


def test_a_pair_without_a_match_is_left_out_on_request_and_small_clouds_are_refused():
    want = CO.collate(items("batch3"), placeholder_matches=False)
    got = build(CS.scene("batch3"), placeholder_matches=False)
    assert not same(got, want)
    assert got["placeholder_pairs"] == [] and len(got["len_batch"]) == 2 and tuple(got["T_gt"].shape) == (8, 4)
    tiny = CS.no_match_sample(3)
    with pytest.raises(ValueError, match="placeholder"):
        build([tiny])
    alone = build([tiny], placeholder_matches=False)
    assert alone["len_batch"] == [] and alone["pcd0"] == [] and tuple(alone["correspondences"].shape) == (0, 2)


def test_a_sample_is_bitwise_the_same_alone_anywhere_in_a_batch_and_twice():
    from gcl_amd.lib.complement_data_gpu import pair_dicts
    samples = CS.scene("batch3")
    whole = build(samples)
    assert equal_batches(whole, build(samples, stream=torch.cuda.Stream(DEV)))           # twice, on another stream
    alone = [build([s]) for s in samples]
    split = pair_dicts(whole)
    assert len(split) == 3
    for d, a in zip(split, alone):
        assert tuple(d["T_gt"].shape) == (4, 4) and int(d["sinput0_C"][:, 0].max()) == 0
        a = dict(a)
        assert equal_batches(d, a)
    turned = pair_dicts(build(samples[::-1]))[::-1]                                     # every sample at another position
    for d, a in zip(turned, alone):
        assert equal_batches(d, dict(a))
    assert split[1]["placeholder_pairs"] == [0] and split[0]["placeholder_pairs"] == []
    assert split[1]["correspondences"].tolist() == [[1, 1], [2, 2], [3, 3]]


def test_bad_samples_are_refused_before_any_gpu_work(monkeypatch):
    from gcl_amd import _lib
    from gcl_amd.lib.complement_data_gpu import build_complement_pair_batch_gpu
    s = dict(CS.scene("k1")[0])
    lib = _lib.require_gpu()
    monkeypatch.setattr(_lib, "check", lambda *a, **k: pytest.fail("a kernel entry was called"))
    skew = np.eye(3)
    skew[0, 1] = 1e-5
    for bad, word in ((dict(rotation0=skew), "rotation"), (dict(scale=-1.0), "scale"), (dict(xyz0=s["xyz0"][:0]), "empty"),
                      (dict(list_M0=s["list_M0"][:1]), "list_M0"), (dict(cmpl1=None), "cmpl"),
                      (dict(trans=np.eye(3)), "trans")):
        with pytest.raises(ValueError, match=word):
            build_complement_pair_batch_gpu([dict(s, **bad)], CS.VOXEL, DEV)
    with pytest.raises(ValueError, match="16"):
        build_complement_pair_batch_gpu([s] * 17, CS.VOXEL, DEV)
    with pytest.raises(ValueError, match="cmpl"):
        build_complement_pair_batch_gpu([s, CS.scene("test_phase")[0]], CS.VOXEL, DEV)
    assert lib is not None


def test_given_poses_are_composed_as_the_loaders_compose_them():
    """``poses="given"`` (``use_old_pose`` off): ``inv(pos1) @ pos0`` and ``inv(pos_core) @ pos_k``, then the builder."""
    from gcl_amd.lib.complement_data_gpu import complement_pairs_from_scans
    s = CS.scene("k1")[0]
    pos0 = CS.rigid(0.3, -0.1, (12.0, -7.0, 1.0))
    pos = {"pos0": pos0, "pos1": pos0 @ np.linalg.inv(s["trans"]),
           "pos_cmpl0": [pos0 @ M for M in s["list_M0"]]}
    pos["pos_cmpl1"] = [pos["pos1"] @ M for M in s["list_M1"]]
    given = {k: v for k, v in s.items() if k not in ("trans", "list_M0", "list_M1")}
    given.update(pos)
    want = dict(s, trans=np.linalg.inv(pos["pos1"]) @ pos0)
    for k in (0, 1):
        want[f"list_M{k}"] = [np.linalg.inv(pos[f"pos{k}"]) @ P for P in pos[f"pos_cmpl{k}"]]
    got = complement_pairs_from_scans([given], np.eye(4), 1, CS.VOXEL, DEV, poses="given")
    torch.cuda.synchronize()
    assert equal_batches(got, build([want])) and len(got["correspondences"]) > 100
    test_phase = {k: v for k, v in given.items() if "cmpl" not in k}
    got = complement_pairs_from_scans([test_phase], np.eye(4), 1, CS.VOXEL, DEV, poses="given", K=1)
    only = {k: v for k, v in want.items() if "cmpl" not in k and "list_M" not in k}
    assert "pcd_nghb0" not in got and equal_batches(got, build([only], K=1))
    with pytest.raises(ValueError, match="poses"):
        complement_pairs_from_scans([given], np.eye(4), 1, CS.VOXEL, DEV, poses="new")
    with pytest.raises(ValueError, match="complement scans"):
        complement_pairs_from_scans([given], np.eye(4), 3, CS.VOXEL, DEV, poses="given")


def test_kernels_at_a_three_launch_scan_against_numpy():
    """The entries alone at 600 000 complement points in 5 scans on 3 sides (one side without a scan): beyond the 524 288
    entries up to which the prefix sum runs in two launches.  Flags, moved points, kept counts and the compacted rows are
    numpy's bit for bit."""
    from gcl_amd import _lib
    import augment_oracle as AO
    lib = _lib.require_gpu()
    rng = np.random.RandomState(9)
    sizes, sides = [250000, 1, 0, 300000, 49999], [0, 0, 0, 2, 2]
    cmpl = (rng.normal(size=(sum(sizes), 3)) * 20.0).astype(np.float32)
    Ms = [CS.rigid(0.1 * k, 0.02 * k, (k, -k, 0.1 * k)) for k in range(5)]
    centre = [(rng.normal(size=(n, 3)) * 12.0).astype(np.float32) for n in (1025, 300, 1)]
    R = [CS.rotation(1), None, CS.rotation(2)]
    cent = [c.astype(np.float64).mean(axis=0) for c in centre]
    T = [AO.affine(r, c) if r is not None else None for r, c in zip(R, cent)]
    aug = np.stack([np.concatenate([(np.eye(3) if r is None else r).reshape(-1), [1.0, 0.0 if r is None else 1.0, 0.0]]) for r in R])
    aff = np.stack([(np.eye(4) if t is None else t)[:3].reshape(-1) for t in T])
    want_max = np.array([CO.range2(AO.apply_f32(c, t)).max() for c, t in zip(centre, T)], dtype=np.float32)
    scan_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    parts = np.split(cmpl, scan_off[1:-1])
    moved = np.concatenate([CO.moved_complements([x], [M], T[s])[0] for x, M, s in zip(parts, Ms, sides)])
    keep = CO.range2(moved) < want_max[np.repeat(sides, sizes)]
    assert 1000 < keep.sum() < len(keep) - 1000
    offs_c = np.concatenate([[0], np.cumsum([len(c) for c in centre])]).astype(np.int64)
    side_off = np.array([0, 250001, 250001, 600000], dtype=np.int64)
    side_arr = np.asarray(sides, dtype=np.int32)
    i64p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    with torch.cuda.device(DEV):
        st = _lib.stream()
        d_c, d_x, d_aug, d_aff = dev(np.concatenate(centre)), dev(cmpl), dev(aug), dev(aff)
        d_M = dev(np.stack([M[:3].reshape(-1) for M in Ms]))
        pc = len(cmpl)
        maxv = torch.empty(3, dtype=torch.float32, device=DEV)
        d_moved = torch.empty((pc, 3), dtype=torch.float32, device=DEV)
        flags = torch.empty(pc, dtype=torch.int32, device=DEV)
        out = torch.full((pc, 3), -7.0, dtype=torch.float32, device=DEV)
        kept = torch.empty(4, dtype=torch.int32, device=DEV)
        scr = torch.empty(lib.gcl_nghb_scratch_len(pc), dtype=torch.int32, device=DEV)
        _lib.check(lib.gcl_nghb_range_max(_lib.ptr(d_c), len(d_c), i64p(offs_c), 3, _lib.ptr(d_aug), _lib.ptr(d_aff), _lib.ptr(maxv), st))
        _lib.check(lib.gcl_nghb_flags(_lib.ptr(d_x), pc, i64p(scan_off), side_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 5, 3,
                                      _lib.ptr(d_M), _lib.ptr(d_aug), _lib.ptr(d_aff), _lib.ptr(maxv), _lib.ptr(d_moved), _lib.ptr(flags), st))
        _lib.check(lib.gcl_nghb_compact(_lib.ptr(d_moved), _lib.ptr(flags), pc, i64p(side_off), 3, _lib.ptr(scr), _lib.ptr(out),
                                        _lib.ptr(kept), st))
        torch.cuda.synchronize()
    assert np.array_equal(maxv.cpu().numpy().view(np.int32), want_max.view(np.int32))
    assert np.array_equal(d_moved.cpu().numpy().view(np.int32), moved.view(np.int32))
    assert np.array_equal(flags.cpu().numpy(), keep.astype(np.int32))
    n = int(keep.sum())
    assert kept.tolist() == [int(keep[:250001].sum()), 0, int(keep[250001:].sum()), n]
    got = out.cpu().numpy()
    assert np.array_equal(got[:n].view(np.int32), moved[keep].view(np.int32)) and (got[n:] == -7.0).all()


def test_scans_to_validation_meters_end_to_end():
    """The wiring: raw scans and poses -> ``complement_pairs_from_scans(poses="old")`` -> ``validate_pairs``.  The meters must
    be those of the same pairs built by the oracle from the poses the two existing stages return for the same scans."""
    import multiway_scenes as S
    import gcl_amd.lib.validation as V
    from gcl_amd.lib.complement_data_gpu import complement_pairs_from_scans, pair_dicts
    from gcl_amd.lib.icp import refine_pair_poses
    from gcl_amd.lib.multiway import _pair_init, multiway_registration
    from gcl_amd.model import load_model
    voxel, radius = 0.1, 0.15
    sets = [S.raw_set(seed, 4, copies=4) for seed in (1, 2)]          # four scans in a chain: 1 and 2 are the pair
    Vc = sets[0][3]
    samples = []
    for raw, _, pos, Vs in sets:
        # raw_set draws a velo2cam per seed and a loader has one: the poses are restated under the first set's
        pos = [Vc.T @ (np.linalg.inv(Vs.T) @ P @ Vs.T) @ np.linalg.inv(Vc.T) for P in pos]
        samples.append({"xyz0": raw[1], "pos0": pos[1], "cmpl0": [raw[0], raw[2]], "pos_cmpl0": [pos[0], pos[2]],
                        "xyz1": raw[2], "pos1": pos[2], "cmpl1": [raw[1], raw[3]], "pos_cmpl1": [pos[1], pos[3]], "radius": radius})
    samples[1].update(rotation0=CS.rotation(5), rotation1=CS.rotation(6), scale=0.9)
    with torch.cuda.device(DEV):
        batch = complement_pairs_from_scans(samples, Vc, 1, voxel, DEV, poses="old")
        trans = refine_pair_poses([{"xyz0": s["xyz0"], "xyz1": s["xyz1"], "M": _pair_init(Vc, s["pos0"], s["pos1"])} for s in samples])
        raw_samples = []
        for s, T in zip(samples, trans):
            r = {k: s[k] for k in ("xyz0", "xyz1", "cmpl0", "cmpl1", "radius", "rotation0", "rotation1", "scale") if k in s}
            r["trans"] = T
            for k in (0, 1):
                r[f"list_M{k}"] = multiway_registration(s[f"xyz{k}"], s[f"cmpl{k}"], s[f"pos{k}"], s[f"pos_cmpl{k}"], Vc, 1)
            raw_samples.append(r)
        want = CO.collate([CO.build_sample(r, centroids_of(r), voxel) for r in raw_samples])
        assert not same(batch, want) and want["placeholder_pairs"] == [] and len(want["correspondences"]) > 200
        for T, s in zip(trans, samples):                     # the poses are poses: the pair's motion, not the identity
            assert np.abs(T - np.eye(4)).max() > 0.05
        torch.manual_seed(3)
        model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV)
        host = []
        for b in range(2):
            n0 = sum(x[0] for x in want["len_batch"][:b])
            n1 = sum(x[1] for x in want["len_batch"][:b])
            m0 = sum(want["len_matches"][:b])
            sl = lambda k, a: want[f"sinput{k}_C"][a:a + want["len_batch"][b][k]]
            d = {"pcd0": [torch.from_numpy(want["pcd0"][b])], "pcd1": [torch.from_numpy(want["pcd1"][b])],
                 "T_gt": torch.from_numpy(want["T_gt"][4 * b:4 * b + 4])}
            for k, a in ((0, n0), (1, n1)):
                C = sl(k, a).copy()
                C[:, 0] = 0
                d[f"sinput{k}_C"], d[f"sinput{k}_F"] = torch.from_numpy(C), torch.ones((len(C), 1))
            d["correspondences"] = torch.from_numpy(want["correspondences"][m0:m0 + want["len_matches"][b]] - np.array([[n0, n1]]))
            host.append(d)
        np.random.seed(3)
        m_got, t_got, d_got = V.validate_pairs(model, pair_dicts(batch), batch_pairs=2)
        np.random.seed(3)
        m_want, t_want, d_want = V.validate_pairs(model, host, batch_pairs=2)
    assert t_got.shape == (2, 6) and t_got.tobytes() == t_want.tobytes() and m_got == m_want and d_got == d_want
