"""tests/complement_oracle.py and ``augment.draw_complement_pair`` against the reference's own functions, without a GPU:
tests/golden/complement_s0.npz holds what ``sample_random_trans`` and ``apply_transform`` of lib/complement_data_loader.py make
of one raw sample (tests/golden/make_complement_golden.py).  BLAS evaluates ``pts @ R.T`` in another order than the written-out
((x0 r0 + x1 r1) + x2 r2) + t, so coordinates are compared within a per-point fp64 bound (``complement_oracle.stage_bound``)
and crop decisions wherever the squared range is farther from the maximum than that bound implies.  The second half proves
that the scenes of tests/test_gpu_complement.py are what they claim to be."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as AO            # noqa: E402
import complement_oracle as CO         # noqa: E402
import complement_scenes as CS         # noqa: E402
from gcl_amd.lib import augment        # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "complement_s0.npz")
G = np.load(GOLDEN)


def _split(k):
    return np.split(G[f"cmpl{k}"], np.cumsum(G[f"cmpl{k}_sizes"])[:-1])


def _replay():
    """The fixture's draws through augment.draw_complement_pair: one generator, the three ranges in order."""
    randg = np.random.RandomState()
    randg.seed(int(G["seed"]))
    draws = [augment.draw_complement_pair(randg, random.Random(0), float(r), True, False, 0.8, 1.2) for r in G["ranges"]]
    return randg, draws


def test_draws_consume_the_generators_as_the_reference_does():
    randg, draws = _replay()
    assert len(draws) == 3
    for d, T in zip(draws, G["T"]):
        assert d["scale"] is None
        for k in (0, 1):          # T0's draws first, then T1's: two fp64 evaluations (Rodrigues / expm) of one matrix
            assert np.abs(d[f"rotation{k}"] - T[k][:3, :3]).max() <= 1e-12
            augment.checked_rotation(d[f"rotation{k}"])
    state = randg.get_state()
    assert np.array_equal(state[1], G["state_key"]) and state[2] == int(G["state_pos"])
    lo, hi = G["min_max_scale"]
    seen = set()
    for seed, want in enumerate(G["scales"]):
        a, b = random.Random(seed), np.random.RandomState(3)
        before = b.get_state()[2]
        d = augment.draw_complement_pair(b, a, np.pi / 4, False, True, float(lo), float(hi))
        assert d["rotation0"] is None and d["rotation1"] is None and b.get_state()[2] == before      # randg untouched
        assert (d["scale"] is None and np.isnan(want)) or d["scale"] == want
        ref = random.Random(seed)
        ref.random()
        if not np.isnan(want):
            ref.random()
        assert a.getstate() == ref.getstate()          # one draw, or two
        seen.add(d["scale"] is None)
    assert seen == {True, False}
    none = augment.draw_complement_pair(np.random.RandomState(1), random.Random(1), np.pi / 4, False, False, 0.8, 1.2)
    assert none == {"rotation0": None, "rotation1": None, "scale": None}


def test_chain_is_the_reference_s_within_the_float32_evaluation_bound():
    _, draws = _replay()
    n_points = sum(len(G[f"cmpl{k}"]) for k in (0, 1))
    assert 1500 <= n_points <= 5000 and os.path.getsize(GOLDEN) < 300e3
    inside_total = 0
    for k in (0, 1):
        cmpl, Ms = _split(k), G[f"list_M{k}"]
        xyz = G[f"xyz{k}"]
        s1 = np.concatenate(CO.moved_complements(cmpl, Ms))
        b1 = np.concatenate([CO.stage_bound(x, M) for x, M in zip(cmpl, Ms)])
        err = np.abs(s1.astype(np.float64) - G[f"stage1_{k}"])
        print(f"side {k} stage 1: max error {err.max():.3e}, bound up to {b1.max():.3e}, rows that differ {(err > 0).any(1).sum()}")
        assert (err <= b1).all()
        # without a rotation the crop reads stage 1 and the raw centre scan
        cat, keep = CO.crop(CO.moved_complements(cmpl, Ms), CO.range2(xyz).max())
        margin = CO.range_bound(cat, b1)
        far = np.abs(CO.range2_f64(cat) - CO.range2_f64(xyz).max()) > margin
        assert np.array_equal(keep[far], G[f"keep_plain_{k}"][far])
        inside_total += int((~far).sum())
        P = len(xyz)
        centroid = xyz.astype(np.float64).sum(axis=0) / P
        for i, d in enumerate(draws):
            T = AO.affine(d[f"rotation{k}"], centroid)
            # the reference's T: expm against Rodrigues (1e-12), and a float32 np.mean for the centroid -- recursive float32
            # summation of P terms is off by at most (P - 1) 2^-24 max|x| per component, carried through |R|
            dT = np.full((3, 4), 1e-12)
            dT[:, 3] = (P - 1) * 2.0 ** -24 * np.abs(xyz).max() * np.abs(T[:3, :3]).sum(axis=1) + 3e-12 * np.abs(centroid).max()
            assert (np.abs(T[:3] - G["T"][i][k][:3]) <= dT).all()
            centre = AO.apply_f32(xyz, T)
            bc = CO.stage_bound(xyz, T, None, dT)
            assert (np.abs(centre.astype(np.float64) - G[f"centre_{i}_{k}"]) <= bc).all()
            s2 = np.concatenate(CO.moved_complements(cmpl, Ms, T))
            b2 = CO.stage_bound(s1, T, b1, dT)
            err = np.abs(s2.astype(np.float64) - G[f"stage2_{i}_{k}"])
            print(f"side {k} range {float(G['ranges'][i]):.3f} stage 2: max error {err.max():.3e}, bound up to {b2.max():.3e}")
            assert (err <= b2).all()
            max_s = CO.range2(centre).max()
            e_max = CO.range_bound(centre, bc).max()
            assert abs(float(max_s) - float(G[f"max_{i}_{k}"])) <= e_max
            cat, keep = CO.crop(CO.moved_complements(cmpl, Ms, T), max_s)
            margin = CO.range_bound(cat, b2) + e_max
            far = np.abs(CO.range2_f64(cat) - CO.range2_f64(centre).max()) > margin
            assert np.array_equal(keep[far], G[f"keep_{i}_{k}"][far])
            assert 0 < keep.sum() < len(keep)              # the crop decides something on this scene
            inside_total += int((~far).sum())
    print("points inside the margin, over all chains:", inside_total)
    assert inside_total <= 0.01 * n_points


# ---- the scenes of tests/test_gpu_complement.py ------------------------------------------------------------------------------
def _item(s, **kw):
    return CO.build_sample(s, CS.host_centroids(s), CS.VOXEL, **kw)


def test_the_sizes_scene_covers_the_block_and_scan_chunk_sizes_and_contested_voxels():
    s = CS.scene("k3_both")[0]
    assert [len(x) for x in s["cmpl0"]] == [1, 255, 256, 257, 1025, 3000] and [len(x) for x in s["cmpl1"]] == [3000, 1025, 257, 256, 255, 1]
    assert sum(len(x) for k in (0, 1) for x in s[f"cmpl{k}"]) > 8192          # beyond the scan's single-workgroup form
    k1 = CS.scene("k1")[0]
    assert len(k1["cmpl0"]) == 2 and sum(len(x) for k in (0, 1) for x in k1[f"cmpl{k}"]) < 8192
    it = _item(s)
    for k in (0, 1):
        keep = it["kept"][k]
        assert 100 < keep.sum() < len(keep) - 100                              # the crop keeps and drops
        # two complement scans with points in one voxel: the first in concatenation order is the representative
        T = AO.affine(s[f"rotation{k}"], CS.host_centroids(s)[k])
        cat, _ = CO.crop(CO.moved_complements(s[f"cmpl{k}"], s[f"list_M{k}"], T), it["max"][k])
        scan = np.repeat(np.arange(6), [len(x) for x in s[f"cmpl{k}"]])[keep]
        pts, coords, sel = CO.voxelise(cat[keep], CS.VOXEL)
        _, inv = np.unique(AO.coords_f32(cat[keep], CS.VOXEL), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        scans_per_voxel = np.zeros((inv.max() + 1, 6), dtype=bool)
        scans_per_voxel[inv, scan] = True
        contested = scans_per_voxel.sum(axis=1) >= 2
        assert contested.sum() >= 100
        first_scan = np.full(inv.max() + 1, 9)
        np.minimum.at(first_scan, inv, scan)
        assert np.array_equal(scan[sel], first_scan[inv[sel]]) and np.array_equal(pts, it[f"pcd_nghb{k}"])


def test_the_arithmetic_scene_tells_two_float32_transforms_from_one_composed_fp64_transform():
    for name in ("k3_rotation", "k3_both"):
        s = CS.scene(name)[0]
        it = _item(s)
        changed = 0
        for k in (0, 1):
            T = AO.affine(s[f"rotation{k}"], CS.host_centroids(s)[k])
            cat, keep = CO.crop(CO.moved_complements(s[f"cmpl{k}"], s[f"list_M{k}"], T), it["max"][k])
            keep64, vox64 = CO.composed_f64(s[f"cmpl{k}"], s[f"list_M{k}"], T, it["max"][k], CS.VOXEL)
            vox = AO.coords_f32(cat, CS.VOXEL)
            changed += int(((keep != keep64) | (keep & (vox != vox64).any(axis=1))).sum())
        print(name, "points whose crop decision or voxel changes under one composed fp64 transform:", changed)
        assert changed >= 4


def test_the_boundary_scene_has_points_at_the_maximum_and_one_ulp_below():
    s, first, want = CS.boundary_sample()
    assert s.get("rotation0") is None and s["scale"] == 0.9
    it = _item(s)
    assert it["max"][0] == np.float32(4096.0)
    r2 = CO.range2(first)
    one_below = np.nextafter(np.float32(4096.0), np.float32(0.0))
    assert r2[0] == 4096.0 and r2[1] == 4096.0 and r2[2] == one_below and r2[3] < one_below and r2[4] > 4096.0
    assert np.array_equal(s["cmpl0"][0][:5], first) and np.array_equal(s["list_M0"][0], np.eye(4))
    assert it["kept"][0][:5].tolist() == want
    # the maximum is taken before the scale and the neighbourhood is not scaled: the kept points are the raw ones
    assert np.array_equal(it["pcd_nghb0"][0], first[2])
    scaled = _item(s, scale_neighbourhood=True)
    assert np.array_equal(scaled["pcd_nghb0"][0], first[2] * np.float32(0.9)) and np.array_equal(scaled["kept"][0], it["kept"][0])


def test_the_edge_scenes_are_what_they_claim():
    a = CS.scene("all_none")[0]
    it = _item(a)
    assert it["kept"][0].sum() == 0 and len(it["kept"][0]) == 500 and it["pcd_nghb0"].shape == (0, 3)
    assert it["kept"][1].all() and len(it["kept"][1]) > 1000
    e = CS.scene("edge")[0]
    assert [len(x) for x in e["cmpl0"]] == [300, 0, 257] and e["cmpl1"] == [] and e["list_M1"] == []
    it = _item(e)
    assert it["pcd_nghb1"].shape == (0, 3) and len(it["pcd_nghb0"]) > 100
    n = _item(CS.scene("no_match")[0])
    assert len(n["matches"]) == 0 and len(n["pcd0"]) >= 4 and len(n["pcd1"]) >= 4
    tiny = _item(CS.no_match_sample(3))
    assert len(tiny["matches"]) == 0 and len(tiny["pcd0"]) == 3
    with pytest.raises(ValueError, match="placeholder"):
        CO.collate([tiny])
    t = CS.scene("test_phase")
    assert all("cmpl0" not in s for s in t) and "pcd_nghb0" not in CO.collate([_item(s) for s in t])


def test_collate_places_placeholders_and_running_starts():
    items = [_item(s) for s in CS.scene("batch3")]
    b = CO.collate(items)
    assert b["placeholder_pairs"] == [1] and len(b["len_batch"]) == 3 and b["T_gt"].shape == (12, 4)
    n0, n1 = items[0]["coords0"].shape[0], items[0]["coords1"].shape[0]
    m0 = len(items[0]["matches"])
    assert np.array_equal(b["correspondences"][m0:m0 + 3], np.array([[1, 1], [2, 2], [3, 3]]) + [n0, n1])
    assert b["len_matches"] == [m0, 3, len(items[2]["matches"])]
    assert np.array_equal(np.unique(b["sinput0_C"][:, 0]), [0, 1, 2])
    left_out = CO.collate(items, placeholder_matches=False)
    assert left_out["placeholder_pairs"] == [] and len(left_out["len_batch"]) == 2 and left_out["T_gt"].shape == (8, 4)
    assert len(left_out["pcd_nghb0"]) == 2 and len(left_out["sinput0_C"]) == len(b["sinput0_C"])
    assert len(left_out["correspondences"]) == len(b["correspondences"]) - 3
