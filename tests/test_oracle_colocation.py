"""The co-location scenes and references without a GPU (tests/colocation_scenes.py): the vectorised numpy references of the
hits and the emit stage against oracle/colocation_oracle.py (a loop over the centre points) and, where no distance ties,
against the cKDTree builder of gcl_amd/synthetic.py; and the condition every scene of the case table exists for -- which R,
K, survivor word, tie, margin and launch shape it reaches -- as assertions: a scene that misses its condition is a broken
test, not a skipped one.  test_coverage_table prints the table (pytest -s)."""
import os
import sys

import numpy as np
import pytest

from oracle import colocation_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/colocation_scenes.py
import colocation_scenes as S                                          # noqa: E402

CASES = {c[0]: c for c in S.HITS_CASES}


def clouds(s, key):
    return [s[key][s["starts"][c]:s["starts"][c + 1]] for c in range(s["n_clouds"])]


def as_lists(emit):
    group, index, finest, _ = emit
    return group.tolist(), index.tolist(), [bool(f) for f in finest]


# ---------------------------------------------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_numpy_references_equal_the_loop_oracle(name):
    _, _, _, _, radius, K = CASES[name]
    s, (hits, cnt, rng), emit, _ = S.scene_of(name)
    own, cf = clouds(s, "xyz_own"), clouds(s, "xyz_cf")
    assert np.array_equal(own[0], cf[0])                                  # the centre cloud is its own centre frame
    want = O.colocation_groups(own[0], own[1:], s["list_M"], radius, K=K, nghb_cf=cf[1:])
    got = as_lists(emit)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == [bool(f) for f in want[2]]
    assert emit[3] == (len(want[0]), len(want[1]))
    # the hits stage's own invariants: counts, padding, the query itself first (distance 0) in the centre cloud
    assert ((hits >= 0).sum(2) == cnt).all() and (cnt <= K).all()
    assert np.array_equal(hits[:, 0, 0], np.arange(s["n_center"]))
    assert ((rng[:, 1:] == S.NO_RANGE) == (cnt[:, 1:] == 0)).all()


@pytest.mark.parametrize("name", S.KDTREE_CASES)
def test_numpy_references_equal_the_kdtree_builder(name):
    from gcl_amd.synthetic import colocation_groups
    _, kind, _, _, radius, K = CASES[name]
    s, _, emit, stats = S.scene_of(name)
    assert kind == "random" and not stats["tied"].any() and not stats["sphere"].any()
    own = clouds(s, "xyz_own")
    for c in range(1, s["n_clouds"]):                                      # the builder transforms the neighbours itself
        a, b = s["starts"][c], s["starts"][c + 1]
        assert np.array_equal((own[c] @ s["list_M"][c - 1][:3, :3].T + s["list_M"][c - 1][:3, 3]).astype(np.float32),
                              s["xyz_cf"][a:b])
    want = colocation_groups(own[0], own[1:], s["list_M"], radius, K=K)
    got = as_lists(emit)
    assert got[0] == list(want[0]) and got[1] == list(want[1]) and got[2] == [bool(f) for f in want[2]]


def _emit_loop(hits, cnt, first_rng):
    """k_colocation_sizes / k_colocation_emit as their comments state them, one centre row at a time."""
    group, index, finest = [], [], []
    n, n_clouds, K = hits.shape
    for i in range(n):
        if cnt[i, 1:].sum() == 0:
            continue
        best, bv = 0, first_rng[i, 0]
        for c in range(1, n_clouds):
            if cnt[i, c] > 0 and first_rng[i, c] < bv:
                best, bv = c, first_rng[i, c]
        members, fpos = [], 0
        for c in range(n_clouds):
            if c == best and c > 0:
                fpos = len(members)
            members += hits[i, c, :cnt[i, c]].tolist()
        group.append(len(members))
        index += members
        finest += [j == fpos for j in range(len(members))]
    return group, index, finest


@pytest.mark.parametrize("n_center,n_clouds,K", [(1, 1, 1), (1, 2, 5), (255, 7, 8), (257, 16, 1), (300, 2, 5), (300, 7, 5)])
def test_emit_reference_equals_the_loop(n_center, n_clouds, K):
    hits, cnt, rng = S.emit_inputs(n_center + n_clouds + K, n_center, n_clouds, K)
    got = S.emit_reference(hits, cnt, rng)
    want = _emit_loop(hits, cnt, rng)
    assert as_lists(got) == (want[0], want[1], want[2]) and got[3] == (len(want[0]), len(want[1]))
    if n_clouds == 1:
        assert got[3] == (0, 0)
    if n_center >= 255 and n_clouds >= 2:                                   # the inputs hold what they are for
        no_hit, no_nb = (cnt.sum(1) == 0).sum(), ((cnt[:, 1:].sum(1) == 0) & (cnt[:, 0] > 0)).sum()
        a, b = S.finest_ties(cnt, rng)
        assert no_hit >= 20 and no_nb >= 10 and a.sum() >= 10 and b.sum() >= (10 if n_clouds > 2 else 0)


# ---------------------------------------------------------------------------------------------------------------
# what the case table reaches
# ---------------------------------------------------------------------------------------------------------------
def test_coverage_table():
    rows, seen_RK = [], set()
    more, fewer, none = {1: 0, 5: 0, 8: 0}, {1: 0, 5: 0, 8: 0}, 0
    full_lane = 0
    for name, kind, args, voxel, radius, K in S.HITS_CASES:
        s, (hits, cnt, rng), emit, stats = S.scene_of(name)
        R = S.abi_R(radius, voxel)
        inside = stats["inside"]
        seen_RK.add((R, K))
        more[K] += int((inside > K).sum())
        fewer[K] += int(((inside >= 1) & (inside <= K - 1)).sum())
        none += int((inside == 0).sum())
        lane = 0
        if kind == "lattice" and K == 8 and R >= 3:
            lane = sum(int((S.busiest_lane(s, c, radius, R) >= 8).sum()) for c in range(s["n_clouds"]))
            full_lane += lane
        per_lane = -(-(2 * R + 1) ** 3 // S.LANES)
        rows.append((name, R, K, s["n_center"], s["n_clouds"], len(s["xyz_own"]), per_lane, (per_lane + 31) // 32,
                     int((inside > K).sum()), int(((inside >= 1) & (inside < K)).sum()), int((inside == 0).sum()),
                     int(stats["tied"].sum()), int(stats["sphere"].sum()), lane, emit[3][0], emit[3][1]))
    head = ("case", "R", "K", "n_center", "n_clouds", "rows", "cand/lane", "keep words", ">K", "1..K-1", "none", "tie@K",
            "d2==r2", "lane>=8", "groups", "entries")
    print("\n" + " | ".join(head))
    for r in rows:
        print(" | ".join(str(v) for v in r))
    print(f"pairs with more than K inside: {more}; with 1 .. K-1: {fewer}; with none: {none}; one lane >= 8 at K = 8, R >= 3: "
          f"{full_lane}")
    by = {r[0]: r for r in rows}
    # R: 1 .. 4, every survivor word; a radius that is a whole number of voxels; a radius the ABI must refuse
    assert {r[1] for r in rows} == {1, 2, 3, 4}
    assert {r[7] for r in rows} == {1, 2, 3}
    assert any(radius / voxel == round(radius / voxel) and radius / voxel >= 2 for _, _, _, voxel, radius, _ in S.HITS_CASES)
    assert S.abi_R(S.REFUSED[1], S.REFUSED[0]) == 5
    # K
    assert {(R, K) for R in (1, 4) for K in (1, 5, 8)} <= seen_RK
    assert all(more[K] >= 100 for K in (1, 5, 8)), more
    assert all(fewer[K] >= 100 for K in (5, 8)), fewer                    # (no count lies between 1 and K - 1 at K = 1)
    assert none >= 100
    assert full_lane >= 100
    # sizes
    assert {1, 31, 32, 33, 257} <= {r[3] for r in rows} and max(r[3] for r in rows) > 1000
    assert {1, 2, 3, 16} <= {r[4] for r in rows}
    assert max(s for s in np.diff(S.scene_of("random-R3-K8-1100rows")[0]["starts"])) <= 1500
    one = by["random-R2-K5-1cloud"]
    assert one[4] == 1 and (one[14], one[15]) == (0, 0)
    # the random scenes: a half cloud and, from four clouds on, a cloud without any hit
    s, (_, cnt, _), _, _ = S.scene_of("random-R2-K5-16clouds")
    assert (cnt[:, 15] == 0).all() and (cnt[:, 1:15].sum(0) > 0).all()
    s, (_, cnt, _), _, _ = S.scene_of("random-R4-K5")
    left = s["xyz_cf"][:s["n_center"], 0] < -1.5
    assert left.sum() >= 10 and (cnt[left, 1] == 0).all() and (cnt[left, 2] > 0).any()
    assert (s["xyz_cf"] < 0).any() and (s["coords"][:, 1:] < 0).any()


def test_lattice_ties_and_strict_radius():
    tie_k = on_sphere = centre_tie = nb_tie = 0
    for name, kind, args, voxel, radius, K in S.HITS_CASES:
        if kind != "lattice":
            continue
        s, (hits, cnt, rng), emit, stats = S.scene_of(name)
        tie_k += int(stats["tied"].any(1).sum())
        on_sphere += int(stats["sphere"].sum())
        a, b = S.finest_ties(cnt, rng)
        centre_tie += int(a.sum())
        nb_tie += int(b.sum())
        # rows are unrelated to position: the tie at the K-th place is not already resolved by ascending rows of a raster
        assert not np.array_equal(np.lexsort(s["coords"][:s["n_center"], ::-1].T), np.arange(s["n_center"])) or s["n_center"] < 3
        if a.any():                                                        # a tie with the centre leaves the flag at member 0
            group, _, finest, _ = emit
            kept = cnt[:, 1:].sum(1) > 0
            first = (np.cumsum(group) - group)[np.cumsum(kept)[a] - 1]
            assert (finest[first] == 1).all()
    print(f"\nlattice: queries tied at the K-th place {tie_k}, points at d2 == r2 {on_sphere}, centre/neighbour range ties "
          f"{centre_tie}, neighbour/neighbour ties below the centre {nb_tie}")
    assert tie_k >= 100 and on_sphere >= 100 and centre_tie >= 50 and nb_tie >= 50
    r = S.SQRT2_UP
    assert r * r > 0.125 and np.nextafter(r, 0) == 0.25 * np.sqrt(2.0)
    _, _, _, stats = S.scene_of("lattice-rsqrt2-K5")
    assert stats["inside"][:, 1:].max() == 19                              # 1 + 6 + 12 of a full neighbourhood


@pytest.mark.parametrize("name", ["corner-0", "corner-400", "corner-30000"])
def test_corner_hits_sit_where_the_box_test_decides(name):
    _, _, (_, offset), voxel, radius, K = CASES[name]
    s, (hits, cnt, rng), _, stats = S.scene_of(name)
    a, b = int(s["starts"][1]), int(s["starts"][2])
    d2, rows, n_in, _ = S.sorted_d2(s["xyz_cf"], a, b, 0, s["n_center"], radius)
    hit = np.zeros((s["n_center"], b - a), bool)
    np.put_along_axis(hit, rows - a, np.isfinite(d2), 1)
    box = S.box_distance(s, voxel)
    decisive = hit & (np.abs(box - radius / float(np.float32(voxel))) <= 1e-3)
    print(f"\n{name}: centre rows {s['n_center']}, true hits {int(hit.sum())}, with the box within 1e-3 voxels of the radius "
          f"{int(decisive.sum())}")
    assert hit.sum() >= 200 and decisive.sum() >= 100
    # the corner points are the low corners of their voxels, the coordinates are where the case says, all of them packable
    v = s["coords"][a:b, 1:]
    own = s["xyz_own"][a:b]
    vox = np.float32(voxel)
    assert (np.floor(own / vox) == v).all() and (np.floor(np.nextafter(own, np.float32(-np.inf)) / vox) == v - 1).all()
    assert np.abs(s["coords"][:, 1:] - offset).max() <= 32 and np.abs(s["coords"][:, 1:]).max() + 5 <= 32767


def test_mirror_pairs_tie_unfused_and_part_when_fused():
    """The mirrored pairs tie exactly in the reference; a kernel that contracted a product into the sum, either way round, would
    order the hits of these queries differently.  One such query is enough to fail a fused kernel; 20 of the 180 are asked for
    so that the case does not hang on one pair."""
    s, (hits, cnt, rng), _, stats = S.scene_of("mirror-R4-K8")
    q = s["xyz_cf"][:s["n_center"]]
    assert (q[:, 0] == q[:, 1]).all() and s["starts"][2] - s["starts"][1] == 750
    swaps = [S.mirror_swaps(s, hits, cnt, variant) for variant in (0, 1)]
    tied = int((stats["tied"][:, 1]).sum())
    print(f"\nmirror: queries whose hits change under contraction {swaps} of {s['n_center']}, tied at the K-th place {tied}")
    assert min(swaps) >= 20


def test_batch_samples_are_the_single_samples_shifted():
    b = S.batch_scene()
    assert len({smp["radius"] for smp in b["samples"]}) == 3 and len({smp["n_center"] for smp in b["samples"]}) == 3
    assert {S.abi_R(smp["radius"], b["voxel"]) for smp in b["samples"]} == {1, 2, 3}
    for si, smp in enumerate(b["samples"]):
        p, row0 = smp["part"], smp["row0"]
        n = len(p["xyz_own"])
        assert np.array_equal(b["xyz_own"][row0:row0 + n], p["xyz_own"]) and np.array_equal(b["xyz_cf"][row0:row0 + n], p["xyz_cf"])
        assert np.array_equal(b["coords"][row0:row0 + n, 0], p["coords"][:, 0]) and smp["starts"][0] == row0
        assert set(p["coords"][:, 0].tolist()) == {3 * si, 3 * si + 1, 3 * si + 2}
        alone = S.hits_reference(p["xyz_own"], p["xyz_cf"], p["starts"], p["n_center"], 0, smp["radius"], S.BATCH_K)
        in_batch = S.hits_reference(b["xyz_own"], b["xyz_cf"], smp["starts"], smp["n_center"], row0, smp["radius"], S.BATCH_K)
        assert np.array_equal(np.where(alone[0] >= 0, alone[0] + row0, -1), in_batch[0])
        assert np.array_equal(alone[1], in_batch[1]) and np.array_equal(alone[2], in_batch[2])
        assert (in_batch[1][:, 1:].sum(0) > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# key-less loaders
# ---------------------------------------------------------------------------------------------------------------
def test_voxel_inputs_hold_what_a_reciprocal_would_get_wrong():
    assert set(S.VOXELS) == {0.3, 0.025, 0.05, 1.0} and set(S.VOXEL_POINTS) == {1, 255, 257, 5000}
    for voxel in S.VOXELS:
        x = S.voxel_inputs(voxel, 5000)
        assert x.shape == (5000, 3) and x.dtype == np.float32
        wrong = int((np.floor(x * np.float32(1.0 / voxel)) != np.floor(x / np.float32(voxel))).sum())
        print(f"\nvoxel {voxel}: {wrong} inputs whose floor differs under multiplication by the reciprocal")
        assert wrong >= 100 or voxel == 1.0                                # (exact for a power of two)
        f = x.reshape(-1)
        assert (f == 0).sum() >= 2 and np.signbit(f[f == 0]).any() and ((f < 0) & (f > -1e-6)).sum() >= 3
        k = np.round(f.astype(np.float64) / float(np.float32(voxel)))
        on = (k * float(np.float32(voxel))).astype(np.float32)
        assert (f == on).sum() >= 1000 and (f == np.nextafter(on, np.float32(np.inf))).sum() >= 1000
        assert (f == np.nextafter(on, np.float32(-np.inf))).sum() >= 1000
        assert np.abs(S.voxel_reference(x, voxel)).max() < 1 << 20
    for p in S.VOXEL_POINTS:
        assert S.voxel_inputs(0.3, p).shape == (p, 3)
    for p in (255, 5000):
        for name, off in S.multi_offsets(p).items():
            sizes = np.diff(off)
            assert off[0] == 0 and off[-1] == p and (sizes >= 0).all() and len(off) <= 65, name
            if name.startswith("empty"):
                assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any() and (sizes > 0).sum() >= 3
            c = S.cloud_of_point(off, p)
            assert all(off[ci] <= i < off[ci + 1] for i, ci in enumerate(c.tolist()))


def test_loader_points_would_show_a_contraction():
    raw, index, coords, M = S.loader_points_scene()
    own, cf = S.loader_points_reference(raw, index, coords, M)
    assert set(coords[:, 0].tolist()) == {0, 1, 2} and (np.diff(coords[:, 0]) >= 0).all()
    for first in (0, 1):
        fused = S.loader_points_fused(raw, index, coords, M, first)
        differ = int((fused.view(np.uint32) != cf.view(np.uint32)).sum())
        print(f"\nloader points: {differ} of {cf.size} outputs differ when the products are contracted (first = {first})")
        assert differ >= 0.01 * cf.size
