"""The brute-force oracle of the pair matcher (tests/pair_matches_oracle.py) against scipy's KD-tree and against counts known
in closed form, and its restatement of ``collate_pair_fn`` against a golden captured from the reference's own function
(tests/golden/make_pair_collate_golden.py: lib/data_loaders.py imports under the stub modules the other generators use).
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_matches_oracle as MO      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_collate.npz")


@pytest.mark.parametrize("radius", MO.RADII_A)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scene_a_hit_sets_equal_scipy_ball_query(seed, radius):
    """scipy's ball query is inclusive and evaluates distances its own way; the sets can only differ for a pair whose distance
    lies at the radius, and the scenes have none within 1e-9 r of it (asserted), nor two equal distances in one row."""
    from scipy.spatial import cKDTree
    xyz0, xyz1, T = MO.scene_a(seed)
    I, J, D = MO.scene_a_hits(seed, radius)
    q = MO.transform(xyz0, T)
    p = xyz1.astype(np.float64)
    tree = cKDTree(p)
    near = tree.query_ball_point(q, radius * (1 + 1e-9))
    inside = tree.query_ball_point(q, radius * (1 - 1e-9))
    assert [sorted(a) for a in near] == [sorted(a) for a in inside], "a pair within 1e-9 r of the radius"
    rows = np.split(J, np.searchsorted(I, np.arange(1, len(xyz0))))
    assert [sorted(r.tolist()) for r in rows] == [sorted(a) for a in inside]
    same_row = I[1:] == I[:-1]
    assert (np.diff(D)[same_row] > 0).all(), "rows are ordered by distance, without ties"
    pairs, cnt = MO.cut(I, J, len(xyz0))
    assert len(pairs) == cnt.sum() >= 9000 and (cnt == 0).sum() >= 100
    for K in (1, 5):
        pk, ck = MO.cut(I, J, len(xyz0), K)
        assert np.array_equal(ck, np.minimum(cnt, K))
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        want = np.concatenate([pairs[f:f + min(c, K)] for f, c in zip(first, cnt)])
        assert np.array_equal(pk, want)


@pytest.mark.parametrize("turned", [False, True])
def test_lattice_counts_strictness_and_ties(turned):
    xyz0, xyz1, T, interior = MO.lattice(turned)
    assert interior.sum() == 6 ** 3
    q = MO.transform(xyz0, T)
    for radius, want, d2max in ((2.0, 27, 3), (3.9, 251, 15)):
        I, J, D = MO.hits(xyz0, xyz1, T, radius)
        _, cnt = MO.cut(I, J, len(xyz0))
        assert (cnt[interior] == want).all() and cnt.max() == want and cnt.min() < want
        sums3 = {a * a + b * b + c * c for a in range(4) for b in range(4) for c in range(4)}
        assert set(np.unique(D).tolist()) == {s for s in sums3 if s <= d2max}, "integer d2; d2 = r r = 4 is excluded"
        e = xyz1.astype(np.float64)[J] - q[I]
        assert np.array_equal((e * e).sum(1), D)
        same_row = I[1:] == I[:-1]
        tie = same_row & (D[1:] == D[:-1])
        assert tie.sum() > 1000 and (np.diff(J)[tie] > 0).all(), "ties are ordered by target row"


def test_far_scene_has_one_point_per_voxel_and_hits():
    xyz0, xyz1, T, v = MO.scene_far()
    c = np.floor(xyz1 / np.float32(v)).astype(np.int64)
    assert len(np.unique(c, axis=0)) == len(c) and c.min() < -32700 and c.max() > 32700
    _, cnt = MO.matches(xyz0, xyz1, T, 3.9 * v)
    assert (cnt > 0).sum() > 1000 and cnt.max() > 50


def _golden_items(g):
    items = []
    for b in range(3):
        n0, n1 = len(g[f"coords0_{b}"]), len(g[f"coords1_{b}"])
        items.append((g[f"xyz0_{b}"], g[f"xyz1_{b}"], g[f"coords0_{b}"], g[f"coords1_{b}"], np.ones((n0, 1), np.float32),
                      np.ones((n1, 1), np.float32), g[f"matches_{b}"], g[f"trans_{b}"]))
    return items


def test_collate_restatement_equals_the_reference_golden():
    g = np.load(GOLDEN)
    assert len(g["matches_1"]) == 0 and len(g["matches_0"]) and len(g["matches_2"])
    out = MO.collate_pairs(_golden_items(g))
    for k, v in out.items():
        ref = g["out_" + k]
        if k == "correspondences":
            assert ref.dtype == np.int32 and v.dtype == np.int64        # the reference's .int() is not kept
            ref = ref.astype(np.int64)
        elif k == "len_batch":
            v = np.asarray(v)
        else:
            assert v.dtype == ref.dtype, k
        assert np.array_equal(v, ref), k
    assert out["len_batch"] == [[40, 50], [25, 35]] and out["T_gt"].shape == (8, 4)
    assert out["correspondences"][-1, 0] >= 40 + 30, "the start indices moved past the pair without matches"
