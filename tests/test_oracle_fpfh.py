"""FPFH without a GPU: the numpy oracle (tests/fpfh_oracle.py) on cases that can be checked by hand, the argument checks of
gcl_amd/lib/fpfh.py, and the C-ABI entries' validation (which comes before any launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as O                                                # noqa: E402
import fpfh_scene as S                                                 # noqa: E402


def _plane(m=9, spacing=0.05):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 2) * spacing
    return np.concatenate([g, np.zeros((m * m, 1))], axis=1).astype(np.float32)


@pytest.mark.parametrize("above", [True, False])
def test_perfect_plane_normals_face_the_viewpoint_and_pairs_land_in_the_centre_bins(above):
    X = _plane()
    vp = np.array([0.2, 0.2, 1.0 if above else -1.0], dtype=np.float32)
    idx, cnt, _ = O.neighbours(X, 0.11, 30)
    assert cnt.min() >= 6                                              # a corner: itself, 2 at 0.05, 1 at 0.0707, 2 at 0.1
    nrm, gap, cosv = O.normals(X, idx, cnt, viewpoint=vp)
    want = np.array([0.0, 0.0, 1.0 if above else -1.0])
    assert np.abs(nrm - want).max() <= 1e-7
    sp, _ = O.spfh(X, nrm, idx, cnt)
    centre = np.zeros(33, dtype=np.float32)
    centre[[5, 16, 27]] = 100.0
    assert (sp == centre).all()
    f = O.fpfh(X, sp, idx, cnt)
    assert np.abs(f - 2 * centre).max() <= 1e-4


def test_pair_features_by_hand():
    # n2 tilted by theta towards the line p1 -> p2: |a1| = 0 < |a2| = sin(theta), the roles swap:
    # f3 = -sin(theta), v = y, w = (-cos, 0, sin), f2 = 0, f1 = atan2(sin, cos) = theta
    th = 0.3
    z = np.array([[0.0, 0.0, 1.0]])
    f1, f2, f3 = O.pair_features(np.zeros((1, 3)), z, np.array([[1.0, 0.0, 0.0]]), np.array([[np.sin(th), 0.0, np.cos(th)]]))
    assert abs(f1[0] - th) < 1e-15 and abs(f2[0]) < 1e-15 and abs(f3[0] + np.sin(th)) < 1e-15
    # coincident points, and a normal along the line (v = 0): zero features
    assert all(f[0] == 0.0 for f in O.pair_features(np.ones((1, 3)), z, np.ones((1, 3)), z))
    assert all(f[0] == 0.0 for f in O.pair_features(np.zeros((1, 3)), z, np.array([[0.0, 0.0, 2.0]]), z))
    # bin coordinates: the centre of the middle bin
    assert np.abs(O.bin_coordinates(np.zeros(1), np.zeros(1), np.zeros(1)) - 5.5).max() < 1e-14


def test_scene_rows_sum_to_600_and_the_stragglers_are_degenerate():
    X = S.scene(0)
    assert X.shape == (1636, 3) and X.dtype == np.float32
    idx1, cnt1, _ = O.neighbours(X, 0.10, 30)
    idx2, cnt2, ncand = O.neighbours(X, 0.25, 100)
    assert cnt1.min() == 1 and cnt1.max() == 30 and cnt2.max() == 100 and ncand.max() > 400
    assert 0.3 < (ncand > 100).mean() < 0.6                            # max_nn binds on a good share of the lists
    # every list starts with a point at d2 = 0 and ascends in (d2, row)
    d2 = O.dist2(X, X)
    for i in (0, 500, 1200, 1500, 1635):
        k = cnt2[i]
        key = [(d2[i, j], j) for j in idx2[i, :k]]
        assert key == sorted(key) and key[0][0] == 0.0 and (idx2[i, k:] == -1).all()
        r2 = np.float64(np.float32(0.25)) ** 2
        assert k == min(100, int((d2[i] <= r2).sum()))
    nrm, gap, cosv = O.normals(X, idx1, cnt1)
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert gap.min() >= 1e-3 and cosv.min() >= 1e-6                    # the oracle alone sets no point aside
    assert (np.einsum("ij,ij->i", nrm.astype(np.float64), -X.astype(np.float64))[cnt1 >= 3] >= 0).all()
    sp, edge = O.spfh(X, nrm, idx2, cnt2)
    assert edge.min() >= 1e-9
    f = O.fpfh(X, sp, idx2, cnt2)
    sums = f.astype(np.float64).sum(axis=1)
    regular = np.ones(len(X), dtype=bool)
    regular[-5:] = False
    assert np.abs(sums[regular] - 600).max() < 1e-3 and f.max() <= 200.0 + 1e-4 and f.min() >= 0
    # the isolated point: alone in its list, zero rows, the default normal
    iso = len(X) - 5
    assert cnt2[iso] == 1 and idx2[iso, 0] == iso and not sp[iso].any() and not f[iso].any()
    assert (nrm[iso] == (0, 0, 1)).all()
    # two points 0.01 apart: one pair each, a full row
    assert (cnt2[iso + 1:iso + 3] == 2).all() and np.abs(sums[iso + 1:iso + 3] - 600).max() < 1e-3
    # the exact duplicates: both lists are (lower row, higher row); d2 = 0 carries no weight, the row is the SPFH row
    a, b = len(X) - 2, len(X) - 1
    assert (X[a] == X[b]).all() and idx2[a, :3].tolist() == [a, b, -1] and idx2[b, :3].tolist() == [a, b, -1]
    assert (f[a] == sp[a]).all() and abs(sums[a] - 300) < 1e-3
    # the loaders' normalisation
    fn = O.fpfh(X, sp, idx2, cnt2, normalize=True)
    assert np.abs(np.linalg.norm(fn[regular].astype(np.float64), axis=1) - 1).max() < 1e-5 and not fn[iso].any()


def test_offsets_keep_clouds_apart_in_the_oracle():
    X = np.concatenate([S.scene(0)[:200], S.scene(0)[:150]])           # the second cloud lies inside the first
    idx, cnt, _ = O.neighbours(X, 0.1, 20, offsets=[0, 200, 350])
    one, c1, _ = O.neighbours(X[:200], 0.1, 20)
    two, c2, _ = O.neighbours(X[200:], 0.1, 20)
    assert (idx[:200] == one).all() and (idx[200:] == np.where(two >= 0, two + 200, -1)).all()
    assert (cnt == np.concatenate([c1, c2])).all()


def test_python_argument_checks():
    from gcl_amd.lib import fpfh as F
    xyz = torch.zeros((8, 3))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        F.radius_neighbours(torch.zeros((8, 4)), 0.1, 30)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        F.estimate_normals(torch.zeros(8), 0.1)
    for bad in (0, 129, -1, 2.5):
        with pytest.raises(ValueError, match="max_nn"):
            F.radius_neighbours(xyz, 0.1, bad)
    with pytest.raises(ValueError, match="max_nn"):
        F.compute_fpfh_feature(xyz, xyz, 0.1, max_nn=200)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radius"):
            F.radius_neighbours(xyz, bad, 30)
    for bad in ([0, 5, 3, 8], [1, 8], [0, 7], [0], [[0, 8]], [0.0, 8.0]):
        with pytest.raises(ValueError, match="offsets"):
            F.radius_neighbours(xyz, 0.1, 30, offsets=bad)
    with pytest.raises(ValueError, match="offsets"):
        F.fpfh_descriptors(xyz, 0.05, offsets=np.array([0, 9]))
    with pytest.raises(ValueError, match="normals"):
        F.compute_fpfh_feature(xyz, torch.zeros((7, 3)), 0.1)
    with pytest.raises(ValueError, match="normals"):
        F.compute_fpfh_feature(xyz, torch.zeros((8, 4)), 0.1)
    with pytest.raises(ValueError, match="viewpoint"):
        F.estimate_normals(xyz, 0.1, viewpoint=[0.0, 1.0])
    with pytest.raises(ValueError, match="viewpoint"):
        F.estimate_normals(xyz, 0.1, viewpoint=torch.zeros((3, 3)), offsets=[0, 4, 8])
    idx, cnt = torch.zeros((8, 30), dtype=torch.int32), torch.ones(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="idx"):
        F.normals_from_neighbours(xyz, idx.long(), cnt)
    with pytest.raises(ValueError, match="idx"):
        F.spfh_from_neighbours(xyz, xyz, idx[:7], cnt)
    with pytest.raises(ValueError, match="cnt"):
        F.spfh_from_neighbours(xyz, xyz, idx, cnt[:7])
    with pytest.raises(ValueError, match="spfh"):
        F.fpfh_from_spfh(xyz, torch.zeros((8, 32)), idx, cnt)
    if not torch.cuda.is_available():                                  # valid arguments: no CPU path
        with pytest.raises(RuntimeError, match="GPU"):
            F.fpfh_descriptors(xyz, 0.05, offsets=[0, 3, 8])


def test_c_abi_entries_validate_before_any_launch():
    from gcl_amd import _lib
    _lib.build()
    lib = _lib.load()
    p8, S_ = ctypes.c_void_p(8), None
    for name in ("gcl_fpfh_cell_keys", "gcl_fpfh_neighbours", "gcl_fpfh_normals", "gcl_fpfh_spfh", "gcl_fpfh_combine"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES

    def bad(rc, word):
        assert rc == -1 and word in lib.gcl_last_error(), (rc, lib.gcl_last_error())

    bad(lib.gcl_fpfh_cell_keys(None, 10, p8, 1, 0.1, p8, S_), b"null")
    bad(lib.gcl_fpfh_cell_keys(p8, 10, None, 1, 0.1, p8, S_), b"offsets")
    bad(lib.gcl_fpfh_cell_keys(p8, -1, p8, 1, 0.1, p8, S_), b"out of range")
    bad(lib.gcl_fpfh_cell_keys(p8, 2 ** 31, p8, 1, 0.1, p8, S_), b"out of range")
    bad(lib.gcl_fpfh_cell_keys(p8, 10, p8, 0, 0.1, p8, S_), b"n_clouds")
    bad(lib.gcl_fpfh_cell_keys(p8, 10, p8, 32768, 0.1, p8, S_), b"n_clouds")
    bad(lib.gcl_fpfh_cell_keys(p8, 10, p8, 1, 0.0, p8, S_), b"radius")
    assert lib.gcl_fpfh_cell_keys(None, 0, p8, 1, 0.1, None, S_) == 0          # nothing to do, nothing touched
    bad(lib.gcl_fpfh_neighbours(p8, 10, p8, 1, p8, p8, 0.1, 0, p8, p8, S_), b"max_nn")
    bad(lib.gcl_fpfh_neighbours(p8, 10, p8, 1, p8, p8, 0.1, 129, p8, p8, S_), b"max_nn")
    bad(lib.gcl_fpfh_neighbours(p8, 10, p8, 1, p8, p8, -0.1, 30, p8, p8, S_), b"radius")
    bad(lib.gcl_fpfh_neighbours(p8, 10, p8, 1, None, p8, 0.1, 30, p8, p8, S_), b"null")
    bad(lib.gcl_fpfh_neighbours(p8, 10, p8, 1, p8, p8, 0.1, 30, p8, None, S_), b"null")
    bad(lib.gcl_fpfh_normals(p8, 10, None, p8, 30, None, p8, 1, p8, S_), b"null")
    bad(lib.gcl_fpfh_normals(p8, 10, p8, p8, 30, None, None, 1, p8, S_), b"offsets")
    bad(lib.gcl_fpfh_normals(p8, 10, p8, p8, 200, None, p8, 1, p8, S_), b"max_nn")
    bad(lib.gcl_fpfh_spfh(p8, None, 10, p8, p8, 100, p8, S_), b"null")
    bad(lib.gcl_fpfh_spfh(p8, p8, 10, p8, p8, 0, p8, S_), b"max_nn")
    bad(lib.gcl_fpfh_spfh(p8, p8, -5, p8, p8, 100, p8, S_), b"out of range")
    bad(lib.gcl_fpfh_combine(p8, p8, 10, p8, p8, 100, 0, None, S_), b"null")
    bad(lib.gcl_fpfh_combine(p8, p8, 10, p8, p8, 100, 0, p8, S_), b"alias")
    bad(lib.gcl_fpfh_combine(p8, p8, 10, p8, p8, 1000, 0, ctypes.c_void_p(16), S_), b"max_nn")
    assert lib.gcl_fpfh_combine(None, None, 0, None, None, 100, 1, None, S_) == 0
