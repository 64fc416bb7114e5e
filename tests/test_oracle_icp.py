"""ICP without a GPU: the numpy oracle (tests/icp_oracle.py) on a case with a known answer, the MARGINS of every scene the GPU
test uses (a condition on the inputs: no near-tie between two targets, no candidate near the radius, no convergence decision
near its threshold -- which makes "same correspondences, same iteration count" a fair demand of fp64 code whose sums run in
another order), the C ABI's tables, and the argument checks of gcl_amd/lib/icp.py and of the C entry."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle as O                                                 # noqa: E402
import icp_scene as S                                                  # noqa: E402

from gcl_amd import _lib                                               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D2_MARGIN, CRITERIA_MARGIN = 1e-8, 1e-9


def exact_case():
    """(source, target, G, init): the target is the exact motion G of the source (up to its float32 rounding), init is G
    off by 0.1 degrees and 0.05 m."""
    src, _, G, _ = S.make_pair(2, 1200)
    tgt = S.apply(G, src)
    delta = S.rigid([0.3, -0.5, 0.8], np.deg2rad(0.1), np.array([0.03, -0.02, 0.0346]))
    return src, tgt, G, delta @ G


def test_exact_rigid_motion_is_recovered():
    src, tgt, G, init = exact_case()
    assert abs(np.linalg.norm((init @ np.linalg.inv(G))[:3, 3]) - 0.05) < 5e-3
    r = O.icp(src, tgt, S.RADIUS, init, 30)
    assert r["status"] == 0 and r["fitness"] == 1.0
    # float32 rounding of the coordinates is ~1e-7 m here: 1e-4 is a loose sanity bound, not a precision claim
    assert np.abs(r["T"] - G).max() < 1e-4
    assert (r["corr"] == np.arange(len(src))).all()


def _check(m, what):
    assert m["gap"] > D2_MARGIN and m["radius"] > D2_MARGIN, (what, m)
    assert m["criteria"] > CRITERIA_MARGIN, (what, m)


@pytest.mark.parametrize("name", sorted(S.FULL))
def test_margins_of_the_full_runs(name):
    src, tgt, _, init = S.make_pair(*S.FULL[name])
    assert len(src) <= 2000 and len(tgt) <= 2000
    for it in S.FULL_ITERATIONS:
        r = O.icp(src, tgt, S.RADIUS, init, it)
        assert r["status"] == 0
        _check(r["margins"], (name, it))


def test_margins_of_the_one_step_cases():
    for n0, n1 in S.STEP_SIZES:
        src, tgt, _, init = S.step_pair(n0, n1)
        assert (len(src), len(tgt)) == (n0, n1)
        _check(O.icp(src, tgt, S.RADIUS, init, 0)["margins"], (n0, n1))


def test_margins_of_the_raw_pairs():
    for seed in S.RAW_SEEDS:
        xyz0, xyz1, M = S.raw_pair(seed)
        a, b = xyz0[S.first_per_voxel(xyz0)], xyz1[S.first_per_voxel(xyz1)]
        assert 15000 <= len(xyz0) and len(a) <= 2000 and len(b) <= 2000
        r = O.icp(a, b, S.RADIUS, M, 200)
        assert r["status"] == 0
        _check(r["margins"], seed)


def test_degenerate_inputs():
    one = np.zeros((1, 3), dtype=np.float32)
    assert O.icp(one[:0], one, 0.25)["status"] == 1 and O.icp(one, one[:0], 0.25)["status"] == 1
    assert O.icp(one, one + 1.0, 0.25)["status"] == 1
    r = O.icp(one, one, 0.25)
    assert r["status"] == 2 and r["updates"] == 0 and r["n_corr"] == 1
    # exactly at the radius: taken; 2^-20 beyond: not; two equidistant targets: the lowest row
    q = np.array([[0.25, 0, 0]], dtype=np.float32)
    assert O.icp(one, q, 0.25)["n_corr"] == 1 and O.icp(one, q + np.float32(2.0 ** -20), 0.25)["n_corr"] == 0
    assert O.icp(one, np.array([[0.125, 0, 0], [-0.125, 0, 0], [0, 0.125, 0]], dtype=np.float32), 0.25)["corr"][0] == 0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_tables_hold_the_icp_entries():
    assert "icp.hip" in _lib.SOURCES
    src = open(os.path.join(ROOT, "include", "gcl_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gcl_icp_scratch_bytes", "gcl_icp_register_batch"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name


def test_c_entry_validates_before_any_launch():
    lib = _lib.load()
    assert lib.gcl_icp_scratch_bytes(-1, 5, 1) == 0 and lib.gcl_icp_scratch_bytes(5, 5, 0) == 0
    assert lib.gcl_icp_scratch_bytes(0, 0, 1) > 0
    assert lib.gcl_icp_scratch_bytes(1000, 2000, 3) >= 16 * 2000 + 136 * (4 + 3)
    p8 = ctypes.c_void_p(8)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    call = lambda o0, o1, B=1, d=0.2, it=30, scratch=p8: lib.gcl_icp_register_batch(
        p8, o0, p8, p8, o1, p8, B, p8, p8, d, p8, it, 1e-6, 1e-6, scratch, p8, p8, p8, None, None)
    ok = i64(0, 10)
    for args, word in (((ok, ok, 0), b"n_pairs"), ((ok, ok, 1, 0.0), b"positive"), ((ok, ok, 1, float("nan")), b"positive"),
                       ((ok, ok, 1, float("inf")), b"positive"), ((ok, ok, 1, 0.2, -1), b"max_iteration"),
                       ((i64(1, 10), ok), b"offsets0_host"), ((ok, i64(0, 5, 3), 2), b"descends"), ((None, ok), b"null"),
                       ((ok, ok, 1, 0.2, 30, None), b"null")):
        assert call(*args) == -1 and word in lib.gcl_last_error(), (args, lib.gcl_last_error())


# ---- gcl_amd/lib/icp.py: every argument error is a ValueError raised before the GPU is required ---------------------------
def test_argument_errors_need_no_gpu():
    from gcl_amd.lib import icp
    x = torch.zeros((10, 3))
    for bad in (torch.zeros((10, 2)), torch.zeros(10), np.zeros((10, 3))):
        with pytest.raises(ValueError):
            icp.registration_icp(bad, x, 0.2)
        with pytest.raises(ValueError):
            icp.registration_icp(x, bad, 0.2)
    for d in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            icp.registration_icp(x, x, d)
    for it in (-1, 2.5):
        with pytest.raises(ValueError, match="max_iteration"):
            icp.registration_icp(x, x, 0.2, max_iteration=it)
    with pytest.raises(ValueError, match="relative"):
        icp.registration_icp(x, x, 0.2, relative_rmse=float("nan"))
    for init in (np.eye(3), torch.eye(3), np.zeros((2, 4, 4)), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError, match="init"):
            icp.registration_icp(x, x, 0.2, init)
    for off in ([1, 10], [0, 6, 5, 10], [0, 9], [0.0, 10.0], [10]):
        with pytest.raises(ValueError, match="offsets"):
            icp.registration_icp_batch(x, off, x, [0, 10], 0.2)
        with pytest.raises(ValueError, match="offsets"):
            icp.registration_icp_batch(x, [0, 10], x, off, 0.2)
    with pytest.raises(ValueError, match="sources"):
        icp.registration_icp_batch(x, [0, 5, 10], x, [0, 10], 0.2)
    with pytest.raises(ValueError):
        icp.icp_refine(x, x[None], torch.eye(4)[None])
    with pytest.raises(ValueError, match="pred_trans"):
        icp.icp_refine(x[None], x[None], torch.eye(4))
    pair = {"xyz0": np.zeros((5, 3), np.float32), "xyz1": np.zeros((5, 3), np.float32), "M": np.eye(4)}
    for pairs, kw in (([], {}), ([pair] * 33, {}), ([pair], {"icp_voxel_size": 0.0}), ([pair], {"max_distance": -0.2}),
                      ([pair], {"max_iteration": -1}), ([dict(pair, M=np.eye(3))], {}),
                      ([dict(pair, xyz0=np.zeros((5, 2), np.float32))], {}),
                      ([dict(pair, xyz0=np.zeros((0, 3), np.float32), xyz1=np.zeros((0, 3), np.float32))], {})):
        with pytest.raises(ValueError):
            icp.refine_pair_poses(pairs, **kw)
