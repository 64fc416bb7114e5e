"""Point-to-point ICP on the GPU (gcl_amd/lib/icp.py, csrc/icp.hip) against the numpy oracle (tests/icp_oracle.py).

tests/test_oracle_icp.py proves on the CPU that the scenes used here have no near-ties (d2 margins above 1e-8 m^2, criterion
margins above 1e-9), so the correspondences and the iteration count must equal the oracle's EXACTLY although the device adds
its fp64 sums in another order.  The transformation: R within 1e-10 and t within 1e-9 (1 + max |coordinate|) -- the one-pass
centring H = sum p q^T - n mp mq^T loses about (|p| / sigma)^2 2^-53 relative, ~1e-14 for a 100 m cloud of 10 m spread, so
the bounds leave four orders.  The measured maxima are printed (run with -s) and recorded in DESIGN.md.

Measured on an MI355X: see DESIGN.md "ICP".
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle as O                                                 # noqa: E402
import icp_scene as S                                                  # noqa: E402
from test_oracle_icp import exact_case                                 # noqa: E402

from gcl_amd.lib import icp                                            # noqa: E402

DEV = "cuda:0"
R_TOL, T_TOL = 1e-10, 1e-9


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _full(name):
    src, tgt, G, init = S.make_pair(*S.FULL[name])
    for a in (src, tgt, init):
        a.setflags(write=False)
    return src, tgt, init


@functools.lru_cache(maxsize=None)
def _full_oracle(name, max_iteration):
    src, tgt, init = _full(name)
    return O.icp(src, tgt, S.RADIUS, init, max_iteration)


def _run(src, tgt, radius, init, max_iteration):
    r = icp.registration_icp_batch(_t(src), None, _t(tgt), None, radius, init, max_iteration, want_corr=True)
    return (r.transformation[0].cpu().numpy(), r.stats[0].cpu().numpy(), int(r.status[0]), r.corr.cpu().numpy())


def _close(T, want, scale, what):
    eR = np.abs(T[:3, :3] - want[:3, :3]).max()
    et = np.abs(T[:3, 3] - want[:3, 3]).max()
    print(f"{what}: |dR| = {eR:.3e} (bound {R_TOL:.0e}), |dt| = {et:.3e} (bound {T_TOL * (1 + scale):.3e})")
    assert eR <= R_TOL and et <= T_TOL * (1 + scale), (what, eR, et)
    assert (T[3] == want[3]).all()


# ---- one step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", S.STEP_SIZES)
def test_one_step_is_the_oracles(n0, n1):
    src, tgt, _, init = S.step_pair(n0, n1)
    want = O.icp(src, tgt, S.RADIUS, init, 0)
    T, stats, status, corr = _run(src, tgt, S.RADIUS, init, 0)
    assert (corr == want["corr"]).all()
    assert stats[2] == want["n_corr"] and stats[0] == want["fitness"] and stats[3] == 0
    assert abs(stats[1] - want["rmse"]) <= 1e-12 * want["rmse"]
    assert status == want["status"] and (T == init).all()
    if (n0, n1) == (5000, 5000):
        assert want["n_corr"] > 4000                                            # the workload's order, not an empty case


# ---- full runs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iteration", S.FULL_ITERATIONS)
@pytest.mark.parametrize("name", sorted(S.FULL))
def test_full_run_is_the_oracles(name, max_iteration):
    src, tgt, init = _full(name)
    want = _full_oracle(name, max_iteration)
    T, stats, status, corr = _run(src, tgt, S.RADIUS, init, max_iteration)
    assert status == 0 and want["status"] == 0
    assert stats[3] == want["updates"], (stats[3], want["updates"])
    if max_iteration == 5:
        assert want["updates"] == 5
    assert (corr == want["corr"]).all()
    assert stats[2] == want["n_corr"] and stats[0] == want["fitness"]
    scale = max(np.abs(src).max(), np.abs(tgt).max())
    _close(T, want["T"], scale, f"{name}/{max_iteration}")
    # the rmse follows T: a point moves by at most 3 (|dR| |x| + |dt|), and so does every distance and their rms
    assert abs(stats[1] - want["rmse"]) <= 3 * (R_TOL * scale + T_TOL * (1 + scale))


# ---- structure --------------------------------------------------------------------------------------------------------------
def _batch(pairs, radius, max_iteration):
    """pairs: (src, tgt, init).  Returns per pair (T, stats, status, corr)."""
    o0 = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])])
    o1 = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])])
    r = icp.registration_icp_batch(_t(np.concatenate([p[0] for p in pairs])), o0, _t(np.concatenate([p[1] for p in pairs])),
                                   o1, radius, np.stack([p[2] for p in pairs]), max_iteration, want_corr=True)
    T, stats, status, corr = (x.cpu().numpy() for x in (r.transformation, r.stats, r.status, r.corr))
    return [(T[b], stats[b], int(status[b]), corr[o0[b]:o0[b + 1]]) for b in range(len(pairs))]


def _same(a, b):
    return all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_a_pair_is_bitwise_the_same_alone_first_last_and_twice():
    A = _full("corner")
    others = [S.step_pair(n0, n1) for n0, n1 in ((3, 65), (257, 63), (1025, 255))]
    pairs = [A] + [(s, t, i) for s, t, _, i in others] + [A]
    alone = _run(A[0], A[1], S.RADIUS, A[2], 30)
    one = _batch(pairs, S.RADIUS, 30)
    two = _batch(pairs, S.RADIUS, 30)
    assert _same(alone, one[0]) and _same(alone, one[4])
    assert all(_same(x, y) for x, y in zip(one, two))
    want = _full_oracle("corner", 30)
    assert alone[1][3] == want["updates"] and (alone[3] == want["corr"]).all()


# ---- boundaries: exactly representable numbers ---------------------------------------------------------------------------------
def test_the_radius_is_inclusive_and_ties_go_to_the_lowest_row():
    o = np.zeros((1, 3), dtype=np.float32)
    at = np.array([[0.25, 0, 0]], dtype=np.float32)
    I = np.eye(4)
    T, stats, status, corr = _run(o, at, 0.25, I, 30)
    assert corr.tolist() == [0] and stats[2] == 1 and stats[1] == 0.25 and status == 2 and (T == I).all()
    T, stats, status, corr = _run(o, at + np.float32(2.0 ** -20), 0.25, I, 30)
    assert corr.tolist() == [-1] and stats[2] == 0 and status == 1 and (T == I).all()
    tie = np.array([[0.125, 0, 0], [-0.125, 0, 0], [0, 0.125, 0], [0, 0, -0.125]], dtype=np.float32)
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):      # the lowest ROW, whatever cell it lies in
        assert _run(o, tie[order], 0.25, I, 0)[3].tolist() == [0]


def test_negative_coordinates_cell_faces_and_empty_cells():
    rng = np.random.RandomState(5)
    g = np.arange(-2, 3) * 0.25
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    tgt = tgt[rng.permutation(len(tgt))]
    h = np.arange(-5, 6) * 0.125
    src = np.stack(np.meshgrid(h, h, h, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    src = np.concatenate([src, [[10.0, 10.0, 10.0], [-10.0, 0.0, 0.0]]]).astype(np.float32)   # their 27 cells are empty
    want = O.icp(src, tgt, 0.25, np.eye(4), 0)
    assert want["margins"]["gap"] == 0.0 and want["margins"]["radius"] == 0.0                  # ties and hits AT the radius
    T, stats, status, corr = _run(src, tgt, 0.25, np.eye(4), 0)
    assert (corr == want["corr"]).all() and corr[-1] == -1 and corr[-2] == -1
    assert stats[2] == want["n_corr"] and abs(stats[1] - want["rmse"]) <= 1e-12 * want["rmse"]


# ---- degenerate pairs ------------------------------------------------------------------------------------------------------
def test_degenerate_pairs_stop_with_their_status_and_leave_the_neighbours_alone():
    A = _full("corner_b")
    e = np.zeros((0, 3), dtype=np.float32)
    o = np.zeros((1, 3), dtype=np.float32)
    two = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    init = S.rigid([0, 0, 1], 0.01, [0.01, 0.0, 0.0])
    pairs = [(e, A[1], init), A, (A[0], e, init), (o, o + 5.0, init), (o, o, init), (two, two, init), A, (e, e, init)]
    out = _batch(pairs, S.RADIUS, 30)
    alone = _run(A[0], A[1], S.RADIUS, A[2], 30)
    assert [r[2] for r in out] == [1, 0, 1, 1, 2, 2, 0, 1]
    for b in (0, 2, 3, 4, 5, 7):
        T, stats, status, corr = out[b]
        assert (T == init).all() and stats[3] == 0 and (corr == (np.arange(len(corr)) if b in (4, 5) else -1)).all()
        assert stats[2] == {4: 1, 5: 2}.get(b, 0) and stats[0] == {4: 1.0, 5: 1.0}.get(b, 0.0)
    for r in out:
        assert np.isfinite(r[0]).all() and np.isfinite(r[1]).all()
    assert _same(alone, out[1]) and _same(alone, out[6])


# ---- the loaders' pose refinement and the benchmark's helper ---------------------------------------------------------------
def test_refine_pair_poses_is_the_numpy_pipeline():
    pairs, want = [], []
    for seed in S.RAW_SEEDS:
        xyz0, xyz1, M = S.raw_pair(seed)
        pairs.append({"xyz0": xyz0, "xyz1": xyz1, "M": M})
        a, b = xyz0[S.first_per_voxel(xyz0)], xyz1[S.first_per_voxel(xyz1)]
        r = O.icp(a, b, S.RADIUS, M, 200)
        want.append((M @ (r["T"] @ np.linalg.inv(M)), max(np.abs(a).max(), np.abs(b).max())))
    got = icp.refine_pair_poses(pairs)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (2, 4, 4)
    for b, (M2, scale) in enumerate(want):
        _close(got[b], M2, scale, f"refine_pair_poses/{S.RAW_SEEDS[b]}")
    one = icp.refine_pair_poses(pairs[1:])
    assert (one[0] == got[1]).all()


def test_exact_rigid_motion_is_recovered_on_the_device():
    src, tgt, G, init = exact_case()
    r = icp.registration_icp(_t(src), _t(tgt), S.RADIUS, init)
    assert int(r.status) == 0 and float(r.fitness) == 1.0
    assert np.abs(r.transformation.cpu().numpy() - G).max() < 1e-4
    cs = r.correspondence_set.cpu().numpy()
    assert cs.shape == (len(src), 2) and (cs[:, 0] == cs[:, 1]).all() and (cs[:, 0] == np.arange(len(src))).all()


def test_icp_refine_is_registration_icp_at_ten_centimetres():
    src, tgt, init = _full("corner")
    pred = torch.from_numpy(init.astype(np.float32))[None].to(DEV)
    out = icp.icp_refine(_t(src)[None], _t(tgt)[None], pred)
    assert out.shape == (1, 4, 4) and out.dtype == torch.float32 and out.device == pred.device
    r = icp.registration_icp(_t(src), _t(tgt), 0.10, pred[0])
    assert int(r.status) == 0 and float(r.stats[3]) >= 1
    assert torch.equal(out[0], r.transformation.float())
