"""The four callers of the rigid-fit solver (csrc/kabsch.h) on the GPU, on the degenerate scenes of tests/kabsch_scenes.py:
gcl_sc2_refine, gcl_sc2_seed_trans, gcl_ransac_register and gcl_icp_register_batch, each against fp64.

tests/test_oracle_kabsch.py proves on the CPU what is assumed here about every scene: its rank and gap, that every sample
of a rigid scene fits every row, the ICP pairs' margins, the seed case's compatibilities and inlier margin.

Tolerances (none is taken from the kernels; DESIGN.md "Rigid fit on degenerate sets" holds the measured values):
- packed fp32 poses (SC2, RANSAC): through the points, max_i |T p_i - T_ref p_i|, and |R - R_ref| where the pose is unique.
  The scale is the disagreement of the two references on the same set -- the repository's float32 torch oracle
  (oracle/sc2pcr_oracle.rigid_transform_3d) and the fp64 numpy fit -- floored at one float32 ulp of the largest coordinate
  (of 1 for R); the bound is 4 x that, against either reference.
- ICP (fp64 T): R_TOL = 1e-10 and T_TOL = 1e-9 (1 + scale) of tests/test_gpu_icp.py, plus the one-pass centring term
  K 2^-53 |c|^2 / (sigma2^2 + d sigma3^2) with K = K_ICP measured on the CPU (a row of dR meets |c|: 3 x the term for t).
The observed maxima are printed (run with -s).

Measured on an MI355X: see DESIGN.md "Rigid fit on degenerate sets".  Every bound keeps a factor of two over the device's
maximum except gcl_sc2_seed_trans on half_turn+far: 6.3e-5 m through the points against a bound of 1.22e-4 (1.93 x).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle as IO                                                # noqa: E402
import kabsch_scenes as KS                                             # noqa: E402
import test_oracle_kabsch as K                                         # noqa: E402

from gcl_amd import _lib                                               # noqa: E402
from gcl_amd.lib import icp                                            # noqa: E402
from gcl_amd.lib.ransac import ransac_correspondences                  # noqa: E402

DEV = "cuda:0"
CASES = KS.cases()
IDS = [KS.label(*c) for c in CASES]
R_TOL, T_TOL = 1e-10, 1e-9                                             # tests/test_gpu_icp.py


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_packed(what, T, refs, pts, coord_max, unique, seen):
    """T [3, 4] of the device against both references under the bound that their own disagreement sets."""
    T = np.asarray(T, dtype=np.float64)
    b_pts, b_rot = K.packed_bounds(refs[0], refs[1], pts, coord_max)
    e_pts = max(np.abs(K.move(T, pts) - K.move(r, pts)).max() for r in refs)
    e_rot = max(np.abs(T[:, :3] - r[:, :3]).max() for r in refs) if unique else 0.0
    seen["pts"] = max(seen.get("pts", 0.0), e_pts / b_pts)
    seen["rot"] = max(seen.get("rot", 0.0), e_rot / b_rot)
    print(f"{what}: through the points {e_pts:.3e} (bound {b_pts:.3e}), |dR| {e_rot:.3e} (bound {b_rot:.3e})"
          + ("" if unique else " [pose not unique: points only]"))
    assert np.isfinite(T).all(), what
    assert e_pts <= b_pts and e_rot <= b_rot, (what, e_pts, b_pts, e_rot, b_rot)
    R = T[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * 2.0 ** -23 and abs(np.linalg.det(R) - 1) <= 4 * 2.0 ** -23, what


# ---- gcl_sc2_refine -----------------------------------------------------------------------------------------------------------
def _refine(src, tgt, iterations):
    lib = _lib.require_gpu()
    with torch.cuda.device(DEV):
        s, t = _t(src), _t(tgt)
        T = torch.eye(4, dtype=torch.float32, device=DEV)[:3].contiguous().view(-1)
        part = torch.empty(lib.gcl_sc2_refine_partial_len(), dtype=torch.float64, device=DEV)
        state = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.gcl_sc2_refine(_lib.ptr(s), _lib.ptr(t), len(src), K.REFINE_THR, iterations, _lib.ptr(part),
                                      _lib.ptr(state), _lib.ptr(T), _lib.stream()), "gcl_sc2_refine")
        return T.cpu().numpy().reshape(3, 4), state.cpu().tolist()


@pytest.mark.parametrize("name,shifted", CASES, ids=IDS)
def test_refine_is_one_weighted_fit_of_the_set(name, shifted):
    seen = {}
    for n in K.REFINE_ROWS:
        src, tgt, _, _ = KS.corr_set(name, n, shifted)
        w = K.refine_weights(src, tgt)
        T64, s, d = K.weighted_fit64(src, tgt, w)
        T32 = K.torch_fit32(src, tgt, w)
        one, state1 = _refine(src, tgt, 1)
        many, state20 = _refine(src, tgt, 20)
        assert state1 == [0, n] and state20 == [1, n], (name, n, state1, state20)      # the second count repeats the first
        assert one.tobytes() == many.tobytes()
        _check_packed(f"refine {KS.label(name, shifted)} n={n}", one, (T32, T64), src, max(np.abs(src).max(), np.abs(tgt).max()),
                      K.is_unique(name, s, d), seen)
    print(f"refine {KS.label(name, shifted)}: largest error / bound: points {seen['pts']:.3f}, R {seen['rot']:.3f}")


# ---- gcl_sc2_seed_trans -----------------------------------------------------------------------------------------------------
def test_seed_trans_of_every_scene_in_one_call():
    c = K.seed_case()
    lib = _lib.require_gpu()
    S, n = len(CASES), len(c["src"])
    with torch.cuda.device(DEV):
        src, tgt, knn = _t(c["src"]), _t(c["tgt"]), _t(c["knn"])
        trans = torch.empty((S, 12), dtype=torch.float32, device=DEV)
        fitness = torch.empty(S, dtype=torch.float32, device=DEV)
        _lib.check(lib.gcl_sc2_seed_trans(_lib.ptr(src), _lib.ptr(tgt), n, _lib.ptr(knn), S, K.SEED["k1"], K.SEED["k2"],
                                          K.SEED["d_thre"], K.SEED["num_iterations"], K.SEED["inlier_thresh"],
                                          _lib.ptr(trans), _lib.ptr(fitness), _lib.stream()), "gcl_sc2_seed_trans")
        trans, fitness = trans.cpu().numpy().reshape(S, 3, 4), fitness.cpu().numpy()
    seen = {}
    k1, k2 = K.SEED["k1"], K.SEED["k2"]
    for i, (name, shifted) in enumerate(CASES):
        rows = slice(i * k1, i * k1 + k2)
        pts = c["src"][rows]
        _check_packed(f"seed_trans {KS.label(name, shifted)}", trans[i], (c["T32"][i], c["T64"][i]), pts,
                      max(np.abs(pts).max(), np.abs(c["tgt"][rows]).max()), K.is_unique(name, *c["sd"][i]), seen)
    print(f"seed_trans: largest error / bound: points {seen['pts']:.3f}, R {seen['rot']:.3f}; fitness {fitness.tolist()}")
    # The count runs over ALL rows of the call, and the sets overlap in space: a pose also fits a few rows of other sets (the
    # CPU test lists them).  Where the pose is unique that number is the oracle's, exactly (no distance within 1.5 mm of the
    # inlier distance).  On a line or in a point the turn about the line is arbitrary and so is the number of foreign rows:
    # there the count is checked against the device's OWN pose in fp64, rows within 8 float32 ulps of the largest coordinate
    # of the inlier distance counting either way, and it holds at least the set's 32 rows.
    for i, (name, shifted) in enumerate(CASES):
        if K.is_unique(name, *c["sd"][i]):
            assert fitness[i] == c["counts"][i], (name, shifted, fitness[i], c["counts"][i])
            continue
        d = np.linalg.norm(K.move(trans[i].astype(np.float64), c["src"]) - c["tgt"], axis=1)
        m = 8 * float(np.spacing(np.float32(max(np.abs(c["src"]).max(), np.abs(c["tgt"]).max()))))
        lo, hi = (d < K.SEED["inlier_thresh"] - m).sum(), (d < K.SEED["inlier_thresh"] + m).sum()
        assert max(lo, k1) <= fitness[i] <= hi, (name, shifted, fitness[i], lo, hi)
        assert (d[i * k1:(i + 1) * k1] < 0.1 * K.SEED["inlier_thresh"]).all()


# ---- gcl_ransac_register ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ransac_device(name, shifted, ransac_n):
    src, tgt, _, _ = KS.corr_set(name, K.RANSAC["n"], shifted)
    with torch.cuda.device(DEV):
        r = ransac_correspondences(_t(src), _t(tgt), K.RANSAC["max_corr_distance"], ransac_n, 0.0, 0.0,
                                   K.RANSAC["max_iteration"], 1.0, K.RANSAC["seed"], chunk=256, want_status=True)
        return (r.transformation.cpu().numpy().copy(), r.info.cpu().numpy().copy(), r.hyp_status.cpu().numpy().copy(),
                r.labels.cpu().numpy().copy())


@pytest.mark.parametrize("ransac_n", (3, 4))
@pytest.mark.parametrize("name,shifted", CASES, ids=IDS)
def test_ransac_poses_of_minimal_samples(name, shifted, ransac_n):
    n = K.RANSAC["n"]
    src, tgt, _, _ = KS.corr_set(name, n, shifted)
    ora = K.ransac_reference(name, shifted, ransac_n)
    T, info, status, labels = _ransac_device(name, shifted, ransac_n)
    assert ((status == -3) == (ora["status"] == -3)).all() and not (status == -4).any()
    assert info[2] == K.RANSAC["max_iteration"] and info[3] == (status >= 0).sum()
    assert (T[3] == np.array([0, 0, 0, 1], dtype=np.float32)).all() and np.isfinite(T).all()
    w = int(info[0])
    if name in KS.RIGID:
        must, thin = K.ransac_claim(name, ora)
        assert (status[must] == n).all(), (name, shifted, np.unique(status[must]))
        assert (status[thin] >= ransac_n).all(), (name, shifted, status[thin])
        assert info[1] == n and status[w] == n and (labels == 1).all()
    else:                                                       # mirrored: the table and the winner under the oracle's borderline rule
        ok = ~ora["borderline"]
        assert ok.mean() >= 0.9
        assert (status[ok] == ora["status"][ok]).all(), np.nonzero(status != ora["status"])[0][:10]
        best = ora["status"][ok].max()
        assert info[1] == best and ora["count"][w] == best
        assert ora["sse"][w] <= (1 + 1e-4) * np.nanmin(ora["sse"][ora["status"] == best])
    if name in ("generic", "planar", "planar_exact") or name in KS.SLABS or name == "mirrored":
        # the winner's pose against the fits of ITS sample (unit weights; rigid_transform_3d's 1e-6 belongs to the torch oracle)
        rows = ora["samples"][w]
        a, b = src[rows], tgt[rows]
        one = np.ones(len(rows), dtype=np.float32)
        T64, s, d = K.weighted_fit64(a, b, one, eps=0.0)
        seen = {}
        _check_packed(f"ransac {KS.label(name, shifted)} ransac_n={ransac_n} winner {w}", T[:3], (K.torch_fit32(a, b, one), T64),
                      src, max(np.abs(src).max(), np.abs(tgt).max()), K.is_unique(name, s, d), seen)


# ---- gcl_icp_register_batch ---------------------------------------------------------------------------------------------------
def _icp_batch(pairs, max_iteration):
    o0 = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])])
    o1 = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])])
    with torch.cuda.device(DEV):
        r = icp.registration_icp_batch(_t(np.concatenate([p[0] for p in pairs])), o0, _t(np.concatenate([p[1] for p in pairs])),
                                       o1, KS.ICP_RADIUS, np.stack([p[3] for p in pairs]), max_iteration, want_corr=True)
        T, stats, status, corr = (x.cpu().numpy() for x in (r.transformation, r.stats, r.status, r.corr))
    return [(T[b], stats[b], int(status[b]), corr[o0[b]:o0[b + 1]]) for b in range(len(pairs))]


@functools.lru_cache(maxsize=None)
def _icp_pairs():
    return [KS.icp_pair(name, shifted) for name, shifted in CASES]


@functools.lru_cache(maxsize=None)
def _icp_device(max_iteration):
    return _icp_batch(_icp_pairs(), max_iteration)


def _icp_tolerances(name, shifted, src, tgt):
    p, q, _ = K.icp_first_step(name, shifted)
    term = K.K_ICP * K.centring_units(p, q)
    scale = max(np.abs(src).max(), np.abs(tgt).max())
    return R_TOL + term, (T_TOL + 3 * term) * (1 + scale), scale


@pytest.mark.parametrize("max_iteration", (1, 30))
def test_icp_of_every_unique_scene_is_the_oracles(max_iteration):
    out = _icp_device(max_iteration)
    worst = [0.0, 0.0]
    for b, (name, shifted) in enumerate(CASES):
        if name not in KS.UNIQUE:
            continue
        src, tgt, G, init = _icp_pairs()[b]
        want = IO.icp(src, tgt, KS.ICP_RADIUS, init, max_iteration)
        T, stats, status, corr = out[b]
        assert status == 0 and want["status"] == 0
        assert stats[3] == want["updates"], (name, shifted, stats[3], want["updates"])
        assert (corr == want["corr"]).all() and stats[2] == want["n_corr"] and stats[0] == want["fitness"]
        r_tol, t_tol, scale = _icp_tolerances(name, shifted, src, tgt)
        eR, et = np.abs(T[:3, :3] - want["T"][:3, :3]).max(), np.abs(T[:3, 3] - want["T"][:3, 3]).max()
        print(f"icp {KS.label(name, shifted)}/{max_iteration}: |dR| = {eR:.3e} (bound {r_tol:.3e}), |dt| = {et:.3e} "
              f"(bound {t_tol:.3e}), {int(stats[3])} updates")
        worst = [max(worst[0], eR / r_tol), max(worst[1], et / t_tol)]
        assert eR <= r_tol and et <= t_tol, (name, shifted, eR, r_tol, et, t_tol)
        assert (T[3] == want["T"][3]).all()
        assert abs(stats[1] - want["rmse"]) <= 3 * (r_tol * scale + t_tol)
    print(f"icp/{max_iteration}: largest error / bound: R {worst[0]:.3f}, t {worst[1]:.3f}")


def test_icp_on_a_line_or_in_a_point_returns_a_rotation_that_fits():
    out = _icp_device(1)
    for b, (name, shifted) in enumerate(CASES):
        if name in KS.UNIQUE:
            continue
        src, tgt, G, init = _icp_pairs()[b]
        want = IO.icp(src, tgt, KS.ICP_RADIUS, init, 1)
        T, stats, status, corr = out[b]
        assert status == 0 and np.isfinite(T).all() and np.isfinite(stats).all() and stats[3] == 1
        assert len(src) >= 3 and stats[2] == len(src)
        R = T[:3, :3]
        ortho, det = np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1)
        assert ortho <= 1e-12 and det <= 1e-12, (name, shifted, ortho, det)
        assert (T[3] == np.array([0.0, 0.0, 0.0, 1.0])).all()
        # the rows matched BEFORE the update, under the new T: no worse than under the oracle's (equally arbitrary) rotation
        x, q = src.astype(np.float64), tgt.astype(np.float64)[want["steps"][0]["corr"]]
        rmse = lambda M: float(np.sqrt((np.linalg.norm(x @ M[:3, :3].T + M[:3, 3] - q, axis=1) ** 2).mean()))
        scale = max(np.abs(src).max(), np.abs(tgt).max())
        tol = 3 * (R_TOL * scale + T_TOL * (1 + scale))
        print(f"icp {KS.label(name, shifted)}: rmse of the matched rows {rmse(T):.3e} (oracle's T {rmse(want['T']):.3e}, "
              f"before {want['steps'][0]['rmse']:.3e}), tolerance {tol:.1e}; |R R^T - I| {ortho:.1e}")
        assert rmse(T) <= rmse(want["T"]) + tol


def test_a_full_rank_pair_next_to_degenerate_ones_is_bitwise_itself():
    for max_iteration in (1, 30):
        out = _icp_device(max_iteration)
        for name, shifted in (("generic", False), ("isotropic", False), ("generic", True), ("isotropic", True)):
            b = CASES.index((name, shifted))                   # isotropic follows coincident, generic+far follows half_turn
            alone = _icp_batch([_icp_pairs()[b]], max_iteration)[0]
            assert all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(alone, out[b])), (name, shifted)
