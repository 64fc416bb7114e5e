"""Multiway registration on the GPU (gcl_amd/lib/multiway.py, csrc/multiway.hip, csrc/posegraph.h) against the numpy oracles
(tests/multiway_oracle.py, tests/icp_oracle.py).

Information matrix: the correspondence count is exact (tests/test_oracle_multiway.py proves that no candidate lies near the
radius), every element lies within n 2^-52 A of the oracle -- the reordering bound of an n-term fp64 sum, A being the oracle's
sum of the absolute terms.

Optimiser: tests/test_oracle_multiway.py proves that every decision of every scene has a relative margin above 1e-6, so
``kept``, both solve counts and ``status`` equal the oracle's exactly.  Poses and confidences lie within 64 s (at least
1e-12), s being the largest elementwise difference between the oracle in float64 and in longdouble: one sample of the scene's
sensitivity to fp64 rounding, times 64 because the device adds in another order.  s, the bound and the device's error are
printed (run with -s) and recorded in DESIGN.md "Multiway registration".
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_scene                                                       # noqa: E402
import multiway_oracle as O                                            # noqa: E402
import multiway_scenes as S                                            # noqa: E402
import test_oracle_multiway as C                                       # noqa: E402

from gcl_amd.lib import multiway                                       # noqa: E402

DEV = "cuda:0"
R_TOL, T_TOL = 1e-10, 1e-9             # the ICP's bounds (tests/test_gpu_icp.py)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- information matrix ------------------------------------------------------------------------------------------------------
def _info(src, tgt, T, distance=S.DISTANCE):
    return multiway.get_information_matrix_from_point_clouds(_t(src), _t(tgt), distance, T).cpu().numpy()


def _info_batch(pairs, distance=S.DISTANCE):
    """pairs: (src, tgt, T) -> [B, 6, 6]."""
    o0 = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])])
    o1 = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])])
    return multiway.information_matrix_batch(_t(np.concatenate([p[0] for p in pairs])), o0,
                                             _t(np.concatenate([p[1] for p in pairs])), o1, distance,
                                             np.stack([p[2] for p in pairs])).cpu().numpy()


@pytest.mark.parametrize("n0,n1", icp_scene.STEP_SIZES)
def test_information_matrix_is_the_oracles(n0, n1):
    src, tgt, G, _ = icp_scene.step_pair(n0, n1)
    want, A, n, _ = O.information(src, tgt, G, S.DISTANCE)
    got = _info(src, tgt, G)
    assert got[5, 5] == n and got[3, 3] == n and got[4, 4] == n
    err = np.abs(got - want)
    print(f"{n0} x {n1}: n = {n}, max |d info| / (n 2^-52 A) = {(err / np.maximum(n * 2.0 ** -52 * A, 1e-300)).max():.3f}")
    assert (err <= n * 2.0 ** -52 * A).all()
    assert (got == got.T).all()
    if (n0, n1) == (5000, 5000):
        assert n > 2500


def _GtG(q):
    x, y, z = (float(v) for v in q)
    G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
    return G.T @ G


def test_information_radius_is_inclusive_and_ties_go_to_the_lowest_row():
    o = np.zeros((1, 3), dtype=np.float32)
    at = np.array([[0.25, 0, 0]], dtype=np.float32)
    I = np.eye(4)
    assert (_info(o, at, I, 0.25) == _GtG(at[0])).all()
    assert (_info(o, at + np.float32(2.0 ** -20), I, 0.25) == 0).all()
    tie = np.array([[0.125, 0, 0], [-0.125, 0, 0], [0, 0.125, 0], [0, 0, -0.125]], dtype=np.float32)
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):      # the lowest ROW, whatever cell it lies in
        assert (_info(o, tie[order], I, 0.25) == _GtG(tie[order][0])).all()
    # the transformation moves the source: (1, 0, 0) + x lands on the target exactly
    move = np.eye(4)
    move[0, 3] = 1.0
    assert (_info(o, at + np.array([1, 0, 0], dtype=np.float32), move, 0.25) == _GtG([1.25, 0, 0])).all()


def test_information_of_empty_and_unmatched_pairs_is_zero_and_neighbours_are_untouched():
    src, tgt, G, _ = icp_scene.step_pair(257, 63)
    e = np.zeros((0, 3), dtype=np.float32)
    far = (tgt.astype(np.float64) + 50.0).astype(np.float32)
    alone = _info(src, tgt, G)
    out = _info_batch([(e, tgt, G), (src, tgt, G), (src, e, G), (src, far, G), (e, e, G), (src, tgt, G)])
    for b in (0, 2, 3, 4):
        assert (out[b] == 0).all() and not np.signbit(out[b]).any()      # all bits zero, no -0.0
    assert (out[1] == alone).all() and (out[5] == alone).all() and alone[5, 5] > 0


def test_information_is_bitwise_the_same_alone_first_last_and_twice():
    a = icp_scene.step_pair(1025, 255)
    others = [icp_scene.step_pair(n0, n1) for n0, n1 in ((3, 65), (257, 63), (255, 1025))]
    pairs = [(a[0], a[1], a[2])] + [(s, t, G) for s, t, G, _ in others] + [(a[0], a[1], a[2])]
    alone = _info(a[0], a[1], a[2])
    one, two = _info_batch(pairs), _info_batch(pairs)
    assert (one[0] == alone).all() and (one[4] == alone).all() and (one == two).all()
    assert alone[5, 5] > 100


# ---- optimiser ----------------------------------------------------------------------------------------------------------------
def _optimize(graphs, **kw):
    """graphs: oracle-style dicts -> per graph (poses, confidence, kept, stats, status) as numpy."""
    n_off = np.concatenate([[0], np.cumsum([len(g["nodes"]) for g in graphs])])
    e_off = np.concatenate([[0], np.cumsum([len(g["edges"]) for g in graphs])])
    cat = lambda k, shape: np.concatenate([np.asarray(g[k], dtype=np.float64).reshape(shape) for g in graphs])
    edges = np.concatenate([np.asarray(g["edges"]).reshape(-1, 2) for g in graphs])
    r = multiway.global_optimization_batch(_t(cat("nodes", (-1, 4, 4))), edges, _t(cat("T", (-1, 4, 4))), _t(cat("info", (-1, 6, 6))),
                                           np.concatenate([np.asarray(g["uncertain"]) for g in graphs]), n_off, e_off,
                                           max_correspondence_distance=S.DISTANCE, **kw)
    poses, conf, kept, stats, status = (x.cpu().numpy() for x in (r.poses, r.confidence, r.kept, r.stats, r.status))
    return [(poses[n_off[g]:n_off[g + 1]], conf[e_off[g]:e_off[g + 1]], kept[e_off[g]:e_off[g + 1]], stats[g], int(status[g]))
            for g in range(len(graphs))]


def _same(a, b):
    return all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _check(got, want, s, bound, cbound, what):
    poses, conf, kept, stats, status = got
    err, cerr = np.abs(poses - want["poses"]).max(), np.abs(conf - want["confidence"]).max()
    print(f"{what}: s = {s:.3e}, bound = {bound:.3e}, |d pose| = {err:.3e}, |d confidence| = {cerr:.3e} (bound {cbound:.3e}), "
          f"solves = {tuple(stats[:2])}")
    assert status == want["status"] == 0
    assert (kept == want["kept"]).all()
    assert (stats[0], stats[1]) == want["solves"]
    assert np.isfinite(poses).all() and np.isfinite(conf).all() and np.isfinite(stats).all()
    assert err <= bound and cerr <= cbound


@pytest.mark.parametrize("n,variant", S.names())
def test_optimiser_is_the_oracles(n, variant):
    want = C.oracle(n, variant)
    s, bound, cbound = C.pose_bound(n, variant)
    _check(_optimize([S.graph(n, variant)])[0], want, s, bound, cbound, f"{n}/{variant}")


def test_optimiser_is_bitwise_the_same_alone_anywhere_in_a_batch_and_twice():
    graphs = [S.graph(n, v) for n, v in S.names()]
    one, two = _optimize(graphs), _optimize(graphs)
    assert all(_same(a, b) for a, b in zip(one, two))
    for i in (0, 4, 8, len(graphs) - 1):                              # 2, 3, 6 and 8 nodes; first and last
        assert _same(_optimize([graphs[i]])[0], one[i])
    back = _optimize(graphs[::-1])[::-1]
    assert all(_same(a, b) for a, b in zip(one, back))


def test_degenerate_graphs_report_their_status_and_leave_the_neighbours_alone():
    a, b = S.graph(6, "outlier"), S.graph(4, "noisy")
    none = dict(S.graph(4, "noisy"))
    none["info"] = np.zeros_like(none["info"])                        # no edge carries a correspondence
    nan = dict(S.graph(3, "noisy"))
    T = nan["T"].copy()
    T[1, 0, 3] = np.nan
    nan["T"] = T
    out = _optimize([none, a, nan, b])
    assert [r[4] for r in out] == [1, 0, 2, 0]
    for r, g in ((out[0], none), (out[2], nan)):
        assert (r[0] == g["nodes"]).all() and r[2].all() and (r[1] == 1).all() and (r[3] == 0).all()
    assert _same(out[1], _optimize([a])[0]) and _same(out[3], _optimize([b])[0])
    assert O.global_optimization(none, S.DISTANCE)["status"] == 1 and O.global_optimization(nan, S.DISTANCE)["status"] == 2


def test_a_wrong_structure_is_a_value_error_and_nothing_is_launched(monkeypatch):
    from gcl_amd import _lib
    launched = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: launched.append(1))
    g = S.graph(3, "noisy")
    for edges in ([(0, 2), (0, 2), (1, 2)], [(0, 1), (2, 0), (1, 2)], [(0, 1), (0, 3), (1, 2)]):
        bad = dict(g, edges=edges)
        with pytest.raises(ValueError):
            _optimize([bad])
    with pytest.raises(ValueError):
        multiway.full_registration_batch([{"clouds": [_t(np.zeros((4, 3), dtype=np.float32))] * 9,
                                           "init": np.tile(np.eye(4), (9, 9, 1, 1))}])
    assert not launched


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_full_registration_batch_is_the_oracle_chain_stage_by_stage():
    """Every stage is compared in its own bound on the DEVICE's input of that stage: the ICPs with the numpy ICP in the ICP's
    bounds, the information matrices with the oracle under the device's transformations, the composed nodes with numpy, the
    optimiser with the oracle on the device's graph."""
    sets = [S.cloud_set(seed, n) for seed, n in C.CHAIN]
    r = multiway.full_registration_batch([{"clouds": [_t(c) for c in clouds], "init": init} for clouds, _, init in sets])
    T = r.icp.transformation.cpu().numpy()
    stats, status = r.icp.stats.cpu().numpy(), r.icp.status.cpu().numpy()
    info, nodes = r.information.cpu().numpy(), r.nodes.cpu().numpy()
    poses, conf, kept = r.poses.cpu().numpy(), r.confidence.cpu().numpy(), r.kept.cpu().numpy()
    ostats, ostatus = r.stats.cpu().numpy(), r.status.cpu().numpy()
    e = 0
    for g, ((clouds, truth, init), (seed, n)) in enumerate(zip(sets, C.CHAIN)):
        icps = C.chain_oracle(seed, n)[0]
        e0, k = e, 0
        for s in range(n):
            for t in range(s + 1, n):
                want = icps[k]
                scale = max(np.abs(clouds[s]).max(), np.abs(clouds[t]).max())
                assert status[e] == 0 and stats[e, 3] == want["updates"] and stats[e, 2] == want["n_corr"]
                assert np.abs(T[e][:3, :3] - want["T"][:3, :3]).max() <= R_TOL
                assert np.abs(T[e][:3, 3] - want["T"][:3, 3]).max() <= T_TOL * (1 + scale)
                winfo, A, cnt, rad = O.information(clouds[s], clouds[t], T[e], S.DISTANCE)
                assert rad > C.D2_MARGIN and info[e][5, 5] == cnt
                assert (np.abs(info[e] - winfo) <= cnt * 2.0 ** -52 * A).all()
                e, k = e + 1, k + 1
        graph = O.compose(T[e0:e], n)
        graph["info"] = info[e0:e]
        lo, hi = int(r.node_offsets[g]), int(r.node_offsets[g + 1])
        assert np.abs(nodes[lo:hi] - graph["nodes"]).max() <= 1e-13      # n - 1 products of rigid 4 x 4, |t| below 2
        graph["nodes"] = nodes[lo:hi]
        want = O.global_optimization(graph, S.DISTANCE)
        wide = O.global_optimization(graph, S.DISTANCE, dtype=np.longdouble)
        for kind, m in want["margins"].items():
            assert m > C.MARGIN, (kind, m)
        sp = float(np.abs(want["poses"].astype(np.longdouble) - wide["poses"]).max())
        sc = float(np.abs(want["confidence"].astype(np.longdouble) - wide["confidence"]).max())
        _check((poses[lo:hi], conf[e0:e], kept[e0:e], ostats[g], int(ostatus[g])), want, sp, max(64 * sp, 1e-12),
               max(64 * sc, 1e-12), f"chain {seed}/{n}")
        assert np.abs(poses[lo:hi] - truth).max() < 0.02


def test_multiway_registration_is_the_numpy_pipeline():
    """End to end the ICP's bounds lead: a pose is a confidence-weighted mean of chains of at most n - 1 = 2 edge
    transformations, each within (R_TOL, T_TOL (1 + scale)) of the oracle's, and inv(P_0) P_i composes two poses: 4 edge
    errors at the most, doubled for the first-order terms left out."""
    k = C.RAW_K
    raw, truth, pos, V = S.raw_set(C.RAW_SEED, 2 * k + 1)
    got = multiway.multiway_registration(raw[0], raw[1:], pos[0], list(pos[1:]), V, k)
    assert len(got) == 2 * k and all(M.shape == (4, 4) and M.dtype == np.float64 for M in got)
    scale = max(np.abs(x).max() for x in raw)
    want = []
    for icps, infos, rads, r in C.raw_oracle(C.RAW_SEED, k):
        want += [np.linalg.inv(r["poses"][0]) @ r["poses"][j] for j in range(1, k + 1)]
    for i, (M, W) in enumerate(zip(got, want)):
        eR, et = np.abs(M[:3, :3] - W[:3, :3]).max(), np.abs(M[:3, 3] - W[:3, 3]).max()
        print(f"multiway_registration/{i}: |dR| = {eR:.3e} (bound {8 * R_TOL:.0e}), |dt| = {et:.3e} "
              f"(bound {8 * T_TOL * (1 + scale):.3e})")
        assert eR <= 8 * R_TOL and et <= 8 * T_TOL * (1 + scale)
        rows = ([0] + list(range(1, k + 1)), [0] + list(range(k + 1, 2 * k + 1)))[i // k]
        assert np.abs(M - np.linalg.inv(truth[0]) @ truth[rows[1 + i % k]]).max() < 0.1
    two = multiway.multiway_registration([raw[0]] * 2, [raw[1:]] * 2, [pos[0]] * 2, [list(pos[1:])] * 2, V, k)
    assert len(two) == 2 and all((a == b).all() for s in two for a, b in zip(s, got))
