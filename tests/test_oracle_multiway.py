"""Multiway registration without a GPU: the numpy oracle (tests/multiway_oracle.py) on the seeded graphs
(tests/multiway_scenes.py), and the host build of csrc/posegraph.h against it.

The oracle reports the smallest relative margin of every decision it takes (each stop test, descent, pruning, the Euler
branch).  They are above 1e-6 on every scene, six orders above what fp64 rounding moves the compared quantities by, so
another summation order -- the device's -- takes the same decisions: kept edges and solve counts are compared exactly.

Poses are compared within 64 s (at least 1e-12), s being the largest elementwise difference between the oracle run in
float64 and in longdouble: one sample of the scene's sensitivity to fp64 rounding.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle                                                      # noqa: E402
import icp_scene                                                       # noqa: E402
import multiway_oracle as O                                            # noqa: E402
import multiway_scenes as S                                            # noqa: E402

from gcl_amd import _lib                                               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6
# m^2 between a squared distance and what it is compared with, in the chain scenes: d2 of coordinates below 10 m is rounded
# by about 1e-14, and the device's ICP pose is within 1e-10 of the oracle's (tests/test_gpu_icp.py), which moves a d2 below
# 0.04 m^2 by less than 1e-10
D2_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def oracle(n, variant, dtype="float64"):
    return O.global_optimization(S.graph(n, variant), S.DISTANCE, dtype=getattr(np, dtype))


def pose_bound(n, variant):
    """(s, bound) of the scene: s = max |poses(float64) - poses(longdouble)|, bound = max(64 s, 1e-12)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    a, b = oracle(n, variant), oracle(n, variant, "longdouble")
    assert a["status"] == 0 and b["status"] == 0
    assert (a["kept"] == b["kept"]).all() and a["solves"] == b["solves"]
    s = float(np.abs(a["poses"].astype(np.longdouble) - b["poses"]).max())
    sc = float(np.abs(a["confidence"].astype(np.longdouble) - b["confidence"]).max())
    return s, max(64 * s, 1e-12), max(64 * sc, 1e-12)


def flat(g):
    """The flat arrays of one graph as the C entries take them."""
    e = np.asarray(g["edges"], dtype=np.int32).reshape(-1, 2)
    return dict(n=len(g["nodes"]), m=len(e), src=np.ascontiguousarray(e[:, 0]), dst=np.ascontiguousarray(e[:, 1]),
                uncertain=np.asarray(g["uncertain"], dtype=np.int32),
                nodes=np.ascontiguousarray(g["nodes"], dtype=np.float64).reshape(-1, 16),
                T=np.ascontiguousarray(g["T"], dtype=np.float64).reshape(-1, 16),
                info=np.ascontiguousarray(g["info"], dtype=np.float64).reshape(-1, 36))


def params(distance=S.DISTANCE, prune=0.25, preference=1.0, reference=0):
    c = O.DEFAULT_CRITERIA
    return np.array([distance, prune, preference, reference, c["max_iteration"], c["min_relative_increment"],
                     c["min_relative_residual_increment"], c["min_right_term"], c["min_residual"], c["max_iteration_lm"],
                     c["upper_scale_factor"], c["lower_scale_factor"]], dtype=np.float64)


@pytest.mark.parametrize("n,variant", S.names())
def test_every_decision_has_a_margin(n, variant):
    r = oracle(n, variant)
    assert r["status"] == 0 and np.isfinite(r["poses"]).all()
    print(n, variant, r["solves"], {k: f"{v:.2e}" for k, v in r["margins"].items()})
    for kind, m in r["margins"].items():
        assert m > MARGIN, (kind, m)
    assert {"right_term", "sy"} <= set(r["margins"])
    if n > 2:          # two nodes chained from their one edge have nothing to move: the pass stops at its first test
        assert r["solves"][0] >= 1 and {"increment", "prune"} <= set(r["margins"])
    if n > 3 or (n == 3 and variant != "outlier"):       # 3 nodes without their one loop closure are a chain again
        assert "descent" in r["margins"]


@pytest.mark.parametrize("n", S.SIZES)
def test_consistent_graphs_come_back_to_their_ground_truth(n):
    g, r = S.graph(n, "consistent"), oracle(n, "consistent")
    assert np.abs(g["nodes"] - g["truth"]).max() > 1e-3            # they did start elsewhere
    assert np.abs(r["poses"] - g["truth"]).max() < 1e-6
    assert r["kept"].all() and (r["confidence"] > 0.99).all()


@pytest.mark.parametrize("n", S.SIZES[1:])
def test_the_rotated_loop_closure_and_only_it_is_dropped(n):
    g, r = S.graph(n, "outlier"), oracle(n, "outlier")
    want = np.ones(len(g["edges"]), dtype=np.int32)
    want[g["outlier"]] = 0
    assert g["uncertain"][g["outlier"]] and (r["kept"] == want).all()
    assert oracle(n, "noisy")["kept"].all()
    assert np.abs(r["poses"] - g["truth"]).max() < 0.05              # the graph without it is the noisy one


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pg") / "libpg_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", _lib.CSRC,
                    os.path.join(ROOT, "tests", "posegraph_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.pg_host.restype = None
    lib.pg_host.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 12
    return lib


def run_host(lib, g, p=None):
    f = flat(g)
    p = params() if p is None else p
    poses, conf = np.zeros((f["n"], 16)), np.zeros(f["m"])
    kept, stats, status = np.zeros(f["m"], dtype=np.int32), np.zeros(3), np.zeros(1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.pg_host(f["n"], f["m"], ptr(f["src"]), ptr(f["dst"]), ptr(f["uncertain"]), ptr(f["nodes"]), ptr(f["T"]),
                ptr(f["info"]), ptr(p), ptr(poses), ptr(conf), ptr(kept), ptr(stats), ptr(status))
    return poses.reshape(-1, 4, 4), conf, kept, stats, int(status[0])


@pytest.mark.parametrize("n,variant", S.names())
def test_the_host_build_of_the_header_is_the_oracle(host_lib, n, variant):
    want = oracle(n, variant)
    s, bound, cbound = pose_bound(n, variant)
    poses, conf, kept, stats, status = run_host(host_lib, S.graph(n, variant))
    err, cerr = np.abs(poses - want["poses"]).max(), np.abs(conf - want["confidence"]).max()
    print(f"{n}/{variant}: s = {s:.3e}, bound = {bound:.3e}, host |d pose| = {err:.3e}, |d conf| = {cerr:.3e}")
    assert status == 0 and (kept == want["kept"]).all()
    assert (stats[0], stats[1]) == want["solves"]
    assert err <= bound and cerr <= cbound
    assert abs(stats[2] - want["residual"]) <= 1e-6 * abs(want["residual"]) + 1e-18


def test_the_host_build_reports_no_correspondence_and_non_finite_inputs(host_lib):
    g = dict(S.graph(4, "noisy"))
    g["info"] = np.zeros_like(g["info"])
    poses, conf, kept, stats, status = run_host(host_lib, g)
    assert status == 1 and (poses == g["nodes"]).all() and kept.all() and (conf == 1).all()
    assert O.global_optimization(g, S.DISTANCE)["status"] == 1
    g = dict(S.graph(4, "noisy"))
    T = g["T"].copy()
    T[2, 1, 3] = np.nan
    g["T"] = T
    poses, conf, kept, stats, status = run_host(host_lib, g)
    assert status == 2 and (poses == g["nodes"]).all() and kept.all()
    assert O.global_optimization(g, S.DISTANCE)["status"] == 2


@pytest.mark.parametrize("n0,n1", [(1, 1), (3, 65), (257, 63), (1025, 255)])
def test_the_information_oracle_is_the_sum_of_GtG(n0, n1):
    src, tgt, G, _ = icp_scene.step_pair(n0, n1)
    info, A, n, rad = O.information(src, tgt, G, S.DISTANCE)
    want = O.information_direct(src, tgt, G, S.DISTANCE)
    assert info[5, 5] == n and (info == info.T).all() and (A >= np.abs(info)).all()
    assert (np.abs(info - want) <= max(n, 1) * 2.0 ** -52 * A).all()
    if n0 >= 257:
        assert n > n0 // 4                                            # a real case, not an empty one


def test_the_information_cases_have_a_radius_margin():
    """No candidate lies within 1e-8 m^2 of the radius: the device's count must be the oracle's."""
    for n0, n1 in icp_scene.STEP_SIZES:
        src, tgt, G, _ = icp_scene.step_pair(n0, n1)
        assert O.information(src, tgt, G, S.DISTANCE)[3] > 1e-8, (n0, n1)


# ---- the chain in numpy ------------------------------------------------------------------------------------------------
def pipeline_oracle(clouds, init):
    """ICP, information and optimiser of the oracles on downsampled clouds: (icps, infos, radius margins, result)."""
    n = len(clouds)
    icps, infos, rads = [], [], []
    for s in range(n):
        for t in range(s + 1, n):
            r = icp_oracle.icp(clouds[s], clouds[t], icp_scene.RADIUS, init[s, t], 200)
            info, _, _, rad = O.information(clouds[s], clouds[t], r["T"], S.DISTANCE)
            icps.append(r)
            infos.append(info)
            rads.append(rad)
    g = O.compose([r["T"] for r in icps], n)
    g["info"] = np.stack(infos)
    return icps, infos, rads, O.global_optimization(g, S.DISTANCE)


@functools.lru_cache(maxsize=None)
def chain_oracle(seed, n):
    clouds, _, init = S.cloud_set(seed, n)
    return pipeline_oracle(clouds, init)


@functools.lru_cache(maxsize=None)
def raw_oracle(seed, k):
    """The two sides of multiway_registration on S.raw_set(seed, 2 k + 1): clouds 0, 1 .. k and clouds 0, k + 1 .. 2 k."""
    raw, _, pos, V = S.raw_set(seed, 2 * k + 1)
    clouds = [x[icp_scene.first_per_voxel(x)] for x in raw]
    sides = []
    for rows in ([0] + list(range(1, k + 1)), [0] + list(range(k + 1, 2 * k + 1))):
        init = np.tile(np.eye(4), (k + 1, k + 1, 1, 1))
        for a in range(k + 1):
            for b in range(a + 1, k + 1):
                init[a, b] = S.reference_init(V, pos[rows[a]], pos[rows[b]])
        sides.append(pipeline_oracle([clouds[i] for i in rows], init))
    return sides


CHAIN = ((35, 3), (35, 4))       # seeds chosen for their margins, which the test below proves
RAW = (RAW_SEED, RAW_K) = (24, 2)


def _staged_margins(icps, infos, rads, r):
    for k, i in enumerate(icps):
        m = i["margins"]
        assert i["status"] == 0 and i["updates"] < 200 and i["fitness"] > 0.5
        assert m["gap"] > D2_MARGIN and m["radius"] > D2_MARGIN and m["criteria"] > 1e-9, (k, m)
        assert rads[k] > D2_MARGIN and infos[k][5, 5] > 100
    assert r["status"] == 0 and r["kept"].all()
    for kind, m in r["margins"].items():
        assert m > MARGIN, (kind, m)


@pytest.mark.parametrize("seed,n", CHAIN)
def test_the_chain_scenes_have_margins_at_every_stage(seed, n):
    icps, infos, rads, r = chain_oracle(seed, n)
    _staged_margins(icps, infos, rads, r)
    assert np.abs(r["poses"] - S.cloud_set(seed, n)[1]).max() < 0.02


def test_the_raw_scene_has_margins_at_every_stage():
    truth = S.raw_set(RAW_SEED, 2 * RAW_K + 1)[1]
    for side, rows in zip(raw_oracle(RAW_SEED, RAW_K), ([0, 1, 2], [0, 3, 4])):
        _staged_margins(*side)
        assert np.abs(side[3]["poses"] - truth[rows]).max() < 0.1          # 8 mm of noise, one point per 5 cm voxel


def test_the_entries_are_declared():
    assert "multiway.hip" in _lib.SOURCES and "multiway.hip" not in _lib.TRAINING_STEP_SOURCES
    header = open(_lib.HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gcl_info_scratch_bytes", "gcl_info_matrix_batch", "gcl_multiway_compose", "gcl_posegraph_optimize_batch"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", header), name
    from gcl_amd.lib import multiway
    for name in ("information_matrix_batch", "get_information_matrix_from_point_clouds", "global_optimization_batch",
                 "full_registration_batch", "multiway_registration"):
        assert callable(getattr(multiway, name))


def test_a_bad_structure_is_a_value_error_before_anything_is_launched():
    from gcl_amd.lib.multiway import check_structure
    ok = [(0, 1), (0, 2), (1, 2)]
    check_structure([3], [ok])
    for bad in ([(0, 2), (1, 2)], [(0, 1), (2, 1), (1, 2)], [(0, 1), (1, 2), (1, 3)], [(0, 1), (1, 1), (1, 2)]):
        with pytest.raises(ValueError):
            check_structure([3], [bad])
    with pytest.raises(ValueError):
        check_structure([9], [[(i, i + 1) for i in range(8)]])
    with pytest.raises(ValueError):
        check_structure([8], [[(i, i + 1) for i in range(7)] + [(0, 2)] * 22])
