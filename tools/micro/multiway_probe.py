"""Time of multiway registration (csrc/multiway.hip, csrc/posegraph.h, gcl_amd/lib/multiway.py) on one MI355X:

    python3 tools/micro/multiway_probe.py [--out profiles/multiway_probe.txt]

Input: a KITTI-sized sample -- 7 synthetic LiDAR scans of one scene 2 m apart (~107 k raw points a scan), the centre scan
and num_complement_one_side = 3 scans a side, voxel 0.05, ICP at 0.2 m for up to 200 iterations, information matrices at
0.075 m, the odometry off by 0.3 degrees and 6 cm a scan: 12 pairs and 2 graphs of 4 nodes.

Every form runs in a child process of its own (`--stage NAME`): after one warm call, REPEATS windows between two device
events, median [min .. max] in ms per call.

    voxelise      voxelise_clouds of the 7 raw host scans: staging, the copy, the voxeliser, the host read of the counts
    icp x 12      registration_icp_batch of the 12 pairs in one call
    info x 12     information_matrix_batch of the 12 pairs: the grid at 0.075 m, its sort, three launches
    solve x 2     gcl_multiway_compose + gcl_posegraph_optimize_batch on the two graphs
    whole         multiway_registration from the raw host scans to the host poses
    host path     the oracles' pipeline (tests/icp_oracle.py, tests/multiway_oracle.py) with scipy's cKDTree as the neighbour
                  search, host clock, one run, on the same machine and the same voxelised clouds

No gate; generated from seeds; not a test.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gcl_amd import _lib, synthetic                                                    # noqa: E402
from gcl_amd.lib import icp, multiway                                                  # noqa: E402
import icp_oracle                                                                      # noqa: E402
import icp_scene                                                                       # noqa: E402
import multiway_oracle                                                                 # noqa: E402

DEV = torch.device("cuda:0")
REPEATS = 7
K, VOXEL, RADIUS, INFO_RADIUS, MAX_IT = 3, 0.05, 0.2, 0.075, 200
STAGES = ("voxelise", "icp x 12", "info x 12", "solve x 2", "whole", "host path")


def sample(seed=50):
    """(raw scans [centre, 3 left, 3 right], poses): V = I, so a pose moves its scan into the world."""
    scene = synthetic.make_scene(seed)
    xs = [0.0, -2.0, -4.0, -6.0, 2.0, 4.0, 6.0]
    rng = np.random.RandomState(seed)
    raw, pos = [], []
    for i, x in enumerate(xs):
        raw.append(synthetic.raycast(scene, np.array([x, 0.0, 0.0]), seed * 37 + i))
        P = np.eye(4)
        P[0, 3] = x
        if i:
            P = P @ icp_scene.rigid(rng.normal(size=3), np.deg2rad(0.3), 0.06 * rng.normal(size=3) / np.sqrt(3))
        pos.append(P)
    return raw, pos


def sides(items):
    return [items[:1] + items[1:1 + K], items[:1] + items[1 + K:]]


def inits(pos):
    out = []
    for side in sides(pos):
        init = np.tile(np.eye(4), (K + 1, K + 1, 1, 1))
        for s in range(K + 1):
            for t in range(s + 1, K + 1):
                init[s, t] = multiway._pair_init(np.eye(4), side[s], side[t])
        out.append(init)
    return out


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_icp(src, tgt, radius, init, max_iteration):
    """tests/icp_oracle.py's loop with a k-d tree in place of the brute-force search."""
    from scipy.spatial import cKDTree
    x, q = src.astype(np.float64), tgt.astype(np.float64)
    tree = cKDTree(q)
    T, prev, k = np.array(init, dtype=np.float64), None, 0
    while True:
        p = x @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(p, distance_upper_bound=radius)
        has = np.isfinite(d)
        n = int(has.sum())
        cur = (n / len(x), float(np.sqrt((d[has] ** 2).sum() / max(n, 1))))
        if n < 3 or (prev is not None and abs(cur[0] - prev[0]) < 1e-6 and abs(cur[1] - prev[1]) < 1e-6) or k >= max_iteration:
            return T, k, tree
        T, prev, k = icp_oracle.umeyama(p[has], q[j[has]]) @ T, cur, k + 1


def host_path(clouds, pos):
    out = []
    for side, init in zip(sides(clouds), inits(pos)):
        Ts, infos = [], []
        for s in range(K + 1):
            for t in range(s + 1, K + 1):
                T, _, tree = host_icp(side[s], side[t], RADIUS, init[s, t], MAX_IT)
                p = side[s].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                d, j = tree.query(p, distance_upper_bound=INFO_RADIUS)
                q = side[t].astype(np.float64)[j[np.isfinite(d)]]
                n, sq, S = float(len(q)), q.sum(axis=0), q.T @ q
                Ts.append(T)
                infos.append(multiway_oracle._assemble(n, sq, S))
        g = multiway_oracle.compose(Ts, K + 1)
        g["info"] = np.stack(infos)
        P = multiway_oracle.global_optimization(g, INFO_RADIUS)["poses"]
        out += [np.linalg.inv(P[0]) @ P[i] for i in range(1, K + 1)]
    return out


def stage(name):
    """One line: the stage's median [min .. max] and a note."""
    assert torch.cuda.is_available(), "multiway_probe needs a GPU: a time taken anywhere else says nothing"
    _lib.require_gpu()
    raw, pos = sample()
    with torch.cuda.device(DEV), torch.no_grad():
        xyz, starts = icp.voxelise_clouds(raw, VOXEL)
        clouds = [xyz[starts[i]:starts[i + 1]] for i in range(2 * K + 1)]
        graphs = [{"clouds": c, "init": i} for c, i in zip(sides(clouds), inits(pos))]
        note = ""
        if name == "host path":
            host = [c.cpu().numpy() for c in clouds]
            got = multiway.multiway_registration(raw[0], raw[1:], pos[0], pos[1:], np.eye(4), K, VOXEL)
            t0 = time.perf_counter()
            want = host_path(host, pos)
            t = [(time.perf_counter() - t0) * 1e3]
            note = f"one run; max |M - device M| = {max(np.abs(a - b).max() for a, b in zip(got, want)):.2e}"
        else:
            if name == "voxelise":
                fn = lambda: icp.voxelise_clouds(raw, VOXEL)
                note = f"{sum(len(r) for r in raw)} raw points, {int(starts[-1])} after the voxels"
            elif name == "whole":
                fn = lambda: multiway.multiway_registration(raw[0], raw[1:], pos[0], pos[1:], np.eye(4), K, VOXEL)
            else:
                src = [g["clouds"][s] for g in graphs for s in range(K + 1) for t in range(s + 1, K + 1)]
                tgt = [g["clouds"][t] for g in graphs for s in range(K + 1) for t in range(s + 1, K + 1)]
                init = np.stack([g["init"][s, t] for g in graphs for s in range(K + 1) for t in range(s + 1, K + 1)])
                off = lambda cs: np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
                x0, x1, o0, o1 = torch.cat(src), torch.cat(tgt), off(src), off(tgt)
                r = icp.registration_icp_batch(x0, o0, x1, o1, RADIUS, init, MAX_IT)
                full = multiway.full_registration_batch(graphs)
                if name == "icp x 12":
                    fn = lambda: icp.registration_icp_batch(x0, o0, x1, o1, RADIUS, init, MAX_IT)
                    note = f"{len(x0)} source rows; updates {r.stats[:, 3].int().tolist()}"
                elif name == "info x 12":
                    fn = lambda: multiway.information_matrix_batch(x0, o0, x1, o1, INFO_RADIUS, r.transformation)
                    note = f"correspondences {full.information[:, 5, 5].int().tolist()}"
                else:
                    lib = _lib.load()
                    G, tn, te = 2, 2 * (K + 1), 2 * (K + 1) * K // 2
                    offs = torch.tensor([0, K + 1, tn, 0, te // 2, te], dtype=torch.int32, device=DEV)
                    nodes = torch.empty((tn, 16), dtype=torch.float64, device=DEV)
                    edges = torch.empty((te, 2), dtype=torch.int32, device=DEV)
                    unc = torch.empty(te, dtype=torch.int32, device=DEV)
                    eT, info = r.transformation.reshape(te, 16), full.information.reshape(te, 36)
                    params = multiway._params(INFO_RADIUS, 0.25, 1.0, 0, None)

                    def fn():
                        _lib.check(lib.gcl_multiway_compose(_lib.ptr(offs[:3]), _lib.ptr(offs[3:]), G, tn, te, _lib.ptr(eT),
                                                            _lib.ptr(nodes), _lib.ptr(edges), _lib.ptr(unc), _lib.stream()))
                        multiway._optimize(nodes, offs[:3], edges, offs[3:], eT, info, unc, G, tn, te, params)
                    note = f"solves {full.stats[:, :2].int().tolist()}, kept {int(full.kept.sum())} of {te} edges"
            fn()
            torch.cuda.synchronize()
            t = [window(fn) for _ in range(REPEATS)]
    print(f"STAGE  {name:<12} {float(np.median(t)):10.3f} [{min(t):10.3f} .. {max(t):10.3f}]   {note}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "multiway_probe.txt"))
    ap.add_argument("--stage", choices=STAGES)
    a = ap.parse_args()
    if a.stage:
        stage(a.stage)
        return
    lines = [f"Multiway registration (csrc/multiway.hip, csrc/posegraph.h): the output of tools/micro/multiway_probe.py on one "
             f"{torch.cuda.get_device_name(0)}.",
             f"ms per call; one child process per line, {REPEATS} event-timed windows after a warm call; median [min .. max]",
             f"one sample: 7 scans, num_complement_one_side = {K}, voxel {VOXEL}, ICP at {RADIUS} m, information at {INFO_RADIUS} m",
             ""]
    for name in STAGES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", name], capture_output=True, text=True,
                           timeout=900)
        got = [l[7:] for l in p.stdout.splitlines() if l.startswith("STAGE  ")]
        if p.returncode != 0 or not got:
            raise RuntimeError(f"stage {name!r} failed (rc = {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        lines.append("  " + got[0])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
