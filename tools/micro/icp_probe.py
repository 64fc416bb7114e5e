"""Time of the point-to-point ICP (csrc/icp.hip, gcl_amd/lib/icp.py) on one MI355X:

    python3 tools/micro/icp_probe.py [--out profiles/icp_probe.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/micro/icp_probe.py --trace-run      (kernel times, a run of its own)

The figures of the lanes-per-query variants that were tried (1, 16, 64; profiles/patches/icp_lanes_per_query_variants.patch puts
them back) stand at the end of profiles/icp_probe.txt; they were taken with this script's "forced" lines, once per variant.

Input: KITTI-sized synthetic pairs (two synthetic LiDAR scans of one scene 10 m apart, ~107 k raw points a scan), voxel 0.05,
radius 0.2, up to 200 iterations, the odometry pose off by 0.3 degrees and 0.1 m.  After one warm call of everything,
REPEATS windows between two device events per line, lines in turn; median [min .. max] in ms per call.

    set-up            gcl_fpfh_cell_keys + the sort of the keys (the sorted copy of the targets is the first launch of the ICP
                      call and is part of every "icp" line)
    icp 0 iterations  the whole call at max_iteration = 0: set-up launch, one step, one update
    icp N forced      the whole call at max_iteration = N with thresholds that never hold (every launch does its work);
                      "per iteration" = (N2 - N1 forced) / (N2 - N1): one step + one update
    icp 200           the call as the loaders make it (converges after `updates` updates; the launches behind that return at
                      once); "idle launch pair" = (icp 200 - icp forced at `updates`) / (200 - updates)
    refine B = 1 / 8  refine_pair_poses from the raw host scans: staging, the copy, voxelisation, ICP, the host read
    host path         the oracle's loop (tests/icp_oracle.py) with scipy's cKDTree as its neighbour search, host clock, on
                      the same machine, on the same voxelised pair

No gate; generated from seeds; not a test.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gcl_amd import _lib, synthetic                                                    # noqa: E402
from gcl_amd.lib import icp                                                            # noqa: E402
import icp_oracle                                                                      # noqa: E402
import icp_scene                                                                       # noqa: E402

DEV = torch.device("cuda:0")
REPEATS = 7
VOXEL, RADIUS, MAX_IT = 0.05, 0.2, 200
N1, N2 = 20, 60


def raw_pair(seed):
    scene = synthetic.make_scene(seed)
    T = np.eye(4)
    T[0, 3] = -10.0
    M = icp_scene.rigid([0.2, -0.1, 1.0], np.deg2rad(0.3), [0.06, -0.06, 0.05]) @ T
    return {"xyz0": synthetic.raycast(scene, np.array([0.0, 0.0, 0.0]), seed * 37),
            "xyz1": synthetic.raycast(scene, np.array([10.0, 0.0, 0.0]), seed * 37 + 1), "M": M}


def window(fn, calls=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


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
            return T, k
        T, prev, k = icp_oracle.umeyama(p[has], q[j[has]]) @ T, cur, k + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "icp_probe.txt"))
    ap.add_argument("--trace-run", action="store_true", help="one forced run, nothing timed: for a tracer")
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "icp_probe needs a GPU: a time taken anywhere else says nothing"
    _lib.require_gpu()
    raws = [raw_pair(50 + b) for b in range(1 if a.trace_run else 8)]
    with torch.cuda.device(DEV), torch.no_grad():
        r0 = raws[0]
        s0 = r0["xyz0"][icp_scene.first_per_voxel(r0["xyz0"])]
        s1 = r0["xyz1"][icp_scene.first_per_voxel(r0["xyz1"])]
        x0, x1 = torch.from_numpy(s0).to(DEV), torch.from_numpy(s1).to(DEV)
        M = r0["M"]
        run = lambda it, rf=1e-6, rr=1e-6: icp.registration_icp_batch(x0, None, x1, None, RADIUS, M, it, rf, rr)
        if a.trace_run:
            run(N1, -1.0, -1.0)
            torch.cuda.synchronize()
            return
        ref = run(MAX_IT)
        updates = int(ref.stats[0, 3])
        off1 = torch.tensor([0, len(x1)], dtype=torch.int64, device=DEV)
        keys = torch.empty(len(x1), dtype=torch.int64, device=DEV)
        lib = _lib.load()

        def setup():
            _lib.check(lib.gcl_fpfh_cell_keys(_lib.ptr(x1), len(x1), _lib.ptr(off1), 1, RADIUS, _lib.ptr(keys), _lib.stream()))
            torch.sort(keys)

        stages = [("set-up", 10, setup), ("icp 0 iterations", 10, lambda: run(0)),
                  (f"icp {N1} forced", 1, lambda: run(N1, -1.0, -1.0)), (f"icp {N2} forced", 1, lambda: run(N2, -1.0, -1.0)),
                  (f"icp {updates} forced", 1, lambda: run(updates, -1.0, -1.0)), (f"icp {MAX_IT}", 1, lambda: run(MAX_IT)),
                  ("refine B = 1", 1, lambda: icp.refine_pair_poses(raws[:1], VOXEL, RADIUS, MAX_IT)),
                  ("refine B = 8", 1, lambda: icp.refine_pair_poses(raws, VOXEL, RADIUS, MAX_IT))]
        for _, _, fn in stages:
            fn()
        torch.cuda.synchronize()
        times = {label: [] for label, _, _ in stages}
        for _ in range(REPEATS):
            for label, calls, fn in stages:
                times[label].append(window(fn, calls))
        med = lambda label: float(np.median(times[label]))
        out(f"Point-to-point ICP (csrc/icp.hip): the output of tools/micro/icp_probe.py on one {torch.cuda.get_device_name(0)}.")
        out(f"ms per call; {REPEATS} event-timed windows per line after a warm call, lines in turn; median [min .. max]")
        out()
        out(f"one pair: {len(r0['xyz0'])} + {len(r0['xyz1'])} raw points, {len(x0)} + {len(x1)} points at voxel {VOXEL}, radius "
            f"{RADIUS}; converged after {updates} updates, fitness {float(ref.stats[0, 0]):.4f}, "
            f"inlier rmse {float(ref.stats[0, 1]):.5f}")
        for label, _, _ in stages:
            t = times[label]
            out(f"  {label:<26} {med(label):9.3f} [{min(t):9.3f} .. {max(t):9.3f}]")
        out()
        out(f"  per iteration (step + update): {(med(f'icp {N2} forced') - med(f'icp {N1} forced')) / (N2 - N1):7.4f} ms")
        idle = (med(f"icp {MAX_IT}") - med(f"icp {updates} forced")) / max(MAX_IT - updates, 1)
        out(f"  idle launch pair after convergence: {idle * 1e3:7.2f} us ({MAX_IT - updates} of them: "
            f"{med(f'icp {MAX_IT}') - med(f'icp {updates} forced'):.3f} ms of the {med(f'icp {MAX_IT}'):.3f} ms call)")
    ht = []
    for _ in range(3):
        t0 = time.perf_counter()
        Th, kh = host_icp(s0, s1, RADIUS, M, MAX_IT)
        ht.append((time.perf_counter() - t0) * 1e3)
    out(f"  host path (numpy + scipy cKDTree, {kh} updates): {float(np.median(ht)):9.1f} [{min(ht):9.1f} .. {max(ht):9.1f}] ms; "
        f"|T - device T| = {np.abs(Th - ref.transformation[0].cpu().numpy()).max():.2e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
