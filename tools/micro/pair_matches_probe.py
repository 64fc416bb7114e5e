"""Time of the ground-truth correspondences of scan pairs (csrc/pairmatch.hip, gcl_amd/util/pointcloud.py,
gcl_amd/lib/pair_data_gpu.py) on one MI355X:

    python3 tools/micro/pair_matches_probe.py [--out profiles/pair_matches_probe.txt]

Cases: one KITTI-sized pair (two synthetic LiDAR scans of one scene 10 m apart, voxel 0.3, radius 0.45 = 1.5 voxels) and a batch
of 8 such pairs of different scenes.  Per case, after one warm call of everything: REPEATS windows between two device events
per stage, stages in turn; median [min .. max] in ms per call.

    count call     gcl_pair_matches_count: argument check kernel, count, scan, totals
    scan alone     gcl_exclusive_scan_i32 over the per-row counts (so count call - scan alone ~ the count kernel + two small ones)
    emit           gcl_pair_matches_emit
    matcher        get_matching_indices_batch with the table given: parameter upload, count, the host read, emit
    whole build    build_pair_batch_gpu from the raw host scans: staging, the copy, voxelisation, matches, the batch dict

For comparison, what the tree could do before: synthetic.pair_correspondences (scipy cKDTree on the host, on voxel CENTRES, per
pair) on the same voxelised clouds, host clock, on the same machine.  No gate; generated from seeds; not a test.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcl_amd import _lib, synthetic                                                    # noqa: E402
from gcl_amd.lib.pair_data_gpu import build_pair_batch_gpu                             # noqa: E402
from gcl_amd.util import pointcloud as PC                                              # noqa: E402

DEV = torch.device("cuda:0")
REPEATS = 9
VOXEL, RADIUS = 0.3, 0.45


def raw_pair(seed):
    scene = synthetic.make_scene(seed)
    T = np.eye(4)
    T[0, 3] = -10.0
    return {"xyz0": synthetic.raycast(scene, np.array([0.0, 0.0, 0.0]), seed * 37),
            "xyz1": synthetic.raycast(scene, np.array([10.0, 0.0, 0.0]), seed * 37 + 1), "trans": T, "radius": RADIUS}


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def case(name, raws, out):
    lib = _lib.require_gpu()
    B = len(raws)
    batch = build_pair_batch_gpu(raws, VOXEL, DEV)
    assert len(batch["len_batch"]) == B
    xyz0, xyz1 = batch["pcd0"], batch["pcd1"]
    o0 = np.concatenate([[0], np.cumsum([l[0] for l in batch["len_batch"]])])
    o1 = np.concatenate([[0], np.cumsum([l[1] for l in batch["len_batch"]])])
    trans, radii = [r["trans"] for r in raws], [r["radius"] for r in raws]
    table, cap = PC.target_table(xyz1, o1, VOXEL)
    host, lay = PC.pack_params(o0, o1, trans, radii)
    params = host.to(DEV)
    at = lambda n: ctypes.c_void_p(params.data_ptr() + 8 * lay[n][0])
    n0, n1, P = len(xyz0), len(xyz1), len(batch["correspondences"])
    cnt = torch.empty(n0, dtype=torch.int32, device=DEV)
    scratch = torch.empty(lib.gcl_pair_matches_scratch_len(n0), dtype=torch.int32, device=DEV)
    meta = torch.empty(2 + B, dtype=torch.int64, device=DEV)
    pairs = torch.empty((P, 2), dtype=torch.int64, device=DEV)
    common = (_lib.ptr(xyz0), n0, at("offsets0"), _lib.ptr(xyz1), n1, at("offsets1"), at("table_row0"), B, _lib.ptr(table), cap,
              0, 1, VOXEL, at("trans"), at("radii"), max(radii), 0)
    st = _lib.stream()
    stages = [
        ("count call", 10, lambda: _lib.check(lib.gcl_pair_matches_count(*common, _lib.ptr(cnt), _lib.ptr(scratch),
                                                                         _lib.ptr(meta), st))),
        ("scan alone", 10, lambda: _lib.check(lib.gcl_exclusive_scan_i32(_lib.ptr(cnt), n0, _lib.ptr(scratch),
                                                                         ctypes.c_void_p(scratch.data_ptr() + 4 * n0), st))),
        ("emit", 10, lambda: _lib.check(lib.gcl_pair_matches_emit(*common, 1, _lib.ptr(scratch), _lib.ptr(meta),
                                                                  _lib.ptr(pairs), P, st))),
        ("matcher", 3, lambda: PC.get_matching_indices_batch(xyz0, o0, xyz1, o1, trans, radii, VOXEL, table=(table, cap),
                                                             absolute=True)),
        ("whole build", 1, lambda: build_pair_batch_gpu(raws, VOXEL, DEV)),
    ]
    for _, _, fn in stages:
        fn()
    torch.cuda.synchronize()
    assert torch.equal(pairs, batch["correspondences"]) and int(meta[0]) == P
    times = [[] for _ in stages]
    for _ in range(REPEATS):
        for k, (_, calls, fn) in enumerate(stages):
            times[k].append(window(fn, calls))
    out()
    out(f"{name}: {B} pair(s), {sum(len(r['xyz0']) + len(r['xyz1']) for r in raws)} raw points, {n0} + {n1} voxels, "
        f"{P} correspondences ({P / max(n0, 1):.1f} per source row)")
    for (label, _, _), t in zip(stages, times):
        out(f"  {label:<14} {float(np.median(t)):9.3f} [{min(t):9.3f} .. {max(t):9.3f}]")
    # the host path the tree had: scipy on voxel centres, pair by pair
    C0, C1 = batch["sinput0_C"].cpu().numpy(), batch["sinput1_C"].cpu().numpy()
    ht = []
    for _ in range(3):
        t0 = time.perf_counter()
        for b in range(B):
            synthetic.pair_correspondences(C0[o0[b]:o0[b + 1], 1:], C1[o1[b]:o1[b + 1], 1:], trans[b], VOXEL, RADIUS / VOXEL)
        ht.append((time.perf_counter() - t0) * 1e3)
    out(f"  {'host scipy':<14} {float(np.median(ht)):9.3f} [{min(ht):9.3f} .. {max(ht):9.3f}]   "
        "(synthetic.pair_correspondences on the voxel centres; the matching alone, no voxelisation)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pair_matches_probe.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "pair_matches_probe needs a GPU: a time taken anywhere else says nothing"
    out(f"Pair correspondences (csrc/pairmatch.hip): the output of tools/micro/pair_matches_probe.py on one "
        f"{torch.cuda.get_device_name(0)}.")
    out(f"ms per call; {REPEATS} event-timed windows per stage after a warm call, stages in turn; median [min .. max]")
    with torch.cuda.device(DEV), torch.no_grad():
        raws = [raw_pair(50 + b) for b in range(8)]
        case("one pair", raws[:1], out)
        case("batch of 8", raws, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
