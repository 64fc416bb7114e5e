"""Time per stage of the FPFH descriptors (gcl_amd/lib/fpfh.py, csrc/fpfh.hip) on one MI355X:

    python3 tools/micro/fpfh_probe.py [--out profiles/fpfh_probe.txt]

Clouds: box-surface clouds (synthetic.make_box_cloud) voxel-downsampled to 5 000, 20 000 and 100 000 points at voxel 0.05; one
synthetic LiDAR scan (synthetic.raycast) downsampled at voxel 0.3, and the same scan scaled by 1 / 6 at voxel 0.05 (the same
cells, other numbers); a batch of 8 x 5 000 through ``offsets``.  The recipe is ``fpfh_descriptors``': normals at (2 voxels, 30),
FPFH at (5 voxels, 100).

Stages are timed in turn in windows of CALLS calls between two device events, REPEATS windows each, after a warm-up of every
stage on every cloud; median, minimum and maximum of the windows are printed.  "neighbours" is the whole of
``radius_neighbours``: cell keys, torch.sort, the search.  For orientation only, one forward pass of the network (ResUNetBN2C,
32 channels, inference) on the same points as one-point-per-voxel input is timed in the same run (host clock around passes that
end in a synchronise).  No gate: nothing is compared against an earlier figure.  Everything is generated from seeds; not a test.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcl_amd import synthetic                                          # noqa: E402
from gcl_amd.lib import fpfh as F                                      # noqa: E402

DEV = torch.device("cuda:0")
CALLS, REPEATS = 10, 9


def downsample(xyz, voxel):
    c = np.floor(xyz / voxel).astype(np.int64)
    c -= c.min(axis=0)
    assert c.max() < 1 << 21
    _, first = np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], return_index=True)      # one point per voxel
    return xyz[np.sort(first)]


def box_cloud(n, voxel=0.05, seed=11):
    """A box-surface cloud downsampled at ``voxel`` to exactly n points: the cube is sized by bisection so that the
    downsampled cloud has a little more than n points, then cut to n."""
    dense = synthetic.make_box_cloud(seed, n_points=6 * n, cube=10.0, n_boxes=8).astype(np.float64)
    lo, hi = 0.01, 100.0                                               # scale of the cloud
    for _ in range(30):
        mid = np.sqrt(lo * hi)
        if len(downsample(dense * mid, voxel)) < 1.02 * n:
            lo = mid
        else:
            hi = mid
    pts = downsample(dense * hi, voxel)
    assert len(pts) >= n, (len(pts), n)
    return pts[:n].astype(np.float32)


def scan_cloud(voxel, scale, seed=5):
    xyz = synthetic.raycast(synthetic.make_scene(seed), np.zeros(3), seed).astype(np.float64) * scale
    return downsample(xyz, voxel).astype(np.float32)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls                                 # ms per call


def case(name, xyz, voxel, offsets=None):
    x = torch.from_numpy(xyz).to(DEV)
    r1, r2 = 2.0 * voxel, 5.0 * voxel
    i1, c1 = F.radius_neighbours(x, r1, 30, offsets)
    nrm = F.normals_from_neighbours(x, i1, c1, None, offsets)
    i2, c2 = F.radius_neighbours(x, r2, 100, offsets)
    sp = F.spfh_from_neighbours(x, nrm, i2, c2)
    stages = [
        ("neighbours (2 v, 30)", lambda: F.radius_neighbours(x, r1, 30, offsets)),
        ("normals", lambda: F.normals_from_neighbours(x, i1, c1, None, offsets)),
        ("neighbours (5 v, 100)", lambda: F.radius_neighbours(x, r2, 100, offsets)),
        ("spfh", lambda: F.spfh_from_neighbours(x, nrm, i2, c2)),
        ("fpfh", lambda: F.fpfh_from_spfh(x, sp, i2, c2, True)),
        ("fpfh_descriptors (all)", lambda: F.fpfh_descriptors(x, voxel, None, offsets)),
    ]
    info = (f"{name}: N = {len(xyz)}, voxel {voxel}; mean list length {c1.float().mean().item():.1f} of 30 at 2 v, "
            f"{c2.float().mean().item():.1f} of 100 at 5 v")
    return dict(name=name, info=info, stages=stages, times=[[] for _ in stages], x=x, voxel=voxel, offsets=offsets)


def network_pass(model, xyz, voxel, offsets):
    from gcl_amd.MinkowskiEngine import utils as me_utils
    from gcl_amd.scripts.test_kitti import forward_clouds
    off = [0, len(xyz)] if offsets is None else list(offsets)
    clouds = []
    for b in range(len(off) - 1):
        coords = me_utils.batched_coordinates([np.floor(xyz[off[b]:off[b + 1]] / voxel).astype(np.int32)])
        clouds.append((torch.ones((len(coords), 1), dtype=torch.float32).to(DEV), coords.to(DEV)))

    def one():
        forward_clouds(model, clouds)

    for _ in range(3):
        one()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(4):
            one()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / 4 * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fpfh_probe.txt"))
    ap.add_argument("--sizes", default="5000,20000,100000")
    ap.add_argument("--no-network", action="store_true")
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "fpfh_probe needs a GPU: a time taken anywhere else says nothing"
    out(f"FPFH descriptors (gcl_amd/lib/fpfh.py): the output of tools/micro/fpfh_probe.py on one {torch.cuda.get_device_name(0)}.")
    out(f"ms per call; {REPEATS} windows of {CALLS} calls per stage, stages in turn; median [min .. max]")
    with torch.cuda.device(DEV), torch.no_grad():
        clouds = [(f"box cloud {n}", box_cloud(n), 0.05, None) for n in (int(s) for s in a.sizes.split(","))]
        clouds.append(("scan, voxel 0.3", scan_cloud(0.3, 1.0), 0.3, None))
        clouds.append(("scan / 6, voxel 0.05", scan_cloud(0.05, 1.0 / 6.0), 0.05, None))
        eight = [box_cloud(5000, seed=20 + b) for b in range(8)]
        clouds.append(("batch of 8 x 5000", np.concatenate(eight), 0.05, np.arange(9) * 5000))
        cases = [case(*c) for c in clouds]                             # also the warm-up of every stage on every cloud
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for c in cases:
                for k, (_, fn) in enumerate(c["stages"]):
                    c["times"][k].append(window(fn, CALLS))
        model = None
        if not a.no_network:
            from gcl_amd.model import load_model
            torch.manual_seed(0)
            model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5,
                                              D=3).to(DEV).eval()
        for c in cases:
            out()
            out(c["info"])
            parts = 0.0
            for (label, _), t in zip(c["stages"], c["times"]):
                med = float(np.median(t))
                if not label.startswith("fpfh_descriptors"):
                    parts += med
                out(f"  {label:<24} {med:9.3f} [{min(t):9.3f} .. {max(t):9.3f}]")
            out(f"  {'sum of the stages':<24} {parts:9.3f}")
            if model is not None:
                t = network_pass(model, c["x"].cpu().numpy(), c["voxel"], c["offsets"])
                out(f"  {'network forward pass':<24} {float(np.median(t)):9.3f} [{min(t):9.3f} .. {max(t):9.3f}]   (orientation only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
