"""What a complement pair loader's sample (lib/complement_data_loader.py:576-716: the neighbourhood transforms, ranges and
crop, voxelisation, matches) costs on the host and on the device, on one MI355X:

    python3 tools/micro/complement_probe.py [--out profiles/complement_probe.txt]

Workload: one KITTI-sized synthetic sample -- two centre scans and 2 x 2 k = 12 complement scans (k = 3) of ~ 120 k points
each, voxel 0.3 m, both rotations and a scale -- alone (B = 1) and four times over (B = 4).  REPEATS rounds after a warm one, the
variants in turn inside every round, the device idle before and after every timed region (torch.cuda.synchronize), host clock;
median [min .. max] in ms:

    (a) host arithmetic       the loaders' own numpy expressions for what csrc/nghb.hip does, on the calling thread: per raw
                              scan a float32 matmul, then the second one, the squared ranges, the mask, the concatenation; no
                              voxelisation, no matches (those need MinkowskiEngine and open3d on the host)
    (b) device build, B = 1   build_complement_pair_batch_gpu, whole: pinned staging, one copy, every launch, three host reads
    (c) device build, B = 4

and, from rounds of their own (events around every entry slow the host), the device time per stage of (b) and (c): events on
the builder's stream around each C-ABI call, summed per stage.  No gate; generated from seeds; not a test.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcl_amd import _lib                                                               # noqa: E402
from gcl_amd.lib import augment                                                        # noqa: E402
from gcl_amd.lib.complement_data_gpu import build_complement_pair_batch_gpu           # noqa: E402

DEV = torch.device("cuda:0")
REPEATS = 7
VOXEL, RADIUS, K_SIDE, POINTS = 0.3, 0.45, 3, 120000
STAGES = (("centroids, affines, range maximum", ("gcl_cloud_centroids", "gcl_cloud_affines", "gcl_nghb_range_max")),
          ("flags", ("gcl_nghb_flags",)),
          ("compaction", ("gcl_nghb_compact",)),
          ("voxelisation", ("gcl_voxel_coords_aug", "gcl_unique_coords", "gcl_cloud_row_starts", "gcl_loader_points_aug")),
          ("matches", ("gcl_pair_matches_count", "gcl_pair_matches_emit")))


def rigid(yaw, t):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = t
    return T


def scan(rng, pose, n=POINTS):
    """n points of a ground surface with walls, dense near the sensor as a spinning lidar's are, in the sensor's frame."""
    r = 75.0 * rng.rand(n) ** 1.7 + 2.0
    a = rng.uniform(-np.pi, np.pi, n)
    w = np.stack([r * np.cos(a) + pose[0, 3], r * np.sin(a) + pose[1, 3], np.zeros(n)], axis=1)
    w[:, 2] = 0.3 * np.sin(0.2 * w[:, 0]) + 0.2 * np.cos(0.15 * w[:, 1]) - 1.7
    wall = rng.rand(n) < 0.3
    w[wall, 1] = np.round(w[wall, 1] / 12.0) * 12.0
    w[wall, 2] += rng.uniform(0.0, 5.0, wall.sum())
    Pi = np.linalg.inv(pose)
    return (w @ Pi[:3, :3].T + Pi[:3, 3] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)


def make_sample(seed):
    rng = np.random.RandomState(seed)
    P = [rigid(0.0, (0.0, 0.0, 0.0)), rigid(0.05, (9.0, 0.5, 0.0))]
    s = {"radius": RADIUS, "trans": np.linalg.inv(P[1]) @ P[0], "scale": 0.93,
         "rotation0": augment.sample_rotation(np.random.RandomState(seed + 1), 360),
         "rotation1": augment.sample_rotation(np.random.RandomState(seed + 2), 360)}
    for k in (0, 1):
        s[f"xyz{k}"] = scan(rng, P[k])
        poses = [P[k] @ rigid(0.02 * j, (1.2 * j, 0.1 * j, 0.0)) for j in range(-K_SIDE, K_SIDE + 1) if j]
        s[f"cmpl{k}"] = [scan(rng, Q) for Q in poses]
        s[f"list_M{k}"] = [np.linalg.inv(P[k]) @ Q for Q in poses]
    return s


def host_arithmetic(s):
    """__getitem__ :576-628 with the reference's own numpy expressions (BLAS matmul, float32 mean)."""
    def trans(pcd, R):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = R.dot(-np.mean(pcd, axis=0))
        return T

    def apply(pts, T):
        T = T.astype(np.float32)
        return pts @ T[:3, :3].T + T[:3, 3]

    out = []
    for k in (0, 1):
        cm = [apply(x, M) for x, M in zip(s[f"cmpl{k}"], s[f"list_M{k}"])]
        T = trans(s[f"xyz{k}"], s[f"rotation{k}"])
        xyz = apply(s[f"xyz{k}"], T)
        cm = [apply(x, T) for x in cm]
        max_d = np.max((xyz ** 2).sum(-1))
        cat = np.concatenate(cm, axis=0)
        out.append(cat[np.where((cat ** 2).sum(-1) < max_d)[0]])
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


class StageEvents:
    """Events around every C-ABI entry the builder calls, while active."""
    def __init__(self, lib):
        self.lib, self.names = lib, [n for _, names in STAGES for n in names]
        self.saved, self.events = {}, []

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = _fn(*a)
                e1.record()
                self.events.append((_name, e0, e1))
                return rc
            setattr(self.lib, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)

    def per_stage(self):
        torch.cuda.synchronize()
        ms = {}
        for name, e0, e1 in self.events:
            ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
        return [sum(ms.get(n, 0.0) for n in names) for _, names in STAGES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "complement_probe.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "complement_probe needs a GPU: a time taken anywhere else says nothing"
    lib = _lib.require_gpu()
    out(f"A complement pair loader's sample on the host and on the device: the output of tools/micro/complement_probe.py on one "
        f"{torch.cuda.get_device_name(0)}.")
    s = make_sample(11)
    pts = sum(len(s[f"xyz{k}"]) + sum(len(x) for x in s[f"cmpl{k}"]) for k in (0, 1))
    out(f"sample: 2 centre scans + 2 x {2 * K_SIDE} complement scans of {POINTS} points, {pts} raw points ({pts * 12 / 1e6:.1f} MB), "
        f"voxel {VOXEL}, both rotations and a scale")
    out(f"ms; {REPEATS} rounds after a warm round, variants in turn inside a round, device idle around every region; "
        "median [min .. max]")
    with torch.cuda.device(DEV):
        labels = ("(a) host arithmetic, one sample", "(b) device build, B = 1", "(c) device build, B = 4")
        times = [[] for _ in labels]
        stage = {1: [], 4: []}
        for rnd in range(REPEATS + 1):
            ta, nghb = timed(lambda: host_arithmetic(s))
            tb, b1 = timed(lambda: build_complement_pair_batch_gpu([s], VOXEL, DEV))
            tc, b4 = timed(lambda: build_complement_pair_batch_gpu([s] * 4, VOXEL, DEV))
            for B in (1, 4):
                with StageEvents(lib) as ev:
                    build_complement_pair_batch_gpu([s] * B, VOXEL, DEV)
                    per = ev.per_stage()
                if rnd:
                    stage[B].append(per)
            if rnd:
                for t, v in zip(times, (ta, tb, tc)):
                    t.append(v)
        for label, t in zip(labels, times):
            out(f"  {label:<34} {float(np.median(t)):9.3f} [{min(t):9.3f} .. {max(t):9.3f}]")
        out(f"  per sample at B = 4: {float(np.median(times[2])) / 4:.3f} ms")
        out(f"  rows: pcd0 {len(b1['pcd0'][0])}, pcd1 {len(b1['pcd1'][0])}, pcd_nghb0 {len(b1['pcd_nghb0'][0])}, "
            f"pcd_nghb1 {len(b1['pcd_nghb1'][0])}, correspondences {len(b1['correspondences'])}; the host's crop keeps "
            f"{len(nghb[0])} + {len(nghb[1])} of {pts - len(s['xyz0']) - len(s['xyz1'])} complement points")
        assert len(b4["pcd0"]) == 4
        out()
        out("device time per stage (events around the stage's entries, rounds of their own), ms:")
        for B in (1, 4):
            arr = np.array(stage[B])
            out(f"  B = {B}")
            for j, (label, _) in enumerate(STAGES):
                out(f"    {label:<36} {float(np.median(arr[:, j])):8.3f} [{arr[:, j].min():8.3f} .. {arr[:, j].max():8.3f}]")
            out(f"    {'sum of the stages':<36} {float(np.median(arr.sum(axis=1))):8.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
