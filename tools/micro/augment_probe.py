"""What the raw-scan loader's augmentation (rotation about the centroid + scale, lib/colocation_data_loader.py:349-370) costs on
the host and on the device, on one MI355X:

    python3 tools/micro/augment_probe.py [--out profiles/augment_probe.txt]

Workload: the bs 4 x 7 scans synthetic batch (synthetic.make_raw_sample without its own rotation / scale: the scans as the files
hold them), one rotation and one scale per sample.  Per batch, REPEATS rounds, the variants in turn inside every round, the
device idle before and after every timed region (torch.cuda.synchronize), host clock; median [min .. max] in ms:

    (a) host augmentation    the reference's arithmetic in numpy on the calling thread: a float32 np.mean per cloud,
                             pts @ R.T + T with the float32 transform, scale * xyz, list_M followed; no GPU work
    (b) build, augmented in  build_batch_gpu on the output of (a): the path without keys
    (c) build, keys          build_batch_gpu on the raw scans with "rotation" / "scale": centroids, affines and the transformed
                             points on the device

and train_from_scans steps/s (the headline model, lr as configured) with a producer that runs (a) before handing a batch over
against one that hands over the raw scans with the keys; the two in turn, twice.  No gate; generated from seeds; not a test.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcl_amd import synthetic                                                          # noqa: E402
from gcl_amd.lib import augment                                                        # noqa: E402
from gcl_amd.lib.colocation_data_gpu import build_batch_gpu, train_from_scans          # noqa: E402

DEV = torch.device("cuda:0")
REPEATS = 9
VOXEL = 0.3
N_BATCHES, WARMUP, STEPS = 3, 4, 16


def raw_batch(first_seed, bs=4):
    out = []
    for b in range(bs):
        s = synthetic.make_raw_sample(first_seed + b, VOXEL, random_rotation=False, random_scale=False)
        s["rotation"] = augment.sample_rotation(np.random.RandomState(first_seed + b), 360)
        s["scale"] = 0.8 + 0.4 * np.random.RandomState(1000 + first_seed + b).rand()
        out.append(s)
    return out


def host_augment(sample):
    """ColocationKittiDataset.__getitem__ :349-370 with the reference's own numpy expressions."""
    R, scale = sample["rotation"], sample["scale"]

    def trans(pcd):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = R.dot(-np.mean(pcd, axis=0))
        return T

    def apply(pts, T):
        T = T.astype(np.float32)
        return pts @ T[:3, :3].T + T[:3, 3]

    xyz, list_M = list(sample["xyz"]), [np.array(M, dtype=np.float64) for M in sample["list_M"]]
    T0 = trans(xyz[0])
    xyz[0] = apply(xyz[0], T0)
    for i in range(1, len(xyz)):
        Tc = trans(xyz[i])
        xyz[i] = apply(xyz[i], Tc)
        list_M[i - 1] = T0 @ list_M[i - 1] @ np.linalg.inv(Tc)
    xyz = [np.float32(scale) * x for x in xyz]
    for M in list_M:
        M[:3, 3] = scale * M[:3, 3]
    return {"xyz": xyz, "list_M": list_M, "radius": sample["radius"] * scale, "rng": sample["rng"]}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def steps_per_s(batches, host_side):
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    torch.manual_seed(0)
    np.random.seed(0)
    trainer = FinestContrastiveLossTrainer(make_config(batch_size=len(batches[0])), device=DEV)

    def feed():
        for i in range(WARMUP + STEPS + 6):
            b = batches[i % len(batches)]
            yield [host_augment(s) for s in b] if host_side else b

    it = train_from_scans(trainer, feed(), voxel_size=VOXEL, jitter=synthetic.raw_sample_jitter)
    for _ in range(WARMUP):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        loss, _, _ = next(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it.close()
    return STEPS / dt, float(loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "augment_probe.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "augment_probe needs a GPU: a time taken anywhere else says nothing"
    out(f"Loader augmentation on the host and on the device: the output of tools/micro/augment_probe.py on one "
        f"{torch.cuda.get_device_name(0)}.")
    batches = [raw_batch(100 + 10 * k) for k in range(N_BATCHES)]
    raw = batches[0]
    pts = sum(len(x) for s in raw for x in s["xyz"])
    out(f"batch: {len(raw)} samples x {len(raw[0]['xyz'])} scans, {pts} raw points ({pts * 12 / 1e6:.1f} MB)")
    out(f"ms per batch; {REPEATS} rounds after a warm round, variants in turn inside a round, device idle around every region; "
        "median [min .. max]")
    with torch.cuda.device(DEV):
        labels = ("(a) host augmentation", "(b) build, augmented in", "(c) build, keys")
        times = [[] for _ in labels]
        for rnd in range(REPEATS + 1):
            ta, hosted = timed(lambda: [host_augment(s) for s in raw])
            tb, bb = timed(lambda: build_batch_gpu(hosted, VOXEL, DEV, jitter=synthetic.raw_sample_jitter(hosted)))
            tc, bc = timed(lambda: build_batch_gpu(raw, VOXEL, DEV, jitter=synthetic.raw_sample_jitter(raw)))
            if rnd:
                for t, v in zip(times, (ta, tb, tc)):
                    t.append(v)
        for label, t in zip(labels, times):
            out(f"  {label:<26} {float(np.median(t)):9.3f} [{min(t):9.3f} .. {max(t):9.3f}]")
        out(f"  voxels per batch: {len(bb['sinput_C'])} after (a) + (b), {len(bc['sinput_C'])} after (c) "
            "(the host's float32 mean and BLAS product are not the device's arithmetic: a few points change voxel)")
        out()
        out(f"train_from_scans, steps/s over {STEPS} steps after {WARMUP} ({N_BATCHES} batches in turn), the two producers in turn:")
        for rnd in range(2):
            for label, host_side in (("host-augmenting producer", True), ("keys, device augmentation", False)):
                sps, loss = steps_per_s(batches, host_side)
                out(f"  run {rnd}: {label:<26} {sps:7.2f} steps/s   (last loss {loss:.4f})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
