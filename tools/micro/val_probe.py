"""Pairs per second of the validation epoch on the host path and on the device path, on one MI355X:

    python3 tools/micro/val_probe.py [--out profiles/val_probe.txt] [--pairs 64]

Pairs: ``synthetic.make_eval_pair`` (voxel 0.3, baseline 1 m), generated from seeds by a pool of worker processes before the
GPU is touched.  An untrained ResUNetBN2C (32 channels) gives the features: the work per pair is the workload's (both clouds
above 5000 rows, so 5000 correspondences per pair), the poses are not meaningful and none is reported.

Three loops over the same pairs, same process, in turn, REPEATS times each after a warm-up pass over the first 8 pairs:
``FinestContrastiveLossTrainer._valid_epoch`` on the host path, and on the device path at ``batch_pairs`` 1 and 8.  Host clock
around a loop that ends with every result on the host.  Then ``gcl_irls_pose_batch`` alone at 5000 rows per pair for B = 1
and 8, in windows of CALLS calls between two device events, and the host estimator alone on the same rows (host clock).
No gate: nothing is compared against an earlier figure.  Not a test."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REPEATS, CALLS = 3, 20


def _pair(seed):
    from gcl_amd import synthetic
    return synthetic.make_eval_pair(seed, voxel_size=0.3, baseline=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "val_probe.txt"))
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    import multiprocessing as mp
    with mp.get_context("fork").Pool(a.workers) as pool:           # before the first GPU call: the workers never open the GPU
        pairs = pool.map(_pair, range(500, 500 + a.pairs))
    import torch
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    from gcl_amd.util.transform_estimation import est_quad_linear_robust, est_quad_linear_robust_batch
    assert torch.cuda.is_available(), "val_probe needs a GPU: a time taken anywhere else says nothing"
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = FinestContrastiveLossTrainer(make_config(), device=dev)
    rows = [len(p["sinput0_C"]) for p in pairs] + [len(p["sinput1_C"]) for p in pairs]
    out(f"Validation epoch (gcl_amd/lib/validation.py): the output of tools/micro/val_probe.py on one {torch.cuda.get_device_name(0)}.")
    out(f"{len(pairs)} synthetic pairs, {min(rows)} .. {max(rows)} rows per cloud, 5000 correspondences per pair; "
        f"{torch.get_num_threads()} host threads")
    loops = [("host path (_valid_epoch, on_device=False)", dict(on_device=False)),
             ("device path, batch_pairs = 1", dict(on_device=True, batch_pairs=1)),
             ("device path, batch_pairs = 8", dict(on_device=True, batch_pairs=8))]
    for _, kw in loops:                                            # warm-up of every shape class and code object
        np.random.seed(1)
        tr._valid_epoch(pairs[:8], val_max_iter=-1, **kw)
    times = [[] for _ in loops]
    for _ in range(REPEATS):
        for k, (_, kw) in enumerate(loops):
            np.random.seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr._valid_epoch(pairs, val_max_iter=-1, **kw)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            assert res["n"] == len(pairs)
    out()
    out(f"pairs / s over {len(pairs)} pairs; {REPEATS} passes per loop, loops in turn; median [min .. max]")
    for (label, _), t in zip(loops, times):
        r = sorted(len(pairs) / x for x in t)
        out(f"  {label:<44} {float(np.median(r)):8.1f} [{r[0]:8.1f} .. {r[-1]:8.1f}]")
    # the estimator alone, 5000 rows per pair
    rng = np.random.RandomState(2)
    out()
    out(f"gcl_irls_pose_batch alone, 5000 rows per pair (20 steps); {REPEATS * 3} windows of {CALLS} calls; us per call, median [min .. max]")
    with torch.cuda.device(dev):
        for B in (1, 8):
            p = rng.uniform(-40, 40, (B * 5000, 3))
            q = p + np.array([0.25, -0.1, 0.05]) + (rng.uniform(size=(B * 5000, 1)) < 0.3) * rng.normal(0, 5, (B * 5000, 3))
            src, tgt = torch.from_numpy(p).float().to(dev), torch.from_numpy(q).float().to(dev)
            off = torch.arange(B + 1, dtype=torch.int64, device=dev) * 5000
            for _ in range(3):
                est_quad_linear_robust_batch(src, tgt, off)
            torch.cuda.synchronize()
            win = []
            for _ in range(REPEATS * 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    est_quad_linear_robust_batch(src, tgt, off)
                e1.record()
                e1.synchronize()
                win.append(e0.elapsed_time(e1) / CALLS * 1e3)
            out(f"  B = {B}: {float(np.median(win)):9.1f} [{min(win):9.1f} .. {max(win):9.1f}]   "
                f"({float(np.median(win)) / B:.1f} us per pair)")
            if B == 1:
                s, t = src.cpu(), tgt.cpu()
                est_quad_linear_robust(s, t)
                host = []
                for _ in range(REPEATS):
                    t0 = time.perf_counter()
                    est_quad_linear_robust(s, t)
                    host.append((time.perf_counter() - t0) * 1e3)
                out(f"  host est_quad_linear_robust on the same rows: {float(np.median(host)):.1f} ms per call "
                    f"[{min(host):.1f} .. {max(host):.1f}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
