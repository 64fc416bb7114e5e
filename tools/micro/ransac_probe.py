"""Feature-matching RANSAC (gcl_ransac_register): milliseconds per registration at the KITTI loop's size.

  n = 5000 correspondences, ransac_n 4, edge similarity 0.9, both distances 0.3, 4 000 000 iterations,
  confidence off (every hypothesis is drawn) and 0.999 (open3d's default: the limit ends the run after the first chunks),
  inlier shares 0.05 / 0.3 / 0.6 (the shares of the SC2-PCR row of DESIGN.md 7.4).

Synthetic correspondences: src uniform in a 100 m cube, a rotation of 0.7 rad about a random axis plus a translation, +-0.05 of
noise on the inliers, the other targets redrawn in the cube.  One process; per configuration two warm calls, then ``--repeats``
calls, each between two events on the stream (the call's allocations -- scratch and outputs, from torch's caching
allocator -- are inside); the median and the minimum are printed.  ``--once`` makes ONE call, share 0.3 with confidence off,
for a kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/micro/ransac_probe.py --once

    python3 tools/micro/ransac_probe.py [--out FILE] [--repeats 9] [--iterations 4000000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np


def correspondences(seed, n, share, half=50.0, noise=0.05):
    rng = np.random.RandomState(seed)
    src = rng.uniform(-half, half, (n, 3))
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    tgt = src @ R.T + np.array([3.0, -2.0, 1.0]) + rng.uniform(-noise, noise, (n, 3))
    out = rng.permutation(n)[int(round(share * n)):]
    tgt[out] = rng.uniform(-half, half, (len(out), 3))
    return src.astype(np.float32), tgt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iterations", type=int, default=4000000)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from gcl_amd.lib.ransac import ransac_correspondences
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"gcl_ransac_register, n = {args.n}, ransac_n 4, similarity 0.9, distances 0.3, {args.iterations} iterations, "
        "scoring: one hypothesis per wave")
    say(f"{'inlier share':>12s} {'confidence':>10s} {'median ms':>10s} {'min ms':>10s}   winner's inliers / covered / scored")
    shares = (0.3,) if args.once else (0.05, 0.3, 0.6)
    with torch.cuda.device(dev):
        for share in shares:
            src, tgt = (torch.from_numpy(a).to(dev) for a in correspondences(1, args.n, share))
            for conf in ((0.0,) if args.once else (0.0, 0.999)):
                def call():
                    return ransac_correspondences(src, tgt, 0.3, 4, 0.9, 0.3, args.iterations, conf, seed=7)
                times = []
                for rep in range(1 if args.once else 2 + args.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = call()
                    e1.record()
                    e1.synchronize()
                    if args.once or rep >= 2:
                        times.append(e0.elapsed_time(e1))
                info = res.info.tolist()
                say(f"{share:12.2f} {('off' if conf == 0.0 else conf)!s:>10s} {np.median(times):10.3f} {np.min(times):10.3f}   "
                    f"{info[1]} / {info[2]} / {info[3]}")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
