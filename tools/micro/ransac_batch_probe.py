"""Batched feature-matching RANSAC: ONE gcl_ransac_register_batch call for a chunk of the KITTI loop against the parent
path, eight gcl_ransac_register calls one after the other.

  8 pairs x 5000 correspondences, ransac_n 4, edge similarity 0.9, both distances 0.3, 4 000 000 iterations, inlier share 0.3,
  confidence off (every hypothesis is drawn) and 0.999 (open3d's default).

Synthetic correspondences as tools/micro/ransac_probe.py makes them, one data seed and one RANSAC seed per pair.  One process;
per configuration one warm run of each path, then the two paths in turn ``--repeats`` times, each run between two events on
the stream with the calls' allocations inside (scratch and outputs from torch's caching allocator: 8 x 40 MB in one block for
the batch, one 40 MB block reused by the singles); the median and the minimum are printed, and the two paths'
transformations are compared bit for bit.

    python3 tools/micro/ransac_batch_probe.py [--out profiles/ransac_batch_probe.txt] [--repeats 9] [--pairs 8]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tools.micro.ransac_probe import correspondences


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iterations", type=int, default=4000000)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.3)
    args = ap.parse_args()
    import torch
    from gcl_amd.lib.ransac import ransac_correspondences, ransac_correspondences_batch
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    B = args.pairs
    seeds = [7 + b for b in range(B)]
    say(f"gcl_ransac_register_batch against {B} x gcl_ransac_register: {B} pairs x {args.n} correspondences, ransac_n 4, "
        f"similarity 0.9, distances 0.3, {args.iterations} iterations, inlier share {args.share}")
    say(f"{'confidence':>10s} {'path':>16s} {'median ms':>10s} {'min ms':>10s} {'ms / pair':>10s}   covered per pair")
    with torch.cuda.device(dev):
        data = [correspondences(1 + b, args.n, args.share) for b in range(B)]
        src = torch.from_numpy(np.stack([d[0] for d in data])).to(dev)
        tgt = torch.from_numpy(np.stack([d[1] for d in data])).to(dev)

        def timed(fns):
            """One warm run of every path, then the paths in turn, ``--repeats`` times: a drift of the clock or of the host
            falls on both alike."""
            times, res = [[] for _ in fns], [None] * len(fns)
            for rep in range(1 + args.repeats):
                for k, fn in enumerate(fns):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res[k] = fn()
                    e1.record()
                    e1.synchronize()
                    if rep >= 1:
                        times[k].append(e0.elapsed_time(e1))
            return times, res

        for conf in (0.0, 0.999):
            def singles():
                return [ransac_correspondences(src[b], tgt[b], 0.3, 4, 0.9, 0.3, args.iterations, conf, seed=seeds[b])
                        for b in range(B)]

            def batch():
                return ransac_correspondences_batch(src, tgt, 0.3, 4, 0.9, 0.3, args.iterations, conf, seeds=seeds)

            (t1, tb), (r1, rb) = timed([singles, batch])
            same = all(torch.equal(r.transformation, rb.transformation[b]) and torch.equal(r.info, rb.info[b])
                       for b, r in enumerate(r1))
            name = "off" if conf == 0.0 else str(conf)
            say(f"{name:>10s} {f'{B} single calls':>16s} {np.median(t1):10.3f} {np.min(t1):10.3f} {np.median(t1) / B:10.3f}   "
                f"{[int(r.info[2]) for r in r1]}")
            say(f"{name:>10s} {'one batched call':>16s} {np.median(tb):10.3f} {np.min(tb):10.3f} {np.median(tb) / B:10.3f}   "
                f"{rb.info[:, 2].tolist()}")
            say(f"{'':>10s} batched / singles = {np.median(tb) / np.median(t1):.3f}, results bitwise equal: {same}")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
