"""Times behind the SC2-PCR benchmark (gcl_nn_rowmin_any, SC2_PCR_bench.eval_per_pair) on one MI355X:

    python3 tools/micro/sc2_bench_probe.py [--out profiles/sc2_bench_probe.txt] [--parts ab]

(a) the feature 1-NN, 5000 x 5000: gcl_nn_rowmin at 32 channels (the yardstick) against gcl_nn_rowmin_any at 32, 33, 40, 64,
    96 and 128 channels; direct C-ABI calls on preallocated scratch, the variants timed in turn (windows of CALLS calls between
    two device events, REPEATS windows each, median and minimum).  Expectation checked: t_any(33) <= 1.1 x (40 / 32) x t(32).
(b) pairs per second of eval_per_pair on 64 ragged synthetic pairs (3000 - 5000 keypoints, 33-channel descriptors, inlier share
    0.3, config_3DMatch.json's values) with batch_pairs 1 and 8; host clock around a whole run (it ends in an event wait).
Everything is generated from seeds; not a test.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcl_amd import _lib                                              # noqa: E402

DEV = torch.device("cuda:0")
CALLS, REPEATS = 500, 9


def nn_variant(entry, c, ma=5000, mb=5000):
    lib = _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(c)
    A = torch.nn.functional.normalize(torch.randn(ma, c, generator=g), dim=1).to(DEV)
    B = torch.nn.functional.normalize(torch.randn(mb, c, generator=g), dim=1).to(DEV)
    ns = lib.gcl_nn_rowmin_scratch_len(ma, mb) if entry == "gcl_nn_rowmin" else lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c)
    scratch = torch.empty(ns, dtype=torch.int32, device=DEV)
    dmin = torch.empty(ma, dtype=torch.float32, device=DEV)
    arg = torch.empty(ma, dtype=torch.int32, device=DEV)
    fn = getattr(lib, entry)
    args = (_lib.ptr(A), None, ma, _lib.ptr(B), None, mb, c, 0, _lib.ptr(scratch), _lib.ptr(dmin), _lib.ptr(arg))

    def window(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = _lib.stream()
        e0.record()
        for _ in range(calls):
            _lib.check(fn(*args, st), entry)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / calls                   # us per call

    window(20)
    agree = (torch.cdist(A.double(), B.double()).argmin(1) == arg.long()).float().mean().item()
    return dict(name=f"{entry} c={c}", c=c, window=window, times=[], agree=agree, keep=(A, B, scratch, dmin, arg))


def part_a(out):
    variants = [nn_variant("gcl_nn_rowmin", 32)] + [nn_variant("gcl_nn_rowmin_any", c) for c in (32, 33, 40, 64, 96, 128)]
    same = bool((variants[0]["keep"][4] == variants[1]["keep"][4]).all() and (variants[0]["keep"][3] == variants[1]["keep"][3]).all())
    for _ in range(REPEATS):                                          # in turn: drift and neighbours hit every variant alike
        for v in variants:
            v["times"].append(v["window"](CALLS))
    out(f"(a) feature 1-NN, 5000 x 5000, us per call (interleave + search + merge; {REPEATS} windows of {CALLS} calls, in turn)")
    out(f"{'entry':>28} {'median':>9} {'min':>9} {'/ old(32)':>10}  index agreement with fp64")
    base = float(np.median(variants[0]["times"]))
    for v in variants:
        med = float(np.median(v["times"]))
        out(f"{v['name']:>28} {med:9.2f} {min(v['times']):9.2f} {med / base:10.3f}  {v['agree']:.5f}")
    out(f"  gcl_nn_rowmin_any at 32 channels bitwise equal to gcl_nn_rowmin (dmin and argmin): {same}")
    t33 = float(np.median(variants[2]["times"]))
    bound = 1.1 * 40 / 32
    out(f"  expectation t_any(33) <= 1.1 x (40 / 32) x t_old(32): ratio {t33 / base:.3f} against {bound:.3f} -> "
        f"{'holds' if t33 <= bound * base else 'DOES NOT HOLD'}")


def _rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def record(rng, n, m, share=0.3, c=33, half=1.5, noise=0.01):
    src = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-half, half, (m, 3)).astype(np.float32)
    fs, ft = rng.normal(size=(n, c)), rng.normal(size=(m, c))
    R, t = _rot(rng, rng.uniform(0.3, 1.2)), rng.uniform(-0.5, 0.5, 3)
    k = int(round(share * n))
    i, j = rng.permutation(n)[:k], rng.permutation(m)[:k]
    tgt[j] = (src[i].astype(np.float64) @ R.T + t + rng.uniform(-noise, noise, (k, 3))).astype(np.float32)
    ft[j] = fs[i] + 0.02 * rng.normal(size=(k, c))
    fs /= np.linalg.norm(fs, axis=1, keepdims=True)
    ft /= np.linalg.norm(ft, axis=1, keepdims=True)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    return src, tgt, fs.astype(np.float32), ft.astype(np.float32), T


def part_b(out):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair, summarize_pairs
    rng = np.random.RandomState(0)
    records = [record(rng, int(rng.randint(3000, 5001)), int(rng.randint(3000, 5001))) for _ in range(64)]
    cfg = dict(inlier_threshold=0.1, num_node="all", use_mutual=False, d_thre=0.1, num_iterations=10, ratio=0.2,
               nms_radius=0.1, max_points=8000, k1=30, k2=20)
    ev = dict(inlier_threshold=0.1, re_thre=15.0, te_thre=30.0)
    runs = {1: [], 8: []}
    tables = {}
    with torch.cuda.device(DEV):
        m = BatchMatcher(**cfg)
        for bp in runs:
            tables[bp] = eval_per_pair(records, m, ev, batch_pairs=bp)       # warm: code objects, allocator
        for _ in range(5):
            for bp in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eval_per_pair(records, m, ev, batch_pairs=bp)
                runs[bp].append(len(records) / (time.perf_counter() - t0))
    out("(b) eval_per_pair on 64 ragged pairs (3000 - 5000 keypoints, 33 channels, inlier share 0.3), pairs/s, five runs each, in turn;")
    out("    host arrays in, table out (uploads, 1-NN, registration, statistics, one pinned copy per chunk)")
    for bp, label in ((1, "batch_pairs = 1 (one registration call per pair)"), (8, "batch_pairs = 8 (one call per chunk)")):
        s = summarize_pairs(tables[bp])
        out(f"  {label:<50} median {np.median(runs[bp]):8.2f}  min {min(runs[bp]):8.2f} pairs/s   success {s['success_rate']:.3f}")
    cols = list(range(9)) + [11]
    out(f"  columns 0 - 8 bitwise equal between the two: {tables[1][:, cols].tobytes() == tables[8][:, cols].tobytes()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sc2_bench_probe.txt"))
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("SC2-PCR benchmark (gcl_nn_rowmin_any, gcl_registration_stats, SC2_PCR_bench): the output of tools/micro/sc2_bench_probe.py "
        f"on one {torch.cuda.get_device_name(0)}.")
    with torch.cuda.device(DEV):
        if "a" in a.parts:
            part_a(out)
            out("")
        if "b" in a.parts:
            part_b(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
