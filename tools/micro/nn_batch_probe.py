"""What batching the matching stage costs and saves (gcl_nn_rowmin_batch, gcl_mutual_*_batch and the loops on them), on one
MI355X, in one call:

    python3 tools/micro/nn_batch_probe.py [--out profiles/nn_batch_probe.txt] [--parent-tree DIR]

(a) device time of 8 searches: ONE gcl_nn_rowmin_batch call against 8 calls of the single entry, on 5000 x 5000 at 32 and 33
    channels, 1000 x 1000 at 32 and a ragged 3000 - 5000 set at 33; windows of CALLS rounds between two device events, the
    two forms in turn, REPEATS windows each.  Condition: at 5000 x 5000 the batch takes at most 1.05 x the sum of singles.
(b) the mutual filters at 5000 keypoints: 8 single launches against one batch launch, the same way.
(c) HOST time to enqueue the matching of a chunk of 8 ragged pairs (33 channels): per pair ``match_pair`` and the copy into the
    padded buffers, against ``match_pairs``; host clock around the enqueuing calls only, the device drained outside it.
(d) the loops: ``eval_per_pair`` on sc2_bench_probe's 64 ragged pairs at batch_pairs 8, the pair loop of ``evaluate_scene``
    on eth_eval_probe's 16-fragment scene (random unit descriptors given: the loop's time does not depend on their values), and
    the validation epoch of val_probe at batch_pairs 8 on PAIRS of its pairs (seven passes after a warm pass over all of them:
    a pass is ~40 ms, and a first pass over new shapes measures the allocator).  Each runs in a child process of its own
    (``--child``); with ``--parent-tree DIR`` (a checkout of the parent commit, built, with this file copied to its
    tools/micro/) the children of the two trees alternate, ROUNDS each, and the figures of both are reported with the
    condition "not slower than the parent by more than 3 %".  Without it only this tree is measured.
Everything is generated from seeds; not a test."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CALLS, REPEATS, ROUNDS, PAIRS = 50, 9, 3, 64


def fmt(v, unit=""):
    return f"{float(np.median(v)):9.2f} [{min(v):9.2f} .. {max(v):9.2f}]{unit}"


def in_turn(forms, rounds_per_window):
    """us per round of every form (a callable that enqueues one round), windows in turn."""
    import torch
    times = [[] for _ in forms]
    for f in forms:
        f()
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for k, f in enumerate(forms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds_per_window):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / rounds_per_window)
    return times


# ---- (a) -----------------------------------------------------------------------------------------------------------------
def search_forms(sizes, c, dev):
    import torch
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    g = torch.Generator().manual_seed(c + len(sizes) + sizes[0][0])
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, c, generator=g), dim=1).to(dev)
    AB = [(unit(ma), unit(mb)) for ma, mb in sizes]
    fixed = c in (16, 32, 64)
    single, keep = [], []
    for (A, B), (ma, mb) in zip(AB, sizes):
        ns = lib.gcl_nn_rowmin_scratch_len(ma, mb) if fixed else lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c)
        scratch = torch.empty(ns, dtype=torch.int32, device=dev)
        dmin, arg = torch.empty(ma, dtype=torch.float32, device=dev), torch.empty(ma, dtype=torch.int32, device=dev)
        single.append((_lib.ptr(A), None, ma, _lib.ptr(B), None, mb, c, 0, _lib.ptr(scratch), _lib.ptr(dmin), _lib.ptr(arg)))
        keep.append((scratch, dmin, arg))
    fn, name = (lib.gcl_nn_rowmin, "gcl_nn_rowmin") if fixed else (lib.gcl_nn_rowmin_any, "gcl_nn_rowmin_any")
    recs = (_lib.NnSearch * len(sizes))()
    outs = []
    for r, (A, B), (ma, mb) in zip(recs, AB, sizes):
        dmin, arg = torch.empty(ma, dtype=torch.float32, device=dev), torch.empty(ma, dtype=torch.int32, device=dev)
        r.a, r.b, r.ma, r.mb, r.dmin, r.argmin = _lib.ptr(A), _lib.ptr(B), ma, mb, _lib.ptr(dmin), _lib.ptr(arg)
        outs.append((dmin, arg))
    ns = lib.gcl_nn_rowmin_batch_scratch_len(ctypes.addressof(recs), len(sizes), c)
    bscratch = torch.empty(ns, dtype=torch.int32, device=dev)
    table = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to(dev)

    def singles():
        st = _lib.stream()
        for args in single:
            _lib.check(fn(*args, st), name)

    def batch():
        _lib.check(lib.gcl_nn_rowmin_batch(ctypes.addressof(recs), _lib.ptr(table), len(sizes), c, 0, _lib.ptr(bscratch),
                                           _lib.stream()), "gcl_nn_rowmin_batch")

    singles()
    batch()
    torch.cuda.synchronize()
    same = all(torch.equal(k[1], o[0]) and torch.equal(k[2], o[1]) for k, o in zip(keep, outs))
    return singles, batch, same, (AB, keep, outs, bscratch, table, recs)


def part_a(out, dev):
    rng = np.random.RandomState(0)
    ragged = [(int(rng.randint(3000, 5001)), int(rng.randint(3000, 5001))) for _ in range(8)]
    out(f"(a) 8 feature 1-NN searches, device time in us per 8 searches (events; {REPEATS} windows of {CALLS} rounds per form, in turn);")
    out("    median [min .. max]")
    out(f"{'searches':>28} {'8 single calls':>36} {'one batch call':>36} {'batch / singles':>16}  bitwise equal")
    ok = True
    for label, sizes, c, gate in (("5000 x 5000, c = 32", [(5000, 5000)] * 8, 32, True), ("5000 x 5000, c = 33", [(5000, 5000)] * 8, 33, True),
                                  ("1000 x 1000, c = 32", [(1000, 1000)] * 8, 32, False), ("ragged 3000 - 5000, c = 33", ragged, 33, False)):
        singles, batch, same, keep = search_forms(sizes, c, dev)
        ts, tb = in_turn([singles, batch], CALLS)
        ratio = float(np.median(tb) / np.median(ts))
        out(f"{label:>28} {fmt(ts):>36} {fmt(tb):>36} {ratio:16.3f}  {same}")
        if gate:
            ok = ok and ratio <= 1.05
    out(f"  condition: at 5000 x 5000 the batch takes at most 1.05 x the sum of the singles -> {'holds' if ok else 'DOES NOT HOLD'}")


# ---- (b) -----------------------------------------------------------------------------------------------------------------
def part_b(out, dev):
    import torch
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    rng = np.random.RandomState(1)
    m, P = 5000, 8
    jobs = []
    for _ in range(P):
        nn01 = rng.randint(0, m, m).astype(np.int32)
        nn10 = rng.randint(0, m, m).astype(np.int32)
        i = rng.permutation(m)[:1500]
        j = rng.permutation(m)[:1500]
        nn01[i], nn10[j] = j, i                                          # ~30 % mutual pairs
        t = lambda x: torch.from_numpy(x).to(dev)
        jobs.append(dict(nn01=t(nn01), nn10=t(nn10), xyz0=t(rng.normal(size=(m, 3)).astype(np.float32)),
                         xyz1=t(rng.normal(size=(m, 3)).astype(np.float32)),
                         T=t(np.eye(4, dtype=np.float32)[:3].reshape(12).copy()),
                         pairs=torch.empty((m, 2), dtype=torch.int32, device=dev), src=torch.empty((m, 3), device=dev),
                         tgt=torch.empty((m, 3), device=dev), count=torch.empty(2, dtype=torch.int32, device=dev)))
    recs = (_lib.MutualJob * P)()
    for r, j in zip(recs, jobs):
        for k, v in j.items():
            setattr(r, k, _lib.ptr(v))
        r.m0 = r.m1 = m
    table = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to(dev)
    p = _lib.ptr

    def match_single():
        st = _lib.stream()
        for j in jobs:
            _lib.check(lib.gcl_mutual_match(p(j["nn01"]), m, p(j["nn10"]), m, p(j["xyz0"]), p(j["xyz1"]), p(j["T"]), 0.1,
                                            p(j["pairs"]), p(j["count"]), st), "gcl_mutual_match")

    def match_batch():
        _lib.check(lib.gcl_mutual_match_batch(ctypes.addressof(recs), p(table), P, 0.1, _lib.stream()), "gcl_mutual_match_batch")

    def corr_single():
        st = _lib.stream()
        for j in jobs:
            _lib.check(lib.gcl_mutual_correspondences(p(j["nn01"]), m, p(j["nn10"]), m, p(j["xyz0"]), p(j["xyz1"]), 3, p(j["src"]),
                                                      p(j["tgt"]), p(j["count"]), st), "gcl_mutual_correspondences")

    def corr_batch():
        _lib.check(lib.gcl_mutual_correspondences_batch(ctypes.addressof(recs), p(table), P, 3, _lib.stream()),
                   "gcl_mutual_correspondences_batch")

    out(f"(b) the mutual filters, 8 pairs of {m} x {m} keypoints (~30 % mutual), device time in us per 8 pairs; median [min .. max]")
    for label, a, b in (("gcl_mutual_match", match_single, match_batch), ("gcl_mutual_correspondences", corr_single, corr_batch)):
        ts, tb = in_turn([a, b], CALLS)
        out(f"  {label:<28} 8 single launches {fmt(ts)}   one batch launch {fmt(tb)}   batch / singles {np.median(tb) / np.median(ts):.3f}")


# ---- (c) -----------------------------------------------------------------------------------------------------------------
def bench_records(n_pairs=64):
    from sc2_bench_probe import record
    rng = np.random.RandomState(0)
    return [record(rng, int(rng.randint(3000, 5001)), int(rng.randint(3000, 5001))) for _ in range(n_pairs)]


SC2_CFG = dict(inlier_threshold=0.1, num_node="all", use_mutual=False, d_thre=0.1, num_iterations=10, ratio=0.2,
               nms_radius=0.1, max_points=8000, k1=30, k2=20)


def part_c(out, dev):
    import torch
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    m = BatchMatcher(**SC2_CFG)
    chunk = [tuple(torch.from_numpy(x).to(dev)[None] for x in r[:4]) for r in bench_records(8)]

    def old():
        held = [m.match_pair(*p) for p in chunk]
        n = [h[0].shape[1] for h in held]
        src = torch.empty((len(held), max(n), 3), dtype=torch.float32, device=dev)
        tgt = torch.empty((len(held), max(n), 3), dtype=torch.float32, device=dev)
        for j, (s, t) in enumerate(held):
            src[j, :n[j]], tgt[j, :n[j]] = s[0], t[0]
        return src, tgt, n

    def new():
        return m.match_pairs(chunk)

    a, b = old(), new()
    torch.cuda.synchronize()
    same = all(torch.equal(a[0][j, :n], b[0][j, :n]) and torch.equal(a[1][j, :n], b[1][j, :n]) for j, n in enumerate(a[2]))
    times = [[], []]
    for _ in range(REPEATS * 3):
        for k, f in enumerate((old, new)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
    out(f"(c) host time to ENQUEUE the matching of a chunk of 8 ragged pairs (3000 - 5000 keypoints, 33 channels), us per chunk,")
    out(f"    {REPEATS * 3} chunks per form, in turn; median [min .. max]; correspondences bitwise equal: {same}")
    out(f"  per pair match_pair + copy into the padded buffers   {fmt(times[0])}")
    out(f"  match_pairs (one gcl_nn_rowmin_batch call)           {fmt(times[1])}")


# ---- (d) -----------------------------------------------------------------------------------------------------------------
def child():
    """The three loops on THIS tree's gcl_amd -> one JSON line."""
    import multiprocessing as mp
    from val_probe import _pair
    with mp.get_context("fork").Pool(8) as pool:                     # before the first GPU call
        val_pairs = pool.map(_pair, range(500, 500 + PAIRS))
    import torch
    dev = torch.device("cuda:0")
    res = {}
    with torch.cuda.device(dev):
        from gcl_amd.scripts.SC2_PCR import BatchMatcher
        from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair
        records = bench_records()
        m, ev = BatchMatcher(**SC2_CFG), dict(inlier_threshold=0.1, re_thre=15.0, te_thre=30.0)
        table = eval_per_pair(records, m, ev, batch_pairs=8)
        res["sc2_table"] = float(np.nansum(table[:, :9]))
        res["sc2"] = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_per_pair(records, m, ev, batch_pairs=8)
            res["sc2"].append(len(records) / (time.perf_counter() - t0))
        import eth_eval_probe as EP
        import gcl_amd.generalization_ETH.evaluate as E
        _, keys, gt = EP.make_scene(16, 10000)
        g = torch.Generator().manual_seed(4)
        descs = [torch.nn.functional.normalize(torch.randn(len(k), 32, generator=g), dim=1).to(dev) for k in keys]
        keys_d = [torch.from_numpy(k).to(dev) for k in keys]
        first = E.evaluate_scene(None, keys_d, gt, descriptors=descs)
        res["eth_table"], res["eth_pairs"], res["eth"] = float(first["table"].sum()), len(gt), []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.evaluate_scene(None, keys_d, gt, descriptors=descs)
            res["eth"].append((time.perf_counter() - t0) * 1e3)
        from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
        torch.manual_seed(0)
        tr = FinestContrastiveLossTrainer(make_config(), device=dev)
        np.random.seed(1)
        tr._valid_epoch(val_pairs, val_max_iter=-1, on_device=True, batch_pairs=8)      # warm: every chunk's shapes
        res["val"] = []
        for _ in range(7):
            np.random.seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = tr._valid_epoch(val_pairs, val_max_iter=-1, on_device=True, batch_pairs=8)
            torch.cuda.synchronize()
            res["val"].append(len(val_pairs) / (time.perf_counter() - t0))
        res["val_meters"] = [float(r[k]) for k in ("loss", "rte", "hit_ratio")]
    print("NN_BATCH_PROBE " + json.dumps(res), flush=True)


def run_child(tree):
    cmd = [sys.executable, os.path.join(tree, "tools", "micro", "nn_batch_probe.py"), "--child"]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    for line in p.stdout.splitlines():
        if line.startswith("NN_BATCH_PROBE "):
            return json.loads(line[len("NN_BATCH_PROBE "):])
    raise RuntimeError(f"{' '.join(cmd)} gave no result (exit {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")


def part_d(out, parent_tree):
    trees = [("this tree", ROOT)] + ([("parent commit", os.path.abspath(parent_tree))] if parent_tree else [])
    runs = {name: [] for name, _ in trees}
    for _ in range(ROUNDS):                                            # the trees alternate: drift hits both alike
        for name, tree in reversed(trees):
            runs[name].append(run_child(tree))
    out(f"(d) the loops at batch_pairs = 8, each tree in {ROUNDS} child processes" + (", the two trees alternating" if parent_tree else "")
        + "; host clock around a whole loop; median [min .. max]")
    loops = (("sc2", "eval_per_pair, 64 ragged pairs (3000 - 5000 keypoints, 33 channels)", "pairs/s", True),
             ("eth", f"evaluate_scene pair loop, 16 fragments x 5000 keypoints, {runs['this tree'][0]['eth_pairs']} logged pairs", "ms per scene", False),
             ("val", f"validation epoch, {PAIRS} pairs of val_probe, device path", "pairs/s", True))
    for key, label, unit, higher in loops:
        out(f"  {label} [{unit}]")
        med = {}
        for name, _ in trees:
            v = [x for r in runs[name] for x in r[key]]
            med[name] = float(np.median(v))
            out(f"    {name:<14} {fmt(v)}")
        if parent_tree:
            rel = med["this tree"] / med["parent commit"]
            slower = (1 / rel if higher else rel) - 1
            same = all(a[k] == b[k] for a in runs["this tree"] for b in runs["parent commit"]
                       for k in ("sc2_table", "eth_table", "val_meters"))
            out(f"    this tree / parent = {rel:.3f} ({'higher' if higher else 'lower'} is better); not slower than the parent by more "
                f"than 3 %: {'holds' if slower <= 0.03 else 'DOES NOT HOLD'}; results equal: {same}")
    if not parent_tree:
        out("  (no --parent-tree: the parent commit was not measured in this run)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "nn_batch_probe.txt"))
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    import torch
    assert torch.cuda.is_available(), "nn_batch_probe needs a GPU: a time taken anywhere else says nothing"
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    out("Batched matching (gcl_nn_rowmin_batch, gcl_mutual_match_batch, gcl_mutual_correspondences_batch): the output of "
        f"tools/micro/nn_batch_probe.py on one {torch.cuda.get_device_name(0)}.")
    with torch.cuda.device(dev):
        for part, fn in (("a", part_a), ("b", part_b), ("c", part_c)):
            if part in a.parts:
                fn(out, dev)
                out()
    if "d" in a.parts:
        part_d(out, a.parent_tree)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
