"""Batched SC2-PCR registration: what ONE gcl_sc2_register_batch call for 8 pairs costs against 8 gcl_sc2_register calls in a
row, whether a single registration moved against the parent commit's library, and the eval loop with one call per chunk.

  (a) 8 pairs, KITTI's configuration (bench.py's registration problem: n correspondences, outliers uniform in the scene, one
      data seed per pair): n = 8000 at inlier shares 0.05, 0.3, 0.6 and n = 5000 at 0.3.  ``BatchMatcher.SC2_PCR`` against 8 x
      ``Matcher.SC2_PCR``: one warm run of each path, then the two paths in turn ``--repeats`` times, each run between two
      events on the stream with the calls' allocations inside (torch's caching allocator: 8 x 528 MB in one block for the
      batch, one 528 MB block reused by the singles); median and minimum, results compared bit for bit.
  (b) ``--parent-lib A --parent-lib-copy B`` (the parent commit's libgcl_hip.so built elsewhere, and a second copy of that
      file under another name): ONE pair through gcl_sc2_register of this tree's library against the parent's, both loaded in
      this process and called in turn, two warm calls and the median of 15; before that the parent against its own copy, the
      same way: the spread a difference has to exceed to mean anything.
  (c) ``eval_batch.eval_pairs(BatchMatcher, batch_registration=True, batch_pairs=8)`` against ``test_kitti.eval_pairs(Matcher,
      batch_pairs=8)`` on bench.py's eight twin pairs, 4 x 8 pairs per timed call, pairs/s as the median of five ~1 s repeats.

    python3 tools/micro/sc2_batch_probe.py [--out profiles/sc2_batch_probe.txt] [--parts abc] [--parent-lib ... --parent-lib-copy ...]
"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

KITTI = dict(inlier_threshold=0.6, use_mutual=False, d_thre=0.1, num_iterations=20, ratio=0.2, nms_radius=0.6, max_points=8000,
             k1=30, k2=20)


def problem(seed, n, share):
    """bench.py's registration problem (tools/sc2pcr_profile.py's), with its own seed."""
    rng = np.random.RandomState(seed)
    src = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    src[:, 2] *= 0.1
    ang = np.deg2rad(15.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    tgt = (src @ R.T + np.array([5.0, 1.0, 0.3]) + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    bad = rng.rand(n) >= share
    tgt[bad] = rng.uniform(-40, 40, (int(bad.sum()), 3)).astype(np.float32)
    return src, tgt


def _twin(seed):
    from gcl_amd import synthetic
    return synthetic.make_twin_eval_pair(seed, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-lib-copy", default=None)
    args = ap.parse_args()
    twins = None
    if "c" in args.parts:                                # numpy ray casts, by forked workers BEFORE the process touches the GPU
        import multiprocessing as mp
        with mp.get_context("fork").Pool(8) as pool:
            twins = pool.map(_twin, [200 + s for s in range(8)])
    import torch
    from gcl_amd import _lib
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res

    def in_turn(fns, warm, repeats):
        """``warm`` runs of every path, then the paths in turn ``repeats`` times: a drift of the clock or of the host falls on
        all alike."""
        times, res = [[] for _ in fns], [None] * len(fns)
        for rep in range(warm + repeats):
            for k, fn in enumerate(fns):
                ms, res[k] = event_ms(fn)
                if rep >= warm:
                    times[k].append(ms)
        return times, res

    B = args.pairs
    with torch.cuda.device(dev), torch.no_grad():
        if "a" in args.parts:
            say(f"(a) one gcl_sc2_register_batch call against {B} x gcl_sc2_register: KITTI configuration, {args.repeats} runs "
                f"each, in turn, allocations included")
            say(f"{'n':>6s} {'share':>6s} {'path':>16s} {'median ms':>10s} {'min ms':>10s} {'ms / pair':>10s}")
            for n, share in ((8000, 0.05), (8000, 0.3), (8000, 0.6), (5000, 0.3)):
                data = [problem(1 + b, n, share) for b in range(B)]
                src = torch.from_numpy(np.stack([d[0] for d in data])).to(dev)
                tgt = torch.from_numpy(np.stack([d[1] for d in data])).to(dev)
                one, bat = Matcher(num_node="all", **KITTI), BatchMatcher(num_node="all", **KITTI)

                def singles():
                    out = []
                    for b in range(B):
                        T = one.SC2_PCR(src[b:b + 1], tgt[b:b + 1])
                        out.append((T, one._labels, one.last["fitness"], one.last["seeds"]))
                    return out

                def batch():
                    T = bat.SC2_PCR(src, tgt)
                    return T, bat._labels, bat.last

                (t1, tb), (r1, rb) = in_turn([singles, batch], 1, args.repeats)
                same = all(torch.equal(r[0][0], rb[0][b]) and torch.equal(r[1][0], rb[1][b]) and
                           torch.equal(r[2], rb[2][b]["fitness"]) and torch.equal(r[3], rb[2][b]["seeds"])
                           for b, r in enumerate(r1))
                say(f"{n:6d} {share:6.2f} {f'{B} single calls':>16s} {np.median(t1):10.3f} {np.min(t1):10.3f} "
                    f"{np.median(t1) / B:10.3f}")
                say(f"{n:6d} {share:6.2f} {'one batched call':>16s} {np.median(tb):10.3f} {np.min(tb):10.3f} "
                    f"{np.median(tb) / B:10.3f}")
                say(f"{'':>13s} batched / singles = {np.median(tb) / np.median(t1):.3f}, results bitwise equal: {same}")
                del src, tgt, r1, rb
                torch.cuda.empty_cache()
        if "b" in args.parts and args.parent_lib and args.parent_lib_copy:
            say("")
            say("(b) ONE pair, n = 8000, through gcl_sc2_register: this tree's library against the parent commit's, both loaded in "
                "one process, called in turn; 2 warm calls, median of 15 (ms)")

            def bind(path):
                lib = ctypes.CDLL(path)
                for name in ("gcl_sc2_register", "gcl_sc2_register_scratch_bytes"):
                    fn = getattr(lib, name)
                    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
                return lib

            libs = {"this tree": bind(_lib.LIB_PATH), "parent": bind(args.parent_lib), "parent, 2nd copy": bind(args.parent_lib_copy)}
            n, ns, k1 = 8000, 1600, 30
            scratch = torch.empty(libs["parent"].gcl_sc2_register_scratch_bytes(n), dtype=torch.uint8, device=dev)
            say(f"{'share':>6s} {'parent':>10s} {'2nd copy':>10s} {'spread':>10s} {'this tree':>10s} {'this - parent':>14s}   verdict")
            worst = False
            for share in (0.05, 0.3, 0.6):
                s, t = (torch.from_numpy(a).to(dev) for a in problem(1, n, share))

                def call(lib):
                    out = dict(conf=torch.empty(n, device=dev), seeds=torch.empty(ns, dtype=torch.int64, device=dev),
                               knn=torch.empty(ns * k1, dtype=torch.int32, device=dev), st=torch.empty(ns * 12, device=dev),
                               fit=torch.empty(ns, device=dev), best=torch.empty(1, dtype=torch.int32, device=dev),
                               T=torch.empty(16, device=dev), lab=torch.empty(n, device=dev))
                    _lib.check(lib.gcl_sc2_register(_lib.ptr(s), _lib.ptr(t), n, 0.1, 20, 0.6, ns, k1, 20, 0.6, 1.2, 20,
                                                    _lib.ptr(scratch), *(_lib.ptr(out[k]) for k in ("conf", "seeds", "knn", "st",
                                                                                                    "fit", "best", "T", "lab")),
                                                    _lib.stream()))
                    return out

                (tp, tq), _ = in_turn([lambda: call(libs["parent"]), lambda: call(libs["parent, 2nd copy"])], 2, 15)
                (tp2, tn), (rp, rn) = in_turn([lambda: call(libs["parent"]), lambda: call(libs["this tree"])], 2, 15)
                raw = lambda t: t.cpu().numpy().tobytes()                       # bytes: a NaN hypothesis equals itself
                differ = [k for k in rp if raw(rp[k]) != raw(rn[k])]
                same = "True" if not differ else f"False ({', '.join(differ)} differ)"
                spread = abs(np.median(tq) - np.median(tp))
                diff = np.median(tn) - np.median(tp2)
                slower = diff > spread
                worst = worst or slower
                say(f"{share:6.2f} {np.median(tp):10.4f} {np.median(tq):10.4f} {spread:10.4f} {np.median(tn):10.4f} {diff:14.4f}   "
                    f"{'SLOWER than the parent by more than the spread' if slower else 'within the spread (or faster)'}; "
                    f"outputs bitwise equal: {same}")
            say("decision: " + ("the single-pair entries go back to the parent's kernels" if worst else
                                "the single-pair kernels stay the shared bodies (one source for both entries)"))
        if "c" in args.parts:
            from gcl_amd.model import load_model
            from gcl_amd.scripts import eval_batch, test_kitti
            say("")
            say("(c) the eval loop on bench.py's 8 twin pairs (4 x 8 pairs per timed call, batch_pairs = 8, num_node 8000): pairs/s, "
                "five ~1 s repeats each")
            torch.manual_seed(0)
            np.random.seed(0)
            model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
            model.eval()
            paths = {"test_kitti.eval_pairs, Matcher (one call per pair)":
                     lambda: test_kitti.eval_pairs(model, twins * 4, Matcher(num_node=8000, **KITTI), device=dev, batch_pairs=8),
                     "eval_batch.eval_pairs, BatchMatcher (one call per chunk)":
                     lambda: eval_batch.eval_pairs(model, twins * 4, BatchMatcher(num_node=8000, **KITTI), device=dev,
                                                   batch_pairs=8, batch_registration=True)}
            res = {}
            for name, fn in paths.items():
                np.random.seed(3)
                res[name] = fn()                                               # warm-up, and the results to compare
                torch.cuda.synchronize()
            rates = {name: [] for name in paths}
            for _ in range(5):
                for name, fn in paths.items():
                    t0, k = time.perf_counter(), 0
                    while True:
                        fn()
                        k += 1
                        torch.cuda.synchronize()
                        if time.perf_counter() - t0 > 1.0 or k >= 50:
                            break
                    rates[name].append(len(twins) * 4 * k / (time.perf_counter() - t0))
            a, b = (res[name] for name in paths)
            same = all(torch.equal(x, y) for x, y in zip(a["T_est"], b["T_est"]))
            for name in paths:
                say(f"  {name:58s} median {np.median(rates[name]):7.2f}  min {np.min(rates[name]):7.2f} pairs/s   "
                    f"success {res[name]['success_rate']:.3f}")
            say(f"  T_est bitwise equal under one np.random seed: {same}")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
