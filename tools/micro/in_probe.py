"""Segmented InstanceNorm (gcl_in_fwd / gcl_in_bwd): what one site costs against the per-cloud loop, and what a ResUNetIN2C
training step costs against the parent commit.

    python3 tools/micro/in_probe.py [--out profiles/in_probe.txt] [--parts ab] [--parent-tree DIR]

(a) ONE InstanceNorm site, forward + backward with residual and ReLU, 28 clouds / about 530 k rows, c = 32, 64, 128, 256: the
    two new entries against the loop this probe writes over the public gcl_bn_* entries (per cloud gcl_bn_stats,
    gcl_bn_apply, gcl_bn_bwd_reduce, gcl_bn_bwd_apply on the cloud's contiguous rows).  Every buffer is allocated before the
    clock starts; a host clock around the calls of one forward + backward, ended by a device synchronise; 3 warm passes, the
    median and range of 15.  y and dx of the two are compared bit for bit first.
(b) a ResUNetIN2C training step (FinestContrastiveLossTrainer.train_step, bs 4 x 7 clouds, ``synthetic`` batches): each tree
    in ROUNDS child processes (``--child``); with ``--parent-tree DIR`` (a checkout of the parent commit, built, with this file
    copied to its tools/micro/) the two trees alternate.  A child warms 3 steps and times 10, each ended by a synchronise.
    Without ``--parent-tree`` only this tree is measured.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ROUNDS = 5
EPS = 1e-8


def fmt(v):
    return f"{np.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"


def timed(fn, warm=3, reps=15):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def part_a(out, dev):
    import torch
    from gcl_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    sizes = [int(v) for v in rs.randint(15000, 23000, size=28)]
    n, ns = sum(sizes), len(sizes)
    out(f"(a) one site, forward + backward (residual, ReLU), {ns} clouds of {min(sizes)} .. {max(sizes)} rows, n = {n}; "
        "ms per forward + backward, median [min .. max]")
    out(f"{'c':>5s} {'per-cloud loop, 6 x 28 launches':>36s} {'gcl_in_fwd + gcl_in_bwd, 8 launches':>38s} {'ratio':>7s}  bits")
    lab = torch.from_numpy(np.repeat(np.arange(ns), sizes))
    seg = torch.zeros(ns + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.as_tensor(sizes), 0)
    seg_off, rows, row_cloud = seg.to(dev), torch.arange(n, dtype=torch.int32, device=dev), lab.to(torch.int32).to(dev)
    st = _lib.stream()
    for c in (32, 64, 128, 256):
        g = torch.Generator().manual_seed(c)
        x, dy, res = (torch.randn(n, c, generator=g).to(dev) for _ in range(3))
        w, b = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        mean, rstd, sum_g, sum_gx = (torch.empty((ns, c), **f32) for _ in range(4))
        y, dx, dres = (torch.empty((n, c), **f32) for _ in range(3))
        mask = torch.empty(lib.gcl_bn_mask_len(n, c), dtype=torch.int64, device=dev)
        scratch = torch.empty(lib.gcl_in_scratch_len(n, ns, c), dtype=torch.float64, device=dev)

        def segmented():
            _lib.check(lib.gcl_in_fwd(_lib.ptr(x), n, c, _lib.ptr(seg_off), _lib.ptr(rows), _lib.ptr(row_cloud), ns, EPS, _lib.ptr(w),
                                      _lib.ptr(b), _lib.ptr(res), 1, _lib.ptr(scratch), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(y),
                                      _lib.ptr(mask), None, st), "gcl_in_fwd")
            _lib.check(lib.gcl_in_bwd(_lib.ptr(x), _lib.ptr(dy), n, c, _lib.ptr(seg_off), _lib.ptr(rows), _lib.ptr(row_cloud), ns,
                                      _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(w), 1, _lib.ptr(mask), _lib.ptr(scratch),
                                      _lib.ptr(sum_g), _lib.ptr(sum_gx), _lib.ptr(dx), _lib.ptr(dres), None, st), "gcl_in_bwd")

        y2, dx2, dres2 = (torch.empty((n, c), **f32) for _ in range(3))
        mean2, rstd2, sg2, sx2 = (torch.empty((ns, c), **f32) for _ in range(4))
        masks = [torch.empty(lib.gcl_bn_mask_len(m, c), dtype=torch.int64, device=dev) for m in sizes]
        scr = [torch.empty(lib.gcl_bn_scratch_len(m, c), dtype=torch.float64, device=dev) for m in sizes]
        # the pointers of every cloud's slices, made once: the loop below is calls into the library only
        P = []
        r0 = 0
        for s, m in enumerate(sizes):
            sl = slice(r0, r0 + m)
            P.append((m, _lib.ptr(x[sl]), _lib.ptr(dy[sl]), _lib.ptr(res[sl]), _lib.ptr(y2[sl]), _lib.ptr(dx2[sl]), _lib.ptr(dres2[sl]),
                      _lib.ptr(mean2[s]), _lib.ptr(rstd2[s]), _lib.ptr(sg2[s]), _lib.ptr(sx2[s]), _lib.ptr(masks[s]), _lib.ptr(scr[s])))
            r0 += m
        pw, pb = _lib.ptr(w), _lib.ptr(b)

        def loop():
            for m, px, pg, pr, py, pdx, pdr, pm, prs, psg, psx, pmask, pscr in P:
                lib.gcl_bn_stats(px, m, c, EPS, 0.0, None, None, pscr, pm, prs, st)
                lib.gcl_bn_apply(px, m, c, pm, prs, pw, pb, pr, 1, py, pmask, None, st)
            for m, px, pg, pr, py, pdx, pdr, pm, prs, psg, psx, pmask, pscr in P:
                lib.gcl_bn_bwd_reduce(px, pg, None, pmask, m, c, pm, prs, 1, pscr, psg, psx, st)
                lib.gcl_bn_bwd_apply(px, pg, None, pmask, m, c, pm, prs, pw, psg, psx, 1, pdx, pdr, None, st)

        segmented()
        loop()
        torch.cuda.synchronize()
        same = all(torch.equal(p, q) for p, q in ((y, y2), (dx, dx2), (dres, dres2), (mean, mean2), (rstd, rstd2), (sum_g, sg2),
                                                  (sum_gx, sx2)))
        tl, ts = timed(loop), timed(segmented)
        out(f"{c:5d} {fmt(tl):>36s} {fmt(ts):>38s} {np.median(ts) / np.median(tl):7.3f}  {'equal' if same else 'DIFFERENT'}")
        del x, dy, res, y, dx, dres, y2, dx2, dres2, mask, scratch, masks, scr, P
        torch.cuda.empty_cache()


def child():
    import torch
    from gcl_amd import synthetic
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    dev = "cuda:0"
    torch.manual_seed(0)
    np.random.seed(0)
    batches = [synthetic.make_train_batch(100 + i, batch_size=4) for i in range(2)]
    tr = FinestContrastiveLossTrainer(make_config(model="ResUNetIN2C"), device=dev)
    res = {"rows": [len(b["sinput_C"]) for b in batches], "clouds": int(batches[0]["sinput_C"][:, 0].max()) + 1, "ms": []}
    for i in range(3):
        loss = tr.train_step(batches[i % 2])[0]
    torch.cuda.synchronize()
    for i in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = tr.train_step(batches[i % 2])[0]
        torch.cuda.synchronize()
        res["ms"].append((time.perf_counter() - t0) * 1e3)
    res["loss"] = float(loss)
    print("IN_PROBE " + json.dumps(res), flush=True)


def run_child(tree):
    cmd = [sys.executable, os.path.join(tree, "tools", "micro", "in_probe.py"), "--child"]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=300)
    for line in p.stdout.splitlines():
        if line.startswith("IN_PROBE "):
            return json.loads(line[len("IN_PROBE "):])
    raise RuntimeError(f"{' '.join(cmd)} gave no result (exit {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")


def part_b(out, parent_tree):
    trees = [("this tree", ROOT)] + ([("parent commit", os.path.abspath(parent_tree))] if parent_tree else [])
    runs = {name: [] for name, _ in trees}
    for _ in range(ROUNDS):                                            # the trees alternate: drift hits both alike
        for name, tree in reversed(trees):
            runs[name].append(run_child(tree))
    r0 = runs["this tree"][0]
    out(f"(b) ResUNetIN2C training step, bs 4 x 7 = {r0['clouds']} clouds, {r0['rows']} rows in the two synthetic batches; each tree in "
        f"{ROUNDS} child processes" + (", the two trees alternating" if parent_tree else "") + "; 3 warm steps, 10 timed (host clock, "
        "synchronised); ms per step, median [min .. max] over all timed steps")
    med = {}
    for name, _ in trees:
        v = [x for r in runs[name] for x in r["ms"]]
        med[name] = float(np.median(v))
        out(f"    {name:<14} {fmt(v)}    medians of the processes: " + " ".join(f"{np.median(r['ms']):.3f}" for r in runs[name]))
    if parent_tree:
        out(f"    this tree / parent = {med['this tree'] / med['parent commit']:.3f} (lower is better); last losses "
            f"{runs['this tree'][0]['loss']:.6f} / {runs['parent commit'][0]['loss']:.6f}")
    else:
        out("  (no --parent-tree: the parent commit was not measured in this run)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "in_probe.txt"))
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    import torch
    assert torch.cuda.is_available(), "in_probe needs a GPU: a time taken anywhere else says nothing"
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    out(f"Segmented InstanceNorm (gcl_in_fwd / gcl_in_bwd): the output of tools/micro/in_probe.py on one {torch.cuda.get_device_name(0)}.")
    if "a" in a.parts:
        with torch.cuda.device(dev):
            part_a(out, dev)
        out()
    if "b" in a.parts:
        part_b(out, a.parent_tree)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
