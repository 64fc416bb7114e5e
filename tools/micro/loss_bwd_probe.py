"""What the ordered loss backward (``deterministic_loss_backward``) costs, measured:

    python tools/micro/loss_bwd_probe.py [--parent DIR] [--out profiles/loss_bwd_ordered.txt]

1. the backward chain alone at the benchmark step's loss shapes (32 channels, groups of 16, the default hard-negative subset
   of 256 rows per sample at batch size 4, 256 selected groups per sample -- and 256 in all), zero fill of dF included:
   atomic = gcl_group_loss_bwd + gcl_neg_loss_bwd; ordered = the two emit entries + gcl_ordered_row_sum.  200 calls per
   sample after 50, events on the stream, 7 samples: median and range.
2. the training step of bench.py's workload with the flag off and on, the same commit, in ALTERNATING child processes
   (5 of each, 20 timed steps after 8): median and range of ms per step.
3. with ``--parent DIR`` (a built checkout of the parent commit): the default step, ``bench.py --gpus 1 --steps 20 --warmup 5``,
   here and there in alternating child processes (5 of each).

The batches of 2. are generated once (before this process touches the GPU) and handed to the children in a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

C, GROUP, N_ROWS = 32, 16, 530000
HN = 256 * 4


def med(v):
    return f"median {statistics.median(v):.3f}  range {min(v):.3f} .. {max(v):.3f}"


# ---- 1. the chain ------------------------------------------------------------------------------------------------------------
def chain_inputs(n_sel, dev):
    rng = np.random.RandomState(0)
    g = torch.Generator().manual_seed(0)
    n_groups = 4096
    F = torch.nn.functional.normalize(torch.randn(N_ROWS, C, generator=g), dim=1)
    index = torch.from_numpy(rng.choice(N_ROWS, n_groups * GROUP, replace=False).astype(np.int64))
    anchors = F[index[::GROUP]].repeat_interleave(GROUP, 0)                # loose groups: both hinges active
    F[index] = torch.nn.functional.normalize(anchors + 0.5 * torch.randn(n_groups * GROUP, C, generator=g) / C ** 0.5, dim=1)
    flag = torch.zeros(n_groups * GROUP, dtype=torch.uint8)
    flag[::GROUP] = 1
    group = torch.full((n_groups,), GROUP, dtype=torch.int64)
    draws = (rng.choice(n_groups, n_sel, replace=False), rng.choice(N_ROWS, HN, replace=False),
             rng.choice(N_ROWS, HN, replace=False))
    return F.to(dev), group, index, flag, draws


def time_chain(n_sel, det, dev, calls=200, warmup=50, samples=7):
    from gcl_amd.lib.colocation_trainer import finest_contrastive_loss
    F, group, index, flag, draws = chain_inputs(n_sel, dev)
    F.requires_grad_(True)
    total = finest_contrastive_loss(F, group, index, None, flag, draws=draws, total_weights=(1.0, 1.0, 1.0),
                                    deterministic_loss_backward=det)[0]
    run = lambda: torch.autograd.grad(total, F, retain_graph=True)         # the loss node's backward: seed, zero fill, the chain
    out = []
    for _ in range(samples):
        for _ in range(warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return out


# ---- 2. the step, flag off / on ------------------------------------------------------------------------------------------------
def child_step(batch_file, det, steps=20, warmup=8):
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config, prefetch_to_device
    batches = torch.load(batch_file, weights_only=False)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    keys = ("sinput_C", "sinput_F", "group", "index", "finest_flag")
    host = [{k: (v.pin_memory() if isinstance(v, torch.Tensor) else v) for k, v in b.items() if k in keys} for b in batches]
    trainer = FinestContrastiveLossTrainer(make_config(batch_size=4, deterministic_loss_backward=bool(det)), device=dev)
    depth = 2
    it = trainer.train_steps(prefetch_to_device((host[i % len(host)] for i in range(warmup + steps + depth)), dev, keys))
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = next(it)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it.close()
    print(json.dumps({"ms_per_step": dt / steps * 1e3, "loss": float(loss)}), flush=True)


def last_json(text):
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("no JSON line in the child's output:\n" + text[-2000:])


def run_child(cmd, cwd, limit):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {r.returncode}:\n{r.stderr[-2000:]}")
    out = last_json(r.stdout)
    print(f"   . {os.path.basename(cwd) or cwd}: {' '.join(cmd[1:])} -> {out.get('ms_per_step'):.3f} ms per step", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child-step", nargs=2, metavar=("BATCHES", "FLAG"))
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if a.child_step:
        child_step(a.child_step[0], int(a.child_step[1]))
        return
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        batch_file = os.path.join(tmp, "batches.pt")
        if not a.no_step:          # forked generator workers: before this process touches the GPU
            import bench
            torch.save(bench.make_batches(0, 4, 4, "fixed16"), batch_file)
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        say(f"loss backward, atomic against ordered (emit + gcl_ordered_row_sum); {torch.cuda.get_device_name(0)}")
        say(f"1. the backward chain alone: dF {N_ROWS} x {C}, groups of {GROUP}, {HN} + {HN} negative rows; us per call, "
            "zero fill of dF and gcl_loss_seed included (200 calls after 50, 7 samples)")
        time_chain(1024, False, dev, samples=2)                             # discarded: the clocks of a fresh process ramp up
        for n_sel in (256, 1024):
            for det in (False, True):
                say(f"   {n_sel:5d} selected groups  {'ordered' if det else 'atomic ':<8} {med(time_chain(n_sel, det, dev))}")
        if not a.no_step:
            say(f"2. the training step of bench.py's workload (batch size 4, four batches in rotation), flag off / on, "
                f"{a.rounds} alternating child processes each, 20 timed steps after 8; ms per step")
            res = {0: [], 1: []}
            for _ in range(a.rounds):
                for det in (0, 1):
                    out = run_child([sys.executable, os.path.abspath(__file__), "--child-step", batch_file, str(det)], ROOT, 600)
                    res[det].append(out["ms_per_step"])
            say(f"   flag off  {med(res[0])}")
            say(f"   flag on   {med(res[1])}")
        if a.parent:
            say(f"3. the default step, bench.py --gpus 1 --steps 20 --warmup 5, this commit against its parent, {a.rounds} "
                "alternating child processes each; ms per step")
            res = {"parent": [], "this": []}
            for _ in range(a.rounds):
                for name, cwd in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
                    out = run_child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd, 900)
                    res[name].append(out["ms_per_step"])
            say(f"   parent    {med(res['parent'])}")
            say(f"   this      {med(res['this'])}")
            say(f"   this / parent (medians): {statistics.median(res['this']) / statistics.median(res['parent']):.4f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
