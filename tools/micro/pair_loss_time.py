"""Time and launch count of the pair family's losses (forward + backward) against the reference's own formulation
executed with torch ops on the same GPU:  python tools/micro/pair_loss_time.py [--out profiles/pair_loss_timing.txt]

The yardstick ("torch") is what lib/trainer.py does, moved to the device as it stands: index_select gathers, the
[num_pos, num_hn, C] broadcast of lib/metrics.py's pdist, ``.min(1)``, the ``.cpu()`` hop of the arg-minima, np.isin on the
host, boolean-mask indexing, autograd.  Sizes: the reference's defaults at batch size 4 (N0, N1 = 20 k rows x 32,
P = 8 k pairs, num_pos 1024, num_hn 2048, num_rand 4096).  50 timed calls after 10, events on the stream.  Launch counts:
each (implementation, loss) runs as a child under ``rocprofv3 --kernel-trace --stats`` with 10 and with 20 calls; the
difference of the kernel-call totals / 10 is the launches per call (set-up kernels cancel).  ``--no-count`` skips that.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N0, N1, P, C = 20000, 20000, 8000, 32
NUM_POS, NUM_HN, NUM_RAND, MARGIN = 1024, 2048, 4096, 1.4
LOSSES = ("contrastive_rand", "triplet", "hardest_triplet")


def inputs(dev):
    g = torch.Generator().manual_seed(0)
    rng = np.random.RandomState(0)
    F0 = torch.nn.functional.normalize(torch.randn(N0, C, generator=g), dim=1)
    F1 = torch.nn.functional.normalize(torch.randn(N1, C, generator=g), dim=1)
    pairs = np.stack([rng.choice(N0, P, replace=False), rng.choice(N1, P, replace=False)], 1).astype(np.int64)
    F1[pairs[:, 1]] = torch.nn.functional.normalize(F0[pairs[:, 0]] + 0.3 * torch.randn(P, C, generator=g) / C ** 0.5, dim=1)
    return F0.to(dev).requires_grad_(True), F1.to(dev).requires_grad_(True), torch.from_numpy(pairs)


# ---- the reference's formulation with torch ops on the device ----------------------------------------------------------
def _keys(a, b, seed):
    return np.asarray(a, dtype=np.int64) + np.asarray(b, dtype=np.int64) * seed


def _pdist(A, B):
    return torch.sqrt((A.unsqueeze(1) - B.unsqueeze(0)).pow(2).sum(2) + 1e-7)


def torch_contrastive_rand(F0, F1, pairs):
    dev, seed = F0.device, max(len(F0), len(F1))
    pn = pairs.numpy()
    cand = np.floor(np.random.rand(2 * len(pn), 2) * np.array([[len(F0), len(F1)]])).astype(np.int64)
    neg = torch.from_numpy(cand[~np.isin(_keys(cand[:, 0], cand[:, 1], seed), _keys(pn[:, 0], pn[:, 1], seed))]).to(dev)
    pp = pairs.to(dev)
    pos_loss = (F0.index_select(0, pp[:, 0]) - F1.index_select(0, pp[:, 1])).pow(2).sum(1)
    neg_loss = torch.relu(1.4 - ((F0.index_select(0, neg[:, 0]) - F1.index_select(0, neg[:, 1])).pow(2).sum(1) + 1e-4).sqrt()).pow(2)
    return pos_loss.mean() + neg_loss.mean()


def _torch_random_triplets(F0, F1, pn, pos_keys, seed):
    rand_pairs = pn[np.random.choice(len(pn), min(len(pn), NUM_RAND), replace=False)]
    negatives = np.random.choice(len(F1), min(len(F1), NUM_RAND), replace=False)
    mask = ~np.isin(_keys(rand_pairs[:, 0], negatives, seed), pos_keys)
    a, p, n = rand_pairs[mask, 0], rand_pairs[mask, 1], negatives[mask]
    rp = torch.sqrt((F0[a] - F1[p]).pow(2).sum(1) + 1e-7)
    rn = torch.sqrt((F0[a] - F1[n]).pow(2).sum(1) + 1e-7)
    return rp, rn


def torch_triplet(F0, F1, pairs):
    seed, pn = max(len(F0), len(F1)), pairs.numpy()
    sample = pairs[np.random.choice(len(pn), NUM_POS, replace=False)] if len(pn) > NUM_POS else pairs
    pos_dist = torch.sqrt((F0[sample[:, 0]] - F1[sample[:, 1]]).pow(2).sum(1) + 1e-7)
    rp, rn = _torch_random_triplets(F0, F1, pn, _keys(pn[:, 0], pn[:, 1], seed), seed)
    return torch.relu(rp + MARGIN - rn).mean(), pos_dist.mean(), rn.mean()


def torch_hardest_triplet(F0, F1, pairs):
    seed, pn = max(len(F0), len(F1)), pairs.numpy()
    sel0 = np.random.choice(len(F0), min(len(F0), NUM_HN), replace=False)
    sel1 = np.random.choice(len(F1), min(len(F1), NUM_HN), replace=False)
    sample = pairs[np.random.choice(len(pn), NUM_POS, replace=False)] if len(pn) > NUM_POS else pairs
    i0, i1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[i0], F1[i1]
    D01min, D01ind = _pdist(posF0, F1[sel1]).min(1)             # the [num_pos, num_hn, C] broadcast
    D10min, D10ind = _pdist(posF1, F0[sel0]).min(1)
    pos_keys = _keys(pn[:, 0], pn[:, 1], seed)
    n01, n10 = sel1[D01ind.cpu().numpy()], sel0[D10ind.cpu().numpy()]          # the host round trip
    mask0 = torch.from_numpy(~np.isin(_keys(i0.numpy(), n01, seed), pos_keys))
    mask1 = torch.from_numpy(~np.isin(_keys(n10, i1.numpy(), seed), pos_keys))
    pos_dist = torch.sqrt((posF0 - posF1).pow(2).sum(1) + 1e-7)
    rp, rn = _torch_random_triplets(F0, F1, pn, pos_keys, seed)
    loss = torch.relu(torch.cat([rp + MARGIN - rn, pos_dist[mask0] + MARGIN - D01min[mask0],
                                 pos_dist[mask1] + MARGIN - D10min[mask1]])).mean()
    return loss, pos_dist.mean(), (D01min.mean() + D10min.mean()).item() / 2


def call(impl, loss, F0, F1, pairs):
    F0.grad = F1.grad = None
    if impl == "torch":
        out = {"contrastive_rand": torch_contrastive_rand, "triplet": torch_triplet,
               "hardest_triplet": torch_hardest_triplet}[loss](F0, F1, pairs)
    else:
        from gcl_amd.lib import trainer as T
        if loss == "contrastive_rand":
            out = sum(T.contrastive_random_negative_loss(F0, F1, pairs))
        elif loss == "triplet":
            out = T.triplet_loss(F0, F1, pairs, NUM_POS, NUM_HN, NUM_RAND, MARGIN)
        else:
            out = T.hardest_triplet_loss(F0, F1, pairs, NUM_POS, NUM_HN, NUM_RAND, MARGIN)
    (out[0] if isinstance(out, tuple) else out).backward()
    return out


def run(impl, loss, calls, warmup):
    dev = torch.device("cuda:0")
    F0, F1, pairs = inputs(dev)
    np.random.seed(1)
    for _ in range(warmup):
        call(impl, loss, F0, F1, pairs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        out = call(impl, loss, F0, F1, pairs)
    e1.record()
    torch.cuda.synchronize()
    first = out[0] if isinstance(out, tuple) else out
    return e0.elapsed_time(e1) / max(calls, 1), float(first.detach())


def count_launches(impl, loss):
    totals = []
    for calls in (10, 20):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "r", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--child", impl, loss, str(calls)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None
            n = 0
            for f in files:
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        n += int(row.get("Calls") or row.get("calls") or 0)
            totals.append(n)
    return (totals[1] - totals[0]) / 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("IMPL", "LOSS", "CALLS"))
    ap.add_argument("--out")
    ap.add_argument("--no-count", action="store_true")
    a = ap.parse_args()
    if a.child:
        run(a.child[0], a.child[1], int(a.child[2]), 0)
        return
    lines = [f"pair losses, forward + backward, N0 = N1 = {N0} x {C}, P = {P}, num_pos {NUM_POS}, num_hn {NUM_HN}, "
             f"num_rand {NUM_RAND}; {torch.cuda.get_device_name(0)}; 50 timed calls after 10",
             f"{'loss':<18}{'impl':<9}{'ms / call':>10}{'launches / call':>17}{'loss value':>14}"]
    for loss in LOSSES:
        for impl in ("hip", "torch"):
            ms, val = run(impl, loss, 50, 10)
            n = None if a.no_count else count_launches(impl, loss)
            lines.append(f"{loss:<18}{impl:<9}{ms:>10.3f}{('n/a' if n is None else f'{n:.1f}'):>17}{val:>14.6f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
