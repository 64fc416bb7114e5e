"""Generates tests/golden/{triplet,hardest_triplet,contrastive_rand}_*.npz by IMPORTING the reference's own Python.

Run:  python tests/golden/make_pair_golden.py        (needs the reference checkout make_golden.py names; arrays only)

Captured, with np.random seeded and every draw re-drawn in the same order to record it:

* ``TripletLossTrainer.triplet_loss``                       lib/trainer.py:545-592
* ``HardestTripletLossTrainer.triplet_loss``                lib/trainer.py:671-744
* ``ContrastiveLossTrainer.generate_rand_negative_pairs``   lib/trainer.py:198-212; the loss that consumes the pairs is
  inline in ``_train_epoch`` (:260-273) and cannot be called, so its value and gradients are computed here from its
  formula: mean |a - b|^2 over the positives, mean relu(neg_thresh - sqrt(|a - b|^2 + 1e-4))^2 over the returned pairs.

Features are stored as int16 on a 2^-14 grid (``F0_q`` / ``F1_q``, F = q / 16384 exactly in fp32) so that a file with
its gradients stays under 1 MiB; the reference was run on exactly those fp32 values.

The script ASSERTS, and writes nothing otherwise, that (i) nearest and second-nearest candidate of every mined row
differ by >= 5e-6 in distance (fp64), (ii) no hinge argument of a kept term lies within 1e-5 of zero, (iii) across the
set every mask has kept and dropped entries and every hinge active and inactive terms in at least one file, and
(iv) a second run into a temporary directory reproduces every array exactly.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import _import_reference, _unit_rows      # noqa: E402
import pair_loss_oracle as PO                               # noqa: E402

Q = 16384.0

# name: N0, N1, P, num_pos, num_hn, num_rand, margin, dense, planted near-duplicates, seed
CASES = {
    "sub": dict(N0=3000, N1=2800, P=1500, num_pos=256, num_hn=512, num_rand=1024, margin=0.4, dense=False, plant=200, seed=0),
    "all": dict(N0=2000, N1=2500, P=300, num_pos=1024, num_hn=4096, num_rand=256, margin=0.4, dense=False, plant=200, seed=1),
    "dense": dict(N0=96, N1=64, P=1500, num_pos=2048, num_hn=32, num_rand=64, margin=0.4, dense=True, plant=12, seed=2),
    "dense_m14": dict(N0=96, N1=64, P=1500, num_pos=2048, num_hn=32, num_rand=64, margin=1.4, dense=True, plant=12, seed=3),
}


def make_inputs(c):
    k = c["seed"]
    gt = torch.Generator().manual_seed(70 + k)
    rng = np.random.RandomState(70 + k)
    N0, N1, P = c["N0"], c["N1"], c["P"]
    F0, F1 = _unit_rows(gt, N0, 32), _unit_rows(gt, N1, 32)
    if c["dense"]:      # P distinct (i, j) of the N0 x N1 grid: every row has many partners
        flat = np.sort(rng.choice(N0 * N1, P, replace=False))
        pairs = np.stack([flat // N1, flat % N1], 1).astype(np.int64)
        first = np.unique(pairs[:, 1], return_index=True)[1]          # one partner per row of cloud 1 gives it its feature
        F1[pairs[first, 1]] = F0[pairs[first, 0]] + 0.3 * torch.randn(len(first), 32, generator=gt)
    else:               # unique-row pairs
        pairs = np.stack([rng.choice(N0, P, replace=False), rng.choice(N1, P, replace=False)], 1).astype(np.int64)
        F1[pairs[:, 1]] = F0[pairs[:, 0]] + 0.3 * torch.randn(P, 32, generator=gt)
    n = c["plant"]      # hard negatives: near-duplicates planted WITHOUT replacement
    F1[rng.choice(N1, n, replace=False)] = F0[rng.choice(N0, n, replace=False)] + 0.05 * torch.randn(n, 32, generator=gt)
    F1 = F1 / F1.norm(dim=1, keepdim=True)
    q0, q1 = torch.round(F0 * Q).to(torch.int16), torch.round(F1 * Q).to(torch.int16)
    return q0.numpy(), q1.numpy(), pairs


def features(q):
    return (torch.from_numpy(q).float() / Q).clone().requires_grad_(True)


def both(x):
    x = np.asarray(x).astype(bool)
    return bool(x.any() and (~x).any())


def generate(out_dir, classes):
    Contrastive, Triplet, HardestTriplet = classes
    seen = {k: False for k in ("rand_mask", "mask0", "mask1", "cand_mask", "rand_hinge", "mined_hinge", "neg_hinge")}
    for name, c in CASES.items():
        q0, q1, pairs = make_inputs(c)
        N0, N1, P = c["N0"], c["N1"], c["P"]
        np_seed = 300 + c["seed"]
        sizes = dict(num_pos=c["num_pos"], num_hn=c["num_hn"], num_rand=c["num_rand"], margin=c["margin"], np_seed=np_seed,
                     F_scale=Q)
        D0, D1 = (torch.from_numpy(q).double() / Q for q in (q0, q1))

        # ---- TripletLossTrainer.triplet_loss ---------------------------------------------------------------------------
        F0, F1 = features(q0), features(q1)
        tr = Triplet.__new__(Triplet)
        tr.neg_thresh = c["margin"]
        np.random.seed(np_seed)
        loss, pos_dist, neg_dist = tr.triplet_loss(F0, F1, torch.from_numpy(pairs), num_pos=c["num_pos"],
                                                   num_hn_samples=c["num_hn"], num_rand_triplet=c["num_rand"])
        loss.backward()
        np.random.seed(np_seed)
        pos_sel = np.random.choice(P, c["num_pos"], replace=False) if P > c["num_pos"] else None
        rand_inds = np.random.choice(P, min(P, c["num_rand"]), replace=False)
        negatives = np.random.choice(N1, min(N1, c["num_rand"]), replace=False)
        o_loss, o_pos, o_neg, rand_mask = PO.triplet(D0, D1, pairs, (pos_sel, rand_inds, negatives), c["margin"])
        assert abs(float(o_loss) - loss.item()) < 1e-5, "the recorded draws are not the ones the reference made"
        rp = pairs[rand_inds]
        arg = PO.hinge_arguments(D0, D1, rp[rand_mask], negatives[rand_mask], np.zeros(int(rand_mask.sum())), c["margin"])
        assert float(arg.abs().min()) >= 1e-5, (name, "random hinge argument too close to zero", float(arg.abs().min()))
        seen["rand_mask"] |= both(rand_mask)
        seen["rand_hinge"] |= both(arg.numpy() > 0)
        np.savez_compressed(os.path.join(out_dir, f"triplet_{name}.npz"), F0_q=q0, F1_q=q1, pairs=pairs,
                            pos_sel=pos_sel if pos_sel is not None else np.zeros(0, np.int64), subsampled=pos_sel is not None,
                            rand_inds=rand_inds, negatives=negatives, rand_mask=rand_mask, loss=loss.item(),
                            pos_dist=float(pos_dist.detach()), neg_dist=float(neg_dist.detach()), grad0=F0.grad.numpy(),
                            grad1=F1.grad.numpy(), **sizes)
        print("triplet", name, loss.item(), pos_dist.item(), neg_dist.item(), int(rand_mask.sum()), len(rand_mask),
              int((arg > 0).sum()), int((arg <= 0).sum()))

        # ---- HardestTripletLossTrainer.triplet_loss --------------------------------------------------------------------
        F0, F1 = features(q0), features(q1)
        tr = HardestTriplet.__new__(HardestTriplet)
        tr.neg_thresh = c["margin"]
        np.random.seed(np_seed)
        loss, pos_dist, neg_dist = tr.triplet_loss(F0, F1, torch.from_numpy(pairs), num_pos=c["num_pos"],
                                                   num_hn_samples=c["num_hn"], num_rand_triplet=c["num_rand"])
        loss.backward()
        np.random.seed(np_seed)
        sel0 = np.random.choice(N0, min(N0, c["num_hn"]), replace=False)
        sel1 = np.random.choice(N1, min(N1, c["num_hn"]), replace=False)
        pos_sel = np.random.choice(P, c["num_pos"], replace=False) if P > c["num_pos"] else None
        rand_inds = np.random.choice(P, min(P, c["num_rand"]), replace=False)
        negatives = np.random.choice(N1, min(N1, c["num_rand"]), replace=False)
        o = PO.hardest_triplet(D0, D1, pairs, (sel0, sel1, pos_sel, rand_inds, negatives), c["margin"])
        assert abs(float(o["loss"]) - loss.item()) < 1e-5, "the recorded draws are not the ones the reference made"
        assert o["gap"] >= 5e-6, (name, "mined nearest / second-nearest too close", o["gap"])
        sample = pairs if pos_sel is None else pairs[pos_sel]
        ns = len(sample)
        arg0 = PO.hinge_arguments(D0, D1, sample, o["neg01"], np.zeros(ns), c["margin"])[torch.from_numpy(o["mask0"])]
        arg1 = PO.hinge_arguments(D0, D1, sample, o["neg10"], np.ones(ns), c["margin"])[torch.from_numpy(o["mask1"])]
        mined = torch.cat([arg0, arg1])
        assert float(mined.abs().min()) >= 1e-5, (name, "mined hinge argument too close to zero", float(mined.abs().min()))
        seen["mask0"] |= both(o["mask0"])
        seen["mask1"] |= both(o["mask1"])
        seen["mined_hinge"] |= both(mined.numpy() > 0)
        np.savez_compressed(os.path.join(out_dir, f"hardest_triplet_{name}.npz"), F0_q=q0, F1_q=q1, pairs=pairs, sel0=sel0,
                            sel1=sel1, pos_sel=pos_sel if pos_sel is not None else np.zeros(0, np.int64),
                            subsampled=pos_sel is not None, rand_inds=rand_inds, negatives=negatives,
                            rand_mask=o["rand_mask"], mask0=o["mask0"], mask1=o["mask1"], neg01=o["neg01"], neg10=o["neg10"],
                            loss=loss.item(), pos_dist=pos_dist.item(), neg_dist=float(neg_dist), grad0=F0.grad.numpy(),
                            grad1=F1.grad.numpy(), gap=o["gap"], **sizes)
        print("hardest_triplet", name, loss.item(), pos_dist.item(), float(neg_dist), "masks",
              int(o["mask0"].sum()), int((~o["mask0"]).sum()), int(o["mask1"].sum()), int((~o["mask1"]).sum()),
              "mined hinge", int((mined > 0).sum()), int((mined <= 0).sum()), "gap", o["gap"])

        # ---- ContrastiveLossTrainer: generate_rand_negative_pairs + the inline loss --------------------------------------
        if name.endswith("_m14"):
            continue
        F0, F1 = features(q0), features(q1)
        tr = Contrastive.__new__(Contrastive)
        np.random.seed(np_seed)
        neg_pairs = tr.generate_rand_negative_pairs(torch.from_numpy(pairs), max(N0, N1), N0, N1)
        np.random.seed(np_seed)
        cand = np.floor(np.random.rand(2 * P, 2) * np.array([[N0, N1]])).astype(np.int64)
        keep = PO.keep_mask(cand[:, 0], cand[:, 1], pairs, max(N0, N1))
        assert np.array_equal(cand[keep], neg_pairs), "the recorded candidates are not the ones the reference drew"
        neg_thresh = 1.4
        np_ = torch.from_numpy(neg_pairs)
        pos_loss = (F0[torch.from_numpy(pairs[:, 0])] - F1[torch.from_numpy(pairs[:, 1])]).pow(2).sum(1).mean()
        D = ((F0[np_[:, 0]] - F1[np_[:, 1]]).pow(2).sum(1) + 1e-4).sqrt()
        neg_loss = torch.relu(neg_thresh - D).pow(2).mean()
        (pos_loss + neg_loss).backward()
        harg = (neg_thresh - D).detach()
        assert float(harg.abs().min()) >= 1e-5, (name, "negative hinge argument too close to zero", float(harg.abs().min()))
        seen["cand_mask"] |= both(keep)
        seen["neg_hinge"] |= both(harg.numpy() > 0)
        np.savez_compressed(os.path.join(out_dir, f"contrastive_rand_{name}.npz"), F0_q=q0, F1_q=q1, pairs=pairs,
                            candidates=cand, keep=keep, neg_pairs=neg_pairs, neg_thresh=neg_thresh, pos=pos_loss.item(),
                            neg=neg_loss.item(), grad0=F0.grad.numpy(), grad1=F1.grad.numpy(), np_seed=np_seed, F_scale=Q)
        print("contrastive_rand", name, pos_loss.item(), neg_loss.item(), int(keep.sum()), int((~keep).sum()),
              int((harg > 0).sum()), int((harg <= 0).sum()))
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"no file of the set has both outcomes for: {missing}"


def main():
    _import_reference()
    from lib.trainer import ContrastiveLossTrainer, TripletLossTrainer, HardestTripletLossTrainer
    classes = (ContrastiveLossTrainer, TripletLossTrainer, HardestTripletLossTrainer)
    torch.set_num_threads(1)          # scatter-adds of a backward pass in one fixed order: (iv) needs exact reruns
    with tempfile.TemporaryDirectory() as first, tempfile.TemporaryDirectory() as second:
        generate(first, classes)
        generate(second, classes)
        names = sorted(os.listdir(first))
        assert names == sorted(os.listdir(second))
        for n in names:
            a, b = np.load(os.path.join(first, n)), np.load(os.path.join(second, n))
            assert a.files == b.files and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a.files), \
                f"{n}: a second run does not reproduce the arrays"
        for n in names:       # every assertion held: publish
            with open(os.path.join(first, n), "rb") as src, open(os.path.join(HERE, n), "wb") as dst:
                dst.write(src.read())
            print("wrote", n, os.path.getsize(os.path.join(HERE, n)))


if __name__ == "__main__":
    main()
