"""FCGF baseline loss on the MI355X kernels (interface of lib/trainer.py:408-462).

``contrastive_hardest_negative_loss``: positive pairs pulled together, and for each positive the hardest negative among
a random subset of the other cloud pushed apart.  The two [num_pos, num_hn] distance matrices are never formed: the
row minimum / arg-minimum come from ``gcl_nn_rowmin`` (one launch each); the selected distances are then re-evaluated
with differentiable torch ops on [num_pos, C] slices, and the positional-hash membership test
(``np.isin(_hash(...), pos_keys)``, :447-456) runs on the device.

The rest of the pair family sits below it: ``contrastive_random_negative_loss`` (:198-273), ``triplet_loss`` (:545-592),
``hardest_triplet_loss`` (:671-744) on the kernels of csrc/pairloss.hip, and the four trainers a reference user selects
with ``--trainer``: ``ContrastiveLossTrainer``, ``HardestContrastiveLossTrainer``, ``TripletLossTrainer``,
``HardestTripletLossTrainer``.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F_
from torch.autograd.function import once_differentiable

from gcl_amd import _lib
from gcl_amd.lib import ordered
from gcl_amd.lib.metrics import pdist_min


def draw_hardest_selections(N0, N1, n_pos_pairs, num_pos, num_hn_samples):
    """The reference's three np.random draws in its order (lib/trainer.py:424-431)."""
    sel0 = np.random.choice(N0, min(N0, num_hn_samples), replace=False)
    sel1 = np.random.choice(N1, min(N1, num_hn_samples), replace=False)
    pos_sel = np.random.choice(n_pos_pairs, num_pos, replace=False) if n_pos_pairs > num_pos else None
    return sel0, sel1, pos_sel


def contrastive_hardest_negative_loss(F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048, pos_thresh=0.1,
                                      neg_thresh=1.4, draws=None, deterministic_loss_backward=False):
    """Returns (pos_loss, neg_loss) like HardestContrastiveLossTrainer.contrastive_hardest_negative_loss
    (``self.pos_thresh`` / ``self.neg_thresh`` become arguments).  F0 [N0, C], F1 [N1, C] on the GPU; positive_pairs
    int [P, 2].  ``draws = (sel0, sel1, pos_sel or None)`` replays recorded selections.
    ``deterministic_loss_backward``: the three terms come from the pair-term kernels (GCL_PAIR_SQ_POS over the sampled
    positives, GCL_PAIR_NEG with eps 1e-7 over the mined pairs of either direction, the membership test a hash-table
    probe) with the ordered backward, instead of torch's gather / index_put_ (float atomics in its backward pass)."""
    if deterministic_loss_backward:
        return _hardest_contrastive_on_kernels(F0, F1, positive_pairs, num_pos, num_hn_samples, pos_thresh, neg_thresh, draws)
    dev = F0.device
    N0, N1 = len(F0), len(F1)
    pairs = torch.as_tensor(np.asarray(positive_pairs) if not torch.is_tensor(positive_pairs) else positive_pairs)
    pairs = pairs.to(torch.int64)
    if draws is None:
        draws = draw_hardest_selections(N0, N1, len(pairs), num_pos, num_hn_samples)
    sel0, sel1, pos_sel = draws
    hash_seed = max(N0, N1)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev, non_blocking=True)
    sel0, sel1 = to_dev(sel0), to_dev(sel1)
    pairs = pairs.to(dev, non_blocking=True)
    sample = pairs if pos_sel is None else pairs[to_dev(pos_sel)]
    ind0, ind1 = sample[:, 0].contiguous(), sample[:, 1].contiguous()
    # hardest negative of every positive among the sampled rows of the other cloud (:441-445)
    _, a01 = pdist_min(F0, F1, "L2", rows_a=ind0, rows_b=sel1)
    _, a10 = pdist_min(F1, F0, "L2", rows_a=ind1, rows_b=sel0)
    n01, n10 = sel1[a01.long()], sel0[a10.long()]
    posF0, posF1 = F0[ind0], F1[ind1]
    D01min = torch.sqrt((posF0 - F1[n01]).pow(2).sum(1) + 1e-7)
    D10min = torch.sqrt((posF1 - F0[n10]).pow(2).sum(1) + 1e-7)
    # positional hash i0 + i1 * hash_seed (util/misc.py:43-55) and the membership test (:447-456)
    pos_keys = pairs[:, 0] + pairs[:, 1] * hash_seed
    mask0 = torch.logical_not(torch.isin(ind0 + n01 * hash_seed, pos_keys))
    mask1 = torch.logical_not(torch.isin(n10 + ind1 * hash_seed, pos_keys))
    pos_loss = F_.relu((posF0 - posF1).pow(2).sum(1) - pos_thresh)
    neg_loss0 = F_.relu(neg_thresh - D01min[mask0]).pow(2)
    neg_loss1 = F_.relu(neg_thresh - D10min[mask1]).pow(2)
    return pos_loss.mean(), (neg_loss0.mean() + neg_loss1.mean()) / 2


def _hardest_contrastive_on_kernels(F0, F1, positive_pairs, num_pos, num_hn_samples, pos_thresh, neg_thresh, draws):
    """contrastive_hardest_negative_loss on gcl_pair_terms_fwd / _bwd_emit: the same three means (lib/trainer.py:441-462)."""
    _require_gpu_features(F0, F1)
    dev = F0.device
    N0, N1 = len(F0), len(F1)
    pairs_d = _pairs_on_device(positive_pairs, dev)
    if draws is None:
        draws = draw_hardest_selections(N0, N1, len(pairs_d), num_pos, num_hn_samples)
    sel0, sel1, pos_sel = draws
    seed = max(N0, N1)
    with torch.cuda.device(dev):
        parts = _upload([sel0, sel1] + ([pos_sel] if pos_sel is not None else []), dev)
        sel0_d, sel1_d = parts[0], parts[1]
        sample = pairs_d if pos_sel is None else pairs_d.index_select(0, parts[2])
        ns = int(sample.shape[0])
        ind0, ind1 = sample[:, 0].contiguous(), sample[:, 1].contiguous()
        _, a01 = pdist_min(F0, F1, "L2", rows_a=ind0, rows_b=sel1_d)
        _, a10 = pdist_min(F1, F0, "L2", rows_a=ind1, rows_b=sel0_d)
        table, cap = _key_table(pairs_d, seed)
        n01 = torch.empty(ns, dtype=torch.int64, device=dev)
        n10 = torch.empty(ns, dtype=torch.int64, device=dev)
        mask0 = _key_mask(table, cap, seed, sample, 0, b=sel1_d, b_arg=a01, b_out=n01)       # key (ind0, sel1[a01])
        mask1 = _key_mask(table, cap, seed, sample, 1, b=sel0_d, b_arg=a10, b_out=n10)       # key (sel0[a10], ind1)
        pos = _PairTermsFn.apply(F0, F1, sample, None, _lib.PAIR_SQ_POS, float(pos_thresh), 0.0, True)
        neg0 = _PairTermsFn.apply(F0, F1, torch.stack([ind0, n01], 1), mask0, _lib.PAIR_NEG, float(neg_thresh), 1e-7, True)
        neg1 = _PairTermsFn.apply(F0, F1, torch.stack([n10, ind1], 1), mask1, _lib.PAIR_NEG, float(neg_thresh), 1e-7, True)
    return pos, (neg0 + neg1) / 2


def _reduce_pair_records(recs, dF0, dF1):
    """The two record lists of a pair-family emit entry (one per cloud) into dF0 and dF1."""
    (row0, val0), (row1, val1) = recs
    ordered.ordered_row_sum(row0, val0, dF0)
    ordered.ordered_row_sum(row1, val1, dF1)


# ---- the rest of the pair family on the HIP kernels of csrc/pairloss.hip ---------------------------------------------
# lib/trainer.py: ContrastiveLossTrainer :198-276, TripletLossTrainer :545-592, HardestTripletLossTrainer :671-744 (the same
# bodies exist a second time in lib/colocation_trainer.py:177-304, :919-1120).  The np.random draws stay on the host in
# the reference's order; everything behind them runs on the device without the host being waited for: the positional-
# hash membership test is a hash-table probe (gcl_pair_key_table / gcl_pair_key_mask), every loss term one launch and
# its mean one more (gcl_triplet_fwd / gcl_pair_terms_fwd), the backward pass one launch of float atomics.
def _require_gpu_features(F0, F1):
    if not (F0.is_cuda and F1.is_cuda):
        raise RuntimeError("gcl_amd operators take GPU tensors only (no CPU path)")
    _lib.require_gpu()


def _pairs_on_device(positive_pairs, dev):
    t = positive_pairs if torch.is_tensor(positive_pairs) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(positive_pairs), dtype=np.int64))
    return t.to(torch.int64).reshape(-1, 2).to(dev, non_blocking=True).contiguous()


def _upload(parts, dev, tags=None):
    """Host int64 arrays (and one uint8 array, ``tags``) in ONE host -> device copy; returns the device views."""
    parts = [np.ascontiguousarray(p, dtype=np.int64).reshape(-1) for p in parts]
    lens = [len(p) for p in parts]
    if tags is not None:
        tags = np.ascontiguousarray(tags, dtype=np.uint8)
        padded = np.zeros((len(tags) + 7) // 8 * 8, dtype=np.uint8)
        padded[:len(tags)] = tags
        parts = parts + [padded.view(np.int64)]
    d = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.int64)).to(dev, non_blocking=True)
    out, off = [], 0
    for n in lens:
        out.append(d[off:off + n])
        off += n
    if tags is not None:
        out.append(d[off:].view(torch.uint8)[:len(tags)])
    return out


def _key_table(pairs_d, seed):
    """Hash table of the positive pairs' keys i0 + i1 * seed (util/misc.py:43-55): (table, cap)."""
    lib = _lib.require_gpu()
    n_pos = int(pairs_d.shape[0])
    cap = 64
    while cap < 2 * n_pos:
        cap *= 2
    table = torch.empty((cap, 2), dtype=torch.int64, device=pairs_d.device)
    _lib.check(lib.gcl_pair_key_table(_lib.ptr(pairs_d, torch.int64) if n_pos else None, n_pos, int(seed),
                                      _lib.ptr(table), cap, _lib.stream()), "gcl_pair_key_table")
    return table, cap


def _key_mask(table, cap, seed, ap, col=0, b=None, b_arg=None, b_out=None, keep=None):
    """keep[t] = candidate t is no positive pair (see gcl_pair_key_mask in include/gcl_amd.h)."""
    lib = _lib.require_gpu()
    m = int(ap.shape[0])
    if keep is None:
        keep = torch.empty(m, dtype=torch.uint8, device=ap.device)
    _lib.check(lib.gcl_pair_key_mask(_lib.ptr(ap, torch.int64), int(col), _lib.ptr(b, torch.int64),
                                     _lib.ptr(b_arg, torch.int32), 0 if b is None else int(b.shape[0]), m, int(seed),
                                     _lib.ptr(table), cap, _lib.ptr(b_out, torch.int64), _lib.ptr(keep, torch.uint8),
                                     _lib.stream()), "gcl_pair_key_mask")
    return keep


class _TripletFn(torch.autograd.Function):
    """(mean hinge over the kept triplets, the GCL_TRIPLET_OUT statistics) of gcl_triplet_fwd; only the mean carries a
    gradient."""

    @staticmethod
    def forward(ctx, F0, F1, ap, neg, tag, keep, margin, deterministic=False):
        lib = _lib.require_gpu()
        ctx.deterministic = bool(deterministic)
        F0, F1 = F0.contiguous(), F1.contiguous()
        m, c = int(ap.shape[0]), int(F0.shape[1])
        if F1.shape[1] != c:
            raise ValueError("F0 and F1 differ in feature width")
        work = torch.empty(int(lib.gcl_triplet_scratch_len(m)), dtype=torch.float32, device=F0.device)
        out = torch.empty(_lib.TRIPLET_OUT, dtype=torch.float32, device=F0.device)
        _lib.check(lib.gcl_triplet_fwd(_lib.ptr(F0, torch.float32), F0.shape[0], _lib.ptr(F1, torch.float32), F1.shape[0], c,
                                       _lib.ptr(ap, torch.int64), _lib.ptr(neg, torch.int64), _lib.ptr(tag, torch.uint8),
                                       _lib.ptr(keep, torch.uint8), m, float(margin), _lib.ptr(work) if m else None,
                                       _lib.ptr(out), _lib.stream()), "gcl_triplet_fwd")
        ctx.save_for_backward(F0, F1, ap, neg, tag, keep, work, out)
        loss, stats = out[0], out.clone()
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _gstats):
        lib = _lib.load()
        F0, F1, ap, neg, tag, keep, work, out = ctx.saved_tensors
        dF0, dF1 = torch.zeros_like(F0), torch.zeros_like(F1)
        g = gloss.reshape(1).contiguous().float()
        m = int(ap.shape[0])
        if m and ctx.deterministic:
            c, n_rec = int(F0.shape[1]), int(lib.gcl_triplet_records(m))
            recs = (ordered.records(n_rec, c, F0.device), ordered.records(n_rec, c, F0.device))
            _lib.check(lib.gcl_triplet_bwd_emit(_lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], c, _lib.ptr(ap),
                                                _lib.ptr(neg), _lib.ptr(tag), _lib.ptr(keep), m, _lib.ptr(work), _lib.ptr(out),
                                                _lib.ptr(g), _lib.ptr(recs[0][0]), _lib.ptr(recs[0][1]), _lib.ptr(recs[1][0]),
                                                _lib.ptr(recs[1][1]), n_rec, _lib.stream()), "gcl_triplet_bwd_emit")
            _reduce_pair_records(recs, dF0, dF1)
        elif m:
            _lib.check(lib.gcl_triplet_bwd(_lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], F0.shape[1], _lib.ptr(ap),
                                           _lib.ptr(neg), _lib.ptr(tag), _lib.ptr(keep), m, _lib.ptr(work), _lib.ptr(out),
                                           _lib.ptr(g), _lib.ptr(dF0), _lib.ptr(dF1), _lib.stream()), "gcl_triplet_bwd")
        return dF0, dF1, None, None, None, None, None, None


class _PairTermsFn(torch.autograd.Function):
    """Mean over the kept pairs of one of the GCL_PAIR_* terms (gcl_pair_terms_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, F0, F1, pairs, keep, mode, thresh, eps, deterministic=False):
        lib = _lib.require_gpu()
        ctx.deterministic = bool(deterministic)
        F0, F1 = F0.contiguous(), F1.contiguous()
        m, c = int(pairs.shape[0]), int(F0.shape[1])
        if F1.shape[1] != c:
            raise ValueError("F0 and F1 differ in feature width")
        work = torch.empty(int(lib.gcl_pair_terms_scratch_len(m)), dtype=torch.float32, device=F0.device)
        out = torch.empty(2, dtype=torch.float32, device=F0.device)
        _lib.check(lib.gcl_pair_terms_fwd(_lib.ptr(F0, torch.float32), F0.shape[0], _lib.ptr(F1, torch.float32), F1.shape[0],
                                          c, _lib.ptr(pairs, torch.int64) if m else None, _lib.ptr(keep, torch.uint8), m,
                                          int(mode), float(thresh), float(eps), _lib.ptr(work) if m else None,
                                          _lib.ptr(out), _lib.stream()), "gcl_pair_terms_fwd")
        ctx.save_for_backward(F0, F1, pairs, keep, work, out)
        ctx.cfg = (int(mode), float(thresh), float(eps))
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean):
        lib = _lib.load()
        F0, F1, pairs, keep, work, out = ctx.saved_tensors
        mode, thresh, eps = ctx.cfg
        dF0, dF1 = torch.zeros_like(F0), torch.zeros_like(F1)
        g = gmean.reshape(1).contiguous().float()
        m = int(pairs.shape[0])
        if m and ctx.deterministic:
            c, n_rec = int(F0.shape[1]), int(lib.gcl_pair_terms_records(m))
            recs = (ordered.records(n_rec, c, F0.device), ordered.records(n_rec, c, F0.device))
            _lib.check(lib.gcl_pair_terms_bwd_emit(_lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], c, _lib.ptr(pairs),
                                                   _lib.ptr(keep), m, mode, thresh, eps, _lib.ptr(work), _lib.ptr(out),
                                                   _lib.ptr(g), _lib.ptr(recs[0][0]), _lib.ptr(recs[0][1]),
                                                   _lib.ptr(recs[1][0]), _lib.ptr(recs[1][1]), n_rec, _lib.stream()),
                       "gcl_pair_terms_bwd_emit")
            _reduce_pair_records(recs, dF0, dF1)
        elif m:
            _lib.check(lib.gcl_pair_terms_bwd(_lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], F0.shape[1],
                                              _lib.ptr(pairs), _lib.ptr(keep), m, mode, thresh, eps, _lib.ptr(work),
                                              _lib.ptr(out), _lib.ptr(g), _lib.ptr(dF0), _lib.ptr(dF1), _lib.stream()),
                       "gcl_pair_terms_bwd")
        return dF0, dF1, None, None, None, None, None, None


def _mean_pair_distance(F0, F1, pairs_d):
    """mean of sqrt(|F0[a] - F1[b]|^2 + 1e-7) over the pairs: a statistic, detached (lib/trainer.py:573, :592)."""
    with torch.no_grad():
        return _PairTermsFn.apply(F0.detach(), F1.detach(), pairs_d, None, _lib.PAIR_DIST, 0.0, 1e-7)


# ---- ContrastiveLossTrainer: random negative pairs ---------------------------------------------------------------------
def draw_rand_negative_pairs(n_pos_pairs, N0, N1, N_neg=0):
    """The one np.random draw of generate_rand_negative_pairs (lib/trainer.py:204-209): int64 [N_neg, 2] candidate pairs,
    N_neg = 2 * #positive pairs unless given."""
    if N_neg < 1:
        N_neg = n_pos_pairs * 2
    return np.floor(np.random.rand(int(N_neg), 2) * np.array([[N0, N1]])).astype(np.int64)


def generate_rand_negative_pairs(positive_pairs, hash_seed, N0, N1, N_neg=0, draws=None, device=None):
    """lib/trainer.py:198-212 with the membership test on the device.  Returns ``(candidates, keep)``: the drawn pairs
    int64 [N_neg, 2] and uint8 [N_neg] (1 = no positive pair) as device tensors -- the reference's return value is
    ``candidates[keep]``; compacting it would need the number of kept pairs on the host, so the mask travels with the
    candidates instead and nothing here copies to the host or synchronises.  ``draws``: recorded candidates
    (``draw_rand_negative_pairs``)."""
    dev = torch.device(device) if device is not None else (
        positive_pairs.device if torch.is_tensor(positive_pairs) and positive_pairs.is_cuda else torch.device("cuda"))
    with torch.cuda.device(dev):
        pairs_d = _pairs_on_device(positive_pairs, dev)
        if draws is None:
            draws = draw_rand_negative_pairs(len(pairs_d), N0, N1, N_neg)
        cand = _upload([np.asarray(draws, dtype=np.int64)], dev)[0].view(-1, 2)
        table, cap = _key_table(pairs_d, hash_seed)
        return cand, _key_mask(table, cap, hash_seed, cand)


def contrastive_random_negative_loss(F0, F1, positive_pairs, neg_thresh=1.4, draws=None, deterministic_loss_backward=False):
    """``(pos_loss_mean, neg_loss_mean)`` of ContrastiveLossTrainer's step (lib/trainer.py:253-273, without ``/ iter_size``):
    mean |F0[i] - F1[j]|^2 over ALL positive pairs, and mean relu(neg_thresh - sqrt(|F0[a] - F1[b]|^2 + 1e-4))^2 over the
    random pairs that are no positive pair.  ``draws``: recorded candidates (``draw_rand_negative_pairs``).  No copy to the
    host, no synchronisation."""
    _require_gpu_features(F0, F1)
    dev = F0.device
    N0, N1 = len(F0), len(F1)
    pairs_d = _pairs_on_device(positive_pairs, dev)
    cand, keep = generate_rand_negative_pairs(pairs_d, max(N0, N1), N0, N1, draws=draws, device=dev)
    det = bool(deterministic_loss_backward)
    pos = _PairTermsFn.apply(F0, F1, pairs_d, None, _lib.PAIR_SQ, 0.0, 0.0, det)
    neg = _PairTermsFn.apply(F0, F1, cand, keep, _lib.PAIR_NEG, float(neg_thresh), 1e-4, det)
    return pos, neg


# ---- TripletLossTrainer / HardestTripletLossTrainer ------------------------------------------------------------------------
def _check_rand_triplet_counts(n_pos_pairs, N1, num_rand_triplet):
    if min(n_pos_pairs, num_rand_triplet) != min(N1, num_rand_triplet):
        raise ValueError(
            f"triplet_loss pairs min(#positive pairs, num_rand_triplet) = {min(n_pos_pairs, num_rand_triplet)} random "
            f"anchors with min(N1, num_rand_triplet) = {min(N1, num_rand_triplet)} random negatives one to one: the two "
            "counts must be equal (the reference fails with a numpy broadcast error here, lib/trainer.py:576-582)")


def draw_triplet_selections(N1, n_pos_pairs, num_pos, num_rand_triplet):
    """The np.random draws of TripletLossTrainer.triplet_loss in its order (lib/trainer.py:559-579):
    ``(pos_sel or None, rand_inds, negatives)``."""
    pos_sel = np.random.choice(n_pos_pairs, num_pos, replace=False) if n_pos_pairs > num_pos else None
    rand_inds = np.random.choice(n_pos_pairs, min(n_pos_pairs, num_rand_triplet), replace=False)
    negatives = np.random.choice(N1, min(N1, num_rand_triplet), replace=False)
    return pos_sel, rand_inds, negatives


def draw_hardest_triplet_selections(N0, N1, n_pos_pairs, num_pos, num_hn_samples, num_rand_triplet):
    """The np.random draws of HardestTripletLossTrainer.triplet_loss in its order (lib/trainer.py:684-726):
    ``(sel0, sel1, pos_sel or None, rand_inds, negatives)``."""
    sel0, sel1, pos_sel = draw_hardest_selections(N0, N1, n_pos_pairs, num_pos, num_hn_samples)
    rand_inds = np.random.choice(n_pos_pairs, min(n_pos_pairs, num_rand_triplet), replace=False)
    negatives = np.random.choice(N1, min(N1, num_rand_triplet), replace=False)
    return sel0, sel1, pos_sel, rand_inds, negatives


def triplet_loss(F0, F1, positive_pairs, num_pos=1024, num_hn_samples=None, num_rand_triplet=1024, neg_thresh=1.4,
                 draws=None, details=None, deterministic_loss_backward=False):
    """``(loss, pos_dist.mean(), rand_neg_dist.mean())`` of TripletLossTrainer.triplet_loss (lib/trainer.py:545-592;
    ``self.neg_thresh``, the margin, becomes an argument; ``num_hn_samples`` is unused, as there).  Random triplets
    (anchor F0[i], positive F1[j] of a drawn positive pair, a drawn row of F1 as negative), those whose (anchor, negative)
    is itself a positive pair removed; loss = mean relu(d_pos + margin - d_neg).  ``draws = (pos_sel or None, rand_inds,
    negatives)`` replays recorded selections (``draw_triplet_selections``).  The second and third value are detached
    device scalars; nothing here copies to the host or synchronises.  ``details``: a dict that receives the device
    tensors ``rand_mask`` (uint8)."""
    dev = F0.device
    N0, N1 = len(F0), len(F1)
    pairs_d = _pairs_on_device(positive_pairs, dev)
    n_pairs = len(pairs_d)
    _check_rand_triplet_counts(n_pairs, N1, num_rand_triplet)
    _require_gpu_features(F0, F1)
    if draws is None:
        draws = draw_triplet_selections(N1, n_pairs, num_pos, num_rand_triplet)
    pos_sel, rand_inds, negatives = draws
    seed = max(N0, N1)
    nr = len(rand_inds)
    with torch.cuda.device(dev):
        parts = _upload([rand_inds, negatives] + ([pos_sel] if pos_sel is not None else []), dev,
                        tags=np.zeros(nr, np.uint8))
        rand_d, neg_d, tag_d = parts[0], parts[1], parts[-1]
        rand_ap = pairs_d.index_select(0, rand_d)
        table, cap = _key_table(pairs_d, seed)
        keep = _key_mask(table, cap, seed, rand_ap, 0, b=neg_d)
        loss, stats = _TripletFn.apply(F0, F1, rand_ap, neg_d, tag_d, keep, float(neg_thresh),
                                       bool(deterministic_loss_backward))
        sample = pairs_d if pos_sel is None else pairs_d.index_select(0, parts[2])
        pos_dist = _mean_pair_distance(F0, F1, sample)
    if details is not None:
        details.update(rand_mask=keep)
    return loss, pos_dist, stats[5]


def hardest_triplet_loss(F0, F1, positive_pairs, num_pos=1024, num_hn_samples=512, num_rand_triplet=1024,
                         neg_thresh=1.4, draws=None, details=None, deterministic_loss_backward=False):
    """``(loss, pos_dist.mean(), (D01min.mean() + D10min.mean()) / 2)`` of HardestTripletLossTrainer.triplet_loss
    (lib/trainer.py:671-744).  The random triplets of ``triplet_loss`` plus, for every sampled positive pair (i, j), the
    hardest negative of F0[i] among ``num_hn_samples`` drawn rows of F1 and of F1[j] among as many rows of F0
    (``gcl_nn_rowmin``: the two [num_pos, num_hn] distance matrices are never formed), each dropped where (anchor,
    negative) is itself a positive pair; loss = mean hinge over the concatenation of the three sets.  The D01min / D10min
    means are over all sampled positives, before the mask, as in the reference.  ``draws = (sel0, sel1, pos_sel or None,
    rand_inds, negatives)`` (``draw_hardest_triplet_selections``).  The second and third value are detached device
    scalars; nothing here copies to the host or synchronises (the reference's ``.cpu()`` of the arg-minima and ``.item()``
    of the statistic are what this removes).  ``details``: a dict that receives the device tensors ``rand_mask``,
    ``mask0``, ``mask1`` (uint8) and ``neg01``, ``neg10`` (the mined rows of F1 / F0)."""
    dev = F0.device
    N0, N1 = len(F0), len(F1)
    pairs_d = _pairs_on_device(positive_pairs, dev)
    n_pairs = len(pairs_d)
    _check_rand_triplet_counts(n_pairs, N1, num_rand_triplet)
    _require_gpu_features(F0, F1)
    if draws is None:
        draws = draw_hardest_triplet_selections(N0, N1, n_pairs, num_pos, num_hn_samples, num_rand_triplet)
    sel0, sel1, pos_sel, rand_inds, negatives = draws
    seed = max(N0, N1)
    pos_idx = np.arange(n_pairs, dtype=np.int64) if pos_sel is None else np.asarray(pos_sel, dtype=np.int64)
    nr, ns = len(rand_inds), len(pos_idx)
    m = nr + 2 * ns
    # the concatenated triplet table (lib/trainer.py:737-742): set 0 random, set 1 mined 0 -> 1, set 2 mined 1 -> 0 (side 1)
    tags = np.concatenate([np.zeros(nr, np.uint8), np.full(ns, 1 << 1, np.uint8), np.full(ns, 1 | (2 << 1), np.uint8)])
    neg_host = np.concatenate([np.asarray(negatives, dtype=np.int64), np.zeros(2 * ns, np.int64)])
    with torch.cuda.device(dev):
        pidx_d, neg_d, sel0_d, sel1_d, tag_d = _upload(
            [np.concatenate([np.asarray(rand_inds, dtype=np.int64), pos_idx, pos_idx]), neg_host, sel0, sel1], dev, tags=tags)
        ap = pairs_d.index_select(0, pidx_d)
        table, cap = _key_table(pairs_d, seed)
        keep = torch.empty(m, dtype=torch.uint8, device=dev)
        _key_mask(table, cap, seed, ap[:nr], 0, b=neg_d[:nr], keep=keep[:nr])
        if ns:
            ind0, ind1 = ap[nr:nr + ns, 0].contiguous(), ap[nr:nr + ns, 1].contiguous()
            # hardest negative of every sampled positive among the drawn rows of the other cloud (:700-704)
            _, a01 = pdist_min(F0, F1, "L2", rows_a=ind0, rows_b=sel1_d)
            _, a10 = pdist_min(F1, F0, "L2", rows_a=ind1, rows_b=sel0_d)
            # keys (ind0, sel1[a01]) and (sel0[a10], ind1) against the positives' (:711-719); the mined rows land in the table
            _key_mask(table, cap, seed, ap[nr:nr + ns], 0, b=sel1_d, b_arg=a01, b_out=neg_d[nr:nr + ns],
                      keep=keep[nr:nr + ns])
            _key_mask(table, cap, seed, ap[nr + ns:], 1, b=sel0_d, b_arg=a10, b_out=neg_d[nr + ns:], keep=keep[nr + ns:])
        loss, stats = _TripletFn.apply(F0, F1, ap, neg_d, tag_d, keep, float(neg_thresh), bool(deterministic_loss_backward))
    if details is not None:
        details.update(rand_mask=keep[:nr], mask0=keep[nr:nr + ns], mask1=keep[nr + ns:], neg01=neg_d[nr:nr + ns],
                       neg10=neg_d[nr + ns:])
    # per-set statistics at stats[2 + 6 s]: {kept, all, d_pos kept, d_neg kept, d_pos all, d_neg all}
    return loss, stats[2 + 6 + 4], (stats[2 + 6 + 5] + stats[2 + 12 + 5]) / 2


# ---- the pair trainers ---------------------------------------------------------------------------------------------------
class ContrastiveLossTrainer:
    """The hot loop body of lib/trainer.py's ContrastiveLossTrainer (``_train_epoch`` :214-289) without the dataset /
    logging / checkpoint shell, in the shape of ``gcl_amd.lib.colocation_trainer.FinestContrastiveLossTrainer``.

    One step = for each of ``config.iter_size`` pair batches (keys ``sinput0_C / _F``, ``sinput1_C / _F``,
    ``correspondences``): model forward on cloud 0, model forward on cloud 1 -- two SEPARATE training-mode passes, so that
    BatchNorm normalises each cloud with its own batch statistics and updates the running statistics twice, cloud 0
    first -- the loss, ``/ iter_size``, backward; then one optimizer step.  Both passes are alive until the backward
    pass: they run the per-operator path (the recorded Tape, one autograd node per pass), not the whole-network native
    plan, whose per-plan state has never been exercised with two passes waiting for their backward.  Data-parallel
    training is not offered here."""

    def __init__(self, config=None, model=None, device=None):
        from gcl_amd.lib.colocation_trainer import make_config
        from gcl_amd.model import load_model
        self.config = cfg = config or make_config()
        self.device = torch.device(device if device is not None else "cuda:0")
        if model is None:
            Model = load_model(cfg.model)
            model = Model(1, cfg.model_n_out, bn_momentum=cfg.bn_momentum, normalize_feature=cfg.normalize_feature,
                          conv1_kernel_size=cfg.conv1_kernel_size, D=3)
        self.model = model.to(self.device)
        if os.environ.get("GCL_FUSED_SGD", "1") == "1":          # same update, one launch (gcl_amd/lib/optim.py)
            from gcl_amd.lib.optim import FusedSGD
            self.optimizer = FusedSGD(self.model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                                      weight_decay=cfg.weight_decay)
        else:
            self.optimizer = torch.optim.SGD(self.model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                                             weight_decay=cfg.weight_decay)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, cfg.exp_gamma)
        self.neg_weight = cfg.neg_weight
        # the loss backward as records + ordered row sum (gcl_amd/lib/ordered.py): read by every pair trainer's pair_loss
        self.deterministic = bool(getattr(cfg, "deterministic_loss_backward", False))
        self._params = [p for p in self.model.parameters()]

    # -- what the four trainers differ in ---------------------------------------------------------------------------------
    def draw_for(self, input_dict):
        """The step's np.random draws for one pair batch, in the reference's order."""
        n0, n1, n_pairs = self._sizes(input_dict)
        return draw_rand_negative_pairs(n_pairs, n0, n1)

    def pair_loss(self, F0, F1, pos_pairs, draws):
        """``(loss, parts)``: the scalar that is back-propagated (before ``/ iter_size``) and the reported terms."""
        pos, neg = contrastive_random_negative_loss(F0, F1, pos_pairs, self.config.neg_thresh, draws=draws,
                                                    deterministic_loss_backward=self.deterministic)
        return pos + self.neg_weight * neg, (pos, neg)

    # -- the step ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _sizes(input_dict):
        return len(input_dict["sinput0_C"]), len(input_dict["sinput1_C"]), len(input_dict["correspondences"])

    def features(self, input_dict, k):
        import gcl_amd.MinkowskiEngine as ME
        sinput = ME.SparseTensor(input_dict[f"sinput{k}_F"].to(self.device, non_blocking=True),
                                 coordinates=input_dict[f"sinput{k}_C"].to(self.device, non_blocking=True))
        return self.model(sinput).F

    def train_step(self, input_dict, draws=None):
        """One optimizer step.  ``input_dict``: one pair batch, or a list of ``iter_size`` of them (``draws`` then is a list
        too).  Returns ``(loss, parts, n_rows)``: device scalars summed over the micro-batches like ``batch_loss``
        (lib/trainer.py:279-281), each already divided by ``iter_size``; no host sync."""
        with torch.cuda.device(self.device):
            self.model.train()
            micro = list(input_dict) if isinstance(input_dict, (list, tuple)) else [input_dict]
            n_micro = len(micro)
            if draws is None:
                mdraws = [self.draw_for(b) for b in micro]
            else:
                mdraws = list(draws) if isinstance(input_dict, (list, tuple)) else [draws]
            for p in self._params:
                p.grad = None
            tot_loss, tot_parts, n_rows = None, None, 0
            for b, d in zip(micro, mdraws):
                F0 = self.features(b, 0)
                F1 = self.features(b, 1)
                loss, parts = self.pair_loss(F0, F1, b["correspondences"], d)
                loss = loss / n_micro
                loss.backward()
                n_rows += F0.shape[0] + F1.shape[0]
                dl, dp = loss.detach(), tuple(p.detach() / n_micro for p in parts)
                tot_loss = dl if tot_loss is None else tot_loss + dl
                tot_parts = dp if tot_parts is None else tuple(x + y for x, y in zip(tot_parts, dp))
            self.optimizer.step()
            return tot_loss, tot_parts, n_rows

    def train_steps(self, batches):
        """Yields ``train_step(...)`` for every ``config.iter_size`` consecutive pair batches (a trailing incomplete group
        is dropped like ``len(data_loader) // iter_size``)."""
        k = max(1, int(getattr(self.config, "iter_size", 1)))
        grp = []
        for b in batches:
            grp.append(b)
            if len(grp) == k:
                yield self.train_step(grp if k > 1 else grp[0])
                grp = []

    def _valid_epoch(self, val_batches, val_max_iter=None, batch_pairs=8):
        """``_valid_epoch`` of lib/trainer.py (the same step as the co-location trainer's) on the device:
        ``gcl_amd.lib.validation.validate_pairs`` over ``val_batches`` (pair dicts with sinput{0,1}_C / _F, pcd0 / pcd1,
        T_gt), ``batch_pairs`` pairs per forward pass.  Returns the reference's dict of meters; leaves the model in eval
        mode, as the reference does (``train_step`` switches back)."""
        from gcl_amd.lib.validation import validate_pairs
        limit = getattr(self.config, "val_max_iter", -1) if val_max_iter is None else val_max_iter
        with torch.cuda.device(self.device):
            return validate_pairs(self.model, val_batches, val_max_iter=limit, batch_pairs=batch_pairs, subsample_size=5000,
                                  hit_ratio_thresh=getattr(self.config, "hit_ratio_thresh", 0.3),
                                  nn_max_n=getattr(self.config, "nn_max_n", 500))[0]


class HardestContrastiveLossTrainer(ContrastiveLossTrainer):
    """lib/trainer.py:408-540: positives against the hardest negatives (``contrastive_hardest_negative_loss``)."""

    def draw_for(self, input_dict):
        cfg = self.config
        n0, n1, n_pairs = self._sizes(input_dict)
        return draw_hardest_selections(n0, n1, n_pairs, cfg.num_pos_per_batch * cfg.batch_size,
                                       cfg.num_hn_samples_per_batch * cfg.batch_size)

    def pair_loss(self, F0, F1, pos_pairs, draws):
        cfg = self.config
        pos, neg = contrastive_hardest_negative_loss(F0, F1, pos_pairs, num_pos=cfg.num_pos_per_batch * cfg.batch_size,
                                                     num_hn_samples=cfg.num_hn_samples_per_batch * cfg.batch_size,
                                                     pos_thresh=cfg.pos_thresh, neg_thresh=cfg.neg_thresh, draws=draws,
                                                     deterministic_loss_backward=self.deterministic)
        return pos + self.neg_weight * neg, (pos, neg)


class TripletLossTrainer(ContrastiveLossTrainer):
    """lib/trainer.py:543-666: random triplets, ``config.neg_thresh`` as the margin.  ``parts`` = the two distance
    statistics the reference's meters receive (means of d_pos and of d_neg)."""

    def _counts(self):
        cfg = self.config
        return (cfg.triplet_num_pos * cfg.batch_size, cfg.triplet_num_hn * cfg.batch_size,
                cfg.triplet_num_rand * cfg.batch_size)

    def draw_for(self, input_dict):
        n0, n1, n_pairs = self._sizes(input_dict)
        num_pos, _, num_rand = self._counts()
        _check_rand_triplet_counts(n_pairs, n1, num_rand)
        return draw_triplet_selections(n1, n_pairs, num_pos, num_rand)

    def pair_loss(self, F0, F1, pos_pairs, draws):
        num_pos, num_hn, num_rand = self._counts()
        loss, pos_dist, neg_dist = triplet_loss(F0, F1, pos_pairs, num_pos=num_pos, num_hn_samples=num_hn,
                                                num_rand_triplet=num_rand, neg_thresh=self.config.neg_thresh, draws=draws,
                                                deterministic_loss_backward=self.deterministic)
        return loss, (pos_dist, neg_dist)


class HardestTripletLossTrainer(TripletLossTrainer):
    """lib/trainer.py:669-744: random triplets plus the hardest negatives of both directions."""

    def draw_for(self, input_dict):
        n0, n1, n_pairs = self._sizes(input_dict)
        num_pos, num_hn, num_rand = self._counts()
        _check_rand_triplet_counts(n_pairs, n1, num_rand)
        return draw_hardest_triplet_selections(n0, n1, n_pairs, num_pos, num_hn, num_rand)

    def pair_loss(self, F0, F1, pos_pairs, draws):
        num_pos, num_hn, num_rand = self._counts()
        loss, pos_dist, neg_dist = hardest_triplet_loss(F0, F1, pos_pairs, num_pos=num_pos, num_hn_samples=num_hn,
                                                        num_rand_triplet=num_rand, neg_thresh=self.config.neg_thresh,
                                                        draws=draws, deterministic_loss_backward=self.deterministic)
        return loss, (pos_dist, neg_dist)
