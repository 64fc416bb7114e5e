"""CPU restatement of the pair family's losses (random-negative contrastive, triplet, hardest triplet), written from
their formulas; torch on the CPU, any float dtype (the GPU tests feed it fp64 copies of the features).

    d(x, y)   = sqrt(sum_c (x_c - y_c)^2 + 1e-7)
    key(i, j) = i + j * seed, seed = max(N0, N1); a candidate (i, j) is kept iff its key is no positive pair's
    hinge     = relu(d(anchor, positive) + margin - d(anchor, negative))

Every function takes the recorded host draws, so that nothing here consumes random numbers.
"""
import numpy as np
import torch


def dist(x, y, eps=1e-7):
    return torch.sqrt(((x - y) ** 2).sum(1) + eps)


def keep_mask(r0, r1, pairs, seed):
    """bool [m]: (r0[t], r1[t]) is not among the positive pairs (int64 keys r0 + r1 * seed)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    keys = np.asarray(r0, dtype=np.int64) + np.asarray(r1, dtype=np.int64) * np.int64(seed)
    return ~np.isin(keys, pairs[:, 0] + pairs[:, 1] * np.int64(seed))


def _idx(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def pair_term(F0, F1, pairs, mode, thresh=0.0, eps=0.0):
    """Per-pair terms of the four pair modes (sq, sq_pos, neg, dist)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    d2 = ((F0[_idx(pairs[:, 0])] - F1[_idx(pairs[:, 1])]) ** 2).sum(1)
    if mode == "sq":
        return d2
    if mode == "sq_pos":
        return torch.relu(d2 - thresh)
    if mode == "neg":
        return torch.relu(thresh - torch.sqrt(d2 + eps)) ** 2
    if mode == "dist":
        return torch.sqrt(d2 + eps)
    raise ValueError(mode)


def triplet_terms(F0, F1, ap, neg, side, margin):
    """(hinge, d_pos, d_neg) per triplet; ap [m, 2] = (row of F0, row of F1); side 0: anchor in F0, positive and negative
    in F1; side 1: anchor in F1, the other two in F0."""
    ap = np.asarray(ap, dtype=np.int64).reshape(-1, 2)
    neg, side = np.asarray(neg, dtype=np.int64), np.asarray(side).astype(bool)
    s1 = torch.from_numpy(side)[:, None]
    i0, i1, ng = _idx(ap[:, 0]), _idx(ap[:, 1]), _idx(neg)
    A = torch.where(s1, F1[i1], F0[i0])
    P = torch.where(s1, F0[i0], F1[i1])
    N = torch.where(s1, F0[ng.clamp(max=len(F0) - 1)], F1[ng.clamp(max=len(F1) - 1)])     # a row id is valid in its own cloud
    dp, dn = dist(A, P), dist(A, N)
    return torch.relu(dp + margin - dn), dp, dn


def contrastive_random_negative(F0, F1, pairs, candidates, neg_thresh=1.4):
    """(pos_mean, neg_mean, keep): mean |a - b|^2 over all positive pairs; mean relu(neg_thresh - sqrt(|a - b|^2 + 1e-4))^2
    over the candidate pairs that are no positive pair."""
    seed = max(len(F0), len(F1))
    cand = np.asarray(candidates, dtype=np.int64).reshape(-1, 2)
    keep = keep_mask(cand[:, 0], cand[:, 1], pairs, seed)
    pos = pair_term(F0, F1, pairs, "sq").mean()
    neg = pair_term(F0, F1, cand[keep], "neg", neg_thresh, 1e-4).mean()
    return pos, neg, keep


def triplet(F0, F1, pairs, draws, margin=1.4):
    """draws = (pos_sel or None, rand_inds, negatives).  Returns (loss, mean d over the sampled positives, mean d_neg over
    the kept random triplets, rand_mask)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pos_sel, rand_inds, negatives = draws
    seed = max(len(F0), len(F1))
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
    rp = pairs[np.asarray(rand_inds, dtype=np.int64)]
    negatives = np.asarray(negatives, dtype=np.int64)
    keep = keep_mask(rp[:, 0], negatives, pairs, seed)
    h, _, dn = triplet_terms(F0, F1, rp[keep], negatives[keep], np.zeros(int(keep.sum())), margin)
    return h.mean(), pair_term(F0, F1, sample, "dist", eps=1e-7).mean(), dn.mean(), keep


def mine(Fa, Fb, rows_a, rows_b):
    """Row minimum / arg-minimum (lowest index on ties) of d(Fa[rows_a[i]], Fb[rows_b[j]]), row by row."""
    rows_a, rows_b = np.asarray(rows_a, dtype=np.int64), np.asarray(rows_b, dtype=np.int64)
    B = Fb[_idx(rows_b)].detach()
    dmin, arg = np.empty(len(rows_a)), np.empty(len(rows_a), dtype=np.int64)
    second = np.empty(len(rows_a))
    for i, r in enumerate(rows_a):
        d = torch.sqrt(((Fa[int(r)].detach()[None] - B) ** 2).sum(1) + 1e-7).double().numpy()
        j = int(np.argmin(d))
        dmin[i], arg[i] = d[j], j
        second[i] = np.partition(d, 1)[1] if len(d) > 1 else np.inf
    return dmin, arg, second


def hardest_triplet(F0, F1, pairs, draws, margin=1.4, mined=None):
    """draws = (sel0, sel1, pos_sel or None, rand_inds, negatives); ``mined = (neg01, neg10)`` evaluates the loss at given
    mined rows (of F1 / of F0) instead of this function's own arg-minima.  Returns a dict: loss, pos_dist (mean over the
    sampled positives), neg_dist ((mean D01min + mean D10min) / 2 over all sampled positives), the three masks, the mined
    rows, the row minima and the gap to the second-nearest candidate."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    sel0, sel1, pos_sel, rand_inds, negatives = draws
    sel0, sel1 = np.asarray(sel0, dtype=np.int64), np.asarray(sel1, dtype=np.int64)
    seed = max(len(F0), len(F1))
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
    ind0, ind1 = sample[:, 0], sample[:, 1]
    out = {}
    if mined is None:
        d01, a01, s01 = mine(F0, F1, ind0, sel1)
        d10, a10, s10 = mine(F1, F0, ind1, sel0)
        neg01, neg10 = sel1[a01], sel0[a10]
        out.update(d01=d01, d10=d10, gap=min(float((s01 - d01).min()), float((s10 - d10).min())) if len(ind0) else np.inf)
    else:
        neg01, neg10 = (np.asarray(x, dtype=np.int64) for x in mined)
    mask0 = keep_mask(ind0, neg01, pairs, seed)
    mask1 = keep_mask(neg10, ind1, pairs, seed)
    rp = pairs[np.asarray(rand_inds, dtype=np.int64)]
    negatives = np.asarray(negatives, dtype=np.int64)
    rand_mask = keep_mask(rp[:, 0], negatives, pairs, seed)
    ns = len(sample)
    h_r, _, _ = triplet_terms(F0, F1, rp[rand_mask], negatives[rand_mask], np.zeros(int(rand_mask.sum())), margin)
    h_0, dp0, dn0 = triplet_terms(F0, F1, sample, neg01, np.zeros(ns), margin)
    h_1, _, dn1 = triplet_terms(F0, F1, sample, neg10, np.ones(ns), margin)
    m0, m1 = torch.from_numpy(mask0), torch.from_numpy(mask1)
    terms = torch.cat([h_r, h_0[m0], h_1[m1]])
    out.update(loss=terms.mean(), pos_dist=dp0.mean(), neg_dist=(dn0.mean() + dn1.mean()) / 2, rand_mask=rand_mask,
               mask0=mask0, mask1=mask1, neg01=neg01, neg10=neg10, terms=terms)
    return out


def hinge_arguments(F0, F1, ap, neg, side, margin):
    """d_pos + margin - d_neg before the relu (how far every hinge is from its kink)."""
    _, dp, dn = triplet_terms(F0, F1, ap, neg, side, 0.0)
    return (dp + margin - dn).detach()


def hardest_contrastive(F0, F1, pairs, draws, pos_thresh=0.1, neg_thresh=1.4, mined=None):
    """The sibling loss of the hardest-contrastive trainer: draws = (sel0, sel1, pos_sel or None).  pos = mean
    relu(|a - b|^2 - pos_thresh) over the sampled positives; neg = (mean relu(neg_thresh - d(F0[i], F1[neg01]))^2 over
    mask0 + the same for (F0[neg10], F1[j]) over mask1) / 2.  Returns a dict like ``hardest_triplet``."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    sel0, sel1, pos_sel = draws
    sel0, sel1 = np.asarray(sel0, dtype=np.int64), np.asarray(sel1, dtype=np.int64)
    seed = max(len(F0), len(F1))
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
    ind0, ind1 = sample[:, 0], sample[:, 1]
    out = {}
    if mined is None:
        d01, a01, _ = mine(F0, F1, ind0, sel1)
        d10, a10, _ = mine(F1, F0, ind1, sel0)
        neg01, neg10 = sel1[a01], sel0[a10]
        out.update(d01=d01, d10=d10)
    else:
        neg01, neg10 = (np.asarray(x, dtype=np.int64) for x in mined)
    mask0 = keep_mask(ind0, neg01, pairs, seed)
    mask1 = keep_mask(neg10, ind1, pairs, seed)
    pos = pair_term(F0, F1, sample, "sq_pos", pos_thresh).mean()
    n0 = pair_term(F0, F1, np.stack([ind0, neg01], 1)[mask0], "neg", neg_thresh, 1e-7).mean()
    n1 = pair_term(F0, F1, np.stack([neg10, ind1], 1)[mask1], "neg", neg_thresh, 1e-7).mean()
    out.update(pos=pos, neg=(n0 + n1) / 2, mask0=mask0, mask1=mask1, neg01=neg01, neg10=neg10)
    return out
