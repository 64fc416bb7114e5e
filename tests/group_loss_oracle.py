"""Per-group reference of the loss entry points of csrc/loss.hip (test infrastructure; plain torch / numpy on the CPU).

One function per C-ABI entry, taking what the entry takes, written from the reference's own lines
(lib/colocation_trainer.py:430-535 finest_contrastive_loss, :538-641 the per-group half of location_circle_loss,
:734-809 location_contrastive_loss, util/misc.py:29-40 the pair keys) as oracle/loss_oracle.py restates them -- one group
at a time, so that every ``pos[s]`` / ``fin[s]`` / ``mean[s]`` / ``keep[r]`` can be compared on its own instead of inside
a mean over hundreds of groups.  Gradients come from autograd on the SAME expressions.

``dtype=torch.float64`` is the reference the kernels are tested against; ``dtype=torch.float32`` evaluates the same
expressions in the kernels' precision, which is how the tests' tolerances are measured (test_oracle_group_loss.py).
"""
import numpy as np
import torch
import torch.nn.functional as Fn

GL_SQRT, GL_BLOCK, GL_PAIR, GL_NOFIN = 1, 2, 4, 8          # GCL_LOSS_* of include/gcl_amd.h


class Terms:
    """Values (detached, numpy float64) of one call and ``grad(...)`` = dF of sum_s g[s] * term[s] (autograd)."""

    def __init__(self, F, **terms):
        self._F = F
        self._t = terms
        for k, v in terms.items():
            setattr(self, k, v.detach().double().numpy() if torch.is_tensor(v) else v)

    def grad(self, gpos, gfin, gmean=None):
        tot = self._F.sum() * 0
        for key, g in (("pos", gpos), ("fin", gfin), ("mean", gmean)):
            if g is None:
                continue
            t = self._t[key]
            assert bool(torch.isfinite(t.detach()).all()), "no gradient is defined through a NaN term"
            tot = tot + (t * torch.as_tensor(np.asarray(g), dtype=t.dtype)).sum()
        (d,) = torch.autograd.grad(tot, self._F, allow_unused=True, retain_graph=True)
        d = torch.zeros_like(self._F) if d is None else d
        return d.double().numpy()


def _leaf(F, dtype):
    return torch.as_tensor(np.asarray(F), dtype=dtype).clone().requires_grad_(True)


def _groups(index, goff, flag, sel):
    index = torch.as_tensor(np.asarray(index), dtype=torch.long)
    flag = torch.as_tensor(np.asarray(flag)).bool()
    goff = [int(g) for g in np.asarray(goff)]
    for s, i in enumerate(np.asarray(sel)):
        yield s, index[goff[i]:goff[i + 1]], flag[goff[i]:goff[i + 1]]


def group_terms(F, index, goff, flag, sel, pos_thresh, fin_thresh, flags, pairpos=None, dtype=torch.float64):
    """gcl_group_loss_fwd / _bwd: lib/colocation_trainer.py:463-488 for each selected group.
    -> Terms with pos, fin [n_sel] (after the hinge) and pos_pre, fin_pre (before it)."""
    F = _leaf(F, dtype)
    sq = not flags & GL_SQRT

    def dist(d2):
        return d2 if sq else torch.sqrt(d2 + 1e-7)

    pos_pre, fin_pre = [], []
    for s, idx, fl in _groups(index, goff, flag, sel):
        fs = F[idx]
        mean = torch.mean(fs, dim=0)
        if flags & GL_PAIR:                                                                           # :466-471
            a, b = int(pairpos[s][0]), int(pairpos[s][1])
            pos_pre.append(dist((fs[a] - fs[b]).pow(2).sum(-1)))
        else:                                                                                         # :472-476
            pos_pre.append(torch.mean(dist((mean - fs).pow(2).sum(-1))))
        if flags & GL_NOFIN:                                                                          # :734-809: no such term
            fin_pre.append(None)
        elif flags & GL_BLOCK:                                                                        # :478-481
            blocked = fs[torch.bitwise_not(fl)]
            fin_pre.append(torch.sqrt((torch.mean(blocked, dim=0) - fs[fl][0].detach()).pow(2).sum() + 1e-7))
        else:                                                                                         # :483-488
            fin_pre.append(dist((mean - fs[fl][0]).pow(2).sum()))
    pos_pre = torch.stack(pos_pre)
    pos = torch.relu(pos_pre - pos_thresh)
    if flags & GL_NOFIN:
        fin_pre = torch.full_like(pos_pre.detach(), float("nan"))
        fin = torch.zeros_like(pos_pre.detach())
    else:
        fin_pre = torch.stack(fin_pre)
        fin = torch.relu(fin_pre - fin_thresh)                                                         # relu(NaN) = NaN
    return Terms(F, pos=pos, fin=fin, pos_pre=pos_pre, fin_pre=fin_pre)


def circle_terms(F, index, goff, flag, sel, pos_thresh, fin_thresh, log_scale, flags, pairpos=None,
                 dtype=torch.float64):
    """gcl_circle_group_fwd / _bwd: lib/colocation_trainer.py:583-641 for each selected group.
    -> Terms with pos, fin [n_sel], mean [n_sel, c]; pos_v / fin_v = every member's value before max(v, 0) (one
    array over all groups), pos_arg / fin_arg = the softplus arguments [n_sel]."""
    F = _leaf(F, dtype)
    sq = not flags & GL_SQRT

    def dist(d2):
        return d2 if sq else torch.sqrt(d2 + 1e-7)

    def lse(v):                                                                                       # :616-619
        return torch.logsumexp(log_scale * v * torch.max(torch.zeros_like(v), v).detach(), dim=-1)

    pos, fin, means, pos_v, fin_v, pos_arg, fin_arg = [], [], [], [], [], [], []
    for s, idx, fl in _groups(index, goff, flag, sel):
        fs = F[idx]
        mean = torch.mean(fs, dim=0)
        means.append(mean)                                                                            # :587
        if flags & GL_PAIR:                                                                           # :597-606
            a, b = int(pairpos[s][0]), int(pairpos[s][1])
            x = dist((fs[a] - fs[b]).pow(2).sum(-1)) - pos_thresh
            pos.append(Fn.softplus(x))
        else:                                                                                         # :609-619
            v = dist((mean - fs).pow(2).sum(-1)) - pos_thresh / 2
            pos_v.append(v.detach())
            x = lse(v)
            pos.append(Fn.softplus(x) / log_scale)
        pos_arg.append(x.detach())
        if flags & GL_BLOCK:                                                                          # :622-629
            v = dist((fs[~fl] - fs[fl][0].detach()).pow(2).sum(-1)) - fin_thresh
        else:                                                                                         # :631-636
            v = dist((fs - fs[fl][0]).pow(2).sum(-1)) - fin_thresh
        fin_v.append(v.detach())
        if len(v) == 0:                                     # logsumexp of an empty set: -inf, softplus: 0, no gradient
            fin_arg.append(torch.tensor(float("-inf"), dtype=dtype))
            fin.append(torch.zeros((), dtype=dtype))
        else:
            x = lse(v)
            fin_arg.append(x.detach())
            fin.append(Fn.softplus(x) / log_scale)                                                    # :637-641
    cat = lambda vs: torch.cat(vs) if vs else torch.zeros(0, dtype=dtype)
    return Terms(F, pos=torch.stack(pos), fin=torch.stack(fin), mean=torch.stack(means), pos_v=cat(pos_v),
                 fin_v=cat(fin_v), pos_arg=torch.stack(pos_arg), fin_arg=torch.stack(fin_arg))


def neg_hash(i1, i2, M):
    """util/misc.py:39-40."""
    i1, i2 = np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64)
    return np.minimum(i1 * M + i2, i1 + i2 * M)


def exhaustive_hash(index, goff, M):
    """util/misc.py:29-36 over every group (one-member groups have no pair)."""
    index, goff = np.asarray(index, dtype=np.int64), np.asarray(goff, dtype=np.int64)
    res = [np.zeros(0, dtype=np.int64)]
    for g in range(len(goff) - 1):
        idx = index[goff[g]:goff[g + 1]]
        for i in range(len(idx) - 1):
            res.append(np.minimum(idx[i] + idx[i + 1:] * M, idx[i] * M + idx[i + 1:]))
    return np.concatenate(res)


def neg_mask(sel1, sel2, arg, index, goff, n_rows=None):
    """gcl_neg_mask: lib/colocation_trainer.py:521-529 -- not the row itself, and the pair's key not among the keys of
    the in-group pairs.  ``n_rows`` = the hash seed (:446, the number of feature rows; any larger value gives the same
    mask, the key being collision-free above the largest row)."""
    sel1, sel2 = np.asarray(sel1, dtype=np.int64), np.asarray(sel2, dtype=np.int64)
    closest = sel2[np.asarray(arg, dtype=np.int64)]
    index = np.asarray(index, dtype=np.int64)
    if n_rows is None:
        n_rows = int(max([sel1.max(), sel2.max()] + ([index.max()] if len(index) else []))) + 1
    pos_keys = exhaustive_hash(index, goff, n_rows)
    mask = np.logical_not(np.isin(neg_hash(sel1, closest, n_rows), pos_keys))
    return (mask & (sel1 != closest)).astype(np.uint8)


def neg_loss(dmin, keep, thresh, dtype=torch.float64):
    """gcl_neg_loss_fwd: :530, :535 -> (mean of relu(thresh - dmin)^2 over the kept rows (NaN if none), their count)."""
    d = torch.as_tensor(np.asarray(dmin), dtype=dtype)[torch.as_tensor(np.asarray(keep)).bool()]
    return float(torch.relu(thresh - d).pow(2).mean()), int(len(d))


def neg_loss_grad(F, sel1, sel2, arg, keep, thresh, gneg, dtype=torch.float64):
    """gcl_neg_loss_bwd: dF of gneg * neg_loss with dmin = sqrt(|F[sel1] - F[sel2[arg]]|^2 + 1e-7) (lib/metrics.py:22-25)."""
    F = _leaf(F, dtype)
    keep = torch.as_tensor(np.asarray(keep)).bool()
    if not keep.any():
        return np.zeros(F.shape)
    ra = torch.as_tensor(np.asarray(sel1), dtype=torch.long)
    rb = torch.as_tensor(np.asarray(sel2), dtype=torch.long)[torch.as_tensor(np.asarray(arg), dtype=torch.long)]
    D = torch.sqrt((F[ra] - F[rb]).pow(2).sum(-1) + 1e-7)
    loss = torch.relu(thresh - D[keep]).pow(2).mean() * float(gneg)
    (d,) = torch.autograd.grad(loss, F)
    return d.double().numpy()


def dmin_of(F, sel1, sel2, arg):
    """sqrt(d2 + 1e-7) in fp64 for the pairs (sel1[r], sel2[arg[r]])."""
    F = np.asarray(F, dtype=np.float64)
    d = F[np.asarray(sel1)] - F[np.asarray(sel2)[np.asarray(arg)]]
    return np.sqrt((d * d).sum(-1) + 1e-7)


def combine(pos, fin, neg, w):
    """gcl_loss_combine: :500 and :865-868 -> (total, pos mean, finest mean, neg) in fp64."""
    pm, fm = float(np.mean(np.asarray(pos, dtype=np.float64))), float(np.mean(np.asarray(fin, dtype=np.float64)))
    return w[0] * pm + w[1] * fm + w[2] * float(neg), pm, fm, float(neg)


def seed(g, w, n_sel):
    """gcl_loss_seed: the upstream gradients of the three terms from that of the total -> (gpos[s], gfin[s], gneg)."""
    g = float(g)
    return np.full(n_sel, g * w[0] / n_sel), np.full(n_sel, g * w[1] / n_sel), g * w[2]
