"""Seeded inputs of the loss-kernel tests (tests/test_oracle_group_loss.py asserts their conditions on the CPU,
tests/test_gpu_loss_kernels.py runs the kernels on them): ONE generator, ``scene``, and the plan of cases.

A scene is ~350 feature rows and ~30 groups:
* group sizes from {1, 2, 3, 5, 16, 35, 70} (70 > the 64 lanes of a wave); one-member groups are left out with PAIR (the
  reference draws two distinct members) and with BLOCK (a one-member group has every member flagged, and exactly one
  all-flagged group is wanted there: it is added separately -- one member without PAIR, three with -- as ``sel[all_s]``);
* the first flag at the first, a middle and the last position in turn; two groups carry two flags;
* members = anchor + noise at two levels: TIGHT (every hinge of the group inactive) and LOOSE (active);
* >= 20 rows are members of two selected groups (a LOOSE group's member replaced by another selected group's row), more
  than a third of the rows are in no selected group, ``sel`` is an unsorted strict subset of the groups;
* rows have unit norm, times ``scale`` (4: softplus's x > 20 branch);
* the seed is redrawn until every value that enters a hinge is further than MARGIN (relative) from its threshold in fp64,
  for both distance forms and both kernel families, so that no fp32 rounding can change the side.
"""
import functools
import types

import numpy as np

import group_loss_oracle as GO

SQRT, BLOCK, PAIR, NOFIN = GO.GL_SQRT, GO.GL_BLOCK, GO.GL_PAIR, GO.GL_NOFIN
POS_THRESH, FIN_THRESH, LOG_SCALE = 0.1, 0.2, 16.0
TIGHT, LOOSE = 0.005, 0.6
MARGIN = 1e-4
WIDTHS = (1, 3, 16, 31, 32, 33, 63, 64)
FULL_GRID = (32, 64)                                       # every flag value at these widths
SCALES = (1.0, 4.0)
GROUP_SPARSE = (0, SQRT, BLOCK | PAIR, SQRT | BLOCK | NOFIN)
CIRCLE_SPARSE = (0, SQRT, BLOCK | PAIR, SQRT | BLOCK)      # the same plan without NOFIN, which the circle loss lacks

GROUP_CASES = [(c, f) for c in WIDTHS for f in (range(16) if c in FULL_GRID else GROUP_SPARSE)]
CIRCLE_CASES = [(c, f) for c in WIDTHS for f in (range(8) if c in FULL_GRID else CIRCLE_SPARSE)]


def _build(seed, c, scale, pair, block):
    rng = np.random.RandomState(seed)
    small = [s for s in (1, 2, 3, 5) if not ((pair or block) and s == 1)]
    sizes = [70, 35, 16, 16, 16] + 3 * small
    sizes += list(rng.choice(small, 29 - len(sizes)))
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    all_g = None
    if block:
        all_g = int(rng.randint(0, len(sizes) + 1))
        sizes.insert(all_g, 3 if pair else 1)
    n_groups, total = len(sizes), int(np.sum(sizes))
    n_rows = total * 3 // 2 + 20
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    index = rng.permutation(n_rows)[:total].astype(np.int64)             # every group starts on rows of its own
    F = rng.normal(size=(n_rows, c))
    flag = np.zeros(total, dtype=np.uint8)
    loose = np.zeros(n_groups, dtype=bool)
    two_flags, seen, turn = [], {}, 0
    for g, n in enumerate(sizes):
        k = seen.get(n, 0)
        seen[n] = k + 1
        loose[g] = n > 1 and ((k % 2 == 0) != (n == 35)) and g != all_g   # the 70 is loose, the 35 tight, the rest in turn
        rows = index[goff[g]:goff[g + 1]]
        anchor = F[rows[0]] / np.linalg.norm(F[rows[0]])
        F[rows] = anchor + (LOOSE if loose[g] else TIGHT) * rng.normal(size=(n, c)) / np.sqrt(c)
        if g == all_g:
            flag[goff[g]:goff[g + 1]] = 1
        elif n in (5, 16) and k == 0:
            flag[[goff[g] + 1, goff[g] + n - 2]] = 1
            two_flags.append(g)
        else:
            flag[goff[g] + (0, n // 2, n - 1)[turn % 3]] = 1
            turn += 1
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    F = (scale * F).astype(np.float32)

    special = set(two_flags) | {sizes.index(n) for n in set(sizes)} | ({all_g} if block else set())   # every size stays
    out = rng.choice([g for g in range(n_groups) if g not in special], 5, replace=False)
    sel = np.array([g for g in range(n_groups) if g not in out], dtype=np.int64)
    while (np.diff(sel) > 0).all():
        sel = rng.permutation(sel)
    # shared rows: a member slot of a LOOSE selected group takes a row of ANOTHER selected group
    slots = [(g, j) for g in sel if loose[g] and sizes[g] >= 3 for j in range(sizes[g])]
    chosen = [slots[i] for i in rng.permutation(len(slots))[:26]]
    donors = [(int(g), int(j)) for g, j in rng.permutation([(g, j) for g in sel for j in range(sizes[g])])
              if (g, j) not in chosen]                                    # a donor keeps its own place
    used = set()
    for b, j in chosen:
        mine = set(index[goff[b]:goff[b + 1]].tolist())
        for a, i in donors:
            row = int(index[goff[a] + i])
            if a != b and row not in mine and row not in used:
                used.add(row)
                index[goff[b] + j] = row
                break
    members = np.zeros(n_rows, dtype=np.int64)
    for g in sel:
        members[np.unique(index[goff[g]:goff[g + 1]])] += 1
    pairpos = None
    if pair:
        pairpos = np.stack([rng.choice(sizes[g], 2, replace=False) for g in sel]).astype(np.int32)
    n_sel = len(sel)
    return types.SimpleNamespace(
        seed=seed, c=c, scale=scale, pair=pair, block=block, F=F, index=index, goff=goff, flag=flag, sel=sel,
        sizes=np.asarray(sizes), loose=loose, two_flags=two_flags, members=members, pairpos=pairpos,
        all_s=int(np.nonzero(sel == all_g)[0][0]) if block else None,
        gpos=rng.uniform(0.5, 1.5, n_sel).astype(np.float32), gfin=rng.uniform(0.5, 1.5, n_sel).astype(np.float32),
        gmean=(0.1 * rng.normal(size=(n_sel, c))).astype(np.float32),
        prefill=(((np.arange(n_rows * c) % 7) + 1) / 64.0).astype(np.float32).reshape(n_rows, c))


def _far(v, thresh):
    v = np.asarray(v)
    v = v[np.isfinite(v)]
    return bool((np.abs(v - thresh) > MARGIN * abs(thresh)).all())


def margins_hold(sc):
    """Every value that enters a hinge (relu, max(v, 0), softplus's x > 20) is clear of its threshold, in fp64."""
    base = (PAIR if sc.pair else 0) | (BLOCK if sc.block else 0)
    for fl in (base, base | SQRT):
        t = GO.group_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, POS_THRESH, FIN_THRESH, fl, sc.pairpos)
        q = GO.circle_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, POS_THRESH, FIN_THRESH, LOG_SCALE, fl, sc.pairpos)
        if not (_far(t.pos_pre, POS_THRESH) and _far(t.fin_pre, FIN_THRESH)
                and _far(q.pos_v + POS_THRESH / 2, POS_THRESH / 2) and _far(q.fin_v + FIN_THRESH, FIN_THRESH)
                and _far(q.pos_arg, 20.0) and _far(q.fin_arg, 20.0)):
            return False
    return True


@functools.lru_cache(maxsize=None)
def scene(c, scale, pair, block):
    """The scene of one (width, scale, PAIR?, BLOCK?): the first seed 1000 k + c whose margins hold."""
    for k in range(200):
        sc = _build(1000 * k + c, c, scale, pair, block)
        if margins_hold(sc):
            return sc
    raise AssertionError("no seed satisfies the margins")


def case_scene(c, flags, scale):
    return scene(c, scale, bool(flags & PAIR), bool(flags & BLOCK))


def without(sc, s):
    """(sel, pairpos, gpos, gfin, gmean) of the scene with the selected entry ``s`` left out (None: as they are)."""
    keep = np.arange(len(sc.sel)) != (-1 if s is None else s)
    return (sc.sel[keep], None if sc.pairpos is None else sc.pairpos[keep], sc.gpos[keep], sc.gfin[keep], sc.gmean[keep])


def touched(sc, sel):
    """Rows that are members of a group of ``sel``."""
    t = np.zeros(len(sc.F), dtype=bool)
    for g in sel:
        t[sc.index[sc.goff[g]:sc.goff[g + 1]]] = True
    return t


def row_error(got, want):
    """max over the rows of |got - want| / (|want| + g), g = the largest row norm of want (0 for an all-zero want)."""
    nw = np.linalg.norm(want, axis=1)
    g = nw.max()
    if g == 0:
        return float(np.abs(got - want).max())
    return float((np.linalg.norm(got - want, axis=1) / (nw + g)).max())


def rel_l2(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


# ---- the negative term ---------------------------------------------------------------------------------------------------
NEG_M = (1, 255, 256, 257, 700)            # the edges of the 256-thread reductions
NEG_WIDTHS = (1, 16, 33, 64)
NEG_THRESH = 1.0
NEG_CASES = [(m, c, side) for m in NEG_M for c in NEG_WIDTHS for side in ((None,) if m > 1 else (True, False))]


@functools.lru_cache(maxsize=None)
def neg_scene(m, c, side=None):
    """m (row, target) pairs over rows whose distances straddle NEG_THRESH; keep random, 0 on self pairs;
    dmin = the fp64 sqrt(d2 + 1e-7) rounded to fp32.  Redrawn until every kept row's dmin is further than MARGIN from the
    threshold and both sides occur (one pair: ``side`` = whether its hinge is active)."""
    for k in range(500):
        rng = np.random.RandomState(1000 * k + 7 * m + c)
        n_rows = max(300, m + 60)
        # two row populations: E d^2 = 0.16, 1.36 or 2.56, so that at 64 channels the distances do not crowd at the threshold
        F = (rng.choice([0.4, 1.6], (n_rows, 1)) * rng.normal(size=(n_rows, c)) / np.sqrt(2 * c)).astype(np.float32)
        sel1, sel2 = rng.choice(n_rows, m, replace=False), rng.choice(n_rows, m, replace=False)
        arg = rng.randint(0, m, m).astype(np.int32)
        where = {int(x): i for i, x in enumerate(sel2)}
        for r in range(0, m, 9):                                           # some self pairs
            if m > 1 and int(sel1[r]) in where:
                arg[r] = where[int(sel1[r])]
        keep = ((rng.rand(m) < 0.7) & (sel1 != sel2[arg])).astype(np.uint8)
        if m == 1:
            keep[:] = sel1 != sel2[arg]
        dmin = GO.dmin_of(F, sel1, sel2, arg).astype(np.float32)
        d = dmin[keep != 0].astype(np.float64)
        active = d < NEG_THRESH
        if len(d) and (np.abs(NEG_THRESH - d) > MARGIN).all() and \
                ((active.any() and not active.all()) if side is None else bool(active[0]) == side):
            return types.SimpleNamespace(F=F, sel1=sel1.astype(np.int64), sel2=sel2.astype(np.int64), arg=arg, keep=keep,
                                         dmin=dmin, gneg=np.float32(0.9),
                                         prefill=(((np.arange(n_rows * c) % 7) + 1) / 64.0).astype(np.float32).reshape(n_rows, c))
    raise AssertionError("no seed satisfies the margins")


# ---- the negative-pair mask ------------------------------------------------------------------------------------------
KINDS = ("self", "same_group", "no_common_group", "second_group", "other_groups_only")


def mask_scene(seed, m, only=None):
    """sel1 (m rows, drawn without replacement), sel2, arg with every kind of (row, target) pair in turn (``only``: one kind):
    self; both in one group; no common group (the target in no group at all); a row of two groups with its target in the
    SECOND; a target that is a member of groups, none of which holds the row.  -> namespace with ``kind[r]``."""
    rng = np.random.RandomState(seed)
    n_rows = max(300, m + 60)
    sizes = [16, 16, 5, 5, 5] + list(rng.choice([2, 3, 5], 25))
    total = int(np.sum(sizes))
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    index = rng.permutation(n_rows)[:total].astype(np.int64)
    for g in range(1, len(sizes)):                                         # members of group g - 1 join group g as well
        index[goff[g]] = index[goff[g - 1] + 1]
        if sizes[g] >= 5 and sizes[g - 1] >= 3:
            index[goff[g] + 2] = index[goff[g] - 1]
    free = np.setdiff1d(np.arange(n_rows), index)
    groups_of = {}
    for g in range(len(sizes)):
        for r in index[goff[g]:goff[g + 1]]:
            groups_of.setdefault(int(r), set()).add(g)
    two = [r for r, gs in groups_of.items() if len(gs) == 2]
    grouped = sorted(groups_of)
    # sel1: the two-group rows and other grouped rows first (so that every kind has rows), then the rest, shuffled
    lead = list(rng.permutation(two)) + list(rng.permutation([r for r in grouped if r not in two]))
    rest = list(rng.permutation(np.setdiff1d(np.arange(n_rows), lead)))
    if m >= len(KINDS):
        head = lead[:max(len(KINDS), m // 2)]
        sel1 = np.array(head + rest[:m - len(head)], dtype=np.int64)[:m]
        sel1 = sel1[rng.permutation(m)]
    else:
        sel1 = np.array(two[:m], dtype=np.int64)
    target, kind, count = np.empty(m, dtype=np.int64), [], [0, 0, 0]
    for r, row in enumerate(sel1):
        row = int(row)
        gs = sorted(groups_of.get(row, ()))
        turn = (("no_common_group", "other_groups_only", "self"), ("same_group", "other_groups_only", "same_group", "self"),
                ("second_group",))[len(gs)]                                # by the number of groups the row is in
        want = only if only is not None else turn[count[len(gs)] % len(turn)]
        count[len(gs)] += 1
        if want in ("same_group", "second_group") and len(gs) < (2 if want == "second_group" else 1):
            want = "no_common_group"
        if want == "self":
            t = row
        elif want in ("same_group", "second_group"):
            g = gs[-1] if want == "second_group" else gs[0]
            mates = [int(x) for x in index[goff[g]:goff[g + 1]] if x != row]
            if want == "second_group":                                      # not a member of the row's first group
                mates = [x for x in mates if gs[0] not in groups_of[x]]
            t = mates[rng.randint(len(mates))]
        elif want == "other_groups_only":
            cand = [x for x in grouped if not (groups_of[x] & set(gs))]
            t = cand[rng.randint(len(cand))]
        else:
            cand = free[free != row] if gs == [] else free
            t = int(cand[rng.randint(len(cand))])
        target[r] = t
        kind.append(want)
    uniq = np.unique(target)
    fill = rng.permutation(np.setdiff1d(np.arange(n_rows), uniq))[:max(0, m - len(uniq))]
    sel2 = rng.permutation(np.concatenate([uniq, fill])).astype(np.int64)
    where = {int(x): i for i, x in enumerate(sel2)}
    arg = np.array([where[int(t)] for t in target], dtype=np.int32)
    return types.SimpleNamespace(n_rows=n_rows, sel1=sel1, sel2=sel2, arg=arg, index=index, goff=goff,
                                 kind=np.array(kind), target=target)
