"""The five loss backward families as emit -> gcl_ordered_row_sum, through the C ABI (include/gcl_amd.h, "Loss backward
without float atomics").  Per case:

  (a) the rec_row sequence equals a numpy restatement of the kernel's program order EXACTLY, -1 where the atomic kernel
      skips (which hinge is active is read from the forward entry's own fp32 output, as the kernel decides it);
  (b) the chain's dF equals the numpy serial replay of the emitted records exactly (tests/ordered_records.py);
  (c) the per-row fp64 sum of the records meets the fp64 oracle's gradient within the tolerances the atomic kernels are held
      to: the TOL / PROJECT tables of test_gpu_loss_kernels.py (the ordered sum is one of the orders those bounds cover),
      1e-5 rel-L2 for the pair family (test_gpu_pair_loss.py);
  (d) on inputs where no row receives more than one contribution the atomic entry and the chain agree on every element
      (``==``: +0 and -0 are equal) -- the two are one kernel body.  The property is asserted on the CPU first.  The circle
      loss hands the finest member a second record (its collected gradient), so there a row may have two, into a ZERO
      buffer: fl(fl(0 + a) + b) = fl(fl(0 + b) + a), the order of two addends cannot show.

Scenes: tests/group_loss_scenes.py (shared rows, both sides of every hinge) at widths 1, 31, 32, 33, 64 with every switch
set test_gpu_loss_kernels.py runs there; the negative term at m = 255, 256, 257; the pair family at widths 4, 16, 17, 32, 33,
64 (4 / 2 / 1 rows per wave) with keep masks and row ids outside their cloud."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_loss_oracle as GO                                         # noqa: E402
import group_loss_scenes as GS                                         # noqa: E402
import pair_loss_oracle as PO                                          # noqa: E402
from ordered_records import named, row_sums64, serial                  # noqa: E402
from test_gpu_loss_kernels import PROJECT, TOL                         # noqa: E402

DEV = "cuda:0"
WIDTHS = (1, 31, 32, 33, 64)
GROUP_CASES = [(c, f) for c, f in GS.GROUP_CASES if c in WIDTHS]
CIRCLE_CASES = [(c, f) for c, f in GS.CIRCLE_CASES if c in WIDTHS]
PAIR_WIDTHS = (4, 16, 17, 32, 33, 64)
PAIR_TOL = 1e-5                                                        # rel-L2 on dF0 / dF1: test_gpu_pair_loss.py


def _tol(fam, what, scale):
    key = (fam, what, float(scale))
    return PROJECT.get(key, TOL[key])


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _call(entry, *args):
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    with torch.cuda.device(DEV):
        a = [_lib.ptr(x) if (x is None or torch.is_tensor(x)) else x for x in args]
        _lib.check(getattr(lib, entry)(*a, _lib.stream()), entry)
        torch.cuda.synchronize()


def _lib_call(name, *args):
    from gcl_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def _records(n_rec, c):
    """lists with stale contents: the entry fills every rec_row, the values of skipped records are never read"""
    return (torch.full((n_rec,), 12345, dtype=torch.int32, device=DEV),
            torch.full((n_rec, c), float("nan"), dtype=torch.float32, device=DEV))


def _reduce(rec_row, rec_val, prefill):
    """gcl_ordered_row_sum of device lists into a copy of ``prefill`` -> numpy"""
    dF = _dev(prefill)
    n_rec, (n_rows, c) = rec_row.shape[0], prefill.shape
    scratch = torch.empty(max(1, _lib_call("gcl_ordered_row_sum_scratch_len", n_rec, n_rows)), dtype=torch.int32, device=DEV)
    _call("gcl_ordered_row_sum", rec_row, rec_val, n_rec, c, n_rows, scratch, dF)
    return dF.cpu().numpy()


def _check_chain(rec_row_d, rec_val_d, prefill, want_rows):
    """(a) and (b) of one list; returns (rec_row, rec_val, dF) on the host."""
    rec_row, rec_val = rec_row_d.cpu().numpy(), rec_val_d.cpu().numpy()
    bad = np.nonzero(rec_row != want_rows)[0]
    assert np.array_equal(rec_row, want_rows), (len(bad), bad[:8], rec_row[bad[:8]], want_rows[bad[:8]])
    ok, _ = named(rec_row, len(prefill))
    assert np.isfinite(rec_val[ok]).all()
    got = _reduce(rec_row_d, rec_val_d, prefill)
    want = serial(rec_row, rec_val, prefill)
    assert np.array_equal(got, want), int((got != want).any(1).sum())
    assert got[np.bincount(rec_row[ok], minlength=len(prefill)) == 0].tobytes() == \
        prefill[np.bincount(rec_row[ok], minlength=len(prefill)) == 0].tobytes()
    return rec_row, rec_val, got


def _check_oracle(fam, scale, rec_row, rec_val, want):
    """(c): the per-row fp64 sum of the records against the fp64 oracle's gradient"""
    sums = row_sums64(rec_row, rec_val, len(want))
    e_all, e_row = GS.rel_l2(sums, want), GS.row_error(sums, want)
    print(f"  records: rel-L2 {e_all:.3e} (tol {_tol(fam, 'df', scale):.3e}), per row {e_row:.3e} (tol {_tol(fam, 'row', scale):.3e})")
    assert np.linalg.norm(want) > 0
    assert e_all <= _tol(fam, "df", scale), e_all
    assert e_row <= _tol(fam, "row", scale), e_row


# ---- group loss and circle loss -------------------------------------------------------------------------------------------
def _scene_args(sc):
    return _dev(sc.F), sc.c, _dev(sc.index), _dev(sc.goff), _dev(sc.flag)


def _group_fwd(sc, flags, sel, pp):
    n_sel = len(sel)
    pos, fin = torch.empty(n_sel, device=DEV), torch.empty(n_sel, device=DEV)
    _call("gcl_group_loss_fwd", *_scene_args(sc), _dev(sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, int(flags), _dev(pp), pos, fin)
    return pos.cpu().numpy(), fin.cpu().numpy()


def _group_emit(sc, flags, sel, pp, gpos, gfin, spare=5):
    n_sel, members = len(sel), int(sc.sizes[sel].sum())
    need = _lib_call("gcl_group_loss_records", members, n_sel, int(flags))
    assert need == members + (2 * n_sel if flags & GS.PAIR else 0)
    rec_row, rec_val = _records(need + spare, sc.c)
    rec_off = torch.full((n_sel + 1,), -9, dtype=torch.int32, device=DEV)
    _call("gcl_group_loss_bwd_emit", *_scene_args(sc), _dev(sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, int(flags), _dev(pp),
          _dev(gpos), _dev(gfin), rec_off, rec_row, rec_val, need + spare)
    extra = 2 if flags & GS.PAIR else 0
    assert np.array_equal(rec_off.cpu().numpy(), np.concatenate([[0], np.cumsum(sc.sizes[sel] + extra)]))
    return rec_row, rec_val


def _group_rows(sc, flags, sel, pp, gp_active, gf_active, spare=5):
    """Program order of k_group_loss_bwd: wave s returns early when neither term has a gradient; else its members in index
    order, then (PAIR) ra, rb when the positive term has one."""
    out = []
    for s, g in enumerate(sel):
        rows = sc.index[sc.goff[g]:sc.goff[g + 1]]
        live = gp_active[s] or gf_active[s]
        out += list(rows) if live else [-1] * len(rows)
        if flags & GS.PAIR:
            out += [rows[pp[s, 0]], rows[pp[s, 1]]] if gp_active[s] else [-1, -1]
    return np.array(out + [-1] * spare, dtype=np.int32)


@pytest.mark.parametrize("scale", GS.SCALES)
@pytest.mark.parametrize("c,flags", GROUP_CASES)
def test_group_loss_records_order_replay_and_oracle(c, flags, scale):
    sc = GS.case_scene(c, flags, scale)
    sel, pp, gpos, gfin, _ = GS.without(sc, sc.all_s if flags & GS.BLOCK else None)
    pos, fin = _group_fwd(sc, flags, sel, pp)
    assert (pos > 0).any() and (pos == 0).any()
    rec_row_d, rec_val_d = _group_emit(sc, flags, sel, pp, gpos, gfin)
    want_rows = _group_rows(sc, flags, sel, pp, pos > 0, fin > 0)
    assert (want_rows[:-5] == -1).any() and (want_rows >= 0).any()               # some wave returns early / skips its pair
    rec_row, rec_val, _ = _check_chain(rec_row_d, rec_val_d, sc.prefill, want_rows)
    _, cnt = named(rec_row, len(sc.F))
    assert cnt.max() >= 2                                                         # shared rows: the order matters
    want = GO.group_terms(sc.F, sc.index, sc.goff, sc.flag, sel, GS.POS_THRESH, GS.FIN_THRESH, flags, pp)
    _check_oracle("group", scale, rec_row, rec_val, want.grad(gpos, gfin))
    # upstream gradients of zero switch a term off like an inactive hinge does: (a) and (b) again
    gpos0, gfin0 = gpos.copy(), gfin.copy()
    gpos0[::3], gfin0[::2] = 0, 0
    rec_row_d, rec_val_d = _group_emit(sc, flags, sel, pp, gpos0, gfin0)
    z = np.arange(len(sel))
    _check_chain(rec_row_d, rec_val_d, sc.prefill,
                 _group_rows(sc, flags, sel, pp, (pos > 0) & (z % 3 != 0), (fin > 0) & (z % 2 != 0)))


def _circle_emit(sc, flags, gpos, gfin, gmean, spare=5):
    n_sel, members = len(sc.sel), int(sc.sizes[sc.sel].sum())
    need = _lib_call("gcl_circle_group_records", members, n_sel, int(flags))
    extra = 3 if flags & GS.PAIR else 1
    assert need == members + extra * n_sel
    rec_row, rec_val = _records(need + spare, sc.c)
    rec_off = torch.full((n_sel + 1,), -9, dtype=torch.int32, device=DEV)
    _call("gcl_circle_group_bwd_emit", *_scene_args(sc), _dev(sc.sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE,
          int(flags), _dev(sc.pairpos), _dev(gpos), _dev(gfin), _dev(gmean), rec_off, rec_row, rec_val, need + spare)
    assert np.array_equal(rec_off.cpu().numpy(), np.concatenate([[0], np.cumsum(sc.sizes[sc.sel] + extra)]))
    return rec_row, rec_val


def _circle_rows(sc, flags, gpos, spare=5):
    """Program order of k_circle_group_bwd: the members, the finest member (first flagged position), then (PAIR) ra, rb when
    the positive term's upstream gradient is not zero.  No wave returns early."""
    out = []
    for s, g in enumerate(sc.sel):
        b, e = sc.goff[g], sc.goff[g + 1]
        rows = sc.index[b:e]
        fl = np.nonzero(sc.flag[b:e])[0]
        out += list(rows) + [rows[fl[0] if len(fl) else 0]]
        if flags & GS.PAIR:
            out += [rows[sc.pairpos[s, 0]], rows[sc.pairpos[s, 1]]] if gpos[s] != 0 else [-1, -1]
    return np.array(out + [-1] * spare, dtype=np.int32)


@pytest.mark.parametrize("scale", GS.SCALES)
@pytest.mark.parametrize("c,flags", CIRCLE_CASES)
def test_circle_group_records_order_replay_and_oracle(c, flags, scale):
    sc = GS.case_scene(c, flags, scale)
    want = GO.circle_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE, flags,
                           sc.pairpos)
    for gmean in (sc.gmean, None):
        rec_row_d, rec_val_d = _circle_emit(sc, flags, sc.gpos, sc.gfin, gmean)
        rec_row, rec_val, _ = _check_chain(rec_row_d, rec_val_d, sc.prefill, _circle_rows(sc, flags, sc.gpos))
        _check_oracle("circle", scale, rec_row, rec_val, want.grad(sc.gpos, sc.gfin, gmean))
    gpos0 = sc.gpos.copy()
    gpos0[::3] = 0
    rec_row_d, rec_val_d = _circle_emit(sc, flags, gpos0, sc.gfin, None)
    _check_chain(rec_row_d, rec_val_d, sc.prefill, _circle_rows(sc, flags, gpos0))


def _disjoint_selection(sc):
    """Selected groups of the scene with no row in common and no row twice inside a group."""
    seen, keep = set(), []
    for s, g in enumerate(sc.sel):
        rows = sc.index[sc.goff[g]:sc.goff[g + 1]].tolist()
        if len(set(rows)) == len(rows) and not (set(rows) & seen):
            seen |= set(rows)
            keep.append(s)
    return np.array(keep)


@pytest.mark.parametrize("c,flags", [(c, f) for c, f in GROUP_CASES if not f & GS.PAIR])
def test_group_loss_one_record_per_row_equals_the_atomic_entry(c, flags):
    sc = GS.case_scene(c, flags, 1.0)
    ks = _disjoint_selection(sc)
    if flags & GS.BLOCK:
        ks = ks[ks != sc.all_s]
    sel, gpos, gfin = sc.sel[ks], sc.gpos[ks], sc.gfin[ks]
    assert len(sel) >= 10
    rec_row_d, rec_val_d = _group_emit(sc, flags, sel, None, gpos, gfin)
    rec_row = rec_row_d.cpu().numpy()
    _, cnt = named(rec_row, len(sc.F))
    assert cnt.max() == 1 and cnt.sum() >= 10                             # every touched row: exactly one record
    zero = np.zeros_like(sc.prefill)
    got = _reduce(rec_row_d, rec_val_d, zero)
    dF = _dev(zero)
    _call("gcl_group_loss_bwd", *_scene_args(sc), _dev(sel), len(sel), GS.POS_THRESH, GS.FIN_THRESH, int(flags), None,
          _dev(gpos), _dev(gfin), dF)
    atomic = dF.cpu().numpy()
    assert np.any(atomic != 0) and (got == atomic).all(), int((got != atomic).sum())


@pytest.mark.parametrize("c,flags", [(c, f) for c, f in CIRCLE_CASES if not f & GS.PAIR])
def test_circle_group_at_most_two_records_per_row_equals_the_atomic_entry(c, flags):
    sc = GS.case_scene(c, flags, 1.0)
    ks = _disjoint_selection(sc)
    sub = GS.types.SimpleNamespace(**{**vars(sc), "sel": sc.sel[ks], "pairpos": None})
    gpos, gfin, gmean = sc.gpos[ks], sc.gfin[ks], sc.gmean[ks]
    assert len(sub.sel) >= 10
    rec_row_d, rec_val_d = _circle_emit(sub, flags, gpos, gfin, gmean)
    rec_row = rec_row_d.cpu().numpy()
    _, cnt = named(rec_row, len(sc.F))
    assert cnt.max() == 2 and (cnt == 2).sum() == len(sub.sel)            # a member's record and, for the finest, the collected one
    zero = np.zeros_like(sc.prefill)                                      # two addends into zero: their order cannot show
    got = _reduce(rec_row_d, rec_val_d, zero)
    dF = _dev(zero)
    _call("gcl_circle_group_bwd", *_scene_args(sc), _dev(sub.sel), len(sub.sel), GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE,
          int(flags), None, _dev(gpos), _dev(gfin), _dev(gmean), dF)
    atomic = dF.cpu().numpy()
    assert np.any(atomic != 0) and (got == atomic).all(), int((got != atomic).sum())


# ---- the negative term ------------------------------------------------------------------------------------------------------
def _neg_fwd(dmin, keep, thresh=GS.NEG_THRESH):
    out = torch.empty(2, device=DEV)
    _call("gcl_neg_loss_fwd", _dev(dmin), _dev(keep), len(dmin), thresh, out)
    return out


def _neg_emit(F, c, sel1, sel2, arg, dmin, keep, out, gneg, spare=3):
    m = len(sel1)
    need = _lib_call("gcl_neg_loss_records", m)
    assert need == 2 * m
    rec_row, rec_val = _records(need + spare, c)
    _call("gcl_neg_loss_bwd_emit", _dev(F), c, _dev(sel1), _dev(sel2), _dev(arg), _dev(dmin), _dev(keep), m, GS.NEG_THRESH, out,
          _dev(np.array([gneg], dtype=np.float32)), rec_row, rec_val, need + spare)
    return rec_row, rec_val


def _neg_rows(sel1, sel2, arg, dmin, keep, spare=3, thresh=GS.NEG_THRESH):
    """r ascending, sel1[r] before sel2[arg[r]]; -1 for a masked row and for an inactive hinge (fp32, as the kernel)"""
    active = (keep != 0) & (np.float32(thresh) - dmin.astype(np.float32) > 0)
    rows = np.stack([sel1, sel2[arg]], 1)
    rows[~active] = -1
    return np.concatenate([rows.reshape(-1), [-1] * spare]).astype(np.int32)


@pytest.mark.parametrize("c", (1, 33, 64))
@pytest.mark.parametrize("m", (255, 256, 257))
def test_neg_loss_records_order_replay_and_oracle(m, c):
    ns = GS.neg_scene(m, c)
    out = _neg_fwd(ns.dmin, ns.keep)
    rec_row_d, rec_val_d = _neg_emit(ns.F, c, ns.sel1, ns.sel2, ns.arg, ns.dmin, ns.keep, out, ns.gneg)
    want_rows = _neg_rows(ns.sel1, ns.sel2, ns.arg, ns.dmin, ns.keep)
    assert (want_rows[:2 * m] == -1).any() and (want_rows >= 0).any() and (ns.keep == 0).any()
    rec_row, rec_val, _ = _check_chain(rec_row_d, rec_val_d, ns.prefill, want_rows)
    assert named(rec_row, len(ns.F))[1].max() >= 2
    _check_oracle("neg", 1.0, rec_row, rec_val,
                  GO.neg_loss_grad(ns.F, ns.sel1, ns.sel2, ns.arg, ns.keep, GS.NEG_THRESH, ns.gneg))


@pytest.mark.parametrize("c", (1, 33, 64))
def test_neg_loss_one_record_per_row_equals_the_atomic_entry(c):
    """distinct sel1, an injective arg, sel1 and sel2 disjoint: every row is named at most once"""
    ns = GS.neg_scene(257, c)
    rng = np.random.RandomState(c)
    m, perm = 120, rng.permutation(len(ns.F))
    sel1, sel2, arg = perm[:m].astype(np.int64), perm[m:2 * m].astype(np.int64), rng.permutation(m).astype(np.int32)
    keep = (rng.rand(m) < 0.8).astype(np.uint8)
    dmin = GO.dmin_of(ns.F, sel1, sel2, arg).astype(np.float32)
    out = _neg_fwd(dmin, keep)
    rec_row_d, rec_val_d = _neg_emit(ns.F, c, sel1, sel2, arg, dmin, keep, out, ns.gneg)
    _, cnt = named(rec_row_d.cpu().numpy(), len(ns.F))
    assert cnt.max() == 1 and cnt.sum() >= 20
    zero = np.zeros_like(ns.prefill)
    got = _reduce(rec_row_d, rec_val_d, zero)
    dF = _dev(zero)
    _call("gcl_neg_loss_bwd", _dev(ns.F), c, _dev(sel1), _dev(sel2), _dev(arg), _dev(dmin), _dev(keep), m, GS.NEG_THRESH, out,
          _dev(np.array([ns.gneg], dtype=np.float32)), dF)
    atomic = dF.cpu().numpy()
    assert np.any(atomic != 0) and (got == atomic).all()


def test_group_loss_then_negative_term_share_one_list():
    """Two entries into one dF, as _GCLLossFn.backward_terms calls them: the lists one after the other in call order, one
    reduction; rows named by both entries get the group loss's records first."""
    c, flags = 32, 0
    sc = GS.case_scene(c, flags, 1.0)
    rng = np.random.RandomState(5)
    m, n_rows = 256, len(sc.F)
    sel1, sel2 = rng.choice(n_rows, m, replace=False).astype(np.int64), rng.choice(n_rows, m, replace=False).astype(np.int64)
    arg = rng.randint(0, m, m).astype(np.int32)
    keep = (sel1 != sel2[arg]).astype(np.uint8)
    dmin = GO.dmin_of(sc.F, sel1, sel2, arg).astype(np.float32)
    thresh = 1.5                              # unit rows: random pairs lie about sqrt(2) apart, on both sides of it
    out = _neg_fwd(dmin, keep, thresh)
    n_sel, members = len(sc.sel), int(sc.sizes[sc.sel].sum())
    cap_g, cap_n = members, 2 * m
    rec_row, rec_val = _records(cap_g + cap_n, c)
    rec_off = torch.empty(n_sel + 1, dtype=torch.int32, device=DEV)
    _call("gcl_group_loss_bwd_emit", *_scene_args(sc), _dev(sc.sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, flags, None,
          _dev(sc.gpos), _dev(sc.gfin), rec_off, rec_row, rec_val, cap_g)
    _call("gcl_neg_loss_bwd_emit", _dev(sc.F), c, _dev(sel1), _dev(sel2), _dev(arg), _dev(dmin), _dev(keep), m, thresh,
          out, _dev(np.array([0.9], dtype=np.float32)), rec_row[cap_g:], rec_val[cap_g:], cap_n)
    pos, fin = _group_fwd(sc, flags, sc.sel, None)
    want_rows = np.concatenate([_group_rows(sc, flags, sc.sel, None, pos > 0, fin > 0, spare=0),
                                _neg_rows(sel1, sel2, arg, dmin, keep, spare=0, thresh=thresh)])
    rr, _, _ = _check_chain(rec_row, rec_val, sc.prefill, want_rows)
    both = np.intersect1d(rr[:cap_g][rr[:cap_g] >= 0], rr[cap_g:][rr[cap_g:] >= 0])
    assert len(both) >= 5


# ---- the pair family --------------------------------------------------------------------------------------------------------
def _unit_rows(seed, n, c):
    f = np.random.RandomState(seed).normal(size=(n, c))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _two_lists(n_rec, c):
    return _records(n_rec, c), _records(n_rec, c)


def _triplet_run(F0, F1, ap, neg, tag, keep, margin, g, spare=4):
    m, c = len(ap), F0.shape[1]
    a = (_dev(F0), len(F0), _dev(F1), len(F1), c, _dev(ap), _dev(neg), _dev(tag), _dev(keep))
    work, out = torch.empty(3 * m, device=DEV), torch.empty(20, device=DEV)
    _call("gcl_triplet_fwd", *a, m, margin, work, out)
    need = _lib_call("gcl_triplet_records", m)
    assert need == 3 * m
    (r0, v0), (r1, v1) = _two_lists(need + spare, c)
    gd = _dev(np.array([g], dtype=np.float32))
    _call("gcl_triplet_bwd_emit", *a, m, work, out, gd, r0, v0, r1, v1, need + spare)
    d0, d1 = torch.zeros(F0.shape, device=DEV), torch.zeros(F1.shape, device=DEV)
    _call("gcl_triplet_bwd", *a, m, work, out, gd, d0, d1)
    return work.cpu().numpy(), (r0, v0), (r1, v1), d0.cpu().numpy(), d1.cpu().numpy()


def _triplet_rows(ap, neg, side, keep, work, m, spare=4):
    """triplet t ascending: anchor (its cloud's list), positive, negative (the other cloud's list); -1 for a masked, inactive
    or dropped triplet (work[t] = the forward's hinge, -1 for a row outside its cloud) and in the other list's slot"""
    lists = np.full((2, 3 * m + spare), -1, dtype=np.int64)
    for t in range(m):
        if (keep is not None and not keep[t]) or not work[t] > 0:
            continue
        s = int(side[t])
        lists[s, 3 * t] = ap[t, s]
        lists[1 - s, 3 * t + 1] = ap[t, 1 - s]
        lists[1 - s, 3 * t + 2] = neg[t]
    return lists.astype(np.int32)


def _triplet_case(seed, c, m, n0=150, n1=130):
    rng = np.random.RandomState(seed)
    F0, F1 = _unit_rows(seed, n0, c), _unit_rows(seed + 1, n1, c)
    ap = np.stack([rng.randint(0, n0, m), rng.randint(0, n1, m)], 1).astype(np.int64)
    side = rng.randint(0, 2, m)
    neg = np.where(side == 1, rng.randint(0, n0, m), rng.randint(0, n1, m)).astype(np.int64)
    tag = (side | (rng.randint(0, 3, m) << 1)).astype(np.uint8)
    keep = (rng.rand(m) < 0.7).astype(np.uint8)
    return F0, F1, ap, neg, side, tag, keep


@pytest.mark.parametrize("c", PAIR_WIDTHS)
def test_triplet_records_order_replay_and_oracle(c):
    m, margin, g = 333, 0.4, 0.7
    F0, F1, ap, neg, side, tag, keep = _triplet_case(100 + c, c, m)
    bad = np.arange(0, m, 11)                                             # row ids outside their cloud: dropped, never read
    ap[bad[::3], 0], neg[bad[1::3]], ap[bad[2::3], 1] = 10 ** 12, -1, len(F0) + len(F1)
    work, l0, l1, _, _ = _triplet_run(F0, F1, ap, neg, tag, keep, margin, g)
    want_rows = _triplet_rows(ap, neg, side, keep, work, m)
    assert (work[:m][bad] == -1).all() and (work[:m] > 0).any()
    valid = np.ones(m, dtype=bool)
    valid[bad] = False
    k = (keep != 0) & valid
    ap_ok, neg_ok = np.where(valid[:, None], ap, 0), np.where(valid, neg, 0)
    D0, D1 = torch.from_numpy(F0).double().requires_grad_(True), torch.from_numpy(F1).double().requires_grad_(True)
    h, _, _ = PO.triplet_terms(D0, D1, ap_ok, neg_ok, side, margin)
    (g * h[torch.from_numpy(k)].mean()).backward()
    for (r_d, v_d), F, want, D in ((l0, F0, want_rows[0], D0), (l1, F1, want_rows[1], D1)):
        prefill = (((np.arange(F.size) % 5) + 1) / 32.0).astype(np.float32).reshape(F.shape)
        rec_row, rec_val, _ = _check_chain(r_d, v_d, prefill, want)
        assert named(rec_row, len(F))[1].max() >= 2
        err = GS.rel_l2(row_sums64(rec_row, rec_val, len(F)), D.grad.numpy())
        assert err < PAIR_TOL, err
    # no keep mask: every valid triplet
    work, l0, l1, _, _ = _triplet_run(F0, F1, ap, neg, tag, None, margin, g)
    want_rows = _triplet_rows(ap, neg, side, None, work, m)
    assert np.array_equal(l0[0].cpu().numpy(), want_rows[0]) and np.array_equal(l1[0].cpu().numpy(), want_rows[1])


@pytest.mark.parametrize("c", PAIR_WIDTHS)
def test_triplet_one_record_per_row_equals_the_atomic_entry(c):
    """every row of either cloud is used by at most one triplet, in one role"""
    m, n0, n1 = 60, 200, 200
    rng = np.random.RandomState(c)
    F0, F1 = _unit_rows(c, n0, c), _unit_rows(c + 1, n1, c)
    p0, p1 = rng.permutation(n0), rng.permutation(n1)
    side = rng.randint(0, 2, m)
    ap = np.stack([p0[:m], p1[:m]], 1).astype(np.int64)
    neg = np.where(side == 1, p0[m:2 * m], p1[m:2 * m]).astype(np.int64)
    keep = (rng.rand(m) < 0.8).astype(np.uint8)
    work, l0, l1, d0, d1 = _triplet_run(F0, F1, ap, neg, side.astype(np.uint8), keep, 0.4, 1.3)
    for (r_d, v_d), F, atomic in ((l0, F0, d0), (l1, F1, d1)):
        _, cnt = named(r_d.cpu().numpy(), len(F))
        assert cnt.max() == 1 and cnt.sum() >= 10
        got = _reduce(r_d, v_d, np.zeros(F.shape, dtype=np.float32))
        assert np.any(atomic != 0) and (got == atomic).all()


def _pairs_run(F0, F1, pairs, keep, mode, thresh, eps, g, spare=4):
    m, c = len(pairs), F0.shape[1]
    a = (_dev(F0), len(F0), _dev(F1), len(F1), c, _dev(pairs), _dev(keep), m, mode, thresh, eps)
    work, out = torch.empty(m, device=DEV), torch.empty(2, device=DEV)
    _call("gcl_pair_terms_fwd", *a, work, out)
    need = _lib_call("gcl_pair_terms_records", m)
    assert need == m
    (r0, v0), (r1, v1) = _two_lists(need + spare, c)
    gd = _dev(np.array([g], dtype=np.float32))
    _call("gcl_pair_terms_bwd_emit", *a, work, out, gd, r0, v0, r1, v1, need + spare)
    d0, d1 = torch.zeros(F0.shape, device=DEV), torch.zeros(F1.shape, device=DEV)
    _call("gcl_pair_terms_bwd", *a, work, out, gd, d0, d1)
    return work.cpu().numpy(), (r0, v0), (r1, v1), d0.cpu().numpy(), d1.cpu().numpy()


def _pairs_rows(pairs, keep, work, mode, thresh, eps, spare=4):
    """pair t: slot t of list 0 (row of F0) and of list 1 (row of F1); -1 for a masked or dropped pair (work = -1) and for an
    inactive hinge, decided in fp32 from the forward's d2 as the kernel decides it"""
    m = len(pairs)
    d2 = work.astype(np.float32)
    if mode == 0:
        active = np.ones(m, dtype=bool)
    elif mode == 1:
        active = d2 - np.float32(thresh) > 0
    else:
        active = np.float32(thresh) - np.sqrt(np.maximum(d2, 0) + np.float32(eps), dtype=np.float32) > 0
    active &= (d2 >= 0) & ((keep != 0) if keep is not None else True)
    lists = np.full((2, m + spare), -1, dtype=np.int64)
    lists[0, :m][active], lists[1, :m][active] = pairs[active, 0], pairs[active, 1]
    return lists.astype(np.int32)


@pytest.mark.parametrize("mode,thresh,eps", [(0, 0.0, 0.0), (1, 1.9, 0.0), (2, 1.4, 1e-4), (2, 1.4, 1e-7)])
@pytest.mark.parametrize("c", PAIR_WIDTHS)
def test_pair_terms_records_order_replay_and_oracle(mode, thresh, eps, c):
    m, g, n0, n1 = 333, 1.3, 150, 130
    rng = np.random.RandomState(7 * c + mode)
    F0, F1 = _unit_rows(c + 50, n0, c), _unit_rows(c + 51, n1, c)
    pairs = np.stack([rng.randint(0, n0, m), rng.randint(0, n1, m)], 1).astype(np.int64)
    bad = np.arange(0, m, 13)
    pairs[bad[::2], 0], pairs[bad[1::2], 1] = -3, n1
    keep = (rng.rand(m) < 0.6).astype(np.uint8)
    work, l0, l1, _, _ = _pairs_run(F0, F1, pairs, keep, mode, thresh, eps, g)
    assert (work[bad] == -1).all()
    want_rows = _pairs_rows(pairs, keep, work, mode, thresh, eps)
    valid = np.ones(m, dtype=bool)
    valid[bad] = False
    k = (keep != 0) & valid
    if mode:
        assert (want_rows[0][:m][k] == -1).any() and (want_rows[0][:m][k] >= 0).any()       # both sides of the hinge
    D0, D1 = torch.from_numpy(F0).double().requires_grad_(True), torch.from_numpy(F1).double().requires_grad_(True)
    terms = PO.pair_term(D0, D1, pairs[k], {0: "sq", 1: "sq_pos", 2: "neg"}[mode], thresh, eps)
    (g * terms.mean()).backward()
    for (r_d, v_d), F, want, D in ((l0, F0, want_rows[0], D0), (l1, F1, want_rows[1], D1)):
        prefill = (((np.arange(F.size) % 5) + 1) / 32.0).astype(np.float32).reshape(F.shape)
        rec_row, rec_val, _ = _check_chain(r_d, v_d, prefill, want)
        assert named(rec_row, len(F))[1].max() >= 2
        err = GS.rel_l2(row_sums64(rec_row, rec_val, len(F)), D.grad.numpy())
        assert err < PAIR_TOL, err
    work, l0, l1, _, _ = _pairs_run(F0, F1, pairs, None, mode, thresh, eps, g)
    want_rows = _pairs_rows(pairs, None, work, mode, thresh, eps)
    assert np.array_equal(l0[0].cpu().numpy(), want_rows[0]) and np.array_equal(l1[0].cpu().numpy(), want_rows[1])


@pytest.mark.parametrize("mode,thresh,eps", [(0, 0.0, 0.0), (1, 1.9, 0.0), (2, 1.4, 1e-7)])
@pytest.mark.parametrize("c", PAIR_WIDTHS)
def test_pair_terms_one_record_per_row_equals_the_atomic_entry(mode, thresh, eps, c):
    m, n0, n1 = 100, 150, 130
    rng = np.random.RandomState(c + mode)
    F0, F1 = _unit_rows(c + 60, n0, c), _unit_rows(c + 61, n1, c)
    pairs = np.stack([rng.permutation(n0)[:m], rng.permutation(n1)[:m]], 1).astype(np.int64)
    keep = (rng.rand(m) < 0.8).astype(np.uint8)
    _, l0, l1, d0, d1 = _pairs_run(F0, F1, pairs, keep, mode, thresh, eps, 0.9)
    for (r_d, v_d), F, atomic in ((l0, F0, d0), (l1, F1, d1)):
        _, cnt = named(r_d.cpu().numpy(), len(F))
        assert cnt.max() == 1 and cnt.sum() >= 10
        got = _reduce(r_d, v_d, np.zeros(F.shape, dtype=np.float32))
        assert np.any(atomic != 0) and (got == atomic).all()
