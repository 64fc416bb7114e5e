"""Every loss kernel of csrc/loss.hip but the 1-NN search (tests/test_gpu_sc2_bench.py has that one), called through the
C ABI and compared PER GROUP and PER ROW with the fp64 reference of tests/group_loss_oracle.py:

  gcl_group_loss_fwd / _bwd    all 16 switch sets, widths 1 .. 64 (the lane < c guard inside and at the edge of a half-wave)
  gcl_circle_group_fwd / _bwd  all 8 switch sets, the same widths, the gradient at the means given and NULL
  gcl_neg_mask                 every kind of (row, target) pair, byte for byte
  gcl_neg_loss_fwd / _bwd, gcl_loss_combine, gcl_loss_seed    at the edges of their 256-thread reductions
  finest_contrastive_loss(total_weights=...)                  at 16 and 64 channels against oracle/loss_oracle.py

Inputs: tests/group_loss_scenes.py (~350 rows, ~30 groups of 1 .. 70 members, shared rows, both sides of every hinge, unit
norm and scaled by 4); their conditions are asserted on the CPU in tests/test_oracle_group_loss.py.  The gradient buffer
arrives pre-filled: the kernels accumulate, rows outside the selected groups come back bit for bit.

Tolerances.  On unit-norm rows the project's own: 2e-6 absolute on a term and 1e-5 rel-L2 on dF (contrastive loss), 1e-5
relative and 1e-4 rel-L2 (circle loss: exp / log chains).  The scaled scenes and the per-row check
|got - want| <= tol (|want| + largest row norm of want) have none, so they are MEASURED: the same oracle evaluated in fp32
on the CPU over the whole case set (test_oracle_group_loss.py::fp32_oracle_errors), its largest error against fp64 per
quantity, times 8 -- the kernels sum the members serially and accumulate with float atomics in arbitrary order, which may
lose a few more bits than torch's pairwise sums."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402
import group_loss_oracle as GO                                         # noqa: E402
import group_loss_scenes as GS                                         # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23

# (family, quantity, scale of the rows): the fp32 oracle's largest error against the fp64 oracle, measured on the CPU
MEASURED = {                                               # measured            -> tolerance = 8 x
    ("group", "term", 1.0): 3.460e-07,                     # (the project's 2e-6 applies instead)
    ("group", "df", 1.0): 1.120e-07,                       # (the project's 1e-5 applies instead)
    ("group", "row", 1.0): 7.866e-08,                      # 6.293e-07
    ("group", "term", 4.0): 2.073e-07,                     # 1.658e-06
    ("group", "df", 4.0): 1.071e-07,                       # 8.568e-07
    ("group", "row", 4.0): 6.938e-08,                      # 5.550e-07
    ("circle", "term", 1.0): 3.637e-07,                    # (the project's 1e-5 applies instead)
    ("circle", "df", 1.0): 5.699e-06,                      # (the project's 1e-4 applies instead)
    ("circle", "row", 1.0): 4.790e-06,                     # 3.832e-05
    ("circle", "term", 4.0): 3.704e-07,                    # 2.963e-06
    ("circle", "df", 4.0): 3.384e-04,                      # 2.707e-03
    ("circle", "row", 4.0): 4.629e-04,                     # 3.703e-03
    ("neg", "df", 1.0): 4.572e-06,                         # 3.658e-05  (rows not of unit norm, the hinge 1e-4 away)
    ("neg", "row", 1.0): 1.850e-06,                        # 1.480e-05
}
TOL = {k: 8 * v for k, v in MEASURED.items()}
# the project's own tolerances where they already apply: unit-norm rows, a term and the rel-L2 of dF
PROJECT = {("group", "term", 1.0): 2e-6, ("group", "df", 1.0): 1e-5,          # test_finest_contrastive_loss_golden
           ("circle", "term", 1.0): 1e-5, ("circle", "df", 1.0): 1e-4}        # test_location_circle_loss_golden


def _tol(fam, what, scale):
    key = (fam, what, float(scale))
    return PROJECT.get(key, TOL[key])


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(entry, *args):
    from gcl_amd import _lib
    lib = _lib.load()
    with torch.cuda.device(DEV):
        a = [_lib.ptr(x) if (x is None or torch.is_tensor(x)) else x for x in args]
        _lib.check(getattr(lib, entry)(*a, _lib.stream()), entry)
        torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy()


def _scene_args(sc):
    return _dev(sc.F), sc.c, _dev(sc.index), _dev(sc.goff), _dev(sc.flag)


def _check_terms(fam, scale, got, want, what):
    """A term per group: absolute on unit-norm rows (relative to max(1, |want|) where the project's tolerance is), relative
    to max(1, |want|) on the scaled rows."""
    tol = _tol(fam, "term", scale)
    rel = np.maximum(1, np.abs(want)) if (scale > 1 or fam == "circle") else 1
    err = np.abs(got.astype(np.float64) - want) / rel
    print(f"  {what}: max err {err.max():.3e} (tol {tol:.3e})")
    assert np.isfinite(got).all() and (err <= tol).all(), (what, int(err.argmax()), err.max(), tol)


def _check_df(fam, sc, sel, got, want, prefill=None):
    prefill = sc.prefill if prefill is None else prefill
    out = ~GS.touched(sc, sel) if sel is not None else (np.linalg.norm(want, axis=1) == 0)
    assert out.sum() * 3 >= len(out) or sel is None
    assert got[out].tobytes() == prefill[out].tobytes(), "a row outside the selected groups changed"
    diff = got.astype(np.float64) - prefill
    e_all, e_row = GS.rel_l2(diff, want), GS.row_error(diff, want)
    scale = getattr(sc, "scale", 1.0)
    print(f"  dF: rel-L2 {e_all:.3e} (tol {_tol(fam, 'df', scale):.3e}), per row {e_row:.3e} (tol {_tol(fam, 'row', scale):.3e})")
    assert np.linalg.norm(want) > 0 and np.isfinite(got).all()
    assert e_all <= _tol(fam, "df", scale), e_all
    assert e_row <= _tol(fam, "row", scale), e_row


# ---- gcl_group_loss_fwd / _bwd -----------------------------------------------------------------------------------------
def _group_fwd(sc, flags, sel, pp):
    n_sel = len(sel)
    pos, fin = torch.full((n_sel,), -7.0, device=DEV), torch.full((n_sel,), -7.0, device=DEV)
    _call("gcl_group_loss_fwd", *_scene_args(sc), _dev(sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, int(flags), _dev(pp),
          pos, fin)
    return _host(pos), _host(fin)


@pytest.mark.parametrize("scale", GS.SCALES)
@pytest.mark.parametrize("c,flags", GS.GROUP_CASES)
def test_group_loss_per_group_and_per_row(c, flags, scale):
    sc = GS.case_scene(c, flags, scale)
    sel, pp, gpos, gfin, _ = GS.without(sc, sc.all_s if flags & GS.BLOCK else None)     # the all-flagged group: below
    want = GO.group_terms(sc.F, sc.index, sc.goff, sc.flag, sel, GS.POS_THRESH, GS.FIN_THRESH, flags, pp)
    assert (want.pos > 0).any() and (want.pos == 0).any()                          # both sides of the hinge
    pos, fin = _group_fwd(sc, flags, sel, pp)
    _check_terms("group", scale, pos, want.pos, "pos")
    if flags & GS.NOFIN:
        assert (fin == 0).all() and (want.fin == 0).all()
    else:
        assert (want.fin > 0).any() and (want.fin == 0).any()
        _check_terms("group", scale, fin, want.fin, "fin")
    assert ((pos == 0) == (want.pos == 0)).all() and ((fin == 0) == (want.fin == 0)).all()
    dF = _dev(sc.prefill)
    _call("gcl_group_loss_bwd", *_scene_args(sc), _dev(sel), len(sel), GS.POS_THRESH, GS.FIN_THRESH, int(flags), _dev(pp),
          _dev(gpos), _dev(gfin), dF)
    _check_df("group", sc, sel, _host(dF), want.grad(gpos, gfin))                   # NOFIN: gfin contributes nothing


@pytest.mark.parametrize("scale", GS.SCALES)
@pytest.mark.parametrize("c,flags", [(c, f) for c, f in GS.GROUP_CASES if f & GS.BLOCK])
def test_group_loss_fwd_on_an_all_flagged_group_is_nan_like_the_reference(c, flags, scale):
    """BLOCK takes the mean of the NON-finest members (lib/colocation_trainer.py:479-481): of an empty set when every member
    is flagged, which is NaN in the reference.  Only that group's finest term is; forward only."""
    sc = GS.case_scene(c, flags, scale)
    want = GO.group_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, GS.POS_THRESH, GS.FIN_THRESH, flags, sc.pairpos)
    pos, fin = _group_fwd(sc, flags, sc.sel, sc.pairpos)
    others = np.arange(len(sc.sel)) != sc.all_s
    _check_terms("group", scale, pos, want.pos, "pos")
    if flags & GS.NOFIN:
        assert (fin == 0).all()
    else:
        assert np.isnan(want.fin[sc.all_s]) and np.isnan(fin[sc.all_s])
        _check_terms("group", scale, fin[others], want.fin[others], "fin")


# ---- gcl_circle_group_fwd / _bwd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", GS.SCALES)
@pytest.mark.parametrize("c,flags", GS.CIRCLE_CASES)
def test_circle_group_per_group_and_per_row(c, flags, scale):
    """BLOCK|PAIR on unit-norm rows at 3, 31, 33 and 63 channels is the case that found k_circle_group_bwd reducing the pair's
    distance inside ``lane < c`` (lanes ended with partial sums at a width that is no power of two: dF off by 8e-3 .. 1.4e-2
    rel-L2, 1.2e-2 per row)."""
    sc = GS.case_scene(c, flags, scale)
    n_sel = len(sc.sel)
    want = GO.circle_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE, flags,
                           sc.pairpos)
    if scale > 1:
        a = want.fin_arg[np.isfinite(want.fin_arg)]
        assert (a > 20).any() and (a < 20).any()                                   # both branches of softplus
    pos, fin = torch.full((n_sel,), -7.0, device=DEV), torch.full((n_sel,), -7.0, device=DEV)
    mean = torch.full((n_sel, c), -7.0, device=DEV)
    cfg = (_dev(sc.sel), n_sel, GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE, int(flags), _dev(sc.pairpos))
    _call("gcl_circle_group_fwd", *_scene_args(sc), *cfg, pos, fin, mean)
    _check_terms("circle", scale, _host(pos), want.pos, "pos")
    _check_terms("circle", scale, _host(fin), want.fin, "fin")
    if flags & GS.BLOCK:                                   # logsumexp of an empty set is -inf: softplus gives 0
        assert want.fin[sc.all_s] == 0 and _host(fin)[sc.all_s] == 0
    # the mean of n members summed one after the other: (n - 1) roundings of the sum and one of the division
    n = sc.sizes[sc.sel].astype(np.float64)[:, None]
    assert (np.abs(_host(mean) - want.mean) <= n * 2.0 ** -24 * scale).all()
    for gmean in (sc.gmean, None):
        dF = _dev(sc.prefill)
        _call("gcl_circle_group_bwd", *_scene_args(sc), *cfg, _dev(sc.gpos), _dev(sc.gfin), _dev(gmean), dF)
        _check_df("circle", sc, sc.sel, _host(dF), want.grad(sc.gpos, sc.gfin, gmean))
    if flags & GS.BLOCK:                                   # ... and that group gets no finest-term gradient
        gfin = np.zeros(n_sel, dtype=np.float32)
        gfin[sc.all_s] = 3.0
        dF = _dev(sc.prefill)
        _call("gcl_circle_group_bwd", *_scene_args(sc), *cfg, _dev(np.zeros(n_sel, dtype=np.float32)), _dev(gfin), None, dF)
        assert _host(dF).tobytes() == sc.prefill.tobytes()


# ---- gcl_neg_mask ------------------------------------------------------------------------------------------------------
def _neg_mask(ms, index, goff):
    m = len(ms.sel1)
    cap = 64
    while cap < 2 * m:                                     # as _GCLLossFn.forward chooses it
        cap *= 2
    table = torch.full((cap, 2), 5, dtype=torch.int64, device=DEV)        # stale words: the call fills what it reads
    keep = torch.full((m,), 9, dtype=torch.uint8, device=DEV)
    _call("gcl_neg_mask", _dev(ms.sel1), _dev(ms.sel2), _dev(ms.arg), m, _dev(index), _dev(goff),
          0 if goff is None else len(goff) - 1, 0 if index is None else len(index), table, cap, keep)
    return _host(keep)


@pytest.mark.parametrize("m", GS.NEG_M)
def test_neg_mask_byte_for_byte(m):
    """(The ``target != row`` of k_neg_mask_scan cannot be told from its absence by any input: it is false only for a self
    pair, whose byte k_neg_mask_init has already cleared.)"""
    scenes = [GS.mask_scene(10 + m, m)] if m > 1 else [GS.mask_scene(10 + i, 1, only=k) for i, k in enumerate(GS.KINDS)]
    for ms in scenes:
        want = GO.neg_mask(ms.sel1, ms.sel2, ms.arg, ms.index, ms.goff, ms.n_rows)
        got = _neg_mask(ms, ms.index, ms.goff)
        assert got.tobytes() == want.tobytes(), {k: int(((got != want) & (ms.kind == k)).sum()) for k in GS.KINDS}
        # no group at all: only the self pairs are masked
        assert _neg_mask(ms, None, None).tobytes() == (ms.sel1 != ms.target).astype(np.uint8).tobytes()
        empty = GO.neg_mask(ms.sel1, ms.sel2, ms.arg, np.zeros(0, np.int64), np.zeros(1, np.int64), ms.n_rows)
        assert empty.tobytes() == (ms.sel1 != ms.target).astype(np.uint8).tobytes()


# ---- gcl_neg_loss_fwd / _bwd -------------------------------------------------------------------------------------------
def _neg_loss(ns, keep, c):
    m = len(ns.sel1)
    out = torch.full((2,), -7.0, device=DEV)
    dmin, keep_d = _dev(ns.dmin), _dev(keep)
    _call("gcl_neg_loss_fwd", dmin, keep_d, m, GS.NEG_THRESH, out)
    dF = _dev(ns.prefill)
    _call("gcl_neg_loss_bwd", _dev(ns.F), c, _dev(ns.sel1), _dev(ns.sel2), _dev(ns.arg), dmin, keep_d, m, GS.NEG_THRESH, out,
          _dev(np.array([ns.gneg], dtype=np.float32)), dF)
    return _host(out), _host(dF)


@pytest.mark.parametrize("m,c,side", GS.NEG_CASES)
def test_neg_loss_count_mean_and_gradient(m, c, side):
    ns = GS.neg_scene(m, c, side)
    d = ns.dmin[ns.keep != 0].astype(np.float64)
    assert (np.abs(GS.NEG_THRESH - d) > GS.MARGIN).all()
    assert ((d < GS.NEG_THRESH).any() and (d > GS.NEG_THRESH).any()) if m > 1 else ((d[0] < GS.NEG_THRESH) == side)
    val, cnt = GO.neg_loss(ns.dmin, ns.keep, GS.NEG_THRESH)
    out, dF = _neg_loss(ns, ns.keep, c)
    assert out[1] == cnt == int(ns.keep.sum())
    # <= 3 roundings per term, <= 3 serial and 8 tree additions, one division; every term is >= 0
    assert abs(out[0] - val) <= 16 * 2.0 ** -24 * val
    want = GO.neg_loss_grad(ns.F, ns.sel1, ns.sel2, ns.arg, ns.keep, GS.NEG_THRESH, ns.gneg)
    if np.linalg.norm(want) == 0:                          # one pair beyond the threshold
        assert m == 1 and not side and dF.tobytes() == ns.prefill.tobytes()
    else:
        _check_df("neg", ns, None, dF, want)
    # every row masked: the mean of an empty set, and nothing is accumulated
    out, dF = _neg_loss(ns, np.zeros(m, dtype=np.uint8), c)
    assert np.isnan(out[0]) and out[1] == 0 and dF.tobytes() == ns.prefill.tobytes()
    assert np.isnan(GO.neg_loss(ns.dmin, np.zeros(m, dtype=np.uint8), GS.NEG_THRESH)[0])


# ---- gcl_loss_combine / gcl_loss_seed -----------------------------------------------------------------------------------
W = (0.7, 1.3, 0.9)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("n_sel", (1, 255, 256, 257, 1000))
def test_loss_combine(n_sel):
    rng = np.random.RandomState(n_sel)
    pos, fin = (2 * rng.rand(n_sel)).astype(np.float32), rng.rand(n_sel).astype(np.float32)
    neg = np.array([0.37], dtype=np.float32)
    out = torch.full((4,), -7.0, device=DEV)
    _call("gcl_loss_combine", _dev(pos), _dev(fin), n_sel, _dev(neg), *W, out)
    out = _host(out)
    w32 = [float(np.float32(w)) for w in W]                                 # the weights as the entry receives them
    tot, pm, fm, ng = GO.combine(pos, fin, neg[0], w32)
    assert abs(out[1] - pm) <= 2 * _ulp(pm) and abs(out[2] - fm) <= 2 * _ulp(fm)
    assert abs(out[0] - tot) <= 4 * _ulp(abs(w32[0] * pm) + abs(w32[1] * fm) + abs(w32[2] * ng))
    assert out[3:].tobytes() == neg.tobytes()


@pytest.mark.parametrize("n_sel", (1, 255, 256, 257, 1000))
def test_loss_seed(n_sel):
    g = np.array([1.7], dtype=np.float32)
    seeds = torch.full((2 * n_sel + 3,), -7.0, device=DEV)                  # one spare word behind every output
    gpos, gfin, gneg = seeds[:n_sel], seeds[n_sel + 1:2 * n_sel + 1], seeds[2 * n_sel + 2:]
    _call("gcl_loss_seed", _dev(g), *W, n_sel, gpos, gfin, gneg)
    got = _host(seeds)
    w = [np.float32(x) for x in W]
    n = np.float32(n_sel)
    assert got[:n_sel].tobytes() == np.full(n_sel, (g[0] * w[0]) / n, dtype=np.float32).tobytes()
    assert got[n_sel + 1:2 * n_sel + 1].tobytes() == np.full(n_sel, (g[0] * w[1]) / n, dtype=np.float32).tobytes()
    assert got[2 * n_sel + 2] == g[0] * w[2]
    assert (got[[n_sel, 2 * n_sel + 1]] == -7.0).all()                      # nothing written past n_sel
    gp, gf, gn = GO.seed(g[0], W, n_sel)
    assert np.allclose(got[:n_sel], gp, rtol=4 * EPS) and np.allclose(got[n_sel + 1:2 * n_sel + 1], gf, rtol=4 * EPS)
    assert abs(got[2 * n_sel + 2] - gn) <= 4 * EPS * abs(gn)


# ---- the wrapper at the other head widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (16, 64))
def test_finest_contrastive_loss_total_at_width(c):
    """finest_contrastive_loss(total_weights=...) at 16 and 64 channels against oracle/loss_oracle.py in fp64, with the
    tolerances of test_finest_contrastive_loss_golden (2e-6 on a term, 1e-5 rel-L2 on dL/dF).  The negative rows are redrawn
    until every row's best and second-best fp64 distances differ by more than 4 (c + 2) 2^-23 relative
    (test_gpu_sc2_bench.py::_separated), so that the fp32 arg-minimum is the oracle's."""
    from gcl_amd.lib.colocation_trainer import finest_contrastive_loss
    from oracle import loss_oracle as LO
    sc = GS.scene(c, 1.0, False, False)
    rng = np.random.RandomState(c)
    n_rows = len(sc.F)
    while True:
        sel1, sel2 = rng.choice(n_rows, 200, replace=False), rng.choice(n_rows, 200, replace=False)
        d2, _, gap = EO.nn(sc.F[sel1], sc.F[sel2], with_gap=True)
        if (gap > 4 * (c + 2) * EPS * (d2 + gap)).all():
            break
    draws = (sc.sel, sel1, sel2)
    group, flag = sc.sizes.astype(np.int32), sc.flag.astype(bool)
    split = np.split(sc.index, sc.goff[1:-1])
    index_hash = LO.exhaustive_hash(split, n_rows)
    Fo = torch.from_numpy(sc.F).double().requires_grad_(True)
    po, fo, no = LO.finest_contrastive_loss(Fo, group, sc.index, index_hash, flag, draws=draws)
    (2.0 * (W[0] * po + W[1] * fo + W[2] * no)).backward()
    F = torch.from_numpy(sc.F).to(DEV).requires_grad_(True)
    with torch.cuda.device(DEV):
        tot, p1, f1, n1 = finest_contrastive_loss(F, torch.from_numpy(group), torch.from_numpy(sc.index), index_hash,
                                                  torch.from_numpy(flag), draws=draws, total_weights=W)
        (2.0 * tot).backward()
    assert abs(p1.item() - po.item()) < 2e-6 and abs(f1.item() - fo.item()) < 2e-6 and abs(n1.item() - no.item()) < 2e-6
    assert abs(tot.item() - (W[0] * po.item() + W[1] * fo.item() + W[2] * no.item())) < 2e-6
    assert po.item() > 0 and fo.item() > 0 and no.item() > 0
    err = GS.rel_l2(F.grad.cpu().numpy().astype(np.float64), Fo.grad.numpy())
    assert err < 1e-5, err
