"""Pins tests/group_loss_oracle.py (the per-group fp64 reference of the loss kernels) against the reference's recorded
outputs and against oracle/loss_oracle.py, asserts the conditions that tests/group_loss_scenes.py promises for the inputs
of tests/test_gpu_loss_kernels.py, and measures -- on the CPU, reproducibly -- the fp32 error of the same oracle over the
whole case set, from which that file's tolerances are taken."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_loss_oracle as GO                                         # noqa: E402
import group_loss_scenes as GS                                         # noqa: E402
from oracle import loss_oracle as L                                    # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FINEST = sorted(glob.glob(os.path.join(G, "finest_loss_*.npz")))
CIRCLE = sorted(glob.glob(os.path.join(G, "circle_loss_*.npz")))
_name = lambda p: os.path.basename(p)[:-4]


def _goff(group):
    return np.concatenate([[0], np.cumsum(np.asarray(group, dtype=np.int64))])


def _flags(z):
    return (0 if bool(z["square_loss"]) else GO.GL_SQRT) | (GO.GL_BLOCK if bool(z["block_finest_gradient"]) else 0) | \
        (GO.GL_PAIR if bool(z["use_pair_group_positive_loss"]) else 0) | \
        (0 if ("finest_term" not in z.files or bool(z["finest_term"])) else GO.GL_NOFIN)


def _fixture_nn(z):
    """The recorded case's hardest negatives as the reference found them (fp32, chunked: lib/eval.py:18-48)."""
    F = torch.from_numpy(z["F_out"])
    return L.find_nn(F[z["sel_hn1"]], F[z["sel_hn2"]], nn_max_n=500).numpy()


@pytest.mark.parametrize("path", FINEST, ids=_name)
def test_group_terms_on_the_finest_fixtures(path):
    z = np.load(path)
    flags, goff, n_sel = _flags(z), _goff(z["group"]), len(z["pos_sel"])
    pp = z["pair_pos"] if "pair_pos" in z.files else None
    t = GO.group_terms(z["F_out"], z["index"], goff, z["finest_flag"], z["pos_sel"], 0.1, 0.2, flags, pp)
    assert abs(t.pos.mean() - float(z["pos"])) <= 1e-6 * max(1, abs(float(z["pos"])))
    assert abs(t.fin.mean() - float(z["finest"])) <= 1e-6 * max(1, abs(float(z["finest"])))
    if flags & GO.GL_NOFIN:
        assert (t.fin == 0).all()
    # the positive + finest part of the gradient: oracle/loss_oracle.py's autograd (its negative term needs no full draw here)
    sw = {k: bool(z[k]) for k in ("square_loss", "block_finest_gradient", "use_pair_group_positive_loss", "finest_term")
          if k in z.files}
    Fo = torch.from_numpy(z["F_out"]).double().requires_grad_(True)
    po, fo, _ = L.finest_contrastive_loss(Fo, z["group"], z["index"], z["index_hash"], z["finest_flag"],
                                          draws=(z["pos_sel"], z["sel_hn1"][:8], z["sel_hn2"][:8], pp), **sw)
    (po + fo).backward()
    mine = t.grad(np.full(n_sel, 1.0 / n_sel), np.full(n_sel, 1.0 / n_sel))
    assert np.abs(mine - Fo.grad.numpy()).max() <= 1e-12
    # ... and with the negative term the recorded gradient
    if np.isnan(float(z["neg"])):
        return
    if "use_hard_negative" in z.files and not bool(z["use_hard_negative"]):
        Fo.grad = None
        draws = (z["pos_sel"], z["sel_hn1"], z["sel_hn2"], pp, z["random_cols"])
        neg = L.finest_contrastive_loss(Fo, z["group"], z["index"], z["index_hash"], z["finest_flag"], draws=draws,
                                        use_hard_negative=False, **sw)[2]
        neg.backward()
        g_neg = Fo.grad.numpy()
    else:
        arg = _fixture_nn(z)
        keep = GO.neg_mask(z["sel_hn1"], z["sel_hn2"], arg, z["index"], goff, len(z["F_out"]))
        val, cnt = GO.neg_loss(GO.dmin_of(z["F_out"], z["sel_hn1"], z["sel_hn2"], arg), keep, 1.4)
        assert cnt == int(keep.sum()) and abs(val - float(z["neg"])) <= 1e-6
        g_neg = GO.neg_loss_grad(z["F_out"], z["sel_hn1"], z["sel_hn2"], arg, keep, 1.4, 1.0)
    assert np.allclose(mine + g_neg, z["grad"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("path", FINEST, ids=_name)
def test_neg_mask_on_the_fixtures(path):
    z = np.load(path)
    arg = _fixture_nn(z)
    closest = z["sel_hn2"][arg]
    want = ~np.isin(L.neg_hash(z["sel_hn1"], closest, len(z["F_out"])), z["index_hash"]) & (z["sel_hn1"] != closest)
    got = GO.neg_mask(z["sel_hn1"], z["sel_hn2"], arg, z["index"], _goff(z["group"]), len(z["F_out"]))
    assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), want)
    assert np.array_equal(GO.neg_mask(z["sel_hn1"], z["sel_hn2"], arg, z["index"], _goff(z["group"])), got)   # default seed
    assert (~want).any()                                   # every fixture masks some pair (g16_s2: all, its neg is NaN)


@pytest.mark.parametrize("path", CIRCLE, ids=_name)
def test_circle_terms_on_the_circle_fixtures(path):
    z = np.load(path)
    flags, goff, n_sel = _flags(z), _goff(z["group"]), len(z["pos_sel"])
    pp = z["pair_pos"] if "pair_pos" in z.files else None
    q = GO.circle_terms(z["F_out"], z["index"], goff, z["finest_flag"], z["pos_sel"], 0.1, 0.2, 16, flags, pp)
    assert abs(q.pos.mean() - float(z["pos"])) <= 2e-6 * max(1, abs(float(z["pos"])))
    assert abs(q.fin.mean() - float(z["finest"])) <= 2e-6 * max(1, abs(float(z["finest"])))
    sw = {k: bool(z[k]) for k in ("square_loss", "block_finest_gradient", "use_pair_group_positive_loss")}
    Fo = torch.from_numpy(z["F_out"]).double().requires_grad_(True)
    po, fo, no = L.location_circle_loss(Fo, z["group"], z["index"], z["finest_flag"], z["points"], z["batch_lengths"],
                                        max_pos_cluster=int(z["max_pos_cluster"]), draws=(z["pos_sel"], pp), **sw)
    g_pf, = torch.autograd.grad(po + fo, Fo, retain_graph=True)
    g_neg, = torch.autograd.grad(no, Fo)
    w = np.full(n_sel, 1.0 / n_sel)
    mine = q.grad(w, w)
    assert np.abs(mine - g_pf.numpy()).max() <= 1e-12
    assert np.allclose(mine + g_neg.numpy(), z["grad"], rtol=1e-4, atol=1e-6)
    # a gradient arriving at the means is spread evenly over the members
    gm = np.random.RandomState(0).normal(size=q.mean.shape)
    want = np.zeros(z["F_out"].shape)
    for s, i in enumerate(z["pos_sel"]):
        rows = z["index"][goff[i]:goff[i + 1]]
        np.add.at(want, rows, gm[s] / len(rows))
        assert np.allclose(q.mean[s], z["F_out"][rows].astype(np.float64).mean(0), rtol=0, atol=1e-15)
    assert np.abs(q.grad(w, w, gm) - mine - want).max() <= 1e-12


def test_combine_and_seed():
    rng = np.random.RandomState(1)
    pos, fin = rng.rand(7), rng.rand(7)
    tot, pm, fm, ng = GO.combine(pos, fin, 0.25, (0.7, 1.3, 0.9))
    assert ng == 0.25 and abs(tot - (0.7 * pos.sum() / 7 + 1.3 * fin.sum() / 7 + 0.9 * 0.25)) <= 1e-15
    gp, gf, gn = GO.seed(2.0, (0.7, 1.3, 0.9), 7)
    assert np.allclose(gp, 0.2) and np.allclose(gf, 2.6 / 7) and gn == 1.8 and gp.shape == (7,)


# ---- the conditions on the GPU tests' inputs -------------------------------------------------------------------------
SCENES = sorted({(c, s, bool(f & GS.PAIR), bool(f & GS.BLOCK)) for c, f in GS.GROUP_CASES + GS.CIRCLE_CASES
                 for s in GS.SCALES})


@pytest.mark.parametrize("c,scale,pair,block", SCENES)
def test_scene_conditions(c, scale, pair, block):
    sc = GS.scene(c, scale, pair, block)
    assert GS.margins_hold(sc)
    n_rows, sizes = len(sc.F), sc.sizes[sc.sel]
    assert 250 <= n_rows <= 450 and 25 <= len(sc.sizes) <= 35
    norms = np.linalg.norm(sc.F.astype(np.float64), axis=1)
    assert np.abs(norms - scale).max() <= 1e-6 * scale
    want_sizes = {2, 3, 5, 16, 35, 70} | (set() if pair else {1})
    assert set(sizes.tolist()) == want_sizes and set(sc.sizes.tolist()) == want_sizes
    assert len(sc.sel) < len(sc.sizes) and len(set(sc.sel.tolist())) == len(sc.sel) and (np.diff(sc.sel) < 0).any()
    assert (sc.members >= 2).sum() >= 20, "rows in two selected groups"
    assert (sc.members == 0).sum() * 3 >= n_rows, "rows in no selected group"
    for g in range(len(sc.sizes)):
        assert len(set(sc.index[sc.goff[g]:sc.goff[g + 1]].tolist())) == sc.sizes[g], "a row twice in one group"
    # flags: first flag first / in the middle / last (groups of 3 and more), two flags, all flagged
    where, n_flags, all_flagged = set(), [], []
    for s, g in enumerate(sc.sel):
        fl = sc.flag[sc.goff[g]:sc.goff[g + 1]]
        n_flags.append(int(fl.sum()))
        assert fl.sum() >= 1
        first = int(np.argmax(fl))
        if len(fl) >= 3 and fl.sum() == 1:
            where.add("first" if first == 0 else ("last" if first == len(fl) - 1 else "middle"))
        if fl.all() and (block or len(fl) > 1):
            all_flagged.append(s)
    assert where == {"first", "middle", "last"} and n_flags.count(2) >= 1
    assert all_flagged == ([sc.all_s] if block else [])
    if pair:
        assert (sc.pairpos[:, 0] < sc.pairpos[:, 1]).any() and (sc.pairpos[:, 0] > sc.pairpos[:, 1]).any()
        assert (sc.pairpos[:, 0] != sc.pairpos[:, 1]).all() and (sc.pairpos.max(1) < sizes).all()
    assert (sc.gpos != sc.gfin).all() and len(set(sc.gpos.tolist())) == len(sc.gpos)
    assert (sc.prefill != 0).all()
    # both sides of every hinge occur among the selected groups, for both distance forms
    base = (GS.PAIR if pair else 0) | (GS.BLOCK if block else 0)
    for fl in (base, base | GS.SQRT):
        t = GO.group_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, GS.POS_THRESH, GS.FIN_THRESH, fl, sc.pairpos)
        fin_pre = t.fin_pre[np.isfinite(t.fin_pre)]
        assert len(fin_pre) == len(sc.sel) - (1 if block else 0)
        assert (t.pos_pre > GS.POS_THRESH).any() and (t.pos_pre < GS.POS_THRESH).any(), fl
        assert (fin_pre > GS.FIN_THRESH).any() and (fin_pre < GS.FIN_THRESH).any(), fl
        q = GO.circle_terms(sc.F, sc.index, sc.goff, sc.flag, sc.sel, GS.POS_THRESH, GS.FIN_THRESH, GS.LOG_SCALE, fl,
                            sc.pairpos)
        assert (q.fin_v > 0).any() and (q.fin_v < 0).any(), fl
        args = [q.fin_arg] + ([] if pair else [q.pos_arg])
        if not pair:
            assert (q.pos_v > 0).any() and (q.pos_v < 0).any(), fl
        if scale > 1:                                      # the scaled scenes are there for softplus's x > 20 branch
            for a in args:
                assert (a > 20).any() and (a[np.isfinite(a)] < 20).any(), fl
        if block:
            assert q.fin[sc.all_s] == 0 and q.fin_arg[sc.all_s] == -np.inf


@pytest.mark.parametrize("m", (1, 255, 256, 257, 700))
def test_mask_scene_conditions(m):
    expect = dict(self=0, same_group=0, second_group=0, no_common_group=1, other_groups_only=1)
    scenes = [GS.mask_scene(10 + m, m)] if m > 1 else [GS.mask_scene(10 + i, 1, only=k) for i, k in enumerate(GS.KINDS)]
    for ms in scenes:
        assert len(ms.sel1) == m and len(set(ms.sel1.tolist())) == m and len(set(ms.sel2.tolist())) == len(ms.sel2)
        assert (ms.sel2[ms.arg] == ms.target).all() and ms.arg.dtype == np.int32
        keep = GO.neg_mask(ms.sel1, ms.sel2, ms.arg, ms.index, ms.goff, ms.n_rows)
        assert np.array_equal(keep, np.array([expect[k] for k in ms.kind], dtype=np.uint8))
    kinds = np.concatenate([ms.kind for ms in scenes])
    for k in GS.KINDS:
        assert (kinds == k).sum() >= (1 if m == 1 else 15), k


# ---- the fp32 error of the same oracle: where the GPU tests' tolerances come from -------------------------------------
def _err(store, key, value):
    store[key] = max(store.get(key, 0.0), float(value))


def _accumulated(sc, d32):
    """What an fp32 accumulation of the gradient into the prefilled buffer leaves, minus the prefill."""
    return (sc.prefill + d32.astype(np.float32)).astype(np.float64) - sc.prefill


def fp32_oracle_errors():
    """max over the case set of the fp32 oracle's error against the fp64 one, per quantity:
    (family, 'term' | 'df' | 'row', scale).  term: |e| (unit rows) or |e| / max(1, |want|) (scaled); df: rel-L2;
    row: group_loss_scenes.row_error."""
    E = {}
    for fam, cases in (("group", GS.GROUP_CASES), ("circle", GS.CIRCLE_CASES)):
        for c, flags in cases:
            for scale in GS.SCALES:
                sc = GS.case_scene(c, flags, scale)
                a = (sc.F, sc.index, sc.goff, sc.flag)
                th = (GS.POS_THRESH, GS.FIN_THRESH) + ((GS.LOG_SCALE,) if fam == "circle" else ())
                fn = GO.group_terms if fam == "group" else GO.circle_terms
                t64 = fn(*a, sc.sel, *th, flags, sc.pairpos)
                t32 = fn(*a, sc.sel, *th, flags, sc.pairpos, dtype=torch.float32)
                for k in ("pos", "fin"):
                    w, g = getattr(t64, k), getattr(t32, k)
                    ok = np.isfinite(w)
                    assert np.array_equal(ok, np.isfinite(g))
                    e = np.abs(g - w)[ok] / (np.maximum(1, np.abs(w[ok])) if (scale > 1 or fam == "circle") else 1)
                    _err(E, (fam, "term", scale), e.max())
                drop = sc.all_s if (fam == "group" and flags & GS.BLOCK) else None
                sel, pp, gpos, gfin, gmean = GS.without(sc, drop)
                if drop is not None:
                    t64, t32 = fn(*a, sel, *th, flags, pp), fn(*a, sel, *th, flags, pp, dtype=torch.float32)
                for gm in ((None,) if fam == "group" else (None, gmean)):
                    want = t64.grad(gpos, gfin, gm)
                    got = _accumulated(sc, t32.grad(gpos, gfin, gm))
                    _err(E, (fam, "df", scale), GS.rel_l2(got, want))
                    _err(E, (fam, "row", scale), GS.row_error(got, want))
    for m, c, side in GS.NEG_CASES:
        ns = GS.neg_scene(m, c, side)
        a = (ns.F, ns.sel1, ns.sel2, ns.arg, ns.keep, GS.NEG_THRESH, ns.gneg)
        want = GO.neg_loss_grad(*a)
        if np.linalg.norm(want) > 0:
            got = _accumulated(ns, GO.neg_loss_grad(*a, dtype=torch.float32))
            _err(E, ("neg", "df", 1.0), GS.rel_l2(got, want))
            _err(E, ("neg", "row", 1.0), GS.row_error(got, want))
    return E


def test_fp32_oracle_errors_are_the_recorded_ones():
    """The constants of tests/test_gpu_loss_kernels.py are 8 x these measurements; a fresh measurement must reproduce the
    recorded figures (to within a factor of 2: torch's CPU kernels may sum in another order on another machine)."""
    import test_gpu_loss_kernels as K
    E = fp32_oracle_errors()
    for key in sorted(E):
        print(key, f"{E[key]:.3e}", "recorded", K.MEASURED[key])
    assert set(E) == set(K.MEASURED)
    for key, v in E.items():
        assert K.MEASURED[key] / 2 <= v <= K.MEASURED[key] * 2, (key, v, K.MEASURED[key])
        assert K.TOL[key] == 8 * K.MEASURED[key]
    # the project's own tolerances on unit-norm rows leave room for the fp32 oracle itself
    assert E[("group", "term", 1.0)] < 2e-6 and E[("group", "df", 1.0)] < 1e-5
    assert E[("circle", "term", 1.0)] < 1e-5 and E[("circle", "df", 1.0)] < 1e-4
