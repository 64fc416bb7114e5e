"""A batch of feature 1-NN searches in the launches of one (gcl_nn_rowmin_batch) and the mutual filters with one workgroup
per pair (gcl_mutual_match_batch, gcl_mutual_correspondences_batch): bit for bit the single entries, against the fp64
oracle, ties, independence of a search from its neighbours, the fused gather of point rows.

Shapes are the edges of the kernel (those of tests/test_gpu_sc2_bench.py): the 64-row A tile (1, 63, 64, 65, 130 rows), an
odd B count, mb = 1, several chunks with a merge (203 columns beside 2 rows of A tiles: the batch's chunk is 8 rows) next to
searches that fit one chunk (written by the search kernel itself) in the same call."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
SIZES = ((1, 1), (65, 2), (130, 9), (67, 203), (64, 8), (3, 1))
ROWS = (False, True, False, True, True, False)      # which searches go through row lists into larger shuffled matrices
FIXED = (16, 32, 64)                                 # -> the chain of gcl_nn_rowmin; every other width: gcl_nn_rowmin_any
WIDTHS = FIXED + (1, 33, 40, 65, 128)
GUARD, SENT = 4, 0x5A5A5A5A


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _single(A, B, rows_a=None, rows_b=None, l2=0):
    """A direct call of the single entry for the width -> (dmin, argmin) on the host."""
    from gcl_amd import _lib
    lib = _lib.load()
    ma = len(A) if rows_a is None else len(rows_a)
    mb = len(B) if rows_b is None else len(rows_b)
    c = A.shape[1]
    entry = "gcl_nn_rowmin" if c in FIXED else "gcl_nn_rowmin_any"
    ns = lib.gcl_nn_rowmin_scratch_len(ma, mb) if c in FIXED else lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c)
    scratch = torch.full((ns,), -1, dtype=torch.int32, device=DEV)
    dmin = torch.empty(ma, dtype=torch.float32, device=DEV)
    arg = torch.empty(ma, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(getattr(lib, entry)(_lib.ptr(A), _lib.ptr(rows_a), ma, _lib.ptr(B), _lib.ptr(rows_b), mb, c, l2,
                                       _lib.ptr(scratch), _lib.ptr(dmin), _lib.ptr(arg), _lib.stream()), entry)
    return dmin.cpu().numpy(), arg.cpu().numpy()


def _batch(searches, l2=0):
    """A direct call of gcl_nn_rowmin_batch.  ``searches``: dicts of device tensors (A, B and optionally rows_a, rows_b, pts_a,
    pts_b).  Scratch is pre-filled with -1; every output is carved from ONE buffer with guard words around it, and the
    guards are checked.  -> per search (dmin, argmin[, src, tgt]) on the host."""
    from gcl_amd import _lib
    lib = _lib.load()
    P, c = len(searches), searches[0]["A"].shape[1]
    recs = (_lib.NnSearch * P)()
    plan, off = [], GUARD
    for s in searches:
        ma = len(s["A"]) if s.get("rows_a") is None else len(s["rows_a"])
        mb = len(s["B"]) if s.get("rows_b") is None else len(s["rows_b"])
        fields = [("dmin", ma), ("argmin", ma)] + ([("src", 3 * ma), ("tgt", 3 * ma)] if "pts_a" in s else [])
        at = {}
        for name, n in fields:
            at[name] = (off, n)
            off += n + GUARD
        plan.append((ma, mb, at))
    buf = torch.full((off,), SENT, dtype=torch.int32, device=DEV)
    for r, s, (ma, mb, at) in zip(recs, searches, plan):
        r.a, r.rows_a, r.ma = _lib.ptr(s["A"]), _lib.ptr(s.get("rows_a")), ma
        r.b, r.rows_b, r.mb = _lib.ptr(s["B"]), _lib.ptr(s.get("rows_b")), mb
        r.pts_a, r.pts_b = _lib.ptr(s.get("pts_a")), _lib.ptr(s.get("pts_b"))
        for name, (o, n) in at.items():
            setattr(r, name, buf.data_ptr() + 4 * o)
    ns = lib.gcl_nn_rowmin_batch_scratch_len(ctypes.addressof(recs), P, c)
    assert ns > 0
    scratch = torch.full((ns,), -1, dtype=torch.int32, device=DEV)
    table = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to(DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.gcl_nn_rowmin_batch(ctypes.addressof(recs), _lib.ptr(table), P, c, l2, _lib.ptr(scratch),
                                           _lib.stream()), "gcl_nn_rowmin_batch")
    host = buf.cpu().numpy()
    written = np.zeros(off, dtype=bool)
    out = []
    for ma, mb, at in plan:
        got = []
        for name, (o, n) in at.items():
            written[o:o + n] = True
            v = host[o:o + n]
            got.append(v.copy() if name == "argmin" else v.view(np.float32).copy())
        out.append(tuple(got))
    assert (host[~written] == SENT).all(), "a guard word between the outputs was overwritten"
    return out


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """The six searches at width c, drawn once: separated inputs (the fp64 oracle alone decides every arg-minimum), the
    searches marked in ROWS reading them through row lists into larger shuffled matrices."""
    rng = np.random.RandomState(500 + c)
    out = []
    for (ma, mb), rows in zip(SIZES, ROWS):
        while True:
            A, B = rng.normal(size=(ma, c)).astype(np.float32), rng.normal(size=(mb, c)).astype(np.float32)
            d2, arg, gap = EO.nn(A, B, with_gap=True)
            if (np.isinf(gap) | (gap > 4 * (c + 2) * EPS * (d2 + gap))).all():
                break
        s = dict(d2=d2, arg=arg)
        if rows:
            pa, pb = rng.permutation(ma + 7)[:ma], rng.permutation(mb + 5)[:mb]
            A_big, B_big = rng.normal(size=(ma + 7, c)).astype(np.float32), rng.normal(size=(mb + 5, c)).astype(np.float32)
            A_big[pa], B_big[pb] = A, B
            s.update(A=_dev(A_big), B=_dev(B_big), rows_a=_dev(pa.astype(np.int64)), rows_b=_dev(pb.astype(np.int64)))
        else:
            s.update(A=_dev(A), B=_dev(B))
        out.append(s)
    return out


def _tensors(s):
    return {k: v for k, v in s.items() if k not in ("d2", "arg")}


@functools.lru_cache(maxsize=None)
def _batch_result(c, l2):
    return _batch([_tensors(s) for s in _inputs(c)], l2)


@pytest.mark.parametrize("c", WIDTHS)
def test_batch_is_bitwise_the_single_entries(c):
    for l2 in (0, 1):
        got = _batch_result(c, l2)
        for i, s in enumerate(_inputs(c)):
            dmin, arg = _single(s["A"], s["B"], s.get("rows_a"), s.get("rows_b"), l2)
            assert got[i][0].tobytes() == dmin.tobytes(), (c, l2, i)
            assert got[i][1].tobytes() == arg.tobytes(), (c, l2, i)


@pytest.mark.parametrize("c", WIDTHS)
def test_batch_matches_the_fp64_oracle(c):
    """Bounds of tests/test_gpu_sc2_bench.py: one rounding per subtraction, product and sum of a channel, c channels; with l2
    half of that for the root's argument, 1/2 for the rounded sum with 1e-7 and 1 for the root itself."""
    sq, l2 = _batch_result(c, 0), _batch_result(c, 1)
    for i, s in enumerate(_inputs(c)):
        d2 = s["d2"]
        assert (sq[i][1] == s["arg"]).all() and (l2[i][1] == s["arg"]).all(), (c, i)
        err = np.abs(sq[i][0].astype(np.float64) - d2) / np.maximum(d2, 1e-300)
        print(f"c={c} search {i} {SIZES[i]}: max rel err {err.max() / EPS:.2f} ulp (bound {c + 2})")
        assert err.max() <= (c + 2) * EPS, (c, i, err.max())
        want = np.sqrt(d2 + 1e-7)
        err = np.abs(l2[i][0] - want) / want
        assert err.max() <= ((c + 2) / 2 + 1.5) * EPS, (c, i, err.max())


@pytest.mark.parametrize("c", (3, 32, 33, 96))
def test_batch_exact_ties_go_to_the_lowest_index(c):
    """B holds five distinct rows, each many times, spread over every chunk and wave; A holds copies of them and random rows.
    Two such searches (one chunk; 26 chunks and a merge) share a batch with a search without ties."""
    rng = np.random.RandomState(7 + c)
    while True:
        U = rng.normal(size=(5, c)).astype(np.float32)
        A = np.concatenate([U[rng.randint(0, 5, 30)], rng.normal(size=(37, c)).astype(np.float32)])
        d2, _, gap = EO.nn(A, U, with_gap=True)
        if (gap > 4 * (c + 2) * EPS * (d2 + gap)).all():
            break
    plain = _inputs(c)[3] if c in (32, 33) else None                     # 67 x 203 through row lists, or drawn below
    searches, want = [], []
    for mb in (9, 203):
        pick = rng.permutation(np.concatenate([np.arange(5), rng.randint(0, 5, mb - 5)]))
        B = U[pick]
        d2, arg = EO.nn(A, B)                                            # np.argmin: the first of equal minima
        assert (d2[:30] == 0).all()
        searches.append(dict(A=_dev(A), B=_dev(B)))
        want.append(arg)
    if plain is None:
        X, Y = rng.normal(size=(67, c)).astype(np.float32), rng.normal(size=(203, c)).astype(np.float32)
        plain = dict(A=_dev(X), B=_dev(Y))
    searches.insert(1, _tensors(plain))
    got = _batch(searches)
    for (dmin, arg), w in zip((got[0], got[2]), want):
        assert (arg == w).all() and (dmin[:30] == 0).all()
    alone = _single(plain["A"], plain["B"], plain.get("rows_a"), plain.get("rows_b"))
    assert got[1][0].tobytes() == alone[0].tobytes() and got[1][1].tobytes() == alone[1].tobytes()


@pytest.mark.parametrize("c", (32, 33))
def test_a_search_does_not_depend_on_its_neighbours(c):
    rng = np.random.RandomState(40 + c)
    x = _tensors(_inputs(c)[3])                                          # 67 x 203 through row lists: 26 chunks alone
    ref = _batch([x])[0]
    same = lambda got: got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    assert same(_batch([x])[0]), "two runs differ"
    single = _single(x["A"], x["B"], x.get("rows_a"), x.get("rows_b"))
    assert same(single)
    small = [dict(A=_dev(rng.normal(size=(ma, c)).astype(np.float32)), B=_dev(rng.normal(size=(mb, c)).astype(np.float32)))
             for ma, mb in ((1, 1), (65, 2), (130, 9), (64, 8), (3, 1), (63, 17), (5, 40), (129, 64))]
    for pos in (0, 4, 8):                                                # first, in the middle and last of a batch of 9
        got = _batch(small[:pos] + [x] + small[pos:])
        assert same(got[pos]), pos
    # next to a search 30 times its size (6 x the rows, 5 x the columns): the batch's chunk is no longer the search's own
    big = dict(A=_dev(rng.normal(size=(402, c)).astype(np.float32)), B=_dev(rng.normal(size=(1015, c)).astype(np.float32)))
    got = _batch([big, x])
    assert same(got[1])
    big_alone = _single(big["A"], big["B"])
    assert got[0][0].tobytes() == big_alone[0].tobytes() and got[0][1].tobytes() == big_alone[1].tobytes()
    # shared inputs: two searches on one b, and the two directions of a pair (a of one is b of the other)
    F0, F1 = _dev(rng.normal(size=(67, c)).astype(np.float32)), _dev(rng.normal(size=(203, c)).astype(np.float32))
    F2 = _dev(rng.normal(size=(130, c)).astype(np.float32))
    got = _batch([dict(A=F0, B=F1), dict(A=F2, B=F1), dict(A=F1, B=F0), x])
    assert same(got[3])
    for g, (a, b) in zip(got, ((F0, F1), (F2, F1), (F1, F0))):
        alone = _single(a, b)
        assert g[0].tobytes() == alone[0].tobytes() and g[1].tobytes() == alone[1].tobytes()


@pytest.mark.parametrize("c", (32, 33))
def test_gather_writes_the_point_rows_into_slices_of_a_padded_buffer(c):
    """src / tgt equal torch indexing with the returned argmin, with and without row lists, written into the rows of a
    [B, n_cap, 3] buffer below each pair's count; the rows beyond keep the sentinel."""
    from gcl_amd.lib.metrics import pdist_min_batch
    rng = np.random.RandomState(60 + c)
    n_cap, sentinel = 140, -77.0
    inputs = _inputs(c)
    src = torch.full((len(inputs), n_cap, 3), sentinel, dtype=torch.float32, device=DEV)
    tgt = torch.full_like(src, sentinel)
    problems, pts = [], []
    for b, s in enumerate(inputs):
        ma = len(s["arg"])
        pa = _dev(rng.normal(size=(len(s["A"]), 3)).astype(np.float32))
        pb = _dev(rng.normal(size=(len(s["B"]), 3)).astype(np.float32))
        pts.append((pa, pb))
        problems.append((s["A"], s["B"], s.get("rows_a"), s.get("rows_b"), pa, pb, src[b, :ma], tgt[b, :ma]))
    with torch.cuda.device(DEV):
        out = pdist_min_batch(problems, "SquareL2")
    plain = _batch_result(c, 0)
    for b, (s, (pa, pb)) in enumerate(zip(inputs, pts)):
        ma = len(s["arg"])
        dmin, arg = out[b][0], out[b][1]
        assert dmin.cpu().numpy().tobytes() == plain[b][0].tobytes() and arg.cpu().numpy().tobytes() == plain[b][1].tobytes()
        ia = s["rows_a"] if "rows_a" in s else torch.arange(ma, device=DEV)
        ib = s["rows_b"][arg.long()] if "rows_b" in s else arg.long()
        assert torch.equal(src[b, :ma], pa[ia]) and torch.equal(tgt[b, :ma], pb[ib]), b
        assert out[b][2].data_ptr() == src[b].data_ptr() and out[b][3].data_ptr() == tgt[b].data_ptr()
        assert (src[b, ma:] == sentinel).all() and (tgt[b, ma:] == sentinel).all(), b
    # mixed widths are refused before any launch
    with pytest.raises(ValueError, match="share the width"):
        pdist_min_batch([(inputs[0]["A"], inputs[0]["B"]), (_inputs(16)[0]["A"], _inputs(16)[0]["B"])])


# ---- the mutual filters ------------------------------------------------------------------------------------------------
MIN_COUNT, TAU = 3, 0.25


def _pair(rng, m0, m1, n_mutual, transform, out_of_range=False):
    """nn01 / nn10 with exactly ``n_mutual`` mutual pairs: random maps, then every accidental mutual pair is broken and
    ``n_mutual`` distinct (i, j) are tied to each other."""
    nn01, nn10 = rng.randint(0, m1, m0).astype(np.int32), rng.randint(0, m0, m1).astype(np.int32)
    ii, jj = rng.permutation(m0)[:n_mutual], rng.permutation(m1)[:n_mutual]
    nn10[:] = -1                                                         # no target names a source ...
    nn10[jj] = ii                                                        # ... but the chosen ones
    nn01[ii] = jj
    others = np.setdiff1d(np.arange(m0), ii)
    clash = others[np.isin(nn01[others], jj)]                            # a source pointing at a tied target is not mutual
    assert (nn10[nn01[clash]] != clash).all()
    if out_of_range:
        free = others[:4]
        nn01[free] = [-1, m1, m1 + 5, -(2 ** 31)][:len(free)]
    # the two clouds lie ~17 apart: no pair is an inlier by accident
    xyz0, xyz1 = rng.normal(size=(m0, 3)).astype(np.float32) + 10, rng.normal(size=(m1, 3)).astype(np.float32)
    T = None
    if transform:
        T = np.concatenate([np.eye(3), rng.normal(size=(3, 1)) * 0.01], axis=1).astype(np.float32).reshape(12)
        xyz0[ii[::2]] = xyz1[jj[::2]] + T[3::4]                         # every other mutual pair is an inlier
    return dict(nn01=_dev(nn01), nn10=_dev(nn10), xyz0=_dev(xyz0), xyz1=_dev(xyz1), T=_dev(T), m0=m0, m1=m1)


def _mutual_pairs():
    rng = np.random.RandomState(11)
    return [_pair(rng, 1, 1, 1, False),                                  # below min_count: the fall-back branch
            _pair(rng, 63, 1025, 0, True),                               # no mutual pair at all
            _pair(rng, 1024, 63, 40, True),
            _pair(rng, 1025, 2100, 700, True, out_of_range=True),
            _pair(rng, 2100, 1024, 900, False, out_of_range=True),
            _pair(rng, 63, 1, 1, True),                                  # fall-back, most targets repeated
            _pair(rng, 2100, 2100, 2, False, out_of_range=True)]         # fall-back with out-of-range entries: zero target rows


def _jobs(pairs, outs):
    from gcl_amd import _lib
    recs = (_lib.MutualJob * len(pairs))()
    for r, p, o in zip(recs, pairs, outs):
        for name in ("nn01", "nn10", "xyz0", "xyz1", "T"):
            setattr(r, name, _lib.ptr(p[name]))
        r.m0, r.m1 = p["m0"], p["m1"]
        for name, t in o.items():
            setattr(r, name, _lib.ptr(t))
    return recs, torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to(DEV)


def test_mutual_match_batch_is_bitwise_the_single_entry():
    from gcl_amd import _lib
    lib = _lib.load()
    pairs = _mutual_pairs()
    new = lambda p: dict(pairs=torch.full((p["m0"], 2), -9, dtype=torch.int32, device=DEV),
                         count=torch.full((2,), -9, dtype=torch.int32, device=DEV))
    one, many = [new(p) for p in pairs], [new(p) for p in pairs]
    with torch.cuda.device(DEV):
        for p, o in zip(pairs, one):
            _lib.check(lib.gcl_mutual_match(_lib.ptr(p["nn01"]), p["m0"], _lib.ptr(p["nn10"]), p["m1"], _lib.ptr(p["xyz0"]),
                                            _lib.ptr(p["xyz1"]), _lib.ptr(p["T"]), TAU, _lib.ptr(o["pairs"]),
                                            _lib.ptr(o["count"]), _lib.stream()), "gcl_mutual_match")
        recs, table = _jobs(pairs, many)
        _lib.check(lib.gcl_mutual_match_batch(ctypes.addressof(recs), _lib.ptr(table), len(pairs), TAU, _lib.stream()),
                   "gcl_mutual_match_batch")
    expect = (1, 0, 40, 700, 900, 1, 2)
    for k, (p, a, b) in enumerate(zip(pairs, one, many)):
        assert torch.equal(a["count"], b["count"]) and torch.equal(a["pairs"], b["pairs"]), k
        stats = b["count"].cpu().numpy()
        assert stats[0] == expect[k], (k, stats)
        assert stats[1] == ((expect[k] + 1) // 2 if p["T"] is not None else 0), (k, stats)


def test_mutual_correspondences_batch_is_bitwise_the_single_entry():
    from gcl_amd import _lib
    lib = _lib.load()
    pairs = _mutual_pairs()
    new = lambda p: dict(src=torch.full((p["m0"], 3), -9.0, dtype=torch.float32, device=DEV),
                         tgt=torch.full((p["m0"], 3), -9.0, dtype=torch.float32, device=DEV),
                         count=torch.full((2,), -9, dtype=torch.int32, device=DEV))
    one, many = [new(p) for p in pairs], [new(p) for p in pairs]
    with torch.cuda.device(DEV):
        for p, o in zip(pairs, one):
            _lib.check(lib.gcl_mutual_correspondences(_lib.ptr(p["nn01"]), p["m0"], _lib.ptr(p["nn10"]), p["m1"],
                                                      _lib.ptr(p["xyz0"]), _lib.ptr(p["xyz1"]), MIN_COUNT, _lib.ptr(o["src"]),
                                                      _lib.ptr(o["tgt"]), _lib.ptr(o["count"]), _lib.stream()),
                       "gcl_mutual_correspondences")
        recs, table = _jobs(pairs, many)
        _lib.check(lib.gcl_mutual_correspondences_batch(ctypes.addressof(recs), _lib.ptr(table), len(pairs), MIN_COUNT,
                                                        _lib.stream()), "gcl_mutual_correspondences_batch")
    expect = ((1, 1), (63, 0), (40, 40), (700, 700), (900, 900), (63, 1), (2100, 2))      # (rows, mutual pairs)
    for k, (a, b) in enumerate(zip(one, many)):
        for name in ("src", "tgt", "count"):
            assert a[name].cpu().numpy().tobytes() == b[name].cpu().numpy().tobytes(), (k, name)
        assert tuple(b["count"].cpu().numpy()) == expect[k], k
