"""Batched RANSAC registration on the GPU (gcl_ransac_register_batch) and the mutual filter (gcl_mutual_correspondences):
the batch against tests/ransac_oracle.py directly, against single gcl_ransac_register calls bit for bit (ragged counts read on
the device, NaN beyond every count, too-short pairs, another order, another n_cap), the per-pair confidence stop, the mutual
rule against tests/mutual_ransac_oracle.py, the mutual-filter registration end to end, and ``eval_pairs`` with one estimator
call per chunk.

Data and parameters are those of tests/test_gpu_ransac.py (``ransac_oracle.planted_case``, edge similarity 0.9, both
distances 0.3); the bounds on borderline hypotheses and on the winner are that file's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutual_ransac_oracle as MO                                      # noqa: E402
import ransac_oracle as RO                                             # noqa: E402

DEV = "cuda:0"
SIM, DIST = 0.9, 0.3
_cache = {}


def _batch_run(rows, counts, n_cap, seeds, ransac_n, iters, confidence, chunk):
    """One gcl_ransac_register_batch call.  ``rows``: per pair (src, tgt) numpy arrays with at least counts[b] rows; the
    device buffers hold NaN from a pair's count on, the counts are a device tensor.  Returns one dict per pair."""
    from gcl_amd.lib.ransac import ransac_correspondences_batch
    B = len(rows)
    S = np.full((B, n_cap, 3), np.nan, dtype=np.float32)
    G = np.full((B, n_cap, 3), np.nan, dtype=np.float32)
    for b, ((s, g), c) in enumerate(zip(rows, counts)):
        k = max(0, min(c, n_cap))
        S[b, :k], G[b, :k] = s[:k], g[:k]
    with torch.cuda.device(DEV):
        r = ransac_correspondences_batch(torch.from_numpy(S).to(DEV), torch.from_numpy(G).to(DEV), DIST, ransac_n, SIM, DIST,
                                         iters, confidence, torch.tensor(counts, dtype=torch.int32, device=DEV), seeds,
                                         chunk=chunk, want_status=True)
        T, info, fit = r.transformation.cpu().numpy(), r.info.cpu().numpy(), r.fit.cpu().numpy()
        labels, status = r.labels.cpu().numpy(), r.hyp_status.cpu().numpy()
    return [dict(T=T[b].copy(), info=info[b].copy(), fit=fit[b].copy(), labels=labels[b].copy(), status=status[b].copy())
            for b in range(B)]


def _single_run(src, tgt, seed, ransac_n, iters, confidence, chunk):
    from gcl_amd.lib.ransac import ransac_correspondences
    with torch.cuda.device(DEV):
        r = ransac_correspondences(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), DIST, ransac_n, SIM, DIST,
                                   iters, confidence, seed, chunk=chunk, want_status=True)
        return dict(T=r.transformation.cpu().numpy().copy(), info=r.info.cpu().numpy().copy(), fit=r.fit.cpu().numpy().copy(),
                    labels=r.labels.cpu().numpy().copy(), status=r.hyp_status.cpu().numpy().copy())


# ---- the batch against the oracle ------------------------------------------------------------------------------------------
# 257 crosses a 256-thread workgroup and does not divide by the 8 score ranges, 64 is one wave, 4096 + 37 leaves a ragged
# last chunk
PAIRS = [(11, 300, 0.4), (12, 257, 0.3), (13, 64, 0.5)]
SEEDS = [21, 22, 23]
ITERS, CHUNK, N_CAP = 4096 + 37, 1024, 300


def _oracle_batch(ransac_n):
    """(per-pair (src, tgt), per-pair oracle result, per-pair device result of ONE batched call), once per module."""
    if ransac_n not in _cache:
        rows = [RO.planted_case(ds, n, share)[:2] for ds, n, share in PAIRS]
        ora = [RO.ransac(s, g, ransac_n, SIM, DIST, DIST, ITERS, 0.0, seed, CHUNK) for (s, g), seed in zip(rows, SEEDS)]
        dev = _batch_run(rows, [n for _, n, _ in PAIRS], N_CAP, SEEDS, ransac_n, ITERS, 0.0, CHUNK)
        _cache[ransac_n] = (rows, ora, dev)
    return _cache[ransac_n]


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_batch_status_tables_match_the_oracle(ransac_n):
    rows, oras, devs = _oracle_batch(ransac_n)
    for (ds, n, share), ora, dev in zip(PAIRS, oras, devs):
        border = ora["borderline"]
        print(f"  pair {(ds, n, share)} ransac_n {ransac_n}: scored = {(ora['status'] >= 0).sum()}, borderline = "
              f"{100 * border.mean():.3f} %, device != oracle on {(dev['status'] != ora['status']).sum()} ids")
        assert border.mean() <= 0.005
        assert dev["status"].shape == ora["status"].shape
        bad = np.nonzero((dev["status"] != ora["status"]) & ~border)[0]
        assert len(bad) == 0, (bad[:10], dev["status"][bad[:10]], ora["status"][bad[:10]])
        assert dev["info"][2] == ITERS and dev["info"][3] == (dev["status"] >= 0).sum()


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_batch_winners_match_the_oracle(ransac_n):
    rows, oras, devs = _oracle_batch(ransac_n)
    for (ds, n, share), (src, tgt), ora, dev in zip(PAIRS, rows, oras, devs):
        st, border = ora["status"], ora["borderline"]
        best = st[~border].max()
        w = int(dev["info"][0])
        assert dev["info"][1] == best and 0 <= w < ITERS
        assert ora["count"][w] == best
        sse_min = np.nanmin(ora["sse"][st == best])
        assert ora["sse"][w] <= (1 + 1e-4) * sse_min
        S, T = src[ora["samples"][w]].astype(np.float64), tgt[ora["samples"][w]].astype(np.float64)
        R, t, _ = RO.kabsch(S[None], T[None])
        err_R, err_t = np.abs(dev["T"][:3, :3] - R[0]).max(), np.abs(dev["T"][:3, 3] - t[0]).max()
        bound_t = 1e-5 * max(1.0, float(np.linalg.norm(S.mean(0))))
        print(f"  pair {(ds, n, share)} ransac_n {ransac_n}: winner {w} (oracle {ora['winner']}), count {best}, "
              f"|R - oracle| = {err_R:.2e}, |t - oracle| = {err_t:.2e} (bound {bound_t:.2e})")
        assert err_R <= 1e-5 and err_t <= bound_t
        assert (dev["T"][3] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
        d = np.linalg.norm(src.astype(np.float64) @ ora["R"][w].T + ora["t"][w] - tgt, axis=1)
        keep = ~ora["inl_border"][w]
        assert dev["labels"].shape == (N_CAP,)
        assert (dev["labels"][:n][keep] == (d < DIST)[keep].astype(np.float32)).all()
        assert (dev["labels"][n:] == 0).all()                                # rows beyond the pair's count
        fit = np.array([best / n, np.sqrt(ora["sse"][w] / best)])          # fitness over the pair's OWN count
        assert (np.abs(dev["fit"] - fit) <= 1e-5 * fit).all()


# ---- the batch against single calls, bit for bit ----------------------------------------------------------------------------
def _prefix_counts(ransac_n):
    return [300, 257, 64, ransac_n, ransac_n - 1, 0]


PREFIX_SEEDS = [31, 32, 33, 34, 35, 36]
PREFIX_ITERS = 2048


def _assert_short_pair(r, n_cap):
    assert (r["T"] == np.eye(4, dtype=np.float32)).all()
    assert (r["info"] == np.array([-1, 0, 0, 0])).all() and (r["fit"] == 0).all()
    assert r["labels"].shape == (n_cap,) and (r["labels"] == 0).all() and (r["status"] == -4).all()


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_batch_is_bitwise_the_single_calls(ransac_n):
    src, tgt = RO.planted_case(11, 300, 0.4)[:2]
    counts = _prefix_counts(ransac_n)
    B = len(counts)
    batch = _batch_run([(src, tgt)] * B, counts, 300, PREFIX_SEEDS, ransac_n, PREFIX_ITERS, 0.0, CHUNK)
    singles = {}
    for b, n_b in enumerate(counts):
        if n_b < ransac_n:
            _assert_short_pair(batch[b], 300)
            continue
        one = singles[b] = _single_run(src[:n_b], tgt[:n_b], PREFIX_SEEDS[b], ransac_n, PREFIX_ITERS, 0.0, CHUNK)
        ora = RO.ransac(src[:n_b], tgt[:n_b], ransac_n, SIM, DIST, DIST, PREFIX_ITERS, 0.0, PREFIX_SEEDS[b], CHUNK)
        print(f"  n_b {n_b} ransac_n {ransac_n}: info {batch[b]['info']}, oracle borderline {100 * ora['borderline'].mean():.3f} %")
        # the oracle's own borderline share: at most 0.0034 for ransac_n 3; for 4 the 64-row prefix has 12 borderline ids
        # of 2048 (0.0059, whatever the seed: few rows, many near the inlier distance), so the cap is asserted for 3 only
        # and the comparison below excludes exactly the borderline ids either way
        assert ransac_n == 4 or ora["borderline"].mean() <= 0.005
        ok = ~ora["borderline"]
        assert (batch[b]["status"][ok] == ora["status"][ok]).all()           # the prefix runs are the oracle's too
        for k in ("T", "info", "fit", "status"):
            assert batch[b][k].tobytes() == one[k].tobytes(), (n_b, k)
        assert batch[b]["labels"][:n_b].tobytes() == one["labels"].tobytes() and (batch[b]["labels"][n_b:] == 0).all()
    assert batch[0]["info"][0] >= 0 and batch[0]["info"][2] == PREFIX_ITERS
    # the same pairs in another order and under another n_cap: every pair keeps its bits
    order = [4, 2, 0, 5, 3, 1]
    again = _batch_run([(src, tgt)] * B, [counts[b] for b in order], 512, [PREFIX_SEEDS[b] for b in order], ransac_n,
                       PREFIX_ITERS, 0.0, CHUNK)
    for pos, b in enumerate(order):
        n_b = counts[b]
        if n_b < ransac_n:
            _assert_short_pair(again[pos], 512)
            continue
        for k in ("T", "info", "fit", "status"):
            assert again[pos][k].tobytes() == batch[b][k].tobytes(), (n_b, k)
        assert again[pos]["labels"][:300].tobytes() == batch[b]["labels"].tobytes() and (again[pos]["labels"][300:] == 0).all()


def test_counts_outside_the_range_are_clamped():
    """A negative count reads as 0, one above n_cap as n_cap."""
    src, tgt = RO.planted_case(11, 300, 0.4)[:2]
    S, G = torch.from_numpy(src).to(DEV)[None].repeat(2, 1, 1), torch.from_numpy(tgt).to(DEV)[None].repeat(2, 1, 1)
    from gcl_amd.lib.ransac import ransac_correspondences_batch
    with torch.cuda.device(DEV):
        r = ransac_correspondences_batch(S, G, DIST, 3, SIM, DIST, 1024, 0.0, torch.tensor([-5, 100000], dtype=torch.int32, device=DEV),
                                         [31, 31], chunk=CHUNK, want_status=True)
        T, info, status = r.transformation.cpu().numpy(), r.info.cpu().numpy(), r.hyp_status.cpu().numpy()
        labels = r.labels.cpu().numpy()
    one = _single_run(src, tgt, 31, 3, 1024, 0.0, CHUNK)
    assert (T[0] == np.eye(4)).all() and (info[0] == np.array([-1, 0, 0, 0])).all() and (status[0] == -4).all()
    assert (labels[0] == 0).all()
    assert T[1].tobytes() == one["T"].tobytes() and info[1].tobytes() == one["info"].tobytes()
    assert status[1].tobytes() == one["status"].tobytes() and labels[1].tobytes() == one["labels"].tobytes()


# ---- the confidence stop is per pair ----------------------------------------------------------------------------------------
def test_confidence_stop_is_per_pair():
    chunk, iters = 512, 8192
    cases = [((11, 256, 0.4), 1, 512), ((11, 256, 0.15), 3, 2560)]
    rows = [RO.planted_case(ds, n, share)[:2] for (ds, n, share), _, _ in cases]
    oras = [RO.ransac(s, g, 3, SIM, DIST, DIST, iters, 0.999, seed, chunk) for (s, g), (_, seed, _) in zip(rows, cases)]
    # oracle side: every limit in force stays clear of the chunk boundaries (tests/test_gpu_ransac.py's margin rule)
    for ora, (_, _, covered) in zip(oras, cases):
        for lim in ora["limits"]:
            assert lim is not None and min(lim % chunk, chunk - lim % chunk) >= 0.01 * chunk, ora["limits"]
        assert ora["covered"] == covered
    assert [o["limit"] for o in oras] == [106, 2109]
    devs = _batch_run(rows, [256, 256], 256, [seed for _, seed, _ in cases], 3, iters, 0.999, chunk)
    print(f"  limits {[o['limits'] for o in oras]}, device info {[d['info'] for d in devs]}")
    assert [int(d["info"][2]) for d in devs] == [512, 2560]
    for ora, dev in zip(oras, devs):
        assert ((dev["status"] == -4) == (ora["status"] == -4)).all()
        assert (dev["status"][ora["covered"]:] == -4).all() and (dev["status"][:ora["covered"]] != -4).all()
        ok = ~ora["borderline"]
        assert (dev["status"][ok] == ora["status"][ok]).all()
        assert dev["info"][1] == ora["status"][ok].max() and dev["info"][3] == (dev["status"] >= 0).sum()


# ---- gcl_mutual_correspondences ---------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 300)


def _device_mutual(nn01, nn10, xyz0, xyz1, min_count):
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    with torch.cuda.device(DEV):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (nn01, nn10, xyz0, xyz1)]
        m0, m1 = len(nn01), len(nn10)
        src = torch.full((m0, 3), float("nan"), device=DEV)
        tgt = torch.full((m0, 3), float("nan"), device=DEV)
        count = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.gcl_mutual_correspondences(_lib.ptr(t[0], torch.int32), m0, _lib.ptr(t[1], torch.int32), m1,
                                                  _lib.ptr(t[2], torch.float32), _lib.ptr(t[3], torch.float32), min_count,
                                                  _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(count), _lib.stream()),
                   "gcl_mutual_correspondences")
        return src.cpu().numpy(), tgt.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("m0", SIZES)
def test_mutual_correspondences_match_the_oracle(m0):
    rng = np.random.RandomState(m0)
    for m1 in SIZES:
        nn01, nn10 = MO.random_tables(m0 * 1000 + m1, m0, m1)
        xyz0, xyz1 = rng.uniform(-5, 5, (m0, 3)).astype(np.float32), rng.uniform(-5, 5, (m1, 3)).astype(np.float32)
        k = len(MO.loop_list(nn01, nn10))
        for min_count in (k, k + 1):                                         # both sides of |M|
            want = MO.correspondences(nn01, nn10, xyz0, xyz1, min_count)
            got = _device_mutual(nn01, nn10, xyz0, xyz1, min_count)
            assert tuple(got[2]) == tuple(want[2]) == ((k, k) if min_count <= k else (m0, k)), (m0, m1, min_count)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (m0, m1, min_count)


# ---- the mutual filter end to end -------------------------------------------------------------------------------------------
def test_mutual_filter_registration_on_a_planted_motion():
    from gcl_amd.lib.ransac import (FeatureRansac, ransac_correspondences,
                                    registration_ransac_based_on_mutual_feature_matching)
    F0, F1, perm = MO.planted_features(2)
    src, tgt, R, t, _ = RO.planted_case(11, 300, 0.4)
    xyz1 = np.empty_like(tgt)
    xyz1[perm] = tgt
    nn01, nn10, gap = MO.tables(F0, F1)
    assert gap >= 1e-3
    s, g, count = MO.correspondences(nn01, nn10, src, xyz1, 3)
    assert count[0] == 300
    with torch.cuda.device(DEV):
        d = [torch.from_numpy(a).to(DEV) for a in (src, xyz1, F0, F1)]
        res = registration_ransac_based_on_mutual_feature_matching(*d, DIST, 3, SIM, DIST, 4096, 0.0, seed=7)
        assert int(res.count) == 300 and int(res.n_mutual) == 300
        one = ransac_correspondences(torch.from_numpy(s).to(DEV), torch.from_numpy(g).to(DEV), DIST, 3, SIM, DIST, 4096, 0.0, 7)
        for a, b in ((res.transformation[0], one.transformation), (res.fit[0], one.fit), (res.info[0], one.info),
                     (res.labels[0], one.labels)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert res.src_corr[0].cpu().numpy().tobytes() == s.tobytes() and res.tgt_corr[0].cpu().numpy().tobytes() == g.tobytes()
        T = res.transformation[0].cpu().numpy()
        # the same through the Matcher interface, two pairs in one call
        m = FeatureRansac(DIST, 3, SIM, DIST, 4096, 0.0, seed=7, mutual_filter=True)
        Tb, labels, sc, tc = m.estimator(*(x[None].repeat(2, 1, 1) for x in d))
        assert Tb.shape == (2, 4, 4) and labels.shape == (2, 300) and sc.shape == tc.shape == (2, 300, 3)
        assert Tb[0].cpu().numpy().tobytes() == T.tobytes() and Tb[1].cpu().numpy().tobytes() == T.tobytes()
        assert m.last.count.tolist() == [300, 300]
    err_R, err_t = np.abs(T[:3, :3] - R).max(), np.abs(T[:3, 3] - t).max()
    print(f"  |R - planted| = {err_R:.2e}, |t - planted| = {err_t:.2e}")
    assert err_R < 2e-2 and err_t < 0.2


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_mutual_filter_falls_back_below_ransac_n(ransac_n):
    """The funnel: 1 + e mutual pairs.  e = ransac_n - 2: open3d's fall-back, bitwise the registration without the filter;
    e = ransac_n - 1: exactly ransac_n mutual pairs, the list is used (the >= boundary)."""
    from gcl_amd.lib.ransac import (registration_ransac_based_on_feature_matching,
                                    registration_ransac_based_on_mutual_feature_matching)
    rng = np.random.RandomState(4)
    xyz0 = rng.uniform(-5, 5, (MO.FUNNEL_M0, 3)).astype(np.float32)
    xyz1 = rng.uniform(-5, 5, (MO.FUNNEL_M1, 3)).astype(np.float32)
    with torch.cuda.device(DEV):
        for e, want in ((ransac_n - 2, (MO.FUNNEL_M0, ransac_n - 1)), (ransac_n - 1, (ransac_n, ransac_n))):
            F0, F1 = MO.funnel_features(5, e)
            nn01, nn10, gap = MO.tables(F0, F1)
            assert gap >= 1e-3
            s, g, count = MO.correspondences(nn01, nn10, xyz0, xyz1, ransac_n)
            assert tuple(count) == want
            d = [torch.from_numpy(a).to(DEV) for a in (xyz0, xyz1, F0, F1)]
            res = registration_ransac_based_on_mutual_feature_matching(*d, 4.0, ransac_n, 0.0, 4.0, 1024, 0.0, seed=9)
            assert (int(res.count), int(res.n_mutual)) == want
            assert res.src_corr[0].cpu().numpy().tobytes() == s.tobytes() and res.tgt_corr[0].cpu().numpy().tobytes() == g.tobytes()
            if want[0] == MO.FUNNEL_M0:
                ref = registration_ransac_based_on_feature_matching(*d, False, 4.0, ransac_n, 0.0, 4.0, 1024, 0.0, seed=9)
                assert int(ref.info[3]) > 0                                   # something was scored: the comparison says something
                for a, b in ((res.transformation[0], ref.transformation), (res.fit[0], ref.fit), (res.info[0], ref.info),
                             (res.labels[0], ref.labels)):
                    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- eval_pairs -------------------------------------------------------------------------------------------------------------
def _twin_pair(seed, shift_voxels=(8, 0, 0), voxel=0.3):
    """tests/test_gpu_ransac.py's helper, restated: an eval pair whose second cloud is the first one moved by a multiple of 8
    voxels -- twin voxels get equal features from an untrained network, everything else is an outlier."""
    from gcl_amd import synthetic
    p = synthetic.make_eval_pair(seed, voxel_size=voxel, baseline=6.0, n_boxes=25)
    keep = torch.arange(0, len(p["sinput0_C"]), 3)
    C0 = p["sinput0_C"][keep].clone()
    xyz0 = p["pcd0"][0][keep].clone()
    sh = torch.tensor(shift_voxels, dtype=torch.int32)
    C1 = C0.clone()
    C1[:, 1:] += sh
    xyz1 = xyz0 + sh.float() * voxel
    F = 1.0 + 0.05 * torch.randn(len(C0), 1, generator=torch.Generator().manual_seed(seed))
    T = torch.eye(4)
    T[:3, 3] = sh.float() * voxel
    return {"pcd0": (xyz0,), "pcd1": (xyz1,), "sinput0_C": C0, "sinput1_C": C1, "sinput0_F": F, "sinput1_F": F.clone(),
            "T_gt": T}


def test_eval_pairs_with_one_registration_call_per_chunk():
    from gcl_amd.lib.ransac import FeatureRansac
    from gcl_amd.model import load_model
    from gcl_amd.scripts.SC2_PCR import Matcher
    from gcl_amd.scripts.eval_batch import eval_pairs
    torch.manual_seed(5)
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            elif name.endswith("bn.bias"):
                p.uniform_(-0.1, 0.1)
    m.eval()
    pairs = [_twin_pair(60, (8, 0, 0)), _twin_pair(61, (-8, 16, 0)), _twin_pair(62, (16, 8, 8)), _twin_pair(63, (0, -8, 8))]
    NPTS = 1500
    assert all(len(p["sinput0_C"]) > NPTS for p in pairs)
    with pytest.raises(ValueError, match="batch_registration"):
        eval_pairs(m, pairs, Matcher(), device=DEV, batch_pairs=4, batch_registration=True)
    results = []
    for batched in (False, True):
        np.random.seed(9)
        results.append(eval_pairs(m, pairs, FeatureRansac.kitti(0.3, seed=5), device=DEV, batch_pairs=4, subsample_size=NPTS,
                                  n_points=NPTS, batch_registration=batched))
    one, bat = results
    assert len(bat["T_est"]) == 4 and bat["n_pairs"] == 4
    for a, b in zip(one["T_est"], bat["T_est"]):
        assert torch.equal(a, b), "one registration call per chunk must not change a single bit"
    assert one["rte"] == bat["rte"] and one["success"] == bat["success"]
    assert all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(one["rre"], bat["rre"]))
    assert bat["success_rate"] == 1.0
