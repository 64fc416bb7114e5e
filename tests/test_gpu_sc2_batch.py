"""Batched SC2-PCR registration on the GPU (gcl_sc2_register_batch, ``BatchMatcher``): every pair of a batch against
``Matcher`` run on that pair alone, bit for bit in every stage -- the four goldens in one call and in reversed order, counts
on the word / tile / chunk edges, pairs that leave the power iteration and the refinement at different times, stale
scratch, another stream, sub-batches, ``estimator`` with host draws and the eval loop with one registration call per chunk.

Sizes are the smallest that reach the edges named in each test; the configuration is the goldens' (KITTI's).  Rows beyond a
pair's count are NaN in every batch: nothing may read them."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_oracle as RO                                             # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = dict(inlier_threshold=0.6, d_thre=0.1, num_iterations=20, ratio=0.2, nms_radius=0.6, max_points=8000, k1=30, k2=20)
STAGES = ("conf", "seeds", "knn", "seed_trans", "fitness", "best")
_cache = {}


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _single(key, src, tgt):
    """``Matcher`` on one pair alone: the bytes of the transformation, the labels and every stage.  Computed once per key."""
    if key not in _cache:
        from gcl_amd.scripts.SC2_PCR import Matcher
        with torch.cuda.device(DEV):
            m = Matcher(num_node="all", use_mutual=False, **CFG)
            T = m.SC2_PCR(torch.from_numpy(src).to(DEV)[None], torch.from_numpy(tgt).to(DEV)[None])
            res = {k: _bytes(m.last[k]) for k in STAGES}
            res.update(out=_bytes(T), labels=_bytes(m._labels), T=T[0].cpu().numpy())
        _cache[key] = res
    return _cache[key]


def _padded(pairs, n_cap=None):
    n_cap = n_cap or max(len(s) for s, _ in pairs)
    src = np.full((len(pairs), n_cap, 3), np.nan, np.float32)
    tgt = np.full((len(pairs), n_cap, 3), np.nan, np.float32)
    for b, (s, t) in enumerate(pairs):
        src[b, :len(s)], tgt[b, :len(t)] = s, t
    return torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), [len(s) for s, _ in pairs]


def _batch(pairs, n_cap=None, **kw):
    """One ``BatchMatcher.SC2_PCR`` call on the pairs (padded to n_cap with NaN rows); per pair the same dict as ``_single``."""
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    with torch.cuda.device(DEV):
        m = BatchMatcher(num_node="all", use_mutual=False, **CFG, **kw)
        src, tgt, counts = _padded(pairs, n_cap)
        T = m.SC2_PCR(src, tgt, counts=counts)
        assert T.shape == (len(pairs), 4, 4) and m._labels.shape == (len(pairs), src.shape[1]) and len(m.last) == len(pairs)
        res = []
        for b, n in enumerate(counts):
            r = {k: _bytes(m.last[b][k]) for k in STAGES}
            r.update(out=_bytes(m.last[b]["out"]), labels=_bytes(m.last[b]["labels"]), T=T[b].cpu().numpy())
            assert _bytes(T[b]) == r["out"]
            assert (m._labels[b, n:] == 0).all(), "labels are 0 from a pair's count on"
            res.append(r)
    return res


def _assert_same(got, want, what):
    for k in ("out", "labels") + STAGES:
        assert got[k] == want[k], f"{what}: {k} differs from the single call"


def _planted(seed, n, share, noise=0.05):
    src, tgt, _, _, _ = RO.planted_case(seed, n, share, noise=noise)
    return src, tgt


def _goldens():
    z = [np.load(p) for p in sorted(glob.glob(os.path.join(G, "sc2pcr_s[0-3].npz")))]
    assert [len(x["src"]) for x in z] == [1500, 2500, 800, 1200]
    for x in z:
        assert all(float(x[k]) == CFG[k] for k in CFG)
    return z


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_four_goldens_in_one_call_and_in_reversed_order():
    z = _goldens()
    pairs = [(x["src"], x["tgt"]) for x in z]
    want = [_single(("golden", i), *p) for i, p in enumerate(pairs)]
    got = _batch(pairs, n_cap=2500)
    for i in range(4):
        _assert_same(got[i], want[i], f"golden {i}")
        err = np.abs(got[i]["T"] - z[i]["T_ref"]).max()
        print(f"  golden {i}: |T - T_ref| = {err:.2e}")
        assert err < 2e-3
    rev = _batch(pairs[::-1], n_cap=2500)
    for i in range(4):
        _assert_same(rev[3 - i], want[i], f"golden {i} in reversed order")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_word_tile_and_chunk_edges_in_one_batch():
    """64 | 65: one bit word and two; 256 | 257: one SC_TILE and two; per = ceil(n / 8) = 8, 9, 17, 32, 33, 126: even (16-byte
    entry loads) and odd side by side; 12, 13, 25, 51, 51, 200 seeds: no multiple of SK_TS = 16."""
    counts = (64, 65, 129, 256, 257, 1001)
    assert all(int(n * CFG["ratio"]) % 16 for n in counts)
    pairs = [_planted(100 + n, n, 0.5) for n in counts]
    got = _batch(pairs)
    for n, p, g in zip(counts, pairs, got):
        _assert_same(g, _single(("edges", n), *p), f"n = {n}")


def test_a_batch_below_k1_uses_the_four_nearest():
    counts = (5, 7, 20, 29)
    pairs = [_planted(200 + n, n, 0.5) for n in counts]
    got = _batch(pairs)
    for n, p, g in zip(counts, pairs, got):
        want = _single(("below k1", n), *p)
        _assert_same(g, want, f"n = {n}")
        assert len(want["knn"]) == int(n * CFG["ratio"]) * 4 * 4            # (k1, k2) = (4, 4), int32


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_pairs_leave_the_iterations_independently():
    """An exact pair (every correspondence an inlier, no noise: the refinement stands still at once), a noisy pair with a
    share of 0.3 and a pair without any inlier, in one batch and in another order; and a batch of one."""
    pairs = [_planted(301, 600, 1.0, noise=0.0), _planted(302, 900, 0.3), _planted(303, 700, 0.0)]
    keys = [("exits", 301), ("exits", 302), ("exits", 303)]
    want = [_single(k, *p) for k, p in zip(keys, pairs)]
    assert len({w["out"] for w in want}) == 3
    for order in ((0, 1, 2), (2, 0, 1)):
        got = _batch([pairs[i] for i in order])
        for g, i in zip(got, order):
            _assert_same(g, want[i], f"pair {i} in order {order}")
    for i in range(3):
        _assert_same(_batch([pairs[i]])[0], want[i], f"pair {i} as a batch of one")


def test_more_pairs_than_one_launch_sequence_takes():
    """33 pairs: the entry makes one launch sequence per 32 pairs, the second with every pointer moved on by 32 pairs."""
    counts = [40 + 3 * b for b in range(33)]
    pairs = [_planted(800 + b, n, 0.5) for b, n in enumerate(counts)]
    got = _batch(pairs)
    for b, (p, g) in enumerate(zip(pairs, got)):
        _assert_same(g, _single(("33 pairs", b), *p), f"pair {b} of 33")


def test_no_iterations_staged_calls_single_call_and_batch_agree(monkeypatch):
    """num_iterations = 0: the confidence stays at ones and the per-seed power iteration does not run.  Counts (129, 65)
    padded to n_cap = 160: each pair alone through ``Matcher`` equals the five staged calls (their tight bits come from
    k_sc_tight_bits, the one call's from the build pass, which runs without any product) in every stage and in the
    transformation, bit for bit; and the batch equals the single calls bit for bit."""
    import gcl_amd.scripts.SC2_PCR as S
    cfg = dict(CFG, num_iterations=0)
    counts = (129, 65)
    pairs = [_planted(900 + n, n, 0.5) for n in counts]
    want = []
    with torch.cuda.device(DEV):
        for src, tgt in pairs:
            s, t = torch.from_numpy(src).to(DEV)[None], torch.from_numpy(tgt).to(DEV)[None]
            res = []
            for one_call in (False, True):
                monkeypatch.setattr(S, "ONE_CALL", one_call)
                m = S.Matcher(num_node="all", use_mutual=False, **cfg)
                T = m.SC2_PCR(s, t)
                r = {k: m.last[k].clone() for k in STAGES}
                r.update(out=T.clone(), labels=m._labels)
                res.append(r)
            staged, one = res
            assert staged["labels"] is None and one["labels"] is not None
            assert torch.equal(staged["out"], one["out"])
            for k in STAGES:
                assert torch.equal(staged[k].to(one[k].dtype), one[k]), k
            assert bool((one["conf"] == 1).all())
            want.append({k: _bytes(v) for k, v in one.items()})
        monkeypatch.setattr(S, "ONE_CALL", True)
        m = S.BatchMatcher(num_node="all", use_mutual=False, **cfg)
        src, tgt, cnt = _padded(pairs, 160)
        T = m.SC2_PCR(src, tgt, counts=cnt)
        for b, n in enumerate(counts):
            got = {k: _bytes(m.last[b][k]) for k in ("out", "labels") + STAGES}
            _assert_same(got, want[b], f"n = {n}, no iterations")
            assert _bytes(T[b]) == got["out"] and bool((m._labels[b, n:] == 0).all())
    assert want[0]["out"] != want[1]["out"]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_stale_scratch_and_labels_beyond_the_counts():
    """The C entry itself, twice on one scratch block that is filled with 0xFF in between (and before): same bytes."""
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    counts = (300, 65, 257)
    pairs = [_planted(400 + n, n, 0.5) for n in counts]
    n_seeds = [int(n * CFG["ratio"]) for n in counts]
    B, n_cap, S, k1 = 3, 320, max(n_seeds), CFG["k1"]
    with torch.cuda.device(DEV):
        src, tgt, _ = _padded(pairs, n_cap)
        scratch = torch.empty(lib.gcl_sc2_register_batch_scratch_bytes(B, n_cap), dtype=torch.uint8, device=DEV)
        runs = []
        for _ in range(2):
            scratch.fill_(0xFF)
            out = dict(conf=torch.empty((B, n_cap), device=DEV), seeds=torch.empty((B, S), dtype=torch.int64, device=DEV),
                       knn=torch.empty((B, S, k1), dtype=torch.int32, device=DEV), seed_trans=torch.empty((B, S, 12), device=DEV),
                       fitness=torch.empty((B, S), device=DEV), best=torch.empty(B, dtype=torch.int32, device=DEV),
                       out=torch.empty((B, 16), device=DEV), labels=torch.full((B, n_cap), 7.0, device=DEV))
            _lib.check(lib.gcl_sc2_register_batch(
                _lib.ptr(src), _lib.ptr(tgt), B, n_cap, (ctypes.c_int32 * B)(*counts), (ctypes.c_int32 * B)(*n_seeds),
                CFG["d_thre"], CFG["num_iterations"], CFG["nms_radius"], k1, CFG["k2"], CFG["inlier_threshold"], 1.2, 20,
                _lib.ptr(scratch), *(_lib.ptr(out[k]) for k in ("conf", "seeds", "knn", "seed_trans", "fitness", "best", "out",
                                                                "labels")), _lib.stream()), "gcl_sc2_register_batch")
            runs.append(out)
        for b, (n, ns) in enumerate(zip(counts, n_seeds)):
            want = _single(("stale", n), *pairs[b])
            for r in runs:
                got = dict(conf=r["conf"][b, :n], seeds=r["seeds"][b, :ns], knn=r["knn"][b, :ns], seed_trans=r["seed_trans"][b, :ns],
                           fitness=r["fitness"][b, :ns], best=r["best"][b], out=r["out"][b], labels=r["labels"][b, :n])
                _assert_same({k: _bytes(v.contiguous()) for k, v in got.items()}, want, f"n = {n}")
                assert (r["labels"][b, n:] == 0).all()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_another_stream_and_sub_batches():
    from gcl_amd import _lib
    counts = (257, 129, 300, 64, 200)
    pairs = [_planted(500 + n, n, 0.5) for n in counts]
    want = [_single(("streams", n), *p) for n, p in zip(counts, pairs)]
    with torch.cuda.device(DEV):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _batch(pairs)
        torch.cuda.current_stream().wait_stream(side)
    for n, g, w in zip(counts, got, want):
        _assert_same(g, w, f"n = {n} on another stream")
    one = _lib.load().gcl_sc2_register_batch_scratch_bytes(1, 300)
    from gcl_amd.scripts.SC2_PCR import split_batch
    assert split_batch(5, one, 2 * one + 1) == [(0, 2), (2, 4), (4, 5)]
    got = _batch(pairs, max_batch_bytes=2 * one + 1)
    for n, g, w in zip(counts, got, want):
        _assert_same(g, w, f"n = {n} in sub-batches of 2 + 2 + 1")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_estimator_with_draws_equals_one_estimator_call_per_pair():
    """num_node = 700 rows drawn WITH replacement from 500-row clouds (as KITTI's 8000 from 5000), planted descriptors: the
    1-NN of source row i is target row perm[i], by a wide margin."""
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    B, N, NODE = 3, 500, 700
    rng = np.random.RandomState(6)
    x0, x1, f0, f1 = [], [], [], []
    for b in range(B):
        src, tgt = _planted(600 + b, N, 0.5)
        perm = rng.permutation(N)
        F0 = rng.normal(size=(N, 32)).astype(np.float32)
        F0 /= np.linalg.norm(F0, axis=1, keepdims=True)
        F1, xyz1 = np.empty_like(F0), np.empty_like(tgt)
        F1[perm], xyz1[perm] = F0 + 0.01 * rng.normal(size=F0.shape).astype(np.float32), tgt
        F1 /= np.linalg.norm(F1, axis=1, keepdims=True)
        for lst, a in ((x0, src), (x1, xyz1), (f0, F0), (f1, F1)):
            lst.append(torch.from_numpy(a))
    with torch.cuda.device(DEV):
        x0, x1, f0, f1 = (torch.stack(v).to(DEV) for v in (x0, x1, f0, f1))
        np.random.seed(13)
        one = Matcher(num_node=NODE, use_mutual=False, **CFG)
        want = [one.estimator(x0[b:b + 1], x1[b:b + 1], f0[b:b + 1], f1[b:b + 1]) for b in range(B)]
        end = np.random.get_state()
        np.random.seed(13)
        T, labels, sc, tc = BatchMatcher(num_node=NODE, use_mutual=False, **CFG).estimator(x0, x1, f0, f1)
        assert (np.random.get_state()[1] == end[1]).all()
        assert T.shape == (B, 4, 4) and labels.shape == (B, NODE) and sc.shape == tc.shape == (B, NODE, 3)
        for b in range(B):
            for got, ref in zip((T, labels, sc, tc), want[b]):
                assert _bytes(got[b]) == _bytes(ref[0]), b
        assert len({_bytes(T[b]) for b in range(B)}) == B and float(labels.sum()) > 0.3 * B * NODE


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def _twin_pair(seed, shift_voxels=(8, 0, 0), voxel=0.3):
    """tests/test_gpu_ransac_batch.py's helper, restated: an eval pair whose second cloud is the first one moved by a multiple
    of 8 voxels -- twin voxels get equal features from an untrained network, everything else is an outlier."""
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


@pytest.fixture(scope="module")
def eval_setup():
    from gcl_amd.model import load_model
    from gcl_amd.scripts import test_kitti as TK
    from gcl_amd.scripts.SC2_PCR import Matcher
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
    assert all(len(p["sinput0_C"]) > 1500 for p in pairs)
    ref = {}

    def per_pair_loop(batch_pairs):
        if batch_pairs not in ref:
            np.random.seed(9)
            ref[batch_pairs] = (TK.eval_pairs(m, pairs, Matcher(num_node=2000, use_mutual=False, **CFG), device=DEV,
                                              batch_pairs=batch_pairs, subsample_size=1500, n_points=1500),
                                np.random.get_state())
        return ref[batch_pairs]

    return m, pairs, per_pair_loop


@pytest.mark.parametrize("batch_pairs", [4, 3])
def test_eval_pairs_with_one_sc2_registration_call_per_chunk(eval_setup, batch_pairs):
    """batch_pairs = 3 leaves a last chunk of one pair."""
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    from gcl_amd.scripts.eval_batch import eval_pairs
    m, pairs, per_pair_loop = eval_setup
    one, end = per_pair_loop(batch_pairs)
    np.random.seed(9)
    bat = eval_pairs(m, pairs, BatchMatcher(num_node=2000, use_mutual=False, **CFG), device=DEV, batch_pairs=batch_pairs,
                     subsample_size=1500, n_points=1500, batch_registration=True)
    assert (np.random.get_state()[1] == end[1]).all(), "np.random is consumed in the per-pair loop's order"
    assert len(bat["T_est"]) == 4 and bat["n_pairs"] == 4
    for a, b in zip(one["T_est"], bat["T_est"]):
        assert torch.equal(a, b), "one registration call per chunk must not change a single bit"
    assert one["success"] == bat["success"] and one["rte"] == bat["rte"]
    assert all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(one["rre"], bat["rre"]))
