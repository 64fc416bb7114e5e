"""Feature-match recall on the GPU (csrc/match.hip, gcl_amd/generalization_ETH/evaluate.py) against the fp64 brute-force
restatement in tests/eth_eval_oracle.py.

Where the data makes fp32 arithmetic exact (lattice coordinates, descriptor entries that are small multiples of 1/16)
indices, distances and pair lists must be equal to the oracle's; elsewhere the chosen neighbour must be optimal within the
bound derived for the arithmetic form (stated at each test)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/eth_eval_oracle.py
import eth_eval_oracle as EO                                           # noqa: E402

DEV = "cuda:0"
M_SIZES = (1, 63, 64, 65, 257)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------
# 1. exact lattice
# ---------------------------------------------------------------------------------------------------------------
def _lattice(seed, m, n, coarse):
    """Multiples of 0.125 in [-64, 64] (``coarse``: of 8, so that most queries have several equidistant points); a third
    of the points are exact duplicates of earlier ones and every third query sits on a point."""
    rng = np.random.RandomState(seed)
    draw = (lambda k: rng.randint(-8, 9, (k, 3)) * 8.0) if coarse else (lambda k: rng.randint(-512, 513, (k, 3)) * 0.125)
    p = draw(n)
    k = n // 3
    if k:
        p[n - k:] = p[rng.randint(0, n - k, k)]
    q = draw(m)
    q[::3] = p[rng.randint(0, n, len(q[::3]))]
    return q.astype(np.float32), p.astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4099, 70001])
def test_nn3_exact_on_a_lattice(n):
    """Every fp32 difference, square and sum of these coordinates is exact (<= 2^22 in units of 1/64), so argmin must be
    the oracle's lowest-index minimum for EVERY query and d2min bit-equal, whatever the tile and chunk boundaries."""
    from gcl_amd import _lib
    from gcl_amd.lib.metrics import nn3_min
    lib = _lib.load()
    if n == 70001:
        assert lib.gcl_nn3_scratch_len(257, n) // (2 * 257) > 100, "this size is meant to span many chunks"
    if n <= 256:
        assert lib.gcl_nn3_scratch_len(257, n) == 0, "this size is meant to be a single chunk"
    for coarse in (False, True):
        q, p = _lattice(1000 * n + coarse, max(M_SIZES), n, coarse)
        d2_ref, arg_ref = EO.nn(q, p)
        P = dev(p)
        for m in M_SIZES:
            d2, arg = nn3_min(dev(q[:m]), P)
            assert d2.dtype == torch.float32 and arg.dtype == torch.int32 and d2.shape == arg.shape == (m,)
            arg, d2 = arg.cpu().numpy(), d2.cpu().numpy()
            assert np.array_equal(arg, arg_ref[:m]), (n, m, coarse, np.nonzero(arg != arg_ref[:m])[0][:5])
            assert np.array_equal(d2, d2_ref[:m].astype(np.float32)), (n, m, coarse)
            assert np.all(d2[::3] == 0.0)               # a query equal to a point
    # without the distances (d2min NULL), through the C ABI
    m = 65
    arg = torch.full((m,), -1, dtype=torch.int32, device=DEV)
    ns = lib.gcl_nn3_scratch_len(m, n)
    scratch = torch.empty(max(1, ns), dtype=torch.int32, device=DEV)
    Q = dev(q[:m])
    _lib.check(lib.gcl_nn3_rowmin(_lib.ptr(Q), m, _lib.ptr(P), n, None, 0, _lib.ptr(scratch), None, _lib.ptr(arg), None,
                                  _lib.stream()), "gcl_nn3_rowmin")
    assert np.array_equal(arg.cpu().numpy(), arg_ref[:m])


def test_nn3_empty_query_set():
    from gcl_amd.lib.metrics import nn3_min
    d2, arg, desc = nn3_min(torch.zeros((0, 3), device=DEV), torch.zeros((5, 3), device=DEV), torch.ones((5, 7), device=DEV))
    assert d2.shape == (0,) and arg.shape == (0,) and desc.shape == (0, 7)


# ---------------------------------------------------------------------------------------------------------------
# 2. far from the origin
# ---------------------------------------------------------------------------------------------------------------
def test_nn3_far_from_the_origin():
    """A jittered 5 cm grid centred at (800, -600, 50), m = 300, n = 20 000.  For every query the fp64 squared distance of the
    chosen point (from the fp32-rounded inputs) must be <= the fp64 minimum * (1 + 1e-6).

    Bound of the difference form: inside one binade the fp32 differences are exact, the square and the two FMAs round once
    each, so a computed distance is within (1 + 2^-24)^3 of the true one and the chosen point within twice that of the
    minimum: about 2.4e-7.  The expansion |q|^2 + |p|^2 - 2 q.p FAILS this test: its terms are ~10^6 with an fp32 ulp of
    0.06 - 0.12 m^2 against 2.5e-3 m^2 between neighbouring voxels (tests/test_oracle_eth_eval.py shows it on this data).
    d2min itself is held to 1e-6 relative (three roundings: 1.8e-7)."""
    from gcl_amd.lib.metrics import nn3_min
    q, p = EO.far_grid_case()
    assert q.shape == (300, 3) and p.shape == (20000, 3)
    d2_ref, _ = EO.nn(q, p)
    d2, arg = nn3_min(dev(q), dev(p))
    arg, d2 = arg.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)
    assert arg.min() >= 0 and arg.max() < len(p)
    chosen = ((q.astype(np.float64) - p[arg].astype(np.float64)) ** 2).sum(1)
    excess = chosen / d2_ref - 1
    print(f"  worst chosen / min - 1 = {excess.max():.3e}; worst |d2min / fp64 - 1| = {np.abs(d2 / chosen - 1).max():.3e}")
    assert np.all(chosen <= d2_ref * (1 + 1e-6))
    assert np.all(np.abs(d2 - chosen) <= 1e-6 * chosen)


# ---------------------------------------------------------------------------------------------------------------
# 3. fused gather
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 16, 32, 33])
def test_nn3_fused_gather(c):
    """desc is bit-equal to feat[argmin], from the search kernel (one chunk) and from the merge kernel (several)."""
    from gcl_amd import _lib
    from gcl_amd.lib.metrics import nn3_min
    lib = _lib.load()
    rng = np.random.RandomState(c)
    for m, n in ((300, 200), (300, 5000), (1, 1)):
        assert (lib.gcl_nn3_scratch_len(m, n) == 0) == (n <= 200)
        q = rng.uniform(-10, 10, (m, 3)).astype(np.float32)
        p = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
        feat = dev(rng.normal(size=(n, c)).astype(np.float32))
        d2, arg, desc = nn3_min(dev(q), dev(p), feat)
        d2b, argb = nn3_min(dev(q), dev(p))
        assert desc.shape == (m, c) and torch.equal(arg, argb) and torch.equal(d2, d2b)
        assert torch.equal(desc, feat[arg.long()])
        chosen = ((q.astype(np.float64) - p[arg.cpu().numpy()].astype(np.float64)) ** 2).sum(1)
        assert np.all(chosen <= EO.nn(q, p)[0] * (1 + 1e-6))


def test_find_nearest_voxel_feature_is_the_gather():
    from gcl_amd.generalization_ETH.evaluate import find_nearest_voxel_feature
    rng = np.random.RandomState(0)
    full, partial = rng.uniform(-3, 3, (900, 3)), rng.uniform(-3, 3, (70, 3))       # float64 hosts arrays, as open3d's
    feat = dev(rng.normal(size=(900, 32)).astype(np.float32))
    got = find_nearest_voxel_feature(torch.from_numpy(full), torch.from_numpy(partial).to(DEV), feat)
    ref = EO.nn(partial.astype(np.float32), full.astype(np.float32))[1]
    assert torch.equal(got, feat[torch.from_numpy(ref).to(DEV)])


# ---------------------------------------------------------------------------------------------------------------
# 4. mutual filter and counts
# ---------------------------------------------------------------------------------------------------------------
def _mutual_case(seed, m0, m1):
    rng = np.random.RandomState(seed)
    nn01 = rng.randint(0, m1, m0).astype(np.int64)
    nn10 = rng.randint(0, m0, m1).astype(np.int64)
    for i in rng.permutation(m0)[: max(1, (2 * m0) // 3)]:      # make two thirds of the sources mutual (later ones may undo some)
        nn10[nn01[i]] = i
    if m0 >= 5:                                                  # out-of-range entries: never dereferenced, never mutual
        bad = rng.permutation(m0)[: max(2, m0 // 10)]
        nn01[bad] = rng.choice([-1, m1, m1 + 5, -2 ** 31, 2 ** 31 - 1], len(bad))
    if m1 >= 3:
        bad = rng.permutation(m1)[: max(1, m1 // 10)]
        nn10[bad] = rng.choice([-1, m0, m0 + 3, -2 ** 31, 2 ** 31 - 1], len(bad))
    T = EO.rigid(rng, 20.0)[:3].astype(np.float32)
    kp1 = rng.uniform(-30, 30, (m1, 3)).astype(np.float32)
    j = np.clip(nn01, 0, m1 - 1)
    step = rng.normal(size=(m0, 3))
    step /= np.linalg.norm(step, axis=1, keepdims=True)
    inlier = rng.rand(m0) < 0.6
    length = np.where(inlier, rng.uniform(0.0, 0.05, m0), rng.uniform(0.5, 3.0, m0))
    kp0 = (EO.apply(T.astype(np.float64), kp1[j]) + step * length[:, None]).astype(np.float32)
    return nn01, nn10, kp0, kp1, T


def _run_mutual(nn01, nn10, kp0, kp1, T, tau, m0=None):
    from gcl_amd import _lib
    lib = _lib.load()
    m0 = len(nn01) if m0 is None else m0
    a, b = dev(nn01.astype(np.int32)), dev(nn10.astype(np.int32))
    pairs = torch.full((max(1, m0), 2), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((3, 2), -7, dtype=torch.int32, device=DEV)            # the middle row is the slot
    K0, K1, Td = (dev(kp0), dev(kp1), dev(T.reshape(-1))) if T is not None else (None, None, None)
    _lib.check(lib.gcl_mutual_match(_lib.ptr(a), m0, _lib.ptr(b), len(nn10), _lib.ptr(K0), _lib.ptr(K1), _lib.ptr(Td),
                                    ctypes.c_float(tau), _lib.ptr(pairs), _lib.ptr(stats[1]), _lib.stream()),
               "gcl_mutual_match")
    return pairs.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("m0,m1", [(1, 1), (5, 3), (64, 64), (130, 257), (1000, 777), (2500, 3000)])
def test_mutual_match_pairs_and_inlier_count(m0, m1):
    """Pairs and their order exactly the oracle's; the inlier count exact (residuals <= 0.05 or >= 0.5 by construction, and no
    fp64 residual within 1e-3 of tau, so fp32 rounding of ~1e-5 m cannot move one across); two runs bit-identical."""
    tau = 0.1
    nn01, nn10, kp0, kp1, T = _mutual_case(m0 * 7 + m1, m0, m1)
    want = EO.mutual(nn01, nn10)
    res = EO.residuals(want, kp0, kp1, T)
    assert len(res) == 0 or np.abs(res - tau).min() > 1e-3
    n_in = int((res < tau).sum())
    if m0 >= 64:
        assert 0 < n_in < len(want) < m0
    pairs, stats = _run_mutual(nn01, nn10, kp0, kp1, T, tau)
    assert stats[1].tolist() == [len(want), n_in] and np.all(stats[[0, 2]] == -7)
    assert np.array_equal(pairs[:len(want)], want)
    assert np.all(pairs[len(want):] == -7)                      # nothing is written past the list
    pairs2, stats2 = _run_mutual(nn01, nn10, kp0, kp1, T, tau)
    assert np.array_equal(pairs, pairs2) and np.array_equal(stats, stats2)
    # no transformation: the pairs alone, stats[1] = 0
    pairs3, stats3 = _run_mutual(nn01, nn10, None, None, None, tau)
    assert np.array_equal(pairs3, pairs) and stats3[1].tolist() == [len(want), 0]
    # no sources: the counters are still written
    _, stats4 = _run_mutual(nn01, nn10, kp0, kp1, T, tau, m0=0)
    assert stats4[1].tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------
# 5. calculate_M
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 32, 64])
def test_calculate_M_exact_on_representable_features(c):
    """Entries are multiples of 1/16 in [-1/2, 1/2]: differences, squares and the <= 64-term sums are exact in fp32, so both
    1-NN searches return the oracle's lowest-index minima (many rows are duplicated) and the pairs are exactly its pairs."""
    from gcl_amd.generalization_ETH.evaluate import calculate_M
    rng = np.random.RandomState(c)
    m0, m1 = 333, 270
    a = rng.randint(-8, 9, (m0, c)) / 16.0
    b = rng.randint(-8, 9, (m1, c)) / 16.0
    b[:150] = a[rng.permutation(m0)[:150]]
    b[200:230] = b[:30]                   # duplicated targets
    a[300:320] = a[:20]                   # duplicated sources
    want = EO.mutual(EO.nn(a, b)[1], EO.nn(b, a)[1])
    assert 50 < len(want) < 150 + 30
    for src, tgt in ((dev(a, torch.float32), dev(b, torch.float32)), (a.astype(np.float32), b.astype(np.float32))):
        got = calculate_M(src, tgt)
        assert got.dtype == torch.int64 and got.is_cuda and got.shape == (len(want), 2)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("c", [16, 32, 64])
def test_calculate_M_on_normalised_features(c):
    """L2-normalised random features: each GPU arg-minimum must be near-optimal (fp64 distance <= min * (1 + 1e-5): a c-term
    fp32 chain is good to (c + 3) 2^-24 <= 4e-6 per distance, twice that between two candidates), and the pairs must be the
    oracle's filter applied to those arg-minima."""
    from gcl_amd.generalization_ETH.evaluate import calculate_M
    from gcl_amd.lib.metrics import pdist_min
    rng = np.random.RandomState(100 + c)
    m0, m1 = 700, 650
    a = rng.normal(size=(m0, c))
    b = rng.normal(size=(m1, c))
    b[:400] = a[:400] + 0.1 * rng.normal(size=(400, c))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    b = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)
    A, B = dev(a), dev(b)
    nn01 = pdist_min(A, B, "SquareL2")[1].cpu().numpy().astype(np.int64)
    nn10 = pdist_min(B, A, "SquareL2")[1].cpu().numpy().astype(np.int64)
    for x, y, arg in ((a, b, nn01), (b, a, nn10)):
        chosen = ((x.astype(np.float64) - y[arg].astype(np.float64)) ** 2).sum(1)
        assert np.all(chosen <= EO.nn(x, y)[0] * (1 + 1e-5))
    want = EO.mutual(nn01, nn10)
    assert len(want) > 200
    assert np.array_equal(calculate_M(A, B).cpu().numpy(), want)


def test_calculate_M_rejects_other_widths():
    from gcl_amd.generalization_ETH.evaluate import calculate_M, match_fragments
    x = torch.zeros((8, 48), device=DEV)
    with pytest.raises(ValueError, match="16, 32 or 64"):
        calculate_M(x, x)
    with pytest.raises(ValueError, match="16, 32 or 64"):
        match_fragments(torch.zeros((8, 3), device=DEV), torch.zeros((8, 3), device=DEV), x, x, None)
    assert calculate_M(torch.zeros((0, 32), device=DEV), torch.zeros((4, 32), device=DEV)).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------
# 6. scene
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from gcl_amd import synthetic
    return EO.scene_case(synthetic.make_box_cloud(11, n_points=8000, cube=8.0))


class _HostReads:
    """Counts device -> host reads made through torch.Tensor (cpu / item / tolist / numpy / to('cpu') / bool, int, float, index)."""

    NAMES = ("cpu", "item", "tolist", "numpy", "to", "__bool__", "__int__", "__float__", "__index__")

    def __init__(self):
        self.count = 0
        self._depth = 0

    def __enter__(self):
        self._own = {n: torch.Tensor.__dict__[n] for n in self.NAMES if n in torch.Tensor.__dict__}
        for name in self.NAMES:
            setattr(torch.Tensor, name, self._wrap(name, getattr(torch.Tensor, name)))
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            if name in self._own:
                setattr(torch.Tensor, name, self._own[name])
            else:
                delattr(torch.Tensor, name)           # back to the inherited method

    def _wrap(self, name, fn):
        counter = self

        def wrapped(t, *args, **kw):
            reads = t.is_cuda and counter._depth == 0
            if reads and name == "to":
                target = kw.get("device", args[0] if args else None)
                reads = isinstance(target, (str, torch.device)) and torch.device(target).type == "cpu"
            if reads:
                counter.count += 1
            counter._depth += 1               # one read may be built from another (tolist -> ...): counted once
            try:
                return fn(t, *args, **kw)
            finally:
                counter._depth -= 1
        return wrapped


def test_scene_with_planted_descriptors(scene):
    """Recall 100 %, the inlier count of every logged pair = the number of keypoints the two fragments share, the whole
    table equal to the brute-force one; the pair that is not in the log counts (0, 0, 0).  With the rolled copy: recall 0."""
    from gcl_amd.generalization_ETH.evaluate import evaluate_scene
    want = EO.scene_table(scene["keypoints"], scene["descriptors"], scene["gt_log"])
    with _HostReads() as reads:
        out = evaluate_scene(scene["fragments"], scene["keypoints"], scene["gt_log"], descriptors=scene["descriptors"])
    assert reads.count == 1, "the scene's counts leave the device in one read"
    ids = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    assert out["pairs"] == ids and out["table"].shape == (6, 3)
    assert out["recall"] == 100.0 and out["correct_match"] == 5 and out["gt_match"] == 5
    assert [int(r[0]) for r in out["table"]] == [scene["shared"][p] if p != (0, 3) else 0 for p in ids]
    assert np.array_equal(out["table"], want)
    assert out["ave_num_inliers"] == np.mean([scene["shared"][p] for p in ids if p != (0, 3)])
    # device tensors give the same result
    again = evaluate_scene(None, [dev(k) for k in scene["keypoints"]], scene["gt_log"],
                           descriptors=[dev(d) for d in scene["descriptors"]])
    assert np.array_equal(again["table"], out["table"])
    bad = evaluate_scene(scene["fragments"], scene["keypoints"], scene["gt_log"], descriptors=scene["shuffled"])
    assert bad["recall"] == 0.0 and bad["correct_match"] == 0 and bad["gt_match"] == 5 and bad["ave_num_inliers"] == 0.0
    assert np.array_equal(bad["table"], EO.scene_table(scene["keypoints"], scene["shuffled"], scene["gt_log"]))


def test_match_fragments_handle(scene):
    from gcl_amd.generalization_ETH.evaluate import match_fragments
    k, d, T = scene["keypoints"], scene["descriptors"], scene["gt_log"]["1_2"]
    slot = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    with _HostReads() as reads:
        h = match_fragments(k[1], k[2], dev(d[1]), dev(d[2]), T, tau1=0.1, out=slot)
        assert reads.count == 0, "match_fragments reads nothing back"
        pairs, n_in = h.result()
        assert reads.count == 1
    want = EO.mutual(EO.nn(d[1], d[2])[1], EO.nn(d[2], d[1])[1])
    assert np.array_equal(pairs.cpu().numpy(), want) and n_in == scene["shared"][(1, 2)]
    assert slot.tolist() == [len(want), n_in] and h.stats.data_ptr() == slot.data_ptr()


def test_scene_with_a_network(scene):
    """A small ResUNetFatBN (random weights, n_out = 32, eval mode): the per-fragment descriptors of the scene driver are
    bitwise those of the reference-shaped per-pair recomputation (both clouds voxelised and run for every pair), the scene
    result is the oracle's aggregation of the product's own per-pair table, and the pair loop reads the device once."""
    from gcl_amd.generalization_ETH import evaluate as E
    from gcl_amd.model import load_model
    torch.manual_seed(4)
    model = load_model("ResUNetFatBN")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV)
    with pytest.raises(RuntimeError, match="eval"):
        E.fragment_descriptors(model.train(), scene["fragments"][0], scene["keypoints"][0], 0.05)
    model.eval()
    frags, kps = scene["fragments"], scene["keypoints"]
    descs = [E.fragment_descriptors(model, frags[i], kps[i], 0.05) for i in range(4)]
    assert all(d.shape == (len(k), 32) and d.dtype == torch.float32 and d.is_cuda for d, k in zip(descs, kps))
    with torch.no_grad():
        for a, b in ((0, 1), (2, 3)):                     # evaluate.py:138-145, once per pair
            s0, s1, v0, v1 = E.prepare_pcd_to_input(frags[a], frags[b], 0.05, DEV)
            F0, F1 = model(s0).F.detach(), model(s1).F.detach()
            assert len(v0) == len(F0) and len(v1) == len(F1)
            src = E.find_nearest_voxel_feature(v0.to(DEV), torch.from_numpy(kps[a]).to(DEV), F0)
            tgt = E.find_nearest_voxel_feature(v1.to(DEV), torch.from_numpy(kps[b]).to(DEV), F1)
            assert torch.equal(src, descs[a]) and torch.equal(tgt, descs[b])
    # the scene driver: one descriptor computation per fragment, one read in the pair loop
    calls = []
    real = E.fragment_descriptors
    with _HostReads() as reads:
        def counted(*args, **kw):
            out = real(*args, **kw)
            calls.append(reads.count)
            reads.count = 0               # what follows the last fragment's descriptors is the pair loop
            return out
        E.fragment_descriptors = counted
        try:
            out = E.evaluate_scene(frags, kps, scene["gt_log"], model=model)
        finally:
            E.fragment_descriptors = real
    assert len(calls) == 4
    assert reads.count == 1
    given = E.evaluate_scene(None, kps, scene["gt_log"], descriptors=descs)
    assert np.array_equal(out["table"], given["table"])
    want = EO.scene(out["table"], 0.05)
    assert {k: out[k] for k in want} == want
    assert np.all(out["table"][:, 2] == [1, 1, 0, 1, 1, 1]) and np.all(out["table"][2] == 0)
    rows = out["table"][out["table"][:, 2] == 1]
    assert np.all(rows[:, 1] >= 0) and np.all(rows[:, 1] <= 1) and np.all(rows[:, 0] == np.round(rows[:, 0]))


def test_scene_with_the_sc2pcr_matcher(scene):
    """With a Matcher every logged pair is registered too; on planted descriptors the estimate is the pair's transformation:
    the logged inverse equals gt_log's matrix (which moves the target into the source frame) to 1e-3 -- keypoints of a few
    metres in fp32, exact correspondences among the mutual pairs."""
    from gcl_amd.generalization_ETH.evaluate import evaluate_scene
    from gcl_amd.scripts.SC2_PCR import Matcher
    out = evaluate_scene(scene["fragments"], scene["keypoints"], scene["gt_log"], descriptors=scene["descriptors"],
                         matcher=Matcher())
    assert out["recall"] == 100.0
    assert [(a, b) for a, b, _ in out["pred_log"]] == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    for a, b, T in out["pred_log"]:
        err = np.abs(T - scene["gt_log"][f"{a}_{b}"]).max()
        print(f"  pair {a}_{b}: max |inverse(estimate) - gt| = {err:.2e}")
        assert T.shape == (4, 4) and err < 1e-3
