"""The loops that match a chunk of pairs (BatchMatcher.estimator / match_pairs, FeatureRansac.estimator, eval_per_pair,
evaluate_scene, validate_pairs) make ONE search call per chunk -- the per-pair entries are replaced by functions that raise
-- and give, bit for bit, what the same call gives pair by pair.  Per-pair host draws are replayed through ``seeds`` / a
re-seeded ``np.random``."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402
from test_gpu_sc2_bench import CFG_3DMATCH, EVAL_CFG, _record          # noqa: E402
from test_gpu_val_pose import _twin_pair                               # noqa: E402

DEV = "cuda:0"
B = 3


def _raise(name):
    def blocked(*args, **kwargs):
        raise AssertionError(f"{name} was called: the chunk's matching must be one batch call")
    return blocked


def _block(monkeypatch):
    """Every per-pair search / mutual-filter entry the loops used to call, in every module that imported the name, and the
    single native entries themselves."""
    import gcl_amd.generalization_ETH.evaluate as E
    import gcl_amd.lib.ransac as R
    import gcl_amd.lib.validation as V
    import gcl_amd.scripts.SC2_PCR as S
    for mod in (S, R, E, V):
        monkeypatch.setattr(mod, "pdist_min", _raise(mod.__name__ + ".pdist_min"))
    monkeypatch.setattr(R, "mutual_correspondences", _raise("mutual_correspondences"))
    monkeypatch.setattr(E, "_mutual", _raise("evaluate._mutual (gcl_mutual_match)"))
    monkeypatch.setattr(E, "match_fragments", _raise("match_fragments"))
    from gcl_amd import _lib
    lib = _lib.load()
    for name in ("gcl_mutual_match", "gcl_mutual_correspondences", "gcl_nn_rowmin", "gcl_nn_rowmin_any"):
        monkeypatch.setattr(lib, name, _raise(name))


@pytest.fixture
def per_pair_entries_blocked(monkeypatch):
    _block(monkeypatch)


def _same(a, b):
    return a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _pairs(seed, sizes, c=33):
    rng = np.random.RandomState(seed)
    recs = [_record(rng, n, m, c=c) for n, m in sizes]
    return recs, [tuple(torch.from_numpy(x).to(DEV) for x in r[:4]) for r in recs]


# ---- BatchMatcher ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimator_reference():
    """[B, N, ...] inputs and, per ``num_node``, the draws and the results of the estimator called pair by pair."""
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    _, dev = _pairs(31, [(400, 450)] * B)
    stacked = [torch.stack([p[k] for p in dev]) for k in range(4)]
    ref = {}
    with torch.cuda.device(DEV):
        for num_node in ("all", 250):
            m = BatchMatcher(**dict(CFG_3DMATCH, num_node=num_node))
            np.random.seed(5)
            seeds = [m.draw_seed(400, 450) for _ in range(B)]
            ref[num_node] = (seeds, [m.estimator(*(x[b:b + 1] for x in stacked), seeds=seeds[b:b + 1]) for b in range(B)])
    return stacked, ref


@pytest.mark.parametrize("num_node", ("all", 250))
def test_batch_matcher_estimator_is_one_call_and_bitwise_pair_by_pair(estimator_reference, per_pair_entries_blocked, num_node):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    stacked, ref = estimator_reference
    seeds, one = ref[num_node]
    m = BatchMatcher(**dict(CFG_3DMATCH, num_node=num_node))
    with torch.cuda.device(DEV):
        got = m.estimator(*stacked, seeds=seeds)
        np.random.seed(5)
        drawn = m.estimator(*stacked)                                    # the draws made inside, in pair order
    for b in range(B):
        for k in range(4):
            assert _same(got[k][b:b + 1], one[b][k]), (b, k)
            assert _same(drawn[k][b:b + 1], one[b][k]), (b, k)


@pytest.mark.parametrize("num_node", ("all", 250))
def test_match_pairs_on_ragged_pairs(num_node):
    """Rows below a pair's count are ``match_pair``'s; with an integer ``num_node`` the np.random stream after the call is
    where B ``match_pair`` calls in a row leave it."""
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    _, dev = _pairs(32, [(300, 340), (557, 500), (130, 777)])
    m = BatchMatcher(**dict(CFG_3DMATCH, num_node=num_node))
    with torch.cuda.device(DEV):
        np.random.seed(9)
        one = [m.match_pair(*(x[None] for x in p)) for p in dev]
        after_pairs = np.random.get_state()
        np.random.seed(9)
        src, tgt, counts = m.match_pairs(dev)
        after_batch = np.random.get_state()
    assert counts == ([300, 557, 130] if num_node == "all" else [250] * 3)
    assert src.shape == tgt.shape == (B, max(counts), 3) and src.dtype == torch.float32
    for b in range(B):
        assert _same(src[b, :counts[b]], one[b][0][0]) and _same(tgt[b, :counts[b]], one[b][1][0]), b
    assert after_pairs[0] == after_batch[0] and after_pairs[2:] == after_batch[2:]
    assert np.array_equal(after_pairs[1], after_batch[1])
    if num_node != "all":                                                # the draws did move the stream
        np.random.seed(9)
        assert not np.array_equal(np.random.get_state()[1], after_batch[1])


def test_match_pairs_is_one_call(per_pair_entries_blocked):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    _, dev = _pairs(32, [(300, 340), (557, 500), (130, 777)])
    with torch.cuda.device(DEV):
        src, tgt, counts = BatchMatcher(**CFG_3DMATCH).match_pairs([tuple(x[None] for x in p) for p in dev])
    assert counts == [300, 557, 130] and bool(torch.isfinite(src[1]).all())


# ---- FeatureRansac ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ransac_reference():
    from gcl_amd.lib.ransac import FeatureRansac
    _, dev = _pairs(33, [(400, 450)] * B, c=32)
    stacked = [torch.stack([p[k] for p in dev]) for k in range(4)]
    ref = {}
    with torch.cuda.device(DEV):
        for mutual in (False, True):
            m = FeatureRansac.eth(mutual_filter=mutual)
            ref[mutual] = [m.estimator(*(x[b:b + 1] for x in stacked), seeds=[11 + b]) for b in range(B)]
    return stacked, ref


@pytest.mark.parametrize("mutual", (False, True))
def test_feature_ransac_estimator_is_one_call_and_bitwise_pair_by_pair(ransac_reference, per_pair_entries_blocked, mutual):
    from gcl_amd.lib.ransac import FeatureRansac
    stacked, ref = ransac_reference
    m = FeatureRansac.eth(mutual_filter=mutual)
    with torch.cuda.device(DEV):
        got = m.estimator(*stacked, seeds=[11, 12, 13])
        if mutual:
            n_mutual = m.last.n_mutual.tolist()
            assert all(60 < k < 400 for k in n_mutual), n_mutual        # the planted share and more: the filter did filter
    for b in range(B):
        for k in range(4):
            assert _same(got[k][b:b + 1], ref[mutual][b][k]), (b, k)


# ---- the benchmark loop ----------------------------------------------------------------------------------------------------
def test_eval_per_pair_chunks_are_one_call_each(monkeypatch):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair
    rng = np.random.RandomState(13)
    records = [_record(rng, n, m) for n, m in [(300, 340), (557, 500), (900, 777), (431, 431), (640, 901), (350, 352)]]
    with torch.cuda.device(DEV):
        one = eval_per_pair(records, Matcher(**CFG_3DMATCH), EVAL_CFG, scene_ind=2)
        _block(monkeypatch)
        batch = eval_per_pair(records, BatchMatcher(**CFG_3DMATCH), EVAL_CFG, batch_pairs=B, scene_ind=2)
    cols = list(range(9)) + [11]
    assert one[:, cols].tobytes() == batch[:, cols].tobytes()
    assert (batch[:, 0] == 1).all() and (batch[:, 9:11] > 0).all()


# ---- feature-match recall of a scene ---------------------------------------------------------------------------------------
def test_evaluate_scene_matches_its_pairs_in_chunks(monkeypatch):
    import gcl_amd.generalization_ETH.evaluate as E
    from gcl_amd import synthetic
    scene = EO.scene_case(synthetic.make_box_cloud(11, n_points=8000, cube=8.0))
    args = (scene["fragments"], scene["keypoints"], scene["gt_log"])
    calls = []
    batch_fn = E.match_fragments_batch
    monkeypatch.setattr(E, "match_fragments_batch", lambda jobs, *a, **k: (calls.append(len(jobs)), batch_fn(jobs, *a, **k))[1])
    with torch.cuda.device(DEV):
        one = E.evaluate_scene(*args, descriptors=scene["descriptors"], max_batch_bytes=1)       # a pair per chunk: old path
        assert calls == []
        lib, m = E._lib.load(), [len(d) for d in scene["descriptors"]]
        pair_bytes = max(4 * (lib.gcl_nn_rowmin_scratch_len(a, b) + lib.gcl_nn_rowmin_scratch_len(b, a)) for a in m for b in m)
        two = E.evaluate_scene(*args, descriptors=scene["descriptors"], max_batch_bytes=2 * pair_bytes)   # >= 2 pairs a chunk
        assert calls and min(calls) >= 2
        _block(monkeypatch)
        calls_before = list(calls)
        out = E.evaluate_scene(*args, descriptors=scene["descriptors"])                          # the five logged pairs: one chunk
    assert calls == calls_before + [5] and sum(calls_before) <= 5
    assert out["gt_match"] == 5 and out["recall"] == 100.0
    want = EO.scene_table(scene["keypoints"], scene["descriptors"], scene["gt_log"])
    for res in (one, two, out):
        assert np.array_equal(res["table"], want) and res["table"].tobytes() == one["table"].tobytes()


# ---- the validation loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsample_size", (700, 6000))
def test_validate_pairs_chunk_is_one_call(monkeypatch, subsample_size):
    """Three clouds of 5 - 6 thousand rows; 700: every pair is searched through its two draws (row lists), 6000: whole clouds."""
    import gcl_amd.lib.validation as V
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    torch.manual_seed(5)
    model = FinestContrastiveLossTrainer(make_config(hit_ratio_thresh=0.3), device=DEV).model
    pairs = [_twin_pair(80 + k, (8 * (k % 2), 0, 8 * (k // 2))) for k in range(B)]
    n = [len(p["sinput0_C"]) for p in pairs]
    assert all(700 < k < 6000 for k in n), n
    with torch.cuda.device(DEV):
        np.random.seed(3)
        m1, t1, d1 = V.validate_pairs(model, pairs, batch_pairs=1, subsample_size=subsample_size)
        _block(monkeypatch)
        np.random.seed(3)
        m3, t3, d3 = V.validate_pairs(model, pairs, batch_pairs=B, subsample_size=subsample_size)
    assert t1.shape == (B, 6) and t1.tobytes() == t3.tobytes() and m1 == m3 and d1 == d3
    assert (t3[:, 4] == ([700] * B if subsample_size == 700 else n)).all()
