"""Batched RANSAC registration and the mutual filter without a GPU: the exports and argument checks of
gcl_ransac_register_batch / gcl_ransac_batch_scratch_bytes / gcl_mutual_correspondences, the numpy oracle of the mutual rule
(tests/mutual_ransac_oracle.py) on constructions whose mutual pairs are known, and the Python surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402
import mutual_ransac_oracle as MO                                      # noqa: E402
import ransac_oracle as RO                                             # noqa: E402

NEW = ("gcl_ransac_batch_scratch_bytes", "gcl_ransac_register_batch", "gcl_mutual_correspondences")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_the_batch_entries(lib):
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name in NEW:
        assert hasattr(raw, name) and f" {name}(" in header, name
    assert "40 MB" in header and "SCRATCH FOOTPRINT" in header          # the footprint is stated where the entry is declared


def test_batch_argument_errors_come_before_any_hip_call(lib):
    """Dummy pointers throughout: a call that got past the checks would reach HIP (GCL_ERR_HIP, -2, without a GPU)."""
    p8 = ctypes.c_void_p(8)
    seeds = (ctypes.c_uint64 * 4)(1, 2, 3, 4)

    def call(src=p8, tgt=p8, batch=4, n_cap=100, n_dev=p8, ransac_n=3, sim=0.9, check=0.3, dist=0.3, iters=1000, conf=0.999,
             seeds=seeds, chunk=0, scratch=p8, trans=p8, info=p8, fit=p8):
        return lib.gcl_ransac_register_batch(src, tgt, batch, n_cap, n_dev, ransac_n, sim, check, dist, iters, conf, seeds,
                                             chunk, scratch, trans, info, fit, None, None, None)

    for kw, word in ((dict(src=None), b"null"), (dict(tgt=None), b"null"), (dict(seeds=None), b"null"),
                     (dict(scratch=None), b"null"), (dict(trans=None), b"null"), (dict(info=None), b"null"),
                     (dict(fit=None), b"null"), (dict(batch=0), b"batch"), (dict(batch=-3), b"batch"),
                     (dict(ransac_n=2), b"ransac_n"), (dict(ransac_n=5), b"ransac_n"), (dict(n_cap=2), b"fewer"),
                     (dict(n_cap=3, ransac_n=4), b"fewer"), (dict(n_cap=(1 << 24) + 1), b"more than"),
                     (dict(iters=0), b"max_iteration"), (dict(dist=0.0), b"max_corr_distance"),
                     (dict(dist=-1.0), b"max_corr_distance"), (dict(chunk=-1), b"chunk")):
        assert call(**kw) == -1, kw
        assert word in lib.gcl_last_error() and b"gcl_ransac_register_batch" in lib.gcl_last_error(), (kw, lib.gcl_last_error())


def test_mutual_correspondences_argument_errors(lib):
    p8 = ctypes.c_void_p(8)

    def call(nn01=p8, m0=10, nn10=p8, m1=10, xyz0=p8, xyz1=p8, min_count=3, src=p8, tgt=p8, count=p8):
        return lib.gcl_mutual_correspondences(nn01, m0, nn10, m1, xyz0, xyz1, min_count, src, tgt, count, None)

    for kw, word in ((dict(nn01=None), b"null"), (dict(nn10=None), b"null"), (dict(xyz0=None), b"null"),
                     (dict(xyz1=None), b"null"), (dict(src=None), b"null"), (dict(tgt=None), b"null"),
                     (dict(count=None), b"null"), (dict(m0=0), b"sizes"), (dict(m1=0), b"sizes"), (dict(m0=-1), b"sizes")):
        assert call(**kw) == -1, kw
        assert word in lib.gcl_last_error(), (kw, lib.gcl_last_error())


def test_batch_scratch_bytes(lib):
    one = lib.gcl_ransac_scratch_bytes(5000, 1024)
    sizes = [lib.gcl_ransac_batch_scratch_bytes(b, 5000, 1024) for b in (1, 2, 8, 64)]
    assert sizes == [one, 2 * one, 8 * one, 64 * one] and one > 0
    assert lib.gcl_ransac_batch_scratch_bytes(8, 5000, 0) == 8 * lib.gcl_ransac_scratch_bytes(5000, 0) > 8 * 30e6
    assert lib.gcl_ransac_batch_scratch_bytes(8, 6000, 1024) > sizes[2]
    for bad in ((0, 5000, 1024), (-1, 5000, 1024), (8, 0, 1024), (8, (1 << 24) + 1, 1024), (8, 5000, -1)):
        assert lib.gcl_ransac_batch_scratch_bytes(*bad) == 0, bad


def _points(seed, m0, m1):
    rng = np.random.RandomState(seed)
    return rng.uniform(-5, 5, (m0, 3)).astype(np.float32), rng.uniform(-5, 5, (m1, 3)).astype(np.float32)


def test_oracle_planted_features_are_all_mutual():
    F0, F1, perm = MO.planted_features(2)
    nn01, nn10, gap = MO.tables(F0, F1)
    assert gap >= 1e-3, gap
    assert (nn01 == perm).all() and (nn10[perm] == np.arange(300)).all()
    xyz0, xyz1 = _points(3, 300, 300)
    src, tgt, count = MO.correspondences(nn01, nn10, xyz0, xyz1, 4)
    assert tuple(count) == (300, 300) and (src == xyz0).all() and (tgt == xyz1[perm]).all()


def test_oracle_planted_motion_is_recovered():
    """The end-to-end GPU test's data: planted features on a planted motion -- the oracle registration on the oracle's list
    recovers it within tests/test_oracle_ransac.py's bounds."""
    F0, F1, perm = MO.planted_features(2)
    src, tgt, R, t, inl = RO.planted_case(11, 300, 0.4)
    xyz1 = np.empty_like(tgt)
    xyz1[perm] = tgt
    nn01, nn10, _ = MO.tables(F0, F1)
    s, g, count = MO.correspondences(nn01, nn10, src, xyz1, 3)
    assert count[0] == 300 and (s == src).all() and (g == tgt).all()
    r = RO.ransac(s, g, 3, 0.9, 0.3, 0.3, 4096, 0.0, 7, 1024)
    w = r["winner"]
    assert w >= 0 and np.abs(r["R"][w] - R).max() < 2e-2 and np.abs(r["t"][w] - t).max() < 0.2


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_oracle_funnel_boundary(ransac_n):
    """|M| = 1 + e: with e = ransac_n - 1 there are exactly ransac_n mutual pairs and the list is used (the >= boundary);
    one fewer and the rule falls back to all 40 sources."""
    xyz0, xyz1 = _points(4, MO.FUNNEL_M0, MO.FUNNEL_M1)
    for e, used in ((ransac_n - 1, True), (ransac_n - 2, False)):
        F0, F1 = MO.funnel_features(5, e)
        nn01, nn10, gap = MO.tables(F0, F1)
        assert gap >= 1e-3, gap
        far = [MO.FUNNEL_M0 - 1 - k for k in range(e)]
        rest = np.setdiff1d(np.arange(MO.FUNNEL_M0), far)
        assert (nn01[rest] == MO.FUNNEL_SINK).all() and nn10[MO.FUNNEL_SINK] == MO.FUNNEL_HALVED
        pairs = EO.mutual(nn01, nn10)
        want = sorted([(MO.FUNNEL_HALVED, MO.FUNNEL_SINK)] + [(MO.FUNNEL_M0 - 1 - k, 10 + k) for k in range(e)])
        assert [tuple(p) for p in pairs] == want and len(pairs) == 1 + e
        src, tgt, count = MO.correspondences(nn01, nn10, xyz0, xyz1, ransac_n)
        if used:
            assert tuple(count) == (ransac_n, ransac_n)
            assert (src[:ransac_n] == xyz0[pairs[:, 0]]).all() and (tgt[:ransac_n] == xyz1[pairs[:, 1]]).all()
            assert (src[ransac_n:] == 0).all() and (tgt[ransac_n:] == 0).all()
        else:
            assert tuple(count) == (MO.FUNNEL_M0, ransac_n - 1)
            assert (src == xyz0).all() and (tgt == xyz1[nn01]).all()


@pytest.mark.parametrize("m0,m1", [(1, 1), (63, 300), (64, 64), (65, 63), (300, 65)])
def test_oracle_random_tables_against_a_plain_loop(m0, m1):
    nn01, nn10 = MO.random_tables(m0 * 1000 + m1, m0, m1)
    if m0 >= 63:
        assert (nn01 == -1).any() and (nn01 == m1).any()
    want = MO.loop_list(nn01, nn10)
    assert [tuple(p) for p in EO.mutual(nn01, nn10)] == want
    xyz0, xyz1 = _points(6, m0, m1)
    k = len(want)
    for min_count in (k, k + 1):
        src, tgt, count = MO.correspondences(nn01, nn10, xyz0, xyz1, min_count)
        if min_count <= k:
            assert tuple(count) == (k, k) and (src[k:] == 0).all() and (tgt[k:] == 0).all()
            assert all((src[q] == xyz0[i]).all() and (tgt[q] == xyz1[j]).all() for q, (i, j) in enumerate(want))
        else:
            assert tuple(count) == (m0, k) and (src == xyz0).all()
            for i in range(m0):
                assert (tgt[i] == (xyz1[nn01[i]] if 0 <= nn01[i] < m1 else 0)).all()


def test_feature_ransac_with_the_mutual_filter_needs_a_gpu():
    from gcl_amd.lib import ransac as R
    m = R.FeatureRansac(0.3, mutual_filter=True)
    assert m.mutual_filter and m.accepts_batch and not R.FeatureRansac(0.3).mutual_filter
    assert R.FeatureRansac.kitti(0.3, mutual_filter=True).mutual_filter and R.FeatureRansac.eth(mutual_filter=True).mutual_filter
    assert not R.FeatureRansac.kitti(0.3).mutual_filter and not R.FeatureRansac.eth().mutual_filter
    assert R.FeatureRansac(0.3, seed=5).draw_seed() == 5
    x, f = torch.randn(2, 8, 3), torch.randn(2, 8, 32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            m.estimator(x, x, f, f)
        with pytest.raises(RuntimeError, match="GPU"):
            R.registration_ransac_based_on_mutual_feature_matching(x[0], x[0], f[0], f[0])
        with pytest.raises(RuntimeError, match="GPU"):
            R.ransac_correspondences_batch(x, x, 0.3)
    with pytest.raises(NotImplementedError, match="registration_ransac_based_on_mutual_feature_matching"):
        R.registration_ransac_based_on_feature_matching(x[0], x[0], f[0], f[0], mutual_filter=True)


def test_eval_pairs_refuses_a_matcher_without_a_batch_estimator_first():
    """Before any GPU work: neither the model nor the pairs are touched."""
    from gcl_amd.scripts.eval_batch import eval_pairs

    class OnePairMatcher:
        def estimator(self, *a):
            raise AssertionError("must not be called")

    with pytest.raises(ValueError, match="batch_registration"):
        eval_pairs(None, iter(()), OnePairMatcher(), batch_registration=True)
