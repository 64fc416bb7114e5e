"""Feature-matching RANSAC without a GPU: the C entry's exports and argument checks, and the numpy oracle itself
(tests/ransac_oracle.py) against independent facts -- the published splitmix64 sequence, scipy's Kabsch, a planted motion."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/ransac_oracle.py
import ransac_oracle as RO                                             # noqa: E402


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_the_ransac_entries(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gcl_ransac_scratch_bytes", "gcl_ransac_default_chunk", "gcl_ransac_register"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.gcl_ransac_default_chunk() >= 1024


def test_argument_errors_come_before_any_hip_call(lib):
    """Dummy pointers throughout: a call that got past the checks would reach HIP (GCL_ERR_HIP, -2, without a GPU)."""
    p8 = ctypes.c_void_p(8)

    def call(src=p8, tgt=p8, n=100, ransac_n=3, sim=0.9, check=0.3, dist=0.3, iters=1000, conf=0.999, chunk=0, scratch=p8,
             trans=p8, info=p8, fit=p8):
        return lib.gcl_ransac_register(src, tgt, n, ransac_n, sim, check, dist, iters, conf, 1, chunk, scratch, trans, info,
                                       fit, None, None, None)

    for kw, word in ((dict(src=None), b"null"), (dict(tgt=None), b"null"), (dict(scratch=None), b"null"),
                     (dict(trans=None), b"null"), (dict(info=None), b"null"), (dict(fit=None), b"null"),
                     (dict(ransac_n=2), b"ransac_n"), (dict(ransac_n=5), b"ransac_n"), (dict(n=2), b"fewer"),
                     (dict(n=3, ransac_n=4), b"fewer"), (dict(n=(1 << 24) + 1), b"more than"), (dict(iters=0), b"max_iteration"), (dict(dist=0.0), b"max_corr_distance"),
                     (dict(dist=-1.0), b"max_corr_distance"), (dict(chunk=-1), b"chunk")):
        assert call(**kw) == -1, kw
        assert word in lib.gcl_last_error(), (kw, lib.gcl_last_error())


def test_scratch_bytes(lib):
    sizes = [lib.gcl_ransac_scratch_bytes(n, 1024) for n in (3, 64, 256, 5000, 100000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.gcl_ransac_scratch_bytes(5000, 0) == lib.gcl_ransac_scratch_bytes(5000, lib.gcl_ransac_default_chunk())
    assert lib.gcl_ransac_scratch_bytes(5000, 2048) > lib.gcl_ransac_scratch_bytes(5000, 1024)
    assert lib.gcl_ransac_scratch_bytes(0, 0) == 0 and lib.gcl_ransac_scratch_bytes(10, -1) == 0


def test_oracle_draw_is_splitmix64():
    """Sample j of hypothesis h is output 4 h + j + 1 of splitmix64(seed); the generator's published first outputs for seed 0
    are E220A8397B1DCDAF, 6E789E6AA1B965F4, 06C45D188009454F, ..., and idx = floor(high 32 bits * n / 2^32)."""
    assert RO.draw(0, 0, 0, 256) == 0xE2                                  # 0xE220A839 * 256 >> 32
    assert RO.draw(0, 0, 1, 256) == 0x6E
    assert RO.draw(0, 0, 2, 1 << 16) == 0x06C4
    hs = np.arange(50)
    for seed, n in ((0, 256), (12345, 5000), ((1 << 64) - 1, 250)):       # the vectorised form wraps like the integers
        got = RO.draw_all(seed, hs, 4, n)
        want = np.array([[RO.draw(seed, int(h), j, n) for j in range(4)] for h in hs])
        assert (got == want).all() and got.min() >= 0 and got.max() < n


def test_oracle_kabsch_matches_scipy():
    from scipy.spatial.transform import Rotation
    src, tgt, R, t, inl = RO.planted_case(3, 64, 1.0, noise=0.0)
    S, T = src[None, :4].astype(np.float64), tgt[None, :4].astype(np.float64)
    Ro, to, sv = RO.kabsch(S, T)
    rot, _ = Rotation.align_vectors(T[0] - T[0].mean(0), S[0] - S[0].mean(0))      # T ~ rot S
    assert np.abs(Ro[0] - rot.as_matrix()).max() < 1e-9
    assert np.abs(Ro[0] - R).max() < 1e-5 and np.abs(to[0] - t).max() < 1e-4      # fp32 points: ~ 1e-6 of noise
    assert np.abs(Ro[0] @ Ro[0].T - np.eye(3)).max() < 1e-12 and np.linalg.det(Ro[0]) > 0 and sv[0, 0] >= sv[0, 1] >= sv[0, 2]
    # three points: H has rank 2 and the result must still be a proper rotation
    Ro3, to3, _ = RO.kabsch(S[:, :3], T[:, :3])
    assert np.abs(Ro3[0] - R).max() < 1e-5 and np.linalg.det(Ro3[0]) > 0


def test_oracle_recovers_a_planted_motion():
    src, tgt, R, t, inl = RO.planted_case(5, 256, 0.4)
    r = RO.ransac(src, tgt, 3, 0.9, 0.3, 0.3, 4096, 0.0, 7, 1024)
    st = r["status"]
    assert set(np.unique(st[st < 0])) <= {-1, -2, -3} and r["covered"] == 4096 and r["limit"] is None
    assert (st == -1).sum() > 0.85 * 4096                                  # the edge-length checker removes most samples
    w = r["winner"]
    assert w >= 0 and st[w] == st.max() >= 0.9 * len(inl)
    assert np.abs(r["R"][w] - R).max() < 2e-2 and np.abs(r["t"][w] - t).max() < 0.2
    assert r["borderline"].mean() < 0.005
    # the confidence stop: after the first chunk the limit is far below a chunk, so nothing else runs
    r2 = RO.ransac(src, tgt, 3, 0.9, 0.3, 0.3, 4096, 0.999, 7, 1024)
    assert r2["covered"] == 1024 and (r2["status"][1024:] == -4).all() and (r2["status"][:1024] == st[:1024]).all()
    assert r2["limit"] == RO.limit_of(int(r2["status"][:1024].max()), 256, 3, 0.999) < 1024
    assert RO.limit_of(256, 256, 3, 0.999) == 0 and RO.limit_of(0, 256, 3, 0.999) is None and RO.limit_of(9, 256, 3, 1.0) is None


def test_feature_ransac_needs_a_gpu():
    from gcl_amd.lib.ransac import FeatureRansac, registration_ransac_based_on_feature_matching
    m = FeatureRansac.kitti(0.3)
    assert (m.ransac_n, m.max_iteration, m.max_correspondence_distance, m.checker_distance) == (4, 4000000, 0.3, 0.3)
    e = FeatureRansac.eth()
    assert (e.ransac_n, e.max_iteration, e.max_correspondence_distance, e.checker_distance) == (3, 50000, 0.05, 0.05)
    x, f = torch.randn(1, 8, 3), torch.randn(1, 8, 32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            m.estimator(x, x, f, f)
    with pytest.raises(NotImplementedError, match="mutual_filter"):
        registration_ransac_based_on_feature_matching(x[0], x[0], f[0], f[0], mutual_filter=True)
