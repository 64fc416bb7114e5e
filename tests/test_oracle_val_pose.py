"""The device validation path's host side, without a GPU: the two native entries are exported and refuse bad arguments
before any launch, the Python entries fail loudly, the chunk former honours ``val_max_iter`` / ``batch_pairs``, and the
per-pair draws are ``find_corr``'s (the host ``_valid_epoch``'s) in its order."""
import ctypes

import numpy as np
import pytest
import torch

from gcl_amd import _lib


def test_both_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ("gcl_irls_pose_batch", "gcl_val_stats_batch", "gcl_irls_pose_scratch_len"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "valpose.hip" in _lib.SOURCES
    assert lib.gcl_irls_pose_scratch_len(0) == 0 and lib.gcl_irls_pose_scratch_len(5000) == 15000


def test_argument_refusals_come_before_any_launch():
    lib = _lib.load()
    p8 = ctypes.c_void_p(8)

    def pose(src=p8, tgt=p8, total=10, off=p8, B=1, n_iter=20, par0=1.0, halve=5, scratch=p8, T=p8, status=p8):
        return lib.gcl_irls_pose_batch(src, tgt, total, off, B, None, n_iter, par0, halve, scratch, T, status, None)

    for kwargs, word in [(dict(B=0), b"B = 0"), (dict(n_iter=-1), b"n_iter"), (dict(par0=0.0), b"par0"),
                         (dict(par0=-1.0), b"par0"), (dict(halve=0), b"halve_every"), (dict(off=None), b"offsets"),
                         (dict(T=None), b"T"), (dict(status=None), b"status"), (dict(src=None), b"src"),
                         (dict(tgt=None), b"tgt"), (dict(scratch=None), b"scratch"), (dict(total=-1), b"total")]:
        assert pose(**kwargs) == -1, kwargs
        msg = lib.gcl_last_error()
        assert b"gcl_irls_pose_batch" in msg and word in msg, (kwargs, msg)

    def stats(src=p8, tgt=p8, total=10, off=p8, xyz0=p8, total0=10, off0=p8, B=1, Te=p8, Tg=p8, out=p8):
        return lib.gcl_val_stats_batch(src, tgt, total, off, xyz0, total0, off0, B, Te, Tg, None, 1.0, 0.3, out, None)

    for kwargs, word in [(dict(B=0), b"B = 0"), (dict(off=None), b"offsets"), (dict(off0=None), b"offsets0"),
                         (dict(Te=None), b"T_est"), (dict(Tg=None), b"T_gt"), (dict(out=None), b"out"),
                         (dict(src=None), b"src"), (dict(xyz0=None), b"xyz0"), (dict(total0=-1), b"total0")]:
        assert stats(**kwargs) == -1, kwargs
        msg = lib.gcl_last_error()
        assert b"gcl_val_stats_batch" in msg and word in msg, (kwargs, msg)


def test_python_entries_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gcl_amd.lib.validation import validate_pairs
    from gcl_amd.util.transform_estimation import est_quad_linear_robust_batch
    with pytest.raises(RuntimeError, match="GPU"):
        est_quad_linear_robust_batch(torch.zeros(4, 3), torch.zeros(4, 3), [0, 4])
    with pytest.raises(RuntimeError, match="GPU"):
        validate_pairs(torch.nn.Linear(1, 1), [])


def test_chunk_former_honours_val_max_iter_and_batch_pairs():
    from gcl_amd.lib.validation import form_chunks
    assert [c for c in form_chunks(range(7), -1, 3)] == [[0, 1, 2], [3, 4, 5], [6]]
    assert [c for c in form_chunks(range(7), 0, 8)] == [[0, 1, 2, 3, 4, 5, 6]]
    assert [c for c in form_chunks(range(7), 5, 2)] == [[0, 1], [2, 3], [4]]
    assert [c for c in form_chunks(range(7), 4, 2)] == [[0, 1], [2, 3]]
    assert [c for c in form_chunks(range(7), 400, 1)] == [[i] for i in range(7)]
    assert [c for c in form_chunks([], 400, 8)] == []
    pulled = []

    def source():
        for i in range(10):
            pulled.append(i)
            yield i

    assert [c for c in form_chunks(source(), 3, 2)] == [[0, 1], [2]]
    assert len(pulled) <= 4                       # a loader is not drained past the limit
    with pytest.raises(ValueError):
        list(form_chunks(range(3), -1, 0))


def test_draws_are_find_corrs_in_its_order(monkeypatch):
    """``find_corr`` (what the host ``_valid_epoch`` calls per pair) with the 1-NN kernel replaced by a torch one, against
    ``draw_subsample`` over the same sequence of pairs: same index arrays, same generator state afterwards -- also for a
    pair at or below the subsample size, where neither draws."""
    from gcl_amd.lib import eval as ev
    from gcl_amd.lib.validation import draw_subsample

    def cpu_pdist_min(A, B, dist_type="L2", rows_a=None, rows_b=None):
        d = torch.cdist(A.double(), B.double())
        return d.min(1).values.float(), d.argmin(1).int()

    monkeypatch.setattr(ev, "pdist_min", cpu_pdist_min)
    sizes, sub = [(90, 70), (40, 80), (50, 30), (51, 51), (200, 45)], 50
    g = torch.Generator().manual_seed(3)
    clouds = [(torch.randn(n0, 3, generator=g), torch.randn(n1, 3, generator=g), torch.randn(n0, 8, generator=g),
               torch.randn(n1, 8, generator=g)) for n0, n1 in sizes]
    calls = []
    real_choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        calls.append((int(a), int(size), bool(replace)))
        return real_choice(a, size, replace=replace, p=p)

    monkeypatch.setattr(np.random, "choice", recording_choice)
    np.random.seed(11)
    host = [ev.DeferredCorr(x0, x1, F0, F1, subsample_size=sub) for x0, x1, F0, F1 in clouds]
    host_calls, host_state = list(calls), np.random.get_state()[1].copy()
    del calls[:]
    np.random.seed(11)
    mine = [draw_subsample(n0, n1, sub) for n0, n1 in sizes]
    assert calls == host_calls and len(calls) == 2 * 3
    assert calls[:2] == [(90, 50, False), (70, 50, False)] and calls[4:] == [(200, 50, False), (45, 45, False)]
    assert np.array_equal(np.random.get_state()[1], host_state)
    for h, (i0, i1) in zip(host, mine):
        if h.subsampled:
            assert np.array_equal(h.inds0, i0) and np.array_equal(h.inds1, i1)
        else:
            assert i0 is None and i1 is None
