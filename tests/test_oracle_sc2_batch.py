"""Batched SC2-PCR registration without a GPU: the exports, signatures, scratch size and argument checks of
gcl_sc2_register_batch / gcl_sc2_register_batch_scratch_bytes, and the host logic of ``BatchMatcher`` (its draws against
``Matcher.match_pair``'s, the sub-batch chunking, the two refusals)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from gcl_amd import _lib

NEW = ("gcl_sc2_register_batch_scratch_bytes", "gcl_sc2_register_batch")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_the_batch_entries(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        decl = re.search(r"^\w+ %s\(([^;]*)\);" % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    i = re.search(r"^\w+ %s\(" % NEW[0], header, re.M).start()
    comment = header[header.rindex("/*", 0, i):i]                        # the footprint is stated where the entry is declared
    assert "528 MB" in comment and "SCRATCH FOOTPRINT" in comment


def test_batch_scratch_bytes(lib):
    size = lib.gcl_sc2_register_batch_scratch_bytes
    for bad in ((0, 5000), (-1, 5000), (4, 0), (4, -7), (4, 8193)):
        assert size(*bad) == 0, bad
    for n_cap in (1, 5, 64, 257, 1001, 5000, 8000, 8192):
        one = lib.gcl_sc2_register_scratch_bytes(n_cap)
        assert one > 0
        for batch in (1, 2, 5, 8, 33):
            got = size(batch, n_cap)
            assert got >= batch * one and got == batch * size(1, n_cap) and size(1, n_cap) % 256 == 0, (batch, n_cap)
    assert 520e6 < size(1, 8000) < 540e6                                 # the stated footprint: ~ 8 n^2 bytes per pair


def test_batch_argument_errors_come_before_any_hip_call(lib):
    """Dummy pointers throughout: a call that got past the checks would reach HIP (GCL_ERR_HIP, -2, without a GPU)."""
    p8 = ctypes.c_void_p(8)
    i32x4 = lambda *v: (ctypes.c_int32 * 4)(*v)

    def call(src=p8, tgt=p8, batch=4, n_cap=100, counts=i32x4(100, 60, 80, 100), n_seeds=i32x4(20, 12, 16, 20), k1=30, k2=20,
             scratch=p8, conf=p8, seeds=p8, knn=p8, seed_trans=p8, fitness=p8, best=p8, trans16=p8, labels=p8):
        return lib.gcl_sc2_register_batch(src, tgt, batch, n_cap, counts, n_seeds, 0.1, 10, 0.1, k1, k2, 0.1, 0.1, 20, scratch,
                                          conf, seeds, knn, seed_trans, fitness, best, trans16, labels, None)

    cases = [(dict([(name, None)]), b"null") for name in ("src", "tgt", "counts", "n_seeds", "scratch", "conf", "seeds", "knn",
                                                          "seed_trans", "fitness", "best", "trans16", "labels")]
    cases += [(dict(counts=i32x4(100, 101, 80, 100)), b"pair 1"), (dict(n_seeds=i32x4(20, 12, 0, 20)), b"pair 2"),
              (dict(n_seeds=i32x4(20, 61, 16, 20)), b"pair 1"), (dict(batch=0), b"batch"), (dict(batch=-2), b"batch"),
              (dict(n_cap=8193, counts=i32x4(8193, 8193, 8193, 8193)), b"n_cap"), (dict(n_cap=0), b"n_cap"),
              (dict(counts=i32x4(100, 29, 80, 100), n_seeds=i32x4(20, 5, 16, 20)), b"k1"), (dict(k1=33), b"k1"),
              (dict(k2=31), b"k2")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.gcl_last_error() and b"gcl_sc2_register_batch" in lib.gcl_last_error(), (kw, lib.gcl_last_error())


# ---- BatchMatcher's host logic ------------------------------------------------------------------------------------------------
def test_draw_seed_makes_match_pairs_draws():
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    assert BatchMatcher.accepts_batch and not getattr(Matcher, "accepts_batch", False)
    n0, n1, node = 500, 431, 700
    np.random.seed(21)
    a, b = np.random.choice(n0, node), np.random.choice(n1, node)          # Matcher.match_pair's two draws, in its order
    want = np.random.get_state()
    np.random.seed(21)
    got = BatchMatcher(num_node=node).draw_seed(n0, n1)
    state = np.random.get_state()
    assert state[0] == want[0] and (state[1] == want[1]).all() and state[2:] == want[2:]
    assert (got[0] == a).all() and (got[1] == b).all()
    np.random.seed(22)
    before = np.random.get_state()
    assert BatchMatcher(num_node="all").draw_seed(n0, n1) is None
    after = np.random.get_state()
    assert (before[1] == after[1]).all() and before[2:] == after[2:]


def test_sub_batches_under_a_byte_limit(lib):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, split_batch
    one = lib.gcl_sc2_register_batch_scratch_bytes(1, 1000)
    assert split_batch(5, one, 2 * one) == [(0, 2), (2, 4), (4, 5)]
    assert split_batch(5, one, 3 * one - 1) == [(0, 2), (2, 4), (4, 5)]
    assert split_batch(5, one, 5 * one) == [(0, 5)] and split_batch(5, one, 100 * one) == [(0, 5)]
    assert split_batch(5, one, 5 * one - 1) == [(0, 4), (4, 5)]
    assert split_batch(3, one, 0) == [(0, 1), (1, 2), (2, 3)]              # a pair always runs, whatever the limit
    assert split_batch(1, one, one) == [(0, 1)]
    assert BatchMatcher().max_batch_bytes == 8 << 30 and BatchMatcher(max_batch_bytes=123).max_batch_bytes == 123
    eight = lib.gcl_sc2_register_batch_scratch_bytes(1, 8000)
    assert split_batch(17, eight, 8 << 30) == [(0, 16), (16, 17)]          # the default: 16 pairs of 8000 per call


def test_plan_and_its_two_refusals():
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    m = BatchMatcher(ratio=0.2, max_points=1000, k1=30, k2=20)
    assert m.plan(2500, [1500, 2500, 800, 30]) == ([1000, 1000, 800, 30], [200, 200, 160, 6], 30, 20)
    assert m.plan(64, None, 3) == ([64, 64, 64], [12, 12, 12], 30, 20)
    assert m.plan(29, [5, 7, 20, 29]) == ([5, 7, 20, 29], [1, 1, 4, 5], 4, 4)      # the reference's k1 > n rule, all pairs
    with pytest.raises(ValueError, match="too few correspondences"):
        m.plan(100, [100, 4, 100])
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.plan(100, [100, 29, 100])
    with pytest.raises(ValueError, match="at most 8192"):                  # not a C-level refusal of a scratch size of 0
        BatchMatcher(max_points=9000).plan(8193, None, 2)
    assert BatchMatcher(max_points=8000).plan(8193, None, 2)[0] == [8000, 8000]
    x = torch.zeros(3, 100, 3)
    with pytest.raises(ValueError, match="too few correspondences"):       # before any GPU work: CPU tensors never get there
        m.SC2_PCR(x, x, counts=[100, 4, 100])
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.SC2_PCR(x, x, counts=[100, 29, 100])
    f = torch.zeros(3, 4, 32)
    with pytest.raises(ValueError, match="too few correspondences"):
        BatchMatcher(num_node="all").estimator(x[:, :4], x[:, :4], f, f)
