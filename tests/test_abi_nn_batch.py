"""The batch matching entries (gcl_nn_rowmin_batch, gcl_mutual_match_batch, gcl_mutual_correspondences_batch) without a
GPU: exported with the header's argument counts, every refusal comes before any launch and names the entry and the search
/ pair at fault, and the scratch length is host arithmetic."""
import ctypes
import os
import re

from gcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gcl_nn_rowmin_batch", "gcl_nn_rowmin_batch_scratch_len", "gcl_mutual_match_batch",
           "gcl_mutual_correspondences_batch")
P8 = 8          # a non-null pointer value that is never dereferenced: the checks come before any HIP call


def _search(ma=10, mb=10, **over):
    s = _lib.NnSearch()
    s.a = s.b = s.dmin = s.argmin = P8
    s.ma, s.mb = ma, mb
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _table(*recs):
    arr = (type(recs[0]) * len(recs))(*recs)
    return arr, ctypes.addressof(arr)


def _refused(rc, *words):
    msg = _lib.load().gcl_last_error()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_entries_are_exported_with_the_headers_argument_counts():
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcl_amd.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    # the records of the binding table have the header's layout: ten pointers, two offsets, two sizes / nine and two
    assert ctypes.sizeof(_lib.NnSearch) == 10 * 8 + 2 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.MutualJob) == 9 * 8 + 2 * 4


def test_nn_rowmin_batch_refusals():
    lib = _lib.load()
    tab, at = _table(_search(), _search(67, 203))
    assert lib.gcl_nn_rowmin_batch_scratch_len(at, 2, 33) > 0
    call = lambda host, dev, P, c, scratch=P8: lib.gcl_nn_rowmin_batch(host, dev, P, c, 0, scratch, None)
    _refused(call(at, P8, 0, 33), "gcl_nn_rowmin_batch", "number of searches")
    _refused(call(at, P8, -3, 33), "gcl_nn_rowmin_batch", "number of searches")
    _refused(call(None, P8, 2, 33), "gcl_nn_rowmin_batch", "null")
    _refused(call(at, None, 2, 33), "gcl_nn_rowmin_batch", "null")
    _refused(call(at, P8, 2, 0), "gcl_nn_rowmin_batch", "1 .. 128")
    _refused(call(at, P8, 2, 129), "gcl_nn_rowmin_batch", "1 .. 128")
    _refused(call(at, P8, 2, 33, None), "gcl_nn_rowmin_batch", "scratch")
    for field in ("a", "b", "dmin", "argmin"):
        bad, at_bad = _table(_search(), _search(**{field: None}))
        _refused(call(at_bad, P8, 2, 33), "gcl_nn_rowmin_batch", "search 1", "null")
    for sizes in (dict(ma=0), dict(mb=0), dict(ma=-4)):
        bad, at_bad = _table(_search(**sizes), _search())
        _refused(call(at_bad, P8, 2, 33), "gcl_nn_rowmin_batch", "search 0", "empty")
    bad, at_bad = _table(_search(), _search(), _search(pts_a=P8, src=P8, tgt=P8))
    _refused(call(at_bad, P8, 3, 33), "gcl_nn_rowmin_batch", "search 2", "go together")
    bad, at_bad = _table(_search(pts_b=P8, src=P8, tgt=P8))
    _refused(call(at_bad, P8, 1, 33), "gcl_nn_rowmin_batch", "search 0", "go together")
    bad, at_bad = _table(_search(pts_a=P8, pts_b=P8, src=P8))
    _refused(call(at_bad, P8, 1, 33), "gcl_nn_rowmin_batch", "search 0", "src and tgt")
    # a table whose scratch offsets were never filled (or were filled for another width) is refused, not run
    raw, at_raw = _table(_search(), _search(67, 203))
    _refused(call(at_raw, P8, 2, 33), "gcl_nn_rowmin_batch", "search 0", "scratch offsets")


def test_nn_rowmin_batch_scratch_len():
    lib = _lib.load()
    for ma, mb in ((1, 1), (67, 203), (5000, 5000), (130, 9)):
        for c in (1, 16, 32, 33, 64, 128):
            tab, at = _table(_search(ma, mb))
            n = lib.gcl_nn_rowmin_batch_scratch_len(at, 1, c)
            assert n >= lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c) > 0
            if c in (16, 32, 64):
                assert n >= lib.gcl_nn_rowmin_scratch_len(ma, mb)
            assert tab[0].bi_off == 0 and tab[0].part_off >= (mb + 1) // 2 * 2 * c
    tab, at = _table(_search(), _search(67, 203))
    assert lib.gcl_nn_rowmin_batch_scratch_len(at, 0, 32) == 0
    assert lib.gcl_nn_rowmin_batch_scratch_len(at, -1, 32) == 0
    assert lib.gcl_nn_rowmin_batch_scratch_len(at, 2, 0) == 0
    assert lib.gcl_nn_rowmin_batch_scratch_len(at, 2, 129) == 0
    assert lib.gcl_nn_rowmin_batch_scratch_len(None, 2, 32) == 0
    n = lib.gcl_nn_rowmin_batch_scratch_len(at, 2, 32)
    # the searches' ranges of scratch are disjoint and inside the length returned
    assert 0 == tab[0].bi_off < tab[0].part_off <= tab[1].bi_off < tab[1].part_off < n


def _job(m0=10, m1=10, **over):
    j = _lib.MutualJob()
    j.nn01 = j.nn10 = j.xyz0 = j.xyz1 = j.pairs = j.src = j.tgt = j.count = P8
    j.m0, j.m1 = m0, m1
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_mutual_batch_refusals():
    lib = _lib.load()
    tab, at = _table(_job(), _job())
    for name, fn, arg in (("gcl_mutual_match_batch", lib.gcl_mutual_match_batch, 0.1),
                          ("gcl_mutual_correspondences_batch", lib.gcl_mutual_correspondences_batch, 3)):
        _refused(fn(at, P8, 0, arg, None), name, "number of pairs")
        _refused(fn(None, P8, 2, arg, None), name, "null")
        _refused(fn(at, None, 2, arg, None), name, "null")
        bad, at_bad = _table(_job(), _job(count=None))
        _refused(fn(at_bad, P8, 2, arg, None), name, "pair 1", "null")
        bad, at_bad = _table(_job(m0=-1), _job())
        _refused(fn(at_bad, P8, 2, arg, None), name, "pair 0")
    bad, at_bad = _table(_job(), _job(T=P8, xyz1=None))
    _refused(lib.gcl_mutual_match_batch(at_bad, P8, 2, 0.1, None), "gcl_mutual_match_batch", "pair 1", "transformation")
    bad, at_bad = _table(_job(), _job(m1=0))
    _refused(lib.gcl_mutual_correspondences_batch(at_bad, P8, 2, 3, None), "gcl_mutual_correspondences_batch", "pair 1", ">= 1")
    bad, at_bad = _table(_job(src=None))
    _refused(lib.gcl_mutual_correspondences_batch(at_bad, P8, 1, 3, None), "gcl_mutual_correspondences_batch", "pair 0", "null")
