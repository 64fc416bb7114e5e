"""The record entries (gcl_*_bwd_emit, gcl_*_records) and the ordered row sum without a GPU: exported with the header's
argument counts, the record-count and scratch formulas are the header's, and every refusal comes before any HIP call and
names the entry."""
import ctypes
import os
import re

from gcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMIT = ("gcl_group_loss_bwd_emit", "gcl_circle_group_bwd_emit", "gcl_neg_loss_bwd_emit", "gcl_triplet_bwd_emit",
        "gcl_pair_terms_bwd_emit")
ENTRIES = EMIT + ("gcl_group_loss_records", "gcl_circle_group_records", "gcl_neg_loss_records", "gcl_triplet_records",
                  "gcl_pair_terms_records", "gcl_ordered_row_sum_window", "gcl_ordered_row_sum_scratch_len",
                  "gcl_ordered_row_sum")
P8 = 8          # a non-null pointer value that is never dereferenced: the checks come before any HIP call
PAIR = 4        # GCL_LOSS_PAIR


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
        params = m.group(1).strip()
        assert (0 if params in ("", "void") else params.count(",") + 1) == len(_lib.SIGNATURES[name][1]), name
    # an emit entry takes its atomic twin's arguments with dF replaced by the record lists
    for name, extra in zip(EMIT, (3, 3, 2, 3, 3)):
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-5]][1]) + extra, name
    assert "ordered.hip" in _lib.SOURCES and "ordered.hip" not in _lib.TRAINING_STEP_SOURCES


def test_record_counts_and_scratch_length_are_the_documented_formulas():
    lib = _lib.load()
    for members, n_sel in ((0, 1), (1, 1), (350, 29), (4096, 256), (3_000_000_000, 1024)):
        for flags in range(16):
            pair = bool(flags & PAIR)
            assert lib.gcl_group_loss_records(members, n_sel, flags) == members + n_sel * (2 if pair else 0)
            assert lib.gcl_circle_group_records(members, n_sel, flags & 7) == members + n_sel * (3 if pair else 1)
    for n_sel in (0, -3):
        assert lib.gcl_group_loss_records(100, n_sel, PAIR) == 0 and lib.gcl_circle_group_records(100, n_sel, 0) == 0
    assert lib.gcl_group_loss_records(-1, 5, 0) == 0 and lib.gcl_circle_group_records(-1, 5, 0) == 0
    for m in (1, 255, 256, 257, 5000, 2 ** 30):
        assert lib.gcl_neg_loss_records(m) == 2 * m and lib.gcl_triplet_records(m) == 3 * m
        assert lib.gcl_pair_terms_records(m) == m
    for m in (0, -7):
        assert lib.gcl_neg_loss_records(m) == 0 and lib.gcl_triplet_records(m) == 0 and lib.gcl_pair_terms_records(m) == 0
    for n_rec, n_rows in ((1, 1), (64, 7), (5000, 530000), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.gcl_ordered_row_sum_scratch_len(n_rec, n_rows) == 2 + 2 * n_rows + 3 * n_rec
    assert lib.gcl_ordered_row_sum_scratch_len(0, 100) == 0 and lib.gcl_ordered_row_sum_scratch_len(-4, 100) == 0
    assert lib.gcl_ordered_row_sum_scratch_len(100, 0) == 0 and lib.gcl_ordered_row_sum_scratch_len(100, -1) == 0
    assert lib.gcl_ordered_row_sum_scratch_len(100, 2 ** 31) == 0
    w = lib.gcl_ordered_row_sum_window()
    assert w >= 64 and w % 64 == 0


def _group(lib, **over):
    a = dict(f=P8, c=32, index=P8, goff=P8, flag=P8, sel=P8, n_sel=10, pos_thresh=0.1, fin_thresh=0.2, flags=0, pairpos=None,
             gpos=P8, gfin=P8, rec_off=P8, rec_row=P8, rec_val=P8, n_rec=100, stream=None)
    a.update(over)
    return lib.gcl_group_loss_bwd_emit(*a.values())


def _circle(lib, **over):
    a = dict(f=P8, c=32, index=P8, goff=P8, flag=P8, sel=P8, n_sel=10, pos_thresh=0.1, fin_thresh=0.2, log_scale=16.0,
             flags=0, pairpos=None, gpos=P8, gfin=P8, gmean=None, rec_off=P8, rec_row=P8, rec_val=P8, n_rec=100, stream=None)
    a.update(over)
    return lib.gcl_circle_group_bwd_emit(*a.values())


def _neg(lib, **over):
    a = dict(f=P8, c=32, sel1=P8, sel2=P8, arg=P8, dmin=P8, keep=P8, m=10, thresh=1.4, out=P8, gneg=P8, rec_row=P8,
             rec_val=P8, n_rec=20, stream=None)
    a.update(over)
    return lib.gcl_neg_loss_bwd_emit(*a.values())


def _triplet(lib, **over):
    a = dict(f0=P8, n0=50, f1=P8, n1=60, c=32, ap=P8, neg=P8, tag=P8, keep=None, m=10, work=P8, out=P8, g=P8, rec_row0=P8,
             rec_val0=P8, rec_row1=P8, rec_val1=P8, n_rec=30, stream=None)
    a.update(over)
    return lib.gcl_triplet_bwd_emit(*a.values())


def _pairs(lib, **over):
    a = dict(f0=P8, n0=50, f1=P8, n1=60, c=32, pairs=P8, keep=None, m=10, mode=0, thresh=0.0, eps=0.0, work=P8, out=P8, g=P8,
             rec_row0=P8, rec_val0=P8, rec_row1=P8, rec_val1=P8, n_rec=10, stream=None)
    a.update(over)
    return lib.gcl_pair_terms_bwd_emit(*a.values())


def _sum(lib, **over):
    a = dict(rec_row=P8, rec_val=P8, n_rec=10, c=32, n_rows=100, scratch=P8, df=P8, stream=None)
    a.update(over)
    return lib.gcl_ordered_row_sum(*a.values())


def test_refusals_come_before_any_launch_and_name_the_entry():
    lib = _lib.load()
    cases = (
        ("gcl_group_loss_bwd_emit", _group, ("f", "index", "goff", "flag", "sel", "gpos", "gfin", "rec_off", "rec_row",
                                             "rec_val"), ("n_sel", "n_rec")),
        ("gcl_circle_group_bwd_emit", _circle, ("f", "index", "goff", "flag", "sel", "gpos", "gfin", "rec_off", "rec_row",
                                                "rec_val"), ("n_sel", "n_rec")),
        ("gcl_neg_loss_bwd_emit", _neg, ("f", "sel1", "sel2", "arg", "dmin", "keep", "out", "gneg", "rec_row", "rec_val"),
         ("m", "n_rec")),
        ("gcl_triplet_bwd_emit", _triplet, ("f0", "f1", "ap", "neg", "tag", "work", "out", "g", "rec_row0", "rec_val0",
                                            "rec_row1", "rec_val1"), ("m", "n_rec")),
        ("gcl_pair_terms_bwd_emit", _pairs, ("f0", "f1", "pairs", "work", "out", "g", "rec_row0", "rec_val0", "rec_row1",
                                             "rec_val1"), ("m", "n_rec")),
        ("gcl_ordered_row_sum", _sum, ("rec_row", "rec_val", "scratch", "df"), ("n_rec",)),
    )
    for name, call, ptrs, counts in cases:
        for p in ptrs:                                  # a null pointer with non-zero counts
            _refused(call(lib, **{p: None}), name, "null")
        for k in counts:                                # a negative count
            _refused(call(lib, **{k: -1}), name, "negative")
        for c in (0, 65, -2):
            _refused(call(lib, c=c), name, "width")
    # a capacity below the entry's own record count, where the host knows it
    _refused(_neg(lib, n_rec=19), "gcl_neg_loss_bwd_emit", "n_rec")
    _refused(_triplet(lib, n_rec=29), "gcl_triplet_bwd_emit", "n_rec")
    _refused(_pairs(lib, n_rec=9), "gcl_pair_terms_bwd_emit", "n_rec")
    # the switches of the atomic twins
    _refused(_group(lib, flags=PAIR), "gcl_group_loss_bwd_emit", "pair positions")
    _refused(_group(lib, flags=16), "gcl_group_loss_bwd_emit", "flags")
    _refused(_circle(lib, flags=8), "gcl_circle_group_bwd_emit", "flags")
    _refused(_circle(lib, log_scale=0.0), "gcl_circle_group_bwd_emit", "log_scale")
    _refused(_pairs(lib, mode=3), "gcl_pair_terms_bwd_emit", "no backward")
    # record rows are int32
    _refused(_triplet(lib, n0=2 ** 31), "gcl_triplet_bwd_emit", "2^31")
    _refused(_pairs(lib, n1=2 ** 31), "gcl_pair_terms_bwd_emit", "2^31")
    _refused(_sum(lib, n_rows=2 ** 31), "gcl_ordered_row_sum", "n_rows")
    _refused(_sum(lib, n_rows=-1), "gcl_ordered_row_sum", "n_rows")


def test_empty_calls_return_without_a_launch():
    """Zero counts with null pointers are no error and touch nothing (no GPU here: a launch would fail)."""
    lib = _lib.load()
    assert _sum(lib, n_rec=0, rec_row=None, rec_val=None, scratch=None) == 0
    assert _sum(lib, n_rows=0, df=None, scratch=None) == 0
