"""The neighbourhood entries (gcl_nghb_range_max, gcl_nghb_flags, gcl_nghb_scratch_len, gcl_nghb_compact) without a GPU:
exported with the header's argument counts, the scratch length is the header's formula, and every refusal comes before any HIP
call and names the entry."""
import ctypes
import os
import re

import numpy as np

from gcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gcl_nghb_range_max", "gcl_nghb_flags", "gcl_nghb_scratch_len", "gcl_nghb_compact")
P8 = 8          # a non-null pointer value that is never dereferenced: the checks come before any HIP call


def _refused(rc, *words):
    msg = _lib.load().gcl_last_error()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def _i64(v):
    if v is None:
        return None, None
    a = np.asarray(v, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _i32(v):
    if v is None:
        return None, None
    a = np.asarray(v, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_entries_are_exported_with_the_headers_argument_counts():
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcl_amd.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    assert "nghb.hip" in _lib.SOURCES and "nghb.hip" not in _lib.TRAINING_STEP_SOURCES
    assert re.search(r"#define\s+GCL_NGHB_MAX_SCANS\s+(\d+)", src).group(1) == str(_lib.NGHB_MAX_SCANS)


def test_scratch_len_is_the_documented_formula():
    lib = _lib.load()
    for pc in (1, 255, 2047, 2048, 2049, 8192, 8193, 524288, 524289, 720000):
        assert lib.gcl_nghb_scratch_len(pc) == pc + pc // 2048 + 64, pc
        assert lib.gcl_nghb_scratch_len(pc) >= pc + (pc + 2047) // 2048       # the prefix sums + the scan's block totals
    assert lib.gcl_nghb_scratch_len(0) == 0 and lib.gcl_nghb_scratch_len(-3) == 0 and lib.gcl_nghb_scratch_len(2 ** 31) == 0


def _range_max(lib, offs=(0, 60, 100), **over):
    keep, op = _i64(offs)
    a = dict(xyz=P8, p=100, offs=op, n_clouds=2, aug=P8, aff=P8, max=P8, stream=None)
    a.update(over)
    return lib.gcl_nghb_range_max(*a.values())


def _flags(lib, offs=(0, 30, 30, 100), sides=(0, 0, 1), **over):
    k1, op = _i64(offs)
    k2, sp = _i32(sides)
    a = dict(cmpl=P8, pc=100, offs=op, sides=sp, n_scans=3, n_sides=2, scan_aff=P8, aug=P8, aff=P8, max=P8, moved=P8, flags=P8,
             stream=None)
    a.update(over)
    return lib.gcl_nghb_flags(*a.values())


def _compact(lib, offs=(0, 30, 100), **over):
    keep, op = _i64(offs)
    a = dict(moved=P8, flags=P8, pc=100, offs=op, n_sides=2, scratch=P8, out=P8, kept=P8, stream=None)
    a.update(over)
    return lib.gcl_nghb_compact(*a.values())


def test_refusals_come_before_any_launch_and_name_the_entry():
    lib = _lib.load()
    name = "gcl_nghb_range_max"
    for p in ("xyz", "offs", "aug", "aff", "max"):
        _refused(_range_max(lib, **{p: None}), name, "null")
    _refused(_range_max(lib, p=-1), name, "negative")
    _refused(_range_max(lib, n_clouds=-2), name, "negative")
    _refused(_range_max(lib, n_clouds=0), name, "clouds")
    _refused(_range_max(lib, offs=[0] * 65 + [100], n_clouds=65), name, "64")
    for offs in ((0, 101, 100), (1, 60, 100), (0, 60, 99), (0, 60, 101)):
        _refused(_range_max(lib, offs=offs), name, "ascending")
    name = "gcl_nghb_flags"
    for p in ("cmpl", "offs", "sides", "scan_aff", "aug", "aff", "max", "moved", "flags"):
        _refused(_flags(lib, **{p: None}), name, "null")
    _refused(_flags(lib, pc=-1), name, "negative")
    _refused(_flags(lib, n_scans=-1), name, "negative")
    _refused(_flags(lib, n_sides=-1), name, "negative")
    _refused(_flags(lib, n_sides=0), name, "sides")
    _refused(_flags(lib, n_sides=65), name, "64")
    _refused(_flags(lib, offs=[0] * 257 + [100], sides=[0] * 257, n_scans=257), name, "256")
    _refused(_flags(lib, n_scans=0), name, "without a scan")
    for offs in ((0, 31, 30, 100), (2, 30, 30, 100), (0, 30, 30, 99)):
        _refused(_flags(lib, offs=offs), name, "ascending")
    for sides in ((0, 0, 2), (0, -1, 1), (1, 0, 1)):
        _refused(_flags(lib, sides=sides), name, "side")
    name = "gcl_nghb_compact"
    for p in ("moved", "flags", "offs", "scratch", "out", "kept"):
        _refused(_compact(lib, **{p: None}), name, "null")
    _refused(_compact(lib, pc=-1), name, "negative")
    _refused(_compact(lib, n_sides=-1), name, "negative")
    _refused(_compact(lib, n_sides=0), name, "sides")
    _refused(_compact(lib, offs=[0] * 65 + [100], n_sides=65), name, "64")
    for offs in ((0, 130, 100), (3, 30, 100), (0, 30, 90)):
        _refused(_compact(lib, offs=offs), name, "ascending")
    # no points, no launch: the flags entry needs no pointer at all
    k1, op = _i64([0])
    assert lib.gcl_nghb_flags(None, 0, op, None, 0, 2, None, None, None, None, None, None, None) == 0
