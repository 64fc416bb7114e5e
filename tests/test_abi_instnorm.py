"""The InstanceNorm entries (gcl_in_scratch_len, gcl_in_fwd, gcl_in_bwd) without a GPU: exported with the header's argument
counts, the scratch length is the header's formula, and every refusal comes before any HIP call and names the entry."""
import ctypes
import os
import re

from gcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gcl_in_scratch_len", "gcl_in_fwd", "gcl_in_bwd")
P8 = 8          # a non-null pointer value that is never dereferenced: the checks come before any HIP call


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
    assert "instnorm.hip" in _lib.SOURCES and "instnorm.hip" not in _lib.TRAINING_STEP_SOURCES


def test_scratch_len_is_the_documented_formula():
    lib = _lib.load()
    for n, ns, c in ((1, 1, 4), (64, 1, 32), (65, 3, 32), (50834, 6, 32), (131078, 2, 32), (1515, 5, 256),
                     (530000, 28, 64), (7, 65535, 128)):
        want = ((n + 63) // 64 + ns) * 2 * c + (ns + 1) + (ns + 1) // 2
        assert lib.gcl_in_scratch_len(n, ns, c) == want, (n, ns, c)
    assert lib.gcl_in_scratch_len(0, 3, 32) == 0 and lib.gcl_in_scratch_len(-5, 3, 32) == 0
    assert lib.gcl_in_scratch_len(100, 0, 32) == 0 and lib.gcl_in_scratch_len(100, 3, 0) == 0


def _fwd(lib, **over):
    a = dict(x=P8, n=100, c=32, seg_off=P8, rows=P8, row_cloud=P8, n_clouds=3, eps=1e-8, weight=P8, bias=P8, residual=None,
             relu=0, scratch=P8, mean=P8, rstd=P8, y=P8, relu_mask=None, y_amax=None, stream=None)
    a.update(over)
    return lib.gcl_in_fwd(*a.values())


def _bwd(lib, **over):
    a = dict(x=P8, dy=P8, n=100, c=32, seg_off=P8, rows=P8, row_cloud=P8, n_clouds=3, mean=P8, rstd=P8, weight=P8, relu=0,
             relu_mask=None, scratch=P8, sum_g=P8, sum_gx=P8, dx=P8, dres=None, dx_amax=None, stream=None)
    a.update(over)
    return lib.gcl_in_bwd(*a.values())


def test_refusals_come_before_any_launch_and_name_the_entry():
    lib = _lib.load()
    for name, call, ptrs in (("gcl_in_fwd", _fwd, ("x", "seg_off", "row_cloud", "weight", "bias", "scratch", "mean", "rstd", "y")),
                             ("gcl_in_bwd", _bwd, ("x", "dy", "seg_off", "row_cloud", "mean", "rstd", "weight", "scratch",
                                                   "sum_g", "sum_gx", "dx"))):
        for p in ptrs:
            _refused(call(lib, **{p: None}), name, "null")
        for n in (0, -7):
            _refused(call(lib, n=n), name, "shape")
        for ns in (0, -1):
            _refused(call(lib, n_clouds=ns), name, "n_clouds")
        for c in (0, 2, 6, 24, 40, 2048):          # what gcl_bn_stats refuses: not a multiple of 4, or c / 4 does not divide 256
            _refused(call(lib, c=c), name, "shape")
            assert lib.gcl_bn_stats(P8, 100, c, 1e-8, 0.0, None, None, P8, P8, P8, None) == -1
        _refused(call(lib, relu=1), name, "relu_mask")
