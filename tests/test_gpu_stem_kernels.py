"""The first-layer ("stem") kernels behind gcl_stem_fwd / gcl_stem_bwd_weight, per launch shape: k_stem_fwd,
k_stem_fwd_occ, k_stem_bwd_weight<64> and k_stem_reduce (csrc/conv.hip), through the C ABI on synthetic neighbour tables
(tests/synthetic_tables.py; no voxel clouds, so any K from 1 to 125 and any n_in is one line of the table below).

CASES names every launch shape: Cout 32 .. 256 (blockIdx.y > 0: the `+ blockIdx.y * 32` offsets into W, y, dY and the
slabs), Cin 1 .. 4, K on the borders of the 25-offset batch of the forward walk, of the 32-bit presence words and of the
128-row A tile, row counts on the 64-row tile / 256-row workgroup / 32-row occupancy pass / 512-row slab range, slab counts on
both sides of the unrolled loop of k_stem_reduce (taken when b + 48 < n_slabs, 64 slabs a trip) and of its 16 parts, one
launch above the 512-row floor of stem_rows_per_wg, a strided map, and the three occupancy mixes.  A test that needs no GPU
pins the slab count of every case against gcl_stem_bwd_weight_scratch_len and the refusals of both entries.

Per case, two data sets:

  * small integers (|v| <= 2): y and dW must EQUAL the int64 result, element for element -- any dropped, duplicated or
    misplaced row, offset, channel, column block or slab shows, whatever its size;
  * Gaussian: relative L2 against fp64 below PREC_TOL["f32"] of tests/test_gpu_parity.py, and elementwise
    |got - ref| <= depth * 2^-24 * sum |terms|, depth = roundings on the longest chain to the element:
      forward          K * Cin: one fma per (offset, channel), k ascending, ci ascending (absent offsets add fma(0, w, acc));
                       the occupancy kernel adds the present offsets in the same order;
      weight gradient  rows_per_wg / 8 MFMA steps of a wave (a tile of 64 rows is 16 rows per wave, two rows per
                       v_mfma_f32_32x32x2_f32; rows_per_wg / 64 tiles), 3 cross-wave adds ((w0 + w1) + w2) + w3,
                       ceil(n_slabs / 64) adds of a thread of k_stem_reduce into each of its four accumulators, 2 adds
                       joining the four, 4 for the tree over the 16 parts.  (An MFMA step adds two products, and the tail
                       loop of the reduce up to three slabs to the first accumulator: counting a step as one rounding
                       and the loops as ceil(n_slabs / 64) keeps the bound on the tight side.)
    The worst measured ratio error / bound goes to conftest.precision_log_path(); measured: y <= 0.17, dW <= 0.04.

Every output (y, dW) and the slab scratch -- exactly gcl_stem_bwd_weight_scratch_len floats -- sits between guards and is filled
with NaN before the launch: no guard may change, no NaN may survive, rows without neighbours are exact zeros (the
elementwise bound is 0 there).  With Cin = 1 every case but the strided one runs a second time with presence words and its
occupancy mix, and must give the bits of the table launch.  Further bitwise relations on the Gaussian set: column slices
(Cout 128 / 256 against Cout = 32 launches), row invariance, determinism.
"""
import ctypes
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

import synthetic_tables as S
from test_gpu_conv_instances import Guarded
from test_gpu_parity import PREC_TOL

DEV = "cuda:0"
gpu = pytest.mark.gpu

Case = namedtuple("Case", "name cout cin K n_out stride occ slabs rows_per_wg")


def C(name, cout, cin, K, n_out, occ, slabs, stride=1, rows_per_wg=512):
    return Case(name, cout, cin, K, n_out, stride, occ, slabs, rows_per_wg)


# occ: the occupancy mix of the second run (Cin = 1), None = table path only.  slabs, rows_per_wg: what the case claims of
# stem_rows_per_wg (pinned without a GPU below)
CASES = [
    # ---- K borders x row counts x Cout x Cin
    C("k1-n1", 32, 1, 1, 1, "zeros", 1),
    C("k24-n31", 64, 1, 24, 31, "ones", 1),
    C("k25-n63-cin2", 32, 2, 25, 63, None, 1),
    C("k26-n64", 128, 1, 26, 64, "runs", 1),
    C("k27-n65-cin3", 32, 3, 27, 65, None, 1),
    C("k31-n255", 256, 1, 31, 255, "zeros", 1),
    C("k32-n256-cin4", 64, 4, 32, 256, None, 1),
    C("k33-n257", 32, 1, 33, 257, "runs", 1),
    C("k50-n511-cout96", 96, 1, 50, 511, "runs", 1),
    C("k51-n512-cin2", 32, 2, 51, 512, None, 1),
    C("k64-n513", 128, 1, 64, 513, "ones", 2),
    C("k65-n577", 64, 1, 65, 577, "runs", 2),
    C("k96-n577", 32, 1, 96, 577, "zeros", 2),
    C("k97-n257-cin2", 64, 2, 97, 257, None, 1),
    C("k124-n65-cin4", 128, 4, 124, 65, None, 1),
    C("k125-n513", 256, 1, 125, 513, "runs", 2),
    C("k125-n255-cin4", 32, 4, 125, 255, None, 1),
    C("k27-n577-cin3-cout256", 256, 3, 27, 577, None, 2),
    # ---- the K borders and row counts that the cases above have with Cin > 1 only, with Cin = 1 and presence words
    C("k25-n65", 64, 1, 25, 65, "runs", 1),
    C("k32-n63", 32, 1, 32, 63, "runs", 1),
    C("k51-n256", 128, 1, 51, 256, "zeros", 1),
    C("k97-n512", 32, 1, 97, 512, "runs", 1),
    C("k124-n257", 64, 1, 124, 257, "ones", 1),
    # ---- slab counts of k_stem_reduce (Cout = 32: one slab per 512 rows)
    C("slabs5", 32, 1, 27, 2500, "runs", 5),
    C("slabs16", 32, 1, 27, 8192, "zeros", 16),
    C("slabs17", 32, 1, 27, 8193, "runs", 17),
    C("slabs48", 32, 1, 27, 24576, "ones", 48),
    C("slabs49", 32, 1, 27, 25085, "runs", 49),
    C("slabs64", 32, 1, 27, 32768, "runs", 64),
    C("slabs65", 32, 1, 27, 33180, "zeros", 65),
    C("slabs81", 32, 1, 27, 41000, "runs", 81),
    C("slabs49-cin2-cout64", 64, 2, 27, 25085, None, 49),
    # ---- rows_per_wg above its floor: cdiv(70001, 64) = 1094 tiles > 8 * 1024 / (256 / 32)
    C("rows576", 256, 1, 27, 70001, "runs", 122, rows_per_wg=576),
    # ---- strided maps: n_in = 3 n_out, entries over the whole of x, table path only
    C("strided-cin3", 64, 3, 27, 300, None, 1, stride=3),
    C("strided-cin1", 32, 1, 27, 257, None, 1, stride=3),
]

K_BORDERS = {1, 24, 25, 26, 27, 31, 32, 33, 50, 51, 64, 65, 96, 97, 124, 125}
ROW_COUNTS = {1, 31, 63, 64, 65, 255, 256, 257, 511, 512, 513, 577}
SLAB_COUNTS = {1, 5, 16, 17, 48, 49, 64, 65, 81}


def dw_depth(case):
    return case.rows_per_wg // 8 + 3 + -(-case.slabs // 64) + 2 + 4


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_claims_its_slab_layout_and_covers_every_axis():
    """gcl_stem_bwd_weight_scratch_len is host arithmetic and is what the entry sizes its launch by: every case has the slab
    count and rows per workgroup it claims, and the table reaches every Cout, Cin, K border, row count, slab count, a
    rows_per_wg above the floor, a strided map and the three occupancy mixes, with and without presence words."""
    from gcl_amd import _lib
    lib = _lib.load()
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        mat = c.K * c.cin * c.cout
        n = lib.gcl_stem_bwd_weight_scratch_len(c.K, c.cin, c.cout, c.n_out)
        assert n % mat == 0 and n // mat == c.slabs, (c.name, n / mat)
        assert -(-c.n_out // c.rows_per_wg) == c.slabs and c.rows_per_wg % 64 == 0, c.name
        # the same rows_per_wg by the rule of stem_rows_per_wg: tiles dealt to at most 1024 / column blocks, floor 8 tiles
        tiles, wgs = -(-c.n_out // 64), 1024 // (c.cout // 32)
        assert max(8, -(-tiles // wgs)) * 64 == c.rows_per_wg, c.name
        assert c.occ is None or c.cin == 1, c.name
        assert c.occ is None or c.stride == 1, c.name          # occupancy assumes the same map
        assert (c.occ is not None) == (c.cin == 1 and c.stride == 1), c.name
    with_words = [c for c in CASES if c.occ]
    for cases in (CASES, with_words):          # every axis value, and again among the cases run with presence words
        assert {32, 64, 128, 256} <= {c.cout for c in cases}
        assert K_BORDERS <= {c.K for c in cases}
        assert ROW_COUNTS <= {c.n_out for c in cases}
        assert SLAB_COUNTS <= {c.slabs for c in cases}
        assert any(c.rows_per_wg > 512 for c in cases)
    assert {c.cin for c in CASES} == {1, 2, 3, 4}
    assert [c.cout for c in CASES].count(96) == 1
    assert {c.occ for c in with_words} == {"zeros", "ones", "runs"}
    # Cin > 1 (the ci loops of both kernels, x rows of 2 .. 4 floats) at K on both sides of a word border and at Cout > 32
    assert {c.cin for c in CASES if c.K > 96} >= {2, 4} and any(c.cin > 1 and c.cout == 256 for c in CASES)
    # both loops of k_stem_reduce: the unrolled one runs when 48 < n_slabs, the tail when n_slabs % 64 is in 1..48; a
    # count that is no multiple of 16 gives the 16 parts chains of different lengths
    slabs = {c.slabs for c in CASES}
    assert any(s > 48 for s in slabs) and any(s <= 48 for s in slabs) and any(s > 64 and 0 < s % 64 <= 48 for s in slabs)
    assert any(s % 16 for s in slabs) and {48, 49} <= slabs and {64, 65} <= slabs and {16, 17} <= slabs
    assert any(c.stride > 1 and c.cin == 1 for c in CASES) and any(c.stride > 1 and c.cin > 1 for c in CASES)
    assert max(c.n_out for c in CASES) * 2 * 2 < 2 ** 24          # the integer data set's premise, largest case


def test_stem_entries_refuse_bad_arguments_before_any_launch():
    """Cin = 5, Cout = 48, K = 126, n_out = 0 and presence without not_ones: nonzero from the argument checks (the message
    is the entry's own, so the launch was never reached); the buffers are host memory no kernel could read."""
    from gcl_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    ok = dict(n_out=8, K=27, cin=1, cout=32, presence=None, not_ones=None)
    bad = [dict(cin=5), dict(cout=48), dict(K=126), dict(n_out=0), dict(presence=p), dict(not_ones=p), dict(cin=0),
           dict(cout=0), dict(K=0)]
    for kw in bad:
        a = dict(ok, **kw)
        shape = (a["n_out"], a["K"], a["cin"], a["cout"])
        for name, call in (
                ("gcl_stem_fwd", lambda: lib.gcl_stem_fwd(p, p, p, *shape, p, a["presence"], a["not_ones"], None)),
                ("gcl_stem_bwd_weight", lambda: lib.gcl_stem_bwd_weight(p, p, p, *shape, p, p, a["presence"], a["not_ones"],
                                                                        None))):
            rc = call()
            msg = (lib.gcl_last_error() or b"").decode()
            assert rc != 0, (name, kw)
            assert msg.startswith(name) and ("supports Cin <= 4" in msg or "go together" in msg), (name, kw, msg)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Problem:
    """One case and data set: table, presence words, flags and operands on the host and on the device."""

    def __init__(self, case, kind, n_out=None, cout=None):
        self.case, self.kind, c = case, kind, case
        self.n_out = n_out = c.n_out if n_out is None else n_out
        self.cout = cout = c.cout if cout is None else cout
        self.n_in = n_in = c.stride * n_out
        seed = (c.K * 1000003 + c.n_out * 101 + c.cout * 7 + c.cin) % (2 ** 31)
        rng = np.random.RandomState(seed + (kind == "gauss"))
        self.flags = S.occupancy_flags(c.occ, n_out) if c.occ else None
        self.nbr, self.info = S.make_table(c.K, n_out, n_in, seed, self.flags)
        self.x = S.draw(rng, (n_in, c.cin), kind)
        if kind == "gauss" and c.occ:
            self.x = (1.0 + 0.5 * self.x).astype(np.float32)          # non-unit features around the occupancy value
        if c.occ:
            self.x[self.flags == 0] = 1.0          # unflagged rows are exactly 1.0; the flagged ones carry the data set
        self.W = S.draw(rng, (c.K, c.cin, cout), kind, 0.1)
        self.dY = S.draw(rng, (n_out, cout), kind)
        self.A = S.gathered(self.nbr, self.x)
        self.d = {k: dev(getattr(self, k)) for k in ("nbr", "x", "W", "dY")}
        if c.occ:
            self.d["presence"] = dev(S.presence_words(self.nbr).view(np.int32))
            self.d["flags"] = dev(self.flags)

    def fwd(self, words=False, W=None, nbr=None, n_out=None, presence=None, flags=None):
        """gcl_stem_fwd -> y as numpy; y sits between guard rows, starts as NaN, the guards are checked."""
        from gcl_amd import _lib
        lib, c = _lib.require_gpu(), self.case
        W = self.d["W"] if W is None else W
        n_out = self.n_out if n_out is None else n_out
        y = Guarded((n_out, W.shape[2]))
        pres = (self.d["presence"] if presence is None else presence) if words else None
        fl = (self.d["flags"] if flags is None else flags) if words else None
        with torch.cuda.device(DEV):
            _lib.check(lib.gcl_stem_fwd(_lib.ptr(self.d["x"]), _lib.ptr(W), _lib.ptr(self.d["nbr"] if nbr is None else nbr),
                                        n_out, c.K, c.cin, W.shape[2], _lib.ptr(y.t), _lib.ptr(pres), _lib.ptr(fl),
                                        _lib.stream()), "gcl_stem_fwd")
        torch.cuda.synchronize()
        assert y.intact(), f"{c.name}: gcl_stem_fwd wrote outside y"
        return y.t.cpu().numpy()

    def dw(self, words=False, dY=None):
        """gcl_stem_bwd_weight -> dW as numpy; the scratch is exactly gcl_stem_bwd_weight_scratch_len floats."""
        from gcl_amd import _lib
        lib, c = _lib.require_gpu(), self.case
        dY = self.d["dY"] if dY is None else dY
        cout = dY.shape[1]
        scratch = Guarded((lib.gcl_stem_bwd_weight_scratch_len(c.K, c.cin, cout, self.n_out),))
        dw = Guarded((c.K, c.cin, cout))
        with torch.cuda.device(DEV):
            _lib.check(lib.gcl_stem_bwd_weight(_lib.ptr(self.d["x"]), _lib.ptr(dY), _lib.ptr(self.d["nbr"]), self.n_out, c.K,
                                               c.cin, cout, _lib.ptr(scratch.t), _lib.ptr(dw.t),
                                               _lib.ptr(self.d["presence"]) if words else None,
                                               _lib.ptr(self.d["flags"]) if words else None, _lib.stream()),
                       "gcl_stem_bwd_weight")
        torch.cuda.synchronize()
        assert scratch.intact(), f"{c.name}: gcl_stem_bwd_weight wrote outside its scratch"
        assert dw.intact(), f"{c.name}: gcl_stem_bwd_weight wrote outside dW"
        assert bool(torch.isfinite(scratch.t).all()), f"{c.name}: slab elements left unwritten"
        return dw.t.cpu().numpy()


_T = {"t0": None, "cases": 0}


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_stem_case(case):
    """Forward and weight gradient of one case on both data sets; with Cin = 1 again with presence words, bit for bit."""
    from conftest import precision_log_path
    c = case
    if _T["t0"] is None:
        _T["t0"] = time.time()
    for kind in ("int", "gauss"):
        p = Problem(c, kind)
        y, dw = p.fwd(), p.dw()
        Wm, absA = p.W.astype(np.float64).reshape(c.K * c.cin, c.cout), np.abs(p.A)
        dY64 = p.dY.astype(np.float64)
        y_ref, y_mag = p.A @ Wm, absA @ np.abs(Wm)
        dw_ref = (p.A.T @ dY64).reshape(c.K, c.cin, c.cout)
        dw_mag = (absA.T @ np.abs(dY64)).reshape(c.K, c.cin, c.cout)
        empty = p.info["empty"]
        assert not y_mag[empty].any() and (len(empty) > 0) == (c.n_out >= 4)
        if kind == "int":
            S.assert_exact(y, y_ref, y_mag, f"{c.name} y")
            S.assert_exact(dw, dw_ref, dw_mag, f"{c.name} dW")
        else:
            tol = PREC_TOL["f32"]
            ry, qy = S.fp64_errors(y, y_ref, y_mag, c.K * c.cin, f"{c.name} y")
            rw, qw = S.fp64_errors(dw, dw_ref, dw_mag, dw_depth(c), f"{c.name} dW")
            line = (f"stem_kernels {c.name} cout={c.cout} cin={c.cin} K={c.K} n_out={c.n_out} slabs={c.slabs} "
                    f"y_rel_l2={ry:.4e} y_ratio={qy:.4f} dw_rel_l2={rw:.4e} dw_ratio={qw:.4f}")
            print("[stem] " + line)
            with open(precision_log_path(), "a") as fh:
                fh.write(line + "\n")
            assert ry < tol and rw < tol, (c.name, ry, rw)
            assert qy <= 1.0 and qw <= 1.0, (c.name, qy, qw)
        assert not y[empty].any(), f"{c.name}: a row without neighbours is not zero"
        k0 = p.info["k_absent"]
        assert k0 is None or not dw[k0].any(), f"{c.name}: dW of the all-absent offset is not zero"
        if c.occ:          # the same launch with presence words: the occupancy kernels on the unflagged rows
            yo, dwo = p.fwd(words=True), p.dw(words=True)
            assert np.array_equal(yo.view(np.int32), y.view(np.int32)), \
                f"{c.name} ({kind}, {c.occ}): y with presence words: {S.first_difference(yo, y)}"
            assert np.array_equal(dwo.view(np.int32), dw.view(np.int32)), \
                f"{c.name} ({kind}, {c.occ}): dW with presence words: {S.first_difference(dwo, dw)}"
    _T["cases"] += 1
    if c is CASES[-1]:
        print(f"[stem] {_T['cases']} cases in {time.time() - _T['t0']:.1f} s")


SLICE_CASES = [
    C("slices-cout128-cin3", 128, 3, 27, 1100, None, 3),
    C("slices-cout256-k125", 256, 1, 125, 577, "runs", 2),
    # the forward of the largest case; its dW has no Cout = 32 twin: at Cout = 32 no row count gives 576 rows per workgroup
    # with 122 slabs of these rows (stem_rows_per_wg(70001, 32) = 512), so that sub-check is dropped
    C("slices-rows576-forward-only", 256, 1, 27, 70001, "runs", 122, rows_per_wg=576),
]


@gpu
@pytest.mark.parametrize("case", SLICE_CASES, ids=lambda c: c.name)
def test_column_blocks_equal_the_cout32_launches_of_their_slices(case):
    """A column's sum is the same chain whatever block holds it: y and dW at Cout = 128 / 256 equal, column block by column
    block, the Cout = 32 launch on W[:, :, 32 j : 32 j + 32] / dY[:, 32 j : 32 j + 32] -- dW at the same slab layout (same
    rows per workgroup at both widths, asserted), with and without presence words."""
    from gcl_amd import _lib
    lib, c = _lib.require_gpu(), case
    p = Problem(c, "gauss")
    mat = c.K * c.cin
    same_slabs = lib.gcl_stem_bwd_weight_scratch_len(c.K, c.cin, 32, c.n_out) // (mat * 32) == c.slabs
    assert lib.gcl_stem_bwd_weight_scratch_len(c.K, c.cin, c.cout, c.n_out) // (mat * c.cout) == c.slabs
    assert same_slabs == (c.rows_per_wg == 512)
    for words in ((False, True) if c.occ else (False,)):
        y = p.fwd(words)
        dw = p.dw(words) if same_slabs else None
        for j in range(c.cout // 32):
            Wj = p.d["W"][:, :, 32 * j:32 * j + 32].contiguous()
            yj = p.fwd(words, W=Wj)
            assert np.array_equal(y[:, 32 * j:32 * j + 32].view(np.int32), yj.view(np.int32)), \
                f"{c.name}: y column block {j}: {S.first_difference(y[:, 32 * j:32 * j + 32], yj)}"
            if same_slabs:
                dwj = p.dw(words, dY=p.d["dY"][:, 32 * j:32 * j + 32].contiguous())
                assert np.array_equal(dw[:, :, 32 * j:32 * j + 32].view(np.int32), dwj.view(np.int32)), \
                    f"{c.name}: dW column block {j}: {S.first_difference(dw[:, :, 32 * j:32 * j + 32], dwj)}"


@gpu
@pytest.mark.parametrize("case", [C("rows-cin3", 64, 3, 27, 577, None, 2), C("rows-occ", 64, 1, 65, 577, "runs", 2)],
                         ids=lambda c: c.name)
def test_forward_of_the_first_rows_is_the_first_rows_of_the_forward(case):
    """A row's result does not depend on the launch around it: the first 300 rows of the table (sliced, contiguous) give the
    first 300 rows of the full launch."""
    p = Problem(case, "gauss")
    n = 300
    nbr = p.d["nbr"][:, :n].contiguous()
    for words in ((False, True) if case.occ else (False,)):
        full = p.fwd(words)
        kw = dict(presence=p.d["presence"][:n].contiguous(), flags=p.d["flags"][:n].contiguous()) if words else {}
        part = p.fwd(words, nbr=nbr, n_out=n, **kw)
        assert np.array_equal(part.view(np.int32), full[:n].view(np.int32)), S.first_difference(part, full[:n])


@gpu
def test_weight_gradient_is_deterministic():
    """Two launches into different scratch buffers: identical bits (slabs + ordered reduction, no atomics)."""
    for case in (C("det-49", 64, 2, 27, 25085, None, 49), C("det-occ", 32, 1, 125, 8193, "runs", 17)):
        p = Problem(case, "gauss")
        for words in ((False, True) if case.occ else (False,)):
            a, b = p.dw(words), p.dw(words)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (case.name, S.first_difference(a, b))
