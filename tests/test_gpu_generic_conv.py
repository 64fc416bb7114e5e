"""The generic forward / input-gradient kernel k_conv_generic<8> / <16> and the generic weight packers
(k_pack_weights_generic, the generic branch of k_pack_weights_multi; csrc/conv.hip), through gcl_pack_weights,
gcl_pack_weights_multi, gcl_conv_fwd and gcl_conv_fwd_fused on synthetic neighbour tables (tests/synthetic_tables.py).

CASES names the launch shapes: TC = 8 (Cout <= 8) and TC = 16, Cout a multiple of TC and not (a partial last column tile),
several column tiles, Cin % 4 == 0 (float4 row reads) and not (scalar reads), K = 1 without a table, K = 1 with one, 8, 27,
28, 125 (a 32 -> 32 layer that is generic because of K alone), row counts around the 256-row workgroup, n_in on both sides
of n_out, the three pack modes.  A test that needs no GPU pins path, TC and grid of every case against
gcl_conv_fwd_launch_shape -- the function the dispatcher itself calls.

Per case: the packed buffer bit for bit against the numpy index permutation
    mode 0  wp[k, c, n] = W[k, c, n]      mode 1  wp[k, c, n] = W[k, n, c]      mode 2  wp[k, c, n] = W[K-1-k, n, c]
(for modes 1 and 2 the convolution runs with Cin and Cout swapped: the input gradient), then the convolution on two data sets:

  * small integers (|v| <= 2, col_scale a power of two): y must EQUAL the int64 result, element for element;
  * Gaussian: relative L2 against fp64 below PREC_TOL["f32"] of tests/test_gpu_parity.py, and elementwise
    |got - ref| <= depth * 2^-24 * sum |terms|.  The kernel adds one fma per (offset, channel) to a column's accumulator,
    k ascending, c ascending: K * Cin roundings; the epilogue adds one for each of col_scale, bias and residual that is
    there (acc * scale + bias is two roundings, or one if contracted to an fma); ReLU and the gate round nothing.  The terms
    are |x| |w| |scale|, |bias| and |residual|; where the gate closes the bound is 0 and y an exact zero.
    The worst measured ratio error / bound goes to conftest.precision_log_path(); measured: <= 0.30 (K = 1, Cin = 3:
    a chain of four roundings), <= 0.07 elsewhere.

y and the packed weights sit between guards and start as NaN: no guard may change, no NaN survive; rows without neighbours are
epilogue(0), exactly.  The epilogue variants run on one TC = 8 and one TC = 16 shape with a partial last column tile, with
the exact relations tests/test_gpu_conv_epilogue.py states for the MFMA kernels; `order` and the entry's refusals likewise.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

import synthetic_tables as S
from test_gpu_conv_instances import GENERIC, Guarded, launch_shape
from test_gpu_parity import PREC_TOL

DEV = "cuda:0"
gpu = pytest.mark.gpu

Case = namedtuple("Case", "name cin cout K table n_out n_in mode tc")

# cin, cout: of the launch (for modes 1 and 2 the weight tensor is [K, cout, cin]); table False: tbl = NULL, idx = r
CASES = [
    Case("1x1-k1-notable", 1, 1, 1, False, 1, 1, 0, 8),
    Case("3x7-k1", 3, 7, 1, True, 63, 40, 1, 8),
    Case("30x7-k8", 30, 7, 8, True, 64, 100, 2, 8),
    Case("32x8-k27", 32, 8, 27, True, 65, 65, 0, 8),
    Case("32x9-k27", 32, 9, 27, True, 255, 300, 1, 16),
    Case("64x16-k28", 64, 16, 28, True, 256, 200, 2, 16),
    Case("17x33-k27", 17, 33, 27, True, 257, 257, 0, 16),
    Case("48x80-k8", 48, 80, 8, True, 1000, 700, 1, 16),
    Case("80x48-k27", 80, 48, 27, True, 1000, 1300, 2, 16),
    Case("5x40-k125", 5, 40, 125, True, 257, 500, 0, 16),
    Case("32x32-k125", 32, 32, 125, True, 1000, 1000, 2, 16),
    Case("64x16-k1-notable", 64, 16, 1, False, 1000, 1000, 1, 16),
]
# the shapes of the epilogue, `order` and refusal tests: TC = 8 and TC = 16, both with a partial last column tile
EPI_CASES = [
    Case("epi-30x7", 30, 7, 27, True, 257, 300, 0, 8),          # one tile of 7 columns, scalar reads
    Case("epi-48x40", 48, 40, 27, True, 257, 200, 2, 16),       # tiles of 16, 16 and 8 columns, float4 reads
]

# what the launch is given besides the table: bias (default yes), col_scale, residual ("own", or "y": the output itself),
# relu mode, amax slot.  "plain" and "bias" go through gcl_conv_fwd, the others through gcl_conv_fwd_fused
EPILOGUES = {
    "plain": dict(bias=False),
    "bias": dict(),
    "convbn": dict(scale=True, res="own", relu=1, amax=True),
    "gate": dict(res="own", relu=2, amax=True),
    "accumulate": dict(res="y", relu=0),
    "amax": dict(amax=True),
}


def is_fused(e):
    return bool(e.get("scale") or e.get("res") or e.get("relu") or e.get("amax"))


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_both_generic_instances_and_their_edges():
    """Every case is on the GENERIC path with the TC and grid it claims, with and without the fused epilogue; both TC values,
    partial and full last column tiles, several column tiles, both row-read forms, every K, row count and pack mode."""
    from gcl_amd import _lib
    lib = _lib.load()
    for c in CASES + EPI_CASES:
        for fused in (0, 1):
            s = launch_shape(lib, c.n_out, c.K, c.cin, c.cout, 4, 0, fused, int(c.table), 0, 0)
            assert (s["path"], s["nb"], s["pl"], s["pre"], s["epi"], s["block"], s["swz"]) == \
                (GENERIC, c.tc, 0, 0, fused, 256, 0), (c.name, s)
            assert (s["gx"], s["gy"]) == (-(-c.n_out // 256), -(-c.cout // c.tc)), (c.name, s)
        assert c.tc == (16 if c.cout > 8 else 8)
        assert c.cin % 32 or c.cout % 32 or c.K > 27
        assert c.table or (c.K == 1 and c.n_in >= c.n_out)
    assert len({c.name for c in CASES + EPI_CASES}) == len(CASES + EPI_CASES)
    assert {(c.cin, c.cout) for c in CASES} >= {(1, 1), (3, 7), (30, 7), (32, 8), (32, 9), (64, 16), (17, 33), (48, 80),
                                                (80, 48), (5, 40), (32, 32)}
    assert {(c.K, c.table) for c in CASES} == {(1, False), (1, True), (8, True), (27, True), (28, True), (125, True)}
    assert {c.n_out for c in CASES} == {1, 63, 64, 65, 255, 256, 257, 1000}
    assert any(c.n_in < c.n_out for c in CASES) and any(c.n_in > c.n_out for c in CASES)
    for tc in (8, 16):
        of_tc = [c for c in CASES if c.tc == tc]
        assert any(c.cout % tc for c in of_tc) and any(c.cout % tc == 0 for c in of_tc), tc          # partial / full tile
        assert any(c.cin % 4 for c in of_tc) and any(c.cin % 4 == 0 for c in of_tc), tc              # scalar / float4 reads
        assert {c.mode for c in of_tc} == {0, 1, 2}, tc
        assert any(c.tc == tc and c.cout % tc for c in EPI_CASES), tc
    assert any(c.cout > 2 * c.tc for c in CASES) and any(c.cout > 2 * c.tc and c.cout % c.tc for c in EPI_CASES)
    assert any((c.cin, c.cout, c.K) == (32, 32, 125) for c in CASES)          # generic because of K alone


# ---------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Problem:
    """One case and data set: table, operands, the epilogue's tensors, the weight tensor in the layout of the case's pack
    mode and the effective weights W_eff[k][c][n] the launch multiplies by."""

    def __init__(self, case, kind):
        self.case, self.kind, c = case, kind, case
        seed = (c.K * 1000003 + c.n_out * 101 + c.cout * 7 + c.cin) % (2 ** 31)
        rng = np.random.RandomState(seed + (kind == "gauss"))
        self.nbr, self.info = S.make_table(c.K, c.n_out, c.n_in, seed) if c.table else (None, dict(empty=np.zeros(0, int)))
        self.x = S.draw(rng, (c.n_in, c.cin), kind)
        self.W = S.draw(rng, (c.K, c.cin, c.cout) if c.mode == 0 else (c.K, c.cout, c.cin), kind, 0.1)
        self.W_eff = np.ascontiguousarray({0: self.W, 1: self.W.transpose(0, 2, 1), 2: self.W[::-1].transpose(0, 2, 1)}[c.mode])
        assert self.W_eff.shape == (c.K, c.cin, c.cout)
        self.bias = S.draw(rng, (c.cout,), kind, 0.3)
        self.res = S.draw(rng, (c.n_out, c.cout), kind)
        self.scale = (2.0 ** rng.randint(0, 3, c.cout) if kind == "int" else 0.5 + rng.rand(c.cout)).astype(np.float32)
        A = S.gathered(self.nbr, self.x[:c.n_out] if self.nbr is None else self.x)
        Wm = self.W_eff.astype(np.float64).reshape(c.K * c.cin, c.cout)
        self.conv64, self.conv_mag = A @ Wm, np.abs(A) @ np.abs(Wm)
        self.d = {k: dev(getattr(self, k)) for k in ("x", "W", "bias", "res", "scale")}
        self.d["nbr"] = dev(self.nbr) if c.table else None
        self._wp = None

    def expected(self, epi):
        """(fp64 result, sum |terms|, depth) of an epilogue variant."""
        e, c = EPILOGUES[epi], self.case
        sc = self.scale.astype(np.float64) if e.get("scale") else 1.0
        b = self.bias.astype(np.float64) if e.get("bias", True) else 0.0
        r = self.res.astype(np.float64)
        v, mag = self.conv64 * sc + b, self.conv_mag * np.abs(sc) + np.abs(b)
        depth = c.K * c.cin + bool(e.get("scale")) + bool(e.get("bias", True))
        if e.get("relu") == 2:
            return np.where(r > 0, v, 0.0), np.where(r > 0, mag, 0.0), depth
        if e.get("res"):
            v, mag, depth = v + r, mag + np.abs(r), depth + 1
        return (np.maximum(v, 0.0) if e.get("relu") == 1 else v), mag, depth

    def packed(self):
        """gcl_pack_weights of the case's mode into a guarded NaN-filled buffer, checked bit for bit against W_eff."""
        from gcl_amd import _lib
        if self._wp is None:
            lib, c = _lib.require_gpu(), self.case
            K, ca, cb = self.W.shape
            assert lib.gcl_pack_weights_bytes(K, ca, cb, 4) == 4 * self.W.size
            wp = Guarded((c.K, c.cin, c.cout))
            with torch.cuda.device(DEV):
                _lib.check(lib.gcl_pack_weights(_lib.ptr(self.d["W"]), K, ca, cb, c.mode, 4, None, _lib.ptr(wp.t),
                                                _lib.stream()), "gcl_pack_weights")
            torch.cuda.synchronize()
            assert wp.intact(), f"{c.name}: gcl_pack_weights wrote outside the packed tensor"
            got = wp.t.cpu().numpy()
            assert np.array_equal(bits(got), bits(self.W_eff)), \
                f"{c.name}: pack mode {c.mode}: {S.first_difference(bits(got), bits(self.W_eff))}"
            self._wp = wp
        return self._wp.t

    def run(self, epi, order=None, nbr=None):
        """One launch -> (y as numpy, max|y| bits or None).  y between guard rows, NaN before the launch (for "accumulate": the
        residual, which the launch reads from y itself)."""
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        lib, c = _lib.require_gpu(), self.case
        e = EPILOGUES[epi] if isinstance(epi, str) else epi
        y = Guarded((c.n_out, c.cout))
        if e.get("res") == "y":
            y.t.copy_(self.d["res"])
        tbl = self.d["nbr"] if nbr is None else nbr
        head = (_lib.ptr(self.d["x"]), c.n_in, 0, _lib.ptr(self.packed()), 4, None, None, _lib.ptr(tbl), _lib.ptr(order), None,
                c.n_out, c.K, c.cin, c.cout, _lib.ptr(self.d["bias"]) if e.get("bias", True) else None)
        slot = None
        with torch.cuda.device(DEV):
            if not is_fused(e):
                _lib.check(lib.gcl_conv_fwd(*head, _lib.ptr(y.t), None, 0, _lib.stream()), "gcl_conv_fwd")
            else:
                slot = ME.ops.amax_slot(self.d["x"].device) if e.get("amax") else None
                res = {"own": self.d["res"], "y": y.t, None: None}[e.get("res")]
                _lib.check(lib.gcl_conv_fwd_fused(*head, _lib.ptr(self.d["scale"]) if e.get("scale") else None, _lib.ptr(res),
                                                  e.get("relu", 0), _lib.ptr(slot), _lib.ptr(y.t), None, 0, _lib.stream()),
                           "gcl_conv_fwd_fused")
        torch.cuda.synchronize()
        assert y.intact(), f"{c.name} {epi}: the launch wrote outside y"
        amax = int(ME.ops.amax_value(slot).view(torch.int32).item()) if slot is not None else None
        return y.t.cpu().numpy(), amax


def check_launch(p, epi, y, amax, log):
    """The data set's assertion on one launch's y, the published amax, the rows without neighbours."""
    from conftest import precision_log_path
    c = p.case
    ref, mag, depth = p.expected(epi)
    what = f"{c.name} {epi} ({p.kind})"
    if p.kind == "int":
        S.assert_exact(y, ref, mag, what)
    else:
        rel, ratio = S.fp64_errors(y, ref, mag, depth, what)
        line = (f"generic_conv {c.name} {c.cin}->{c.cout} K={c.K} n_out={c.n_out} mode={c.mode} epi={epi} "
                f"rel_l2={rel:.4e} ratio={ratio:.4f}")
        print("[generic] " + line)
        if log:
            with open(precision_log_path(), "a") as fh:
                fh.write(line + "\n")
        assert rel < PREC_TOL["f32"], (what, rel)
        assert ratio <= 1.0, (what, ratio)
    if amax is not None:          # bit for bit max|y| of the written tensor
        want = int(np.abs(y).max().view(np.int32))
        assert amax == want, (what, amax, want)
    return ref


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_generic_case(case):
    """Pack (bit for bit) and convolution with a bias of one case, on both data sets."""
    for kind in ("int", "gauss"):
        p = Problem(case, kind)
        y, _ = p.run("bias")
        check_launch(p, "bias", y, None, log=True)
        empty = p.info["empty"]
        assert np.array_equal(bits(y[empty]), bits(np.broadcast_to(p.bias, (len(empty), case.cout)))), \
            f"{case.name}: a row without neighbours is not the bias"


@gpu
@pytest.mark.parametrize("case", EPI_CASES, ids=lambda c: c.name)
def test_generic_epilogues(case):
    """Every epilogue branch of k_conv_generic on both data sets, and the exact relations between the variants."""
    for kind in ("int", "gauss"):
        p = Problem(case, kind)
        ys = {}
        for epi in EPILOGUES:
            y, amax = p.run(epi)
            check_launch(p, epi, y, amax, log=True)
            assert (amax is not None) == bool(EPILOGUES[epi].get("amax"))
            ys[epi] = y
        empty = p.info["empty"]
        assert len(empty) and not ys["plain"][empty].any()          # epilogue(0) of the plain launch: exact zeros
        # the gate passes the bias launch's value exactly where residual > 0 and writes exact zeros elsewhere
        want = np.where(p.res > 0, ys["bias"], np.float32(0))
        assert np.array_equal(bits(ys["gate"]), bits(want)), S.first_difference(ys["gate"], want)
        assert (p.res <= 0).any() and (p.res > 0).any() and not bits(ys["gate"])[p.res <= 0].any()
        # relu 1 is max(v, 0) of the same launch with relu 0
        y0, _ = p.run(dict(EPILOGUES["convbn"], relu=0))
        assert np.array_equal(bits(ys["convbn"]), bits(np.maximum(y0, np.float32(0)))), \
            S.first_difference(ys["convbn"], np.maximum(y0, np.float32(0)))
        assert (y0 < 0).any()
        # the residual read from y itself: the bits of the same launch with the residual in a tensor of its own
        y1, _ = p.run(dict(res="own", relu=0))
        assert np.array_equal(bits(ys["accumulate"]), bits(y1)), S.first_difference(ys["accumulate"], y1)
        # y_amax alone changes nothing of y
        assert np.array_equal(bits(ys["amax"]), bits(ys["bias"]))


@gpu
@pytest.mark.parametrize("case", EPI_CASES, ids=lambda c: c.name)
def test_generic_order_indirection(case):
    """`order`: a random permutation of the output rows with the table given in that order (column r of the table is output
    row order[r]); residual and gate are read, y written, at the permuted row -- row for row the bits of the plain launch."""
    p = Problem(case, "gauss")
    perm = np.random.RandomState(case.n_out).permutation(case.n_out).astype(np.int32)
    assert (perm != np.arange(case.n_out)).any()
    order, nbr_p = dev(perm), dev(p.nbr[:, perm])
    for epi in ("bias", "convbn", "gate", "accumulate"):
        y, amax = p.run(epi)
        yp, amax_p = p.run(epi, order=order, nbr=nbr_p)
        assert np.array_equal(bits(yp), bits(y)), f"{case.name} {epi}: {S.first_difference(yp, y)}"
        assert amax_p == amax
        check_launch(p, epi, yp, amax_p, log=False)


@gpu
@pytest.mark.parametrize("case", EPI_CASES, ids=lambda c: c.name)
def test_generic_launch_refusals(case):
    """residual_ld != 0, stats != NULL, x_is_planes = 1 and K = 126 return nonzero for a generic shape and launch nothing: y
    keeps its NaN fill.  Every buffer is real and large enough for the launch that must not happen."""
    from gcl_amd import _lib
    lib, c = _lib.require_gpu(), case
    p = Problem(case, "int")
    K_big = 126
    tbl = dev(np.concatenate([p.nbr, np.full((K_big - c.K, c.n_out), -1, np.int32)]))
    wp = torch.zeros(K_big * c.cin * c.cout, device=DEV)
    wp[:p.packed().numel()] = p.packed().reshape(-1)
    stats = torch.zeros(4 * c.cout * c.n_out, device=DEV)
    y = Guarded((c.n_out, c.cout))

    def call(K=c.K, planes=0, stats=None, ld=0):
        with torch.cuda.device(DEV):
            return lib.gcl_conv_fwd_fused_ld(_lib.ptr(p.d["x"]), c.n_in, planes, _lib.ptr(wp), 4, None, None, _lib.ptr(tbl), None,
                                             None, c.n_out, K, c.cin, c.cout, _lib.ptr(p.d["bias"]), None, _lib.ptr(p.d["res"]),
                                             ld, 0, None, _lib.ptr(y.t), _lib.ptr(stats), 0, _lib.stream())
    for kw in (dict(ld=c.cout), dict(ld=c.cout + 8), dict(stats=stats), dict(planes=1), dict(K=K_big)):
        assert call(**kw) != 0, kw
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.t).all()) and y.intact(), kw
    assert not stats.any()
    assert call() == 0          # the same call without the refused argument runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.t).all()) and y.intact()


# (K, Cin, Cout, mode) of the weight tensors of one gcl_pack_weights_multi launch: generic tensors of different shapes and
# modes around one MFMA-shaped tensor; 3 + 120 + 216 + 500 + 1 workgroups, so the search has to land on all five
MULTI = [(27, 3, 7, 0), (8, 80, 48, 1), (27, 32, 64, 0), (125, 32, 32, 2), (1, 1, 1, 0)]


@gpu
@pytest.mark.parametrize("prec", [4, 2], ids=["fp16x3", "bf16x3"])
def test_pack_weights_multi_equals_the_single_tensor_packs(prec):
    """One descriptor list, every region bit for bit the gcl_pack_weights result of its tensor (generic: fp32 W_eff, checked
    against the numpy permutation as well), and no byte between or around the regions changed."""
    from gcl_amd import _lib
    from gcl_amd.MinkowskiEngine.ops import AMAX_WORDS
    lib = _lib.require_gpu()
    rng = np.random.RandomState(prec)
    FILL, GAP = 0xA5, 512
    Ws = [S.draw(rng, (K, ca, cb), "gauss", 0.1) for K, ca, cb, _ in MULTI]
    Wd = [dev(w) for w in Ws]
    slots = torch.zeros((len(MULTI), AMAX_WORDS), dtype=torch.int32, device=DEV)
    rows, regions, off, wg = [], [], 4096, 0
    for i, ((K, ca, cb, mode), w) in enumerate(zip(MULTI, Wd)):
        nbytes = lib.gcl_pack_weights_bytes(K, ca, cb, prec)
        generic = bool(ca % 32 or cb % 32 or K > 27)
        assert nbytes == 4 * w.numel()          # fp32 W_eff, or two 2-byte planes per element at prec 4 and 2
        rows.append([w.data_ptr(), K, ca, cb, mode, i, off, wg])
        regions.append((off, nbytes, generic))
        off += (nbytes + 255) // 256 * 256 + GAP
        wg += (K * ca * cb + 255) // 256
    assert [r[2] for r in regions] == [True, True, False, True, True]
    assert [r[7] for r in rows] == [0, 3, 123, 339, 839] and wg == 840
    out = torch.full((off + 4096,), FILL, dtype=torch.uint8, device=DEV)
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    with torch.cuda.device(DEV):
        for i, w in enumerate(Wd):
            _lib.check(lib.gcl_amax(_lib.ptr(w), w.numel(), _lib.ptr(slots[i]), 0, _lib.stream()), "gcl_amax")
        _lib.check(lib.gcl_pack_weights_multi(_lib.ptr(desc), len(MULTI), wg, prec, _lib.ptr(slots), _lib.ptr(out),
                                              _lib.stream()), "gcl_pack_weights_multi")
        torch.cuda.synchronize()
        untouched = torch.ones(out.numel(), dtype=torch.bool, device=DEV)
        for i, ((K, ca, cb, mode), w, (o, nbytes, generic)) in enumerate(zip(MULTI, Wd, regions)):
            single = torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)
            _lib.check(lib.gcl_pack_weights(_lib.ptr(w), K, ca, cb, mode, prec, _lib.ptr(slots[i]), _lib.ptr(single),
                                            _lib.stream()), "gcl_pack_weights")
            torch.cuda.synchronize()
            assert torch.equal(out[o:o + nbytes], single), f"tensor {i} {MULTI[i]}: region differs from gcl_pack_weights"
            untouched[o:o + nbytes] = False
            if generic:
                W_eff = {0: Ws[i], 1: Ws[i].transpose(0, 2, 1), 2: Ws[i][::-1].transpose(0, 2, 1)}[mode]
                got = out[o:o + nbytes].cpu().numpy().view(np.int32)
                assert np.array_equal(got, bits(W_eff).reshape(-1)), f"tensor {i} {MULTI[i]}: not the permutation of mode {mode}"
        assert bool((out[untouched] == FILL).all()), "gcl_pack_weights_multi wrote outside the packed regions"
