"""The fused epilogue of the forward / input-gradient kernels against the PLAIN path of the same kernels.

The epilogue (csrc/conv.hip: conv_fwd_epilogue, k_conv_fwd_tall, k_conv_groups_sum) fetches its residual / gate operand for
all of a wave's elements before its first store.  What it computes is pinned here by the launch that has no epilogue at all
(gcl_conv_fwd, the EPI = false instances), never by another fused launch:

    add      relu = 0, residual [n, cout]                    y == torch.add(y_plain, residual)                 bit for bit
    sliced   relu = 0, residual a column slice, ld = cout+32 y == torch.add(y_plain, slice)                    bit for bit
    gate     relu = 2                                        y == torch.where(residual > 0, y_plain, 0), y_amax == max|y|
    eval     col_scale, bias, relu = 1                       relu(conv * scale + bias) in fp64 at PREC_TOL
    all      tile partials: min / max equal those of the written y, sums within the fp32 summation bound; 128 guard rows
             before and after y untouched

Sizes: for NB = 1, 2, 4 the smallest row count at which gcl_conv_fwd_nb selects that width, plus 3 (the last workgroup is
one wave of four rows and three inactive waves), and n = 29 / n = 131 at NB = 1 (less than one wave; one full workgroup and
three rows).  A test without a GPU pins those band edges.  K = 27 stride-1 map over random voxels that fill 40 % of a small
box, so rows have missing neighbours and tiles have missing offsets.  fp16x3, fp32 rows and plane images, LDS-DMA and
register staging: k_conv_fwd_dma<NB, PRE, *> and k_conv_fwd_split<NB, 4, PRE, *>.  The inference kernels
(k_conv_groups_sum, k_conv_fwd_tall) get the same relations on one Cin = 128 layer.
"""
import ctypes

import numpy as np
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu

PREC = 4                        # fp16x3
PREC_TOL = 2e-6                 # tests/test_gpu_parity.py PREC_TOL["fp16x3"]: per-operator relative L2 against fp64
DMA, TALL, NO_DMA = 2, 4, 8     # include/gcl_amd.h GCL_CONV_DMA / GCL_CONV_TALL / GCL_CONV_NO_DMA
CIN, COUT = 32, 256
# (NB, last row count of the band below it); n = edge + 1 + 3
BANDS = [(1, 0), (2, 8064), (4, 16256)]
SIZES = [(nb, edge + 4) for nb, edge in BANDS] + [(1, 29), (1, 131)]
SENTINEL = 0x7FC5A5A5           # a quiet NaN
GUARD_ROWS = 128


def test_sizes_sit_at_the_band_edges_of_conv_fwd_nb():
    """Host arithmetic: n - 3 is the smallest row count of its NB band (Cout = 256, fp16x3), and every size is ragged."""
    from gcl_amd import _lib
    lib = _lib.load()
    for nb, edge in BANDS:
        assert lib.gcl_conv_fwd_nb(edge + 1, COUT, PREC) == nb and lib.gcl_conv_fwd_nb(edge + 4, COUT, PREC) == nb
        assert edge == 0 or lib.gcl_conv_fwd_nb(edge, COUT, PREC) < nb
        assert edge % 128 == 0          # the last workgroup of n = edge + 4: four rows in its first wave
    assert lib.gcl_conv_fwd_nb(29, COUT, PREC) == 1 and lib.gcl_conv_fwd_nb(131, COUT, PREC) == 1
    assert sorted({nb for nb, _ in SIZES}) == [1, 2, 4]


INFER_LAYER = (2051, 128, 128)          # rows, Cin, Cout of the inference-sized layer


def test_inference_layer_reaches_the_group_launches_and_the_sixteen_wave_kernel():
    """Host arithmetic (gcl_conv_fwd_launch_shape, the function the dispatcher calls): with GCL_CONV_TALL the inference layer
    runs the offset-group launches + k_conv_groups_sum when it is handed scratch and k_conv_fwd_tall when it is not, with
    and without the fused epilogue."""
    from gcl_amd import _lib
    lib = _lib.load()
    n, cin, cout = INFER_LAYER
    out = (ctypes.c_int32 * 8)()
    assert lib.gcl_conv_fwd_groups_scratch_len(n, 27, cin, cout) == 4 * n * cout
    for fused in (0, 1):
        for has_scratch, path, block in ((1, 5, 256), (0, 4, 1024)):       # include/gcl_amd.h GCL_FWD_PATH_GROUPS, _TALL
            assert lib.gcl_conv_fwd_launch_shape(n, 27, cin, cout, PREC, 0, fused, 1, has_scratch, TALL, out) == 0
            assert (out[0], out[3], out[6]) == (path, 2 * fused, block), (fused, has_scratch, list(out))


def make_cloud(n, seed):
    """n distinct voxels, 40 % of a box: int32 [n, 4], batch index 0."""
    rng = np.random.RandomState(seed)
    s = max(3, int(np.ceil((2.5 * n) ** (1.0 / 3.0))))
    cells = rng.permutation(s ** 3)[:n]
    c = np.stack(np.unravel_index(cells, (s, s, s)), axis=1) - s // 2
    return np.concatenate([np.zeros((n, 1), c.dtype), c], axis=1).astype(np.int32)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def where_differs(a, b):
    bad = torch.nonzero(~((a == b) | (a.isnan() & b.isnan())))
    if len(bad) == 0:
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at {i}: {float(a[i])!r} != {float(b[i])!r}"


class Layer:
    """One (cloud, cin, cout): the sorted table, operands in both forms, the epilogue's tensors, the fp64 product."""

    def __init__(self, n, cin, cout):
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        self.lib = lib = _lib.require_gpu()
        self.n, self.cin, self.cout = n, cin, cout
        mgr = ME.CoordinateManager(torch.from_numpy(make_cloud(n, 1000 + n)).to(DEV))
        km = mgr.get_kernel_map(1, 3, 1)
        self.nbr, self.table = km.nbr, km.sorted_table()
        assert tuple(self.nbr.shape) == (27, n)
        assert n < 27 or bool((self.nbr < 0).any()), "the cloud has no missing neighbour"
        g = torch.Generator().manual_seed(n + 7 * cin + 13 * cout)
        self.x = torch.randn(n, cin, generator=g).to(DEV)
        self.W = (0.1 * torch.randn(27, cin, cout, generator=g)).to(DEV)
        self.bias = (0.3 * torch.randn(cout, generator=g)).to(DEV)
        self.scale = (0.5 + torch.rand(cout, generator=g)).to(DEV)
        self.res = torch.randn(n, cout, generator=g).to(DEV)
        self.res_wide = torch.randn(n, cout + 32, generator=g).to(DEV)          # the slice: columns 32 .. 32 + cout
        with torch.cuda.device(DEV):
            self.xa, self.wa = ME.ops.amax_slot(self.x.device), ME.ops.amax_slot(self.x.device)
            _lib.check(lib.gcl_amax(_lib.ptr(self.x), self.x.numel(), _lib.ptr(self.xa), 1, _lib.stream()), "gcl_amax")
            _lib.check(lib.gcl_amax(_lib.ptr(self.W), self.W.numel(), _lib.ptr(self.wa), 1, _lib.stream()), "gcl_amax")
            self.planes = torch.empty((n, cin), dtype=torch.int32, device=DEV)
            _lib.check(lib.gcl_split_planes(_lib.ptr(self.x), n, cin, _lib.ptr(self.xa), _lib.ptr(self.planes),
                                            _lib.stream()), "gcl_split_planes")
            self.wp = torch.empty(lib.gcl_pack_weights_bytes(27, cin, cout, PREC), dtype=torch.uint8, device=DEV)
            _lib.check(lib.gcl_pack_weights(_lib.ptr(self.W), 27, cin, cout, 0, PREC, _lib.ptr(self.wa), _lib.ptr(self.wp),
                                            _lib.stream()), "gcl_pack_weights")
        xd, Wd = self.x.double(), self.W.double()
        self.conv64 = torch.zeros(n, cout, dtype=torch.float64, device=DEV)
        for k in range(27):
            rows = torch.nonzero(self.nbr[k] >= 0).squeeze(1)
            if len(rows):
                self.conv64[rows] += xd[self.nbr[k][rows].long()] @ Wd[k]
        self._plain = {}

    def launch(self, form, flags, scale=False, bias=False, res=None, relu=0, amax=False, partials=True, scratch=None):
        """One launch.  res: None, "own" or "wide".  No epilogue operand at all: gcl_conv_fwd (the EPI = false instance).
        Returns (y, tile partials or None, max|y| slot value or None); y sits between sentinel rows that are checked here."""
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        lib, n, cout = self.lib, self.n, self.cout
        buf = torch.full(((n + 2 * GUARD_ROWS) * cout,), SENTINEL, dtype=torch.int32, device=DEV)
        y = buf[GUARD_ROWS * cout:(GUARD_ROWS + n) * cout].view(torch.float32).view(n, cout)
        stats = None
        if scratch is not None:
            stats = scratch
        elif partials:
            stats = torch.full((4, cout, (n + 127) // 128), float("nan"), device=DEV)
        tbl, order, mask = self.table
        xin = self.planes if form == "planes" else self.x
        head = (_lib.ptr(xin), n, int(form == "planes"), _lib.ptr(self.wp), PREC, _lib.ptr(self.xa), _lib.ptr(self.wa),
                _lib.ptr(tbl), _lib.ptr(order), _lib.ptr(mask), n, 27, self.cin, cout, _lib.ptr(self.bias) if bias else None)
        tail = (_lib.ptr(y), _lib.ptr(stats), flags, _lib.stream())
        slot = None
        with torch.cuda.device(DEV):
            if not (scale or res or relu or amax):
                _lib.check(lib.gcl_conv_fwd(*head, *tail), "gcl_conv_fwd")
            else:
                slot = ME.ops.amax_slot(self.x.device) if amax else None
                sc = _lib.ptr(self.scale) if scale else None
                if res == "wide":
                    rp = ctypes.c_void_p(self.res_wide.data_ptr() + 4 * 32)
                    _lib.check(lib.gcl_conv_fwd_fused_ld(*head, sc, rp, cout + 32, relu, _lib.ptr(slot), *tail),
                               "gcl_conv_fwd_fused_ld")
                else:
                    _lib.check(lib.gcl_conv_fwd_fused(*head, sc, _lib.ptr(self.res) if res else None, relu, _lib.ptr(slot),
                                                      *tail), "gcl_conv_fwd_fused")
        torch.cuda.synchronize()
        lead = GUARD_ROWS * cout
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[-lead:] == SENTINEL).all()), "the launch wrote outside y"
        assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} elements of y left unwritten"
        return y, (stats if scratch is None else None), (ME.ops.amax_value(slot) if slot is not None else None)

    def plain(self, form, flags, scratch=None):
        """y of the launch without an epilogue; computed once per (form, flags) and left unchanged."""
        key = (form, flags, scratch is not None)
        if key not in self._plain:
            self._plain[key] = self.launch(form, flags, partials=False, scratch=scratch)[0].clone()
        return self._plain[key]

    def check_partials(self, y, stats, what):
        """Tile t holds the rows order[128 t .. 128 t + 127]: minimum and maximum exactly, the sums within 128 fp32
        additions (+ one rounding of each square)."""
        n, cout = self.n, self.cout
        n_tiles, order = (n + 127) // 128, self.table[1].long()
        assert bool(torch.isfinite(stats).all()), f"{what}: partials left unwritten"
        ys = y[order]
        pad = n_tiles * 128 - n

        def tiles(t, fill):
            return torch.cat([t, torch.full((pad, cout), fill, dtype=t.dtype, device=DEV)]).view(n_tiles, 128, cout)
        lo, hi = tiles(ys, float("inf")).amin(1).T, tiles(ys, float("-inf")).amax(1).T
        assert torch.equal(stats[2], lo), f"{what}: tile minimum (column, tile): {where_differs(stats[2], lo)}"
        assert torch.equal(stats[3], hi), f"{what}: tile maximum (column, tile): {where_differs(stats[3], hi)}"
        yd = tiles(ys.double(), 0.0)
        s1, a1, s2 = yd.sum(1).T, yd.abs().sum(1).T, (yd * yd).sum(1).T
        u = 2.0 ** -24
        d1, d2 = (stats[0].double() - s1).abs(), (stats[1].double() - s2).abs()
        assert bool((d1 <= 128 * u * a1).all()), (what, "sum", float((d1 / a1.clamp_min(1e-300)).max()) / u)
        assert bool((d2 <= 130 * u * s2).all()), (what, "squares", float((d2 / s2.clamp_min(1e-300)).max()) / u)


_LAYERS = {}


def layer(n, cin, cout):
    if (n, cin, cout) not in _LAYERS:
        _LAYERS[(n, cin, cout)] = Layer(n, cin, cout)
    return _LAYERS[(n, cin, cout)]


def check_relations(p, form, flags, name, partials=True, scratch=None):
    """add, sliced, gate and eval of one kernel against its own launch without an epilogue."""
    y_plain = p.plain(form, flags, scratch)
    kw = dict(partials=partials, scratch=scratch)
    # add
    y, st, _ = p.launch(form, flags, res="own", **kw)
    want = torch.add(y_plain, p.res)
    assert torch.equal(y, want), f"{name} add: {where_differs(y, want)}"
    if st is not None:
        p.check_partials(y, st, f"{name} add")
    # sliced residual, pitch cout + 32
    y, st, _ = p.launch(form, flags, res="wide", **kw)
    want = torch.add(y_plain, p.res_wide[:, 32:32 + p.cout])
    assert torch.equal(y, want), f"{name} sliced: {where_differs(y, want)}"
    if st is not None:
        p.check_partials(y, st, f"{name} sliced")
    # gate
    y, st, amax = p.launch(form, flags, res="own", relu=2, amax=True, **kw)
    want = torch.where(p.res > 0, y_plain, torch.zeros_like(y_plain))
    assert torch.equal(y, want), f"{name} gate: {where_differs(y, want)}"
    assert float(amax) == float(y.abs().max()), (name, "gate", float(amax), float(y.abs().max()))
    if st is not None:
        p.check_partials(y, st, f"{name} gate")
    # eval: BatchNorm scale / shift and ReLU, against fp64
    y, st, amax = p.launch(form, flags, scale=True, bias=True, relu=1, amax=True, **kw)
    want64 = (p.conv64 * p.scale.double() + p.bias.double()).clamp_min(0.0)
    err = rel_l2(y, want64)
    print(f"[conv epilogue] {name} n={p.n} eval: rel-L2 vs fp64 {err:.3e}")
    assert err < PREC_TOL, (name, "eval", err)
    assert float(amax) == float(y.abs().max()), (name, "eval", float(amax), float(y.abs().max()))
    if st is not None:
        p.check_partials(y, st, f"{name} eval")


@gpu
@pytest.mark.parametrize("staging", ["dma", "split"])
@pytest.mark.parametrize("form", ["rows", "planes"])
@pytest.mark.parametrize("nb,n", SIZES, ids=[f"nb{nb}-n{n}" for nb, n in SIZES])
def test_fused_epilogue_equals_the_plain_launch(nb, n, form, staging):
    p = layer(n, CIN, COUT)
    assert p.lib.gcl_conv_fwd_nb(n, COUT, PREC) == nb
    pre = "true" if form == "planes" else "false"
    name = f"k_conv_fwd_dma<{nb},{pre},true>" if staging == "dma" else f"k_conv_fwd_split<{nb},4,{pre},true>"
    check_relations(p, form, DMA if staging == "dma" else NO_DMA, name)


@gpu
@pytest.mark.parametrize("kernel", ["groups", "tall"])
def test_inference_kernels_fused_epilogue_equals_their_plain_launch(kernel):
    """One inference-sized layer (Cin = 128: 108 steps per tile, GCL_CONV_TALL): the offset-group launches +
    k_conv_groups_sum when the launch is handed scratch, the sixteen-wave k_conv_fwd_tall when it is not."""
    n, cin, cout = INFER_LAYER
    p = layer(n, cin, cout)
    gs_len = p.lib.gcl_conv_fwd_groups_scratch_len(n, 27, cin, cout)
    assert n <= 65536 and gs_len > 0
    scratch = torch.empty(gs_len, dtype=torch.float32, device=DEV) if kernel == "groups" else None
    name = "k_conv_groups_sum<true,4>" if kernel == "groups" else "k_conv_fwd_tall<true>"
    check_relations(p, "rows", TALL, name, partials=False, scratch=scratch)
    # the two kernels compute the same bits (tests/test_gpu_parity.py holds the full claim); here: of the plain launches
    if kernel == "tall":
        other = torch.empty(gs_len, dtype=torch.float32, device=DEV)
        assert torch.equal(p.plain("rows", TALL), p.plain("rows", TALL, other))
