"""Every kernel instance behind gcl_conv_fwd / gcl_conv_fwd_fused / gcl_conv_fwd_fused_ld, named and tested one by one.

For MFMA shapes the forward entry (which also computes every input gradient) is 37 template instances, picked by the
host dispatcher from (n_out, cout, prec, operand form, epilogue, flags):

    k_conv_fwd_dma<NB, PRE, EPI>          fp16x3, default               NB 1, 2, 4 x PRE x EPI   12
    k_conv_fwd_split<NB, 4, PRE, EPI>     fp16x3, GCL_CONV_NO_DMA       NB 1, 2, 4 x PRE x EPI   12
    k_conv_fwd_split<NB, 2, false, EPI>   bf16x3                        NB 1, 2, 4 x EPI          6
    k_conv_fwd_split<NB, 3, false, EPI>   bf16x6                        NB 1, 2    x EPI          4
    k_conv_fwd<NB>                        exact f32                     NB 1, 2, 4                3

NB (32-column blocks per wave) follows from (n_out, cout, prec) in conv_fwd_nb (csrc/conv.hip); small launches take
narrower blocks, so a test has to pick its row count to reach a wide instance.  CASES below names the instance of every
case; a test that needs no GPU pins those names against gcl_conv_fwd_launch_shape -- the function the dispatcher itself
calls -- and requires the table to reach all 37, so a change of the dispatcher cannot silently move these tests onto other
kernels.  Further tests without a GPU pin the paths outside the matrix (generic shapes, the inference kernels of
GCL_CONV_TALL) and the profile labels of MinkowskiEngine/ops.py.

Per case, on the GPU: y against the fp64 product at the per-operator bound; y, the BatchNorm tile partials and max|y| bit
for bit against NB = 1 launches of every 32-column slice (the claim "a column's sum is the same chain of products whatever
block holds it"); the tile partials against the written y; guard rows around y and the partials; the fused epilogue's exact
relations; GCL_CONV_XCD_RANGES and the LDS-DMA / register-staged pair bit for bit.  The only numeric bounds are PREC_TOL,
the 1e-6 of the BatchNorm statistics and the derived fp32 summation bound of the tile partials.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import me_oracle as O

DEV = "cuda:0"
gpu = pytest.mark.gpu

PREC_CODE = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 4}
# per-operator tolerance (relative L2 against fp64) of each MFMA arithmetic: tests/test_gpu_parity.py PREC_TOL
PREC_TOL = {"f32": 2e-6, "bf16x6": 2e-6, "bf16x3": 3e-5, "fp16x3": 2e-6}
XCD, DMA, TALL, NO_DMA = 1, 2, 4, 8          # include/gcl_amd.h GCL_CONV_XCD_RANGES / _DMA / _TALL / _NO_DMA
# include/gcl_amd.h GCL_FWD_PATH_*
GENERIC, F32, SPLIT, DMA_PATH, TALL_PATH, GROUPS = range(6)

# Row counts.  n % 128 in 1..31: the last workgroup has one partly filled wave and three idle ones; the "b" counts have
# n % 128 in 33..127 (full waves, a partly filled one and idle ones).  Tiles of 128 rows: 6 (< 8, fewer tiles than XCDs),
# 23, 97, 161, 321 (none a multiple of 8: the per-XCD range split has a remainder).
N6, N23, N97, N161, N321 = 643, 2835, 12305, 20493, 40967
N97B, N161B, N321B = 12369, 20543, 41053

# epilogue variants: what the launch is given besides `bias` (every launch has a bias: it is not part of the EPI template axis)
EPILOGUES = {
    "plain": dict(),                                                       # gcl_conv_fwd: the EPI = false instances
    "convbn": dict(scale=True, res="own", relu=1, amax=True),            # eval-mode ConvBN + residual + ReLU
    "gate": dict(res="own", relu=2, amax=True),                          # threshold_backward: residual is the gate
    "ld": dict(scale=True, res="wide", relu=0, amax=True),               # residual a column slice, residual_ld > cout
    "add": dict(res="own", relu=0),                                      # the backward accumulate
}

# (prec, cin, cout, conv, n_out, operand form, epilogue, flags, NB)
#   conv: "s1" K = 27 same map; "tr2" K = 27 transposed from the stride-2 map (n_in = coarse rows); "k1" K = 1, no table
CASES = [
    # ---- k_conv_fwd_dma<NB, PRE, EPI>
    ("fp16x3", 64, 64, "s1", N23, "rows", "plain", DMA, 1),
    ("fp16x3", 32, 128, "s1", N97, "rows", "convbn", DMA, 1),
    ("fp16x3", 128, 128, "s1", N23, "planes", "plain", DMA, 1),
    ("fp16x3", 128, 64, "tr2", N97, "planes", "gate", DMA, 1),
    ("fp16x3", 64, 256, "s1", N97, "rows", "plain", DMA, 2),
    ("fp16x3", 64, 64, "s1", N321, "rows", "add", DMA, 2),
    ("fp16x3", 128, 128, "s1", N161, "planes", "plain", DMA, 2),
    ("fp16x3", 256, 256, "s1", N97, "planes", "convbn", DMA, 2),
    ("fp16x3", 64, 128, "s1", N321, "rows", "plain", DMA, 4),
    ("fp16x3", 32, 256, "k1", N161, "rows", "ld", DMA, 4),
    ("fp16x3", 128, 256, "s1", N161, "planes", "plain", DMA, 4),
    ("fp16x3", 256, 128, "tr2", N321, "planes", "gate", DMA, 4),
    ("fp16x3", 128, 256, "s1", N97B, "planes", "convbn", DMA, 2),
    ("fp16x3", 64, 64, "s1", N6, "rows", "convbn", DMA, 1),
    # ---- k_conv_fwd_split<NB, 4, PRE, EPI>
    ("fp16x3", 32, 64, "s1", N23, "rows", "plain", NO_DMA, 1),
    ("fp16x3", 64, 128, "tr2", N97, "rows", "ld", NO_DMA, 1),
    ("fp16x3", 128, 64, "s1", N97, "planes", "plain", NO_DMA, 1),
    ("fp16x3", 128, 128, "s1", N23, "planes", "convbn", NO_DMA, 1),
    ("fp16x3", 64, 64, "s1", N321, "rows", "plain", NO_DMA, 2),
    ("fp16x3", 64, 256, "s1", N97, "rows", "gate", NO_DMA, 2),
    ("fp16x3", 256, 256, "s1", N97, "planes", "plain", NO_DMA, 2),
    ("fp16x3", 128, 128, "s1", N161, "planes", "add", NO_DMA, 2),
    ("fp16x3", 32, 256, "s1", N161, "rows", "plain", NO_DMA, 4),
    ("fp16x3", 64, 128, "s1", N321, "rows", "convbn", NO_DMA, 4),
    ("fp16x3", 128, 128, "k1", N321, "planes", "plain", NO_DMA, 4),
    ("fp16x3", 128, 256, "s1", N161, "planes", "ld", NO_DMA, 4),
    ("fp16x3", 64, 256, "s1", N161B, "rows", "convbn", NO_DMA, 4),
    ("fp16x3", 128, 128, "s1", N6, "planes", "add", NO_DMA, 1),
    # ---- k_conv_fwd_split<NB, 2, false, EPI>
    ("bf16x3", 64, 64, "s1", N23, "rows", "plain", 0, 1),
    ("bf16x3", 64, 128, "s1", N97, "rows", "gate", 0, 1),
    ("bf16x3", 64, 128, "s1", N161, "rows", "plain", 0, 2),
    ("bf16x3", 128, 256, "s1", N97, "rows", "convbn", 0, 2),
    ("bf16x3", 64, 256, "tr2", N161, "rows", "plain", 0, 4),
    ("bf16x3", 64, 128, "s1", N321, "rows", "ld", 0, 4),
    ("bf16x3", 32, 64, "s1", N321B, "rows", "add", 0, 2),
    ("bf16x3", 32, 64, "s1", N6, "rows", "convbn", 0, 1),
    # ---- k_conv_fwd_split<NB, 3, false, EPI>
    ("bf16x6", 64, 128, "s1", N97, "rows", "plain", 0, 1),
    ("bf16x6", 32, 64, "s1", N23, "rows", "convbn", 0, 1),
    ("bf16x6", 64, 256, "s1", N97, "rows", "plain", 0, 2),
    ("bf16x6", 64, 128, "s1", N161, "rows", "gate", 0, 2),
    ("bf16x6", 128, 256, "tr2", N161B, "rows", "ld", 0, 2),
    ("bf16x6", 64, 64, "s1", N6, "rows", "add", 0, 1),
    # ---- k_conv_fwd<NB> (exact f32: NB follows cout alone; no statistics, no fused epilogue)
    ("f32", 64, 32, "s1", N23, "rows", "plain", 0, 1),
    ("f32", 64, 64, "s1", N97, "rows", "plain", 0, 2),
    ("f32", 64, 128, "s1", N23, "rows", "plain", 0, 4),
    ("f32", 32, 256, "tr2", N97B, "rows", "plain", 0, 4),
    ("f32", 32, 64, "s1", N6, "rows", "plain", 0, 2),
]


def launch_shape(lib, n_out, K, cin, cout, prec, planes=0, fused=0, table=1, scratch=0, flags=0):
    out = (ctypes.c_int32 * 8)()
    rc = lib.gcl_conv_fwd_launch_shape(n_out, K, cin, cout, PREC_CODE.get(prec, prec), planes, fused, table, scratch, flags, out)
    assert rc == 0, (n_out, K, cin, cout, prec, planes, fused, table, scratch, flags)
    s = dict(zip(("path", "nb", "pl", "pre_epi", "gx", "gy", "block", "swz"), out))
    s["pre"], s["epi"] = s["pre_epi"] & 1, s["pre_epi"] >> 1
    return s


def case_shape(lib, case, flags=None):
    """What the dispatcher launches for a CASES entry ("k1" has K = 1 and no table), from gcl_conv_fwd_launch_shape."""
    prec, cin, cout, conv, n, form, epi, fl, _nb = case
    return launch_shape(lib, n, 1 if conv == "k1" else 27, cin, cout, prec, int(form == "planes"), int(epi != "plain"),
                        int(conv != "k1"), 0, fl if flags is None else flags)


def instance_of(lib, case, flags=None):
    """Name of the kernel instance the dispatcher launches for a case."""
    s = case_shape(lib, case, flags)
    pre, e = ("false", "true")[s["pre"]], ("false", "true")[s["epi"]]
    return {F32: f"k_conv_fwd<{s['nb']}>", DMA_PATH: f"k_conv_fwd_dma<{s['nb']},{pre},{e}>",
            SPLIT: f"k_conv_fwd_split<{s['nb']},{s['pl']},{pre},{e}>"}[s["path"]]


def claimed_instance(case):
    """The instance a CASES entry claims: its section of the table and its NB column, spelled as a name."""
    prec, _cin, _cout, _conv, _n, form, epi, flags, nb = case
    pre, e = ("true" if form == "planes" else "false"), ("true" if epi != "plain" else "false")
    return {"f32": f"k_conv_fwd<{nb}>", "fp16x3": f"k_conv_fwd_dma<{nb},{pre},{e}>" if flags == DMA else
            f"k_conv_fwd_split<{nb},4,{pre},{e}>"}.get(prec, f"k_conv_fwd_split<{nb},{PREC_CODE[prec]},{pre},{e}>")


def full_instance_matrix():
    tf = ("true", "false")
    m = {f"k_conv_fwd_dma<{nb},{p},{e}>" for nb in (1, 2, 4) for p in tf for e in tf}
    m |= {f"k_conv_fwd_split<{nb},4,{p},{e}>" for nb in (1, 2, 4) for p in tf for e in tf}
    m |= {f"k_conv_fwd_split<{nb},2,false,{e}>" for nb in (1, 2, 4) for e in tf}
    m |= {f"k_conv_fwd_split<{nb},3,false,{e}>" for nb in (1, 2) for e in tf}
    m |= {f"k_conv_fwd<{nb}>" for nb in (1, 2, 4)}
    return m


def make_cloud(n, seed=None):
    """Exactly n unique int32 coords [n, 4] of one cloud: a blob at about one voxel in ten with a thin sheet through it
    (LiDAR-like), negative coordinates included.  Unique-ing shrinks a random draw, so more points are drawn and the
    shuffled result is cut to n."""
    rng = np.random.RandomState(n if seed is None else seed)
    e = max(4, int(round((1.25 * n) ** (1.0 / 3.0))))
    pts = rng.randint(-e, e, (n + (3 * n) // 5 + 64, 3))
    pts[: len(pts) // 4, 2] = rng.randint(-1, 1, len(pts) // 4)
    c = np.unique(pts, axis=0)
    rng.shuffle(c)
    assert len(c) >= n, (n, len(c))
    c = c[:n]
    return np.concatenate([np.zeros((n, 1), c.dtype), c], axis=1).astype(np.int32)


# the autograd direction at wide NB (section 3): (cin, cout, stride, transpose, fine rows,
#   {prec: (NB of the forward launch, NB of the input-gradient launch)})
LAYER_CASES = [
    (256, 256, 1, False, N161, {"fp16x3": (4, 4), "bf16x3": (4, 4), "bf16x6": (2, 2), "f32": (4, 4)}),
    (256, 256, 1, False, N97, {"fp16x3": (2, 2), "bf16x3": (2, 2), "bf16x6": (2, 2), "f32": (4, 4)}),
    (128, 256, 2, False, N321, {"fp16x3": (4, 4), "bf16x3": (4, 4), "bf16x6": (2, 2), "f32": (4, 4)}),
    (256, 128, 2, True, N321, {"fp16x3": (4, 4), "bf16x3": (4, 4), "bf16x6": (2, 2), "f32": (4, 4)}),
    (64, 64, 1, False, N321, {"fp16x3": (2, 2), "bf16x3": (2, 2), "bf16x6": (2, 2), "f32": (2, 2)}),
]


def layer_rows(stride, transpose, n_fine):
    """(n_in, n_out, coordinates) of a LAYER_CASES entry: a strided layer maps the cloud to its stride-2 level, a
    transposed one maps that level back."""
    C = make_cloud(n_fine)
    if stride == 1:
        return n_fine, n_fine, C
    n_coarse = len(O.stride_coords(C, 2))
    return (n_coarse, n_fine, C) if transpose else (n_fine, n_coarse, C)


# ---------------------------------------------------------------------------------------------------------------
# without a GPU: the table names the instances it reaches, and reaches all of them
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_names_its_kernel_instances_and_covers_the_matrix():
    """gcl_conv_fwd_launch_shape is host arithmetic, and it is what the dispatcher launches: every case reaches the instance
    (kernel family, NB, planes, operand form, epilogue) it claims, every case is ragged, the reached instances are exactly
    the 37 of the dispatcher, and the band edges of conv_fwd_nb are where the table assumes them (the 256-workgroup rule of
    small launches and the 513..1024 rule), so that a change of either fails here instead of moving the GPU tests onto
    other kernels."""
    from gcl_amd import _lib
    lib = _lib.load()
    reached, second_form = {}, set()
    for case in CASES:
        prec, cin, cout, conv, n, form, epi, flags, nb = case
        s = case_shape(lib, case)
        want_path = F32 if prec == "f32" else (DMA_PATH if flags == DMA else SPLIT)
        assert (s["path"], s["nb"], s["pl"], s["pre"], s["epi"]) == \
            (want_path, nb, PREC_CODE[prec], int(form == "planes"), int(epi != "plain")), (case, s)
        assert lib.gcl_conv_fwd_nb(n, cout, PREC_CODE[prec]) == nb, (prec, cout, n, nb)
        # the grid: one workgroup per 128-row tile and block of 32 NB columns; with more than one column block a 1-D grid
        # of the tiles rounded up to 8 (the exact-f32 kernel keeps the 2-D grid)
        tiles, cols = (n + 127) // 128, cout // (32 * nb)
        assert s["block"] == 256 and (s["gx"], s["gy"]) == \
            ((tiles, cols) if prec == "f32" else (((tiles + 7) // 8 * 8 * cols, 1) if cols > 1 else (tiles, 1))), (case, s)
        assert s["swz"] == (0 if prec == "f32" else (2 if cols > 1 else 0) | (16 if conv != "k1" else 0)), (case, s)
        sx = case_shape(lib, case, flags | XCD)       # GCL_CONV_XCD_RANGES: the same instance and grid, another launch order
        assert sx["swz"] == (0 if prec == "f32" else (2 if cols > 1 else 0) | 1) and \
            {k: v for k, v in sx.items() if k != "swz"} == {k: v for k, v in s.items() if k != "swz"}, (case, sx)
        assert 1 <= n % 128 <= 31 or 33 <= n % 128 <= 127, n
        assert epi in EPILOGUES and conv in ("s1", "tr2", "k1") and form in ("rows", "planes")
        assert cin % 32 == 0 and cout % 32 == 0
        assert (prec == "fp16x3") == (flags in (DMA, NO_DMA)) and (form == "rows" or prec == "fp16x3")
        assert prec != "f32" or epi == "plain"
        name = instance_of(lib, case)
        assert name == claimed_instance(case), (case, name)
        if prec == "fp16x3":          # the other staging of check (g): the twin instance
            other = instance_of(lib, case, flags ^ (DMA | NO_DMA))
            assert other == claimed_instance(case[:7] + (flags ^ (DMA | NO_DMA), nb)) and other != name
        reached[name] = reached.get(name, 0) + 1
        if n % 128 >= 33:
            second_form.add(name.split("<")[0] + ("/" + str(PREC_CODE[prec]) if "split" in name else ""))
    assert set(reached) == full_instance_matrix(), (sorted(full_instance_matrix() - set(reached)),
                                                    sorted(set(reached) - full_instance_matrix()))
    assert len(full_instance_matrix()) == 37
    # the second ragged form (33..127 rows in the last tile) in every kernel family
    assert second_form == {"k_conv_fwd_dma", "k_conv_fwd_split/4", "k_conv_fwd_split/2", "k_conv_fwd_split/3", "k_conv_fwd"}
    # tile counts below 8 and not divisible by 8 (GCL_CONV_XCD_RANGES splits the tiles over 8 XCDs, with a remainder)
    tiles = {(n + 127) // 128 for *_, n, _f, _e, _fl, _nb in CASES}
    assert min(tiles) < 8 and any(t > 8 and t % 8 for t in tiles)
    # band edges of conv_fwd_nb, two-plane precisions (fp16x3, bf16x3): (cout, last row count of a band, NB, NB after it)
    for prec in (4, 2):
        for cout, edge, nb, nb_next in [(64, 32640, 1, 2), (128, 16256, 1, 2), (128, 32640, 2, 4), (128, 65536, 4, 2),
                                        (128, 131072, 2, 4), (256, 8064, 1, 2), (256, 16256, 2, 4), (256, 32768, 4, 2),
                                        (256, 65536, 2, 4)]:
            assert lib.gcl_conv_fwd_nb(edge, cout, prec) == nb and lib.gcl_conv_fwd_nb(edge + 1, cout, prec) == nb_next, \
                (prec, cout, edge)
        assert lib.gcl_conv_fwd_nb(10 ** 7, 64, prec) == 2 and lib.gcl_conv_fwd_nb(10 ** 7, 32, prec) == 1
    # bf16x6 caps NB at 2; exact f32 follows cout alone
    for cout, edge in [(64, 32640), (128, 16256), (256, 8064)]:
        assert lib.gcl_conv_fwd_nb(edge, cout, 3) == 1 and lib.gcl_conv_fwd_nb(edge + 1, cout, 3) == 2
        assert lib.gcl_conv_fwd_nb(10 ** 7, cout, 3) == 2
    for n in (1, 8064, 8065, 32768, 32769, 10 ** 7):
        assert [lib.gcl_conv_fwd_nb(n, c, 0) for c in (32, 64, 96, 128, 256)] == [1, 2, 1, 4, 4]
        assert all(lib.gcl_conv_fwd_nb(n, 32, p) == 1 for p in (0, 2, 3, 4))       # the slice launches of the bitwise check
    # the layer cases: both launches of every precision are the NB the table claims
    for cin, cout, stride, transpose, n_fine, claims in LAYER_CASES:
        n_in, n_out, _ = layer_rows(stride, transpose, n_fine)
        for prec, (nb_fwd, nb_dgrad) in claims.items():
            assert lib.gcl_conv_fwd_nb(n_out, cout, PREC_CODE[prec]) == nb_fwd, (cin, cout, prec, n_out)
            assert lib.gcl_conv_fwd_nb(n_in, cin, PREC_CODE[prec]) == nb_dgrad, (cin, cout, prec, n_in)
        assert sorted(claims) == sorted(PREC_CODE)
    for nb in (2, 4):       # wide instances in both directions
        assert any(c["fp16x3"] == (nb, nb) for *_, c in LAYER_CASES)


def test_launch_shape_pins_the_paths_outside_the_matrix():
    """The inference kernels of GCL_CONV_TALL, the register-staged twin and the generic kernel: which shapes reach them,
    with which grid, and where gcl_conv_fwd_groups_scratch_len ends.  Defaults of `shape`: a 128 -> 64 layer of 2835 rows,
    K = 27 (108 steps per tile), fp16x3 on fp32 rows, sorted table, GCL_CONV_TALL, no scratch."""
    from gcl_amd import _lib
    lib = _lib.load()
    glen = lib.gcl_conv_fwd_groups_scratch_len

    def shape(n=N23, K=27, cin=128, cout=64, prec=4, planes=0, fused=0, table=1, scratch=0, flags=TALL):
        return launch_shape(lib, n, K, cin, cout, prec, planes, fused, table, scratch, flags)

    def path(**kw):
        return shape(**kw)["path"]
    tiles8 = ((N23 + 127) // 128 + 7) // 8 * 8
    s = shape(scratch=1)          # scratch handed over: four times as many four-wave workgroups + the slab sum
    assert (s["path"], s["nb"], s["pl"], s["pre"], s["epi"]) == (GROUPS, 2, 4, 0, 0), s
    assert (s["gx"], s["gy"], s["block"], s["swz"]) == (tiles8 * (64 // 64) * 4, 1, 256, 2 | 16), s
    assert glen(N23, 27, 128, 64) == 4 * N23 * 64
    s = shape()                   # no scratch: sixteen waves per workgroup
    assert (s["path"], s["gx"], s["gy"], s["block"], s["swz"]) == (TALL_PATH, tiles8 * (64 // 64), 1, 1024, 2 | 16), s
    assert shape(cout=256, scratch=1)["gx"] == tiles8 * 4 * 4 and shape(cout=256)["gx"] == tiles8 * 4
    assert shape(fused=1)["epi"] == 1 and shape(fused=1, scratch=1)["epi"] == 1
    # 65536 rows: the last size of the group launches
    assert glen(65536, 27, 128, 64) == 4 * 65536 * 64 and glen(65537, 27, 128, 64) == 0
    assert path(n=65536, scratch=1) == GROUPS and path(n=65537, scratch=1) == TALL_PATH and path(n=65537) == TALL_PATH
    # 108 steps per full tile, K >= 8, Cout a multiple of 64: decided by the layer's shape alone
    for kw in (dict(cin=96), dict(cout=96), dict(K=8, cin=416), dict(K=7, cin=512), dict(K=1, cin=3456)):
        assert glen(N23, kw.get("K", 27), kw.get("cin", 128), kw.get("cout", 64)) == 0, kw
        assert path(**kw) == DMA_PATH and path(scratch=1, **kw) == DMA_PATH, kw
    assert path(K=8, cin=448) == TALL_PATH and path(K=8, cin=448, scratch=1) == GROUPS and glen(N23, 8, 448, 64) > 0
    assert path(cin=128, cout=128) == TALL_PATH and path(cin=256, cout=192) == TALL_PATH
    assert glen(0, 27, 128, 64) == 0 and glen(N23, 28, 128, 64) == 0 and glen(N23, 27, 130, 64) == 0
    # fp16x3 on fp32 rows with a sorted table only, and not with GCL_CONV_XCD_RANGES; the flag itself
    for scratch in (0, 1):
        assert path(planes=1, scratch=scratch) == DMA_PATH and path(flags=TALL | XCD, scratch=scratch) == DMA_PATH
        assert path(prec=2, scratch=scratch) == SPLIT and path(prec=3, scratch=scratch) == SPLIT
        assert path(prec=0, scratch=scratch) == F32 and path(table=0, scratch=scratch) == DMA_PATH
        assert path(flags=0, scratch=scratch) == DMA_PATH and path(flags=DMA, scratch=scratch) == DMA_PATH
        assert path(flags=TALL | NO_DMA, scratch=scratch) == (GROUPS if scratch else TALL_PATH)
        assert path(cin=96, flags=TALL | NO_DMA, scratch=scratch) == SPLIT
    # GCL_CONV_NO_DMA: the register-staged twin; GCL_CONV_DMA changes nothing
    s = shape(flags=NO_DMA)
    assert (s["path"], s["pl"], s["nb"], s["block"]) == (SPLIT, 4, lib.gcl_conv_fwd_nb(N23, 64, 4), 256), s
    assert shape(flags=DMA) == shape(flags=0) and shape(flags=DMA)["path"] == DMA_PATH
    assert shape(flags=NO_DMA, prec=2) == shape(flags=0, prec=2)
    # generic shapes: TC = 8 up to Cout = 8, else 16; one thread per row, 256 rows per workgroup
    for kw, tc in ((dict(cin=32, cout=8), 8), (dict(cin=32, cout=9), 16), (dict(K=28, cin=32, cout=32), 16),
                   (dict(cin=3, cout=1), 8), (dict(K=125, cin=1, cout=17, prec=0), 16), (dict(cin=48, cout=64), 16)):
        for flags in (0, TALL, NO_DMA, XCD):
            s = shape(flags=flags, **kw)
            assert (s["path"], s["nb"], s["pl"], s["pre"], s["block"], s["swz"]) == (GENERIC, tc, 0, 0, 256, 0), (kw, s)
            assert (s["gx"], s["gy"]) == ((N23 + 255) // 256, -(-kw["cout"] // tc)), (kw, s)
    assert path(K=27, cin=32, cout=32, flags=0) == DMA_PATH
    # arguments the entry itself refuses
    out = (ctypes.c_int32 * 8)()
    ok = (N23, 27, 128, 64, 4, 0, 0, 1, 0, 0)
    assert lib.gcl_conv_fwd_launch_shape(*ok, out) == 0
    assert lib.gcl_conv_fwd_launch_shape(*ok, None) != 0
    for i, v in ((0, 0), (1, 0), (1, 126), (2, 0), (3, 0), (4, 1), (4, 5)):
        assert lib.gcl_conv_fwd_launch_shape(*ok[:i], v, *ok[i + 1:], out) != 0, (i, v)
    assert lib.gcl_conv_fwd_launch_shape(N23, 27, 128, 64, 2, 1, 0, 1, 0, 0, out) != 0          # planes are fp16x3
    assert lib.gcl_conv_fwd_launch_shape(N23, 27, 100, 64, 4, 1, 0, 1, 0, 0, out) != 0          # ... of MFMA shapes
    assert lib.gcl_conv_fwd_launch_shape(N23, 27, 128, 64, 0, 0, 1, 1, 0, 0, out) != 0          # exact f32 has no fused epilogue


def test_profile_labels_come_from_the_launch_shape_exports():
    """MinkowskiEngine/ops.py labels a profiled launch with the instance the library's own dispatcher function names: for
    every case of this table and of the weight-gradient table (tests/test_gpu_dw_instances.py) the label is the claimed
    instance, in the spelling profiles/pmc_summary.json is keyed by (a trailing `false` template argument left out)."""
    import re
    import test_gpu_dw_instances as DW
    from gcl_amd import _lib
    from gcl_amd.MinkowskiEngine import ops
    lib = _lib.load()
    for case in CASES:
        prec, cin, cout, conv, n, form, epi, flags, nb = case
        got = ops.fwd_instance_name(lib, n, 1 if conv == "k1" else 27, cin, cout, PREC_CODE[prec], form == "planes",
                                    epi != "plain", conv != "k1", flags=flags)
        assert got == claimed_instance(case), (case, got)
    assert ops.fwd_instance_name(lib, N23, 27, 64, 16, 4) == "k_conv_generic"
    assert ops.fwd_instance_name(lib, N23, 27, 128, 64, 4, fused=True, flags=TALL) == "k_conv_fwd_tall<true>"
    assert ops.fwd_instance_name(lib, N23, 27, 128, 64, 4, scratch=True, flags=TALL) == "k_conv_groups_sum<false,4>"
    labels = set()
    for case in DW.CASES:
        lname, ca, cb, prec, pl, claim = case[:6]
        L = DW.pair_list(lname)
        want = re.sub(r",false>$", ">", claim.split(" ")[0].replace("<false>", ""))
        got = ops.dw_instance_name(lib, L.K, ca, cb, DW.PREC_CODE[prec], pl, L.side, L.n_sorted(), int(L.seg[-1]))
        assert got == want, (DW.case_id(case), got, want)
        labels.add(got)
    # today's spellings, and the one label that changed: a range-grouped launch under its own name
    assert {"k_conv_bwd_weight_split<64,64,4,true>", "k_conv_bwd_weight_split<64,64,4,false>", "k_conv_bwd_weight_wg128",
            "k_conv_bwd_weight<64,64>", "k_conv_bwd_weight_generic", "k_conv_bwd_weight_split<64,64,4,false,true>",
            "k_bwd_weight_reduce"} <= labels, sorted(labels)
    assert ops.fwd_instance_name(lib, N23, 27, 128, 128, 4, planes=True) == "k_conv_fwd_dma<1,true,false>"
    assert ops.fwd_instance_name(lib, N161, 27, 128, 128, 4, planes=True) == "k_conv_fwd_dma<2,true,false>"


# ---------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


SENTINEL = 0x7FC5A5A5          # a quiet NaN: what is left of it inside y is found by isfinite, outside by its bits
GUARD = 4096                   # guard floats before and after the partials (y: 32 guard rows on either side)


class Guarded:
    """A tensor inside a larger sentinel-filled allocation."""

    def __init__(self, shape):
        numel = int(np.prod(shape))
        lead = GUARD if len(shape) != 2 else 32 * shape[1]
        self.buf = torch.full((lead + numel + lead,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.buf[lead:lead + numel].view(torch.float32).view(*shape)
        self.lead = lead

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[-self.lead:] == SENTINEL).all())


_MGRS, _PROBLEMS = {}, {}


class Problem:
    """One (cloud, conv, cin, cout): tables, operands, the epilogue's tensors and the fp64 product, shared by every case
    (precision, operand form, kernel choice, epilogue) that runs it."""

    def __init__(self, n, conv, cin, cout):
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        self.lib = lib = _lib.load()
        if n not in _MGRS:
            _MGRS[n] = ME.CoordinateManager(torch.from_numpy(make_cloud(n)).to(DEV))
        mgr = _MGRS[n]
        self.n_out, self.cin, self.cout = n, cin, cout
        if conv == "s1":
            km = mgr.get_kernel_map(1, 3, 1)
            self.nbr, self.table, self.n_in, self.K = km.nbr, km.sorted_table(), n, 27
        elif conv == "tr2":
            km = mgr.get_kernel_map(1, 3, 2)
            self.nbr, self.table, self.n_in, self.K = km.nbr_t, km.sorted_table(transposed=True), km.n_out, 27
        else:
            self.nbr, self.table, self.n_in, self.K = None, (None, None, None), n, 1
        assert self.nbr is None or tuple(self.nbr.shape) == (27, n)
        g = torch.Generator().manual_seed(n + 7 * cin + 13 * cout + len(conv))
        self.x = torch.randn(self.n_in, cin, generator=g).to(DEV)
        self.W = (0.1 * torch.randn(self.K, cin, cout, generator=g)).to(DEV)
        self.bias = (0.3 * torch.randn(cout, generator=g)).to(DEV)
        self.scale = (0.5 + torch.rand(cout, generator=g)).to(DEV)
        self.res_wide = torch.randn(n, cout + 64, generator=g).to(DEV)          # "ld": columns 32 .. 32 + cout of it
        self.res = torch.randn(n, cout, generator=g).to(DEV)                    # residual / gate of its own
        self.xa, self.wa = ME.ops.amax_slot(self.x.device), ME.ops.amax_slot(self.x.device)
        _lib.check(lib.gcl_amax(_lib.ptr(self.x), self.x.numel(), _lib.ptr(self.xa), 1, _lib.stream()), "gcl_amax")
        _lib.check(lib.gcl_amax(_lib.ptr(self.W), self.W.numel(), _lib.ptr(self.wa), 1, _lib.stream()), "gcl_amax")
        self._planes, self._packs = None, {}
        # the fp64 product over nbr (plain torch, fp64): y[j] = sum_k x[nbr[k, j]] W[k]
        xd, Wd = self.x.double(), self.W.double()
        if self.nbr is None:
            self.conv64 = xd @ Wd[0]
        else:
            self.conv64 = torch.zeros(n, cout, dtype=torch.float64, device=DEV)
            for k in range(27):
                rows = torch.nonzero(self.nbr[k] >= 0).squeeze(1)
                if len(rows):
                    self.conv64[rows] += xd[self.nbr[k][rows].long()] @ Wd[k]

    def planes(self):
        from gcl_amd import _lib
        if self._planes is None:
            self._planes = torch.empty((self.n_in, self.cin), dtype=torch.int32, device=DEV)
            _lib.check(self.lib.gcl_split_planes(_lib.ptr(self.x), self.n_in, self.cin, _lib.ptr(self.xa),
                                                 _lib.ptr(self._planes), _lib.stream()), "gcl_split_planes")
        return self._planes

    def packed(self, prec, j=None):
        """Weights in MFMA order: the whole tensor, or its 32-column slice j at the WHOLE tensor's scale (w_amax)."""
        from gcl_amd import _lib
        if (prec, j) not in self._packs:
            W = self.W if j is None else self.W[:, :, 32 * j:32 * j + 32].contiguous()
            code = PREC_CODE[prec]
            wp = torch.empty(self.lib.gcl_pack_weights_bytes(self.K, self.cin, W.shape[2], code), dtype=torch.uint8, device=DEV)
            _lib.check(self.lib.gcl_pack_weights(_lib.ptr(W), self.K, self.cin, W.shape[2], 0, code,
                                                 _lib.ptr(self.wa) if code == 4 else None, _lib.ptr(wp), _lib.stream()), "pack")
            self._packs[(prec, j)] = wp
        return self._packs[(prec, j)]

    def expected64(self, epi):
        e = EPILOGUES[epi]
        v = self.conv64 * (self.scale.double() if e.get("scale") else 1.0) + self.bias.double()
        r = {"own": self.res, "wide": self.res_wide[:, 32:32 + self.cout], None: None}[e.get("res")]
        if e.get("relu") == 2:
            return torch.where(r > 0, v, torch.zeros_like(v))
        if r is not None:
            v = v + r.double()
        return v.clamp_min(0.0) if e.get("relu") == 1 else v

    def run(self, prec, form, epi, flags, j=None, want_stats=True):
        """One launch: the whole width, or (j) the 32-column slice j as a launch of its own -- weights, bias and col_scale
        sliced, the residual as a column slice of the same tensor (gcl_conv_fwd_fused_ld).  Returns (y, stats, max|y|);
        y and stats sit between guards that are checked here."""
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        lib, code = self.lib, PREC_CODE[prec]
        e = EPILOGUES[epi] if isinstance(epi, str) else epi
        cout = self.cout if j is None else 32
        c0 = 0 if j is None else 32 * j
        off = lambda t, el: ctypes.c_void_p(t.data_ptr() + 4 * el)
        tbl, order, mask = self.table
        y = Guarded((self.n_out, cout))
        stats = Guarded((4, cout, (self.n_out + 127) // 128)) if (want_stats and code != 0) else None
        xin = self.planes() if form == "planes" else self.x
        head = (_lib.ptr(xin), self.n_in, int(form == "planes"), _lib.ptr(self.packed(prec, j)), code,
                _lib.ptr(self.xa) if code == 4 else None, _lib.ptr(self.wa) if code == 4 else None, _lib.ptr(tbl),
                _lib.ptr(order), _lib.ptr(mask), self.n_out, self.K, self.cin, cout, off(self.bias, c0))
        tail = (_lib.ptr(y.t), _lib.ptr(stats.t) if stats else None, flags, _lib.stream())
        slot = None
        with torch.cuda.device(DEV):
            if not e:
                _lib.check(lib.gcl_conv_fwd(*head, *tail), "gcl_conv_fwd")
            else:
                slot = ME.ops.amax_slot(self.x.device) if e.get("amax") else None
                scale = off(self.scale, c0) if e.get("scale") else None
                if e["res"] == "wide":
                    res, ld = off(self.res_wide, 32 + c0), self.cout + 64
                else:
                    res, ld = off(self.res, c0), (0 if j is None else self.cout)
                if ld == 0:
                    _lib.check(lib.gcl_conv_fwd_fused(*head, scale, res, e["relu"], _lib.ptr(slot), *tail), "gcl_conv_fwd_fused")
                else:
                    _lib.check(lib.gcl_conv_fwd_fused_ld(*head, scale, res, ld, e["relu"], _lib.ptr(slot), *tail),
                               "gcl_conv_fwd_fused_ld")
        torch.cuda.synchronize()
        assert y.intact(), "the launch wrote outside y"
        assert stats is None or stats.intact(), "the launch wrote outside the tile partials"
        return y.t, (stats.t if stats else None), (ME.ops.amax_value(slot) if slot is not None else None)


def problem(n, conv, cin, cout):
    key = (n, conv, cin, cout)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(*key)
    return _PROBLEMS[key]


def where_differs(a, b):
    """(row, column, values) of the first differing element, for the failure message."""
    bad = torch.nonzero(~((a == b) | (a.isnan() & b.isnan())))
    if len(bad) == 0:
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at {i}: {float(a[i])!r} != {float(b[i])!r}"


_T0 = []


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv_fwd_instance(case):
    """Checks (a) - (g) of one case; see the module docstring.  On failure the message names the instance and the first
    differing (row, column) or (plane, column, tile)."""
    from gcl_amd import _lib
    import gcl_amd.MinkowskiEngine as ME
    from conftest import precision_log_path
    prec, cin, cout, conv, n, form, epi, flags, nb = case
    if not _T0:
        _T0.append(time.time())
    lib = _lib.require_gpu()
    code = PREC_CODE[prec]
    name = instance_of(lib, case)
    p = problem(n, conv, cin, cout)
    n_out, n_tiles = p.n_out, (p.n_out + 127) // 128
    assert n_out == n and lib.gcl_conv_fwd_nb(n_out, cout, code) == nb and lib.gcl_conv_fwd_nb(n_out, 32, code) == 1
    e = EPILOGUES[epi]
    y, stats, amax = p.run(prec, form, epi, flags)

    # (a) fp64, (d) every row of y written
    assert bool(torch.isfinite(y).all()), f"{name}: {int((~torch.isfinite(y)).sum())} elements of y left unwritten"
    err = rel_l2(y, p.expected64(epi))
    print(f"[conv instance] {name} {prec} {cin}->{cout} {conv} n_out={n_out} {epi}: rel-L2 vs fp64 {err:.3e}")
    with open(precision_log_path(), "a") as fh:
        fh.write(f"conv_instance {name} {prec} {cin}->{cout} {conv} n_out={n_out} epi={epi} rel_l2={err:.4e}\n")
    assert err < PREC_TOL[prec], (name, err)

    # (e) the exact relations of the fused epilogue
    if amax is not None:
        assert float(amax) == float(y.abs().max()), (name, float(amax), float(y.abs().max()))
    if e.get("relu") == 1:          # the same launch without the ReLU
        y0, _, _ = p.run(prec, form, dict(e, relu=0), flags, want_stats=False)
        assert torch.equal(y, torch.clamp_min(y0, 0.0)), (name, where_differs(y, torch.clamp_min(y0, 0.0)))
    if e.get("relu") == 2:          # the plain launch, gated
        y0, _, _ = p.run(prec, form, "plain", flags, want_stats=False)
        want = torch.where(p.res > 0, y0, torch.zeros_like(y0))
        assert torch.equal(y, want), (name, where_differs(y, want))
        rc = lib.gcl_conv_fwd_fused(_lib.ptr(p.x), p.n_in, 0, _lib.ptr(p.packed(prec)), code, _lib.ptr(p.xa), _lib.ptr(p.wa),
                                    _lib.ptr(p.table[0]), _lib.ptr(p.table[1]), _lib.ptr(p.table[2]), n_out, p.K, cin, cout,
                                    None, None, None, 2, None, _lib.ptr(y0), None, 0, _lib.stream())
        assert rc != 0          # mode 2 without its gate tensor

    # (b) bit for bit the NB = 1 launches of the 32-column slices
    slice_amax = []
    for j in range(cout // 32):
        ys, ss, sa = p.run(prec, form, epi, flags, j=j)
        assert torch.equal(y[:, 32 * j:32 * j + 32], ys), \
            f"{name}: column block {j} differs from its NB = 1 launch: {where_differs(y[:, 32 * j:32 * j + 32], ys)}"
        if stats is not None:
            assert torch.equal(stats[:, 32 * j:32 * j + 32], ss), \
                f"{name}: partials of column block {j} (plane, column, tile): {where_differs(stats[:, 32 * j:32 * j + 32], ss)}"
        if sa is not None:
            slice_amax.append(float(sa))
    if amax is not None:
        assert float(amax) == max(slice_amax), (name, float(amax), slice_amax)

    # (c) the tile partials of the real epilogue: tile t holds the rows order[128 t .. 128 t + 127]
    if stats is not None:
        assert bool(torch.isfinite(stats).all()), f"{name}: partials left unwritten"
        order = p.table[1].long() if p.table[1] is not None else torch.arange(n_out, device=DEV)
        ys = y[order]
        pad = n_tiles * 128 - n_out

        def tiles(t, fill):
            return torch.cat([t, torch.full((pad, cout), fill, dtype=t.dtype, device=DEV)]).view(n_tiles, 128, cout)
        lo, hi = tiles(ys, float("inf")).amin(1).T, tiles(ys, float("-inf")).amax(1).T
        assert torch.equal(stats[2], lo), f"{name}: tile minimum (column, tile): {where_differs(stats[2], lo)}"
        assert torch.equal(stats[3], hi), f"{name}: tile maximum (column, tile): {where_differs(stats[3], hi)}"
        yd = tiles(ys.double(), 0.0)
        s1, a1, s2 = yd.sum(1).T, yd.abs().sum(1).T, (yd * yd).sum(1).T
        u = 2.0 ** -24          # 128 fp32 additions (+ one rounding of each square): derived, not tuned
        d1, d2 = (stats[0].double() - s1).abs(), (stats[1].double() - s2).abs()
        assert bool((d1 <= 128 * u * a1).all()), (name, "sum", float((d1 / a1.clamp_min(1e-300)).max()) / u)
        assert bool((d2 <= 130 * u * s2).all()), (name, "squares", float((d2 / s2.clamp_min(1e-300)).max()) / u)
        mean, rstd = torch.empty(cout, device=DEV), torch.empty(cout, device=DEV)
        xrange = torch.empty((2, cout), device=DEV)
        ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
        with torch.cuda.device(DEV):
            slot = ME.ops.amax_slot(y.device)
            _lib.check(lib.gcl_bn_stats_from_tiles_range(_lib.ptr(stats), n_tiles, n_out, cout, 1e-5, 0.05, None, None,
                                                         _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(xrange), _lib.ptr(ones),
                                                         _lib.ptr(zeros), 0, None, None, _lib.ptr(slot), _lib.stream()),
                       "gcl_bn_stats_from_tiles_range")
        y64 = y.double()
        assert rel_l2(mean, y64.mean(0)) < 1e-6, (name, rel_l2(mean, y64.mean(0)))
        want_rstd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)
        assert rel_l2(rstd, want_rstd) < 1e-6, (name, rel_l2(rstd, want_rstd))
        assert torch.equal(xrange[0], y.amin(0)) and torch.equal(xrange[1], y.amax(0)), name

    # (f) GCL_CONV_XCD_RANGES is a launch-order hint only
    yx, sx, ax = p.run(prec, form, epi, flags | XCD)
    assert torch.equal(yx, y), f"{name}: GCL_CONV_XCD_RANGES changes y: {where_differs(yx, y)}"
    assert stats is None or torch.equal(sx, stats), f"{name}: GCL_CONV_XCD_RANGES changes the partials"
    assert amax is None or torch.equal(ax, amax)

    # (g) LDS-DMA staging against register staging
    if prec == "fp16x3":
        other = instance_of(lib, case, flags ^ (DMA | NO_DMA))
        assert other != name
        yo, so, ao = p.run(prec, form, epi, flags ^ (DMA | NO_DMA))
        assert torch.equal(yo, y), f"{name} against {other}: {where_differs(yo, y)}"
        assert torch.equal(so, stats), f"{name} against {other}, partials: {where_differs(so, stats)}"
        assert amax is None or torch.equal(ao, amax)
    if case is CASES[-1]:
        print(f"[conv instance] {len(CASES)} cases in {time.time() - _T0[0]:.1f} s")


# ---------------------------------------------------------------------------------------------------------------
# the input-gradient and autograd direction at wide NB, through the layer surface
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["fp16x3", "bf16x6", "f32", "bf16x3"])
def precision(request):
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import ops
    old = ops.PRECISION
    ME.set_conv_precision(request.param)
    yield request.param
    ME.set_conv_precision(old)


_LAYER_REF = {}


def _layer_reference(cin, cout, stride, transpose, n_fine):
    """Operands and the fp64 oracle's y, dx, dW of a layer case; made once, shared by the four precisions."""
    key = (cin, cout, stride, transpose, n_fine)
    if key not in _LAYER_REF:
        n_in, n_out, C = layer_rows(stride, transpose, n_fine)
        omgr = O.CoordinateManager(C)
        g = torch.Generator().manual_seed(cin + cout + n_fine)
        x = torch.randn(n_in, cin, generator=g).double()
        W = (0.1 * torch.randn(27, cin, cout, generator=g)).double()
        gy = torch.randn(n_out, cout, generator=g).double()
        xo, Wo = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
        yo = O.sparse_conv(xo, Wo, omgr.get_kernel_map(1, 3, stride), n_out, transpose=transpose)
        yo.backward(gy)
        _LAYER_REF[key] = (C, x, W, gy, yo.detach(), xo.grad, Wo.grad)
    return _LAYER_REF[key]


@gpu
@pytest.mark.parametrize("cin,cout,stride,transpose,n_fine,claims", LAYER_CASES,
                         ids=[f"{c[0]}-{c[1]}-s{c[2]}{'t' if c[3] else ''}-{c[4]}" for c in LAYER_CASES])
def test_layer_forward_and_input_gradient_at_wide_nb(cin, cout, stride, transpose, n_fine, claims, precision):
    """ME.MinkowskiConvolution(+Transpose) at row counts where the forward launch (n_out, cout) and the input-gradient launch
    (n_in, effective cout = cin; mode-1 / mode-2 weights, the transposed / mirrored table) run the NB = 2 and NB = 4 instances:
    y, dx, dW against the oracle at the per-operator bound, under all four precisions."""
    from gcl_amd import _lib
    import gcl_amd.MinkowskiEngine as ME
    from conftest import precision_log_path
    lib = _lib.require_gpu()
    C, x, W, gy, yo, dxo, dWo = _layer_reference(cin, cout, stride, transpose, n_fine)
    mgr = ME.CoordinateManager(torch.from_numpy(C).to(DEV))
    t_in = 2 if transpose else 1
    n_in, n_out = len(x), len(gy)
    assert mgr.num_rows(t_in) == n_in and mgr.num_rows(t_in // stride if transpose else t_in * stride) == n_out
    code = PREC_CODE[precision]
    nbs = (lib.gcl_conv_fwd_nb(n_out, cout, code), lib.gcl_conv_fwd_nb(n_in, cin, code))
    assert nbs == claims[precision], (nbs, claims[precision])
    cls = ME.MinkowskiConvolutionTranspose if transpose else ME.MinkowskiConvolution
    conv = cls(cin, cout, kernel_size=3, stride=stride, dimension=3).to(DEV)
    with torch.no_grad():
        conv.kernel.copy_(W.float().reshape(conv.kernel.shape))
    xg = x.float().to(DEV).requires_grad_(True)
    y = conv(ME.SparseTensor(xg, coordinate_map_key=ME.CoordinateMapKey(t_in), coordinate_manager=mgr)).F
    assert y.shape == yo.shape
    y.backward(gy.float().to(DEV))
    errs = dict(y=rel_l2(y.detach().cpu(), yo), dx=rel_l2(xg.grad.cpu(), dxo),
                dW=rel_l2(conv.kernel.grad.cpu().reshape(dWo.shape), dWo))
    print(f"[conv layer] {cin}->{cout} stride {stride}{' transposed' if transpose else ''} {precision} "
          f"n_in={n_in} n_out={n_out} NB fwd/dgrad {nbs}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    with open(precision_log_path(), "a") as fh:
        fh.write(f"conv_layer {cin}->{cout} s{stride}{'t' if transpose else ''} {precision} n_in={n_in} n_out={n_out} "
                 f"nb_fwd={nbs[0]} nb_dgrad={nbs[1]} " + " ".join(f"{k}_rel_l2={v:.4e}" for k, v in errs.items()) + "\n")
    tol = PREC_TOL[precision]
    assert errs["y"] < tol and errs["dx"] < tol and errs["dW"] < tol, errs
