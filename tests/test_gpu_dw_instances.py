"""Every kernel instance behind gcl_conv_bwd_weight / gcl_conv_bwd_weight_rg, named and tested offset by offset.

For channel counts that are multiples of 32 the weight-gradient entry is 33 template instances, picked by the host
dispatcher (dw_launch_shape in csrc/conv.hip) from (K, Ca, Cb, prec, operand form, sorted side, rows of the sorted side):

    k_conv_bwd_weight<TA, TB>                        exact f32                   TA, TB in {32, 64}        4
    k_conv_bwd_weight_split<TA, TB, PL, false, false>  bf16x3 / bf16x6 / fp16x3 rows   PL 2, 3, 4 x 4 tiles     12
    k_conv_bwd_weight_split<TA, TB, 4, true, false>    fp16x3 plane images             4 tiles                   4
    k_conv_bwd_weight_split<TA, TB, PL, false, true>   range-grouped (RG) mode         PL 2, 3, 4 x 4 tiles     12
    k_conv_bwd_weight_wg128<false>                   fp16x3 planes, 128 x 128 block                            1

plus k_conv_bwd_weight_generic for every other channel count, and the reduce kernels k_bwd_weight_reduce,
k_bwd_weight_reduce_rg and k_pair_bounds.  CASES names the instance and the launch shape (W workgroups of `per` chunks;
rows per range and ranges of the RG mode) of every case; a test that needs no GPU pins those claims against
gcl_conv_bwd_weight_launch_shape -- the function the dispatcher itself calls -- requires the table to reach all 33 + 1, and
derives from the returned numbers that the table holds every launch-shape edge: one workgroup over many offsets, empty
segments first / last / two in a row, a one-pair segment, the cap of 512 workgroups with a short last one, idle workgroups
of the swizzled grid, K = 125, and for the RG mode all four range sizes, a range count that is no multiple of 8, pairs on
both sides of a range boundary, empty cells, ragged cells of more than one chunk and both sorted sides.

Operands come from synthetic pair lists built in numpy (the entry takes any lists whose segments are padded with -1 to
multiples of 128 and whose sorted side ascends inside a segment), so every edge sits exactly where the case wants it at the
smallest size: an RG case declares 310 k rows on its sorted side and holds some ten thousand pairs.

Per case, on the GPU: every dW[k] on its own against the fp64 product over that offset's real pairs at the per-operator
bound PREC_TOL (and the whole tensor at the same bound); exactly +0.0 for an offset without pairs; scratch of exactly
gcl_conv_bwd_weight_scratch_len floats and dW inside sentinel-filled allocations whose guard words must survive, scratch
itself prefilled with the sentinel (a slab that is read but never written would surface as a NaN); two launches bit for bit,
and a launch over zeroed scratch bit for bit.  RG cases also: gcl_conv_bwd_weight_bounds against np.searchsorted, the
launch with those prebuilt bounds bit for bit, and the classic k-major launch of the same lists (sorted_side = 0) at
PREC_TOL.  wg128 cases also: the 64 x 64-block kernel (bit 1 of `planes`) at PREC_TOL.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu

PREC_CODE = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 4}
# per-operator tolerance (relative L2 against fp64) of each MFMA arithmetic: tests/test_gpu_parity.py PREC_TOL
PREC_TOL = {"f32": 2e-6, "bf16x6": 2e-6, "bf16x3": 3e-5, "fp16x3": 2e-6}
# include/gcl_amd.h GCL_DW_PATH_*
NONE, GENERIC, F32, SPLIT, PLANES, RG, WG128 = range(7)
CHUNK = 128                         # GCL_PAIR_CHUNK
NO_PAIRS = "k_bwd_weight_reduce alone (no pairs)"


# ---------------------------------------------------------------------------------------------------------------
# synthetic pair lists
# ---------------------------------------------------------------------------------------------------------------
class PairList:
    """pair_a / pair_b / seg_off of K segments, each padded with -1 to a multiple of 128; the rows of operand `side`
    (1 = A, 2 = B) ascend inside every segment.  Rows repeat; row 0 and the last row of both operands occur."""

    def __init__(self, K, n_a, n_b, side, sorted_rows, seed):
        rng = np.random.RandomState(seed)
        n_s, n_o = (n_a, n_b) if side == 1 else (n_b, n_a)
        srt = [np.sort(np.asarray(r, np.int64)) for r in sorted_rows]
        oth = [rng.randint(0, n_o, len(r)).astype(np.int64) for r in srt]
        assert len(srt) == K
        nz = [k for k in range(K) if len(srt[k])]
        if nz:
            srt[nz[0]][0], srt[nz[-1]][-1] = 0, n_s - 1
            oth[nz[0]][0], oth[nz[-1]][-1] = n_o - 1, 0
            assert sum(len(r) for r in srt) > 1 or (n_s == 1 and n_o == 1)
        self.K, self.n_a, self.n_b, self.side = K, n_a, n_b, side
        self.seg = np.zeros(K + 1, np.int64)
        for k in range(K):
            self.seg[k + 1] = self.seg[k] + (len(srt[k]) + CHUNK - 1) // CHUNK * CHUNK
        ps, po = np.full(self.seg[K], -1, np.int32), np.full(self.seg[K], -1, np.int32)
        for k in range(K):
            ps[self.seg[k]:self.seg[k] + len(srt[k])] = srt[k]
            po[self.seg[k]:self.seg[k] + len(oth[k])] = oth[k]
        self.pair_a, self.pair_b = (ps, po) if side == 1 else (po, ps)
        self.sorted = srt                                          # real rows of the sorted side, per offset
        self.real_a, self.real_b = (srt, oth) if side == 1 else (oth, srt)
        self.counts = np.array([len(r) for r in srt])
        self.nc = int(self.seg[K] // CHUNK)
        for rows, n in ((self.real_a, n_a), (self.real_b, n_b)):
            allr = np.concatenate(rows) if nz else np.zeros(0, np.int64)
            assert not nz or (allr.min() == 0 and allr.max() == n - 1), "row 0 and the last row of each operand"
            assert len(allr) <= 2 or len(np.unique(allr)) < len(allr), "indices repeat"
        for r in srt:
            assert (np.diff(r) >= 0).all()

    def n_sorted(self, side=None):
        return {0: 0, 1: self.n_a, 2: self.n_b}[self.side if side is None else side]

    def cells(self, rr, nr):
        """[K, nr + 1] cell limits of the RG mode: first position of offset k whose sorted-side row is >= j rr (padding
        counts as +infinity)."""
        return np.stack([self.seg[k] + np.searchsorted(self.sorted[k], np.arange(nr + 1, dtype=np.int64) * rr, "left")
                         for k in range(self.K)])


def _ragged(chunks, rng):
    """Real pairs of segments of the given chunk counts: the last chunk of a segment holds 1 .. 128 real entries."""
    return [0 if c == 0 else CHUNK * (c - 1) + int(rng.randint(1, CHUNK + 1)) for c in chunks]


def _classic(K, n_a, n_b, counts, seed):
    rng = np.random.RandomState(seed + 1000)
    return PairList(K, n_a, n_b, 2, [rng.randint(0, n_b, c) for c in counts], seed)


def _rg(K, n_a, n_b, side, rr, empty, seed):
    """Sorted-side rows of an RG list: a few pairs spread over all rows (most cells hold none or a handful), one dense run
    inside a single range (a cell of more than a chunk with a ragged end), and the rows j rr - 1 and j rr on both sides
    of range boundaries."""
    rng = np.random.RandomState(seed + 1000)
    n_s = n_a if side == 1 else n_b
    nr = (n_s + rr - 1) // rr
    rows = []
    for k in range(K):
        if k in empty:
            rows.append(np.zeros(0, np.int64))
            continue
        j0 = (5 * k + 1) % nr
        parts = [rng.randint(0, n_s, 30 + 3 * k), rng.randint(j0 * rr, min((j0 + 1) * rr, n_s), 131 + 17 * k)]
        for j in {1, (k % (nr - 1)) + 1, nr - 1}:
            parts.append(np.array([j * rr - 1, j * rr, j * rr]))
        rows.append(np.concatenate(parts))
    return PairList(K, n_a, n_b, side, rows, seed)


def _make_list(name):
    rng = np.random.RandomState(len(name) + 31 * ord(name[0]))
    if name in ("S", "S1"):     # 15 chunks, K = 27: ONE workgroup walks 13 offsets; empty first, last, runs of empties; one pair
        counts = np.zeros(27, int)
        for k, c in {1: 128, 2: 100, 3: 130, 5: 1, 7: 64, 8: 128, 9: 33, 10: 127, 11: 129, 14: 5, 16: 96, 20: 128, 25: 17}.items():
            counts[k] = c
        return _classic(27, 37 if name == "S" else 1, 53, counts, 1)
    if name == "M":             # 107 chunks: 13 workgroups (no multiple of 8) of 9 chunks, the 13th without work
        chunks = [0, 5, 3, 6, 4, 1, 7, 2, 5, 4, 6, 3, 0, 0, 13, 4, 5, 3, 6, 4, 5, 2, 7, 4, 3, 5, 0]
        counts = _ragged(chunks, rng)
        counts[5] = 1
        return _classic(27, 700, 900, counts, 2)
    if name == "C":             # 4100 chunks: just beyond the cap of 512 workgroups
        return _classic(27, 2000, 2100, _ragged([0] + [164] * 25 + [0], rng), 3)
    if name == "Q":             # K = 125
        chunks = [0 if (k % 7 == 0 or k in (62, 124)) else 1 + k % 3 for k in range(125)]
        return _classic(125, 500, 300, _ragged(chunks, rng), 4)
    if name == "P1":            # one pair in all
        return _classic(27, 1, 1, [int(k == 13) for k in range(27)], 5)
    if name == "Z":             # no pairs at all
        return _classic(27, 5, 7, [0] * 27, 6)
    if name == "R512":
        return _rg(5, 1500, 33100, 2, 512, {3}, 7)
    if name == "R1024":
        return _rg(27, 1200, 78000, 2, 1024, {0, 13, 14, 26}, 8)
    if name == "R2048":
        return _rg(27, 900, 156000, 2, 2048, {26}, 9)
    if name == "R4096":
        return _rg(27, 310700, 1100, 1, 4096, {7}, 10)
    raise KeyError(name)


_LISTS = {}


def pair_list(name):
    if name not in _LISTS:
        _LISTS[name] = _make_list(name)
    return _LISTS[name]


# (list, Ca, Cb, prec, planes argument, instance, W, per, rr, n_ranges)
CASES = [
    # ---- k_conv_bwd_weight<TA, TB>
    ("C", 32, 32, "f32", 0, "k_conv_bwd_weight<32,32>", 512, 9, 0, 0),
    ("M", 128, 64, "f32", 0, "k_conv_bwd_weight<64,64>", 13, 9, 0, 0),
    ("S", 64, 96, "f32", 0, "k_conv_bwd_weight<64,32>", 1, 15, 0, 0),
    ("Q", 32, 64, "f32", 0, "k_conv_bwd_weight<32,64>", 26, 8, 0, 0),
    # ---- k_conv_bwd_weight_split<TA, TB, PL, false, false>
    ("S1", 32, 32, "bf16x3", 0, "k_conv_bwd_weight_split<32,32,2,false,false>", 1, 15, 0, 0),
    ("Q", 64, 64, "bf16x3", 0, "k_conv_bwd_weight_split<64,64,2,false,false>", 26, 8, 0, 0),
    ("M", 64, 32, "bf16x3", 0, "k_conv_bwd_weight_split<64,32,2,false,false>", 13, 9, 0, 0),
    ("S", 96, 64, "bf16x3", 0, "k_conv_bwd_weight_split<32,64,2,false,false>", 1, 15, 0, 0),
    ("Q", 32, 32, "bf16x6", 0, "k_conv_bwd_weight_split<32,32,3,false,false>", 26, 8, 0, 0),
    ("S", 64, 64, "bf16x6", 0, "k_conv_bwd_weight_split<64,64,3,false,false>", 1, 15, 0, 0),
    ("S1", 64, 32, "bf16x6", 0, "k_conv_bwd_weight_split<64,32,3,false,false>", 1, 15, 0, 0),
    ("M", 32, 128, "bf16x6", 0, "k_conv_bwd_weight_split<32,64,3,false,false>", 13, 9, 0, 0),
    ("M", 96, 32, "fp16x3", 0, "k_conv_bwd_weight_split<32,32,4,false,false>", 13, 9, 0, 0),
    ("C", 32, 32, "fp16x3", 0, "k_conv_bwd_weight_split<32,32,4,false,false>", 512, 9, 0, 0),
    ("M", 128, 64, "fp16x3", 0, "k_conv_bwd_weight_split<64,64,4,false,false>", 13, 9, 0, 0),
    ("Q", 64, 32, "fp16x3", 0, "k_conv_bwd_weight_split<64,32,4,false,false>", 26, 8, 0, 0),
    ("S", 32, 64, "fp16x3", 0, "k_conv_bwd_weight_split<32,64,4,false,false>", 1, 15, 0, 0),
    ("P1", 64, 64, "fp16x3", 0, "k_conv_bwd_weight_split<64,64,4,false,false>", 1, 1, 0, 0),
    # ---- k_conv_bwd_weight_split<TA, TB, 4, true, false>
    ("S", 96, 96, "fp16x3", 1, "k_conv_bwd_weight_split<32,32,4,true,false>", 1, 15, 0, 0),
    ("M", 128, 64, "fp16x3", 1, "k_conv_bwd_weight_split<64,64,4,true,false>", 13, 9, 0, 0),
    ("M", 64, 96, "fp16x3", 1, "k_conv_bwd_weight_split<64,32,4,true,false>", 13, 9, 0, 0),
    ("Q", 160, 64, "fp16x3", 1, "k_conv_bwd_weight_split<32,64,4,true,false>", 26, 8, 0, 0),
    # ---- k_conv_bwd_weight_wg128 (each case also runs bit 1 of `planes`: k_conv_bwd_weight_split<64,64,4,true,false>)
    ("S", 128, 128, "fp16x3", 1, "k_conv_bwd_weight_wg128<false>", 1, 15, 0, 0),
    ("P1", 128, 128, "fp16x3", 1, "k_conv_bwd_weight_wg128<false>", 1, 1, 0, 0),
    ("M", 256, 128, "fp16x3", 1, "k_conv_bwd_weight_wg128<false>", 13, 9, 0, 0),
    ("Q", 128, 128, "fp16x3", 1, "k_conv_bwd_weight_wg128<false>", 26, 8, 0, 0),
    # ---- k_conv_bwd_weight_split<TA, TB, PL, false, true>: the range-grouped mode
    ("R512", 32, 32, "bf16x3", 0, "k_conv_bwd_weight_split<32,32,2,false,true>", 1, 8, 512, 65),
    ("R512", 32, 32, "bf16x6", 0, "k_conv_bwd_weight_split<32,32,3,false,true>", 1, 8, 512, 65),
    ("R512", 32, 32, "fp16x3", 0, "k_conv_bwd_weight_split<32,32,4,false,true>", 1, 8, 512, 65),
    ("R1024", 64, 64, "bf16x3", 0, "k_conv_bwd_weight_split<64,64,2,false,true>", 11, 8, 1024, 77),
    ("R1024", 64, 64, "bf16x6", 0, "k_conv_bwd_weight_split<64,64,3,false,true>", 11, 8, 1024, 77),
    ("R1024", 64, 64, "fp16x3", 0, "k_conv_bwd_weight_split<64,64,4,false,true>", 11, 8, 1024, 77),
    ("R2048", 64, 32, "bf16x3", 0, "k_conv_bwd_weight_split<64,32,2,false,true>", 12, 9, 2048, 77),
    ("R2048", 64, 32, "bf16x6", 0, "k_conv_bwd_weight_split<64,32,3,false,true>", 12, 9, 2048, 77),
    ("R2048", 64, 32, "fp16x3", 0, "k_conv_bwd_weight_split<64,32,4,false,true>", 12, 9, 2048, 77),
    ("R4096", 32, 64, "bf16x3", 0, "k_conv_bwd_weight_split<32,64,2,false,true>", 12, 9, 4096, 76),
    ("R4096", 32, 64, "bf16x6", 0, "k_conv_bwd_weight_split<32,64,3,false,true>", 12, 9, 4096, 76),
    ("R4096", 32, 64, "fp16x3", 0, "k_conv_bwd_weight_split<32,64,4,false,true>", 12, 9, 4096, 76),
    # ---- k_conv_bwd_weight_generic (exact fp32 whatever prec says)
    ("Q", 1, 1, "fp16x3", 0, "k_conv_bwd_weight_generic", 26, 8, 0, 0),
    ("Q", 17, 33, "fp16x3", 0, "k_conv_bwd_weight_generic", 26, 8, 0, 0),
    ("Q", 30, 7, "f32", 0, "k_conv_bwd_weight_generic", 26, 8, 0, 0),
    # ---- no pairs at all: the reduce alone writes the zeros
    ("Z", 64, 64, "fp16x3", 0, NO_PAIRS, 1, 1, 0, 0),
    ("Z", 128, 128, "fp16x3", 1, NO_PAIRS, 1, 1, 0, 0),
    ("Z", 17, 33, "f32", 0, NO_PAIRS, 1, 1, 0, 0),
]


def case_id(c):
    inst = c[5].split(" ")[0].replace("k_conv_bwd_weight", "dw").replace("k_bwd_weight_reduce", "none")
    return "-".join(str(v) for v in c[:5]) + "-" + inst.replace("<", "_").replace(">", "").replace(",", "_")


def launch_shape(lib, K, ca, cb, prec, planes, side, n_sorted, n_pairs_padded):
    out = (ctypes.c_int32 * 8)()
    rc = lib.gcl_conv_bwd_weight_launch_shape(K, ca, cb, PREC_CODE.get(prec, prec), planes, side, n_sorted, n_pairs_padded, out)
    assert rc == 0, (K, ca, cb, prec, planes, side, n_sorted, n_pairs_padded)
    return dict(zip(("path", "ta", "tb", "W", "per", "stiles", "rr", "nr"), out))


def case_shape(lib, case, side=None, planes=None):
    lname, ca, cb, prec, pl = case[:5]
    L = pair_list(lname)
    side = L.side if side is None else side
    return launch_shape(lib, L.K, ca, cb, prec, pl if planes is None else planes, side, L.n_sorted(side), int(L.seg[-1]))


def instance_of(s, prec):
    """Name of the kernel instance of a launch shape (gcl_conv_bwd_weight_rg in csrc/conv.hip)."""
    t, pl = f"{s['ta']},{s['tb']}", {"f32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 4}[prec]
    return {NONE: NO_PAIRS, GENERIC: "k_conv_bwd_weight_generic", F32: f"k_conv_bwd_weight<{t}>",
            SPLIT: f"k_conv_bwd_weight_split<{t},{pl},false,false>", PLANES: f"k_conv_bwd_weight_split<{t},4,true,false>",
            RG: f"k_conv_bwd_weight_split<{t},{pl},false,true>", WG128: "k_conv_bwd_weight_wg128<false>"}[s["path"]]


def full_instance_matrix():
    tiles = [f"{a},{b}" for a in (32, 64) for b in (32, 64)]
    m = {f"k_conv_bwd_weight<{t}>" for t in tiles}
    m |= {f"k_conv_bwd_weight_split<{t},{pl},false,false>" for t in tiles for pl in (2, 3, 4)}
    m |= {f"k_conv_bwd_weight_split<{t},4,true,false>" for t in tiles}
    m |= {f"k_conv_bwd_weight_split<{t},{pl},false,true>" for t in tiles for pl in (2, 3, 4)}
    m |= {"k_conv_bwd_weight_wg128<false>"}
    return m


# ---------------------------------------------------------------------------------------------------------------
# without a GPU: the table names the instances and launch shapes it reaches, and reaches all of them
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_names_its_kernel_instances_and_holds_every_launch_shape_edge():
    """gcl_conv_bwd_weight_launch_shape is host arithmetic, and it is what the dispatcher launches: every case's instance, W,
    per, rr and n_ranges are the ones it claims, the reached instances are exactly the 33 of the dispatcher plus the generic
    kernel, every launch-shape edge is in the table (derived from the returned numbers and the lists, not from comments),
    and the band edges of dw_rg_shape, dw_range_rows, bwd_weight_wgs and the tile choice are where the table assumes them."""
    from gcl_amd import _lib
    lib = _lib.load()
    reached, edges, rg_seen = {}, set(), {}
    for case in CASES:
        lname, ca, cb, prec, pl, name, W, per, rr, nr = case
        L, s = pair_list(lname), case_shape(lib, case)
        assert (instance_of(s, prec), s["W"], s["per"], s["rr"], s["nr"]) == (name, W, per, rr, nr), (case_id(case), s)
        reached[name] = reached.get(name, 0) + 1
        nz = np.nonzero(L.counts)[0]
        mfma = s["path"] in (F32, SPLIT, PLANES, WG128)
        tiles = (ca // s["ta"]) * (cb // s["tb"]) if mfma else 0
        assert s["stiles"] in (0, tiles) and (s["stiles"] == 0) == (tiles <= 1 or s["path"] == F32), (case_id(case), s)
        first_chunk, last_chunk = L.seg[:-1][nz] // CHUNK, L.seg[1:][nz] // CHUNK - 1
        wgs_of = {int(k): (int(f) // per, int(l) // per) for k, f, l in zip(nz, first_chunk, last_chunk)}
        if mfma and W == 1 and L.K == 27 and len(nz) > 8:
            edges.add("one workgroup, several offsets")
            edges.add(f"one workgroup, several offsets: {name.split('<')[0]}")
        if s["path"] != NONE and len(nz) and L.counts[0] == 0 and L.counts[-1] == 0 and \
                any(L.counts[k] == 0 and L.counts[k + 1] == 0 and nz[0] < k < nz[-1] - 1 for k in range(L.K - 1)):
            edges.add(f"empty first, last, two in a row: path {s['path']}")
        if mfma and (L.counts == 1).any() and L.nc > 1:
            edges.add("one-pair segment")
        if s["path"] == WG128 and L.counts.sum() == 1:
            edges.add("wg128: one-pair list")
        if mfma and W == 512 and per == 9 and L.nc > 4096 and 0 < L.nc - (-(-L.nc // per) - 1) * per < per and W * per > L.nc:
            edges.add("cap of 512 workgroups, last one short")
        if s["stiles"] > 1 and W % 8 and W > 1 and (ca, cb) == (128, 64):
            edges.add(f"idle workgroups of the swizzled grid: path {s['path']}")
        if s["stiles"] > 1 and W % 8 and s["path"] == WG128:
            edges.add("idle workgroups of the swizzled grid: wg128")
        if mfma and L.K == 125:
            edges.add(f"K = 125: path {s['path']}")
            assert lib.gcl_conv_bwd_weight_scratch_len(125, ca, cb, int(L.seg[-1]), L.n_sorted()) == (W + 125) * ca * cb
        if mfma and any(hi - lo >= 2 for lo, hi in wgs_of.values()):
            edges.add("an offset over three or more workgroups")
        if s["path"] == GENERIC and L.K == 125 and (L.counts == 0).any():
            edges.add(f"generic {ca} x {cb}")
        if ca % 32 or cb % 32:          # fp64 slabs, aligned inside the float scratch
            assert lib.gcl_conv_bwd_weight_scratch_len(L.K, ca, cb, int(L.seg[-1]), L.n_sorted()) == 2 * (W + L.K) * ca * cb + 2
        if s["path"] == NONE:
            assert L.nc == 0
            edges.add(f"no pairs: {'generic' if ca % 32 else ('planes' if pl else 'rows')}")
        if s["path"] == RG:
            assert L.n_sorted() >= 32768 and 1 < L.K <= 27 and nr == -(-L.n_sorted() // rr)
            # the same lists with sorted_side = 0 go down the classic path (the comparison launch of the GPU test)
            assert case_shape(lib, case, side=0)["path"] == SPLIT
            lim = L.cells(rr, nr)
            size = np.diff(lim, axis=1)
            allr = np.concatenate(L.sorted)
            f = rg_seen.setdefault(lname, set())
            f.add(f"rr {rr}")
            f.add(f"side {L.side}")
            if nr % 8:
                f.add("n_ranges no multiple of 8")
            if (size[nz] == 0).any() and (size[L.counts == 0] == 0).all() and (L.counts == 0).any():
                f.add("empty cells")
            if ((size > CHUNK) & (size % CHUNK != 0)).any() and (lim[:, :-1][size > 0] % CHUNK != 0).any():
                f.add("ragged cells")
            if any(((allr == j * rr).any() and (allr == j * rr - 1).any()) for j in range(1, nr)):
                f.add("boundary rows")
            assert lib.gcl_conv_bwd_weight_bounds_len(L.K, L.n_sorted()) == L.K * (nr + 1)
            mat = ca * cb
            assert lib.gcl_conv_bwd_weight_scratch_len(L.K, ca, cb, int(L.seg[-1]), L.n_sorted()) == \
                max(nr * L.K * mat + L.K * (nr + 1) + 64, (W + L.K) * mat)
        elif mfma:
            assert lib.gcl_conv_bwd_weight_scratch_len(L.K, ca, cb, int(L.seg[-1]), L.n_sorted()) == (W + L.K) * ca * cb
    matrix = full_instance_matrix()
    assert len(matrix) == 33
    assert set(reached) == matrix | {"k_conv_bwd_weight_generic", NO_PAIRS}, \
        (sorted(matrix - set(reached)), sorted(set(reached) - matrix))
    want_edges = {"one workgroup, several offsets", "one-pair segment", "cap of 512 workgroups, last one short",
                  "wg128: one-pair list", "idle workgroups of the swizzled grid: wg128", "an offset over three or more workgroups",
                  "generic 1 x 1", "generic 17 x 33", "generic 30 x 7", "no pairs: generic", "no pairs: planes", "no pairs: rows"}
    want_edges |= {f"one workgroup, several offsets: {k}" for k in ("k_conv_bwd_weight", "k_conv_bwd_weight_split",
                                                                      "k_conv_bwd_weight_wg128")}
    want_edges |= {f"empty first, last, two in a row: path {p}" for p in (GENERIC, F32, SPLIT, PLANES, RG, WG128)}
    want_edges |= {f"idle workgroups of the swizzled grid: path {p}" for p in (SPLIT, PLANES)}
    want_edges |= {f"K = 125: path {p}" for p in (F32, SPLIT, PLANES, WG128)}
    assert edges == want_edges, (sorted(want_edges - edges), sorted(edges - want_edges))
    per_list = {"n_ranges no multiple of 8", "empty cells", "ragged cells", "boundary rows"}
    assert {k: v for k, v in rg_seen.items()} == {
        "R512": per_list | {"rr 512", "side 2"}, "R1024": per_list | {"rr 1024", "side 2"},
        "R2048": per_list | {"rr 2048", "side 2"}, "R4096": per_list | {"rr 4096", "side 1"}}, rg_seen

    # ---- band edges.  dw_rg_shape: the 32768-row threshold and every other condition of the RG mode
    def shape(K=27, ca=64, cb=64, prec=4, planes=0, side=2, n=40000, nc=300):
        return launch_shape(lib, K, ca, cb, prec, planes, side, n, nc * CHUNK)
    assert shape(n=32767)["path"] == SPLIT and shape(n=32768)["path"] == RG
    assert shape(side=1)["path"] == RG and shape(side=0)["path"] == SPLIT
    assert shape(K=1)["path"] == SPLIT and shape(K=2, n=2 ** 20)["path"] == RG and shape(K=28)["path"] == SPLIT
    assert shape(prec=0)["path"] == F32 and shape(prec=2)["path"] == RG and shape(prec=3)["path"] == RG
    assert shape(planes=1)["path"] == PLANES and shape(nc=0)["path"] == NONE
    for ca, cb, rg in [(32, 32, True), (32, 64, True), (64, 32, True), (96, 64, False), (64, 128, False), (128, 128, False)]:
        s = shape(ca=ca, cb=cb)
        assert (s["path"] == RG) == rg and (not rg or (s["ta"], s["tb"]) == (ca, cb)), (ca, cb, s)
    # dw_range_rows: a power of two in [512, 4096], doubling where n K / 2048 reaches twice the range (K = 27, 2, 5)
    for K, n, rr in [(27, 32768, 512), (27, 77672, 512), (27, 77673, 1024), (27, 155344, 1024), (27, 155345, 2048),
                     (27, 310689, 2048), (27, 310690, 4096), (27, 10 ** 7, 4096), (2, 2 ** 20 - 1, 512), (2, 2 ** 20, 1024),
                     (2, 2 ** 22 - 1, 2048), (2, 2 ** 22, 4096), (5, 419430, 512), (5, 419431, 1024)]:
        s = shape(K=K, n=n, ca=32, cb=32)
        assert (s["path"], s["rr"], s["nr"]) == (RG, rr, -(-n // rr)), (K, n, s)
        assert lib.gcl_conv_bwd_weight_bounds_len(K, n) == K * (-(-n // rr) + 1)
    assert lib.gcl_conv_bwd_weight_bounds_len(27, 32767) == 0 and lib.gcl_conv_bwd_weight_bounds_len(1, 40000) == 0
    assert lib.gcl_conv_bwd_weight_bounds_len(28, 40000) == 0
    # bwd_weight_wgs: nc / 8 workgroups, at least 1, at most 512; per = ceil(nc / W)
    for nc, W, per in [(1, 1, 1), (7, 1, 7), (15, 1, 15), (16, 2, 8), (23, 2, 12), (24, 3, 8), (107, 13, 9), (4095, 511, 9),
                       (4096, 512, 8), (4097, 512, 9), (4103, 512, 9), (4608, 512, 9), (4609, 512, 10), (10 ** 6, 512, 1954)]:
        for kw in (dict(n=100), dict(prec=0, n=100), dict(ca=128, cb=128, planes=1, n=100), dict(ca=17, cb=5, prec=0, n=100),
                   dict()):
            s = shape(nc=nc, **kw)
            assert (s["W"], s["per"]) == (W, per), (nc, kw, s)
    # the tile choice: 64 wide where the channel count is a multiple of 64, else 32; 128 x 128 on planes of multiples of 128
    for prec, planes, path in [(0, 0, F32), (2, 0, SPLIT), (3, 0, SPLIT), (4, 0, SPLIT), (4, 1, PLANES), (4, 3, PLANES)]:
        for ca in (32, 64, 96, 128, 160, 192, 256):
            for cb in (32, 64, 96, 128, 160, 256):
                s = shape(ca=ca, cb=cb, prec=prec, planes=planes, n=100)
                if planes == 1 and ca % 128 == 0 and cb % 128 == 0:
                    assert (s["path"], s["ta"], s["tb"]) == (WG128, 128, 128), (ca, cb, s)
                    tiles = (ca // 128) * (cb // 128)
                else:
                    assert (s["path"], s["ta"], s["tb"]) == (path, 64 if ca % 64 == 0 else 32, 64 if cb % 64 == 0 else 32), \
                        (prec, planes, ca, cb, s)
                    tiles = (ca // s["ta"]) * (cb // s["tb"])
                assert s["stiles"] == (tiles if tiles > 1 and prec != 0 else 0)
    for ca, cb in [(1, 1), (17, 33), (30, 7), (32, 48), (31, 64)]:
        s = shape(ca=ca, cb=cb, n=100)
        assert (s["path"], s["ta"], s["tb"], s["stiles"]) == (GENERIC, 16, 16, 0)
    # arguments the entry itself refuses
    out = (ctypes.c_int32 * 8)()
    assert lib.gcl_conv_bwd_weight_launch_shape(27, 64, 64, 2, 1, 2, 100, 1280, out) != 0           # planes are fp16x3
    assert lib.gcl_conv_bwd_weight_launch_shape(126, 64, 64, 4, 0, 2, 100, 1280, out) != 0
    assert lib.gcl_conv_bwd_weight_launch_shape(27, 64, 64, 4, 0, 2, 100, 1281, out) != 0           # padded to chunks
    assert lib.gcl_conv_bwd_weight_launch_shape(27, 64, 64, 4, 0, 2, 100, 1280, None) != 0


# ---------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC5A5A5          # a quiet NaN (tests/test_gpu_conv_instances.py): inside found by isfinite, outside by its bits
GUARD = 4096                   # guard words on either side, or two slabs where those are larger


class Guarded:
    """`numel` 32-bit words inside a larger sentinel-filled allocation; the words themselves start as `fill`."""

    def __init__(self, numel, guard, fill=SENTINEL, dtype=torch.float32):
        self.buf = torch.full((guard + numel + guard,), SENTINEL, dtype=torch.int32, device=DEV)
        self.guard, self.numel = guard, numel
        self.buf[guard:guard + numel] = fill
        self.t = self.buf[guard:guard + numel].view(dtype)

    def intact(self):
        return bool((self.buf[:self.guard] == SENTINEL).all()) and bool((self.buf[self.guard + self.numel:] == SENTINEL).all())


def rel_l2_per_offset(got, want):
    """[K] relative L2 errors of got[k] against want[k] (fp64); 0 where both are zero."""
    g, w = got.double().flatten(1), want.double().flatten(1)
    return (g - w).norm(dim=1) / w.norm(dim=1).clamp_min(1e-300)


def where_differs(a, b):
    bad = torch.nonzero(~((a == b) | (a.isnan() & b.isnan())))
    if len(bad) == 0:
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at (k, row, column) {i}: {float(a[i])!r} != {float(b[i])!r}"


_PROBLEMS = {}


class Problem:
    """One (pair list, Ca, Cb): the operands (A Gaussian, B Gaussian x 3e-3: the scale of a gradient), their amax slots and
    plane images, and the fp64 product of every offset over its real pairs; shared by every arithmetic that runs it."""

    def __init__(self, lname, ca, cb):
        from gcl_amd import _lib
        import gcl_amd.MinkowskiEngine as ME
        self.lib = lib = _lib.require_gpu()
        self.L = L = pair_list(lname)
        self.ca, self.cb, self.K, self.mat = ca, cb, L.K, ca * cb
        g = torch.Generator().manual_seed(L.nc + 7 * ca + 13 * cb + L.n_a)
        with torch.cuda.device(DEV):
            self.a = torch.randn(L.n_a, ca, generator=g).to(DEV)
            self.b = (torch.randn(L.n_b, cb, generator=g) * 3e-3).to(DEV)
            self.aa, self.ba = ME.ops.amax_slot(self.a.device), ME.ops.amax_slot(self.a.device)
            _lib.check(lib.gcl_amax(_lib.ptr(self.a), self.a.numel(), _lib.ptr(self.aa), 1, _lib.stream()), "gcl_amax")
            _lib.check(lib.gcl_amax(_lib.ptr(self.b), self.b.numel(), _lib.ptr(self.ba), 1, _lib.stream()), "gcl_amax")
        # one spare word behind the lists keeps a zero-length list a valid pointer
        self.pa = torch.from_numpy(np.append(L.pair_a, np.int32(-1))).to(DEV)
        self.pb = torch.from_numpy(np.append(L.pair_b, np.int32(-1))).to(DEV)
        self.seg_host = _lib.host_i64(L.seg)
        self._planes = None
        self.ref = torch.zeros(L.K, ca, cb, dtype=torch.float64, device=DEV)
        for k in np.nonzero(L.counts)[0]:
            ia, ib = torch.from_numpy(L.real_a[k]).to(DEV), torch.from_numpy(L.real_b[k]).to(DEV)
            self.ref[k] = self.a[ia].double().T @ self.b[ib].double()
        self.empty = torch.from_numpy(L.counts == 0).to(DEV)

    def planes(self):
        from gcl_amd import _lib
        if self._planes is None:
            with torch.cuda.device(DEV):
                xa = torch.empty((self.L.n_a, self.ca), dtype=torch.int32, device=DEV)
                xb = torch.empty((self.L.n_b, self.cb), dtype=torch.int32, device=DEV)
                _lib.check(self.lib.gcl_split_planes(_lib.ptr(self.a), self.L.n_a, self.ca, _lib.ptr(self.aa), _lib.ptr(xa),
                                                     _lib.stream()), "gcl_split_planes")
                _lib.check(self.lib.gcl_split_planes(_lib.ptr(self.b), self.L.n_b, self.cb, _lib.ptr(self.ba), _lib.ptr(xb),
                                                     _lib.stream()), "gcl_split_planes")
            self._planes = (xa, xb)
        return self._planes

    def fp32_product(self, k):
        """The fp32 torch product of one offset (what a failure message sets the kernel's error against)."""
        ia, ib = torch.from_numpy(self.L.real_a[k]).to(DEV), torch.from_numpy(self.L.real_b[k]).to(DEV)
        return self.a[ia].T @ self.b[ib]

    def run(self, prec, planes, side, fill=SENTINEL, bounds=None, entry="rg"):
        """One launch into guarded dW and guarded scratch of exactly the advertised length; returns dW [K, Ca, Cb]."""
        from gcl_amd import _lib
        lib, L = self.lib, self.L
        guard = max(GUARD, 2 * self.mat)
        ln = lib.gcl_conv_bwd_weight_scratch_len(L.K, self.ca, self.cb, int(L.seg[-1]), L.n_sorted(side))
        assert ln >= (1 + L.K) * self.mat
        scratch, dw = Guarded(ln, guard, fill), Guarded(L.K * self.mat, guard)
        xa, xb = self.planes() if planes & 1 else (self.a, self.b)
        args = (_lib.ptr(xa), L.n_a, _lib.ptr(xb), L.n_b, planes, side, _lib.ptr(self.pa), _lib.ptr(self.pb), self.seg_host,
                L.K, self.ca, self.cb, PREC_CODE[prec], _lib.ptr(self.aa), _lib.ptr(self.ba), _lib.ptr(scratch.t),
                _lib.ptr(dw.t))
        with torch.cuda.device(DEV):
            if entry == "rg":
                _lib.check(lib.gcl_conv_bwd_weight_rg(*args, _lib.ptr(bounds) if bounds is not None else None, _lib.stream()),
                           "gcl_conv_bwd_weight_rg")
            else:
                assert bounds is None
                _lib.check(lib.gcl_conv_bwd_weight(*args, _lib.stream()), "gcl_conv_bwd_weight")
        torch.cuda.synchronize()
        assert scratch.intact(), "the launch wrote outside scratch[gcl_conv_bwd_weight_scratch_len]"
        assert dw.intact(), "the launch wrote outside dW"
        return dw.t.view(L.K, self.ca, self.cb)


def problem(lname, ca, cb):
    key = (lname, ca, cb)
    if key not in _PROBLEMS:      # 33 problems, about 100 MB in all (mostly the sorted operands of the four RG lists)
        _PROBLEMS[key] = Problem(*key)
    return _PROBLEMS[key]


_T0, _WORST = [], {}


def check_against_fp64(p, dw, prec, name, what):
    """Every offset of dw on its own, and the whole tensor, against the fp64 product at PREC_TOL[prec]; offsets without pairs
    exactly +0.0.  Returns the largest per-offset error."""
    tol = PREC_TOL[prec]
    assert bool(torch.isfinite(dw).all()), f"{name} ({what}): {int((~torch.isfinite(dw)).sum())} elements of dW are not " \
        f"finite (an unwritten slab or element), first offsets {torch.nonzero(~torch.isfinite(dw).flatten(1).all(1))[:5, 0].tolist()}"
    zeros = dw.view(torch.int32)[p.empty]
    assert bool((zeros == 0).all()), f"{name} ({what}): an offset without pairs is not exactly +0.0"
    if bool(p.empty.all()):
        return 0.0
    err = rel_l2_per_offset(dw, p.ref)
    err[p.empty] = 0.0
    k = int(err.argmax())
    worst = float(err[k])
    whole = float((dw.double() - p.ref).norm() / p.ref.norm())
    if not (worst < tol and whole < tol):
        over = torch.nonzero(err >= tol)[:, 0].tolist() or [k]
        f32 = {j: float(rel_l2_per_offset(p.fp32_product(j)[None], p.ref[j][None])[0]) for j in over[:16]}
        raise AssertionError(f"{name} ({what}): whole tensor {whole:.3e}, bound {tol:.1e}; (offset, pairs, rel-L2 against fp64, the "
                             f"same of torch's fp32 product of that offset) over the bound: "
                             + ", ".join(f"({j}, {int(p.L.counts[j])}, {float(err[j]):.3e}, {f32[j]:.3e})" for j in over[:16]))
    return worst


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_bwd_weight_instance(case):
    """All checks of one case; see the module docstring.  A failure names the instance, the offset and the launch.

    Measured on an MI355X, largest per-offset rel-L2 against fp64 over all cases: fp16x3 3.3e-7, bf16x6 2.2e-7, exact f32
    3.5e-7, the generic kernel 5.1e-8 (bounds 2e-6), bf16x3 4.6e-6 (bound 3e-5).

    The generic kernel keeps fp64 accumulators and slabs: with Ca = Cb = 1 (case Q-1-1) dW[k] is ONE number, the sum of some
    hundred products of either sign, and fp32 accumulation missed the bound there on six of 105 offsets (worst 2.19e-4 on 302
    pairs, the same as torch's own fp32 product a[pa_k].T @ b[pb_k] of that offset)."""
    from gcl_amd import _lib
    from conftest import precision_log_path
    lname, ca, cb, prec, pl, name, W, per, rr, nr = case
    if not _T0:
        _T0.append(time.time())
    lib = _lib.require_gpu()
    p = problem(lname, ca, cb)
    L = p.L
    s = case_shape(lib, case)
    assert (instance_of(s, prec), s["W"], s["per"], s["rr"], s["nr"]) == (name, W, per, rr, nr), s
    arith = "f32" if s["path"] in (GENERIC, NONE) and ca % 32 else prec        # the generic kernel is exact fp32

    # sentinel scratch, twice (once through each entry), and zeroed scratch: bit for bit
    dw = p.run(prec, pl, L.side)
    worst = check_against_fp64(p, dw, arith, name, "first launch")
    again = p.run(prec, pl, L.side, entry="plain")
    assert torch.equal(dw, again), f"{name}: two launches differ: {where_differs(dw, again)}"
    zeroed = p.run(prec, pl, L.side, fill=0)
    assert torch.equal(dw, zeroed), f"{name}: sentinel scratch against zeroed scratch: {where_differs(dw, zeroed)}"
    if s["path"] == NONE:
        assert bool((dw.view(torch.int32) == 0).all())

    if s["path"] == WG128:          # bit 1 of `planes`: the 64 x 64-block kernel on the same plane images
        other = instance_of(case_shape(lib, case, planes=3), prec)
        assert other == "k_conv_bwd_weight_split<64,64,4,true,false>"
        legacy = p.run(prec, 3, L.side)
        worst = max(worst, check_against_fp64(p, legacy, arith, other, "bit 1 of planes"))
        d = rel_l2_per_offset(dw, legacy)
        assert bool((d < PREC_TOL[prec]).all()), (name, "against the 64 x 64-block kernel", float(d.max()))

    if s["path"] == RG:
        # the cell limits: integers, exactly, in a guarded buffer of exactly bounds_len words
        blen = lib.gcl_conv_bwd_weight_bounds_len(L.K, L.n_sorted())
        assert blen == L.K * (nr + 1)
        bounds = Guarded(blen, GUARD, dtype=torch.int32)
        srt = p.pa if L.side == 1 else p.pb
        with torch.cuda.device(DEV):
            _lib.check(lib.gcl_conv_bwd_weight_bounds(_lib.ptr(srt), p.seg_host, L.K, L.n_sorted(), _lib.ptr(bounds.t),
                                                      _lib.stream()), "gcl_conv_bwd_weight_bounds")
        torch.cuda.synchronize()
        assert bounds.intact(), "gcl_conv_bwd_weight_bounds wrote outside bounds[gcl_conv_bwd_weight_bounds_len]"
        got, want = bounds.t.cpu().numpy().reshape(L.K, nr + 1), L.cells(rr, nr)
        assert np.array_equal(got, want), (name, "cell limits (offset, range)", np.argwhere(got != want)[:5].tolist())
        pre = p.run(prec, pl, L.side, bounds=bounds.t)
        assert torch.equal(dw, pre), f"{name}: prebuilt bounds against bounds made per launch: {where_differs(dw, pre)}"
        assert bounds.intact()
        # the classic k-major launch of the same lists
        cname = instance_of(case_shape(lib, case, side=0), prec)
        assert cname == name.replace("false,true", "false,false")
        classic = p.run(prec, pl, 0)
        worst = max(worst, check_against_fp64(p, classic, arith, cname, "sorted_side = 0"))
        d = rel_l2_per_offset(dw, classic)
        d[p.empty] = 0.0
        assert bool((d < PREC_TOL[prec]).all()), (name, "against the classic launch", float(d.max()))
        assert float((dw.double() - classic.double()).norm() / classic.double().norm()) < PREC_TOL[prec]

    _WORST[arith] = max(_WORST.get(arith, 0.0), worst)
    print(f"[dw instance] {name} {lname} {ca}x{cb} {prec} W={W} per={per} rr={rr} nr={nr}: worst offset rel-L2 vs fp64 "
          f"{worst:.3e}")
    with open(precision_log_path(), "a") as fh:
        fh.write(f"dw_instance {name} list={lname} {ca}x{cb} {prec} W={W} per={per} rr={rr} nr={nr} "
                 f"worst_offset_rel_l2={worst:.4e}\n")
    if case is CASES[-1]:
        print(f"[dw instance] {len(CASES)} cases in {time.time() - _T0[0]:.1f} s; largest per-offset error per arithmetic: "
              + ", ".join(f"{k} {v:.3e}" for k, v in sorted(_WORST.items())))
