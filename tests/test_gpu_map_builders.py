"""Every launch shape of the map builders (csrc/coords.hip, maps_build of csrc/plan.hip), called directly through the C ABI,
against the numpy references of tests/map_scenes.py.

All of it is integer work: every comparison in this file is EXACT.  Outputs live inside sentinel-filled allocations whose guard
words must survive the call, scratch is pre-filled with the sentinel (nothing may depend on what it held), and every launch runs
twice with fresh buffers, the two results compared bit for bit.  The cases come from the tables of map_scenes.py, which
tests/test_oracle_maps.py pins to gcl_map_launch_shape; the scene conditions they rely on (exact row counts, segment lengths,
wrapping probe chains, presence-bitmap false positives) are asserted there, without a GPU."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/map_scenes.py
import map_scenes as S                                                 # noqa: E402

DEV = "cuda:0"
SENT = -0x5A5A5A5B          # sentinel of outputs, scratch and guards
GUARD = 64                  # guard elements on either side of an output (64 x 4 bytes keeps the 16-byte alignment of rows)
I32, I64 = torch.int32, torch.int64
LLONG_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def lib():
    from gcl_amd import _lib
    return _lib.require_gpu()


def P(t):
    from gcl_amd import _lib
    return _lib.ptr(t.t if isinstance(t, Guarded) else t)


def STREAM():
    from gcl_amd import _lib
    return _lib.stream()


def ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.gcl_last_error())


class Guarded:
    """A tensor inside a larger sentinel-filled allocation."""

    def __init__(self, shape, dtype=I32, fill=SENT):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if fill != SENT:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def np(self):
        return self.t.cpu().numpy()


def dev(a, dtype=I32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def read_table(table):
    """(keys uint64, vals int64) of the used slots of a table read back, sorted by key; every unused slot must be untouched."""
    t = table.np()
    keys, vals = t[:, 0].view(np.uint64), t[:, 1]
    used = keys != S.EMPTY_KEY
    assert (vals[~used] == LLONG_MAX).all()
    o = np.argsort(keys[used])
    return keys[used][o], vals[used][o]


def insert(lib, C, cap=None):
    """gcl_coords_insert of the rows C -> (table, status)."""
    n = len(C)
    cap = cap or S.pow2_cap(n)
    table, status, Cd = Guarded((cap, 2), I64), Guarded(4), dev(C)
    ok(lib, lib.gcl_coords_insert(P(Cd), n, P(table), cap, P(status), STREAM()), "gcl_coords_insert")
    torch.cuda.synchronize()
    assert table.intact() and status.intact()
    return table, status


def identity_lookup(lib, coords, n, table, cap):
    """gcl_kernel_map with ks = 1, same_map = 0 on a level's own coordinates: rows 0 .. n - 1, counts[0] = n."""
    nbr, counts, scratch = Guarded((1, n)), Guarded(1), Guarded(lib.gcl_kernel_map_scratch_len(1, n))
    ok(lib, lib.gcl_kernel_map(P(coords), n, P(table), cap, 1, 1, 0, None, P(scratch), P(nbr), None, n, P(counts), STREAM()),
       "gcl_kernel_map ks=1")
    torch.cuda.synchronize()
    assert nbr.intact() and counts.intact() and scratch.intact()
    assert np.array_equal(nbr.np()[0], np.arange(n)) and counts.np().tolist() == [n]


# ---------------------------------------------------------------------------------------------------------------
# gcl_coords_insert
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(S.STRIDE_ROWS))
def test_coords_insert_table_and_status(lib, n):
    """Rows with duplicates and rows outside the packable range at cap = pow2 >= 2 n (cap == 2 n at the powers of two): status =
    exact counts, the table's keys = the packable voxels, each with the row of its FIRST occurrence."""
    C = S.stride_scene(n, 1)
    bad, dup = S.insert_status(C)
    want_rows, want_first, _ = S.stride_level(C, 1)
    results = []
    for _ in range(2):
        table, status = insert(lib, C)
        assert status.np().tolist() == [bad, dup, 0, 0]
        keys, vals = read_table(table)
        o = np.argsort(S.pack_key(want_rows))
        assert np.array_equal(keys, S.pack_key(want_rows)[o]) and np.array_equal(vals, want_first[o])
        results.append((keys, vals))
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    if n >= 255:
        assert bad == 3 and dup > 0


# ---------------------------------------------------------------------------------------------------------------
# gcl_stride_map / gcl_unique_coords
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def _stride_scene(n_in, t_out):
    return S.stride_scene(n_in, t_out)


def stride_call(lib, C, n_in, n_dev, t_out, unique=False):
    """One gcl_stride_map (gcl_unique_coords) call on rows C[:n_in]; n_dev None = NULL.  Returns the guarded outputs."""
    cap = S.pow2_cap(n_in)
    Cd = dev(C[:n_in])
    out = dict(table=Guarded((cap, 2), I64), scratch=Guarded(lib.gcl_scan_scratch_len(n_in)), coords=Guarded((n_in, 4)),
               n_out=Guarded(1), status=Guarded(4), cap=cap)
    if unique:
        out["index"] = Guarded(n_in, I64)
        ok(lib, lib.gcl_unique_coords(P(Cd), n_in, P(out["table"]), cap, P(out["scratch"]), P(out["coords"]), P(out["index"]),
                                      P(out["n_out"]), P(out["status"]), STREAM()), "gcl_unique_coords")
    else:
        nd = None if n_dev is None else dev(np.asarray([n_dev]))
        ok(lib, lib.gcl_stride_map(P(Cd), n_in, P(nd), t_out, P(out["table"]), cap, P(out["scratch"]), P(out["coords"]),
                                   P(out["n_out"]), P(out["status"]), STREAM()), "gcl_stride_map")
    torch.cuda.synchronize()
    for k, g in out.items():
        assert k == "cap" or g.intact(), k
    return out


def check_level(lib, out, want, functional=True):
    """One call's outputs against (coords, first rows, bad rows) of the reference; rows past n_out must be untouched."""
    rows, first, bad = want
    m = len(rows)
    assert out["n_out"].np().tolist() == [m]
    assert out["status"].np().tolist() == [bad, 0, 0, 0]
    got = out["coords"].np()
    assert np.array_equal(got[:m], rows) and (got[m:] == SENT).all()
    if "index" in out:
        idx = out["index"].np()
        assert np.array_equal(idx[:m], first) and (idx[m:] == SENT).all()
    keys, vals = read_table(out["table"])
    o = np.argsort(S.pack_key(rows))
    assert np.array_equal(keys, S.pack_key(rows)[o]) and np.array_equal(vals, o)          # a voxel's value = its output row
    if functional:
        identity_lookup(lib, out["coords"].t, m, out["table"], out["cap"])
    return got, keys, vals


@pytest.mark.parametrize("t_out", S.STRIDE_T_OUT)
@pytest.mark.parametrize("n_in", sorted(S.STRIDE_ROWS))
def test_stride_map_every_form_and_row_bound(lib, n_in, t_out):
    """Short form (up to 256 scan blocks, the last shape included) and long form, with the row bound on the host (NULL), on the
    device and equal to n_in, on the device and below n_in with duplicates and bad rows in the tail, and n_dev = 1."""
    C = _stride_scene(n_in, t_out)
    ways = [("null", None, C), ("equal", n_in, C), ("one", 1, S.garbage_tail(C, 1))]
    if n_in >= 2:
        n_dev = n_in - max(1, n_in // 3)
        ways.append(("below", n_dev, S.garbage_tail(C, n_dev)))
    for way, n_dev, rows in ways:
        n_valid = n_in if n_dev is None else n_dev
        want = S.stride_level(rows[:n_valid], t_out)
        runs = [check_level(lib, stride_call(lib, rows, n_in, n_dev, t_out), want, functional=(r == 0)) for r in range(2)]
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), way
        if way == "below":      # == the call on the first n_dev rows alone
            alone = check_level(lib, stride_call(lib, rows, n_dev, None, t_out), want, functional=False)
            assert np.array_equal(alone[0][:len(want[0])], runs[0][0][:len(want[0])])
    if t_out == 1:
        want = S.stride_level(C, 1)
        runs = [check_level(lib, stride_call(lib, C, n_in, None, 1, unique=True), want, functional=(r == 0)) for r in range(2)]
        assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_hash_table_at_its_limits(lib):
    """n = 32 rows in 64 slots, ten of them with their home in the last four slots: the cluster wraps from slot 63 to slot 0.
    Insert, strided levels, and lookups (absent neighbours probe through the cluster) with and without the bitmap."""
    C = S.hash_stress()
    table, status = insert(lib, C, cap=64)
    assert status.np().tolist() == [0, 0, 0, 0]
    keys, vals = read_table(table)
    o = np.argsort(S.pack_key(C))
    assert np.array_equal(keys, S.pack_key(C)[o]) and np.array_equal(vals, o)
    slots = np.nonzero(table.np()[:, 0].view(np.uint64) != S.EMPTY_KEY)[0]
    assert set(slots.tolist()) == set(S.simulate_probes(C, 64)[0].tolist()) and {63, 0} <= set(slots.tolist())      # it wrapped
    for ks in (1, 3, 5):
        kernel_map_variants(lib, C, C, table, 64, ks, 1, 1 if ks > 1 else 0)
    for t_out in (1, 2, 4):
        check_level(lib, stride_call(lib, C, 32, None, t_out), S.stride_level(C, t_out))
    check_level(lib, stride_call(lib, C, 32, None, 1, unique=True), S.stride_level(C, 1))


def test_ends_of_the_packable_range(lib):
    """Rows at -32768 and 32767 on every axis, batch 65534: they pack, their outer neighbours do not exist; rows one step
    outside are counted and dropped."""
    ends, outside = S.range_ends()
    mixed = np.concatenate([ends[:7], outside[:4], ends[7:], outside[4:], ends[:3]])
    _, status = insert(lib, mixed)
    assert status.np().tolist() == [len(outside), 3, 0, 0]
    for t_out in (1, 2, 8):
        check_level(lib, stride_call(lib, mixed, len(mixed), None, t_out), S.stride_level(mixed, t_out))
    table, status = insert(lib, ends)
    assert status.np().tolist() == [0, 0, 0, 0]
    for ks, step in ((3, 1), (5, 1), (3, 4), (1, 1)):
        kernel_map_variants(lib, ends, ends, table, S.pow2_cap(len(ends)), ks, step, 1 if ks > 1 else 0)
    lvl = S.stride_level(ends, 2)[0]                                                       # a stride-2 map at the ends
    kernel_map_variants(lib, ends, lvl, table, S.pow2_cap(len(ends)), 3, 1, 0)


# ---------------------------------------------------------------------------------------------------------------
# gcl_kernel_map
# ---------------------------------------------------------------------------------------------------------------
def kernel_map_variants(lib, C_in, C_out, table, cap, ks, step, same, full=True):
    """Every flag variant of one kernel map -- counts by atomics (bit 2) on / off, the caller's -1 fill (bit 3) on / off, no
    bitmap / a fresh one / one reused with bit 1 -- against the reference, twice each; all of them bit for bit the same."""
    K, n_in, n_out = ks ** 3, len(C_in), len(C_out)
    want = S.kernel_map(C_in, C_out, ks, step)
    want_t = None if same else S.transpose_table(want, n_in)
    want_d, want_td, want_c = dev(want), None if same else dev(want_t), dev(S.offset_counts(want))
    Cd = dev(C_out)
    filled = None                    # a bitmap some earlier variant built for THIS table
    variants = [(acc, pre, bm) for acc in (0, 4) for pre in (0, 8) for bm in ("none", "fresh", "reused")]
    if not full:
        variants = [(0, 0, "none"), (4, 0, "fresh"), (0, 8, "reused"), (4, 8, "none")]
    for acc, pre, bm in variants:
        for run in range(2):
            bitmap = None
            if bm == "fresh":
                bitmap = Guarded(lib.gcl_kernel_map_bitmap_len())
            elif bm == "reused":
                assert filled is not None
                bitmap = filled
            nbr = Guarded((K, n_out), fill=-1 if pre else SENT)
            nbr_t = None if same else Guarded((K, n_in), fill=-1 if pre else SENT)
            counts = Guarded(K, fill=0 if acc else SENT)
            scratch = Guarded(lib.gcl_kernel_map_scratch_len(ks, n_out))
            flags = same | acc | pre | (2 if bm == "reused" else 0)
            ok(lib, lib.gcl_kernel_map(P(Cd), n_out, P(table), cap, ks, step, flags, None if bitmap is None else P(bitmap),
                                       P(scratch), P(nbr), None if same else P(nbr_t), n_in, P(counts), STREAM()), "gcl_kernel_map")
            torch.cuda.synchronize()
            tag = (ks, step, same, acc, pre, bm, run)
            assert nbr.intact() and counts.intact() and scratch.intact() and (bitmap is None or bitmap.intact()), tag
            assert torch.equal(counts.t, want_c), (tag, counts.np().tolist(), want_c.tolist())
            assert torch.equal(nbr.t, want_d), tag
            if not same:
                assert nbr_t.intact() and torch.equal(nbr_t.t, want_td), tag
            if bm == "fresh":
                filled = bitmap
    return want


@lru_cache(maxsize=2)
def _kmap_scene(case):
    return S.kmap_scene(*case[:5])


@pytest.mark.parametrize("case", S.KMAP_CASES, ids=[c[0] for c in S.KMAP_CASES])
def test_kernel_map_every_launch_shape_and_flag(lib, case):
    name, n_out, ks, same, step, blocks, acc = case
    C_in, C_out = _kmap_scene(case)
    assert len(C_out) == n_out
    table, status = insert(lib, C_in)
    assert status.np().tolist() == [0, 0, 0, 0]
    want = kernel_map_variants(lib, C_in, C_out, table, S.pow2_cap(len(C_in)), ks, step, same)
    if ks > 1 and n_out > 1:
        assert (want >= 0).sum() > n_out                     # the scene has neighbours to find


def test_kernel_map_262145_rows_with_bitmap_false_positives(lib):
    """1025 blocks, a table of 2^20 slots: with the bitmap (1.5 % of the absent lookups hit a set bit and must still end in -1:
    counted in tests/test_oracle_maps.py) and without it."""
    name, n_out, ks, same, step, blocks, acc = S.KMAP_BIG
    C, _ = S.kmap_scene(name, n_out, ks, same, step)
    table, status = insert(lib, C)
    assert status.np().tolist() == [0, 0, 0, 0]
    kernel_map_variants(lib, C, C, table, S.pow2_cap(n_out), ks, step, same, full=False)


# ---------------------------------------------------------------------------------------------------------------
# gcl_kernel_map_pairs
# ---------------------------------------------------------------------------------------------------------------
def pairs_case(lib, nbr):
    K, n_out = nbr.shape
    seg, want_in, want_out = S.pair_lists(nbr)
    total = int(seg[-1])
    from gcl_amd import _lib
    runs, nbr_d = [], dev(nbr)
    for _ in range(2):
        pin, pout = Guarded(max(total, 1)), Guarded(max(total, 1))
        scratch = Guarded(K * ((n_out + 1023) // 1024) + K + 1)
        ok(lib, lib.gcl_kernel_map_pairs(P(nbr_d), K, n_out, _lib.host_i64(seg.tolist()), P(scratch), P(pin), P(pout), STREAM()),
           "gcl_kernel_map_pairs")
        torch.cuda.synchronize()
        assert pin.intact() and pout.intact() and scratch.intact()
        a, b = pin.np(), pout.np()
        assert np.array_equal(a[:total], want_in) and np.array_equal(b[:total], want_out), (K, n_out)
        assert (a[total:] == SENT).all() and (b[total:] == SENT).all()
        runs.append((a, b))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("n_out,K,blocks", S.PAIR_CASES)
def test_pair_lists_segment_edges(lib, n_out, K, blocks):
    """Segments of 0, 1, 127, 128, 129 pairs (empty first, empty last, two empty in a row, exact multiples of 128 without
    padding), hits anywhere and a last compaction block without hits; 256 / 257 blocks: the second trip of the carry loop."""
    if n_out >= 262144:
        counts = [n_out // 2, 129, 0][:K]
        pairs_case(lib, S.synthetic_table(K, n_out, counts, seed=n_out))
        pairs_case(lib, S.synthetic_table(K, n_out, [128, 0, n_out // 3][:K], seed=n_out + 1, hit_rows=(blocks - 1) * 1024))
        return
    counts = S.segment_counts(K, n_out)
    pairs_case(lib, S.synthetic_table(K, n_out, counts, seed=K + n_out))
    pairs_case(lib, S.synthetic_table(K, n_out, counts[::-1], seed=K + n_out + 1))
    if blocks > 1:
        hit_rows = (blocks - 1) * 1024
        pairs_case(lib, S.synthetic_table(K, n_out, np.minimum(counts, hit_rows), seed=K, hit_rows=hit_rows))
    pairs_case(lib, S.synthetic_table(K, n_out, np.zeros(K, np.int64)))                   # no pair at all
    pairs_case(lib, S.synthetic_table(K, n_out, np.full(K, n_out)))                       # every row in every segment


# ---------------------------------------------------------------------------------------------------------------
# gcl_kernel_map_3_from_5, gcl_presence_bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.TABLE_ROWS)
def test_map_3_from_5_rows_and_counts(lib, n):
    rng = np.random.RandomState(n)
    nbr5 = S.synthetic_table(125, n, rng.randint(0, n + 1, 125), seed=n)
    counts5 = S.offset_counts(nbr5)
    want, k5 = S.map3_from_map5(nbr5)
    assert len(set(counts5[k5].tolist())) > 1 or n == 1
    runs, nbr5_d, counts5_d = [], dev(nbr5), dev(counts5)
    for _ in range(2):
        nbr3, counts3 = Guarded((27, n)), Guarded(27)
        ok(lib, lib.gcl_kernel_map_3_from_5(P(nbr5_d), P(counts5_d), n, P(nbr3), P(counts3), STREAM()), "gcl_kernel_map_3_from_5")
        torch.cuda.synchronize()
        assert nbr3.intact() and counts3.intact()
        assert np.array_equal(nbr3.np(), want) and np.array_equal(counts3.np(), counts5[k5])
        runs.append(nbr3.np())
    assert np.array_equal(*runs)


@pytest.mark.parametrize("K", S.PRESENCE_K)
@pytest.mark.parametrize("n", S.TABLE_ROWS)
def test_presence_bits_every_word_count(lib, n, K):
    """K = 32 / 33: the last word full / one bit; K = 128: four full words; bits beyond K stay clear."""
    rng = np.random.RandomState(1000 * K + n)
    counts = rng.randint(0, n + 1, K)
    counts[0], counts[-1] = n, n                                                         # the first and the last offset in every row
    nbr = S.synthetic_table(K, n, counts, seed=K + n)
    want = S.presence_words(nbr)
    runs, nbr_d = [], dev(nbr)
    for _ in range(2):
        bits = Guarded((n, (K + 31) // 32))
        ok(lib, lib.gcl_presence_bits(P(nbr_d), K, n, P(bits), STREAM()), "gcl_presence_bits")
        torch.cuda.synchronize()
        assert bits.intact()
        got = bits.np().view(np.uint32)
        assert np.array_equal(got, want), (n, K)
        runs.append(got)
    assert np.array_equal(*runs)


# ---------------------------------------------------------------------------------------------------------------
# gcl_maps_build
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(S.BUILD_ROWS))
def test_maps_build_on_both_sides_of_its_limits(lib, n):
    """ResUNetBN2C's training maps at exactly 65 536 / 65 537 input rows (one -1 fill for all tables, or a fill per map) and
    262 144 / 262 145 (no presence bitmap, or one shared by the maps of a level): every level's coordinates and the (1, 3, 1)
    map against the reference; every table, count, sorted table and pair list bit for bit the per-operator path's."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.model import load_model
    torch.manual_seed(5)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV)
    specs = model.native_map_specs()
    Cn = S.blob_sheet(n, n)
    C = dev(Cn)
    with torch.cuda.device(DEV):
        ref = ME.CoordinateManager(C).prefetch([s for s in specs if s[1] > 1])
        nat = ME.CoordinateManager.build_native(C, specs)
        assert nat.native is not None and nat.native.desc.arena_used <= nat.native.arena.numel()
        level = Cn
        levels = {1: Cn}
        for t in (2, 4, 8):
            level = S.stride_level(level, t)[0]
            levels[t] = level
        for t in (1, 2, 4, 8):
            got = nat.get_coords(t)
            assert np.array_equal(got.cpu().numpy(), levels[t]), t
            assert torch.equal(ref.get_coords(t), got), t
        km = nat.get_kernel_map(1, 3, 1)
        want = S.kernel_map(Cn, Cn, 3, 1)
        assert torch.equal(km.nbr, dev(want)) and list(km.counts) == S.offset_counts(want).tolist()
        for t_in, ks, stride, tables, pairs in (s[:5] for s in specs):
            if ks == 1:
                a, b = ref.identity_pairs(len(C)), nat.identity_pairs(len(C))
                assert torch.equal(a[0], b[0]) and a[2] == b[2]
                continue
            ka, kb = ref.get_kernel_map(t_in, ks, stride), nat.get_kernel_map(t_in, ks, stride)
            assert torch.equal(ka.nbr, kb.nbr) and ka.counts == kb.counts and ka.n_pairs == kb.n_pairs, (t_in, ks, stride)
            assert (ka.nbr_t is None) == (kb.nbr_t is None)
            if ka.nbr_t is not None:
                assert torch.equal(ka.nbr_t, kb.nbr_t), (t_in, ks, stride)
            for tr in tables:
                for u, v in zip(ka.sorted_table(transposed=tr), kb.sorted_table(transposed=tr)):
                    assert torch.equal(u, v), (t_in, ks, stride, tr)
            if pairs:
                pa, pb = ka.pairs(), kb.pairs()
                assert pa[2] == pb[2] and torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]), (t_in, ks, stride)
