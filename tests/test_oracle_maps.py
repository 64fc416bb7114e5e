"""The map builders' references and scenes without a GPU (tests/map_scenes.py): the vectorised numpy references against plain
loops on every small scene, the conditions each GPU case of tests/test_gpu_map_builders.py depends on (exact row counts, the
segment lengths, wrapping probe chains, presence-bitmap false positives, neighbours outside the packable range), and the case
tables against gcl_map_launch_shape -- the function the dispatchers themselves call -- so that a moved limit fails HERE."""
import ctypes
import os
import sys

import numpy as np
import pytest

from gcl_amd import _lib
from oracle import me_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/map_scenes.py
import map_scenes as S                                                 # noqa: E402


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def shape(lib, n, ks=3, flags=0):
    out = (ctypes.c_int32 * 12)()
    assert lib.gcl_map_launch_shape(n, ks, flags, out) == 0, lib.gcl_last_error()
    return dict(zip(S.SHAPE_WORDS, list(out)))


# ---------------------------------------------------------------------------------------------------------------
# the hash functions, against Python's unbounded integers
# ---------------------------------------------------------------------------------------------------------------
def _mix64_int(h):
    m = (1 << 64) - 1
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & m
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & m
    h ^= h >> 33
    return h


def _key_int(c):
    return (c[0] << 48) | ((c[1] + 32768) << 32) | ((c[2] + 32768) << 16) | (c[3] + 32768)


def test_hash_functions_equal_integer_arithmetic():
    ends, _ = S.range_ends()
    rows = np.concatenate([ends, S.blob_sheet(50, 3)]).astype(np.int64)
    keys = S.pack_key(rows)
    for c, k in zip(rows.tolist(), keys.tolist()):
        assert k == _key_int(c) and k != (1 << 64) - 1                # no packable row is the EMPTY key
        assert int(S.mix64(np.uint64(k))) == _mix64_int(k)
        assert int(S.bitmap_pos(np.uint64(k))) == _mix64_int(k ^ 0x9e3779b97f4a7c15) >> 40
    assert _key_int([65535, 32767, 32767, 32767]) == (1 << 64) - 1     # why batch 65535 is not packable
    assert S.pack_ok([[65534, -32768, 32767, 0]]).all()
    assert not S.pack_ok([[65535, 0, 0, 0], [-1, 0, 0, 0], [0, 32768, 0, 0], [0, 0, -32769, 0], [0, 0, 0, (1 << 31) - 1]]).any()
    assert [S.pow2_cap(n) for n in (1, 32, 33, 256, 262144, 262145)] == [64, 64, 128, 512, 524288, 1048576]


# ---------------------------------------------------------------------------------------------------------------
# vectorised references == plain loops, on every small scene
# ---------------------------------------------------------------------------------------------------------------
def _small_scenes():
    ends, outside = S.range_ends()
    blob = S.blob_sheet(300, 1)
    return {
        "blob+sheet": blob,
        "dense cube": S.dense_cube(6),
        "line": S.line_x(40),
        "range ends": ends,
        "hash stress": S.hash_stress(),
        "one row": S.blob_sheet(1, 5),
    }


@pytest.mark.parametrize("name", ["blob+sheet", "dense cube", "line", "range ends", "hash stress", "one row"])
def test_kernel_map_reference_equals_kernel_map_dict(name):
    C = _small_scenes()[name]
    for ks, step in ((1, 1), (3, 1), (5, 1), (3, 2), (3, 4)):
        Cs = C.astype(np.int64)
        if name != "range ends":
            Cs[:, 1:] *= step                                            # a level of tensor stride `step`
        nbr = S.kernel_map(Cs, Cs, ks, step)
        assert nbr.shape == (ks ** 3, len(C)) and nbr.dtype == np.int32
        assert np.array_equal(O.canonical(S.triples_of(nbr)), O.canonical(O.kernel_map_dict(Cs, Cs, ks, step))), (ks, step)
        assert np.array_equal(nbr[ks ** 3 // 2], np.arange(len(C)))      # the centre offset of a same-map is the row itself
        assert np.array_equal(nbr[::-1], S.transpose_table(nbr, len(C)))  # mirror offsets: nbr_t[k] == nbr[K - 1 - k]
    # a stride-2 map: the level below onto shuffled output rows
    if name in ("blob+sheet", "dense cube", "one row"):
        for step in (1, 2):
            Cout = C.astype(np.int64)
            Cout[:, 1:] *= 2 * step
            Cin = S.children_of(Cout, step, 3)
            lvl, _, bad = S.stride_level(Cin, 2 * step)
            assert bad == 0 and np.array_equal(np.sort(S.pack_key(lvl)), np.sort(S.pack_key(Cout)))
            nbr = S.kernel_map(Cin, Cout, 3, step)
            assert np.array_equal(O.canonical(S.triples_of(nbr)), O.canonical(O.kernel_map_dict(Cin, Cout, 3, step)))
            nbr_t = S.transpose_table(nbr, len(Cin))
            want = np.full_like(nbr_t, -1)
            for k, u, v in S.triples_of(nbr).tolist():
                want[k, u] = v
            assert np.array_equal(nbr_t, want) and (nbr_t >= 0).sum() == (nbr >= 0).sum()


@pytest.mark.parametrize("name", ["blob+sheet", "dense cube", "line", "range ends", "hash stress", "one row"])
def test_strided_level_reference_equals_first_occurrence_loop(name):
    C = _small_scenes()[name]
    _, outside = S.range_ends()
    with_bad = np.concatenate([C[: len(C) // 2], outside, C[len(C) // 2:], C[:5], outside[:2]])      # duplicates and bad rows
    for rows in (C, with_bad, S.duplicates(700, 2), S.garbage_tail(S.blob_sheet(300, 4), 200)):
        for t in (1, 2, 4, 8):
            got, want = S.stride_level(rows, t), S.stride_level_loop(rows, t)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, t)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert np.array_equal(S.stride_level(S.blob_sheet(300, 1), 4)[0], O.stride_coords(S.blob_sheet(300, 1), 4))
    bad, dup = S.insert_status(with_bad)
    assert bad == len(outside) + 2 and dup == min(5, len(C))


def test_pair_list_presence_and_count_references_equal_loops():
    for K, n in ((1, 1), (27, 300), (125, 257), (33, 40)):
        nbr = S.synthetic_table(K, n, S.segment_counts(K, n), seed=K)
        for a, b in zip(S.pair_lists(nbr), S.pair_lists_loop(nbr)):
            assert np.array_equal(a, b) and a.dtype == b.dtype
        assert np.array_equal(S.offset_counts(nbr), [sum(int(x) >= 0 for x in row) for row in nbr])
        bits = S.presence_words(nbr)
        for v in range(n):
            for k in range(K):
                assert (int(bits[v, k >> 5]) >> (k & 31)) & 1 == int(nbr[k, v] >= 0)
        assert not any(int(bits[v, -1]) >> (((K - 1) & 31) + 1) for v in range(n))          # no bit beyond K
    nbr5 = S.synthetic_table(125, 50, np.full(125, 20), seed=9)
    nbr3, k5 = S.map3_from_map5(nbr5)
    o3, o5 = S.kernel_offsets(3), S.kernel_offsets(5)
    for k3 in range(27):
        assert np.array_equal(o5[k5[k3]], o3[k3]) and np.array_equal(nbr3[k3], nbr5[k5[k3]])
    # on a real cloud: the 3^3 map is those 27 rows of the 5^3 map
    C = S.dense_cube(6)
    assert np.array_equal(S.map3_from_map5(S.kernel_map(C, C, 5, 1))[0], S.kernel_map(C, C, 3, 1))


# ---------------------------------------------------------------------------------------------------------------
# what the GPU cases depend on
# ---------------------------------------------------------------------------------------------------------------
def test_scenes_have_exactly_the_requested_unique_rows():
    for n in (1, 255, 256, 257, 2047, 2048, 2049, 16385, 65537):
        C = S.blob_sheet(n, n)
        assert C.shape == (n, 4) and C.dtype == np.int32 and len(np.unique(S.pack_key(C))) == n
        if n > 255:
            assert C[:, 1:].min() < 0 < C[:, 1:].max() and set(C[:, 0]) == {0, 1}
    assert np.array_equal(S.blob_sheet(257, 3), S.blob_sheet(257, 3))                  # deterministic
    for n in (1, 255, 2049):
        assert S.duplicates(n, n).shape == (n, 4) and S.line_x(n).shape == (n, 4)
    for n_in in S.STRIDE_ROWS:
        if n_in <= 2049:
            for t in S.STRIDE_T_OUT:
                C = S.stride_scene(n_in, t)
                assert C.shape == (n_in, 4) and (C[S.pack_ok(C)][:, 1:] % max(1, t // 2) == 0).all()
                assert (~S.pack_ok(C)).sum() == (3 if n_in >= 255 else 0)
    for name, n_out, ks, same, step, _, _ in S.KMAP_CASES[:7]:
        Cin, Cout = S.kmap_scene(name, n_out, ks, same, step)
        assert Cout.shape == (n_out, 4) and len(np.unique(S.pack_key(Cout))) == n_out
        assert len(np.unique(S.pack_key(Cin))) == len(Cin)
        if not same and ks > 1:
            lvl = S.stride_level(Cin, 2 * step)[0]
            assert len(lvl) == n_out and (n_out == 1 or not np.array_equal(lvl, Cout))                 # same voxels, another row order
            assert (Cin[:, 1:] % step == 0).all()


def test_dense_cube_and_line_scenes():
    C = S.dense_cube(6)
    for ks in (3, 5):
        nbr = S.kernel_map(C, C, ks, 1)
        assert ((nbr >= 0).all(0)).sum() == (6 - 2 * (ks // 2)) ** 3                   # interior rows own every offset
        assert (S.offset_counts(nbr) > 0).all()
    counts = S.offset_counts(S.kernel_map(S.line_x(300), S.line_x(300), 3, 1))
    assert counts.tolist() == [0] * 12 + [299, 300, 299] + [0] * 12                    # first, last and runs of empty segments
    counts5 = S.offset_counts(S.kernel_map(S.line_x(300), S.line_x(300), 5, 1))
    assert (counts5 > 0).sum() == 5 and counts5[0] == 0 and counts5[-1] == 0


def test_synthetic_tables_hold_the_segment_edges():
    for K in (27, 125):
        c = S.segment_counts(K, 1025)
        assert {0, 1, 127, 128, 129} <= set(c.tolist()) and c[0] == 0 and c[-1] == 0
        assert any(c[k] == 0 and c[k + 1] == 0 for k in range(K - 1))
        nbr = S.synthetic_table(K, 1025, c, seed=1, hit_rows=1024)
        assert np.array_equal(S.offset_counts(nbr), c)
        assert (nbr[:, 1024:] < 0).all()                                               # the last compaction block has no hit
        seg = S.segment_offsets(c)
        assert (seg % 128 == 0).all() and seg[-1] > c.sum()
        assert any(c[k] and c[k] % 128 == 0 for k in range(K))                         # a segment without padding
    assert S.segment_counts(1, 1).tolist() == [0] and S.segment_counts(27, 1).max() == 1


def test_hash_stress_scene_wraps_and_chains():
    C = S.hash_stress()
    assert C.shape == (32, 4) and len(np.unique(S.pack_key(C))) == 32 and S.pow2_cap(32) == 64      # cap == 2 n, n a power of two
    home = S.home_slots(C, 64)
    assert (home >= 60).sum() >= 8
    slot, probes, wrapped = S.simulate_probes(C, 64)
    assert len(wrapped) >= 1 and probes.max() >= 6
    assert len(set(slot.tolist())) == 32 and (slot[wrapped] < 60).all()                # wrapped rows live at the table's start
    # whatever the order of insertion, the crowd's cluster is slots 60 .. 63, 0 .. 5
    for seed in range(3):
        s2, _, w2 = S.simulate_probes(C[np.random.RandomState(seed).permutation(32)], 64)
        assert set(s2.tolist()) == set(slot.tolist()) and len(w2) >= 1


def test_duplicates_scene_spans_block_borders():
    C = S.duplicates(6000, 1)
    keys = S.pack_key(C)
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    assert cnt.min() == 1 and cnt.max() == 5 and set(cnt.tolist()) == {1, 2, 3, 4, 5}
    _, first, _ = S.stride_level(C, 1)
    first_of = np.full(len(cnt), -1)
    first_of[inv[first]] = first
    later = np.nonzero(first_of[inv] != np.arange(len(C)))[0]
    gap = later - first_of[inv[later]]
    assert (gap > 2048).sum() > 100 and (first_of[inv[later]] // 256 != later // 256).sum() > 100
    assert not np.array_equal(first, np.arange(len(first)))


def test_range_scene_counts_neighbours_outside_the_range():
    ends, outside = S.range_ends()
    assert not S.pack_ok(outside).any() and S.pack_ok(ends).all()
    assert {S.LO, S.HI} <= set(ends[:, 1]) and S.BATCH_MAX in ends[:, 0]
    _, ok = S.neighbour_queries(ends, 3, 1)
    corner = (np.abs(ends[:, 1:].astype(np.int64) * 2 + 1) == 65535).all(1)            # all three axes at an end
    assert corner.sum() == 16
    assert ((~ok)[:, corner].sum(0) == 27 - 8).all()                                   # 19 of a corner's 27 neighbours do not exist
    by_loop = sum(1 for c in ends.tolist() for o in S.kernel_offsets(3).tolist()
                  if not all(S.LO <= c[1 + a] + o[a] <= S.HI for a in range(3)))
    assert int((~ok).sum()) == by_loop == 16 * 19 + 2 * (27 - 12)      # + two rows with two axes at an end
    _, ok4 = S.neighbour_queries(ends, 3, 4)
    assert (~ok4).sum() > (~ok).sum()                                                  # a step of 4 reaches further out


def test_garbage_tail_holds_duplicates_and_bad_rows():
    C = S.blob_sheet(300, 2)
    G = S.garbage_tail(C, 200)
    assert np.array_equal(G[:200], C[:200])
    tail_ok = S.pack_ok(G[200:])
    assert tail_ok.sum() == 50 and (~tail_ok).sum() == 50
    assert np.isin(S.pack_key(G[200:][tail_ok]), S.pack_key(C[:200])).all()
    a, b = S.stride_level(G[:200], 2), S.stride_level(G, 2)
    assert b[2] == a[2] + 50 and np.array_equal(a[0], b[0])                            # the tail changes the status only


def test_the_big_scene_has_bitmap_false_positives():
    """262 145 keys set 1.5 % of the 2^24 presence bits: absent neighbours whose bit is set must still end in -1."""
    name, n_out, ks, same, step, _, _ = S.KMAP_BIG
    C, _ = S.kmap_scene(name, n_out, ks, same, step)
    absent, false_pos = S.bitmap_false_positives(C, C, ks, step)
    assert len(C) == 262145 and absent > 1000000 and false_pos >= 100, (absent, false_pos)


# ---------------------------------------------------------------------------------------------------------------
# the case tables name the launch shape they expect
# ---------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_the_launch_shapes_they_name(lib):
    for n_in, (long_form, blocks) in S.STRIDE_ROWS.items():
        s = shape(lib, n_in, 1, 0)
        assert (s["stride_long"], s["scan_blocks"]) == (long_form, blocks), n_in
    for name, n_out, ks, same, step, blocks, acc in S.KMAP_CASES + [S.KMAP_BIG]:
        K = ks ** 3
        for bit3 in (0, 8):
            s = shape(lib, n_out, ks, same | 4 | bit3)
            assert s["grid_x"] == blocks and s["acc"] == acc and s["reduce"] == 1 - acc, name
            assert s["grid_y"] == -(-(K // 2 + 1 if same else K) // s["kpt"]), name
            s = shape(lib, n_out, ks, same | bit3 | 2)
            assert s["grid_x"] == blocks and s["acc"] == 0 and s["reduce"] == 1, name
    for n_out, K, blocks in S.PAIR_CASES:
        assert shape(lib, n_out)["pair_blocks"] == blocks, n_out
    for n, (prefill, bitmap) in S.BUILD_ROWS.items():
        s = shape(lib, n)
        assert (s["prefill"], s["use_bitmap"]) == (prefill, bitmap), n
    assert lib.gcl_map_launch_shape(0, 3, 0, (ctypes.c_int32 * 12)()) == -1
    assert lib.gcl_map_launch_shape(10, 4, 0, (ctypes.c_int32 * 12)()) == -1 and b"gcl_map_launch_shape" in lib.gcl_last_error()


def test_case_tables_hold_both_sides_of_every_limit():
    assert {256, 257} <= {b for _, b in S.STRIDE_ROWS.values()} and {0, 1} == {f for f, _ in S.STRIDE_ROWS.values()}
    blocks = {c[5] for c in S.KMAP_CASES}
    assert {64, 65} <= blocks and {256, 257} <= blocks and {0, 1} == {c[6] for c in S.KMAP_CASES}      # map and count blocks
    assert {256, 257} <= {b for _, _, b in S.PAIR_CASES}
    assert {(1, 0), (0, 0), (0, 1)} == set(S.BUILD_ROWS.values())
    assert {1, 3, 5} == {c[2] for c in S.KMAP_CASES} and {1, 2, 4} == {c[4] for c in S.KMAP_CASES}
    assert all(c[2] == 3 or c[1] <= 16385 or c[2] == 1 for c in S.KMAP_CASES)          # 5^3 only up to 16 385 rows
