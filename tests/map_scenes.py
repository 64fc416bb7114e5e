"""Scenes and numpy references for the map builders of csrc/coords.hip (test infrastructure, numpy only).

Everything here is integer work, so every reference is exact.  The references take arbitrary coordinate arrays (any batch
index, any coordinate, in or out of the packable range) and restate what the C ABI documents:

* a row is packable when 0 <= batch < 65535 and -32768 <= x, y, z <= 32767; other rows are counted in status[0] and dropped;
* a strided level holds floor(c / t) * t of its input rows, unique, in order of FIRST occurrence;
* nbr[k][v] = row of c_out[v] + o_k * step in the input map or -1 (x fastest in k); nbr_t[k][u] = v is its transpose;
* pair lists: per offset the (in, out) rows with out ascending, every segment padded with -1 to a multiple of 128;
* presence words: bit (k & 31) of word k >> 5 of row v = nbr[k][v] >= 0.

``pack_key``, ``mix64`` and ``bitmap_pos`` are the library's hash functions in numpy uint64 (csrc/common.h, csrc/coords.hip),
so that a scene can place keys in chosen slots of the hash table and count the presence bitmap's false positives.

The case tables at the end name, for every GPU case of tests/test_gpu_map_builders.py, the launch shape it is meant to reach;
tests/test_oracle_maps.py pins them against gcl_map_launch_shape, so a moved limit fails there and does not silently move a case.
"""
import numpy as np

COORD_OFF = 1 << 15
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
PAIR_CHUNK = 128
BITMAP_BITS_LOG2 = 24
LO, HI, BATCH_MAX = -32768, 32767, 65534      # the ends of the packable range


# ---------------------------------------------------------------------------------------------------------------
# hash functions
# ---------------------------------------------------------------------------------------------------------------
def pack_ok(C):
    C = np.asarray(C, dtype=np.int64).reshape(-1, 4)
    return (C[:, 0] >= 0) & (C[:, 0] <= BATCH_MAX) & (C[:, 1:] >= LO).all(1) & (C[:, 1:] <= HI).all(1)


def pack_key(C):
    """uint64 keys of packable rows [n, 4]."""
    C = np.asarray(C, dtype=np.int64).reshape(-1, 4)
    assert pack_ok(C).all()
    k = (C[:, 0] << 48) | ((C[:, 1] + COORD_OFF) << 32) | ((C[:, 2] + COORD_OFF) << 16) | (C[:, 3] + COORD_OFF)
    return k.view(np.uint64)          # (batch 65534 << 48 wraps in int64; the bit pattern is the key)


def mix64(h):
    h = np.asarray(h, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def bitmap_pos(key):
    return (mix64(np.asarray(key, dtype=np.uint64) ^ np.uint64(0x9e3779b97f4a7c15)) >> np.uint64(64 - BITMAP_BITS_LOG2)).astype(np.int64)


def pow2_cap(n):
    cap = 64
    while cap < 2 * n:
        cap *= 2
    return cap


def home_slots(C, cap):
    return (mix64(pack_key(C)) & np.uint64(cap - 1)).astype(np.int64)


def simulate_probes(C, cap):
    """Inserts the rows one after the other (linear probing).  Returns (slot of every row, probes of every row, rows whose
    chain wrapped from slot cap - 1 to 0).  The CLUSTERS of the final table do not depend on the order of insertion."""
    home = home_slots(C, cap)
    used = np.zeros(cap, bool)
    slot, probes, wrapped = [], [], []
    for i, h in enumerate(home):
        s, p, w = int(h), 1, False
        while used[s]:
            w = w or s == cap - 1
            s = (s + 1) & (cap - 1)
            p += 1
        used[s] = True
        slot.append(s)
        probes.append(p)
        if w:
            wrapped.append(i)
    return np.asarray(slot), np.asarray(probes), wrapped


# ---------------------------------------------------------------------------------------------------------------
# references, vectorised
# ---------------------------------------------------------------------------------------------------------------
def floor_to(C, t):
    D = np.asarray(C, dtype=np.int64).reshape(-1, 4).copy()
    D[:, 1:] = np.floor_divide(D[:, 1:], t) * t
    return D


def stride_level(C, t_out):
    """(coords_out int32 [m, 4], index_out int64 [m], rows outside the packable range) of gcl_stride_map / gcl_unique_coords."""
    D = floor_to(C, t_out)
    ok = pack_ok(D)
    rows = np.nonzero(ok)[0]
    _, first = np.unique(pack_key(D[rows]), return_index=True)
    first = np.sort(rows[first])
    return D[first].astype(np.int32), first.astype(np.int64), int((~ok).sum())


def insert_status(C):
    """(rows outside the packable range, rows whose key was already in the table) of gcl_coords_insert."""
    ok = pack_ok(C)
    keys = pack_key(np.asarray(C).reshape(-1, 4)[ok])
    return int((~ok).sum()), int(len(keys) - len(np.unique(keys)))


def kernel_offsets(ks):
    k = np.arange(ks ** 3)
    r = ks // 2
    return np.stack([k % ks - r, (k // ks) % ks - r, k // (ks * ks) - r], 1).astype(np.int64)


def neighbour_queries(C_out, ks, step):
    """(Q int64 [K, n_out, 4], packable [K, n_out]): the coordinates a kernel map looks up."""
    C_out = np.asarray(C_out, dtype=np.int64).reshape(-1, 4)
    Q = np.repeat(C_out[None], ks ** 3, 0)
    Q[:, :, 1:] += (kernel_offsets(ks) * step)[:, None, :]
    return Q, pack_ok(Q.reshape(-1, 4)).reshape(ks ** 3, -1)


def kernel_map(C_in, C_out, ks, step):
    """nbr int32 [K, n_out].  C_in: unique packable rows (its row numbers are the table's values)."""
    kin = pack_key(C_in)
    order = np.argsort(kin, kind="stable")
    skeys = kin[order]
    assert len(skeys) == 0 or (skeys[1:] != skeys[:-1]).all(), "the input map holds a voxel twice"
    Q, ok = neighbour_queries(C_out, ks, step)
    nbr = np.full(ok.shape, -1, np.int32)
    q = pack_key(Q[ok])
    pos = np.minimum(np.searchsorted(skeys, q), len(skeys) - 1)
    hit = skeys[pos] == q
    flat = np.full(len(q), -1, np.int32)
    flat[hit] = order[pos[hit]]
    nbr[ok] = flat
    return nbr


def transpose_table(nbr, n_in):
    nbr_t = np.full((nbr.shape[0], n_in), -1, np.int32)
    k, v = np.nonzero(nbr >= 0)
    nbr_t[k, nbr[k, v]] = v
    return nbr_t


def offset_counts(nbr):
    return (nbr >= 0).sum(1).astype(np.int32)


def segment_offsets(counts):
    pad = (np.asarray(counts, dtype=np.int64) + PAIR_CHUNK - 1) // PAIR_CHUNK * PAIR_CHUNK
    return np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)


def pair_lists(nbr):
    """(seg_off int64 [K + 1], pair_in, pair_out int32 [seg_off[K]])."""
    seg = segment_offsets(offset_counts(nbr))
    pin = np.full(int(seg[-1]), -1, np.int32)
    pout = np.full(int(seg[-1]), -1, np.int32)
    for k in range(nbr.shape[0]):
        v = np.nonzero(nbr[k] >= 0)[0]
        pin[seg[k]:seg[k] + len(v)] = nbr[k, v]
        pout[seg[k]:seg[k] + len(v)] = v
    return seg, pin, pout


def presence_words(nbr):
    K, n = nbr.shape
    bits = np.zeros((n, (K + 31) // 32), np.uint32)
    for k in range(K):
        bits[:, k >> 5] |= (nbr[k] >= 0).astype(np.uint32) << np.uint32(k & 31)
    return bits


def map3_from_map5(nbr5):
    k3 = np.arange(27)
    k5 = (k3 % 3 + 1) + 5 * ((k3 // 3) % 3 + 1) + 25 * (k3 // 9 + 1)
    return nbr5[k5].copy(), k5


def bitmap_false_positives(C_in, C_out, ks, step):
    """(absent packable lookups, those among them whose presence bit is set by some key of C_in)."""
    bits = np.zeros(1 << BITMAP_BITS_LOG2, bool)
    bits[bitmap_pos(pack_key(C_in))] = True
    Q, ok = neighbour_queries(C_out, ks, step)
    nbr = kernel_map(C_in, C_out, ks, step)
    absent = ok & (nbr < 0)
    return int(absent.sum()), int(bits[bitmap_pos(pack_key(Q[absent]))].sum())


# ---------------------------------------------------------------------------------------------------------------
# references, plain loops (tests/test_oracle_maps.py pins the vectorised forms to these)
# ---------------------------------------------------------------------------------------------------------------
def stride_level_loop(C, t_out):
    seen, rows, bad = {}, [], 0
    for i, c in enumerate(np.asarray(C).reshape(-1, 4).tolist()):
        d = (c[0],) + tuple((v // t_out) * t_out for v in c[1:])           # Python's // floors
        if not (0 <= d[0] <= BATCH_MAX and all(LO <= v <= HI for v in d[1:])):
            bad += 1
        elif d not in seen:
            seen[d] = i
            rows.append(d)
    return np.asarray(rows, np.int32).reshape(-1, 4), np.asarray(list(seen.values()), np.int64), bad


def triples_of(nbr):
    k, v = np.nonzero(nbr >= 0)
    return np.stack([k, nbr[k, v], v], 1).astype(np.int64)


def pair_lists_loop(nbr):
    seg, pin, pout = [0], [], []
    for k in range(nbr.shape[0]):
        c = 0
        for v in range(nbr.shape[1]):
            if nbr[k, v] >= 0:
                pin.append(int(nbr[k, v]))
                pout.append(v)
                c += 1
        while c % PAIR_CHUNK:
            pin.append(-1)
            pout.append(-1)
            c += 1
        seg.append(len(pin))
    return np.asarray(seg, np.int64), np.asarray(pin, np.int32), np.asarray(pout, np.int32)


# ---------------------------------------------------------------------------------------------------------------
# scenes: exactly the requested number of unique rows (generate, unique, shuffle, truncate)
# ---------------------------------------------------------------------------------------------------------------
def _exactly(rows, n, rng):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    _, first = np.unique(pack_key(rows), return_index=True)
    rows = rows[np.sort(first)]
    assert len(rows) >= n, (len(rows), n)
    rows = rows[rng.permutation(len(rows))[:n]]
    return rows.astype(np.int32)


def blob_sheet(n, seed=0, batch=2):
    """A blob plus a two-voxel-thick sheet per cloud (the shape of random_cloud), negative coordinates included."""
    rng = np.random.RandomState(seed)
    e = max(2, int(round((n / batch) ** (1.0 / 3.0))))          # blob: ~ n / (2 batch) points in (2e)^3 cells
    rows = []
    have = 0
    while have < n:
        m = n + 64
        b = rng.randint(0, batch, m)
        pts = rng.randint(-e, e, (m, 3))
        sheet = rng.rand(m) < 0.5
        pts[sheet, :2] = rng.randint(-6 * e, 6 * e, (int(sheet.sum()), 2))
        pts[sheet, 2] = rng.randint(-1, 1, int(sheet.sum()))
        rows.append(np.concatenate([b[:, None], pts], 1))
        have = len(np.unique(pack_key(np.concatenate(rows))))
    return _exactly(np.concatenate(rows), n, rng)


def dense_cube(side, seed=0, lo=-3):
    """Every cell of a side^3 block, shuffled: interior voxels own all 27 (side >= 3) / 125 (side >= 5) neighbours."""
    g = np.arange(lo, lo + side)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rows = np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1)
    return _exactly(rows, side ** 3, np.random.RandomState(seed))


def line_x(n, seed=0):
    """n voxels in a row along x: every offset with dy != 0 or dz != 0 has no pair (the first and the last offset among them)."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((n, 4), np.int64)
    rows[:, 1] = np.arange(n) - n // 2
    return _exactly(rows, n, rng)


def range_ends():
    """(packable rows at the ends of the range, rows one step outside it).  The packable rows sit at -32768 and 32767 on each
    axis, in batch 65534 (and 0), so that neighbours of theirs fall outside the range."""
    ends = [LO, HI]
    rows = [[b, x, y, z] for b in (0, BATCH_MAX) for x in ends for y in ends for z in ends]
    rows += [[BATCH_MAX, LO + 1, 0, 0], [BATCH_MAX, HI - 1, 0, 0], [BATCH_MAX, HI, HI, HI - 1], [0, LO, LO, LO + 1]]
    outside = [[BATCH_MAX + 1, 0, 0, 0], [-1, 0, 0, 0], [0, HI + 1, 0, 0], [0, 0, LO - 1, 0], [0, 0, 0, HI + 1], [3, LO - 1, HI + 1, 0],
               [0, 2 ** 31 - 1, 0, 0], [0, 0, -2 ** 31, 0]]
    rng = np.random.RandomState(1)
    return _exactly(rows, len(rows), rng), np.asarray(outside, np.int32)


def hash_stress(n=32, cap=64, crowd=10):
    """n rows for a table of `cap` slots: `crowd` keys whose home is one of the LAST FOUR slots (their cluster wraps from slot
    cap - 1 to 0), the rest with homes in the middle of the table.  Picked by evaluating mix64, lowest candidates first."""
    g = np.arange(-8, 8)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cand = np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1)
    home = home_slots(cand, cap)
    last = np.nonzero(home >= cap - 4)[0][:crowd]
    mid = np.nonzero((home >= cap // 4) & (home < cap // 2))[0][:n - crowd]
    assert len(last) == crowd and len(mid) == n - crowd
    rows = np.concatenate([cand[mid], cand[last]])          # the crowd goes in last: its chains are the longest
    return rows.astype(np.int32)


def duplicates(n, seed=0):
    """n rows for gcl_unique_coords: every voxel 1 to 5 times, at random places of the array (first and later occurrences of a
    voxel lie blocks apart once n is a few thousand)."""
    rng = np.random.RandomState(seed)
    mult = rng.randint(1, 6, n)
    m = int(np.searchsorted(np.cumsum(mult), n)) + 1            # voxels needed
    mult = mult[:m]
    mult[-1] -= int(mult.sum()) - n
    assert mult.min() >= 1 and mult.sum() == n
    vox = blob_sheet(m, seed + 1000)
    rows = np.repeat(vox, mult, axis=0)
    return rows[rng.permutation(n)].astype(np.int32)


def children_of(C_out, step, seed=0):
    """An input map whose stride-2 level is exactly the rows of C_out (multiples of 2 * step): 1 to 8 of every voxel's children."""
    rng = np.random.RandomState(seed)
    C_out = np.asarray(C_out, dtype=np.int64)
    keep = rng.rand(len(C_out), 8) < 0.4
    keep[np.arange(len(C_out)), rng.randint(0, 8, len(C_out))] = True
    v, j = np.nonzero(keep)
    rows = C_out[v].copy()
    rows[:, 1] += (j & 1) * step
    rows[:, 2] += ((j >> 1) & 1) * step
    rows[:, 3] += ((j >> 2) & 1) * step
    return rows[rng.permutation(len(rows))].astype(np.int32)


def synthetic_table(K, n, counts, seed=0, n_in=None, hit_rows=None):
    """nbr int32 [K, n] with exactly counts[k] entries >= 0 in row k, at random output rows below `hit_rows` (default n)."""
    rng = np.random.RandomState(seed)
    n_in = n_in or n
    hit_rows = n if hit_rows is None else hit_rows
    nbr = np.full((K, n), -1, np.int32)
    for k in range(K):
        c = int(counts[k])
        assert c <= hit_rows
        v = rng.permutation(hit_rows)[:c]
        nbr[k, v] = rng.randint(0, n_in, c)
    return nbr


def segment_counts(K, n, seed=0):
    """Per-offset counts that cycle through the edges 0, 1, 127, 128, 129 (clipped to n), with an empty first and last segment
    and two empty segments in a row when K allows."""
    edge = [0, 1, 127, 128, 129, 0, 0, 255, 256, 257]
    c = np.asarray([min(edge[k % len(edge)], n) for k in range(K)], np.int64)
    if K > 1:
        c[-1] = 0
    return c


# ---------------------------------------------------------------------------------------------------------------
# case tables.  shape words: gcl_map_launch_shape's out[]
# ---------------------------------------------------------------------------------------------------------------
SHAPE_WORDS = ("stride_long", "scan_blocks", "acc", "grid_x", "grid_y", "reduce", "pair_blocks", "prefill", "use_bitmap", "kpt")

# gcl_coords_insert / gcl_stride_map / gcl_unique_coords: n_in -> (form, scan blocks)
STRIDE_ROWS = {1: (0, 1), 255: (0, 1), 256: (0, 1), 257: (0, 1), 2047: (0, 1), 2048: (0, 1), 2049: (0, 2),
               524288: (0, 256), 524289: (1, 257)}
STRIDE_T_OUT = (1, 2, 4, 8)

# gcl_kernel_map: (name, n_out, ks, same_map, step) -> blocks; counts by atomics with flag bit 2; count blocks of the reduction
#   n_out 16384 / 16385: 64 / 65 map blocks (atomic counts on / off); 65536 / 65537: 256 / 257 blocks per k_count_reduce row
KMAP_CASES = [
    # name,            n_out,  ks, same, step, blocks, acc with bit 2
    ("one-row",            1,   3,    1,    1,      1, 1),
    ("one-row-k1",         1,   1,    0,    1,      1, 1),
    ("one-row-down",       1,   3,    0,    1,      1, 1),
    ("255-same-k5",      255,   5,    1,    1,      1, 1),
    ("256-down-step2",   256,   3,    0,    2,      1, 1),
    ("257-same-step4",   257,   3,    1,    4,      2, 1),
    ("257-k1",           257,   1,    0,    1,      2, 1),
    ("16384-same",     16384,   3,    1,    1,     64, 1),
    ("16384-down",     16384,   3,    0,    1,     64, 1),
    ("16384-same-k5",  16384,   5,    1,    2,     64, 1),
    ("16385-same",     16385,   3,    1,    1,     65, 0),
    ("16385-down-s4",  16385,   3,    0,    4,     65, 0),
    ("16385-same-k5",  16385,   5,    1,    1,     65, 0),
    ("65536-same",     65536,   3,    1,    1,    256, 0),
    ("65537-same",     65537,   3,    1,    2,    257, 0),
    ("65537-down",     65537,   3,    0,    1,    257, 0),
    ("65537-k1",       65537,   1,    0,    1,    257, 0),
]
KMAP_BIG = ("262145-same", 262145, 3, 1, 1, 1025, 0)       # with and without the bitmap; its false positives are counted on the CPU

# gcl_kernel_map_pairs: (n_out, K) -> compaction blocks
PAIR_CASES = [(1, 1, 1), (1, 27, 1), (1023, 27, 1), (1024, 125, 1), (1025, 27, 2), (1025, 1, 2), (1025, 125, 2),
              (262144, 3, 256), (262145, 3, 257)]

# gcl_maps_build: input rows -> (prefill, use_bitmap)
BUILD_ROWS = {65536: (1, 0), 65537: (0, 0), 262144: (0, 0), 262145: (0, 1)}

TABLE_ROWS = (1, 255, 256, 257)                      # gcl_kernel_map_3_from_5, gcl_presence_bits
PRESENCE_K = (1, 27, 32, 33, 125, 128)


def kmap_scene(name, n_out, ks, same, step, seed=0):
    """(C_in, C_out) of a kernel-map case: same-map cases read their own coordinates (multiples of `step`); the others map the
    level below onto n_out rows that are multiples of 2 * step, in shuffled (not first-occurrence) order."""
    C = blob_sheet(n_out, seed + n_out).astype(np.int64)
    if ks == 1:
        C[:, 1:] *= step
        return C.astype(np.int32), C.astype(np.int32)
    if same:
        C[:, 1:] *= step
        return C.astype(np.int32), C.astype(np.int32)
    C[:, 1:] *= 2 * step
    return children_of(C, step, seed + 7), C.astype(np.int32)


def stride_scene(n_in, t_out, seed=0):
    """n_in rows for a strided level: duplicates for t_out = 1, raw rows for 2, multiples of t_out / 2 above (what the chain of
    levels feeds), with three rows outside the packable range among them once there is room."""
    if t_out == 1:
        C = duplicates(n_in, seed + n_in).astype(np.int64)
    else:
        C = blob_sheet(n_in, seed + n_in + t_out).astype(np.int64)
        C[:, 1:] *= t_out // 2
    if n_in >= 255:
        _, outside = range_ends()
        C[[n_in // 7, n_in // 2, n_in - 2]] = outside[[0, 2, 6]]
    return C.astype(np.int32)


def garbage_tail(C, n_dev):
    """The first n_dev rows of C followed by len(C) - n_dev rows the entry must not read as data: duplicates of earlier rows
    alternating with rows outside the packable range."""
    C = np.asarray(C, dtype=np.int32).copy()
    _, outside = range_ends()
    j = np.arange(len(C) - n_dev)
    C[n_dev:] = np.where((j % 2 == 0)[:, None], C[(j * 7919) % n_dev], outside[j % len(outside)])
    return C
