"""The co-location group kernels (csrc/data.hip: k_colocation_hits, k_colocation_sizes / k_colocation_emit) and the key-less
loader kernels beside them, called directly through the C ABI against the numpy references of tests/colocation_scenes.py.

Every comparison in this file is EXACT (first_rng and the loader's points as bit patterns).  Outputs live inside allocations
filled with the byte 0xA5 whose guard bytes must survive the call, scratch is pre-filled with the same byte (nothing may
depend on what it held), and every launch runs twice on fresh buffers, the two results compared bit for bit.  What each
scene of the case table reaches -- R = 1 .. 4 and so every survivor word, K = 1 / 5 / 8, a lane's list filled to KMAX, exact
distance and range ties, points exactly on the radius, hits whose voxel box lies at the radius, pairs of points that are
equidistant only when no product is fused into a sum, every scan shape -- is asserted without a GPU in
tests/test_oracle_colocation.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/colocation_scenes.py
import colocation_scenes as S                                          # noqa: E402
from map_scenes import pow2_cap                                        # noqa: E402

DEV = "cuda:0"
FILL = 0xA5                 # every byte of outputs, scratch and guards before a call
GUARD = 256                 # guard bytes on either side of an output
I32, I64, F32, F64, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8
ERR_ARG = -1
PD = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    from gcl_amd import _lib
    return _lib.require_gpu()


class Guarded:
    """A tensor inside a larger allocation filled with the byte 0xA5."""

    def __init__(self, shape, dtype=I32):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.bytes = int(np.prod(self.shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((self.bytes + 2 * GUARD,), FILL, dtype=U8, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.bytes].view(dtype).view(self.shape)

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.bytes:] == FILL).all())

    def np(self):
        return self.t.cpu().numpy()

    def untouched(self, first=0):
        """Every element from flat position `first` on still holds the fill."""
        size = self.t.element_size()
        return bool((self.buf[GUARD + first * size:GUARD + self.bytes] == FILL).all())


def P(t, offset=0):
    from gcl_amd import _lib
    t = t.t if isinstance(t, Guarded) else t
    if t is None:
        return None
    return ctypes.c_void_p(_lib.ptr(t).value + offset * t.element_size()) if offset else _lib.ptr(t)


def STREAM():
    from gcl_amd import _lib
    return _lib.stream()


def ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.gcl_last_error())


def refused(lib, rc, name):
    msg = lib.gcl_last_error()
    assert rc == ERR_ARG and msg and name in msg.decode(), (name, rc, msg)


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype).to(DEV)          # a copy: the scenes are read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def device_table(lib, coords):
    """gcl_coords_insert of the scene's coordinates; the status words must be clean."""
    n, cap = len(coords), pow2_cap(len(coords))
    table, status, Cd = Guarded((cap, 2), I64), Guarded(4), dev(coords, I32)
    ok(lib, lib.gcl_coords_insert(P(Cd), n, P(table), cap, P(status), STREAM()), "gcl_coords_insert")
    torch.cuda.synchronize()
    assert table.intact() and status.intact() and status.np().tolist() == [0, 0, 0, 0]
    return table, cap


def host_doubles(a):
    a = np.array(a, dtype=np.float64).reshape(-1)
    return a, a.ctypes.data_as(PD)


def emit_call(lib, hits, cnt, rng, n, n_clouds, K):
    """gcl_colocation_emit on device inputs -> the guarded outputs, guards and scratch checked."""
    cap = max(n * n_clouds * K, 1)
    out = dict(scratch=Guarded(4 * n + lib.gcl_scan_scratch_len(n)), group=Guarded(n), index=Guarded(cap, I64),
               finest=Guarded(cap, U8), totals=Guarded(2))
    ok(lib, lib.gcl_colocation_emit(P(hits), P(cnt), P(rng), n, n_clouds, K, P(out["scratch"]), P(out["group"]), P(out["index"]),
                                    P(out["finest"]), P(out["totals"]), STREAM()), "gcl_colocation_emit")
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), k
    return out


def check_emit(out, want, tag):
    group, index, finest, (g, e) = want
    assert out["totals"].np().tolist() == [g, e], tag
    assert np.array_equal(out["group"].np()[:g], group) and out["group"].untouched(g), tag
    assert np.array_equal(out["index"].np()[:e], index) and out["index"].untouched(e), tag
    assert np.array_equal(out["finest"].np()[:e], finest) and out["finest"].untouched(e), tag
    return out["group"].np()[:g], out["index"].np()[:e], out["finest"].np()[:e]


# ---------------------------------------------------------------------------------------------------------------
# gcl_colocation_hits, then gcl_colocation_emit on its outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in S.HITS_CASES])
def test_hits_then_emit_equal_the_reference(lib, name):
    _, _, _, voxel, radius, K = next(c for c in S.HITS_CASES if c[0] == name)
    s, (hits, cnt, rng), emit, _ = S.scene_of(name)
    n, nc = s["n_center"], s["n_clouds"]
    own, cf = dev(s["xyz_own"], F32), dev(s["xyz_cf"], F32)
    table, cap = device_table(lib, s["coords"])
    keep, to_cloud = host_doubles(s["to_cloud"])
    runs = []
    for _ in range(2):
        h, c, r = Guarded((n, nc, K)), Guarded((n, nc)), Guarded((n, nc), F64)
        ok(lib, lib.gcl_colocation_hits(P(own), P(cf), n, nc, to_cloud, P(table), cap, S.inv_voxel(voxel), float(radius), K,
                                        P(h), P(c), P(r), STREAM()), "gcl_colocation_hits")
        torch.cuda.synchronize()
        assert h.intact() and c.intact() and r.intact() and table.intact()
        got_h, got_c, got_r = h.np(), c.np(), r.np()
        wrong = np.nonzero((got_h != hits).any(2) | (got_c != cnt))
        assert np.array_equal(got_c, cnt) and np.array_equal(got_h, hits), (name, len(wrong[0]), wrong[0][:8], wrong[1][:8])
        assert np.array_equal(bits(got_r), bits(rng)), name
        out = emit_call(lib, h.t, c.t, r.t, n, nc, K)
        runs.append((got_h, got_c, bits(got_r)) + check_emit(out, emit, name))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_hits_at_writes_each_sample_of_a_batch_into_its_slice(lib):
    """Three samples in one coordinate table, each written by its own gcl_colocation_hits_at call (row0, cloud0) into its slice
    of shared buffers, in an order that is not the samples': the other slices keep what they held.  The emit stage then runs
    over all of them at once."""
    b = S.batch_scene()
    K, nc = S.BATCH_K, S.BATCH_CLOUDS
    own, cf = dev(b["xyz_own"], F32), dev(b["xyz_cf"], F32)
    table, cap = device_table(lib, b["coords"])
    want = [S.hits_reference(b["xyz_own"], b["xyz_cf"], m["starts"], m["n_center"], m["row0"], m["radius"], K) for m in b["samples"]]
    first = np.concatenate([[0], np.cumsum([m["n_center"] for m in b["samples"]])])
    nct = int(first[-1])
    runs = []
    for _ in range(2):
        h, c, r = Guarded((nct, nc, K)), Guarded((nct, nc)), Guarded((nct, nc), F64)
        state = [h.np().copy(), c.np().copy(), bits(r.np()).copy()]
        for si in (1, 2, 0):
            m, c0 = b["samples"][si], int(first[si])
            keep, to_cloud = host_doubles(m["to_cloud"])
            ok(lib, lib.gcl_colocation_hits_at(P(own), P(cf), m["row0"], m["n_center"], m["cloud0"], nc, to_cloud, P(table), cap,
                                               S.inv_voxel(b["voxel"]), m["radius"], K, P(h, c0 * nc * K), P(c, c0 * nc),
                                               P(r, c0 * nc), STREAM()), "gcl_colocation_hits_at")
            torch.cuda.synchronize()
            assert h.intact() and c.intact() and r.intact()
            rows = slice(c0, c0 + m["n_center"])
            state[0][rows], state[1][rows], state[2][rows] = want[si][0], want[si][1], bits(want[si][2])
            assert np.array_equal(h.np(), state[0]) and np.array_equal(c.np(), state[1]), si
            assert np.array_equal(bits(r.np()), state[2]), si
        all_hits, all_cnt, all_rng = (np.concatenate([w[k] for w in want]) for k in range(3))
        out = emit_call(lib, h.t, c.t, r.t, nct, nc, K)
        runs.append(tuple(state) + check_emit(out, S.emit_reference(all_hits, all_cnt, all_rng), "batch"))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------
# gcl_colocation_emit alone
# ---------------------------------------------------------------------------------------------------------------
def emit_alone(lib, n, nc, K):
    hits, cnt, rng = S.emit_inputs(1000 * nc + K + n % 1000, n, nc, K)
    want = S.emit_reference(hits, cnt, rng)
    hd, cd, rd = dev(hits, I32), dev(cnt, I32), dev(rng, F64)
    runs = [check_emit(emit_call(lib, hd, cd, rd, n, nc, K), want, (n, nc, K)) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    if nc == 1:
        assert want[3] == (0, 0)
    return want


@pytest.mark.parametrize("n", S.EMIT_ROWS)
def test_emit_every_scan_shape_cloud_count_and_K(lib, n):
    """Synthetic outputs of the hits stage: rows without hits, rows without neighbour hits, range ties also in clouds without
    hits; 8192 rows scan in one launch, 8193 in two."""
    groups = 0
    for nc in S.EMIT_CLOUDS:
        for K in S.EMIT_K:
            groups += emit_alone(lib, n, nc, K)[3][0]
    assert groups > 0 or n == 1


def test_emit_524289_rows_scan_in_three_launches(lib):
    n, nc, K = S.EMIT_BIG
    assert emit_alone(lib, n, nc, K)[3][0] > n // 4


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_function_and_write_nothing(lib):
    name = "random-R1-K5"
    _, _, _, voxel, radius, K = next(c for c in S.HITS_CASES if c[0] == name)
    s, (hits, cnt, rng), _, _ = S.scene_of(name)
    n, nc = s["n_center"], s["n_clouds"]
    own, cf = dev(s["xyz_own"], F32), dev(s["xyz_cf"], F32)
    table, cap = device_table(lib, s["coords"])
    keep, to_cloud = host_doubles(np.concatenate([s["to_cloud"]] * 9)[:17])
    h, c, r = Guarded((n, 17, S.KMAX + 1)), Guarded((n, 17)), Guarded((n, 17), F64)
    # xyz_own, xyz_cf, row0, n_center, cloud0, n_clouds, to_cloud, table, cap, inv_voxel, radius, K, hits, cnt, first_rng
    good = [P(own), P(cf), 0, n, 0, nc, to_cloud, P(table), cap, S.inv_voxel(voxel), float(radius), K, P(h), P(c), P(r)]
    bad = {"K = 0": {11: 0}, "K = 9": {11: S.KMAX + 1}, "0 clouds": {5: 0}, "17 clouds": {5: 17}, "n_center = 0": {3: 0},
           "radius = 0": {10: 0.0}, "radius < 0": {10: -radius}, "inv_voxel = 0": {9: 0.0}, "inv_voxel < 0": {9: -1.0},
           "R = 5": {9: S.inv_voxel(S.REFUSED[0]), 10: S.REFUSED[1]}, "row0 < 0": {2: -1}, "cloud0 < 0": {4: -1},
           "cloud0 + n_clouds > 65535": {4: 65536 - nc}}
    bad.update({f"null pointer {i}": {i: None} for i in (0, 1, 6, 7, 12, 13, 14)})
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        refused(lib, lib.gcl_colocation_hits_at(*args, STREAM()), "gcl_colocation_hits")
        if not {2, 4} & set(change):                                        # the form without offsets refuses the same
            refused(lib, lib.gcl_colocation_hits(*(args[:2] + [args[3]] + args[5:]), STREAM()), "gcl_colocation_hits")
    args = list(good)
    args[9], args[10] = S.inv_voxel(S.REFUSED[0]), S.REFUSED[1]
    refused(lib, lib.gcl_colocation_hits_at(*args, STREAM()), "R = 5")
    torch.cuda.synchronize()
    assert all(g.untouched() and g.intact() for g in (h, c, r))
    args = list(good)
    args[4] = 65535 - nc                                                    # the last cloud ids that pack are accepted
    ok(lib, lib.gcl_colocation_hits_at(*args, STREAM()), "cloud0 + n_clouds == 65535")
    torch.cuda.synchronize()
    assert (h.np().reshape(-1)[:n * nc * K] == -1).all() and (c.np().reshape(-1)[:n * nc] == 0).all()      # no such cloud in the table
    assert h.intact() and c.intact() and r.intact()

    # gcl_colocation_emit: hits, cnt, first_rng, n_center, n_clouds, K, scratch, group, index, finest, totals
    hd, cd, rd = dev(hits, I32), dev(cnt, I32), dev(rng, F64)
    out = [Guarded(4 * n + lib.gcl_scan_scratch_len(n)), Guarded(n), Guarded(n * nc * K, I64), Guarded(n * nc * K, U8), Guarded(2)]
    good = [P(hd), P(cd), P(rd), n, nc, K] + [P(g) for g in out]
    bad = {"K = 0": {5: 0}, "K = 9": {5: S.KMAX + 1}, "0 clouds": {4: 0}, "n_center = 0": {3: 0}}
    bad.update({f"null pointer {i}": {i: None} for i in (0, 1, 2, 6, 7, 8, 9, 10)})
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        refused(lib, lib.gcl_colocation_emit(*args, STREAM()), "gcl_colocation_emit")
    torch.cuda.synchronize()
    assert all(g.untouched() and g.intact() for g in out)


# ---------------------------------------------------------------------------------------------------------------
# key-less loaders
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", S.VOXELS)
def test_voxel_coords_floor_of_the_float32_division(lib, voxel):
    """+-0.0, tiny negatives, multiples of the voxel and their float32 neighbours, and values whose floor differs when the
    division is replaced by a multiplication with the reciprocal (counted in tests/test_oracle_colocation.py)."""
    for p in S.VOXEL_POINTS:
        xyz = S.voxel_inputs(voxel, p)
        want = np.concatenate([np.full((p, 1), 7, np.int32), S.voxel_reference(xyz, voxel)], axis=1)
        xd, runs = dev(xyz, F32), []
        for _ in range(2):
            coords = Guarded((p, 4))
            ok(lib, lib.gcl_voxel_coords(P(xd), p, voxel, 7, P(coords), STREAM()), "gcl_voxel_coords")
            torch.cuda.synchronize()
            assert coords.intact()
            bad = np.nonzero((coords.np() != want).any(1))[0]
            assert len(bad) == 0, (voxel, p, xyz[bad[:4]], coords.np()[bad[:4]], want[bad[:4]])
            runs.append(coords.np())
        assert np.array_equal(*runs)


@pytest.mark.parametrize("p", (255, 5000))
def test_voxel_coords_multi_cloud_of_every_point(lib, p):
    from gcl_amd import _lib
    voxel = 0.3
    xyz = S.voxel_inputs(voxel, p, seed=1)
    xd = dev(xyz, F32)
    for name, off in S.multi_offsets(p).items():
        want = np.concatenate([S.cloud_of_point(off, p)[:, None], S.voxel_reference(xyz, voxel)], axis=1)
        runs = []
        for _ in range(2):
            coords = Guarded((p, 4))
            ok(lib, lib.gcl_voxel_coords_multi(P(xd), p, _lib.host_i64(off), len(off) - 1, voxel, P(coords), STREAM()), name)
            torch.cuda.synchronize()
            assert coords.intact() and np.array_equal(coords.np(), want), name
            runs.append(coords.np())
        assert np.array_equal(*runs)
    coords = Guarded((p, 4))
    off65 = np.linspace(0, p, 66).astype(np.int64).tolist()
    for off in (off65, [1, p], [0, p // 2, p - 1], [0, p // 2, p + 1]):
        refused(lib, lib.gcl_voxel_coords_multi(P(xd), p, _lib.host_i64(off), len(off) - 1, voxel, P(coords), STREAM()),
                "gcl_voxel_coords_multi")
    torch.cuda.synchronize()
    assert coords.untouched() and coords.intact()


@pytest.mark.parametrize("n_max,n_dev", [(1, 1), (257, 256), (1000, 700)])
def test_cloud_row_starts_below_the_row_bound(lib, n_max, n_dev):
    """Clouds 0, 3 and 7 (the last) have no rows: -1.  Rows from *n_dev on hold other cloud ids, out of order."""
    n_clouds = 8
    rng = np.random.RandomState(n_max)
    ids = np.sort(rng.choice([1, 2, 4, 5, 6], n_dev)).astype(np.int32) if n_dev > 1 else np.asarray([5], np.int32)
    tail = rng.choice([7, 3, 0, 6], n_max - n_dev).astype(np.int32)
    coords = rng.randint(-50, 50, (n_max, 4)).astype(np.int32)
    coords[:, 0] = np.concatenate([ids, tail])
    want = S.row_starts_reference(ids, n_clouds)
    assert want[n_clouds] == n_dev and (want[[0, 3, 7]] == -1).all() and ((want >= 0).sum() >= 5 or n_dev == 1)
    cd, nd, runs = dev(coords, I32), dev([n_dev], I32), []
    for _ in range(2):
        starts = Guarded(n_clouds + 1)
        ok(lib, lib.gcl_cloud_row_starts(P(cd), n_max, P(nd), n_clouds, P(starts), STREAM()), "gcl_cloud_row_starts")
        torch.cuda.synchronize()
        assert starts.intact() and np.array_equal(starts.np(), want), (starts.np(), want)
        runs.append(starts.np())
    assert np.array_equal(*runs)


def test_loader_points_unfused_fp64_transform(lib):
    """xyz_own = the raw point, xyz_cf = fp32(((x m0 + y m1) + z m2) + t) in fp64, bit for bit, on points where a contracted
    product changes the float32 result (tests/test_oracle_colocation.py counts them); rows from *n_dev on stay untouched."""
    raw, index, coords, M = S.loader_points_scene()
    n_max, n_dev = len(index), 700
    want_own, want_cf = S.loader_points_reference(raw, index, coords, M)
    rd, idx, cd, md, nd = dev(raw, F32), dev(index, I64), dev(coords, I32), dev(M, F64), dev([n_dev], I32)
    runs = []
    for _ in range(2):
        own, cf = Guarded((n_max, 3), F32), Guarded((n_max, 3), F32)
        ok(lib, lib.gcl_loader_points(P(rd), P(idx), P(cd), n_max, P(nd), P(md), P(own), P(cf), STREAM()), "gcl_loader_points")
        torch.cuda.synchronize()
        assert own.intact() and cf.intact() and own.untouched(3 * n_dev) and cf.untouched(3 * n_dev)
        assert np.array_equal(bits(own.np()[:n_dev]), bits(want_own[:n_dev]))
        bad = np.nonzero(bits(cf.np()[:n_dev]) != bits(want_cf[:n_dev]))
        assert len(bad[0]) == 0, (len(bad[0]), cf.np()[:n_dev][bad][:4], want_cf[:n_dev][bad][:4])
        runs.append(bits(cf.np()))
    assert np.array_equal(*runs)
