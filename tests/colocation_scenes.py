"""Scenes, case tables and numpy references of the co-location group kernels (csrc/data.hip: k_colocation_hits,
k_colocation_sizes / k_colocation_emit) and of the key-less loader kernels beside them.  No GPU, no torch.

The references restate the kernels' documented results the plain way: brute-force fp64 squared distances from the float32
centre-frame points, `(ex*ex + ey*ey) + ez*ez` as separate numpy operations (numpy does not fuse them), strictly inside
the radius, ascending (d2, row), the first K.  tests/test_oracle_colocation.py pins them to oracle/colocation_oracle.py (a
loop over the centre points) and asserts the conditions each scene exists for; tests/test_gpu_colocation_kernels.py runs
the kernels on the same tables.  Every scene is seeded and deterministic."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64
KMAX, LANES = 8, 8               # csrc/data.hip: KMAX, HITS_LANES
NO_RANGE = 1e300                 # first_rng of a neighbour cloud without hits


def inv_voxel(voxel):
    """The float the callers pass: fp32 of the fp64 reciprocal."""
    return float(F32(1.0 / voxel))


def abi_R(radius, voxel):
    """R as gcl_colocation_hits_at computes it."""
    return int(float(radius) * inv_voxel(voxel)) + 1


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def own_range(p):
    p = np.asarray(p, dtype=F64)
    a, b, c = p[..., 0], p[..., 1], p[..., 2]
    return np.sqrt((a * a + b * b) + c * c)


def sorted_d2(xyz_cf, a, b, row0, n_center, radius):
    """Per query: squared distances to the rows a .. b - 1, ascending (d2, row) with everything not strictly inside the radius
    moved to +inf -> (sorted d2 [n_center, b - a], rows in that order, number inside, number at d2 == radius^2 exactly)."""
    Q = np.asarray(xyz_cf[row0:row0 + n_center], dtype=F64)
    P = np.asarray(xyz_cf[a:b], dtype=F64)
    ex = P[None, :, 0] - Q[:, None, 0]
    ey = P[None, :, 1] - Q[:, None, 1]
    ez = P[None, :, 2] - Q[:, None, 2]
    d2 = (ex * ex + ey * ey) + ez * ez
    r2 = float(radius) * float(radius)
    inside = d2 < r2
    on_sphere = (d2 == r2).sum(1)
    d2 = np.where(inside, d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")            # stable: equal d2 stay in ascending row order
    return np.take_along_axis(d2, order, 1), order + a, inside.sum(1), on_sphere


def hits_reference(xyz_own, xyz_cf, starts, n_center, row0, radius, K, stats=None):
    """hits [n_center, n_clouds, K] (rows of xyz_*, -1 padded), cnt [n_center, n_clouds], first_rng [n_center, n_clouds] of the
    queries row0 .. row0 + n_center - 1 against the clouds starts[c] .. starts[c + 1] - 1.  `stats` (a dict) receives the
    per-(query, cloud) number of points inside the radius, the number exactly on it and whether the K-th place is tied."""
    n_clouds = len(starts) - 1
    hits = np.full((n_center, n_clouds, K), -1, np.int32)
    cnt = np.zeros((n_center, n_clouds), np.int32)
    rng = np.full((n_center, n_clouds), NO_RANGE, F64)
    inside = np.zeros((n_center, n_clouds), np.int64)
    sphere = np.zeros((n_center, n_clouds), np.int64)
    tied = np.zeros((n_center, n_clouds), bool)
    for c in range(n_clouds):
        a, b = int(starts[c]), int(starts[c + 1])
        if b > a:
            d2, rows, n_in, on = sorted_d2(xyz_cf, a, b, row0, n_center, radius)
            k = min(K, b - a)
            cnt[:, c] = np.minimum(n_in, K)
            hits[:, c, :k] = np.where(np.arange(k)[None, :] < cnt[:, c, None], rows[:, :k], -1)
            inside[:, c], sphere[:, c] = n_in, on
            if b - a > K:
                tied[:, c] = (n_in > K) & (d2[:, K - 1] == d2[:, K])
            if c > 0:
                has = cnt[:, c] > 0
                rng[has, c] = own_range(xyz_own[rows[has, 0]])
        if c == 0:
            rng[:, 0] = own_range(xyz_own[row0:row0 + n_center])
    if stats is not None:
        stats.update(inside=inside, sphere=sphere, tied=tied)
    return hits, cnt, rng


def emit_reference(hits, cnt, first_rng):
    """(group int32 [G], index int64 [E], finest uint8 [E], totals (G, E)) from the hits stage's outputs alone: a centre row
    makes a group only when some neighbour cloud has a hit; members are cloud-major; the finest member is the first one of the
    first arg-min (strict <) of [centre range, nearest-hit range of every neighbour cloud WITH hits]."""
    n, n_clouds, K = hits.shape
    cnt = np.asarray(cnt, dtype=np.int64)
    kept = cnt[:, 1:].sum(1) > 0
    size = cnt.sum(1)[kept]
    member = np.arange(K)[None, None, :] < cnt[:, :, None]
    index = hits[kept][member[kept]].astype(np.int64)                  # C order: cloud-major, then nearest first
    r = np.array(first_rng, dtype=F64)
    r[:, 1:][cnt[:, 1:] == 0] = np.inf
    best = np.argmin(r, axis=1)                                        # the FIRST minimum
    before = np.cumsum(cnt, axis=1) - cnt
    fpos = np.where(best == 0, 0, before[np.arange(n), best])[kept]
    off = np.cumsum(size) - size
    finest = np.zeros(int(size.sum()), np.uint8)
    finest[off + fpos] = 1
    return size.astype(np.int32), index, finest, (int(kept.sum()), int(size.sum()))


def finest_ties(cnt, first_rng):
    """Per centre row with a group: (the minimum range is the centre's AND some neighbour's, the minimum is below the centre's
    and reached by two or more neighbours)."""
    cnt = np.asarray(cnt)
    kept = cnt[:, 1:].sum(1) > 0
    r = np.array(first_rng, dtype=F64)
    r[:, 1:][cnt[:, 1:] == 0] = np.inf
    low = r.min(1)
    at_low = r[:, 1:] == low[:, None]
    return kept & (r[:, 0] == low) & at_low.any(1), kept & (r[:, 0] > low) & (at_low.sum(1) >= 2)


# ---------------------------------------------------------------------------------------------------------------
# scene building blocks
# ---------------------------------------------------------------------------------------------------------------
def voxel_of(own, voxel):
    return np.floor(np.asarray(own, dtype=F32) / F32(voxel)).astype(np.int32)          # float32 division, as the loaders


def one_per_voxel(own, voxel):
    """The first point of every voxel, in input order."""
    _, first = np.unique(voxel_of(own, voxel), axis=0, return_index=True)
    return own[np.sort(first)]


def to_centre_frame(own, M):
    """((x m0 + y m1) + z m2) + t in fp64 from the float32 points, rounded to float32 (k_loader_points)."""
    x, y, z = (np.asarray(own[:, k], dtype=F64) for k in range(3))
    M = np.asarray(M, dtype=F64)
    return np.stack([((x * M[k, 0] + y * M[k, 1]) + z * M[k, 2]) + M[k, 3] for k in range(3)], axis=1).astype(F32)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rigid(rot, t, about=None):
    """4 x 4 of x -> rot (x - about) + about + t."""
    M = np.eye(4)
    M[:3, :3] = rot
    about = np.zeros(3) if about is None else np.asarray(about, dtype=F64)
    M[:3, 3] = about - rot @ about + np.asarray(t, dtype=F64)
    return M


def grid_rotations():
    """The 24 rotations that map the voxel grid onto itself."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in np.ndindex(2, 2, 2):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = 1.0 - 2.0 * signs[r]
            if np.linalg.det(m) > 0:
                out.append(m)
    return out


def assemble(clouds_own, list_M, voxel, rng, cloud0=0):
    """clouds_own: float32 [n_c, 3] per cloud (centre first, one point per voxel); list_M: neighbour -> centre 4 x 4.  Rows of
    every cloud are shuffled; returns the tables the ABI takes."""
    own, cf, coords, starts = [], [], [], [0]
    for c, pts in enumerate(clouds_own):
        pts = np.ascontiguousarray(pts, dtype=F32)[rng.permutation(len(pts))]
        v = voxel_of(pts, voxel)
        assert len(np.unique(v, axis=0)) == len(pts), "one point per voxel"
        own.append(pts)
        cf.append(pts.copy() if c == 0 else to_centre_frame(pts, list_M[c - 1]))
        coords.append(np.concatenate([np.full((len(pts), 1), cloud0 + c, np.int32), v], axis=1))
        starts.append(starts[-1] + len(pts))
    to_cloud = np.zeros((len(clouds_own), 12), F64)
    to_cloud[0] = np.eye(4)[:3].reshape(-1)
    for j, M in enumerate(list_M):
        to_cloud[j + 1] = np.linalg.inv(np.asarray(M, dtype=F64))[:3].reshape(-1)          # as colocation_data_gpu makes them
    return dict(xyz_own=np.concatenate(own), xyz_cf=np.concatenate(cf), coords=np.concatenate(coords).astype(np.int32),
                list_M=[np.asarray(M, dtype=F64) for M in list_M], to_cloud=to_cloud, starts=np.asarray(starts, np.int64),
                n_center=len(clouds_own[0]), n_clouds=len(clouds_own), voxel=voxel)


def apply64(M, x):
    return np.asarray(x, dtype=F64) @ M[:3, :3].T + M[:3, 3]


# ---------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------
CUBE = 2.0          # half side of the random scenes, metres


def random_scene(seed, n_clouds, n_pts, n_center, voxel=0.3, cloud0=0):
    """Uniform points in a cube of +-2 m around the centre frame's origin.  Neighbour transforms: any rotation, translations of
    up to 3 voxels.  From three clouds on, cloud 1 covers only x > 0 of the centre frame; from four clouds on, the last one is
    translated 50 voxels away and has no hit at all."""
    rng = np.random.RandomState(seed)
    if n_center == 1:
        centre = rng.uniform(-0.2, 0.2, (1, 3)).astype(F32)
    else:
        centre = one_per_voxel(rng.uniform(-CUBE, CUBE, (4 * n_center + 64, 3)).astype(F32), voxel)[:n_center]
    assert len(centre) == n_center
    clouds, list_M = [centre], []
    for j in range(1, n_clouds):
        M = rigid(random_rotation(rng), rng.uniform(-3, 3, 3) * voxel)
        pts = rng.uniform(-CUBE, CUBE, (3 * n_pts, 3))
        if n_clouds >= 3 and j == 1:
            pts[:, 0] = np.abs(pts[:, 0])
        if n_clouds >= 4 and j == n_clouds - 1:
            pts[:, 0] += 50 * voxel
        own = apply64(np.linalg.inv(M), pts).astype(F32)
        clouds.append(one_per_voxel(own, voxel)[:n_pts])
        list_M.append(M)
    return assemble(clouds, list_M, voxel, rng, cloud0)


LATTICE_VOXEL = 0.25
LATTICE_LO, LATTICE_HI = -4, 8          # voxels per axis: 12^3 = 1728 lattice points, negative coordinates included


def lattice_scene(seed, n_center, voxel=LATTICE_VOXEL):
    """Every point at a voxel centre (v + 0.5) * 0.25 of its own frame; neighbour -> centre transforms are rotations of the grid
    with translations that are multiples of 0.125, so every centre-frame point and every d2 is exact and ties are exact.
    Clouds 1 and 2: untranslated rotations -- their points coincide with centre points and have the centre point's own-frame
    range (ties the centre with a neighbour, and two neighbours with each other).  Clouds 3 and 4: translated by 0.5 m along x
    and along y -- for centre points with x == y > 0.25 their coincident points tie and both beat the centre.  Cloud 5:
    translated by an odd multiple of 0.125, its points lie on the corners of the centre's voxels.  Every neighbour cloud
    misses a random tenth of the lattice."""
    assert voxel == LATTICE_VOXEL
    rng = np.random.RandomState(seed)
    v = np.stack(np.meshgrid(*[np.arange(LATTICE_LO, LATTICE_HI)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lattice = (v + 0.5) * voxel                                              # exact in float32
    rots = grid_rotations()
    centre = lattice[rng.permutation(len(lattice))[:n_center]].astype(F32)
    clouds, list_M = [centre], []
    for j, t in enumerate(([0, 0, 0], [0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.125, -0.375, 0.625])):
        M = rigid(rots[(5 + 7 * j + seed) % 24], t)
        keep = lattice[rng.rand(len(lattice)) >= 0.1]
        cf = keep + np.asarray(t)                                            # centre-frame points: the lattice, shifted by t
        own = apply64(np.linalg.inv(M), cf)                                  # exact: a signed permutation of exact values
        assert np.array_equal(own.astype(F32).astype(F64), own)
        clouds.append(own.astype(F32))
        list_M.append(M)
    s = assemble(clouds, list_M, voxel, rng)
    for c in range(1, s["n_clouds"]):                                       # the float32 transform was exact
        a, b = s["starts"][c], s["starts"][c + 1]
        assert np.array_equal(s["xyz_cf"][a:b].astype(F64), apply64(list_M[c - 1], s["xyz_own"][a:b]))
    return s


def corner_f32(v, voxel):
    """Per element the smallest float32 h with floor(h / float32(voxel)) == v."""
    vox = F32(voxel)
    h = (np.asarray(v, dtype=F64) * float(vox)).astype(F32)
    for _ in range(8):
        low = np.floor(h / vox) < v
        h = np.where(low, np.nextafter(h, F32(np.inf)), h)
    for _ in range(8):
        down = np.nextafter(h, F32(-np.inf))
        h = np.where(np.floor(down / vox) == v, down, h)
    assert (np.floor(h / vox) == v).all() and (np.floor(np.nextafter(h, F32(-np.inf)) / vox) == v - 1).all()
    return h


CORNER_VOXEL, CORNER_RADIUS = 0.3, 0.45


def corner_scene(seed, offset, n_pts=1000, voxel=CORNER_VOXEL, radius=CORNER_RADIUS):
    """One neighbour cloud whose own-frame points sit on the low corners of their voxels, around `offset` voxels on every axis,
    and one query per point just inside the radius along a direction of the positive octant: the hit's voxel box is as far
    from the query as a box holding a hit can be, which is where k_colocation_hits' box test decides.  The neighbour -> centre
    transform is a random rotation about the offset point plus a translation of up to 2 voxels, so both frames stay within a
    few voxels of the offset."""
    rng = np.random.RandomState(seed)
    v = np.unique(rng.randint(-6, 7, (2 * n_pts, 3)), axis=0)
    v = v[rng.permutation(len(v))[:n_pts]] + offset
    h = corner_f32(v, voxel)
    M = rigid(random_rotation(rng), rng.uniform(-2, 2, 3) * voxel, about=np.full(3, offset * voxel))
    n = len(h)
    u = np.abs(rng.standard_normal((n, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    axis = np.eye(3)[rng.randint(0, 3, n)]
    u = np.where((np.arange(n) % 2 == 0)[:, None], axis, u)
    eps = 10.0 ** rng.uniform(-8, -4, n)
    q_own = h.astype(F64) - (radius * (1.0 - eps))[:, None] * u
    centre = one_per_voxel(apply64(M, q_own).astype(F32), voxel)
    return assemble([centre, h], [M], voxel, rng)


def mirror_scene(seed, n_center, n_pairs=375, voxel=0.3):
    """Every query lies on the plane x == y and the one neighbour cloud (identity transform) holds its points in pairs (u, v, w)
    and (v, u, w): the two are exactly equidistant from every query when each product of (ex ex + ey ey) + ez ez is rounded --
    ex and ey swap, and the sum of two rounded squares commutes -- so the lower row comes first.  Under contraction one square
    enters the sum unrounded and the two distances differ in their last bit wherever that square is not exact: the queries
    keep |x| = |y| between 0.001 and 0.29 (a column of voxels along z), well below the neighbours' coordinates, so that ex has
    more than 26 significant bits.  A kernel that fuses orders such a pair by that bit instead of by row."""
    rng = np.random.RandomState(seed)
    t = (rng.choice([-1.0, 1.0], 8 * n_center) * 10.0 ** rng.uniform(-3, np.log10(0.29), 8 * n_center)).astype(F32)
    z = rng.uniform(-15, 15, 8 * n_center).astype(F32)
    centre = one_per_voxel(np.stack([t, t, z], 1), voxel)[:n_center]
    assert len(centre) == n_center
    p = rng.uniform([-1.3, -1.3, -15], [1.3, 1.3, 15], (3 * n_pairs, 3)).astype(F32)
    both = np.stack([p, p[:, [1, 0, 2]]], 1)                                   # [pair, 2, 3]
    vox = voxel_of(both.reshape(-1, 3), voxel)
    _, first, count = np.unique(vox, axis=0, return_index=True, return_counts=True)
    alone = np.zeros(len(vox), bool)
    alone[first[count == 1]] = True
    both = both[alone.reshape(-1, 2).all(1)][:n_pairs]                         # pairs whose two voxels nobody else is in
    assert len(both) == n_pairs
    s = assemble([centre, both.reshape(-1, 3)], [np.eye(4)], voxel, rng)
    assert np.array_equal(s["xyz_cf"], s["xyz_own"])
    return s


def fused_d2(e, variant):
    """fp64 d2 of the fp64 difference e = (ex, ey, ez) when the products are contracted, exactly rounded per fused operation:
    variant 0: fma(ez, ez, fma(ey, ey, ex ex)), variant 1: fma(ez, ez, fma(ex, ex, ey ey))."""
    ex, ey, ez = (Fraction(float(v)) for v in (e if variant == 0 else (e[1], e[0], e[2])))
    s = float(ey * ey + Fraction(float(ex * ex)))
    return float(ez * ez + Fraction(s))


def mirror_swaps(s, hits, cnt, variant):
    """Queries whose list of hits in cloud 1 would change under fused_d2: two neighbouring hits tie exactly in the reference and
    the fused distances put the higher row first."""
    n, changed = s["n_center"], 0
    cf = np.asarray(s["xyz_cf"], dtype=F64)
    for i in range(n):
        rows = hits[i, 1, :cnt[i, 1]]
        e = cf[rows] - cf[i]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        for j in range(len(rows) - 1):
            if d2[j] == d2[j + 1] and fused_d2(e[j], variant) > fused_d2(e[j + 1], variant):
                changed += 1
                break
    return changed


BATCH_SAMPLES = ((101, 33, 0.28), (102, 257, 0.45), (103, 100, 0.75))       # (seed, centre rows, radius) of the batch's samples
BATCH_CLOUDS, BATCH_K, BATCH_VOXEL = 3, 5, 0.3


def batch_scene():
    """Three random samples of 3 clouds each behind one another: one coordinate table with batch ids si * 3 + c."""
    parts = [random_scene(seed, BATCH_CLOUDS, 500, n_center, BATCH_VOXEL, cloud0=si * BATCH_CLOUDS)
             for si, (seed, n_center, _) in enumerate(BATCH_SAMPLES)]
    row, samples = 0, []
    for si, p in enumerate(parts):
        samples.append(dict(row0=row, cloud0=si * BATCH_CLOUDS, n_center=p["n_center"], starts=p["starts"] + row,
                            to_cloud=p["to_cloud"], radius=BATCH_SAMPLES[si][2], part=p))
        row += len(p["xyz_own"])
    return dict(xyz_own=np.concatenate([p["xyz_own"] for p in parts]), xyz_cf=np.concatenate([p["xyz_cf"] for p in parts]),
                coords=np.concatenate([p["coords"] for p in parts]), samples=samples, voxel=BATCH_VOXEL)


def emit_inputs(seed, n_center, n_clouds, K, zero_rows=0.15, no_neighbour_rows=0.15):
    """Synthetic outputs of the hits stage: random counts 0 .. K, a share of rows without any hit and a share whose neighbour
    clouds have none (neither makes a group), arbitrary row numbers in `hits` -- also beyond a cloud's count, where nothing
    may read them -- and first ranges from five values, so that ties are frequent, also where a cloud has no hit."""
    rng = np.random.RandomState(seed)
    cnt = rng.randint(0, K + 1, (n_center, n_clouds)).astype(np.int32)
    kind = rng.rand(n_center)
    cnt[kind < zero_rows] = 0
    cnt[(kind >= zero_rows) & (kind < zero_rows + no_neighbour_rows), 1:] = 0
    hits = rng.randint(0, 1 << 30, (n_center, n_clouds, K)).astype(np.int32)
    first_rng = rng.choice(np.asarray([0.5, 1.0, 1.0, 2.0, 3.5]), (n_center, n_clouds))
    return hits, cnt, first_rng


# ---------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------
SQRT2_UP = float(np.nextafter(0.25 * np.sqrt(2.0), np.inf))       # 0.25 * sqrt(2), one ulp up: the 12 face diagonals are inside

# (name, scene, args, voxel, radius, K); random: (seed, n_clouds, points per neighbour cloud, centre rows), lattice: (seed,
# centre rows), corner: (seed, offset in voxels), mirror: (seed, centre rows)
HITS_CASES = [
    ("random-R1-K1", "random", (11, 3, 1200, 257), 0.3, 0.28, 1),
    ("random-R1-K5", "random", (12, 2, 1500, 33), 0.3, 0.28, 5),
    ("random-R1-K8", "random", (13, 3, 1500, 32), 0.3, 0.29, 8),
    ("random-R2-K5-16clouds", "random", (14, 16, 600, 33), 0.3, 0.45, 5),
    ("random-R2-K5-1cloud", "random", (15, 1, 0, 100), 0.3, 0.45, 5),
    ("random-R2-K8-1row", "random", (16, 3, 1200, 1), 0.3, 0.55, 8),
    ("random-R3-K8-1100rows", "random", (17, 3, 1200, 1100), 0.3, 0.75, 8),
    ("random-R4-K1", "random", (18, 3, 1200, 31), 0.3, 1.05, 1),
    ("random-R4-K5", "random", (19, 3, 1200, 257), 0.3, 1.05, 5),
    ("random-R4-K8", "random", (20, 2, 1500, 100), 0.3, 1.19, 8),
    ("lattice-r0.25-K5", "lattice", (31, 1728), 0.25, 0.25, 5),
    ("lattice-r0.5-K8", "lattice", (32, 257), 0.25, 0.5, 8),
    ("lattice-rsqrt2-K5", "lattice", (33, 257), 0.25, SQRT2_UP, 5),
    ("lattice-r0.8-K8", "lattice", (34, 300), 0.25, 0.8, 8),
    ("corner-0", "corner", (41, 0), CORNER_VOXEL, CORNER_RADIUS, 5),
    ("corner-400", "corner", (42, 400), CORNER_VOXEL, CORNER_RADIUS, 5),
    ("corner-30000", "corner", (43, 30000), CORNER_VOXEL, CORNER_RADIUS, 5),
    ("mirror-R4-K8", "mirror", (51, 180), 0.3, 1.19, 8),
]
KDTREE_CASES = ("random-R4-K5", "random-R3-K8-1100rows")       # random scenes: no exact ties, cKDTree's order is defined
REFUSED = (0.3, 1.25)                                            # (voxel, radius) with R = 5

EMIT_ROWS = (1, 255, 256, 257, 8192, 8193)                       # the one-launch scan up to 8192 rows, two launches beyond
EMIT_CLOUDS = (1, 2, 7, 16)
EMIT_K = (1, 5, 8)
EMIT_BIG = (524289, 2, 1)                                        # three launches

_BUILDERS = dict(random=random_scene, lattice=lattice_scene, corner=corner_scene, mirror=mirror_scene)


@lru_cache(maxsize=None)
def scene_of(name):
    """(scene, reference outputs of both stages, statistics) of a hits case; built once per process and left unchanged."""
    _, kind, args, voxel, radius, K = next(c for c in HITS_CASES if c[0] == name)
    s = _BUILDERS[kind](*args, voxel=voxel)
    stats = {}
    hits, cnt, rng = hits_reference(s["xyz_own"], s["xyz_cf"], s["starts"], s["n_center"], 0, radius, K, stats)
    for a in (hits, cnt, rng, *s.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s, (hits, cnt, rng), emit_reference(hits, cnt, rng), stats


def query_base_voxel(s, c):
    """floor(q * inv_voxel) of every query in the frame of cloud c, the way k_colocation_hits finds its candidate block (only
    used on the lattice, where every step is exact)."""
    m = s["to_cloud"][c].reshape(3, 4)
    q = (np.asarray(s["xyz_cf"][:s["n_center"]], dtype=F64) @ m[:, :3].T + m[:, 3]).astype(F32)
    return np.floor(q * F32(inv_voxel(s["voxel"]))).astype(np.int64)


def busiest_lane(s, c, radius, R):
    """Per query: the largest number of points of cloud c inside the radius whose voxels fall to ONE lane of the query's eight.
    Candidate number of the voxel at (dx, dy, dz) from the query's: ((dz + R) W + (dy + R)) W + (dx + R), W = 2 R + 1; the
    candidates are dealt round-robin, lane = number % 8."""
    a, b = int(s["starts"][c]), int(s["starts"][c + 1])
    base = query_base_voxel(s, c)
    vox = s["coords"][a:b, 1:].astype(np.int64)
    Q, P = np.asarray(s["xyz_cf"][:s["n_center"]], F64), np.asarray(s["xyz_cf"][a:b], F64)
    e = P[None] - Q[:, None]
    inside = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2] < radius * radius
    d = vox[None] - base[:, None]
    assert (np.abs(d)[inside] <= R).all()
    W = 2 * R + 1
    lane = ((((d[..., 2] + R) * W + (d[..., 1] + R)) * W + (d[..., 0] + R)) % LANES)
    return np.stack([(inside & (lane == l)).sum(1) for l in range(LANES)], 1).max(1)


def box_distance(s, voxel):
    """corner scenes: per (query, neighbour point) the fp64 distance, in voxels, from the query mapped into the neighbour's
    frame to the point's voxel box [v, v + 1) * float32(voxel)."""
    a, b = int(s["starts"][1]), int(s["starts"][2])
    m = s["to_cloud"][1].reshape(3, 4)
    q = (np.asarray(s["xyz_cf"][:s["n_center"]], dtype=F64) @ m[:, :3].T + m[:, 3]) / float(F32(voxel))
    v = s["coords"][a:b, 1:].astype(F64)
    gap = np.maximum(np.maximum(v[None] - q[:, None], q[:, None] - (v[None] + 1.0)), 0.0)
    return np.sqrt((gap * gap).sum(-1))


# ---------------------------------------------------------------------------------------------------------------
# key-less loaders
# ---------------------------------------------------------------------------------------------------------------
VOXELS = (0.3, 0.025, 0.05, 1.0)
VOXEL_POINTS = (1, 255, 257, 5000)


@lru_cache(maxsize=None)
def floor_mismatches(voxel, want=150):
    """float32 values x near multiples of the voxel for which floor(x * float32(1 / voxel)) != floor(x / float32(voxel)): what a
    kernel that multiplied by the reciprocal would get wrong.  None exist for a power of two."""
    vox, inv = F32(voxel), F32(1.0 / voxel)
    k = np.arange(-40000, 40001, dtype=F64)
    x = (k * float(vox)).astype(F32)
    up, down = np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))
    x = np.unique(np.concatenate([x, up, np.nextafter(up, F32(np.inf)), down, np.nextafter(down, F32(-np.inf))]))
    bad = x[np.floor(x * inv) != np.floor(x / vox)]
    return bad[np.linspace(0, len(bad) - 1, min(want, len(bad))).astype(np.int64)] if len(bad) else bad


def voxel_inputs(voxel, p, seed=0):
    """float32 [p, 3]: +-0.0, tiny negatives, k * voxel with its float32 neighbours on both sides, the floor mismatches of the
    voxel, and uniform values; in a seeded random order (the first rows of the specials survive when p is small)."""
    rng = np.random.RandomState(seed + p)
    k = rng.randint(-3000, 3001, 3 * p + 9).astype(F64)
    on = (k * float(F32(voxel))).astype(F32)
    special = np.concatenate([
        np.asarray([0.0, -0.0, -1e-45, -1e-38, -1e-7, 1e-45], dtype=F32), floor_mismatches(voxel),
        on[0::3], np.nextafter(on[1::3], F32(np.inf)), np.nextafter(on[2::3], F32(-np.inf))])
    vals = np.concatenate([special, rng.uniform(-50, 50, 3 * p).astype(F32)])[:max(3 * p, 3)]
    vals = vals[rng.permutation(len(vals))] if p > 2 else vals
    return np.ascontiguousarray(vals[:3 * p].reshape(p, 3))


def voxel_reference(xyz, voxel):
    return np.floor(xyz / F32(voxel)).astype(np.int32)


# cloud offsets of gcl_voxel_coords_multi over p points: empty clouds first, in the middle and last; one cloud; 64 clouds
def multi_offsets(p):
    cuts = sorted({0, p // 5, p // 2, (4 * p) // 5, p})
    return {
        "empty first/middle/last": [0, 0] + [c for c in cuts[1:-1] for _ in (0, 1)] + [p, p],
        "one cloud": [0, p],
        "64 clouds": np.linspace(0, p, 65).astype(np.int64).tolist(),
    }


def cloud_of_point(offsets, p):
    """The last cloud c with offsets[c] <= i."""
    return (np.searchsorted(np.asarray(offsets[:-1]), np.arange(p), side="right") - 1).astype(np.int32)


def row_starts_reference(cloud_ids, n_clouds):
    out = np.full(n_clouds + 1, -1, np.int32)
    out[n_clouds] = len(cloud_ids)
    for i in range(len(cloud_ids) - 1, -1, -1):
        if i == 0 or cloud_ids[i - 1] != cloud_ids[i]:
            out[cloud_ids[i]] = i
    return out


LOADER_CLOUDS = 3


@lru_cache(maxsize=None)
def loader_points_scene(seed=7, n_raw=1200, n_rows=900):
    """Raw points of three clouds, the rows (first points of voxels) that gcl_loader_points reads and the clouds' to-centre
    3 x 4 matrices.  Cloud 0 is the identity.  Clouds 1 and 2 are rotations; in cloud 1 the first row's translation is 0 and a
    third of its points are chosen so that x m0 + y m1 + z m2 cancels twice over: x = fl32(-y m1 / m0) leaves a sum 2^-24 of
    its terms, z = fl32(-(x m0 + y m1) / m2) leaves 2^-48.  The unfused fp64 evaluation then computes that remainder from the
    ROUNDED products, a fused one from an exact product, and the two differ in the leading bits of the float32 result: the
    only kind of point on which a bitwise float32 comparison can see a contraction (elsewhere the fp64 results differ in their
    last bit and round to the same float32)."""
    rng = np.random.RandomState(seed)
    M = np.zeros((LOADER_CLOUDS, 3, 4))
    M[0] = np.eye(4)[:3]
    for c in (1, 2):
        M[c, :, :3] = random_rotation(rng)
        M[c, :, 3] = rng.uniform(-5, 5, 3)
    M[1, 0, 3] = 0.0
    raw = rng.uniform(-30, 30, (n_raw, 3)).astype(F32)
    index = np.sort(rng.permutation(n_raw)[:n_rows]).astype(np.int64)
    cloud = np.sort(rng.randint(0, LOADER_CLOUDS, n_rows)).astype(np.int32)
    m0, m1, m2 = (Fraction(float(v)) for v in M[1, 0, :3])
    for i in np.nonzero(cloud == 1)[0][::3]:
        r = index[i]
        y = Fraction(float(raw[r, 1]))
        x = F32(float(-y * m1 / m0))
        z = F32(float(-(Fraction(float(x)) * m0 + y * m1) / m2))
        raw[r, 0], raw[r, 2] = x, z
    coords = np.concatenate([cloud[:, None], rng.randint(-100, 100, (n_rows, 3)).astype(np.int32)], axis=1).astype(np.int32)
    return raw, index, coords, M.reshape(LOADER_CLOUDS, 12)


def loader_points_reference(raw, index, coords, M):
    """(xyz_own, xyz_cf) float32: own = the raw point, cf = ((x m0 + y m1) + z m2) + t in fp64 -> float32."""
    own = raw[index]
    m = M.reshape(-1, 3, 4)[coords[:, 0]]
    x, y, z = (own[:, k].astype(F64) for k in range(3))
    cf = np.stack([((x * m[:, k, 0] + y * m[:, k, 1]) + z * m[:, k, 2]) + m[:, k, 3] for k in range(3)], axis=1)
    return own, cf.astype(F32)


def _rn(fr):
    return float(fr)          # int / int true division: correctly rounded to fp64


def loader_points_fused(raw, index, coords, M, first):
    """The same expression with every product contracted into the sum that follows it, evaluated exactly (Fractions) and rounded
    once per fused operation.  `first`: which product of x m0 + y m1 stays a rounded product (0: x m0, 1: y m1) -- a compiler
    may pick either."""
    own = raw[index]
    out = np.zeros((len(index), 3), F32)
    Fr = Fraction
    for i in range(len(index)):
        x, y, z = (Fr(float(v)) for v in own[i])
        m = M[coords[i, 0]].reshape(3, 4)
        for k in range(3):
            m0, m1, m2, t = (Fr(float(v)) for v in m[k])
            s = _rn(x * m0 + Fr(_rn(y * m1))) if first == 1 else _rn(y * m1 + Fr(_rn(x * m0)))
            s = _rn(z * m2 + Fr(s))
            out[i, k] = F32(_rn(Fr(s) + t))
    return out
