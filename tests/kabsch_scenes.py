"""Seeded correspondence sets for the rigid-fit solver (csrc/kabsch.h) and its four callers: tests/test_oracle_kabsch.py
proves on the CPU that every set is what it claims to be, tests/test_gpu_kabsch_callers.py feeds them to the kernels.
numpy only; generators and their constants, nothing else.

``corr_set(name, n, shifted)`` -> (src float32 [n, 3], tgt float32 [n, 3], R, t): tgt is the float32 rounding of R src + t
(for ``mirrored``: of R M src + t, M the mirror of the thin axis, so that NO rotation fits).  The motion is 0.7 rad about a
seeded random axis and t = (3, -2, 1) unless the set says otherwise.  ``shifted`` moves the whole set by SHIFT (the shift of
icp_scene.FULL["far"]) and turns about the shifted origin, so both clouds stay near SHIFT.

  generic          uniform in the box of half extents (4, 2, 1)
  planar           a plane of half extents (4, 2), tilted by a random rotation: planar to float32 rounding
  planar_exact     z = 0 on multiples of 1/8, rotation about z: H has an exact zero row and column
  slab_1e-2 ..     the generic box with the half extent 1 replaced by 1e-2, 1e-4, 1e-6
  mirrored         half extents (4, 2, 0.5), tgt = R M src + t
  collinear        a line of half length 4 in a random direction, collinear to float32 rounding
  collinear_exact  y = z = 0, x on multiples of 1/8, rotation about x: H has ONE non-zero entry
  coincident       every source row is one point, every target row its image
  isotropic        cube vertices and face centres: rows come in shells (8 vertices, then 4 x 6 face centres, each shell at
                   its own dyadic scale; period 32), so that rows 0 .. 19, 0 .. 31, 0 .. 63, ... have covariance c I and H = c R
  half_turn        the generic box turned by pi about a random axis

``icp_pair(name, shifted)`` -> (source, target, G, init): the target is a grid at spacing 0.05 on the set's support (box,
plane, rough sheet, line, cube; for ``coincident`` a line grid that ONE repeated source point matches in one row), the source
is the target moved by inv(G), G = 0.01 rad about the grid's centre and 5 mm, and init is the identity.
"""
import numpy as np

SHIFT = (500.0, -120.0, 30.0)
ANGLE, TRANSLATION = 0.7, (3.0, -2.0, 1.0)
SLABS = {"slab_1e-2": 1e-2, "slab_1e-4": 1e-4, "slab_1e-6": 1e-6}
NAMES = ("generic", "planar", "planar_exact", "slab_1e-2", "slab_1e-4", "slab_1e-6", "mirrored", "collinear",
         "collinear_exact", "coincident", "isotropic", "half_turn")
# what a set claims: the rank of its H, and whether one rotation fits best (rank >= 2 and, mirrored, s2 > s3)
RANK = {"generic": 3, "planar": 2, "planar_exact": 2, "slab_1e-2": 3, "slab_1e-4": 3, "slab_1e-6": 3, "mirrored": 3,
        "collinear": 1, "collinear_exact": 1, "coincident": 0, "isotropic": 3, "half_turn": 3}
UNIQUE = tuple(k for k in NAMES if RANK[k] >= 2)
RIGID = tuple(k for k in NAMES if k != "mirrored")            # some rotation maps every source row onto its target row
MIRROR = np.diag([1.0, 1.0, -1.0])

ICP_SPACING, ICP_RADIUS, ICP_ANGLE, ICP_STEP = 0.05, 0.02, 0.01, 0.005


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _rng(name, salt=0):
    return np.random.RandomState(4105 + 17 * NAMES.index(name) + salt)


def _dyadic(rng, n, half):
    return rng.randint(-8 * half, 8 * half + 1, size=n) / 8.0


def _isotropic_rows(n):
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    f = np.concatenate([np.eye(3), -np.eye(3)])
    rows, k = [], 0
    while sum(len(r) for r in rows) < n:
        rows.append((v if k % 5 == 0 else f) * (1.0 + 0.25 * (k % 7)))
        k += 1
    return np.concatenate(rows)[:n]


def _local(name, n):
    """(points float64 [n, 3] in the set's own frame, R): before the shift and the float32 rounding."""
    rng = _rng(name)
    axis = rng.normal(size=3)
    R = rotation(axis, ANGLE)
    if name == "generic" or name == "half_turn":
        x = rng.uniform(-1, 1, (n, 3)) * [4.0, 2.0, 1.0]
        if name == "half_turn":
            R = rotation(axis, np.pi)
    elif name in SLABS:
        x = rng.uniform(-1, 1, (n, 3)) * [4.0, 2.0, SLABS[name]]
    elif name == "mirrored":
        x = rng.uniform(-1, 1, (n, 3)) * [4.0, 2.0, 0.5]
    elif name == "planar":
        x = (rng.uniform(-1, 1, (n, 3)) * [4.0, 2.0, 0.0]) @ rotation(rng.normal(size=3), 1.1).T
    elif name == "planar_exact":
        x = np.stack([_dyadic(rng, n, 4), _dyadic(rng, n, 2), np.zeros(n)], axis=1)
        R = rotation([0, 0, 1], ANGLE)
    elif name == "collinear":
        d = rng.normal(size=3)
        x = rng.uniform(-4, 4, (n, 1)) * (d / np.linalg.norm(d))[None]
    elif name == "collinear_exact":
        x = np.stack([_dyadic(rng, n, 4), np.zeros(n), np.zeros(n)], axis=1)
        R = rotation([1, 0, 0], ANGLE)
    elif name == "coincident":
        x = np.tile(rng.uniform(-1, 1, (1, 3)) * [4.0, 2.0, 1.0], (n, 1))
    elif name == "isotropic":
        x = _isotropic_rows(n)
    else:
        raise KeyError(name)
    return x, R


def corr_set(name, n, shifted=False):
    x, R = _local(name, n)
    shift = np.asarray(SHIFT if shifted else (0.0, 0.0, 0.0))
    src = (x + shift).astype(np.float32)
    t = np.asarray(TRANSLATION) + shift - R @ shift                       # turn about the set, not about the far origin
    s = src.astype(np.float64)
    if name == "mirrored":
        s = (s - shift) @ MIRROR + shift
    tgt = (s @ R.T + t).astype(np.float32)
    return src, tgt, R, t


def cases():
    """Every (name, shifted) in a fixed order."""
    return [(name, shifted) for shifted in (False, True) for name in NAMES]


def label(name, shifted):
    return name + ("+far" if shifted else "")


# ---- ICP pairs -------------------------------------------------------------------------------------------------------
def _grid(name):
    """The target grid in the set's own frame, float64 [m, 3], about its own centre."""
    rng = _rng(name, salt=5)
    ax = lambda k: (np.arange(k) - (k - 1) / 2.0) * ICP_SPACING
    mesh = lambda *a: np.stack(np.meshgrid(*a, indexing="ij"), axis=-1).reshape(-1, 3)
    if name in ("generic", "half_turn"):
        return mesh(ax(9), ax(5), ax(3))
    if name == "mirrored":
        return mesh(ax(9), ax(5), ax(2))
    if name == "isotropic":
        return mesh(ax(5), ax(5), ax(5))
    if name == "planar":
        return mesh(ax(16), ax(8), ax(1)) @ rotation(rng.normal(size=3), 1.1).T
    if name == "planar_exact":
        return mesh(ax(16) + ICP_SPACING / 2, ax(8) + ICP_SPACING / 2, ax(1))
    if name in SLABS:                                         # a rough sheet: every node off the plane by up to +- the thickness
        g = mesh(ax(16), ax(8), ax(1))
        g[:, 2] = rng.uniform(-1, 1, len(g)) * SLABS[name]
        return g
    if name == "collinear":
        d = rng.normal(size=3)
        return ax(24)[:, None] * (d / np.linalg.norm(d))[None]
    if name in ("collinear_exact", "coincident"):
        return mesh(ax(24) + ICP_SPACING / 2, ax(1), ax(1))
    raise KeyError(name)


def icp_pair(name, shifted=False):
    shift = np.asarray(SHIFT if shifted else (0.0, 0.0, 0.0))
    rng = _rng(name, salt=9)
    tgt = (_grid(name) + shift).astype(np.float32)
    G = np.eye(4)
    G[:3, :3] = rotation(rng.normal(size=3), ICP_ANGLE)
    step = rng.normal(size=3)
    G[:3, 3] = step / np.linalg.norm(step) * ICP_STEP + shift - G[:3, :3] @ shift
    rows = tgt[[7] * 5] if name == "coincident" else tgt
    Gi = np.linalg.inv(G)
    src = (rows.astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32)
    return src, tgt, G, np.eye(4)
