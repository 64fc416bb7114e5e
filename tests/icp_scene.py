"""The seeded scenes of the ICP tests (tests/test_oracle_icp.py proves their margins on the CPU, tests/test_gpu_icp.py runs
them on the device).  numpy only.

A pair is two independent samplings of the surfaces of tests/fpfh_scene.py (same geometry, different jitter: two scans of
one room corner), each downsampled to the first point of every 0.05 voxel; the source is then moved by inv(G), so that G is
the motion that registers it, and ``init`` is G times a perturbation of 0.1 - 0.5 degrees and at most 0.1 m.
"""
import functools

import numpy as np

from fpfh_scene import rotation, scene

VOXEL, RADIUS = 0.05, 0.2


def first_per_voxel(xyz, voxel=VOXEL):
    """Rows of the first point of every voxel, ascending: sparse_quantize(xyz / voxel, return_index=True)."""
    c = np.floor(np.asarray(xyz, dtype=np.float32) / np.float32(voxel)).astype(np.int64)
    _, first = np.unique(c, axis=0, return_index=True)
    return np.sort(first)


def rigid(axis, angle, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(axis, angle), t
    return T


def apply(T, xyz):
    return (np.asarray(xyz, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def nearest_rows(xyz, anchor, k):
    """The k rows nearest to ``anchor``, ascending: a dense local crop."""
    d = ((xyz.astype(np.float64) - anchor) ** 2).sum(axis=1)
    return np.sort(np.argsort(d, kind="stable")[:k])


def make_pair(seed, n, shift=(0.0, 0.0, 0.0)):
    """(source float32 [N0, 3], target float32 [N1, 3], G, init): about ``n`` points a side."""
    rng = np.random.RandomState(7000 + seed)
    shift = np.asarray(shift, dtype=np.float64)
    tgt = (scene(seed, n, stragglers=False).astype(np.float64) + shift).astype(np.float32)
    tgt = tgt[first_per_voxel(tgt)]
    src_w = (scene(seed + 500, n, stragglers=False).astype(np.float64) + shift).astype(np.float32)
    G = rigid(rng.normal(size=3), rng.uniform(0.2, 0.8), rng.uniform(-1.0, 1.0, size=3))
    G[:3, 3] += shift - G[:3, :3] @ shift                      # turn about the scene, not about the far origin
    src = apply(np.linalg.inv(G), src_w)
    src = src[first_per_voxel(src)]
    t = rng.normal(size=3)
    delta = rigid(rng.normal(size=3), np.deg2rad(rng.uniform(0.1, 0.5)), t / np.linalg.norm(t) * rng.uniform(0.02, 0.1))
    delta[:3, 3] += shift - delta[:3, :3] @ shift
    return src, tgt, G, delta @ G


# name -> (seed, points a side, shift): the full runs (<= 2000 points a side after the voxels)
FULL = {"corner": (3, 1500, (0.0, 0.0, 0.0)), "corner_b": (5, 1100, (0.0, 0.0, 0.0)), "far": (4, 1300, (500.0, -120.0, 30.0))}
FULL_ITERATIONS = (30, 200, 5)       # 5: the iteration limit binds
RAW_SEEDS = (1, 2)

# (source rows, target rows) of the one-step cases: the minimum, the wave border, the block border, several blocks, the
# workload's order
STEP_SIZES = [(1, 1), (3, 65), (63, 257), (64, 64), (65, 3), (255, 1025), (256, 256), (257, 63), (1025, 255), (1, 5000),
              (5000, 1), (5000, 5000)]
STEP_SEED, STEP_N = 11, 10000


@functools.lru_cache(maxsize=None)
def _step_scene():
    src, tgt, G, init = make_pair(STEP_SEED, STEP_N)
    for a in (src, tgt, G, init):
        a.setflags(write=False)
    return src, tgt, G, init


def step_pair(n0, n1):
    """The one-step case: dense local crops of n0 source and n1 target rows around one point of a pair of more than 5000
    points a side."""
    src, tgt, G, init = _step_scene()
    anchor = tgt[len(tgt) // 3].astype(np.float64)
    s = nearest_rows(apply(G, src), anchor, n0)
    t = nearest_rows(tgt, anchor, n1)
    return src[s], tgt[t], G, init


def raw_pair(seed, copies=30):
    """A raw scan pair of about 20 k points a side for refine_pair_poses: every point of a ~1000-point pair ``copies``
    times with 8 mm of noise, so that the 0.05 voxels keep <= 2000 points a side.  Returns (xyz0, xyz1, M): M is the
    odometry pose (the true motion off by 0.1 - 0.5 degrees and <= 0.1 m)."""
    rng = np.random.RandomState(9000 + seed)
    src, tgt, G, init = make_pair(seed, 1000)
    dense = lambda x: (np.repeat(x.astype(np.float64), copies, axis=0) + 0.008 * rng.normal(size=(copies * len(x), 3)))
    xyz0 = dense(src)[rng.permutation(copies * len(src))].astype(np.float32)
    xyz1 = dense(tgt)[rng.permutation(copies * len(tgt))].astype(np.float32)
    return xyz0, xyz1, init
