"""The seeded test scene of the FPFH tests (tests/test_oracle_fpfh.py, tests/test_gpu_fpfh.py) and the registration pair
made from it.  numpy only.

``scene(seed, n=1500)`` -> float32 [1636, 3]:
  three mutually perpendicular square patches (the planes z = 0, y = 0, x = 0 of a room corner) on an m x m jittered grid,
  m = floor(sqrt(n / 4)) = 19, spacing 0.05, in-plane jitter uniform within a cell, out-of-plane noise sigma 0.004;
  an upper half-sphere of m^2 points, radius 0.2 with 0.4 % radial noise, standing on the z = 0 patch;
  a clump of n / 8 uniform points in a 0.12 cube (so that max_nn binds);
  five stragglers (the LAST five rows): one isolated point, two points 0.01 apart, one exact duplicate pair;
  everything shifted by (1.0, 1.5, 0.7); the viewpoint is the origin.
"""
import numpy as np

SHIFT = np.array([1.0, 1.5, 0.7])
N_STRAGGLERS = 5


def scene(seed, n=1500, stragglers=True):
    rng = np.random.RandomState(1000 + seed)
    m = int(np.floor(np.sqrt(n / 4)))
    parts = []
    for axis in range(3):                                    # the patch with normal `axis`
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 2)
        uv = (g + rng.uniform(0.0, 1.0, size=g.shape)) * 0.05
        p = np.zeros((m * m, 3))
        p[:, [c for c in range(3) if c != axis]] = uv
        p[:, axis] = rng.normal(0.0, 0.004, size=m * m)
        parts.append(p)
    d = rng.normal(size=(m * m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = np.abs(d[:, 2])
    parts.append(np.array([0.55, 0.45, 0.0]) + d * (0.2 * (1.0 + 0.004 * rng.normal(size=(m * m, 1)))))
    parts.append(np.array([0.6, 0.6, 0.6]) + rng.uniform(-0.06, 0.06, size=(n // 8, 3)))
    if stragglers:
        parts.append(np.array([[2.0, 2.0, 2.0],                                     # isolated
                               [-1.0, 2.0, 0.5], [-1.0, 2.01, 0.5],                 # 0.01 apart
                               [2.0, -1.0, 0.5], [2.0, -1.0, 0.5]]) - 0.0)          # exact duplicates
    return (np.concatenate(parts) + SHIFT).astype(np.float32)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pair(seed, noise=0.002):
    """(A float32 [NA, 3], B float32 [NB, 3], rows of A behind B's points [NB], T float64 [4, 4] with B ~ T A, viewpoint of
    B [3]): A is the scene without its stragglers, B the 75 % of A with the largest x plus noise, moved by a rotation of
    0.9 rad about a random axis and t = (0.4, -0.3, 0.2).  A's viewpoint is the origin, B's moves with it."""
    A = scene(seed, stragglers=False)
    rng = np.random.RandomState(2000 + seed)
    keep = np.sort(np.argsort(A[:, 0], kind="stable")[len(A) // 4:])
    R = rotation(rng.normal(size=3), 0.9)
    t = np.array([0.4, -0.3, 0.2])
    Bp = A[keep].astype(np.float64) + noise * rng.normal(size=(len(keep), 3))
    B = (Bp @ R.T + t).astype(np.float32)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return A, B, keep, T, t.astype(np.float32)
