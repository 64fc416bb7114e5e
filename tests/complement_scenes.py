"""The raw samples the complement-loader tests share (tests/test_oracle_complement.py proves what they claim without a GPU,
tests/test_gpu_complement.py runs them): partial views of one synthetic surface from nearby poses, in sensor frames that lie
some kilometres from the origin, so that a float32 transform rounds at ~ 2.4e-4 m and points cross voxel faces and the crop
sphere when the arithmetic changes.  Everything is computed once per process."""
import functools

import numpy as np

VOXEL = 0.3
RADIUS = 0.45
SHIFT = np.array([3000.0, -2000.0, 10.0])
SIZES = (1, 255, 256, 257, 1025, 3000)          # either side of a block of 256 and of the scan's 2048 / 8192-entry chunks


def rigid(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    T[:3, 3] = t
    return T


def rotation(seed):
    from gcl_amd.lib import augment
    return augment.sample_rotation(np.random.RandomState(seed), 360)


@functools.lru_cache(maxsize=None)
def world(seed, n=60000):
    """A continuous surface with walls: fp64 [n, 3] about the origin, 45 m across."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(-45.0, 45.0, (n, 2))
    z = 0.8 * np.sin(0.21 * xy[:, 0]) + 0.5 * np.cos(0.17 * xy[:, 1])
    wall = rng.rand(n) < 0.25                       # a quarter of the points climb walls along a few lines x = const
    xy[wall, 0] = np.round(xy[wall, 0] / 15.0) * 15.0 + rng.normal(0, 0.02, wall.sum())
    z[wall] += rng.uniform(0.0, 4.0, wall.sum())
    return np.concatenate([xy, z[:, None]], axis=1)


def view(seed, pose, n, rng, reach, shift=SHIFT):
    """n points of the world within ``reach`` of the sensor, in the sensor's frame (pose: sensor -> world), moved by
    ``shift``, with 5 mm of noise: float32 [n, 3]."""
    W = world(seed)
    near = np.flatnonzero(np.linalg.norm(W - pose[:3, 3], axis=1) < reach)
    rows = np.sort(rng.choice(near, n, replace=False))
    Pi = np.linalg.inv(pose)
    local = W[rows] @ Pi[:3, :3].T + Pi[:3, 3] + rng.normal(0, 0.005, (n, 3))
    return (local + shift).astype(np.float32)


def framed(M, shift=SHIFT):
    """A transform between two sensor frames, between the same frames moved by ``shift``."""
    S = np.eye(4)
    S[:3, 3] = shift
    return S @ M @ np.linalg.inv(S)


def make_sample(seed, sizes0, sizes1, n_centre=3000, rotate=False, scale=None, shift=SHIFT):
    """One raw sample: two centre scans 2 m apart and, per side, complement scans of the given sizes from poses up to 3 m
    around it.  The centre scans reach 22 m, the complement scans 26 m: part of every complement scan lies outside the
    centre's range."""
    rng = np.random.RandomState(1000 + seed)
    P = [rigid(0.02, 0.01, (0.0, 0.0, 1.7)), rigid(-0.03, 0.0, (2.0, 0.4, 1.7))]
    s = {"radius": RADIUS, "trans": framed(np.linalg.inv(P[1]) @ P[0], shift)}
    for k, sizes in ((0, sizes0), (1, sizes1)):
        s[f"xyz{k}"] = view(seed, P[k], n_centre, rng, 22.0, shift)
        if sizes is None:
            continue
        s[f"cmpl{k}"], s[f"list_M{k}"] = [], []
        for j, n in enumerate(sizes):
            Pj = P[k] @ rigid(0.05 * (j - 2), 0.01 * j, ((j - 2.5) * 1.1, 0.3 * j, 0.02 * j))
            s[f"cmpl{k}"].append(view(seed, Pj, n, rng, 26.0, shift) if n else np.zeros((0, 3), dtype=np.float32))
            s[f"list_M{k}"].append(framed(np.linalg.inv(P[k]) @ Pj, shift))
    if rotate:
        s["rotation0"], s["rotation1"] = rotation(70 + seed), rotation(170 + seed)
    if scale is not None:
        s["scale"] = scale
    return s


def boundary_sample():
    """No rotation, frames about the origin: centre scan 0's farthest point is (0, 64, 0), so max_0 = 4096 exactly, and
    complement scan 0 (identity transform) opens with points AT the maximum, which must go, and one float32 ulp below it
    (4096 - 2^-12 = fl(fl((64 - 2^-18)^2) + 2^-12)), which must stay.  ``first`` names the opening rows."""
    rng = np.random.RandomState(31)
    s = make_sample(3, (400,), (300,), n_centre=800, scale=0.9, shift=np.zeros(3))
    x0 = s["xyz0"]
    x0 = x0[np.linalg.norm(x0.astype(np.float64), axis=1) < 60.0]
    s["xyz0"] = np.concatenate([x0[:300], np.array([[0.0, 64.0, 0.0]], dtype=np.float32), x0[300:]])
    below = np.float32(64.0) - np.float32(2.0 ** -18)
    first = np.array([[64.0, 0.0, 0.0], [0.0, 0.0, -64.0], [below, 2.0 ** -6, 0.0], [below, 0.0, 0.0],
                      [np.nextafter(np.float32(64.0), np.float32(100.0)), 0.0, 0.0]], dtype=np.float32)
    s["cmpl0"] = [np.concatenate([first, rng.uniform(-40, 40, (200, 3)).astype(np.float32)])]
    s["list_M0"] = [np.eye(4)]
    return s, first, [False, False, True, True, False]


def all_and_none_sample():
    """Side 0: every complement point is cropped (the scan is moved 400 m beyond the centre scan's range).  Side 1: none is
    (the complement scan is the centre scan without its farthest points, under the identity)."""
    s = make_sample(4, (500,), (1,), n_centre=1200)
    far = np.eye(4)
    far[:3, 3] = (400.0, -300.0, 0.0)
    s["list_M0"] = [far @ s["list_M0"][0]]
    x1 = s["xyz1"]
    r = (x1.astype(np.float64) ** 2).sum(1)
    s["cmpl1"] = [x1[r < np.sort(r)[-5]]]
    s["list_M1"] = [np.eye(4)]
    return s


def edge_sample():
    """Side 0: a complement scan, an EMPTY scan, another scan.  Side 1: an empty complement LIST."""
    s = make_sample(5, (300, 0, 257), (), n_centre=900, rotate=True)
    return s


def no_match_sample(n0=700):
    """A pair whose transform puts cloud 0 half a kilometre from cloud 1: no match."""
    s = make_sample(6, (256,), (255,), n_centre=700)
    s["trans"] = s["trans"].copy()
    s["trans"][:3, 3] += (500.0, 0.0, 0.0)
    s["xyz0"] = s["xyz0"][:n0]
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    """A tuple of raw samples."""
    rev = SIZES[::-1]
    if name.startswith("k3_"):
        what = name[3:]
        return (make_sample(1, SIZES, rev, rotate=what in ("rotation", "both"), scale=0.93 if what in ("scale", "both") else None),)
    if name == "k1":
        return (make_sample(2, (257, 1025), (1, 3000), n_centre=1500, rotate=True, scale=1.07),)
    if name == "boundary":
        return (boundary_sample()[0],)
    if name == "all_none":
        return (all_and_none_sample(),)
    if name == "edge":
        return (edge_sample(),)
    if name == "no_match":
        return (no_match_sample(),)
    if name == "batch3":          # B = 3: k = 1 with both draws, a pair without a match in the middle, the edge cases
        return scene("k1") + scene("no_match") + scene("edge")
    if name == "test_phase":      # no cmpl*: collate_debug_pair_fn
        return (make_sample(7, None, None, n_centre=1100, rotate=True, scale=0.95), make_sample(8, None, None, n_centre=600))
    raise KeyError(name)


K3 = ("k3_neither", "k3_rotation", "k3_scale", "k3_both")
NAMES = K3 + ("k1", "boundary", "all_none", "edge", "no_match", "batch3", "test_phase")


def host_centroids(s):
    """fp64 centroids of the two centre scans (the GPU tests take the device's, which have their own test)."""
    return np.stack([np.asarray(s[k], dtype=np.float32).astype(np.float64).sum(axis=0) / len(s[k]) for k in ("xyz0", "xyz1")])
