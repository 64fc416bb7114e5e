"""The seeded pose graphs of the multiway tests (tests/test_oracle_multiway.py proves their margins on the CPU,
tests/test_gpu_multiway.py runs them on the device) and the overlapping clouds of the chain tests.  numpy only.

A graph has every pair s < t as an edge, in the order of the reference's double loop (lib/complement_data_loader.py:429-451):
consecutive pairs are certain, the others uncertain.  Node i's ground truth P_i moves cloud i into cloud 0's frame (P_0 = I);
the exact edge is X = inv(P_t) P_s; an edge's information is sum G^T G over a few hundred seeded points of a 20 m scene.
"""
import functools

import numpy as np

from fpfh_scene import scene
from icp_scene import apply, first_per_voxel, rigid

SIZES = (2, 3, 4, 6, 8)          # 1, 3, 6, 15, 28 edges: one edge; one loop closure; the scripts' shape; the default; the cap
VARIANTS = ("consistent", "noisy", "outlier")
DISTANCE = 0.075


def names():
    """Every scene: the outlier variant needs a loop closure, so 2 nodes have none."""
    return [(n, v) for n in SIZES for v in VARIANTS if not (n == 2 and v == "outlier")]


def _small(rng, deg, metres):
    t = rng.normal(size=3)
    return rigid(rng.normal(size=3), np.deg2rad(deg) * rng.uniform(0.5, 1.0), t / np.linalg.norm(t) * metres * rng.uniform(0.5, 1.0))


def _info(rng):
    n = rng.randint(300, 1500)
    q = np.concatenate([rng.uniform(-10, 10, size=(n, 2)), rng.uniform(-1, 2, size=(n, 1))], axis=1)
    I = np.zeros((6, 6))
    for x, y, z in q:
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
        I += G.T @ G
    return I


@functools.lru_cache(maxsize=None)
def graph(n, variant):
    """dict: nodes [n, 4, 4], edges [(s, t)], T [m, 4, 4], info [m, 6, 6], uncertain [m], truth [n, 4, 4], outlier (edge or
    None)."""
    rng = np.random.RandomState(100 * n + VARIANTS.index(variant))
    truth = [np.eye(4)]
    for _ in range(1, n):                                           # a vehicle's track: about 2 m and 5 degrees a frame
        truth.append(truth[-1] @ rigid([0.1 * rng.normal(), 0.1 * rng.normal(), 1.0], np.deg2rad(rng.uniform(-5, 5)),
                                       [rng.uniform(1.5, 2.5), 0.2 * rng.normal(), 0.05 * rng.normal()]))
    edges = [(s, t) for s in range(n) for t in range(s + 1, n)]
    X = [np.linalg.inv(truth[t]) @ truth[s] for s, t in edges]
    info = [_info(rng) for _ in edges]
    outlier = None
    if variant == "consistent":
        nodes = [truth[0]] + [_small(rng, 1.0, 0.05) @ P for P in truth[1:]]
    else:
        X = [_small(rng, 0.05, 0.003) @ x for x in X]
        if variant == "outlier":
            loops = [k for k, (s, t) in enumerate(edges) if t != s + 1]
            outlier = loops[rng.randint(len(loops))]
            X[outlier] = rigid(rng.normal(size=3), np.deg2rad(30.0), [0.0, 0.0, 0.0]) @ X[outlier]
        odometry, nodes = np.eye(4), [np.eye(4)]
        for k in range(1, n):                                       # the reference's chain of the consecutive edges
            odometry = X[edges.index((k - 1, k))] @ odometry
            nodes.append(np.linalg.inv(odometry))
    g = {"nodes": np.stack(nodes), "edges": edges, "T": np.stack(X), "info": np.stack(info),
         "uncertain": np.array([t != s + 1 for s, t in edges]), "truth": np.stack(truth), "outlier": outlier}
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


# ---- overlapping clouds for the chain ---------------------------------------------------------------------------------------
def cloud_set(seed, n, points=700):
    """n samplings of one scene, each in its own frame: (clouds float32 [N_i, 3] downsampled to 0.05 voxels, truth [n, 4, 4]
    with P_0 = I, init float64 [n, n, 4, 4]: for s < t the true motion of cloud s into cloud t's frame off by 0.1 - 0.4
    degrees and at most 5 cm)."""
    rng = np.random.RandomState(4000 + seed)
    truth = [np.eye(4)]
    for _ in range(1, n):
        truth.append(truth[-1] @ rigid([0.0, 0.0, 1.0], np.deg2rad(rng.uniform(-4, 4)), [rng.uniform(0.1, 0.3), 0.05 * rng.normal(), 0.0]))
    clouds = []
    for i in range(n):
        w = scene(seed + 37 * i, points, stragglers=False)           # world = cloud 0's frame
        c = apply(np.linalg.inv(truth[i]), w)
        clouds.append(c[first_per_voxel(c)])
    init = np.tile(np.eye(4), (n, n, 1, 1))
    for s in range(n):
        for t in range(s + 1, n):
            init[s, t] = _small(rng, 0.4, 0.05) @ np.linalg.inv(truth[t]) @ truth[s]
    return clouds, np.stack(truth), init


def reference_init(velo2cam, pos_s, pos_t):
    """The reference's M of a pair (lib/complement_data_loader.py:410-411)."""
    return (velo2cam @ pos_s.T @ np.linalg.inv(pos_t.T) @ np.linalg.inv(velo2cam)).T


def raw_set(seed, n, copies=12):
    """Raw scans for multiway_registration: (raw float32 [P_i, 3]: every point of a cloud_set ``copies`` times with 8 mm of
    noise, shuffled; truth [n, 4, 4]; pos [n, 4, 4] and velo2cam [4, 4], such that reference_init(velo2cam, pos_s, pos_t) is
    the true motion of cloud s into cloud t's frame off by the odometry's error: up to 0.4 degrees and 5 cm a scan)."""
    rng = np.random.RandomState(6000 + seed)
    clouds, truth, _ = cloud_set(seed, n)
    raw = []
    for c in clouds:
        d = np.repeat(c.astype(np.float64), copies, axis=0) + 0.008 * rng.normal(size=(copies * len(c), 3))
        raw.append(d[rng.permutation(len(d))].astype(np.float32))
    V = rigid(rng.normal(size=3), 1.1, rng.normal(size=3))
    odo = [truth[0]] + [P @ _small(rng, 0.4, 0.05) for P in truth[1:]]
    pos = np.stack([V.T @ P @ np.linalg.inv(V.T) for P in odo])      # then M(s, t) = inv(odo_t) odo_s
    return raw, truth, pos, V


def dump(out):
    """Every graph as text for tools/micro/posegraph_host_check.cpp."""
    out.write(f"{len(names())}\n")
    for n, v in names():
        g = graph(n, v)
        out.write(f"{n} {len(g['edges'])}\n")
        for (s, t), u in zip(g["edges"], g["uncertain"]):
            out.write(f"{s} {t} {int(u)}\n")
        for a in (g["nodes"], g["T"], g["info"]):
            out.write(" ".join(repr(float(x)) for x in a.reshape(-1)) + "\n")


if __name__ == "__main__":
    import sys
    dump(sys.stdout)
