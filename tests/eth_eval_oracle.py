"""CPU restatement of the feature-match-recall pieces (generalization_ETH/evaluate.py), brute force in fp64 numpy, written
from their definitions:

    nn(q, p)[i]         = the LOWEST j that minimises sum_c (q[i, c] - p[j, c])^2           (any width: 3-D points, descriptors)
    mutual(nn01, nn10)  = [(i, nn01[i]) for ascending i if 0 <= nn01[i] < len(nn10) and nn10[nn01[i]] == i]
    inliers(pairs, T)   = #{(i, j): |kp0[i] - (R kp1[j] + t)| < tau}                        (the TARGET keypoints are moved)
    scene(table)        = recall = 100 * #(ratio > tau2) / #(gt_flag == 1), ave = sum(num_inliers of those) / #(ratio > tau2)

The reference file itself cannot be imported (open3d and pytorch3d at import), so nothing here is a recording of it.
"""
import numpy as np


def sqdist_rows(q, p, rows):
    """fp64 [len(rows), len(p)] squared distances of q[rows] to every p."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return ((q[rows, None, :] - p[None, :, :]) ** 2).sum(2)


def nn(q, p, block=None, with_gap=False):
    """(d2min fp64 [m], argmin int64 [m]) by brute force; ties -> lowest index (np.argmin returns the first minimum).
    ``with_gap``: also the difference between the second-smallest and the smallest distance of every row (inf for one point)."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    m, n = len(q), len(p)
    if block is None:
        block = max(1, (1 << 22) // max(1, n * q.shape[1]))
    d2 = np.empty(m, dtype=np.float64)
    arg = np.empty(m, dtype=np.int64)
    gap = np.full(m, np.inf)
    for i0 in range(0, m, block):
        rows = np.arange(i0, min(m, i0 + block))
        D = sqdist_rows(q, p, rows)
        a = D.argmin(1)
        arg[rows] = a
        d2[rows] = D[np.arange(len(rows)), a]
        if with_gap and n > 1:
            D[np.arange(len(rows)), a] = np.inf
            gap[rows] = D.min(1) - d2[rows]
    return (d2, arg, gap) if with_gap else (d2, arg)


def mutual(nn01, nn10):
    """int64 [K, 2]: the mutual pairs in ascending source index; out-of-range entries are not mutual."""
    nn01, nn10 = np.asarray(nn01, dtype=np.int64), np.asarray(nn10, dtype=np.int64)
    out = []
    for i in range(len(nn01)):
        j = int(nn01[i])
        if 0 <= j < len(nn10) and int(nn10[j]) == i:
            out.append((i, j))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def residuals(pairs, kp0, kp1, T):
    """fp64 |kp0[i] - (R kp1[j] + t)| of every pair; T is [3, 4] / [4, 4] / 12 numbers, row-major [R | t]."""
    T = np.asarray(T, dtype=np.float64).reshape(-1)[:12].reshape(3, 4)
    kp0, kp1 = np.asarray(kp0, dtype=np.float64), np.asarray(kp1, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    moved = kp1[pairs[:, 1]] @ T[:, :3].T + T[:, 3]
    return np.sqrt(((kp0[pairs[:, 0]] - moved) ** 2).sum(1))


def inliers(pairs, kp0, kp1, T, tau):
    return int((residuals(pairs, kp0, kp1, T) < tau).sum())


def scene(table, tau2=0.05):
    """Aggregation of per-pair rows (num_inliers, inlier_ratio, gt_flag); zero correct matches -> ave_num_inliers 0.0."""
    rows = [tuple(r) for r in np.asarray(table, dtype=np.float64).reshape(-1, 3)]
    gt_match = sum(1 for r in rows if r[2] == 1)
    good = [r for r in rows if r[1] > tau2]
    return dict(recall=(100.0 * len(good) / gt_match) if gt_match else float("nan"), correct_match=len(good),
                gt_match=gt_match, ave_num_inliers=(sum(r[0] for r in good) / len(good)) if good else 0.0)


def pair_row(n_mutual, n_inliers, in_log=True):
    """One row of the scene table from a pair's counts: zero mutual pairs -> ratio 0; the ratio in its 8-decimal text form."""
    if not in_log:
        return (0.0, 0.0, 0.0)
    ratio = (n_inliers / n_mutual) if n_mutual else 0.0
    return (float(n_inliers), float(f"{ratio:.8f}"), 1.0)


# ---------------------------------------------------------------------------------------------------------------
# test data shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------
def far_grid_case(seed=0, m=300, n=20000, centre=(800.0, -600.0, 50.0), pitch=0.05):
    """(q float32 [m, 3], p float32 [n, 3]): a jittered ``pitch`` grid around ``centre`` and queries inside it -- outdoor
    coordinates at voxel resolution, where |q|^2 + |p|^2 - 2 q.p in fp32 cannot tell neighbouring voxels apart."""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(n ** (1.0 / 3.0))) + 1
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    g = g[rng.permutation(len(g))[:n]]
    p = np.asarray(centre) + (g - side / 2.0) * pitch + rng.uniform(-0.4, 0.4, (n, 3)) * pitch
    q = np.asarray(centre) + rng.uniform(-0.45, 0.45, (m, 3)) * side * pitch
    return q.astype(np.float32), p.astype(np.float32)


def expansion_form_fp32(q, p):
    """argmin of |q|^2 + |p|^2 - 2 q.p evaluated in fp32: the form gcl_nn3_rowmin must NOT use."""
    q, p = np.asarray(q, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = (q * q).sum(1, dtype=np.float32)[:, None] + (p * p).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (q @ p.T)
    return d.argmin(1)


def rigid(rng, max_t=5.0):
    """A random rigid transformation as 4x4 fp64."""
    A = rng.normal(size=(3, 3))
    Q, R = np.linalg.qr(A)
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3] = Q
    T[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return T


def apply(T, x):
    return np.asarray(x, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def scene_case(world, seed=0, n_frag=4, n_keys=240, width=32, min_sep=0.3):
    """Four overlapping fragments of one world cloud [N, 3], each in a frame of its own, with PLANTED descriptors.

    Fragment i keeps the points whose x lies in a window that overlaps its neighbours' and is stored as
    inverse(pose_i) applied to them.  World keypoints are points at least ``min_sep`` apart; fragment i holds the ones inside
    its window, in an order of its own; a keypoint's planted descriptor is its world keypoint's row of a random table,
    so a shared keypoint matches itself exactly and two different keypoints are never within the inlier radius.
    gt_log['i_j'] = inverse(pose_i) @ pose_j moves fragment j's points into fragment i's frame; the windows are three
    steps wide and one step apart, so fragments up to two apart overlap and the pair (0, 3), which does not, is left out
    of the log, as a scene's gt.log lists overlapping pairs only.  ``shuffled`` is a copy of the descriptors with every
    fragment's rows rolled by i + 1 places in the (x, y, z) order of the keypoints' world positions: inside an overlap both fragments hold
    the same keypoints in the same order, so a keypoint's exact twin is now always a DIFFERENT world keypoint.
    Returns a dict; ``shared[(i, j)]`` = number of keypoints the two fragments share."""
    rng = np.random.RandomState(seed)
    world = np.asarray(world, dtype=np.float64)
    lo, hi = world[:, 0].min(), world[:, 0].max()
    span = (hi - lo) / (n_frag + 2)
    windows = [(lo + i * span - 1e-9, lo + (i + 3) * span + 1e-9) for i in range(n_frag)]
    keys = []
    for idx in rng.permutation(len(world)):
        if len(keys) == n_keys:
            break
        if all(np.linalg.norm(world[idx] - world[k]) >= min_sep for k in keys):
            keys.append(idx)
    keys = np.asarray(keys)
    table = rng.normal(size=(len(keys), width)).astype(np.float32)
    poses = [rigid(rng) for _ in range(n_frag)]
    frags, kps, descs, members, shuffled = [], [], [], [], []
    for i, (a, b) in enumerate(windows):
        inv = np.linalg.inv(poses[i])
        inside = (world[:, 0] >= a) & (world[:, 0] <= b)
        frags.append(apply(inv, world[inside]).astype(np.float32))
        mine = np.nonzero((world[keys, 0] >= a) & (world[keys, 0] <= b))[0]
        mine = mine[rng.permutation(len(mine))]
        members.append(mine)
        kps.append(apply(inv, world[keys[mine]]).astype(np.float32))
        descs.append(table[mine].copy())
        wk = world[keys[mine]]
        by_x = np.lexsort((wk[:, 2], wk[:, 1], wk[:, 0]))          # by x, then y, z: box faces hold many equal x
        rolled = np.empty_like(descs[-1])
        rolled[by_x] = descs[-1][np.roll(by_x, -(i + 1))]
        shuffled.append(rolled)
    gt_log, shared = {}, {}
    for i in range(n_frag):
        for j in range(i + 1, n_frag):
            shared[(i, j)] = len(np.intersect1d(members[i], members[j]))
            if j - i <= 2:
                gt_log[f"{i}_{j}"] = np.linalg.inv(poses[i]) @ poses[j]
    return dict(fragments=frags, keypoints=kps, descriptors=descs, gt_log=gt_log, shared=shared, poses=poses,
                shuffled=shuffled)


def scene_table(keypoints, descriptors, gt_log, tau1=0.1):
    """The per-pair table of a scene by brute force: fp64 nearest neighbours both ways, the mutual filter, the inlier count."""
    n = len(keypoints)
    rows = []
    for i in range(n):
        for j in range(i + 1, n):
            if f"{i}_{j}" not in gt_log:
                rows.append(pair_row(0, 0, in_log=False))
                continue
            nn01, nn10 = nn(descriptors[i], descriptors[j])[1], nn(descriptors[j], descriptors[i])[1]
            pairs = mutual(nn01, nn10)
            rows.append(pair_row(len(pairs), inliers(pairs, keypoints[i], keypoints[j], gt_log[f"{i}_{j}"], tau1)))
    return np.asarray(rows, dtype=np.float64)
