"""numpy restatement of the FPFH semantics of gcl_amd/lib/fpfh.py (csrc/fpfh.hip): neighbour lists, normals, SPFH, FPFH.
fp64 from the fp32 inputs, every product and sum rounded on its own (numpy has no fused multiply-add), brute force over the
N x N distance matrix of each cloud -- test sizes only.

Besides the four stages it returns, per point, what the tests use to set ill-conditioned points aside: the eigen gap of the
covariance, |cos| between the normal and the view ray, and the smallest distance of a pair feature to an interior bin edge.
"""
import numpy as np

BINS = 33


def _clouds(n, offsets):
    off = np.array([0, n], dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    return [(int(off[b]), int(off[b + 1])) for b in range(len(off) - 1)]


def dist2(P, Q):
    """d2 [len(P), len(Q)] = (dx dx + dy dy) + dz dz in fp64 from fp32 rows."""
    P, Q = np.asarray(P, dtype=np.float32).astype(np.float64), np.asarray(Q, dtype=np.float32).astype(np.float64)
    dx = P[:, None, 0] - Q[None, :, 0]
    dy = P[:, None, 1] - Q[None, :, 1]
    dz = P[:, None, 2] - Q[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbours(xyz, radius, max_nn, offsets=None):
    """(idx int32 [N, max_nn], cnt int32 [N], n_candidates [N]): the max_nn nearest rows of the own cloud with d2 <= r2, the
    point itself included, ascending (d2, row); -1 behind them."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = len(xyz)
    r = np.float64(np.float32(radius))
    r2 = r * r
    idx = np.full((n, max_nn), -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    ncand = np.zeros(n, dtype=np.int64)
    for lo, hi in _clouds(n, offsets):
        d2 = dist2(xyz[lo:hi], xyz[lo:hi])
        for i in range(hi - lo):
            cand = np.nonzero(d2[i] <= r2)[0]
            ncand[lo + i] = len(cand)
            keep = cand[np.lexsort((cand, d2[i, cand]))][:max_nn]        # by d2, then by row
            idx[lo + i, :len(keep)] = keep + lo
            cnt[lo + i] = len(keep)
    return idx, cnt, ncand


def normals(xyz, idx, cnt, viewpoint=None, offsets=None):
    """(normals float32 [N, 3], eigen gap (l1 - l0) / l2 [N], |cos(normal, viewpoint - p)| [N]); the last two are inf / 1
    where cnt < 3 (the normal is (0, 0, 1) by definition there)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    X = xyz.astype(np.float64)
    n = len(X)
    clouds = _clouds(n, offsets)
    vp = np.zeros((len(clouds), 3)) if viewpoint is None else np.broadcast_to(
        np.asarray(viewpoint, dtype=np.float32).astype(np.float64), (len(clouds), 3))
    out = np.zeros((n, 3), dtype=np.float32)
    gap, cosv = np.full(n, np.inf), np.ones(n)
    for b, (lo, hi) in enumerate(clouds):
        for i in range(lo, hi):
            k = int(cnt[i])
            if k < 3:
                out[i] = (0.0, 0.0, 1.0)
                continue
            Q = X[idx[i, :k]]
            D = Q - Q.mean(axis=0)
            C = D.T @ D / k
            w, V = np.linalg.eigh(C)                                     # ascending eigenvalues
            nv = V[:, 0] / np.linalg.norm(V[:, 0])
            ray = vp[b] - X[i]
            dot = float(nv @ ray)
            if dot < 0:
                nv = -nv
            out[i] = nv.astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                gap[i] = (w[1] - w[0]) / w[2]
                cosv[i] = abs(dot) / np.linalg.norm(ray)
    gap[np.isnan(gap)] = 0.0
    cosv[np.isnan(cosv)] = 0.0
    return out, gap, cosv


def pair_features(P1, N1, P2, N2):
    """open3d's ComputePairFeatures on rows: fp64 [M, 3] arrays in, (f1, f2, f3) [M] each out."""
    dp = P2 - P1
    d = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
    zero = d == 0.0
    ds = np.where(zero, 1.0, d)
    a1 = ((N1[:, 0] * dp[:, 0] + N1[:, 1] * dp[:, 1]) + N1[:, 2] * dp[:, 2]) / ds
    a2 = ((N2[:, 0] * dp[:, 0] + N2[:, 1] * dp[:, 1]) + N2[:, 2] * dp[:, 2]) / ds
    swap = np.abs(a1) < np.abs(a2)
    u = np.where(swap[:, None], N2, N1)
    o = np.where(swap[:, None], N1, N2)
    dp = np.where(swap[:, None], -dp, dp)
    f3 = np.where(swap, -a2, a1)
    v = np.stack([dp[:, 1] * u[:, 2] - dp[:, 2] * u[:, 1], dp[:, 2] * u[:, 0] - dp[:, 0] * u[:, 2],
                  dp[:, 0] * u[:, 1] - dp[:, 1] * u[:, 0]], axis=1)
    vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    zero |= vn == 0.0
    v = v / np.where(vn == 0.0, 1.0, vn)[:, None]
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                  u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    f2 = (v[:, 0] * o[:, 0] + v[:, 1] * o[:, 1]) + v[:, 2] * o[:, 2]
    f1 = np.arctan2((w[:, 0] * o[:, 0] + w[:, 1] * o[:, 1]) + w[:, 2] * o[:, 2],
                    (u[:, 0] * o[:, 0] + u[:, 1] * o[:, 1]) + u[:, 2] * o[:, 2])
    return np.where(zero, 0.0, f1), np.where(zero, 0.0, f2), np.where(zero, 0.0, f3)


def bin_coordinates(f1, f2, f3):
    """The three features in bin units [M, 3]; the bin is its floor clamped to 0 .. 10."""
    return np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], axis=1)


def spfh(xyz, nrm, idx, cnt):
    """(SPFH float32 [N, 33], edge distance [N]): integer counts over the list entries 1 .. cnt - 1 times 100 / (cnt - 1);
    the smallest distance (bin units) of any of the point's pair features to an interior bin edge 1 .. 10 (inf: no pair)."""
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    Nr = np.asarray(nrm, dtype=np.float32).astype(np.float64)
    n, K = idx.shape
    t = np.arange(K)[None, :]
    use = (t >= 1) & (t < np.asarray(cnt)[:, None])
    rows, cols = np.nonzero(use)
    nb = idx[rows, cols].astype(np.int64)
    f1, f2, f3 = pair_features(X[rows], Nr[rows], X[nb], Nr[nb])
    bc = bin_coordinates(f1, f2, f3)
    bins = np.clip(np.floor(bc), 0, 10).astype(np.int64) + np.array([0, 11, 22])[None, :]
    counts = np.zeros((n, BINS), dtype=np.int64)
    for c in range(3):
        np.add.at(counts, (rows, bins[:, c]), 1)
    k = np.asarray(cnt).astype(np.int64)
    inc = np.where(k > 1, 100.0 / np.maximum(k - 1, 1).astype(np.float64), 0.0)
    out = (counts.astype(np.float64) * inc[:, None]).astype(np.float32)
    edge = np.full(n, np.inf)
    dist = np.abs(bc - np.clip(np.rint(bc), 1, 10)).min(axis=1)
    np.minimum.at(edge, rows, dist)
    return out, edge


def fpfh(xyz, spfh_rows, idx, cnt, normalize=False):
    """FPFH float32 [N, 33]: per feature 100 / s times the sum over the entries 1 .. cnt - 1 with d2 != 0 of SPFH[entry] / d2
    (s: the same sum over the feature's 11 entries), plus the point's own SPFH row; list order, fp64."""
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    S = np.asarray(spfh_rows, dtype=np.float32).astype(np.float64)
    n, K = idx.shape
    cnt = np.asarray(cnt)
    F = np.zeros((n, BINS))
    s = np.zeros((n, 3))
    for t in range(1, K):
        rows = np.nonzero(cnt > t)[0]
        if len(rows) == 0:
            break
        nb = idx[rows, t].astype(np.int64)
        dx, dy, dz = (X[rows, c] - X[nb, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = d2 != 0.0
        rows, nb, d2 = rows[ok], nb[ok], d2[ok]
        val = S[nb] / d2[:, None]
        F[rows] += val
        s[rows] += val.reshape(-1, 3, 11).sum(axis=2)
    with np.errstate(divide="ignore"):
        scale = np.where(s != 0.0, 100.0 / s, 0.0)
    out = F * np.repeat(scale, 11, axis=1) + S
    out[cnt <= 1] = 0.0
    out = out.astype(np.float32)
    return normalized(out) if normalize else out


def normalized(f):
    """What the reference's loaders apply to FPFH (scripts/SC2_PCR/dataset.py:73-74): f / (|f|_2 + 1e-6)."""
    f = np.asarray(f, dtype=np.float32).astype(np.float64)
    return (f / (np.linalg.norm(f, axis=1, keepdims=True) + 1e-6)).astype(np.float32)


def fpfh_descriptors(xyz, voxel_size, viewpoint=None, offsets=None, normalize=True):
    """(normals, features): normals at (2 voxels, 30), FPFH at (5 voxels, 100)."""
    idx, cnt, _ = neighbours(xyz, 2.0 * voxel_size, 30, offsets)
    nrm, _, _ = normals(xyz, idx, cnt, viewpoint, offsets)
    idx, cnt, _ = neighbours(xyz, 5.0 * voxel_size, 100, offsets)
    sp, _ = spfh(xyz, nrm, idx, cnt)
    return nrm, fpfh(xyz, sp, idx, cnt, normalize)
