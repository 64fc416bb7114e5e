"""numpy fp64 restatement of the feature-matching RANSAC of csrc/ransac.hip (include/gcl_amd.h, gcl_ransac_register).

open3d is not available where the tests run and its RANSAC draws from std::mt19937, so the algorithm is the one the header
states: hypothesis h is a function of (seed, h); this module enumerates exactly the hypotheses the kernels draw and repeats
the five steps, the winner rule and the chunk / limit rule in fp64.  The pose of step 3 is rounded to fp32, as the header
defines it; everything measured with it is fp64.

A hypothesis is BORDERLINE when an fp32 evaluation may legitimately decide it differently: a compared quantity within
relative 1e-4 of its threshold (an edge-length comparison, a sample's checker distance, any correspondence's inlier
distance -- about 100 fp32 roundings at coordinates of tens of metres), or a sample whose H has a second singular value
below 1e-6 of the first (collinear sample: the pose is not unique).
"""
import math

import numpy as np

MASK = (1 << 64) - 1
REL = 1e-4


def draw(seed, h, j, n):
    """Sample index j of hypothesis h, in Python integers."""
    z = (seed + (4 * h + j + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def draw_all(seed, hs, ransac_n, n):
    """int64 [len(hs), ransac_n]: ``draw`` for every hypothesis id of ``hs``, vectorised in wrapping uint64."""
    hs = np.asarray(hs, dtype=np.uint64)[:, None]
    j = np.arange(ransac_n, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + (np.uint64(4) * hs + j + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def kabsch(S, T):
    """TransformationEstimationPointToPoint(False) for a batch of samples S, T [B, k, 3] (fp64): R [B, 3, 3], t [B, 3] with
    R S + t ~ T, and the singular values of H [B, 3] (descending)."""
    S, T = np.asarray(S, dtype=np.float64), np.asarray(T, dtype=np.float64)
    cs, ct = S.mean(1), T.mean(1)
    A, B = S - cs[:, None], T - ct[:, None]
    H = np.einsum("bki,bkj->bij", A, B)
    U, sv, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))
    d[d == 0] = 1.0
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ np.swapaxes(U, 1, 2)
    t = ct - np.einsum("bij,bj->bi", R, cs)
    return R, t, sv


def planted_case(seed, n, share, noise=0.05, half=10.0):
    """Synthetic correspondences: ``src`` uniform in a cube of side 2 ``half``, a rotation of 0.7 rad about a random axis plus
    the translation (3, -2, 1), uniform noise of +-``noise`` on the first round(share n) of a random order, every other
    target redrawn uniformly in the cube.  Returns (src fp32, tgt fp32, R, t, inlier rows)."""
    rng = np.random.RandomState(seed)
    src = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    t = np.array([3.0, -2.0, 1.0])
    tgt = src.astype(np.float64) @ R.T + t + rng.uniform(-noise, noise, (n, 3))
    order = rng.permutation(n)
    out = order[int(round(share * n)):]
    tgt[out] = rng.uniform(-half, half, (len(out), 3))
    return src, tgt.astype(np.float32), R, t, np.sort(order[:int(round(share * n))])


def _near(q, thr):
    return np.abs(q - thr) <= REL * np.abs(thr)


def limit_of(best_count, n, ransac_n, confidence):
    """The id limit after a chunk (None: no limit)."""
    if not (0.0 < confidence < 1.0) or best_count <= 0:
        return None
    f = best_count / n
    if f >= 1.0:
        return 0
    pw = f
    for _ in range(1, ransac_n):          # f * f * f (* f), the kernel's order
        pw *= f
    den = math.log(1.0 - pw)
    if den == 0.0:
        return None
    v = math.ceil(math.log(1.0 - confidence) / den)
    return v if v < 9.0e18 else None


def ransac(src, tgt, ransac_n, edge_similarity, check_distance, max_corr_distance, max_iteration, confidence, seed, chunk):
    """Every hypothesis of a run.  Returns a dict:
    status int64 [max_iteration] (count, or -1 edge / -2 distance / -3 repeated index / -4 skipped), borderline bool
    [max_iteration], count / sse (fp64; sse NaN where not scored), samples int64 [max_iteration, ransac_n], R / t (fp32-rounded
    pose as fp64, NaN where none), inl_border bool [max_iteration, n] (correspondence within the margin of the inlier
    distance), winner (h or -1), covered, scored, limit (the last limit in force, None if none), limits (per executed chunk)."""
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    n, M = len(src), int(max_iteration)
    hs = np.arange(M)
    idx = draw_all(seed, hs, ransac_n, n)
    status = np.zeros(M, dtype=np.int64)
    border = np.zeros(M, dtype=bool)
    srt = np.sort(idx, axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]).any(1)
    status[dup] = -3
    S, T = src[idx], tgt[idx]
    if edge_similarity > 0:
        bad = np.zeros(M, dtype=bool)
        for a in range(ransac_n):
            for b in range(a + 1, ransac_n):
                ds = np.linalg.norm(S[:, a] - S[:, b], axis=1)
                dt = np.linalg.norm(T[:, a] - T[:, b], axis=1)
                bad |= ~((ds >= dt * edge_similarity) & (dt >= ds * edge_similarity))
                border |= ~dup & (_near(ds, dt * edge_similarity) | _near(dt, ds * edge_similarity))
        status[~dup & bad] = -1
    alive = np.nonzero(status == 0)[0]
    R = np.full((M, 3, 3), np.nan)
    t = np.full((M, 3), np.nan)
    count = np.zeros(M, dtype=np.int64)
    sse = np.full(M, np.nan)
    inl_border = np.zeros((M, n), dtype=bool)
    if len(alive):
        Ra, ta, sv = kabsch(S[alive], T[alive])
        Ra, ta = Ra.astype(np.float32).astype(np.float64), ta.astype(np.float32).astype(np.float64)
        R[alive], t[alive] = Ra, ta
        border[alive] |= sv[:, 1] < 1e-6 * sv[:, 0]
        ok = np.ones(len(alive), dtype=bool)
        if check_distance > 0:
            d = np.linalg.norm(np.einsum("bij,bkj->bki", Ra, S[alive]) + ta[:, None] - T[alive], axis=2)
            ok = (d <= check_distance).all(1)
            border[alive] |= _near(d, check_distance).any(1)
        status[alive[~ok]] = -2
        sc = alive[ok]
        for b0 in range(0, len(sc), 32):                    # blocks of hypotheses: [32, n, 3] temporaries at large n
            blk = sc[b0:b0 + 32]
            d = np.linalg.norm(np.einsum("bij,nj->bni", R[blk], src) + t[blk][:, None] - tgt[None], axis=2)
            inl = d < max_corr_distance
            count[blk] = inl.sum(1)
            sse[blk] = np.where(inl, d * d, 0.0).sum(1)
            status[blk] = count[blk]
            inl_border[blk] = _near(d, max_corr_distance)
            border[blk] |= inl_border[blk].any(1)
    # chunks, winner, early stop
    chunk = int(chunk)
    best = (-1, 0, 0.0)                                     # h, count, sse
    limit, limits, covered, scored = None, [], 0, 0
    for h0 in range(0, M, chunk):
        h1 = min(M, h0 + chunk)
        if limit is not None and h0 >= limit:
            status[h0:h1] = -4
            continue
        for h in np.nonzero(status[h0:h1] > 0)[0] + h0:
            c, s = int(count[h]), float(sse[h])
            if best[0] < 0 or c > best[1] or (c == best[1] and s < best[2]):
                best = (int(h), c, s)
        covered += h1 - h0
        scored += int((status[h0:h1] >= 0).sum())
        new = limit_of(best[1], n, ransac_n, confidence)
        limit = new if new is not None else limit
        limits.append(limit)
    return dict(status=status, borderline=border, count=count, sse=sse, samples=idx, R=R, t=t, inl_border=inl_border,
                winner=best[0], covered=covered, scored=scored, limit=limit, limits=limits)
