"""The rigid-fit solver (gcl_amd/csrc/kabsch.h) on the CPU against numpy.linalg.svd in fp64, and the proof that every scene
of tests/kabsch_scenes.py is what it claims to be.  No GPU: oracle/libkabsch_host.so is the kernels' own header compiled for
the host (oracle/kabsch_host.cpp, oracle/Makefile; built by build()).  KABSCH_HOST_LIB names another build of the same
wrapper (how the mutations of the header listed in DESIGN.md "Rigid fit on degenerate sets" were shown to fail here).

Convention (kabsch.h): H = A^T B = U S V^T, R = V diag(1, 1, d) U^T with d = det(V U^T), so R moves A onto B.

Every H is made from a POINT SET (8 rows: A = Q diag(s) U^T, B = Q V^T with Q^T Q = I), so that the reference's own
stability can be measured: the spread of numpy's R under row permutations of that set (another order of the sums that make
H).  Where the rotation is unique -- rank >= 2 and, for d = -1, s2 > s3 -- the solver must give numpy's R within
C 2^-52 s1 / (s2 + d s3); C_BOUND is four times the largest spread measured, in those units (printed under -s and recorded in
DESIGN.md).  Every case: R R^T = I within 1e-13, det R = +1, finite, and R u1 = v1 where s1 is simple.

Out of scope: scales no fp32 coordinates can produce.  The solver's guards are absolute (1e-300), so H below ~1e-300 (and
sums of squares that overflow, H above ~1e150) are not tested; the sweep stops at H = 1e-12 .. 1e+12, coordinates from a
micrometre to 1000 km.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle as IO                                                # noqa: E402
import kabsch_scenes as KS                                             # noqa: E402
import ransac_oracle as RO                                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("KABSCH_HOST_LIB", os.path.join(ROOT, "oracle", "libkabsch_host.so"))
EPS = 2.0 ** -52
C_BOUND = 201.0              # 4 x 50.2, numpy's largest own spread (family two_equal), in units of 2^-52 s1 / (s2 + d s3)
ORTHO_TOL = 1e-13
PERMS = 8
ROWS = 8


@functools.lru_cache(maxsize=None)
def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is missing: build() makes it (oracle/Makefile)")
    lib = ctypes.CDLL(LIB)
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    lib.kabsch_host_pack.argtypes, lib.kabsch_host_pack.restype = [vp, vp, vp, ll, vp], None
    lib.kabsch_host_rotation.argtypes, lib.kabsch_host_rotation.restype = [vp, ll, vp], None
    return lib


def solver_rotation(H):
    H = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(-1, 9))
    R = np.full((len(H), 9), np.nan)
    _lib().kabsch_host_rotation(H.ctypes.data, len(H), R.ctypes.data)
    return R.reshape(-1, 3, 3)


def solver_pack(H, ca, cb):
    H = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(-1, 9))
    ca, cb = (np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1, 3)) for c in (ca, cb))
    T = np.full((len(H), 12), np.nan, dtype=np.float32)
    _lib().kabsch_host_pack(H.ctypes.data, ca.ctypes.data, cb.ctypes.data, len(H), T.ctypes.data)
    return T.reshape(-1, 3, 4)


def numpy_fit(H):
    """(R, s, d, U, V) of a batch of H by numpy.linalg.svd."""
    U, s, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, -1, -2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, -1, -2)))
    d[d == 0] = 1.0
    D = np.zeros_like(H)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    return V @ D @ np.swapaxes(U, -1, -2), s, d, U, V


# ---- the problems: point sets with chosen singular values --------------------------------------------------------------
def _orth(rng, m, rows=3):
    q, r = np.linalg.qr(rng.normal(size=(m, rows, 3)))
    return q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]


def _proper(M):
    M = M.copy()
    M[:, :, 2] *= np.sign(np.linalg.det(M))[:, None]
    return M


def point_sets(rng, s, mirrored):
    """A, B [m, ROWS, 3] with A^T B = U diag(s) V^T; det(V U^T) = -1 where ``mirrored``."""
    m = len(s)
    U, V, Q = _proper(_orth(rng, m)), _proper(_orth(rng, m)), _orth(rng, m, ROWS)
    V[:, :, 2] *= np.where(mirrored, -1.0, 1.0)[:, None]
    A = Q @ (s[:, :, None] * np.swapaxes(U, 1, 2))
    B = Q @ np.swapaxes(V, 1, 2)
    return A, B


def _sv(m, s1, s2, s3):
    return np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), (m,)) for x in (s1, s2, s3)], axis=1)


def families():
    """name -> (A, B, unique).  About 4000 problems."""
    rng = np.random.RandomState(20240)
    out = {}
    m = 512
    s = np.sort(rng.uniform(0.05, 1.0, (m, 3)), axis=1)[:, ::-1] * 10.0 ** rng.uniform(-2, 2, (m, 1))
    out["full_rank"] = point_sets(rng, s, np.zeros(m, bool)) + (True,)
    m = 256
    out["rank2"] = point_sets(rng, _sv(m, 1.0, rng.uniform(0.05, 1.0, m), 0.0), np.zeros(m, bool)) + (True,)
    A, B, _ = out["rank2"]
    A, B = A.copy(), B.copy()
    A[:128, :, rng.randint(0, 3)] = 0.0                          # an exact zero ROW of H ...
    B[128:, :, rng.randint(0, 3)] = 0.0                          # ... and an exact zero COLUMN
    out["rank2_exact_zeros"] = (A, B, True)
    out["rank1"] = point_sets(rng, _sv(m, 1.0, 0.0, 0.0), np.zeros(m, bool)) + (False,)
    A = np.zeros((m, ROWS, 3))
    A[:, :, 0] = rng.normal(size=(m, ROWS))                      # axis-aligned lines: H has ONE non-zero entry
    B = np.zeros((m, ROWS, 3))
    B[:, :, 0] = A[:, :, 0]
    B[m // 2:] = np.roll(B[m // 2:], 1, axis=2)
    out["rank1_axis"] = (A, B, False)
    out["rank0"] = (np.zeros((16, ROWS, 3)), rng.normal(size=(16, ROWS, 3)), False)
    sc = 10.0 ** rng.uniform(-2, 2, m)
    out["two_equal"] = point_sets(rng, _sv(m, sc, sc, sc * rng.uniform(0.05, 0.9, m)), np.zeros(m, bool)) + (True,)
    out["two_equal_low"] = point_sets(rng, _sv(m, sc, sc * 0.3, sc * 0.3), np.zeros(m, bool)) + (True,)
    out["three_equal"] = point_sets(rng, _sv(m, sc, sc, sc), np.zeros(m, bool)) + (True,)
    # 180 degree rotations: V = R_pi U, trace R = -1
    s = np.sort(rng.uniform(0.05, 1.0, (m, 3)), axis=1)[:, ::-1]
    A, B = point_sets(rng, s, np.zeros(m, bool))
    ax = rng.normal(size=(m, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    Rpi = 2 * ax[:, :, None] * ax[:, None, :] - np.eye(3)
    out["half_turn"] = (A, A @ np.swapaxes(Rpi, 1, 2), True)
    # mirrored: d = -1, (s2 - s3) / s1 from 0.5 down to 1e-6
    gaps = 10.0 ** np.linspace(np.log10(0.5), -6, 13)
    for g in gaps:
        s3 = rng.uniform(0.05, 0.4, 32)
        out[f"mirrored_gap_{g:.0e}"] = point_sets(rng, _sv(32, 1.0, s3 + g, s3), np.ones(32, bool)) + (True,)
    out["mirrored_tie"] = point_sets(rng, _sv(32, 1.0, 0.3, 0.3), np.ones(32, bool)) + (False,)
    # s3 / s1 from 1e-1 to 1e-15, across the 1e-12 switch of the completion, both signs of d
    for e in range(1, 16):
        mir = np.arange(64) % 2 == 1
        out[f"thin_1e-{e}"] = point_sets(rng, _sv(64, 1.0, rng.uniform(0.2, 0.9, 64), 10.0 ** -e), mir) + (True,)
    # s2 / s1 across the same switch (the second-column completion): not unique below ~eps, so unique only down to 1e-9
    for e in (3, 6, 9, 11, 13, 15):
        out[f"needle_1e-{e}"] = point_sets(rng, _sv(64, 1.0, 10.0 ** -e, 0.0), np.zeros(64, bool)) + (e <= 9,)
    # H from 1e-12 to 1e+12
    for e in range(-12, 13, 3):
        s = np.sort(rng.uniform(0.05, 1.0, (48, 3)), axis=1)[:, ::-1]
        s[16:32, 2] = 0.0
        s[32:, 1:] = 0.0
        A, B = point_sets(rng, s, np.arange(48) % 3 == 1)
        out[f"scale_1e{e:+d}"] = (A * 10.0 ** e, B, False)     # mixed ranks: the unique ones are picked out by their singular values
    return out


FAMILIES = families()


def _H(A, B):
    return np.swapaxes(A, 1, 2) @ B


def _units(s, d):
    """2^-52 s1 / (s2 + d s3): the condition of the rotation (inf where it is not unique)."""
    den = s[:, 1] + d * s[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, EPS * s[:, 0] / den, np.inf)


def _numpy_spread(A, B):
    """max over PERMS row permutations of |R_perm - R| in units of _units, per problem: numpy's own stability."""
    rng = np.random.RandomState(5)
    R0, s, d, _, _ = numpy_fit(_H(A, B))
    worst = np.zeros(len(A))
    for _ in range(PERMS):
        p = rng.permutation(A.shape[1])
        Rp = numpy_fit(_H(A[:, p], B[:, p]))[0]
        worst = np.maximum(worst, np.abs(Rp - R0).max(axis=(1, 2)))
    return worst / _units(s, d)


def _is_unique(s, d):
    """rank >= 2 and a gap: (s2 + d s3) > 1e-10 s1 (below that the bound itself passes 1e-6 and says nothing)."""
    return (s[:, 1] > 1e-10 * s[:, 0]) & (s[:, 1] + d * s[:, 2] > 1e-10 * s[:, 0])


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_solver_is_numpys_rotation(name):
    A, B, unique = FAMILIES[name]
    H = _H(A, B)
    R = solver_rotation(H)
    Rn, s, d, U, V = numpy_fit(H)
    # every case: a finite proper rotation
    assert np.isfinite(R).all(), name
    ortho = np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max()
    det = np.abs(np.linalg.det(R) - 1.0).max()
    assert ortho <= ORTHO_TOL and det <= ORTHO_TOL, (name, ortho, det)
    # the dominant direction where s1 is simple: R u1 = v1 (the singular vector itself moves by ~eps s1 / (s1 - s2))
    simple = (s[:, 0] > 0) & (s[:, 1] <= 0.5 * s[:, 0])
    dirs = 0.0
    if simple.any():
        e = np.abs(np.einsum("bij,bj->bi", R, U[:, :, 0]) - V[:, :, 0]).max(axis=1)[simple]
        dirs = (e / (EPS * s[simple, 0] / (s[simple, 0] - s[simple, 1]))).max()
        assert dirs <= C_BOUND, (name, dirs)
    # the unique rotation
    pick = _is_unique(s, d) if unique or name.startswith("scale_") else np.zeros(len(H), bool)
    if unique:
        assert pick.all(), (name, "the family is meant to be unique")
    worst = spread = 0.0
    if pick.any():
        err = np.abs(R - Rn).max(axis=(1, 2))[pick] / _units(s, d)[pick]
        spread = _numpy_spread(A[pick], B[pick]).max()
        worst = err.max()
    print(f"{name}: {len(H)} problems, {int(pick.sum())} unique; |R - R_numpy| <= {worst:.2f} units (bound {C_BOUND}), "
          f"numpy's own spread {spread:.2f}; |R R^T - I| {ortho:.1e}, |det - 1| {det:.1e}, |R u1 - v1| {dirs:.2f} units")
    assert 4.0 * spread <= C_BOUND, (name, spread, "C_BOUND is no longer 4 x numpy's own spread")
    assert worst <= C_BOUND, (name, worst)


def test_families_are_what_they_claim():
    s = lambda n: np.linalg.svd(_H(*FAMILIES[n][:2]), compute_uv=False)
    assert (s("rank0") == 0).all()
    assert (s("rank1_axis")[:, 1] == 0).all() and ((_H(*FAMILIES["rank1_axis"][:2]) != 0).sum(axis=(1, 2)) == 1).all()
    H = _H(*FAMILIES["rank2_exact_zeros"][:2])
    assert ((H[:128] == 0).all(axis=2).sum(axis=1) == 1).all() and ((H[128:] == 0).all(axis=1).sum(axis=1) == 1).all()
    for n in ("rank1", "rank2"):
        r = s(n)
        assert (r[:, 2] < 1e-15 * r[:, 0]).all() and ((r[:, 1] < 1e-15 * r[:, 0]).all() == (n == "rank1"))
    Rn = numpy_fit(_H(*FAMILIES["half_turn"][:2]))[0]
    assert np.abs(np.trace(Rn, axis1=1, axis2=2) + 1.0).max() < 1e-12
    r = s("three_equal")
    assert np.abs(r[:, 0] / r[:, 2] - 1).max() < 1e-14
    for n in FAMILIES:
        if n.startswith("mirrored"):
            assert (numpy_fit(_H(*FAMILIES[n][:2]))[2] == -1).all(), n
        if n.startswith("thin_"):                                 # on the intended side of the 1e-12 switch
            r, e = s(n), int(n.split("-")[1])
            if e <= 11:
                assert (r[:, 2] > 2e-12 * r[:, 0]).all(), n
            if e >= 13:
                assert (r[:, 2] < 5e-13 * r[:, 0]).all(), n
    assert sum(len(v[0]) for v in FAMILIES.values()) >= 4000


def test_packed_form_rounds_once():
    rng = np.random.RandomState(3)
    A, B, _ = FAMILIES["full_rank"]
    H = _H(A, B)
    ca, cb = rng.normal(size=(len(H), 3)) * 100.0, rng.normal(size=(len(H), 3)) * 100.0
    T = solver_pack(H, ca, cb)
    R = solver_rotation(H)
    assert (T[:, :, :3] == R.astype(np.float32)).all()
    R32 = T[:, :, :3].astype(np.float64)
    t64 = cb - ((R32[:, :, 0] * ca[:, None, 0] + R32[:, :, 1] * ca[:, None, 1]) + R32[:, :, 2] * ca[:, None, 2])
    half_ulp = np.spacing(np.abs(t64).astype(np.float32)).astype(np.float64) / 2
    assert (np.abs(T[:, :, 3].astype(np.float64) - t64) <= half_ulp * (1 + 1e-6)).all()


# ---- the scenes ------------------------------------------------------------------------------------------------------
SCENE_ROWS = (20, 32, 64)            # the k2 subset of a seed, a seed's rows, the RANSAC set


def scene_fit(src, tgt, w=None):
    """Two-pass fp64 fit of a correspondence set: (R, t, s, d, centroid of src, H)."""
    a, b = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    w = np.ones(len(a)) if w is None else np.asarray(w, dtype=np.float64)
    ca, cb = (w[:, None] * a).sum(0) / w.sum(), (w[:, None] * b).sum(0) / w.sum()
    H = (a - ca).T @ (w[:, None] * (b - cb))
    R, s, d, _, _ = numpy_fit(H[None])
    return R[0], cb - R[0] @ ca, s[0], d[0], ca, H


# s3 / s1 and s2 / s1 against the solver's 1e-12 switches.  A set whose side is its very claim is pinned a decade clear of
# the switch: full rank above, exact zeros and the sets that are flat or straight to float32 rounding near the origin below.
# The same rounding-flat sets at SHIFT, where an ulp is 3e-5 m, have ratios of (rounding / extent)^2 ~ 1e-12: they sit AT the
# switch, on either side depending on the rows taken (printed), which is what they are for -- the answer must not depend
# on the branch.
SWITCH = 1e-12


@pytest.mark.parametrize("name,shifted", KS.cases(), ids=[KS.label(*c) for c in KS.cases()])
def test_every_scene_is_what_it_claims(name, shifted):
    for n in SCENE_ROWS:
        src, tgt, R, t = KS.corr_set(name, n, shifted)
        assert src.dtype == np.float32 and tgt.dtype == np.float32 and src.shape == tgt.shape == (n, 3)
        if shifted:
            assert np.abs(src.mean(0) - KS.SHIFT).max() < 8 and np.abs(tgt.mean(0) - KS.SHIFT).max() < 8
        Rf, tf, s, d, ca, H = scene_fit(src, tgt)
        r2, r3 = (s[1] / s[0], s[2] / s[0]) if s[0] > 0 else (0.0, 0.0)
        print(f"{KS.label(name, shifted)} n={n}: s = {s}, s2/s1 = {r2:.2e}, s3/s1 = {r3:.2e}, d = {d:+.0f}")
        print(f"    completes: second column {r2 <= SWITCH}, third column {r3 <= SWITCH}")
        if KS.RANK[name] == 3 and name != "slab_1e-6":           # full rank: no completion
            assert r3 > 10 * SWITCH, (name, shifted, n, r3)
        if name in ("planar", "collinear", "slab_1e-6") and not shifted:      # flat / straight to rounding: completed
            assert r3 < SWITCH / 10 and (r2 < SWITCH / 10 or name != "collinear"), (name, n, r2, r3)
        if KS.RANK[name] >= 2:
            assert r2 > 10 * SWITCH
        # ransac_oracle's borderline switch (s2 < 1e-6 s1)
        assert (r2 < 1e-7) == (KS.RANK[name] <= 1), (name, shifted, n, r2)
        if name in ("planar_exact", "collinear_exact", "coincident"):
            assert (H == 0).all(axis=1).sum() == 3 - KS.RANK[name] and s[KS.RANK[name]:].max(initial=0.0) == 0.0
        if name == "isotropic":
            assert s[2] > (0.9999 if shifted else 0.999999) * s[0]   # the float32 rounding of the target breaks the tie
        if name == "half_turn":
            assert abs(np.trace(R) + 1) < 1e-12
        assert d == (-1 if name == "mirrored" else 1) or KS.RANK[name] < 3
        resid = np.abs(src.astype(np.float64) @ R.T + t - tgt).max()
        if name in KS.RIGID:                                     # exact under (R, t) up to the float32 rounding of the target
            assert resid <= np.spacing(np.abs(tgt).max()) * 0.5 * (1 + 1e-6), (name, resid)
        else:
            assert resid > 0.1
        if name in KS.UNIQUE:                                    # the reference alone is stable: the gap
            gap = (s[1] + d * s[2]) / s[0]
            assert gap >= 1e-3, (name, shifted, n, gap)
            if name in KS.RIGID:
                lever = np.abs(src - ca).max()
                assert np.abs(Rf - R).max() * lever < 64 * np.spacing(np.abs(tgt).max()) / gap


# ---- RANSAC: what the GPU test asserts, shown with numpy alone first ------------------------------------------------------
RANSAC = dict(n=64, max_corr_distance=0.05, max_iteration=256, seed=12345)


@functools.lru_cache(maxsize=None)
def ransac_reference(name, shifted, ransac_n):
    src, tgt, _, _ = KS.corr_set(name, RANSAC["n"], shifted)
    return RO.ransac(src, tgt, ransac_n, 0.0, 0.0, RANSAC["max_corr_distance"], RANSAC["max_iteration"], 1.0,
                     RANSAC["seed"], 256)


def ransac_claim(name, r):
    """(hypotheses that must count every row, hypotheses that must count at least their own sample) of a rigid scene.

    On a line or in a point ANY proper rotation that maps the sample maps every row, so every drawn hypothesis counts all of
    them.  In a set of rank >= 2 that holds for every sample that spans a plane; a sample that happens to be collinear there
    (three lattice points of planar_exact on one line, three face centres of one axis of the cube) fixes the pose only up
    to a turn about its line, which no solver can be held to -- ransac_oracle's existing borderline rule, s2 < 1e-6 s1 of
    the SAMPLE, names exactly those.  They must still carry their own rows: a count of at least ransac_n."""
    drawn = r["status"] != -3
    if KS.RANK[name] <= 1:
        return drawn, np.zeros_like(drawn)
    return drawn & ~r["borderline"], drawn & r["borderline"]


@pytest.mark.parametrize("ransac_n", (3, 4))
@pytest.mark.parametrize("name,shifted", KS.cases(), ids=[KS.label(*c) for c in KS.cases()])
def test_every_sample_of_a_rigid_scene_fits_every_row(name, shifted, ransac_n):
    r = ransac_reference(name, shifted, ransac_n)
    drawn = r["status"] != -3
    assert drawn.sum() > 200
    if name in KS.RIGID:
        drawn, thin = ransac_claim(name, r)
        assert (r["status"][drawn] == RANSAC["n"]).all(), (name, shifted, np.unique(r["status"]))
        assert (r["status"][thin] >= ransac_n).all() and thin.sum() <= 32
        src, tgt, _, _ = KS.corr_set(name, RANSAC["n"], shifted)
        d = np.linalg.norm(np.einsum("bij,nj->bni", r["R"][drawn], src.astype(np.float64)) + r["t"][drawn][:, None] -
                           tgt[None].astype(np.float64), axis=2).max()
        print(f"{KS.label(name, shifted)} ransac_n={ransac_n}: worst row under any sample's pose {d:.2e} m (inlier distance 0.05)")
        assert d < 0.025                                         # a factor of two inside the inlier distance: fp32 cannot flip it
    else:
        assert r["winner"] >= 0 and (r["status"][drawn] < RANSAC["n"]).all()


# ---- ICP: the margins that make "same correspondences, same update count" a fair demand --------------------------------------
D2_MARGIN, CRITERIA_MARGIN = 1e-8, 1e-9


def icp_iterations(name):
    return (1, 30) if name in KS.UNIQUE else (1,)


@pytest.mark.parametrize("name,shifted", KS.cases(), ids=[KS.label(*c) for c in KS.cases()])
def test_margins_of_the_icp_pairs(name, shifted):
    src, tgt, G, init = KS.icp_pair(name, shifted)
    assert 3 <= len(src) <= 300 and len(tgt) <= 300
    for it in icp_iterations(name):
        r = IO.icp(src, tgt, KS.ICP_RADIUS, init, it)
        m = r["margins"]
        assert r["status"] == 0 and r["n_corr"] == len(src) and r["updates"] >= 1
        assert m["gap"] > D2_MARGIN and m["radius"] > D2_MARGIN and m["criteria"] > CRITERIA_MARGIN, (name, shifted, it, m)
        if name in KS.UNIQUE and it == 30:
            x = np.concatenate([src.astype(np.float64), np.ones((len(src), 1))], axis=1)
            assert np.abs(x @ (r["T"] - G).T).max() < 1e-4 and r["updates"] < 30      # the planted motion, through the points


# ---- what the GPU file shares: the two references of a packed pose and their disagreement ----------------------------------
REFINE_ROWS = (1, 3, 64, 1024, 1025)
REFINE_THR = 1e4


def weighted_fit64(src, tgt, w, eps=1e-6):
    """fp64 restatement of common.py:7-45 (rigid_transform_3d): [R | t] float64 [3, 4], and (s, d) of its H."""
    a, b, w = (np.asarray(x, dtype=np.float64) for x in (src, tgt, w))
    sw = w.sum() + eps
    ca, cb = (w[:, None] * a).sum(0) / sw, (w[:, None] * b).sum(0) / sw
    H = (a - ca).T @ (w[:, None] * (b - cb))
    R, s, d, _, _ = numpy_fit(H[None])
    return np.concatenate([R[0], (cb - R[0] @ ca)[:, None]], axis=1), s[0], d[0]


def torch_fit32(src, tgt, w):
    """The repository's float32 torch oracle (oracle/sc2pcr_oracle.rigid_transform_3d) as float64 [3, 4]."""
    import torch
    from oracle.sc2pcr_oracle import rigid_transform_3d
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None]
    return rigid_transform_3d(f(src), f(tgt), f(w))[0, :3].double().numpy()


def move(T, x):
    return np.asarray(x, dtype=np.float64) @ T[:, :3].T + T[:, 3]


def packed_bounds(Ta, Tb, pts, coord_max):
    """(bound through the points, bound on R) of a packed fp32 pose: 4 x the disagreement of the two references, floored at
    one fp32 ulp of the largest coordinate (of 1 for R)."""
    through = max(np.abs(move(Ta, pts) - move(Tb, pts)).max(), float(np.spacing(np.float32(coord_max))))
    rot = max(np.abs(Ta[:, :3] - Tb[:, :3]).max(), 2.0 ** -23)
    return 4.0 * through, 4.0 * rot


def refine_weights(src, tgt):
    """The weights of one refinement step from T = identity under REFINE_THR, in float32 like the reference and the kernel."""
    d = np.linalg.norm(src.astype(np.float64) - tgt.astype(np.float64), axis=1).astype(np.float32)
    return (1 / (1 + (d / np.float32(REFINE_THR)) ** 2)).astype(np.float32)


def is_unique(name, s, d):
    """One best rotation, and a reference that is stable there: the set's claim and a gap of 1e-3."""
    return name in KS.UNIQUE and s[0] > 0 and (s[1] + d * s[2]) / s[0] >= 1e-3


@pytest.mark.parametrize("name,shifted", KS.cases(), ids=[KS.label(*c) for c in KS.cases()])
def test_refine_sets_have_their_gap(name, shifted):
    for n in REFINE_ROWS:
        src, tgt, _, _ = KS.corr_set(name, n, shifted)
        assert np.linalg.norm(src.astype(np.float64) - tgt, axis=1).max() < 0.01 * REFINE_THR      # every row an inlier, far from thr
        w = refine_weights(src, tgt)
        T64, s, d = weighted_fit64(src, tgt, w)
        assert is_unique(name, s, d) == (name in KS.UNIQUE and n >= 3), (name, shifted, n, s, d)
        T32 = torch_fit32(src, tgt, w)
        assert np.isfinite(T32).all() and np.isfinite(T64).all()


# the seeds of gcl_sc2_seed_trans: one per scene, 32 rows each, the k2 = 20 subset is rows 0 .. 19 because every pair of rows is
# compatible (also in the mirrored set: a mirror keeps distances)
SEED = dict(k1=32, k2=20, d_thre=0.1, num_iterations=20, inlier_thresh=0.1)


@functools.lru_cache(maxsize=None)
def seed_case():
    """src, tgt float32 [24 * 32, 3], knn int32 [24, 32], the float32 torch oracle's [24, 3, 4] (centroids and H in float32 as
    the reference), the fp64 fit with the oracle's weights [24, 3, 4], per-seed (s, d), the oracle's inlier counts and the
    smallest |distance - inlier_thresh| of any (seed, row)."""
    import torch
    from oracle.sc2pcr_oracle import leading_eigenvector, rigid_transform_3d
    sets = [KS.corr_set(name, SEED["k1"], shifted) for name, shifted in KS.cases()]
    src, tgt = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    S = len(sets)
    knn = (np.arange(S)[:, None] * SEED["k1"] + np.arange(SEED["k1"])[None]).astype(np.int32)
    k2 = SEED["k2"]
    s_f = torch.from_numpy(src).view(S, SEED["k1"], 3)[:, :k2].contiguous()
    t_f = torch.from_numpy(tgt).view(S, SEED["k1"], 3)[:, :k2].contiguous()
    cd = torch.abs(torch.norm(s_f[:, :, None] - s_f[:, None], dim=-1) - torch.norm(t_f[:, :, None] - t_f[:, None], dim=-1))
    lsc = torch.clamp(1 - cd ** 2 / SEED["d_thre"] ** 2, min=0)
    ar = torch.arange(k2)
    lsc[:, ar, ar] = 0
    wgt = leading_eigenvector(lsc, SEED["num_iterations"], early_stop=False)
    wgt = wgt / (wgt.sum(-1, keepdim=True) + 1e-6)
    T32 = rigid_transform_3d(s_f, t_f, wgt)[:, :3].double().numpy()
    fits = [weighted_fit64(s_f[i].numpy(), t_f[i].numpy(), wgt[i].numpy()) for i in range(S)]
    T64 = np.stack([f[0] for f in fits])
    dist = np.stack([np.linalg.norm(move(T32[i], src) - tgt, axis=1) for i in range(S)])
    counts = (dist < SEED["inlier_thresh"]).sum(1)
    return dict(src=src, tgt=tgt, knn=knn, T32=T32, T64=T64, sd=[(f[1], f[2]) for f in fits], counts=counts,
                margin=float(np.abs(dist - SEED["inlier_thresh"]).min()), dist=dist)


def test_seed_case_is_what_the_gpu_test_assumes():
    c = seed_case()
    k1 = SEED["k1"]
    for i, (name, shifted) in enumerate(KS.cases()):
        a, b = c["src"][i * k1:(i + 1) * k1].astype(np.float64), c["tgt"][i * k1:(i + 1) * k1].astype(np.float64)
        cd = np.abs(np.linalg.norm(a[:, None] - a[None], axis=-1) - np.linalg.norm(b[:, None] - b[None], axis=-1))
        assert cd.max() < 0.01 * SEED["d_thre"], (name, shifted, cd.max())          # every pair compatible, far from d_thre
        own = c["dist"][i, i * k1:(i + 1) * k1]
        print(f"{KS.label(name, shifted)}: oracle count {c['counts'][i]}, own rows within {own.max():.2e}")
        if name in KS.RIGID:                                     # its own 32 rows, and whatever rows of OTHER sets its pose happens to fit
            assert c["counts"][i] >= k1 and own.max() < 0.1 * SEED["inlier_thresh"], (name, shifted, c["counts"][i], own.max())
        assert is_unique(name, *c["sd"][i]) == (name in KS.UNIQUE)
    # no (seed, row) distance near the inlier distance: the count is the same in float32 and under a pose off by the bound
    print(f"smallest |distance - inlier_thresh| = {c['margin']:.3e}")
    assert c["margin"] > 1.5e-3


# ---- the one-pass centring of the ICP update: K ------------------------------------------------------------------------------
K_ICP = 12.0                 # 4 x 2.83 (isotropic+far), rounded up: in units of 2^-53 |c|^2 / (sigma2^2 + d sigma3^2)


def icp_first_step(name, shifted):
    """(p, q, corr): the matched rows of the first evaluation of an ICP pair (init = identity)."""
    src, tgt, _, init = KS.icp_pair(name, shifted)
    corr = IO.nearest(src.astype(np.float64), tgt.astype(np.float64), KS.ICP_RADIUS ** 2)[0]
    assert (corr >= 0).all()
    return src.astype(np.float64), tgt.astype(np.float64)[corr], corr


def centring_units(p, q):
    """2^-53 |c|^2 / (sigma2^2 + d sigma3^2) of a matched set (sigma^2: the singular values of H / n), inf if not unique."""
    _, _, s, d, ca, _ = scene_fit(p, q)
    den = (s[1] + d * s[2]) / len(p)
    c2 = max((ca ** 2).sum(), (q.mean(0) ** 2).sum())
    return 2.0 ** -53 * c2 / den if den > 0 else np.inf


def test_one_pass_centring_constant():
    worst = 0.0
    rng = np.random.RandomState(1)
    for name, shifted in KS.cases():
        if name not in KS.UNIQUE:
            continue
        p, q, _ = icp_first_step(name, shifted)
        R2 = scene_fit(p, q)[0]
        unit = centring_units(p, q)
        dev = 0.0
        for _ in range(64):
            o = rng.permutation(len(p))
            pp, qq = p[o], q[o]
            n = len(pp)
            H1 = pp.T @ qq - n * np.outer(pp.sum(0) / n, qq.sum(0) / n)
            dev = max(dev, np.abs(numpy_fit(H1[None])[0][0] - R2).max())
        print(f"{KS.label(name, shifted)}: one pass against two passes |dR| = {dev:.2e} = {dev / unit if unit > 0 else 0:.3f} units "
              f"({unit:.2e})")
        if shifted:
            worst = max(worst, dev / unit)
        else:
            assert dev < 1e-12                                   # centred grids: the term vanishes, R_TOL alone holds
    print(f"largest deviation {worst:.3f} units; K_ICP = {K_ICP}")
    assert 4 * worst <= K_ICP
