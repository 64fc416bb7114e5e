"""FPFH on the GPU (gcl_amd/lib/fpfh.py, csrc/fpfh.hip) against the numpy oracle (tests/fpfh_oracle.py), stage by stage:
every stage is predicted from the PRODUCT's previous stage, so a stage's tolerance covers that stage alone.

  neighbours  bit for bit (idx and cnt), any number of in-radius candidates, batches through ``offsets``
  normals     1e-6 per component where the eigen problem is well conditioned (gap >= 1e-3, view-ray cosine >= 1e-6): the
              fp64 eigenvector error is <= ~1e-16 / gap = 1e-13, what remains is the float32 rounding, 6e-8
  SPFH        bit for bit where no pair feature lies within 1e-9 bins of a bin edge (integer counts)
  FPFH        1e-4 per entry (entries <= 200, one float32 ulp there is 1.5e-5; the sums are fp64)
  end to end  1-NN matching of two overlapping views and one SC2-PCR benchmark record
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as O                                                # noqa: E402
import fpfh_scene as S                                                 # noqa: E402

DEV = "cuda:0"
SEEDS = (0, 1)
PARAMS = ((0.10, 30), (0.25, 100))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _scene(seed):
    X = S.scene(seed)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _oracle_lists(seed, radius, max_nn):
    idx, cnt, ncand = O.neighbours(_scene(seed), radius, max_nn)
    for a in (idx, cnt, ncand):
        a.setflags(write=False)
    return idx, cnt, ncand


@functools.lru_cache(maxsize=None)
def _gpu_stages(seed):
    """The product's stages on the scene, each from the previous one: (normals, idx, cnt, spfh, fpfh) as numpy."""
    from gcl_amd.lib import fpfh as F
    with torch.cuda.device(DEV):
        x = _t(_scene(seed))
        nrm = F.estimate_normals(x, 0.10, 30)
        idx, cnt = F.radius_neighbours(x, 0.25, 100)
        sp = F.spfh_from_neighbours(x, nrm, idx, cnt)
        f = F.fpfh_from_spfh(x, sp, idx, cnt)
        out = tuple(a.cpu().numpy() for a in (nrm, idx, cnt, sp, f))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. neighbours ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,max_nn", PARAMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_neighbour_lists_equal_the_oracle_exactly(seed, radius, max_nn):
    from gcl_amd.lib import fpfh as F
    want_idx, want_cnt, ncand = _oracle_lists(seed, radius, max_nn)
    assert ncand.max() > 2 * max_nn and want_cnt.min() == 1            # lists cut by max_nn, and an isolated point
    with torch.cuda.device(DEV):
        idx, cnt = F.radius_neighbours(_t(_scene(seed)), radius, max_nn)
    assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and tuple(idx.shape) == (len(want_idx), max_nn)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert (cnt == want_cnt).all(), np.nonzero(cnt != want_cnt)[0][:10]
    bad = np.nonzero((idx != want_idx).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], idx[bad[:1]], want_idx[bad[:1]])


def test_neighbours_with_1100_candidates_per_query():
    from gcl_amd.lib import fpfh as F
    X = (np.random.RandomState(7).uniform(0.0, 0.1, size=(1100, 3)) + S.SHIFT).astype(np.float32)
    want_idx, want_cnt, ncand = O.neighbours(X, 0.25, 100)
    assert (ncand == 1100).all()
    with torch.cuda.device(DEV):
        idx, cnt = F.radius_neighbours(_t(X), 0.25, 100)
    assert (cnt.cpu().numpy() == want_cnt).all() and (idx.cpu().numpy() == want_idx).all()


@pytest.mark.parametrize("n,max_nn", [(1, 1), (1, 128), (5, 1), (67, 3), (130, 128)])
def test_neighbours_small_clouds_and_list_lengths(n, max_nn):
    from gcl_amd.lib import fpfh as F
    X = (np.random.RandomState(n).uniform(0.0, 0.3, size=(n, 3)) - 0.15).astype(np.float32)   # cells on both sides of 0
    if n > 2:
        X[n // 2] = X[0]                                               # a duplicate: ordered by row
    want_idx, want_cnt, _ = O.neighbours(X, 0.12, max_nn)
    with torch.cuda.device(DEV):
        idx, cnt = F.radius_neighbours(_t(X), 0.12, max_nn)
    assert (cnt.cpu().numpy() == want_cnt).all() and (idx.cpu().numpy() == want_idx).all()


def test_a_batch_through_offsets_equals_its_clouds_run_alone():
    from gcl_amd.lib import fpfh as F
    A, B = _scene(0), _scene(1)[3:]                                    # 1636 + 1633 rows: no multiple of a block's 4 queries
    off = [0, len(A), len(A) + len(B)]
    vp = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]], dtype=np.float32)
    with torch.cuda.device(DEV):
        a, b, ab = _t(A), _t(B), _t(np.concatenate([A, B]))
        for radius, max_nn in PARAMS:
            idx, cnt = F.radius_neighbours(ab, radius, max_nn, offsets=off)
            ia, ca = F.radius_neighbours(a, radius, max_nn)
            ib, cb = F.radius_neighbours(b, radius, max_nn)
            ib = torch.where(ib >= 0, ib + len(A), ib)
            assert torch.equal(idx, torch.cat([ia, ib])) and torch.equal(cnt, torch.cat([ca, cb])), (radius, max_nn)
        # the whole recipe, with a viewpoint per cloud and an EMPTY cloud between the two
        off3 = np.array([0, len(A), len(A), len(A) + len(B)])
        vp3 = np.stack([vp[0], [9.0, 9.0, 9.0], vp[1]]).astype(np.float32)
        n_ab, f_ab = F.fpfh_descriptors(ab, 0.05, viewpoint=vp3, offsets=off3)
        n_a, f_a = F.fpfh_descriptors(a, 0.05, viewpoint=vp[0])
        n_b, f_b = F.fpfh_descriptors(b, 0.05, viewpoint=_t(vp[1]))
        assert torch.equal(n_ab, torch.cat([n_a, n_b])) and torch.equal(f_ab, torch.cat([f_a, f_b]))


# ---- 2. normals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_normals_match_the_oracle_on_well_conditioned_points(seed):
    from gcl_amd.lib import fpfh as F
    X = _scene(seed)
    o_idx, o_cnt, _ = _oracle_lists(seed, 0.10, 30)
    want, gap, cosv = O.normals(X, o_idx, o_cnt)
    with torch.cuda.device(DEV):
        x = _t(X)
        from_oracle = F.normals_from_neighbours(x, _t(o_idx), _t(o_cnt)).cpu().numpy()
        g_idx, g_cnt = F.radius_neighbours(x, 0.10, 30)
        from_gpu = F.normals_from_neighbours(x, g_idx, g_cnt).cpu().numpy()
        whole = F.estimate_normals(x, 0.10, 30).cpu().numpy()
    assert from_oracle.tobytes() == from_gpu.tobytes() == whole.tobytes()
    few = o_cnt < 3
    assert few.sum() >= 5 and (from_gpu[few] == np.array([0, 0, 1], dtype=np.float32)).all()
    good = ~few & (gap >= 1e-3) & (cosv >= 1e-6)
    excluded = 1.0 - (good | few).mean()
    err = np.abs(from_gpu.astype(np.float64) - want.astype(np.float64))[good]
    print(f"normals seed {seed}: max |delta| {err.max():.3e} over {good.sum()} points, excluded {excluded:.4f}, "
          f"smallest gap {gap.min():.3e}, smallest cosine {cosv.min():.3e}")
    assert excluded <= 0.01
    assert err.max() <= 1e-6
    assert np.abs(np.linalg.norm(from_gpu.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


def test_normals_turn_with_the_viewpoint():
    from gcl_amd.lib import fpfh as F
    X = _scene(0)
    with torch.cuda.device(DEV):
        x = _t(X)
        n0 = F.estimate_normals(x, 0.10, 30).cpu().numpy().astype(np.float64)
        vp = np.array([3.0, 4.0, 5.0], dtype=np.float32)                # beyond the scene, on the other side
        n1 = F.estimate_normals(x, 0.10, 30, viewpoint=vp).cpu().numpy().astype(np.float64)
    cnt = _oracle_lists(0, 0.10, 30)[1]
    ok = cnt >= 3
    assert (np.einsum("ij,ij->i", n0, -X.astype(np.float64))[ok] >= 0).all()
    assert (np.einsum("ij,ij->i", n1, vp.astype(np.float64) - X)[ok] >= 0).all()
    same = np.abs(n0 - n1).max(axis=1) == 0
    assert ((same | (np.abs(n0 + n1).max(axis=1) == 0))[ok]).all() and same[ok].any() and (~same[ok]).any()


# ---- 3. SPFH ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_spfh_rows_are_bit_equal_away_from_bin_edges(seed):
    X = _scene(seed)
    nrm, idx, cnt, sp, _ = _gpu_stages(seed)
    o_idx, o_cnt, _ = _oracle_lists(seed, 0.25, 100)
    assert (idx == o_idx).all() and (cnt == o_cnt).all()
    want, edge = O.spfh(X, nrm, idx, cnt)                              # from the GPU's own float32 normals
    good = edge >= 1e-9
    excluded = 1.0 - good.mean()
    diff = (sp != want).any(axis=1)
    print(f"spfh seed {seed}: rows that differ {diff.sum()} (away from edges {(diff & good).sum()}), excluded "
          f"{excluded:.4f}, smallest edge distance {edge.min():.3e} bins")
    assert excluded <= 0.005
    assert sp[good].tobytes() == want[good].tobytes()
    assert not sp[cnt <= 1].any()


# ---- 4. FPFH ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_fpfh_from_the_gpu_spfh(seed):
    from gcl_amd.lib import fpfh as F
    X = _scene(seed)
    nrm, idx, cnt, sp, f = _gpu_stages(seed)
    want = O.fpfh(X, sp, idx, cnt)
    err = np.abs(f.astype(np.float64) - want.astype(np.float64))
    print(f"fpfh seed {seed}: max |delta| {err.max():.3e}, largest entry {f.max():.3f}")
    assert f.max() <= 200.0 + 1e-4
    assert err.max() <= 1e-4
    zero = ~want.any(axis=1)
    assert zero.sum() >= 1 and not f[zero].any()                       # the isolated point: exactly zero
    with torch.cuda.device(DEV):
        x = _t(X)
        fn = F.fpfh_from_spfh(x, _t(sp), _t(idx), _t(cnt), normalize=True).cpu().numpy()
        whole = F.compute_fpfh_feature(x, _t(nrm), 0.25, 100).cpu().numpy()
        whole_n = F.compute_fpfh_feature(x, _t(nrm), 0.25, 100, normalize=True).cpu().numpy()
    assert whole.tobytes() == f.tobytes() and whole_n.tobytes() == fn.tobytes()
    nerr = np.abs(fn.astype(np.float64) - O.normalized(f).astype(np.float64)).max()
    print(f"fpfh seed {seed}: normalised, max |delta| to the formula {nerr:.3e}")
    assert nerr <= 1e-6


# ---- 5. end to end ---------------------------------------------------------------------------------------
def _share(A, keep, nn):
    err = np.linalg.norm(A[nn].astype(np.float64) - A[keep].astype(np.float64), axis=1)
    return float((err < 0.05).mean())


@pytest.mark.parametrize("seed", SEEDS)
def test_two_views_match_as_well_as_with_the_oracle_descriptors_and_register(seed):
    from gcl_amd.lib import fpfh as F
    from gcl_amd.lib.metrics import pdist_min
    from gcl_amd.scripts.SC2_PCR import Matcher
    from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair
    A, B, keep, T, vp_b = S.pair(seed)
    _, fa_o = O.fpfh_descriptors(A, 0.05)
    _, fb_o = O.fpfh_descriptors(B, 0.05, viewpoint=vp_b)
    d = ((fb_o[:, None, :].astype(np.float64) - fa_o[None].astype(np.float64)) ** 2).sum(axis=2)
    share_oracle = _share(A, keep, d.argmin(axis=1))
    with torch.cuda.device(DEV):
        a, b = _t(A), _t(B)
        _, fa = F.fpfh_descriptors(a, 0.05)
        _, fb = F.fpfh_descriptors(b, 0.05, viewpoint=vp_b)
        assert tuple(fa.shape) == (len(A), 33) and fa.dtype == torch.float32
        _, nn = pdist_min(fb, fa, "SquareL2")
        share_gpu = _share(A, keep, nn.cpu().numpy().astype(np.int64))
        print(f"pair seed {seed}: share within 0.05: gpu {share_gpu:.4f}, oracle descriptors {share_oracle:.4f}")
        assert share_oracle > 0.5                                      # the scene is a matchable one
        assert share_gpu >= share_oracle - 0.02
        matcher = Matcher(inlier_threshold=0.10, num_node="all", use_mutual=False, d_thre=0.1, num_iterations=10, ratio=0.2,
                          nms_radius=0.1, max_points=8000, k1=30, k2=20)
        stats = eval_per_pair([(a, b, fa, fb, T.astype(np.float32))], matcher,
                              dict(inlier_threshold=0.10, re_thre=15.0, te_thre=30.0))
    print(f"pair seed {seed}: success {stats[0, 0]}, RE {stats[0, 1]:.3f} deg, TE {stats[0, 2]:.3f} cm, "
          f"input inlier ratio {stats[0, 4]:.3f}")
    assert stats[0, 0] == 1
