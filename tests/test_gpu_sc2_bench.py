"""The SC2-PCR benchmark on the GPU: the feature 1-NN at any width (gcl_nn_rowmin_any) against the fp64 oracle, the per-pair
statistics of a batch in one launch (gcl_registration_stats) against the reference's recorded values, and the benchmark loop
(``SC2_PCR_bench.eval_per_pair``) batched against pair by pair.

Shapes are the smallest that reach the edges: the 64-row A tile (65, 67, 130 rows), an odd B count (the unpaired last row),
several B chunks with a merge (203 columns), padded widths from 8 to 128 and both ways the kernel fetches a B row (whole
up to 40 channels; in groups of 16 above, with a last group of 8 at 65 -> 72 channels)."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402
import sc2_bench_oracle as SO                                          # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = sorted(glob.glob(os.path.join(G, "sc2_bench_s[0-2].npz")))
WIDTHS = (1, 3, 8, 33, 40, 63, 65, 96, 128)
SHAPES = ((1, 1), (65, 2), (130, 9), (67, 203))
EPS = 2.0 ** -23


def _call(entry, A, B, rows_a=None, rows_b=None, l2=0):
    """A direct C-ABI call of ``gcl_nn_rowmin`` / ``gcl_nn_rowmin_any`` on device tensors -> (dmin, argmin) on the host."""
    from gcl_amd import _lib
    lib = _lib.load()
    ma = len(A) if rows_a is None else len(rows_a)
    mb = len(B) if rows_b is None else len(rows_b)
    c = A.shape[1]
    ns = lib.gcl_nn_rowmin_scratch_len(ma, mb) if entry == "gcl_nn_rowmin" else lib.gcl_nn_rowmin_any_scratch_len(ma, mb, c)
    assert ns > 0
    scratch = torch.full((ns,), -1, dtype=torch.int32, device=DEV)      # stale words: the call initialises what it reads
    dmin = torch.empty(ma, dtype=torch.float32, device=DEV)
    arg = torch.empty(ma, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(getattr(lib, entry)(_lib.ptr(A), _lib.ptr(rows_a), ma, _lib.ptr(B), _lib.ptr(rows_b), mb, c, l2,
                                       _lib.ptr(scratch), _lib.ptr(dmin), _lib.ptr(arg), _lib.stream()), entry)
    return dmin.cpu().numpy(), arg.cpu().numpy()


def _separated(rng, ma, mb, c):
    """A [ma, c], B [mb, c] fp32 whose every row's best and second-best fp64 distances differ by more than
    4 (c + 2) 2^-23 relative (redrawn until they do): the fp32 arg-minimum is then the oracle's."""
    while True:
        A, B = rng.normal(size=(ma, c)).astype(np.float32), rng.normal(size=(mb, c)).astype(np.float32)
        d2, arg, gap = EO.nn(A, B, with_gap=True)
        if (np.isinf(gap) | (gap > 4 * (c + 2) * EPS * (d2 + gap))).all():      # one column: no second best (inf)
            return A, B, d2, arg


@pytest.mark.parametrize("c", WIDTHS)
def test_nn_any_width_matches_the_fp64_oracle(c):
    rng = np.random.RandomState(100 + c)
    for ma, mb in SHAPES:
        A, B, d2, arg = _separated(rng, ma, mb, c)
        # without row lists, then the same search through row lists into larger matrices (shuffled, with unused rows)
        pa, pb = rng.permutation(ma + 7)[:ma], rng.permutation(mb + 5)[:mb]
        A_big, B_big = rng.normal(size=(ma + 7, c)).astype(np.float32), rng.normal(size=(mb + 5, c)).astype(np.float32)
        A_big[pa], B_big[pb] = A, B
        for rows in (False, True):
            tA = torch.from_numpy(A_big if rows else A).to(DEV)
            tB = torch.from_numpy(B_big if rows else B).to(DEV)
            ra = torch.from_numpy(pa).to(DEV) if rows else None
            rb = torch.from_numpy(pb).to(DEV) if rows else None
            dmin, got = _call("gcl_nn_rowmin_any", tA, tB, ra, rb)
            assert (got == arg).all(), (c, ma, mb, rows)
            err = np.abs(dmin.astype(np.float64) - d2) / np.maximum(d2, 1e-300)
            assert err.max() <= (c + 2) * EPS, (c, ma, mb, rows, err.max())
        # l2: sqrt(d2 + 1e-7); half the relative error of d2 + 1e-7 (<= (c + 2) / 2 ulp, plus 1/2 for the rounded sum) and
        # the rounding of the root itself (1 ulp)
        dl2, got = _call("gcl_nn_rowmin_any", torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), l2=1)
        want = np.sqrt(d2 + 1e-7)
        assert (got == arg).all() and (np.abs(dl2 - want) / want).max() <= ((c + 2) / 2 + 1.5) * EPS


@pytest.mark.parametrize("c", (3, 33, 96))
def test_nn_any_exact_ties_go_to_the_lowest_index(c):
    """B holds five distinct rows, each many times, spread over every chunk and wave; A holds copies of them and random rows."""
    rng = np.random.RandomState(7 + c)
    while True:
        U = rng.normal(size=(5, c)).astype(np.float32)
        A = np.concatenate([U[rng.randint(0, 5, 30)], rng.normal(size=(37, c)).astype(np.float32)])
        d2, _, gap = EO.nn(A, U, with_gap=True)
        if (gap > 4 * (c + 2) * EPS * (d2 + gap)).all():
            break
    for mb in (9, 203):
        pick = rng.permutation(np.concatenate([np.arange(5), rng.randint(0, 5, mb - 5)]))
        B = U[pick]
        d2, arg = EO.nn(A, B)                                            # np.argmin: the first of equal minima
        assert (d2[:30] == 0).all()
        dmin, got = _call("gcl_nn_rowmin_any", torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV))
        assert (got == arg).all() and (dmin[:30] == 0).all()


def test_nn_any_at_32_channels_is_the_old_entry():
    rng = np.random.RandomState(3)
    A, B, d2, arg = _separated(rng, 130, 203, 32)
    tA, tB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    d_old, a_old = _call("gcl_nn_rowmin", tA, tB)
    d_new, a_new = _call("gcl_nn_rowmin_any", tA, tB)
    assert (a_new == a_old).all() and (a_new == arg).all()
    assert (np.abs(d_new.astype(np.float64) - d_old) <= (32 + 2) * EPS * d2).all()


@pytest.mark.parametrize("c", (16, 32, 64, 33))
def test_pdist_min_dispatch(c):
    """16 / 32 / 64 channels still run gcl_nn_rowmin (bitwise a direct call); every other width reaches the new entry."""
    from gcl_amd.lib.metrics import pdist_min
    rng = np.random.RandomState(c)
    A, B, d2, arg = _separated(rng, 67, 203, c)
    tA, tB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    with torch.cuda.device(DEV):
        dmin, got = pdist_min(tA, tB, "SquareL2")
    direct = _call("gcl_nn_rowmin" if c != 33 else "gcl_nn_rowmin_any", tA, tB)
    assert dmin.cpu().numpy().tobytes() == direct[0].tobytes() and got.cpu().numpy().tobytes() == direct[1].tobytes()
    assert (got.cpu().numpy() == arg).all()


def _run_stats(x, nan_pad=True, labels=False):
    from gcl_amd.scripts.SC2_PCR_bench import registration_stats
    src, tgt = x["src"].copy(), x["tgt"].copy()
    counts = x["counts"]
    if nan_pad:
        for b, n in enumerate(counts):
            src[b, n:], tgt[b, n:] = np.nan, np.nan                      # rows beyond a count are never read
    with torch.cuda.device(DEV):
        out = registration_stats(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), [int(n) for n in counts],
                                 torch.from_numpy(x["pred_trans"]).to(DEV), torch.from_numpy(x["gt_trans"]).to(DEV),
                                 float(x["inlier_threshold"]), float(x["re_thre"]), float(x["te_thre"]), return_labels=labels)
    return [o.cpu().numpy() for o in out] if labels else out.cpu().numpy()


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_registration_stats_on_the_goldens(path):
    x = np.load(path)
    got, pred_l, gt_l = _run_stats(x, labels=True)
    ref, f64, counts = x["stats_ref"], x["stats_f64"], x["counts"]
    print(np.array2string(got, precision=6, max_line_width=220))
    assert np.isfinite(got).all(), "a NaN row beyond a count was read"
    assert (got[:, [0, 3, 5]] == ref[:, [0, 3, 5]]).all(), "success and the two inlier counts are exact"
    for k, col in enumerate((1, 2, 9)):
        assert (np.abs(got[:, col] - f64[:, k]) <= 1e-9 * np.abs(f64[:, k])).all(), (col, got[:, col], f64[:, k])
        assert (np.abs(got[:, col] - ref[:, col]) <= 2 * np.abs(ref[:, col] - f64[:, k]) + 1e-9).all(), col
    assert np.abs(got[:, [4, 6, 7, 8]] - ref[:, [4, 6, 7, 8]]).max() <= 1e-6
    # the labels: 0 from a count on, their sums are the counts behind columns 3, 5 and 6
    thr = float(x["inlier_threshold"])
    for b, n in enumerate(counts):
        assert (pred_l[b, n:] == 0).all() and (gt_l[b, n:] == 0).all()
        assert gt_l[b].sum() == ref[b, 3] and (gt_l[b] * pred_l[b]).sum() == ref[b, 5]
        want = SO.distances(x["src"][b, :n], x["tgt"][b, :n], x["pred_trans"][b], np.float32) < np.float32(thr)
        assert (pred_l[b, :n] == want).all()
    # a pair alone (counts = None, its own extent) gives the row it has in the batch, bit for bit
    from gcl_amd.scripts.SC2_PCR_bench import registration_stats
    with torch.cuda.device(DEV):
        for b, n in enumerate(counts):
            one = registration_stats(torch.from_numpy(x["src"][b:b + 1, :n]).to(DEV), torch.from_numpy(x["tgt"][b:b + 1, :n]).to(DEV),
                                     None, torch.from_numpy(x["pred_trans"][b:b + 1]).to(DEV),
                                     torch.from_numpy(x["gt_trans"][b:b + 1]).to(DEV), thr, float(x["re_thre"]),
                                     float(x["te_thre"]))
            assert one.cpu().numpy().tobytes() == got[b:b + 1].tobytes(), b


def _rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _record(rng, n, m, share=0.3, c=33, half=1.5, noise=0.01):
    """A fragment pair: n source and m target keypoints with c-channel unit descriptors; round(share n) source keypoints
    have their moved copy (and a slightly perturbed copy of their descriptor) among the targets."""
    src = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-half, half, (m, 3)).astype(np.float32)
    fs, ft = rng.normal(size=(n, c)), rng.normal(size=(m, c))
    R, t = _rot(rng, rng.uniform(0.3, 1.2)), rng.uniform(-0.5, 0.5, 3)
    k = int(round(share * n))
    i, j = rng.permutation(n)[:k], rng.permutation(m)[:k]
    tgt[j] = (src[i].astype(np.float64) @ R.T + t + rng.uniform(-noise, noise, (k, 3))).astype(np.float32)
    ft[j] = fs[i] + 0.02 * rng.normal(size=(k, c))
    fs /= np.linalg.norm(fs, axis=1, keepdims=True)
    ft /= np.linalg.norm(ft, axis=1, keepdims=True)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    return src, tgt, fs.astype(np.float32), ft.astype(np.float32), T


CFG_3DMATCH = dict(inlier_threshold=0.1, num_node="all", use_mutual=False, d_thre=0.1, num_iterations=10, ratio=0.2,
                   nms_radius=0.1, max_points=8000, k1=30, k2=20)
EVAL_CFG = dict(inlier_threshold=0.1, re_thre=15.0, te_thre=30.0)


def _tables(records, batch_pairs=4):
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair
    with torch.cuda.device(DEV):
        one = eval_per_pair(records, Matcher(**CFG_3DMATCH), EVAL_CFG, scene_ind=3)
        batch = eval_per_pair(records, BatchMatcher(**CFG_3DMATCH), EVAL_CFG, batch_pairs=batch_pairs, scene_ind=3)
    return one, batch


def test_eval_per_pair_batched_equals_pair_by_pair():
    """Six ragged pairs, 33-channel descriptors, inlier share ~ 0.3, the fourth below k1 = 30 correspondences (it runs with
    (k1, k2) = (4, 4) in a chunk of its own).  Columns 9 and 10 are host times and are not compared."""
    rng = np.random.RandomState(11)
    sizes = [(300, 340), (557, 500), (900, 777), (28, 40), (431, 431), (640, 901)]
    records = [_record(rng, n, m) for n, m in sizes]
    one, batch = _tables(records)
    print(np.array2string(batch[:, :9], precision=4, suppress_small=True, max_line_width=200))
    cols = list(range(9)) + [11]
    assert one.shape == batch.shape == (6, 12) and one.dtype == np.float64
    assert one[:, cols].tobytes() == batch[:, cols].tobytes()
    assert (batch[:, 11] == 3).all() and (batch[:, 9:11] > 0).all()
    assert (batch[:, 0] == 1).all(), "every pair has planted correspondences and must register"
    assert (np.abs(batch[:, 4] - 0.3) < 0.05).all() and (batch[:, 6] > 0.9).all()


def test_eval_per_pair_scores_a_pair_without_a_seed_as_failed():
    """int(4 * 0.2) = 0 seeds: the pair is not registered (identity), it is scored, and nothing raises."""
    rng = np.random.RandomState(12)
    records = [_record(rng, 4, 6, share=0.5), _record(rng, 300, 300)]
    one, batch = _tables(records, batch_pairs=2)
    cols = list(range(9)) + [11]
    assert one[:, cols].tobytes() == batch[:, cols].tobytes() and np.isfinite(batch).all()
    T = records[0][4].astype(np.float64)
    re, te = SO.rotation_translation_error(np.eye(4), T)
    assert batch[0, 0] == 0 and abs(batch[0, 1] - re) <= 1e-9 * re and abs(batch[0, 2] - te) <= 1e-9 * te
    assert batch[1, 0] == 1
