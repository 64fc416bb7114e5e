"""The validation epoch on the GPU (csrc/valpose.hip, gcl_amd/lib/validation.py): the batched robust pose against the
reference-captured goldens and against the host fp64 function, its structure (bitwise independence of the batch and of the
run), degenerate input, the per-pair statistics against the numpy restatement, and the whole loop against the host
``_valid_epoch`` under one seed."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import transform_oracle as TO          # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNTS = [3, 4, 7, 63, 64, 65, 255, 256, 257, 1025, 5000]      # minimum; wave, block and strided-loop borders; the workload


def _dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _pose(pairs, weighted):
    """One ``gcl_irls_pose_batch`` call over ``pairs`` (dicts with src / tgt / weight): (T [B, 4, 4], status [B]) as numpy."""
    from gcl_amd.util.transform_estimation import est_quad_linear_robust_batch
    off = np.cumsum([0] + [len(p["src"]) for p in pairs])
    src = np.concatenate([p["src"].reshape(-1, 3) for p in pairs]).astype(np.float32)
    tgt = np.concatenate([p["tgt"].reshape(-1, 3) for p in pairs]).astype(np.float32)
    w = _dev(np.concatenate([p["weight"].reshape(-1) for p in pairs]).astype(np.float32)) if weighted else None
    with torch.cuda.device(DEV):
        T, status = est_quad_linear_robust_batch(_dev(src), _dev(tgt), _dev(off.astype(np.int64)), w)
        torch.cuda.synchronize()
    assert T.dtype == torch.float64 and T.shape == (len(pairs), 4, 4) and status.dtype == torch.int32
    return T.cpu().numpy(), status.cpu().numpy()


def _stats(src, tgt, off, xyz0, off0, T_est, T_gt, status=None, max_dist=1.0, thresh=0.3):
    from gcl_amd.lib.validation import val_stats_batch
    with torch.cuda.device(DEV):
        out = val_stats_batch(_dev(src, torch.float32), _dev(tgt, torch.float32), _dev(np.asarray(off, dtype=np.int64)),
                              _dev(xyz0, torch.float32), _dev(np.asarray(off0, dtype=np.int64)), _dev(T_est, torch.float64),
                              _dev(T_gt, torch.float64), None if status is None else _dev(status, torch.int32),
                              max_dist=max_dist, thresh=thresh)
        torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. goldens ------------------------------------------------------------------------------------------------------------
def test_goldens_as_one_ragged_batch():
    paths = sorted(glob.glob(os.path.join(G, "validation_s*.npz")))
    assert len(paths) == 3
    gold = [dict(np.load(p)) for p in paths]
    for weighted, key in [(False, "T_ref"), (True, "T_ref_weighted")]:
        T, status = _pose(gold, weighted)
        assert (status == 0).all()
        for d, t in zip(gold, T):
            err = np.abs(t - d[key].astype(np.float64)).max()
            print(f"golden {key}: max |T - ref| = {err:.3e}")
            assert err < 5e-6
    off = np.cumsum([0] + [len(d["src"]) for d in gold])
    src, tgt = np.concatenate([d["src"] for d in gold]), np.concatenate([d["tgt"] for d in gold])
    thr = {float(d["hit_thresh"]) for d in gold}
    assert len(thr) == 1
    out = _stats(src, tgt, off, src, off, np.stack([d["T_ref"] for d in gold]), np.stack([d["T_gt"] for d in gold]),
                 thresh=thr.pop())
    for d, row in zip(gold, out):
        print(f"golden stats: loss {row[0] - float(d['corr_dist']):+.3e}  hit_ratio {row[3] - float(d['hit_ratio']):+.3e}")
        assert abs(row[0] - float(d["corr_dist"])) < 1e-6 and abs(row[3] - float(d["hit_ratio"])) < 1e-6
        assert row[4] == len(d["src"]) and row[5] == 0


# ---- 2. / 3. against the host fp64 function; structure ------------------------------------------------------------------------
def _synthetic_pair(seed, n):
    """Extent +-40 m, rotation 0.03 rad about z plus (0.25, -0.1, 0.05), 30 % of the rows displaced by N(0, 5 m)."""
    rng = np.random.RandomState(seed)
    p = rng.uniform(-40.0, 40.0, (n, 3))
    c, s = np.cos(0.03), np.sin(0.03)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    q = p @ R.T + np.array([0.25, -0.1, 0.05])
    out = rng.uniform(size=n) < 0.3
    q[out] += rng.normal(0.0, 5.0, (int(out.sum()), 3))
    return {"src": p.astype(np.float32), "tgt": q.astype(np.float32), "weight": rng.uniform(0.2, 1.0, n).astype(np.float32)}


def _host64(pair, weighted):
    from gcl_amd.util.transform_estimation import est_quad_linear_robust
    w = torch.from_numpy(pair["weight"]).double() if weighted else None
    T = est_quad_linear_robust(torch.from_numpy(pair["src"]).double(), torch.from_numpy(pair["tgt"]).double(), w)
    assert T.dtype == torch.float64
    return T.numpy()


@pytest.fixture(scope="module")
def pool():
    """33 pairs (every count three times, other points each time) with the host fp64 result of each, computed once, and the
    device result of all 33 as ONE batch."""
    pairs = [_synthetic_pair(100 + k, COUNTS[k % len(COUNTS)]) for k in range(33)]
    ref = {w: [_host64(p, w) for p in pairs] for w in (False, True)}
    got = {w: _pose(pairs, w) for w in (False, True)}
    return pairs, ref, got


def _max_err(T, ref):
    return max(float(np.abs(t - r).max()) for t, r in zip(T, ref))


def test_float64_pose_agrees_with_the_host_function_run_in_double(pool):
    """Both sides are the same algorithm in fp64 and differ in summation order, the 6 x 6 solver and libm only; permuting
    the rows of these inputs moves the host result by <= 1.4e-14, so 1e-10 is four orders of slack.  Batches of 33, 3 and 1
    pairs of mixed sizes and one with a 0-row pair in the middle, with and without weights.
    Measured on an MI355X, maximum over all of them: 6.7e-14 (a 4-row pair with weights; 2.8e-14 at 3 rows, <= 7e-15 from
    63 rows on, 3.9e-15 at 5000) -- the few-row systems are the worst conditioned, the large ones sit at rounding level."""
    pairs, ref, got = pool
    empty = {"src": np.zeros((0, 3), np.float32), "tgt": np.zeros((0, 3), np.float32), "weight": np.zeros(0, np.float32)}
    worst = 0.0
    for w in (False, True):
        T, status = got[w]
        assert (status == 0).all()
        e33 = _max_err(T, ref[w])
        T3, s3 = _pose(pairs[8:11], w)                                    # 257, 1025, 5000 rows
        e3 = _max_err(T3, ref[w][8:11])
        T1, s1 = _pose(pairs[10:11], w)                                   # 5000 rows alone
        e1 = _max_err(T1, ref[w][10:11])
        Tz, sz = _pose([pairs[3], empty, pairs[9]], w)                    # a 0-row pair in the middle
        ez = _max_err(Tz[[0, 2]], [ref[w][3], ref[w][9]])
        per_count = {n: max(float(np.abs(T[k] - ref[w][k]).max()) for k in range(33) if COUNTS[k % 11] == n) for n in COUNTS}
        print(f"weights={w}: max |T - host fp64|  B=33 {e33:.3e}  B=3 {e3:.3e}  B=1 {e1:.3e}  with empty {ez:.3e}")
        print("  per count: " + "  ".join(f"{n}: {e:.1e}" for n, e in per_count.items()))
        assert (s3 == 0).all() and (s1 == 0).all() and list(sz) == [0, 1, 0]
        assert np.array_equal(Tz[1], np.eye(4))
        worst = max(worst, e33, e3, e1, ez)
    print(f"measured maximum: {worst:.3e}")
    assert worst < 1e-10


def test_a_pair_is_bitwise_the_same_alone_in_any_batch_and_on_every_run(pool):
    pairs, _, got = pool
    for w in (False, True):
        T, _ = got[w]
        again, _ = _pose(pairs, w)
        assert np.array_equal(T, again)                                   # two runs
        for k in range(len(COUNTS)):                                      # every count alone
            alone, st = _pose(pairs[k:k + 1], w)
            assert st[0] == 0 and np.array_equal(alone[0], T[k]), COUNTS[k]
        shuffled, _ = _pose(pairs[10:4:-1], w)                            # other neighbours, other order
        assert np.array_equal(shuffled, T[10:4:-1])


# ---- 4. degenerate input --------------------------------------------------------------------------------------------------------
def test_degenerate_pairs_are_flagged_not_faulted():
    from gcl_amd.util.transform_estimation import est_quad_linear_robust
    same = {"src": np.tile(np.float32([[2.0, 0.0, 0.0]]), (50, 1)), "tgt": np.tile(np.float32([[2.5, 0.1, 0.0]]), (50, 1)),
            "weight": np.ones(50, np.float32)}
    with pytest.raises(Exception):                                        # the host function raises on the singular system
        est_quad_linear_robust(torch.from_numpy(same["src"]), torch.from_numpy(same["tgt"]))
    generic = {"src": np.tile(np.float32([[1.3, 2.7, -0.4]]), (300, 1)), "tgt": np.tile(np.float32([[1.1, 2.9, -0.3]]), (300, 1)),
               "weight": np.ones(300, np.float32)}
    line = _synthetic_pair(7, 10)
    line["src"] = (np.linspace(-5, 5, 10)[:, None] * np.float32([[1.0, 2.0, -0.5]])).astype(np.float32)
    line["tgt"] = line["src"] + np.float32([0.1, 0.0, 0.0])
    good = _synthetic_pair(8, 100)
    T, status = _pose([same, good, generic, line], False)
    assert status[0] == 1 and np.array_equal(T[0], np.eye(4))
    assert status[2] == 1 and np.array_equal(T[2], np.eye(4))
    assert status[1] == 0 and np.abs(T[1] - _host64(good, False)).max() < 1e-10
    assert status[3] in (0, 1) and np.isfinite(T[3]).all()               # collinear rows: finite or flagged, nothing more
    if status[3] == 1:
        assert np.array_equal(T[3], np.eye(4))


# ---- 5. statistics ------------------------------------------------------------------------------------------------------------
def _rigid(rng, angle, shift):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    T[:3, 3] = rng.normal(size=3) * shift
    return T


def test_stats_against_the_numpy_restatement():
    from gcl_amd.lib.validation import meters_from_table
    rng = np.random.RandomState(5)
    thresh, max_dist = 0.3, 1.0
    n_corr, n_first = [1, 257, 300, 1000, 64], [700, 1, 513, 256, 90]
    src, tgt, first, Te, Tg = [], [], [], [], []
    for b, (n, n0) in enumerate(zip(n_corr, n_first)):
        gt = _rigid(rng, 0.2, 1.0).astype(np.float32).astype(np.float64)            # float32 values, as the loop passes them
        est = _rigid(rng, 0.01, 0.3) @ gt
        if b == 4:            # trace(R^T R) of a float32-rounded rotation: above 3 by rounding -> rre is NaN
            for k in range(1, 1000):
                cand = _rigid(np.random.RandomState(k), 0.1 * k, 1.0).astype(np.float32).astype(np.float64)
                if (cand[:3, :3] ** 2).sum() > 3.0 + 1e-8:
                    break
            gt = est = cand
        a = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
        d = rng.normal(size=(n, 3))
        d *= (rng.uniform(0.0, 2.0 * thresh, n) / np.linalg.norm(d, axis=1))[:, None]
        bpt = ((a.astype(np.float64) @ gt[:3, :3].T + gt[:3, 3]) + d).astype(np.float32)
        x = rng.uniform(-40, 40, (4 * n0, 3)).astype(np.float32)
        dist = np.linalg.norm((x @ est[:3, :3].T + est[:3, 3]) - (x @ gt[:3, :3].T + gt[:3, 3]), axis=1)
        x = x[np.abs(dist - max_dist) > 1e-3][:n0]                                   # no point near the clamp
        hd = np.sqrt((((a @ gt[:3, :3].T + gt[:3, 3]) - bpt) ** 2).sum(1) + 1e-6)
        bpt[np.abs(hd - thresh) < 1e-3] = (a @ gt[:3, :3].T + gt[:3, 3])[np.abs(hd - thresh) < 1e-3].astype(np.float32)
        assert len(x) == n0
        src.append(a), tgt.append(bpt), first.append(x), Te.append(est), Tg.append(gt)
    # the border condition, asserted on what is actually sent
    for a, bpt, x, est, gt in zip(src, tgt, first, Te, Tg):
        hd = np.sqrt((((a @ gt[:3, :3].T + gt[:3, 3]) - bpt) ** 2).sum(1) + 1e-6)
        dist = np.linalg.norm((x @ est[:3, :3].T + est[:3, 3]) - (x @ gt[:3, :3].T + gt[:3, 3]), axis=1)
        assert np.abs(hd - thresh).min() > 1e-4 and np.abs(dist - max_dist).min() > 1e-4
    off, off0 = np.cumsum([0] + n_corr), np.cumsum([0] + n_first)
    status = np.array([0, 0, 1, 0, 0], dtype=np.int32)
    out = _stats(np.concatenate(src), np.concatenate(tgt), off, np.concatenate(first), off0, np.stack(Te), np.stack(Tg),
                 status, max_dist, thresh)
    for b, (a, bpt, x, est, gt) in enumerate(zip(src, tgt, first, Te, Tg)):
        loss, hit = TO.corr_dist(est, gt, x, max_dist), TO.hit_ratio(a, bpt, gt, thresh)
        rte = float(np.linalg.norm(est[:3, 3] - gt[:3, 3]))
        with np.errstate(invalid="ignore"):
            rre = float(np.arccos((np.trace(est[:3, :3].T @ gt[:3, :3]) - 1) / 2))
        print(f"pair {b}: loss {out[b, 0] - loss:+.2e} rte {out[b, 1] - rte:+.2e} rre {out[b, 2] - rre:+.2e} hit {out[b, 3] - hit:+.2e}")
        assert round(out[b, 3] * len(a)) == round(hit * len(a)) and out[b, 4] == len(a) and out[b, 5] == status[b]
        assert abs(out[b, 0] - loss) < 1e-6 and abs(out[b, 3] - hit) < 1e-6 and abs(out[b, 1] - rte) < 1e-6
        if b == 4:
            assert np.isnan(rre) and np.isnan(out[b, 2])
        else:
            assert abs(out[b, 2] - rre) < 1e-6
    meters, n_deg = meters_from_table(out)
    keep = [0, 1, 3]                                                      # pair 2 is flagged, pair 4's rre is NaN
    assert n_deg == 1 and meters["n"] == 5
    assert abs(meters["rre"] - out[keep, 2].mean()) < 1e-15 and abs(meters["rte"] - out[keep + [4], 1].mean()) < 1e-15
    assert abs(meters["loss"] - out[keep + [4], 0].mean()) < 1e-15 and abs(meters["hit_ratio"] - out[:, 3].mean()) < 1e-15


# ---- 6. the loop ----------------------------------------------------------------------------------------------------------------
def _twin_pair(seed, shift_voxels=(8, 0, 0), voxel=0.3):
    """An eval pair whose second cloud is the first one moved by a multiple of 8 voxels (every U-Net level stays aligned):
    well-conditioned for an UNTRAINED network -- twin voxels get equal features, everything else is an outlier.  Input
    features carry a small per-voxel jitter so that no two voxels have tied features."""
    from gcl_amd import synthetic
    p = synthetic.make_eval_pair(seed, voxel_size=voxel, baseline=6.0, n_boxes=25)
    keep = torch.arange(0, len(p["sinput0_C"]), 3)                      # ~1/3 of the voxels: a few thousand rows
    C0 = p["sinput0_C"][keep].clone()
    xyz0 = p["pcd0"][0][keep].clone()
    sh = torch.tensor(shift_voxels, dtype=torch.int32)
    C1 = C0.clone()
    C1[:, 1:] += sh
    xyz1 = xyz0 + sh.float() * voxel
    F = 1.0 + 0.05 * torch.randn(len(C0), 1, generator=torch.Generator().manual_seed(seed))
    T = torch.eye(4)
    T[:3, 3] = sh.float() * voxel
    return {"pcd0": (xyz0,), "pcd1": (xyz1,), "sinput0_C": C0, "sinput1_C": C1, "sinput0_F": F, "sinput1_F": F.clone(),
            "T_gt": T}


def _small_motion_pairs():
    pairs = []
    for seed, ang, t in [(70, 0.03, (0.25, -0.1, 0.05)), (71, -0.05, (-0.2, 0.15, 0.0))]:
        d = _twin_pair(seed, (0, 0, 0))
        c, s_ = np.cos(ang), np.sin(ang)
        T = torch.eye(4)
        T[:3, :3] = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
        T[:3, 3] = torch.tensor(t)
        d["pcd1"] = (d["pcd0"][0] @ T[:3, :3].t() + T[:3, 3],)
        d["T_gt"] = T
        pairs.append(d)
    return pairs


def test_valid_epoch_on_device_equals_the_host_path_under_one_seed():
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    from gcl_amd.lib.trainer import ContrastiveLossTrainer
    from gcl_amd.scripts.test_kitti import forward_clouds
    torch.manual_seed(5)
    thresh = 0.3
    tr = FinestContrastiveLossTrainer(make_config(hit_ratio_thresh=thresh), device=DEV)
    pairs = _small_motion_pairs()
    np.random.seed(21)
    host = tr._valid_epoch(pairs, on_device=False)
    np.random.seed(21)
    dev1 = tr._valid_epoch(pairs, on_device=True, batch_pairs=1)
    np.random.seed(21)
    dev2 = tr._valid_epoch(pairs, on_device=True, batch_pairs=2)
    # the border condition of the statistics test, on the correspondences the loop saw (same seed, same calls)
    np.random.seed(21)
    with torch.no_grad(), torch.cuda.device(DEV):
        for d in pairs:
            F0, F1 = forward_clouds(tr.model, [(d["sinput0_F"].to(DEV), d["sinput0_C"].to(DEV).int()),
                                               (d["sinput1_F"].to(DEV), d["sinput1_C"].to(DEV).int())])
            a, b = tr.find_corr(d["pcd0"][0], d["pcd1"][0], F0, F1, subsample_size=5000)
            Tg = d["T_gt"].double().numpy()
            hd = np.sqrt((((a.double().numpy() @ Tg[:3, :3].T + Tg[:3, 3]) - b.double().numpy()) ** 2).sum(1) + 1e-6)
            assert np.abs(hd - thresh).min() > 1e-4
    print("host    ", host)
    print("device 1", dev1)
    print("device 2", dev2)
    assert host["n"] == dev1["n"] == dev2["n"] == 2
    assert dev1 == dev2                                                   # batch_pairs 1 and 2: bitwise
    assert dev1["hit_ratio"] == host["hit_ratio"] and dev1["feat_match_ratio"] == host["feat_match_ratio"]
    for k in ("loss", "rte", "rre"):
        assert abs(dev1[k] - host[k]) < 5e-6, k
    assert host["hit_ratio"] > 0.9                                        # the pairs are the well-conditioned ones
    torch.manual_seed(6)
    ct = ContrastiveLossTrainer(make_config(hit_ratio_thresh=thresh), device=DEV)
    np.random.seed(21)
    out = ct._valid_epoch(pairs, batch_pairs=2)
    assert out["n"] == 2 and not ct.model.training
    assert all(np.isfinite(out[k]) for k in ("loss", "rre", "rte", "feat_match_ratio", "hit_ratio"))
