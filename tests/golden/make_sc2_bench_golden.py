"""Generates tests/golden/sc2_bench_s{0,1,2}.npz by IMPORTING the reference's own scoring code (this container only).

Run:  python tests/golden/make_sc2_bench_golden.py        (needs /root/reference and sklearn; writes arrays only)

What is captured: for synthetic ragged batches of correspondence sets, a ground-truth and a "predicted" transformation per
pair, the statistics the reference's benchmark loops compute per pair (scripts/SC2_PCR/test_KITTI.py:46-69):

* ``utils.SE3.transform`` and the fp32 distance test for the ground-truth labels            test_KITTI.py:49-51
* the predicted labels, the same expression under the predicted transformation           SC2_PCR.py:406-408
* ``evaluate_metric.TransformationLoss`` (recall, RE, TE, RMSE), ``ClassificationLoss`` (sklearn precision / recall / F1)

``stats_ref`` [B, 10]: columns 0 - 8 of the reference's table and the RMSE, from fp32 tensors as the loops hold them.
``stats_f64`` [B, 3]: RE, TE and RMSE by the same expressions (evaluate_metric.py:45-50, written out in ``_f64`` because the
class accumulates into float32 tensors whatever its inputs are) in float64 from the stored fp32 inputs.

A pair is rejected and redrawn when a correspondence's distance under either transformation (fp32 or float64) lies within
1e-4 * inlier_threshold of the threshold, or RE or TE within 1e-3 relative of its threshold: no integer column and no success
flag of a kept case can flip from rounding.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/scripts/SC2_PCR"
HERE = os.path.dirname(os.path.abspath(__file__))

KITTI = dict(inlier_threshold=0.6, re_thre=5.0, te_thre=60.0, half=20.0, noise=0.2)          # config_KITTI.json
TDMATCH = dict(inlier_threshold=0.1, re_thre=15.0, te_thre=30.0, half=1.5, noise=0.03)      # config_3DMatch.json


def _rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _trans(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def _draw(rng, n, share, cfg, d_angle, d_shift):
    """One pair: n correspondences, a share of them planted under gt; pred = gt moved by d_angle (rad) and d_shift."""
    half = cfg["half"]
    src = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    R, t = _rot(rng, rng.uniform(0.2, 1.5)), rng.uniform(-half / 4, half / 4, 3)
    tgt = src.astype(np.float64) @ R.T + t + rng.uniform(-cfg["noise"], cfg["noise"], (n, 3))
    out = rng.permutation(n)[int(round(share * n)):]
    tgt[out] = rng.uniform(-half, half, (len(out), 3))
    d = rng.normal(size=3)
    pred = _trans(_rot(rng, d_angle) @ R, t + d_shift * d / np.linalg.norm(d))
    return src, tgt.astype(np.float32), pred, _trans(R, t)


def _score(ev, src, tgt, pred, gt, cfg, dtype):
    """The reference loop's step 3 and 4 for one pair, on tensors of ``dtype``."""
    transform, trans_eval, cls_eval = ev
    s, q = torch.from_numpy(src)[None].to(dtype), torch.from_numpy(tgt)[None].to(dtype)
    P, G = torch.from_numpy(pred)[None].to(dtype), torch.from_numpy(gt)[None].to(dtype)
    thr = cfg["inlier_threshold"]
    warped = s @ P[:, :3, :3].transpose(1, 2) + P[:, None, :3, 3]                              # SC2_PCR.py:406-408
    d_pred = torch.sum((warped - q) ** 2, dim=-1) ** 0.5
    pred_labels = (d_pred < thr).float()
    d_gt = torch.sum((transform(s, G) - q) ** 2, dim=-1) ** 0.5                                # test_KITTI.py:49-51
    gt_labels = (d_gt < thr).float()
    _, recall, Re, Te, rmse = trans_eval(P, G, s, q, pred_labels.to(dtype))
    cls = cls_eval(pred_labels, gt_labels)
    row = [float(recall / 100.0), float(Re), float(Te), int(torch.sum(gt_labels)), float(torch.mean(gt_labels.float())),
           int(torch.sum(gt_labels[pred_labels > 0])), float(cls["precision"]), float(cls["recall"]), float(cls["f1"]),
           float(rmse)]
    return np.array(row, dtype=np.float64), d_gt[0].double().numpy(), d_pred[0].double().numpy()


def _f64(src, tgt, pred, gt):
    """RE (deg), TE (cm), RMSE: evaluate_metric.py:45-50 on float64 copies of the fp32 inputs."""
    s, q = torch.from_numpy(src).double(), torch.from_numpy(tgt).double()
    P, G = torch.from_numpy(pred).double(), torch.from_numpy(gt).double()
    re = torch.acos(torch.clamp((torch.trace(P[:3, :3].T @ G[:3, :3]) - 1) / 2.0, min=-1, max=1)) * 180 / np.pi
    te = torch.sqrt(torch.sum((P[:3, 3] - G[:3, 3]) ** 2)) * 100
    rmse = torch.norm(s @ P[:3, :3].T + P[:3, 3] - q, dim=-1).mean()
    return np.array([float(re), float(te), float(rmse)])


def _kept(row32, row64, dists, cfg):
    thr = cfg["inlier_threshold"]
    if any((np.abs(d - thr) <= 1e-4 * thr).any() for d in dists):
        return False
    for row in (row32, row64):
        if abs(row[-3] - cfg["re_thre"]) <= 1e-3 * cfg["re_thre"] or abs(row[-2] - cfg["te_thre"]) <= 1e-3 * cfg["te_thre"]:
            return False
    return True


def make(ev, name, seed, cfg, pairs):
    """pairs: (n, inlier share, pred rotation offset in rad, pred translation offset in the data's unit) per pair."""
    rng = np.random.RandomState(seed)
    n_cap = max(p[0] for p in pairs)
    B = len(pairs)
    src, tgt = np.zeros((B, n_cap, 3), np.float32), np.zeros((B, n_cap, 3), np.float32)
    pred, gt = np.zeros((B, 4, 4), np.float32), np.zeros((B, 4, 4), np.float32)
    ref, f64, redraws = np.zeros((B, 10)), np.zeros((B, 3)), 0
    for b, (n, share, d_angle, d_shift) in enumerate(pairs):
        while True:
            s, q, P, G = _draw(rng, n, share, cfg, d_angle, d_shift)
            row32, dg32, dp32 = _score(ev, s, q, P, G, cfg, torch.float32)
            row64, dg64, dp64 = _score(ev, s, q, P, G, cfg, torch.float64)      # labels from float64 distances
            exact = _f64(s, q, P, G)
            if _kept(row32[[1, 2, 9]], exact, (dg32, dp32, dg64, dp64), cfg):
                break
            redraws += 1
        assert (row32[[0, 3, 5]] == row64[[0, 3, 5]]).all(), "a kept case must not depend on the precision"
        src[b, :n], tgt[b, :n], pred[b], gt[b], ref[b], f64[b] = s, q, P, G, row32, exact
    np.savez_compressed(os.path.join(HERE, name), src=src, tgt=tgt, counts=np.array([p[0] for p in pairs], np.int32),
                        pred_trans=pred, gt_trans=gt, stats_ref=ref, stats_f64=f64,
                        inlier_threshold=np.float64(cfg["inlier_threshold"]), re_thre=np.float64(cfg["re_thre"]),
                        te_thre=np.float64(cfg["te_thre"]))
    print(name, "redraws", redraws)
    print(np.array2string(ref, precision=4, suppress_small=True, max_line_width=200))
    return ref


def main():
    sys.path.insert(0, REF)
    from evaluate_metric import TransformationLoss, ClassificationLoss
    from utils.SE3 import transform
    ev = lambda cfg: (transform, TransformationLoss(re_thre=cfg["re_thre"], te_thre=cfg["te_thre"]), ClassificationLoss())
    deg = np.pi / 180
    # s0 (KITTI): counts 1, 257 and 700 in one batch; a good pair, a pair failed on TE, one on RE
    r0 = make(ev(KITTI), "sc2_bench_s0.npz", 0, KITTI,
              [(1, 1.0, 0.3 * deg, 0.05), (257, 0.4, 0.5 * deg, 0.1), (700, 0.25, 1.0 * deg, 0.9), (333, 0.5, 9.0 * deg, 0.1)])
    assert list(r0[:, 0]) == [1, 1, 0, 0]
    # s1 (3DMatch): no predicted inlier (the prediction is far off), no gt inlier (nothing planted), a good pair
    r1 = make(ev(TDMATCH), "sc2_bench_s1.npz", 1, TDMATCH,
              [(300, 0.3, 40 * deg, 2.5), (129, 0.0, 1.0 * deg, 0.01), (512, 0.3, 2.0 * deg, 0.02), (64, 0.1, 0.5 * deg, 0.005)])
    assert r1[0, 5] == 0 and (r1[0, 6:9] == 0).all() and r1[0, 0] == 0 and r1[0, 3] > 0, "no predicted inlier, failed"
    assert r1[1, 3] == 0 and (r1[1, 6:9] == 0).all(), "no gt inlier"
    assert r1[2, 0] == 1
    # s2 (3DMatch): counts on the edges of the 256-thread workgroup (256, 513), two correspondences, pairs close to (but a
    # guard band away from) the RE and TE thresholds on either side
    r2 = make(ev(TDMATCH), "sc2_bench_s2.npz", 2, TDMATCH,
              [(256, 0.6, 3.0 * deg, 0.03), (513, 0.2, 14.0 * deg, 0.05), (1000, 0.35, 1.5 * deg, 0.29), (2, 1.0, 1.0 * deg, 0.02),
               (900, 0.05, 16.0 * deg, 0.31)])
    assert list(r2[:, 0]) == [1, 1, 1, 1, 0]


if __name__ == "__main__":
    main()
