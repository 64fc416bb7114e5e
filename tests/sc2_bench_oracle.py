"""numpy restatement of the per-pair statistics of the SC2-PCR benchmark loops (scripts/SC2_PCR/test_KITTI.py:46-69,
evaluate_metric.py), kept in the test tree: what ``gcl_registration_stats`` has to reproduce.

Labels follow the reference's arithmetic (fp32 distances ``sum(d^2) ** 0.5`` against the threshold); RE, TE and the RMSE are
evaluated in float64 from the fp32 inputs; precision / recall / F1 are sklearn's binary definitions with zero division -> 0.
"""
import numpy as np


def distances(src, tgt, trans, dtype):
    """|R p + t - q| per correspondence, every operation in ``dtype``."""
    T = np.asarray(trans).reshape(4, 4).astype(dtype)
    w = np.asarray(src, dtype=dtype) @ T[:3, :3].T + T[:3, 3]
    d = w - np.asarray(tgt, dtype=dtype)
    return np.sum(d * d, axis=-1) ** dtype(0.5)


def rotation_translation_error(pred, gt):
    """(RE in degrees, TE in centimetres) in float64."""
    P, G = np.asarray(pred, dtype=np.float64).reshape(4, 4), np.asarray(gt, dtype=np.float64).reshape(4, 4)
    re = np.arccos(np.clip((np.trace(P[:3, :3].T @ G[:3, :3]) - 1) / 2.0, -1, 1)) * 180 / np.pi
    te = 100 * np.sqrt(np.sum((P[:3, 3] - G[:3, 3]) ** 2))
    return float(re), float(te)


def pair_stats(src, tgt, pred, gt, inlier_threshold, re_thre, te_thre):
    """The 10 statistics of one pair (columns 0 - 8 of the reference's table, then TransformationLoss's RMSE)."""
    n = len(src)
    thr = np.float32(inlier_threshold)
    gt_l = distances(src, tgt, gt, np.float32) < thr
    pr_l = distances(src, tgt, pred, np.float32) < thr
    n_gt, n_pr, both = int(gt_l.sum()), int(pr_l.sum()), int((gt_l & pr_l).sum())
    re, te = rotation_translation_error(pred, gt)
    return np.array([float(re < re_thre and te < te_thre), re, te, n_gt, n_gt / n if n else 0.0, both,
                     both / n_pr if n_pr else 0.0, both / n_gt if n_gt else 0.0,
                     2 * both / (n_pr + n_gt) if n_pr + n_gt else 0.0,
                     float(distances(src, tgt, pred, np.float64).mean()) if n else 0.0], dtype=np.float64)


def batch_stats(src, tgt, counts, pred, gt, inlier_threshold, re_thre, te_thre):
    return np.stack([pair_stats(src[b, :n], tgt[b, :n], pred[b], gt[b], inlier_threshold, re_thre, te_thre)
                     for b, n in enumerate(counts)])
