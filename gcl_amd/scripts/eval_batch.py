"""``eval_pairs`` of ``gcl_amd.scripts.test_kitti`` with ONE registration call per chunk of pairs.

``eval_pairs(model, pairs, matcher, ..., batch_registration=False)`` is that loop itself, untouched, unless
``batch_registration`` is true: then the ``batch_pairs`` pairs of a chunk, which already share one forward pass, are also
registered by one ``matcher.estimator`` call on [B, n_points, ...] tensors instead of one call per pair.  The per-pair loop
is bound by the enqueuing thread (a registration is ~100 dependent launches of a few microseconds); a matcher
that takes a batch (``gcl_amd.lib.ransac.FeatureRansac``: ``gcl_ransac_register_batch``; ``gcl_amd.scripts.SC2_PCR.BatchMatcher``:
``gcl_sc2_register_batch``) makes the launches of one registration for the whole chunk and returns the same transformations
bit for bit.

Everything else is the loop of ``test_kitti.eval_pairs`` and uses its pieces: the same forward passes
(``forward_clouds_stream``), the same host draws in the same per-pair order (``DeferredCorr``, ``random_sample`` twice, then
the matcher's seed where ``estimator`` would have drawn it), one pinned copy of a chunk's transformations, the host half of
a chunk while the next one runs, and the same meters and result dict.  The registrations run on the current stream
(``GCL_EVAL_STREAMS`` is not read here: there is one call per chunk to place).
"""
import time

import numpy as np
import torch

from gcl_amd.lib.eval import DeferredCorr, host_to_device
from gcl_amd.scripts import test_kitti as TK


def eval_pairs(model, pairs, matcher, device=None, batch_pairs=1, subsample_size=5000, n_points=5000, rte_thresh=2.0,
               rre_thresh=5.0, collect=False, batch_registration=False):
    """``test_kitti.eval_pairs`` (same arguments, same result dict); ``batch_registration=True``: one ``matcher.estimator``
    call per chunk.  A matcher whose estimator registers one pair per call (``Matcher``) is refused with a ``ValueError``
    before any GPU work."""
    if not batch_registration:
        return TK.eval_pairs(model, pairs, matcher, device=device, batch_pairs=batch_pairs, subsample_size=subsample_size,
                             n_points=n_points, rte_thresh=rte_thresh, rre_thresh=rre_thresh, collect=collect)
    if not (getattr(matcher, "accepts_batch", False) and hasattr(matcher, "draw_seed")):
        raise ValueError("batch_registration needs a matcher whose estimator takes a batch of pairs (FeatureRansac, "
                         f"BatchMatcher); {type(matcher).__name__} registers one pair per call")
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    model.eval()
    success_meter, rte_meter, rre_meter = TK.AverageMeter(), TK.AverageMeter(), TK.AverageMeter()
    out = dict(T_est=[], rte=[], rre=[], success=[], dists_nn=[], n_voxels=0)
    t_feat = t_reg = 0.0
    pairs = list(pairs)

    def finish(pending):
        """Host half of a chunk whose device work was enqueued one chunk ago (``test_kitti.eval_pairs``'s bookkeeping)."""
        chunk, corrs, T_host, ev = pending
        ev.synchronize()
        for j, d in enumerate(chunk):
            T_est, T_gth = T_host[j].clone(), d["T_gt"]
            if collect:
                xyz0_corr, xyz1_corr = corrs[j].resolve()
                out["dists_nn"].append(TK.evaluate_nn_dist(xyz0_corr, xyz1_corr, T_gth))
            rte, rre = TK.rotation_translation_error(T_est, T_gth)
            if rte < rte_thresh:
                rte_meter.update(rte)
            if not np.isnan(rre) and rre < np.pi / 180 * rre_thresh:
                rre_meter.update(rre * 180 / np.pi)
            ok = rte < rte_thresh and not np.isnan(rre) and rre < np.pi / 180 * rre_thresh
            success_meter.update(1 if ok else 0)
            out["T_est"].append(T_est)
            out["rte"].append(rte)
            out["rre"].append(rre)
            out["success"].append(bool(ok))

    chunks = [pairs[b0:b0 + max(1, batch_pairs)] for b0 in range(0, len(pairs), max(1, batch_pairs))]
    with torch.cuda.device(dev), torch.no_grad():
        pending = None
        main = torch.cuda.current_stream()
        feat_stream = TK.forward_clouds_stream(model, ([(d[f"sinput{k}_F"], d[f"sinput{k}_C"]) for d in chunk for k in (0, 1)]
                                                       for chunk in chunks), device=dev)
        for chunk in chunks:
            t0 = time.perf_counter()
            feats = next(feat_stream)
            t_feat += time.perf_counter() - t0
            corrs, held, seeds = [], [], []
            for j, d in enumerate(chunk):
                F0, F1 = feats[2 * j].detach(), feats[2 * j + 1].detach()
                out["n_voxels"] += len(F0) + len(F1)
                xyz0, xyz1 = d["pcd0"][0], d["pcd1"][0]
                # the draws of a pair in the per-pair loop's order: find_corr's rows, the two samples, the matcher's seed
                corrs.append(DeferredCorr(xyz0, xyz1, F0, F1, subsample_size=subsample_size))
                xyz0s, F0s = TK.random_sample(xyz0.numpy(), F0, n_points)
                xyz1s, F1s = TK.random_sample(xyz1.numpy(), F1, n_points)
                t0 = time.perf_counter()
                held.append((host_to_device(xyz0s, dev), host_to_device(xyz1s, dev), F0s, F1s))
                # a matcher whose draws depend on the two sizes (BatchMatcher: num_node rows of each) is handed them
                seeds.append(matcher.draw_seed(len(F0s), len(F1s)) if getattr(matcher, "draw_takes_sizes", False)
                             else matcher.draw_seed())
                t_reg += time.perf_counter() - t0
            t0 = time.perf_counter()
            T_est, _, _, _ = matcher.estimator(*(torch.stack([h[k] for h in held]) for k in range(4)), seeds=seeds)
            t_reg += time.perf_counter() - t0
            T_host = torch.empty((len(chunk), 4, 4), dtype=torch.float32, pin_memory=True)
            T_host.copy_(T_est, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(main)
            if pending is not None:
                finish(pending)
            pending = (chunk, corrs, T_host, ev)
        if pending is not None:
            finish(pending)
    out.update(rte_avg=rte_meter.avg, rte_var=rte_meter.var, rre_avg=rre_meter.avg, rre_var=rre_meter.var,
               success_rate=success_meter.avg, n_pairs=success_meter.count, feat_enqueue_time=t_feat, reg_enqueue_time=t_reg)
    return out
