"""The validation epoch on the device (``_valid_epoch``, lib/colocation_trainer.py:306-379 and lib/trainer.py of the
reference): the arithmetic that ``FinestContrastiveLossTrainer._valid_epoch`` does on the host once per pair --
``find_corr``'s index read-back, ``est_quad_linear_robust``, ``corr_dist``, RTE, RRE, the hit ratio -- for a chunk of pairs
in one pose launch and one statistics launch (csrc/valpose.hip), read back one chunk late.  The random draws are the
reference's, in its order, so one seed gives both paths the same subsamples."""
import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device
from gcl_amd.lib.metrics import pdist_min, pdist_min_batch

STAT_COLUMNS = ("loss", "rte", "rre", "hit_ratio", "n_corr", "status")


def form_chunks(val_batches, val_max_iter=-1, batch_pairs=8):
    """Lists of at most ``batch_pairs`` consecutive pairs of ``val_batches`` (any iterable; read lazily), stopping after
    ``val_max_iter`` pairs when that is positive -- the reference's ``if 0 < val_max_iter <= num_data: break``."""
    batch_pairs = int(batch_pairs)
    if batch_pairs < 1:
        raise ValueError(f"batch_pairs = {batch_pairs}: a chunk holds at least one pair")
    chunk, taken = [], 0
    for pair in val_batches:
        if 0 < val_max_iter <= taken:
            break
        chunk.append(pair)
        taken += 1
        if len(chunk) == batch_pairs:
            yield chunk
            chunk = []
    if chunk:
        yield chunk


def draw_subsample(n0, n1, subsample_size):
    """``find_corr``'s two draws (lib/colocation_trainer.py:385-388), cloud 0 first; ``(None, None)`` when nothing is drawn."""
    if not (subsample_size > 0 and n0 > subsample_size):
        return None, None
    inds0 = np.random.choice(n0, min(n0, subsample_size), replace=False)
    inds1 = np.random.choice(n1, min(n1, subsample_size), replace=False)
    return inds0, inds1


def val_stats_batch(src, tgt, offsets, xyz0, offsets0, T_est, T_gt, status=None, max_dist=1.0, thresh=0.3):
    """``gcl_val_stats_batch``: device float64 [B, 6] (``STAT_COLUMNS``) of B pairs in one launch.  ``src`` / ``tgt`` float32
    [total, 3] with int64 ``offsets`` [B + 1]: the correspondences (hit ratio); ``xyz0`` float32 [total0, 3] with
    ``offsets0``: the first clouds (loss); ``T_est`` / ``T_gt`` float64 [B, 4, 4]; ``status`` int32 [B] is copied through."""
    lib = _lib.require_gpu()
    B = offsets.numel() - 1
    out = torch.empty((B, 6), dtype=torch.float64, device=src.device)
    _lib.check(lib.gcl_val_stats_batch(_lib.ptr(src, torch.float32), _lib.ptr(tgt, torch.float32), src.shape[0],
                                       _lib.ptr(offsets, torch.int64), _lib.ptr(xyz0, torch.float32), xyz0.shape[0],
                                       _lib.ptr(offsets0, torch.int64), B, _lib.ptr(T_est, torch.float64),
                                       _lib.ptr(T_gt, torch.float64), _lib.ptr(status, torch.int32), float(max_dist),
                                       float(thresh), _lib.ptr(out), _lib.stream()), "gcl_val_stats_batch")
    return out


def meters_from_table(table):
    """The reference's meters (lib/colocation_trainer.py:343-379) from the per-pair table: every pair enters hit_ratio and
    feat_match_ratio; loss and rte skip the pairs with status 1, rre those and a NaN (the reference's ``if not np.isnan``).
    Returns ``(dict, n_degenerate)``."""
    from gcl_amd.scripts.test_kitti import AverageMeter
    hit_ratio_meter, feat_match_ratio, loss_meter, rte_meter, rre_meter = (AverageMeter() for _ in range(5))
    n_degenerate = 0
    for loss, rte, rre, hit, _, status in np.asarray(table, dtype=np.float64).reshape(-1, 6):
        if status != 0:
            n_degenerate += 1
        else:
            loss_meter.update(float(loss))
            rte_meter.update(float(rte))
            if not np.isnan(rre):
                rre_meter.update(float(rre))
        hit_ratio_meter.update(float(hit))
        feat_match_ratio.update(float(hit > 0.05))
    meters = {"loss": loss_meter.avg, "rre": rre_meter.avg, "rte": rte_meter.avg, "feat_match_ratio": feat_match_ratio.avg,
              "hit_ratio": hit_ratio_meter.avg, "n": len(table)}
    return meters, n_degenerate


def _f32(x):
    return torch.as_tensor(x).detach().to(torch.float32).contiguous()


def validate_pairs(model, val_batches, val_max_iter=-1, batch_pairs=8, subsample_size=5000, hit_ratio_thresh=0.3,
                   nn_max_n=500):
    """The validation loop over ``val_batches`` (pair dicts of ``collate_debug_pair_fn``: sinput{0,1}_C / _F, pcd0 / pcd1,
    T_gt), ``batch_pairs`` pairs at a time: one forward pass for the chunk's clouds, per pair the two draws (in the
    reference's order), the chunk's feature 1-NN searches as ONE call that writes the correspondences at their offsets (a
    chunk of one pair: ``pdist_min`` and the gathers), then ONE pose call and ONE statistics call for the chunk and one
    pinned [B, 6] copy, which is read while the next chunk runs.  ``nn_max_n`` is the reference's chunk size against a
    temporary that does not exist here.

    Returns ``(meters, table, n_degenerate)``: the reference's dict (loss, rre, rte, feat_match_ratio, hit_ratio, n), the
    float64 [n, 6] per-pair table (``STAT_COLUMNS``) and the number of pairs with status 1 -- a singular system, where the
    host estimator raises; they stay out of the loss / rte / rre meters.  A NaN rre is skipped as the reference skips it."""
    from gcl_amd.scripts.test_kitti import forward_clouds
    from gcl_amd.util.transform_estimation import est_quad_linear_robust_batch
    _lib.require_gpu()
    dev = next(model.parameters()).device
    model.eval()
    rows = []

    def finish(pending):
        host, ev = pending
        ev.synchronize()
        rows.append(host.numpy().copy())

    with torch.no_grad(), torch.cuda.device(dev):
        main, pending = torch.cuda.current_stream(), None
        for chunk in form_chunks(val_batches, val_max_iter, batch_pairs):
            B = len(chunk)
            feats = forward_clouds(model, [(host_to_device(d[f"sinput{k}_F"], dev), host_to_device(d[f"sinput{k}_C"], dev).int())
                                           for d in chunk for k in (0, 1)])
            src, tgt, first, off, off0 = [], [], [], [0], [0]
            gts = np.empty((B, 16), dtype=np.float64)
            searches = []                                                          # B > 1: the chunk's searches, one call below
            for j, d in enumerate(chunk):
                F0, F1 = feats[2 * j], feats[2 * j + 1]
                xyz0, xyz1 = host_to_device(_f32(d["pcd0"][0]), dev), host_to_device(_f32(d["pcd1"][0]), dev)
                gts[j] = _f32(d["T_gt"]).reshape(16).double().cpu().numpy()          # the reference's T_gt is float32
                inds0, inds1 = draw_subsample(len(F0), len(F1), subsample_size)
                i0, i1 = (None, None) if inds0 is None else (host_to_device(inds0, dev), host_to_device(inds1, dev))
                if B > 1:
                    searches.append((F0, F1, i0, i1, xyz0, xyz1))
                    n = len(F0) if i0 is None else len(i0)
                else:
                    if i0 is None:
                        _, arg = pdist_min(F0, F1, "SquareL2")
                        a, b = xyz0, xyz1[arg.long()]
                    else:
                        _, arg = pdist_min(F0[i0], F1[i1], "SquareL2")
                        a, b = xyz0[i0], xyz1[i1[arg.long()]]
                    src.append(a)
                    tgt.append(b)
                    n = len(a)
                first.append(xyz0)
                off.append(off[-1] + n)
                off0.append(off0[-1] + len(xyz0))
            if B > 1:                         # the searches write their correspondences at the offsets `off` themselves
                src = torch.empty((off[-1], 3), dtype=torch.float32, device=dev)
                tgt = torch.empty_like(src)
                pdist_min_batch([s + (src[off[j]:off[j + 1]], tgt[off[j]:off[j + 1]]) for j, s in enumerate(searches)], "SquareL2")
                first = torch.cat(first)
            else:
                src, tgt, first = src[0], tgt[0], first[0]
            off_d = host_to_device(np.asarray(off, dtype=np.int64), dev)
            off0_d = host_to_device(np.asarray(off0, dtype=np.int64), dev)
            T_est, status = est_quad_linear_robust_batch(src, tgt, off_d)
            st = val_stats_batch(src, tgt, off_d, first, off0_d, T_est, host_to_device(gts, dev).reshape(B, 4, 4), status,
                                 max_dist=1.0, thresh=hit_ratio_thresh)
            host = torch.empty((B, 6), dtype=torch.float64, pin_memory=True)
            host.copy_(st, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(main)
            if pending is not None:
                finish(pending)
            pending = (host, ev)
        if pending is not None:
            finish(pending)
    table = np.concatenate(rows, axis=0) if rows else np.zeros((0, 6))
    meters, n_degenerate = meters_from_table(table)
    return meters, table, n_degenerate
