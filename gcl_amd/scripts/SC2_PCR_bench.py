"""The SC2-PCR registration benchmark loops on the MI355X kernels (scripts/SC2_PCR/test_KITTI.py, test_3DMatch.py,
test_3DLoMatch.py of the reference: ``eval_KITTI_per_pair`` / ``eval_3DMatch_scene`` / ``eval_3DLoMatch_scene`` and the
summaries of ``eval_KITTI`` / ``eval_3DMatch``), on arrays -- the dataset file readers are out of scope, as is ICP refinement
(``use_icp``), ``benchmark_predator`` and the scripts' ``RANSAC`` solver switch.

``eval_per_pair(records, matcher, config)`` fills the reference's [num_pair, 12] table:

    0 success  1 RE (deg)  2 TE (cm)  3 input inlier number  4 input inlier ratio  5 output inlier number
    6 output inlier precision  7 recall  8 F1  9 model time  10 data time  11 scene index

Where the reference scores a pair with ~25 small torch operations and three sklearn calls on host copies (a device-to-host
synchronisation per pair), a chunk of pairs is

* matched per pair (``Matcher.match_pair`` -> ``lib.metrics.pdist_min``, any descriptor width up to 128) into buffers padded
  to the chunk's largest count,
* registered by ONE ``BatchMatcher.SC2_PCR(src, tgt, counts=...)`` call (``gcl_sc2_register_batch``),
* scored by ONE ``gcl_registration_stats`` launch,

and one pinned [B, 10] copy comes back per chunk, read a chunk late (the host half of a chunk runs while the next one is on
the device, as ``scripts/eval_batch.eval_pairs`` does).  With a plain ``Matcher``, or ``batch_pairs=1``, the loop runs pair by
pair through the same statistics kernel; columns 0 - 8 are then bit for bit those of the batched run (a pair's registration
and its statistics do not depend on what shares its batch).  Columns 9 and 10 are host times: a chunk's registration call is
shared evenly among its pairs.

``records[i]`` is ``(src_keypts [N, 3], tgt_keypts [M, 3], src_features [N, C], tgt_features [M, C], gt_trans [4, 4])`` as
numpy arrays or torch tensors, with per-pair sizes (``num_node = 'all'`` of config_3DMatch.json: ragged pairs).  The host
draws of an integer ``num_node`` are made inside ``match_pair`` in pair order, as the reference loop makes them.

A PAIR WITHOUT A SEED (``int(n * ratio) < 1`` correspondences: the reference's ``Matcher`` has no defined outcome there, its
argmax over an empty seed set raises) is not registered: its transformation is the IDENTITY -- what a failed registration
returns in the reference's other back-end (open3d's RANSAC) -- and it is scored like any other pair, so the loop never
raises mid-benchmark.
"""
import time

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device

STAT_COLUMNS = ("success", "re", "te", "input_inlier_num", "input_inlier_ratio", "output_inlier_num", "precision", "recall",
                "f1", "model_time", "data_time", "scene_ind")


def registration_stats(src_corr, tgt_corr, counts, pred_trans, gt_trans, inlier_threshold, re_thre, te_thre,
                       return_labels=False):
    """``gcl_registration_stats``: the [B, 10] float64 table (columns 0 - 8 above, then TransformationLoss's RMSE) of B pairs
    in one launch, left on the device.  ``src_corr`` / ``tgt_corr`` float32 [B, n_cap, 3]; ``counts``: None (n_cap for every
    pair), a device int32 [B] tensor, or a host sequence of B ints (sent through a pinned block); ``pred_trans`` / ``gt_trans``
    [B, 4, 4].  ``return_labels``: also the predicted and the ground-truth labels, float32 [B, n_cap], 0 from a count on."""
    lib = _lib.require_gpu()
    src, tgt = src_corr.to(torch.float32).contiguous(), tgt_corr.to(torch.float32).contiguous()
    if src.dim() != 3 or src.shape[2] != 3 or tgt.shape != src.shape:
        raise ValueError(f"registration_stats takes two [B, n_cap, 3] tensors, got {tuple(src.shape)} and {tuple(tgt.shape)}")
    B, n_cap, dev = src.shape[0], src.shape[1], src.device
    pred = pred_trans.to(torch.float32).reshape(-1, 16).contiguous()
    gt = gt_trans.to(device=dev, dtype=torch.float32).reshape(-1, 16).contiguous()
    if pred.shape[0] != B or gt.shape[0] != B:
        raise ValueError(f"{B} pairs but {pred.shape[0]} predicted and {gt.shape[0]} ground-truth transformations")
    if counts is not None and not torch.is_tensor(counts):
        counts = host_to_device(np.asarray(counts, dtype=np.int32), dev)
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != B):
        raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
    stats = torch.empty((B, 10), dtype=torch.float64, device=dev)
    labels = torch.empty((2, B, n_cap), dtype=torch.float32, device=dev) if return_labels else None
    _lib.check(lib.gcl_registration_stats(_lib.ptr(src), _lib.ptr(tgt), B, n_cap, _lib.ptr(counts), _lib.ptr(pred),
                                          _lib.ptr(gt), float(inlier_threshold), float(re_thre), float(te_thre),
                                          _lib.ptr(stats), _lib.ptr(labels[0]) if return_labels else None,
                                          _lib.ptr(labels[1]) if return_labels else None, _lib.stream()),
               "gcl_registration_stats")
    return (stats, labels[0], labels[1]) if return_labels else stats


def form_chunks(counts, batch_pairs, k1, ratio, max_points):
    """Consecutive chunks ``[(kind, [pair indices]), ...]`` of at most ``batch_pairs`` pairs that one
    ``BatchMatcher.SC2_PCR`` call accepts (``BatchMatcher.plan``): a chunk never mixes pairs below ``k1`` correspondences
    (after the ``max_points`` cut; they run with (k1, k2) = (4, 4), kind ``'small'``) with pairs at or above it (kind
    ``'full'``), and a pair without a seed (``int(n * ratio) < 1``) is a chunk of its own of kind ``'fail'``, which is not
    registered.  The pairs keep their order.  Pure host arithmetic."""
    chunks = []
    for i, n in enumerate(counts):
        n = min(int(n), int(max_points))
        kind = "fail" if int(n * ratio) < 1 else ("small" if k1 > n else "full")
        if chunks and kind != "fail" and chunks[-1][0] == kind and len(chunks[-1][1]) < max(1, int(batch_pairs)):
            chunks[-1][1].append(i)
        else:
            chunks.append((kind, [i]))
    return chunks


def _get(config, name):
    return config[name] if isinstance(config, dict) else getattr(config, name)


def _dev(x, dev, dtype=torch.float32):
    if torch.is_tensor(x):
        return x.to(device=dev, dtype=dtype) if x.is_cuda else host_to_device(x.to(dtype).contiguous(), dev)
    return host_to_device(np.ascontiguousarray(x, dtype=np.float32), dev)


def eval_per_pair(records, matcher, config, batch_pairs=8, scene_ind=-1, device=None):
    """The loop of ``eval_KITTI_per_pair`` (``scene_ind=-1``) / ``eval_3DMatch_scene`` / ``eval_3DLoMatch_scene`` over
    ``records`` (see the module docstring); ``config`` gives ``inlier_threshold``, ``re_thre`` and ``te_thre`` (a dict or an
    object with these attributes).  Returns the [num_pair, 12] float64 table."""
    _lib.require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    thr, re_thre, te_thre = (float(_get(config, k)) for k in ("inlier_threshold", "re_thre", "te_thre"))
    num_pair = len(records)
    stats = np.zeros([num_pair, 12])
    stats[:, 11] = scene_ind
    batched = bool(getattr(matcher, "accepts_batch", False)) and int(batch_pairs) > 1

    def n_corr(rec):
        return int(rec[2].shape[0]) if matcher.num_node == "all" else int(matcher.num_node)

    counts = [n_corr(records[i]) for i in range(num_pair)] if batched else None
    chunks = (form_chunks(counts, batch_pairs, matcher.k1, matcher.ratio, matcher.max_points) if batched
              else [(None, [i]) for i in range(num_pair)])
    eye = np.eye(4, dtype=np.float32)

    def finish(pending):
        idx, host, ev = pending
        ev.synchronize()
        stats[idx, :9] = host.numpy()[:, :9]

    with torch.cuda.device(dev), torch.no_grad():
        main, pending = torch.cuda.current_stream(), None
        for kind, idx in chunks:
            B = len(idx)
            t_data, t_model, held, gts = [], [], [], np.empty((B, 4, 4), dtype=np.float32)
            one_call = kind is not None and kind != "fail" and B > 1                # the chunk's matching as one native call
            for j, i in enumerate(idx):
                t0 = time.perf_counter()
                sk, tk, sf, tf, gt = records[i]
                sk, tk, sf, tf = (_dev(x, dev)[None] for x in (sk, tk, sf, tf))
                gts[j] = gt.detach().cpu().numpy().reshape(4, 4) if torch.is_tensor(gt) else np.asarray(gt).reshape(4, 4)
                t1 = time.perf_counter()
                held.append((sk, tk, sf, tf) if one_call else matcher.match_pair(sk, tk, sf, tf))      # draws in pair order
                t_data.append(t1 - t0)
                t_model.append(time.perf_counter() - t1)
            t0 = time.perf_counter()
            if one_call:
                src, tgt, n = matcher.match_pairs(held)                             # rows from a count on are never read
                pred = matcher.SC2_PCR(src, tgt, counts=n)
                cnt = None if min(n) == max(n) else n
            elif kind is None or kind == "fail":                                    # one pair, its own extent
                n = [held[0][0].shape[1]]
                src, tgt, cnt = held[0][0].to(torch.float32), held[0][1].to(torch.float32), None
                if kind is None and int(min(n[0], matcher.max_points) * matcher.ratio) >= 1:
                    pred = matcher.SC2_PCR(src, tgt).reshape(1, 4, 4)
                else:
                    pred = host_to_device(eye[None].copy(), dev)                    # no seed: identity (module docstring)
            else:                                                                   # a chunk of one pair
                n = [held[0][0].shape[1]]
                src, tgt = held[0][0].to(torch.float32).contiguous(), held[0][1].to(torch.float32).contiguous()
                pred = matcher.SC2_PCR(src, tgt, counts=n)
                cnt = None
            dt = (time.perf_counter() - t0) / B
            st = registration_stats(src, tgt, cnt, pred, host_to_device(gts, dev), thr, re_thre, te_thre)
            host = torch.empty((B, 10), dtype=torch.float64, pin_memory=True)
            host.copy_(st, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(main)
            for j, i in enumerate(idx):
                stats[i, 9], stats[i, 10] = t_model[j] + dt, t_data[j]
            if pending is not None:
                finish(pending)
            pending = (idx, host, ev)
        if pending is not None:
            finish(pending)
    return stats


def summarize_pairs(stats):
    """The all-pair figures of ``eval_KITTI`` (test_KITTI.py:110-118; the same block closes ``eval_3DMatch``): column means
    over all pairs, RE and TE over the successful pairs only (NaN when there is none)."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 12)
    average = stats.mean(0) if len(stats) else np.full(12, np.nan)
    ok = stats[stats[:, 0] == 1]
    correct = ok.mean(0) if len(ok) else np.full(12, np.nan)
    out = dict(zip(STAT_COLUMNS, (float(v) for v in average)))
    del out["scene_ind"]
    out.update(n_pairs=int(stats.shape[0]), success_rate=out.pop("success"), re=float(correct[1]), te=float(correct[2]))
    return out


def summarize_scenes(all_stats):
    """The per-scene rows and their mean of ``eval_3DMatch`` (test_3DMatch.py:119-143) from ``{scene: [n, 12] table}``:
    ``scene_vals`` [S, 12] (a scene's column means, RE and TE over its successful pairs only), ``average`` [12] (mean over
    scenes), ``allpair`` (``summarize_pairs`` of all pairs) and ``all_stats`` (the tables concatenated in scene order)."""
    scenes = list(all_stats)
    scene_vals = np.zeros([len(scenes), 12])
    for k, scene in enumerate(scenes):
        st = np.asarray(all_stats[scene], dtype=np.float64).reshape(-1, 12)
        ok = st[st[:, 0] == 1]
        scene_vals[k] = st.mean(0) if len(st) else np.nan
        scene_vals[k, 1:3] = ok.mean(0)[1:3] if len(ok) else np.nan
    cat = (np.concatenate([np.asarray(all_stats[s], dtype=np.float64).reshape(-1, 12) for s in scenes], axis=0) if scenes
           else np.zeros([0, 12]))
    return dict(scenes=scenes, scene_vals=scene_vals, average=scene_vals.mean(0) if scenes else np.full(12, np.nan),
                allpair=summarize_pairs(cat), all_stats=cat)
