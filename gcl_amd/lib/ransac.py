"""Feature-matching RANSAC registration on the MI355X kernels: open3d's
``registration_ransac_based_on_feature_matching`` as the reference calls it (scripts/test_kitti.py:171-178 -- the default
registration of the KITTI loop -- and generalization_ETH/evaluate.py:171-186).

Putative correspondences are every source row paired with its feature-nearest target row (``pdist_min`` ->
``gcl_nn_rowmin``, open3d's ``mutual_filter=False`` path); the registration is ONE C-ABI call (include/gcl_amd.h,
``gcl_ransac_register``: draw, edge-length checker, fp64 Kabsch, distance checker, inlier scoring, winner and the confidence
stop, all on the device).  Minimal samples come from a counter generator keyed by ``seed`` in place of open3d's
``std::mt19937``: a seeded run is reproducible bit for bit.  Nothing leaves the device until the caller reads the result.

A BATCH of pairs goes through ``ransac_correspondences_batch`` (``gcl_ransac_register_batch``: the launches of one pair,
every pair's correspondence count read on the device), and open3d's ``mutual_filter=True`` through
``registration_ransac_based_on_mutual_feature_matching``: two ``pdist_min`` calls, ``gcl_mutual_correspondences`` (the mutual
pairs as point rows, or open3d's fall-back to all of them, with the count left on the device) and a registration on that
count.

``FeatureRansac`` speaks ``Matcher.estimator``'s calling convention (scripts/SC2_PCR.py), so
``eval_pairs(model, pairs, FeatureRansac.kitti(voxel_size))`` and ``evaluate_scene(..., matcher=FeatureRansac.eth())`` run
the reference's two RANSAC configurations through the loops that already exist.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.metrics import mutual_jobs, pdist_min, pdist_min_batch


class RegistrationResult:
    """Device tensors of one registration: ``transformation`` [4, 4], ``fitness`` and ``inlier_rmse`` (0-d views),
    ``info`` int32 [4] = (winning hypothesis or -1, its inlier count, hypotheses covered, hypotheses scored), ``labels``
    float32 [n] (1 = inlier of the winner), and the correspondences ``src_corr`` / ``tgt_corr`` [n, 3]."""

    def __init__(self, transformation, fit, info, labels, src_corr, tgt_corr, hyp_status=None):
        self.transformation, self.fit, self.info, self.labels = transformation, fit, info, labels
        self.src_corr, self.tgt_corr, self.hyp_status = src_corr, tgt_corr, hyp_status

    @property
    def fitness(self):
        return self.fit[0]

    @property
    def inlier_rmse(self):
        return self.fit[1]


class BatchRegistrationResult:
    """Device tensors of a batch of registrations: ``transformation`` [B, 4, 4], ``fit`` [B, 2] (fitness, inlier rmse),
    ``info`` int32 [B, 4], ``labels`` float32 [B, n] (0 from a pair's count on), ``counts`` int32 [B] (the device counts the
    pairs ran on, None: n for every pair), ``hyp_status`` int32 [B, max_iteration] or None, and the correspondences
    ``src_corr`` / ``tgt_corr`` [B, n, 3] as passed.  ``count`` / ``n_mutual`` (device scalars) are set by the mutual-filter
    registration of one pair."""

    def __init__(self, transformation, fit, info, labels, counts, src_corr, tgt_corr, hyp_status=None):
        self.transformation, self.fit, self.info, self.labels, self.counts = transformation, fit, info, labels, counts
        self.src_corr, self.tgt_corr, self.hyp_status = src_corr, tgt_corr, hyp_status
        self.count = self.n_mutual = None


def _draw_seed(seed):
    # np.random, like every other draw of the eval loops: np.random.seed makes a run reproducible
    return int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF


def ransac_correspondences(src, tgt, max_correspondence_distance, ransac_n=4, edge_length_similarity=0.9,
                           checker_distance=None, max_iteration=4000000, confidence=0.999, seed=None, chunk=0,
                           want_status=False):
    """RANSAC on given correspondences ``src[i] <-> tgt[i]`` (device tensors [n, 3]).  ``chunk`` 0: the library's default,
    capped at the iteration count; ``want_status``: also the per-hypothesis status table (a diagnostic).

    Memory: every call takes its scratch (``gcl_ransac_scratch_bytes``: ~ 150 bytes per hypothesis of a chunk, 40 MB at the
    default chunk of 262 144, most of it the per-range partial scores) and a small output block from torch's caching
    allocator, on the current stream -- cheap after the first call, part of the measured time per registration, and one
    block per stream when registrations run on several streams (``GCL_EVAL_STREAMS`` > 1)."""
    lib = _lib.require_gpu()
    src, tgt = src.detach().to(torch.float32).contiguous(), tgt.detach().to(torch.float32).contiguous()
    if src.dim() != 2 or src.shape[1] != 3 or src.shape != tgt.shape:
        raise ValueError(f"correspondences must be two [n, 3] tensors, got {tuple(src.shape)} and {tuple(tgt.shape)}")
    n, dev = src.shape[0], src.device
    if checker_distance is None:
        checker_distance = max_correspondence_distance
    max_iteration = int(max_iteration)
    if chunk == 0:
        chunk = min(lib.gcl_ransac_default_chunk(), max(256, (max_iteration + 255) // 256 * 256))
    seed = _draw_seed(seed)
    # one block for the outputs: trans16 | info | fit | labels
    off_info, off_fit, off_labels = 64, 128, 256
    buf = torch.empty(off_labels + 4 * max(n, 1), dtype=torch.uint8, device=dev)
    status = torch.empty(max_iteration, dtype=torch.int32, device=dev) if want_status else None
    scratch = torch.empty(max(lib.gcl_ransac_scratch_bytes(n, chunk), 1), dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    _lib.check(lib.gcl_ransac_register(_lib.ptr(src), _lib.ptr(tgt), n, int(ransac_n), float(edge_length_similarity),
                                       float(checker_distance), float(max_correspondence_distance), max_iteration,
                                       float(confidence), ctypes.c_uint64(seed), int(chunk), _lib.ptr(scratch), base,
                                       base + off_info, base + off_fit, base + off_labels, _lib.ptr(status),
                                       _lib.stream()), "gcl_ransac_register")
    return RegistrationResult(buf[:64].view(torch.float32).view(4, 4), buf[off_fit:off_fit + 8].view(torch.float32),
                              buf[off_info:off_info + 16].view(torch.int32),
                              buf[off_labels:off_labels + 4 * n].view(torch.float32), src, tgt, status)


def ransac_correspondences_batch(src, tgt, max_correspondence_distance, ransac_n=4, edge_length_similarity=0.9,
                                 checker_distance=None, max_iteration=4000000, confidence=0.999, counts=None, seeds=None,
                                 chunk=0, want_status=False):
    """RANSAC on B sets of correspondences ``src[b, i] <-> tgt[b, i]`` (device tensors [B, n, 3]) in ONE call with the
    launches of one pair.  ``counts`` (device int32 [B], optional): pair b runs on its first ``counts[b]`` rows, read on the
    device (rows beyond are never read; fewer than ``ransac_n``: identity, info[0] = -1).  ``seeds``: B integers, or None:
    drawn from ``np.random`` in pair order.  A pair's result is bitwise what ``ransac_correspondences`` gives for its rows
    and seed.

    Memory: the scratch is the single-pair layout times B (``gcl_ransac_batch_scratch_bytes``): about 40 MB per pair at the
    default chunk."""
    lib = _lib.require_gpu()
    src, tgt = src.detach().to(torch.float32).contiguous(), tgt.detach().to(torch.float32).contiguous()
    if src.dim() != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape != tgt.shape:
        raise ValueError(f"correspondences must be two [B, n, 3] tensors, got {tuple(src.shape)} and {tuple(tgt.shape)}")
    B, n, dev = src.shape[0], src.shape[1], src.device
    if counts is not None:
        if counts.dtype != torch.int32 or counts.shape != (B,) or counts.device != dev:
            raise ValueError(f"counts must be a device int32 tensor [{B}], got {counts.dtype} {tuple(counts.shape)}")
        counts = counts.contiguous()
    if checker_distance is None:
        checker_distance = max_correspondence_distance
    max_iteration = int(max_iteration)
    if chunk == 0:
        chunk = min(lib.gcl_ransac_default_chunk(), max(256, (max_iteration + 255) // 256 * 256))
    seeds = [_draw_seed(None) for _ in range(B)] if seeds is None else [_draw_seed(s) for s in seeds]
    if len(seeds) != B:
        raise ValueError(f"{B} pairs but {len(seeds)} seeds")
    seed_arr = (ctypes.c_uint64 * B)(*seeds)
    trans = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    fit = torch.empty((B, 2), dtype=torch.float32, device=dev)
    labels = torch.empty((B, n), dtype=torch.float32, device=dev)
    status = torch.empty((B, max_iteration), dtype=torch.int32, device=dev) if want_status else None
    scratch = torch.empty(max(lib.gcl_ransac_batch_scratch_bytes(B, n, chunk), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.gcl_ransac_register_batch(_lib.ptr(src), _lib.ptr(tgt), B, n, _lib.ptr(counts), int(ransac_n),
                                             float(edge_length_similarity), float(checker_distance),
                                             float(max_correspondence_distance), max_iteration, float(confidence), seed_arr,
                                             int(chunk), _lib.ptr(scratch), _lib.ptr(trans), _lib.ptr(info), _lib.ptr(fit),
                                             _lib.ptr(labels), _lib.ptr(status), _lib.stream()),
               "gcl_ransac_register_batch")
    return BatchRegistrationResult(trans, fit, info, labels, counts, src, tgt, status)


def mutual_correspondences(xyz0, xyz1, F0, F1, min_count, src_out=None, tgt_out=None, count_out=None):
    """open3d's correspondence set under ``mutual_filter=True`` on the device: the feature 1-NN both ways (two ``pdist_min``
    calls) and ``gcl_mutual_correspondences``.  Returns ``(src [N0, 3], tgt [N0, 3], count int32 [2])``: the mutual pairs as
    point rows in ascending source order with zero rows behind them and count = (their number, their number), or -- fewer
    than ``min_count`` of them -- every source beside its nearest target and count = (N0, number of mutual pairs).  The
    three outputs may be given (slices of a batch's buffers)."""
    lib = _lib.require_gpu()
    xyz0, xyz1 = xyz0.detach().to(torch.float32).contiguous(), xyz1.detach().to(torch.float32).contiguous()
    m0, m1, dev = xyz0.shape[0], xyz1.shape[0], xyz0.device
    _, nn01 = pdist_min(F0, F1, "SquareL2")
    _, nn10 = pdist_min(F1, F0, "SquareL2")
    src = torch.empty((m0, 3), dtype=torch.float32, device=dev) if src_out is None else src_out
    tgt = torch.empty((m0, 3), dtype=torch.float32, device=dev) if tgt_out is None else tgt_out
    count = torch.empty(2, dtype=torch.int32, device=dev) if count_out is None else count_out
    if tuple(src.shape) != (m0, 3) or tuple(tgt.shape) != (m0, 3) or tuple(count.shape) != (2,):
        raise ValueError("mutual_correspondences: outputs must be [N0, 3], [N0, 3] and [2]")
    _lib.check(lib.gcl_mutual_correspondences(_lib.ptr(nn01, torch.int32), m0, _lib.ptr(nn10, torch.int32), m1, _lib.ptr(xyz0),
                                              _lib.ptr(xyz1), int(min_count), _lib.ptr(src, torch.float32),
                                              _lib.ptr(tgt, torch.float32), _lib.ptr(count, torch.int32), _lib.stream()),
               "gcl_mutual_correspondences")
    return src, tgt, count


def mutual_correspondences_batch(xyz0, xyz1, F0, F1, min_count, src_out=None, tgt_out=None, count_out=None):
    """``mutual_correspondences`` for B pairs ([B, N0, ...] / [B, N1, ...] tensors) in a fixed number of launches: both
    directions of every pair are the 2 B searches of ONE ``pdist_min_batch``, the filter is ONE
    ``gcl_mutual_correspondences_batch`` (one workgroup per pair).  Returns ``(src [B, N0, 3], tgt [B, N0, 3], count int32
    [B, 2])``, every pair's rows bitwise those of ``mutual_correspondences``."""
    lib = _lib.require_gpu()
    xyz0, xyz1 = xyz0.detach().to(torch.float32).contiguous(), xyz1.detach().to(torch.float32).contiguous()
    B, m0, m1, dev = xyz0.shape[0], xyz0.shape[1], xyz1.shape[1], xyz0.device
    src = torch.empty((B, m0, 3), dtype=torch.float32, device=dev) if src_out is None else src_out
    tgt = torch.empty((B, m0, 3), dtype=torch.float32, device=dev) if tgt_out is None else tgt_out
    count = torch.empty((B, 2), dtype=torch.int32, device=dev) if count_out is None else count_out
    if tuple(src.shape) != (B, m0, 3) or tuple(tgt.shape) != (B, m0, 3) or tuple(count.shape) != (B, 2):
        raise ValueError("mutual_correspondences_batch: outputs must be [B, N0, 3], [B, N0, 3] and [B, 2]")
    nn = pdist_min_batch([(F0[b], F1[b]) for b in range(B)] + [(F1[b], F0[b]) for b in range(B)], "SquareL2")
    recs, table = mutual_jobs([dict(nn01=nn[b][1], nn10=nn[B + b][1], xyz0=xyz0[b], xyz1=xyz1[b], src=src[b], tgt=tgt[b],
                                    count=count[b], m0=m0, m1=m1) for b in range(B)], dev)
    _lib.check(lib.gcl_mutual_correspondences_batch(ctypes.addressof(recs), _lib.ptr(table), B, int(min_count),
                                                    _lib.stream()), "gcl_mutual_correspondences_batch")
    return src, tgt, count


def registration_ransac_based_on_mutual_feature_matching(xyz0, xyz1, F0, F1, max_correspondence_distance=0.3, ransac_n=4,
                                                         edge_length_similarity=0.9, checker_distance=None,
                                                         max_iteration=4000000, confidence=0.999, seed=None):
    """open3d's ``registration_ransac_based_on_feature_matching(..., mutual_filter=True)`` (its default since 0.13) for one
    pair: a source is kept when its feature-nearest target has it as ITS nearest source; with fewer than ``ransac_n`` such
    pairs open3d falls back to every source with its nearest target.  The number of correspondences never leaves the
    device: the registration reads it there.  Returns a ``BatchRegistrationResult`` of one pair (``[1, ...]`` tensors, zero
    rows beyond the count) whose ``count`` and ``n_mutual`` are device scalars."""
    _lib.require_gpu()
    dev = xyz0.device
    src = torch.empty((1, xyz0.shape[0], 3), dtype=torch.float32, device=dev)
    tgt = torch.empty_like(src)
    cnt = torch.empty((1, 2), dtype=torch.int32, device=dev)
    mutual_correspondences(xyz0, xyz1, F0, F1, ransac_n, src[0], tgt[0], cnt[0])
    res = ransac_correspondences_batch(src, tgt, max_correspondence_distance, ransac_n, edge_length_similarity,
                                       checker_distance, max_iteration, confidence, cnt[:, 0].contiguous(), [_draw_seed(seed)])
    res.count, res.n_mutual = cnt[0, 0], cnt[0, 1]
    return res


def registration_ransac_based_on_feature_matching(xyz0, xyz1, F0, F1, mutual_filter=False, max_correspondence_distance=0.3,
                                                  ransac_n=4, edge_length_similarity=0.9, checker_distance=None,
                                                  max_iteration=4000000, confidence=0.999, seed=None):
    """open3d's call of the same name on device tensors: points [N0, 3] / [N1, 3], features [N0, C] / [N1, C].  The
    estimation is point-to-point without scaling and the checkers are the two the reference passes (edge length,
    distance; ``checker_distance`` None = ``max_correspondence_distance``, as in both of its call sites)."""
    if mutual_filter:
        raise NotImplementedError("mutual_filter=True is not served by this function: call "
                                  "registration_ransac_based_on_mutual_feature_matching, which keeps the number of "
                                  "correspondences on the device (the reference passes False at both call sites)")
    _lib.require_gpu()
    _, arg = pdist_min(F0, F1, "SquareL2")
    tgt = xyz1.to(torch.float32)[arg.long()]
    return ransac_correspondences(xyz0.to(torch.float32), tgt, max_correspondence_distance, ransac_n,
                                  edge_length_similarity, checker_distance, max_iteration, confidence, seed)


class FeatureRansac:
    """The RANSAC branch as a ``Matcher``: ``estimator`` has ``Matcher.estimator``'s contract for any batch size.  One pair
    without the mutual filter is one ``gcl_ransac_register`` call; a batch, or ``mutual_filter=True`` (open3d's default since
    0.13; the reference passes False), is ONE ``gcl_ransac_register_batch`` call behind the pairs' 1-NN searches (a batch: one ``pdist_min_batch`` call that
    writes the correspondences, with the filter one ``gcl_mutual_correspondences_batch``), and the
    returned tensors are [B, ...] with zero rows beyond a pair's correspondence count.

    NOTE on ``confidence``: the default everywhere here, ``kitti()`` and ``eth()`` included, is open3d's own default 0.999,
    which stops a run once enough hypotheses have been drawn for the best inlier share found (0.3 ms instead of 0.8 ms per
    registration at an inlier share of 0.3).  The reference's two calls pass
    ``RANSACConvergenceCriteria(4000000, 10000)`` / ``(50000, 1000)``: under open3d >= 0.13 that second number is a
    confidence clamped to 1, i.e. NO early stop.  To run exactly what the reference runs on a current open3d pass
    ``confidence=1.0``."""

    def __init__(self, max_correspondence_distance, ransac_n=4, edge_length_similarity=0.9, checker_distance=None,
                 max_iteration=4000000, confidence=0.999, seed=None, mutual_filter=False):
        self.max_correspondence_distance, self.ransac_n = float(max_correspondence_distance), int(ransac_n)
        self.edge_length_similarity = float(edge_length_similarity)
        self.checker_distance = self.max_correspondence_distance if checker_distance is None else float(checker_distance)
        self.max_iteration, self.confidence, self.seed = int(max_iteration), float(confidence), seed
        self.mutual_filter = bool(mutual_filter)
        self.last = None

    accepts_batch = True      # scripts/eval_batch.eval_pairs(..., batch_registration=True) asks for this

    def draw_seed(self):
        """The seed of the next registration (``np.random`` when none was given): what ``estimator`` draws per pair."""
        return _draw_seed(self.seed)

    @classmethod
    def kitti(cls, voxel_size, confidence=0.999, seed=None, mutual_filter=False):
        """scripts/test_kitti.py:170-177: ransac_n 4, both distances one voxel, 4 000 000 iterations.  (The reference's
        second criterion argument, 10000, is ``max_validation`` of older open3d; open3d >= 0.13 reads it as a confidence
        and clamps it to 1, i.e. no early stop: pass ``confidence=1.0`` for that behaviour.)"""
        return cls(voxel_size * 1.0, 4, 0.9, None, 4000000, confidence, seed, mutual_filter)

    @classmethod
    def eth(cls, confidence=0.999, seed=None, mutual_filter=False):
        """generalization_ETH/evaluate.py:180-186: ransac_n 3, both distances 0.05, 50 000 iterations."""
        return cls(0.05, 3, 0.9, 0.05, 50000, confidence, seed, mutual_filter)

    def estimator(self, src_keypts, tgt_keypts, src_features, tgt_features, seeds=None):
        """``seeds``: one per pair, for a caller that has drawn them already (``draw_seed``, in its own order of host
        draws); None: drawn here, in pair order."""
        _lib.require_gpu()
        B = src_keypts.shape[0]
        if B < 1:
            raise ValueError("estimator needs at least one pair")
        if seeds is not None and len(seeds) != B:
            raise ValueError(f"{B} pairs but {len(seeds)} seeds")
        if B == 1 and not self.mutual_filter:
            res = registration_ransac_based_on_feature_matching(
                src_keypts[0], tgt_keypts[0], src_features[0], tgt_features[0], False, self.max_correspondence_distance,
                self.ransac_n, self.edge_length_similarity, self.checker_distance, self.max_iteration, self.confidence,
                self.seed if seeds is None else seeds[0])
            self.last = res
            return res.transformation[None], res.labels[None], res.src_corr[None], res.tgt_corr[None]
        dev = src_keypts.device
        src = torch.empty((B, src_keypts.shape[1], 3), dtype=torch.float32, device=dev)
        tgt = torch.empty_like(src)
        cnt = torch.empty((B, 2), dtype=torch.int32, device=dev) if self.mutual_filter else None
        if B == 1:                                                           # one pair keeps the single entries
            mutual_correspondences(src_keypts[0], tgt_keypts[0], src_features[0], tgt_features[0], self.ransac_n, src[0], tgt[0],
                                   cnt[0])
        elif self.mutual_filter:
            mutual_correspondences_batch(src_keypts, tgt_keypts, src_features, tgt_features, self.ransac_n, src, tgt, cnt)
        else:                                                                # the B searches and their gathers in one call
            kp0, kp1 = src_keypts.to(torch.float32).contiguous(), tgt_keypts.to(torch.float32).contiguous()
            pdist_min_batch([(src_features[b], tgt_features[b], None, None, kp0[b], kp1[b], src[b], tgt[b]) for b in range(B)],
                            "SquareL2")
        if seeds is None:
            seeds = [self.draw_seed() for _ in range(B)]
        res = ransac_correspondences_batch(src, tgt, self.max_correspondence_distance, self.ransac_n,
                                           self.edge_length_similarity, self.checker_distance, self.max_iteration,
                                           self.confidence, None if cnt is None else cnt[:, 0].contiguous(), seeds)
        if cnt is not None:
            res.count, res.n_mutual = cnt[:, 0], cnt[:, 1]
        self.last = res
        return res.transformation, res.labels, res.src_corr, res.tgt_corr
