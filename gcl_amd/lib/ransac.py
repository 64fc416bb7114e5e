"""Feature-matching RANSAC registration on the MI355X kernels: open3d's
``registration_ransac_based_on_feature_matching`` as the reference calls it (scripts/test_kitti.py:171-178 -- the default
registration of the KITTI loop -- and generalization_ETH/evaluate.py:171-186).

Putative correspondences are every source row paired with its feature-nearest target row (``pdist_min`` ->
``gcl_nn_rowmin``, open3d's ``mutual_filter=False`` path); the registration is ONE C-ABI call (include/gcl_amd.h,
``gcl_ransac_register``: draw, edge-length checker, fp64 Kabsch, distance checker, inlier scoring, winner and the confidence
stop, all on the device).  Minimal samples come from a counter generator keyed by ``seed`` in place of open3d's
``std::mt19937``: a seeded run is reproducible bit for bit.  Nothing leaves the device until the caller reads the result.

``FeatureRansac`` speaks ``Matcher.estimator``'s calling convention (scripts/SC2_PCR.py), so
``eval_pairs(model, pairs, FeatureRansac.kitti(voxel_size))`` and ``evaluate_scene(..., matcher=FeatureRansac.eth())`` run
the reference's two RANSAC configurations through the loops that already exist.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.metrics import pdist_min


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


def registration_ransac_based_on_feature_matching(xyz0, xyz1, F0, F1, mutual_filter=False, max_correspondence_distance=0.3,
                                                  ransac_n=4, edge_length_similarity=0.9, checker_distance=None,
                                                  max_iteration=4000000, confidence=0.999, seed=None):
    """open3d's call of the same name on device tensors: points [N0, 3] / [N1, 3], features [N0, C] / [N1, C].  The
    estimation is point-to-point without scaling and the checkers are the two the reference passes (edge length,
    distance; ``checker_distance`` None = ``max_correspondence_distance``, as in both of its call sites)."""
    if mutual_filter:
        raise NotImplementedError("mutual_filter=True is not built: the number of correspondences would have to live on "
                                  "the device (the reference passes False at both call sites)")
    _lib.require_gpu()
    _, arg = pdist_min(F0, F1, "SquareL2")
    tgt = xyz1.to(torch.float32)[arg.long()]
    return ransac_correspondences(xyz0.to(torch.float32), tgt, max_correspondence_distance, ransac_n,
                                  edge_length_similarity, checker_distance, max_iteration, confidence, seed)


class FeatureRansac:
    """The RANSAC branch as a ``Matcher``: ``estimator`` has ``Matcher.estimator``'s contract, batch size 1.

    NOTE on ``confidence``: the default everywhere here, ``kitti()`` and ``eth()`` included, is open3d's own default 0.999,
    which stops a run once enough hypotheses have been drawn for the best inlier share found (0.3 ms instead of 0.8 ms per
    registration at an inlier share of 0.3).  The reference's two calls pass
    ``RANSACConvergenceCriteria(4000000, 10000)`` / ``(50000, 1000)``: under open3d >= 0.13 that second number is a
    confidence clamped to 1, i.e. NO early stop.  To run exactly what the reference runs on a current open3d pass
    ``confidence=1.0``."""

    def __init__(self, max_correspondence_distance, ransac_n=4, edge_length_similarity=0.9, checker_distance=None,
                 max_iteration=4000000, confidence=0.999, seed=None):
        self.max_correspondence_distance, self.ransac_n = float(max_correspondence_distance), int(ransac_n)
        self.edge_length_similarity = float(edge_length_similarity)
        self.checker_distance = self.max_correspondence_distance if checker_distance is None else float(checker_distance)
        self.max_iteration, self.confidence, self.seed = int(max_iteration), float(confidence), seed
        self.last = None

    @classmethod
    def kitti(cls, voxel_size, confidence=0.999, seed=None):
        """scripts/test_kitti.py:170-177: ransac_n 4, both distances one voxel, 4 000 000 iterations.  (The reference's
        second criterion argument, 10000, is ``max_validation`` of older open3d; open3d >= 0.13 reads it as a confidence
        and clamps it to 1, i.e. no early stop: pass ``confidence=1.0`` for that behaviour.)"""
        return cls(voxel_size * 1.0, 4, 0.9, None, 4000000, confidence, seed)

    @classmethod
    def eth(cls, confidence=0.999, seed=None):
        """generalization_ETH/evaluate.py:180-186: ransac_n 3, both distances 0.05, 50 000 iterations."""
        return cls(0.05, 3, 0.9, 0.05, 50000, confidence, seed)

    def estimator(self, src_keypts, tgt_keypts, src_features, tgt_features):
        _lib.require_gpu()
        if src_keypts.shape[0] != 1:
            raise NotImplementedError("batch size 1 only (as Matcher.estimator)")
        res = registration_ransac_based_on_feature_matching(
            src_keypts[0], tgt_keypts[0], src_features[0], tgt_features[0], False, self.max_correspondence_distance,
            self.ransac_n, self.edge_length_similarity, self.checker_distance, self.max_iteration, self.confidence, self.seed)
        self.last = res
        return res.transformation[None], res.labels[None], res.src_corr[None], res.tgt_corr[None]
