"""SC2-PCR registration back-end on the MI355X kernels (interface of scripts/SC2_PCR/SC2_PCR.py: class ``Matcher``).

``Matcher(**config_KITTI.json).estimator(src_keypts, tgt_keypts, src_features, tgt_features)`` as called by the eval
loop (scripts/test_kitti.py:172-180); ``Matcher`` registers one pair per call (the reference asserts it too, :42, :249),
``BatchMatcher`` below takes [B, n, 3] and registers the B pairs in the launches of one (gcl_sc2_register_batch).  Putative
correspondences come from ``gcl_nn_rowmin`` (the reference's argmin of sqrt(2 - 2 f.g) over L2-normalised features
is the argmin of |f - g|^2); the registration itself is ONE C-ABI call (include/gcl_amd.h, gcl_sc2_register; with
``GCL_SC2_ONE_CALL=0`` the five staged calls with three small torch steps in between -- a stable sort for the seeds, an
argmax, the inlier labels -- that it replaced: same kernels, same results).  Nothing leaves the device until the caller
reads the result.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device
from gcl_amd.lib.metrics import pdist_min, pdist_min_batch

import os

SPARSE_CONFIDENCE = os.environ.get("GCL_SC2_SPARSE", "1") != "0"      # gcl_sc2_confidence_sparse (round 5)
ONE_CALL = os.environ.get("GCL_SC2_ONE_CALL", "1") != "0"              # gcl_sc2_register: the stages below as one call


class _Stages:
    """``Matcher.last`` of a one-call registration: views into its output buffer, made when asked for."""

    def __init__(self, buf, fields):
        self._buf, self._fields = buf, fields

    def __getitem__(self, name):
        off, count, dtype, shape = self._fields[name]
        v = self._buf[off:off + count * dtype.itemsize].view(dtype)
        v = v.view(shape) if shape is not None else v
        return v[0] if name == "best" else v

    def keys(self):
        return self._fields.keys()


class Matcher:
    def __init__(self, inlier_threshold=0.10, num_node="all", use_mutual=True, d_thre=0.1, num_iterations=10,
                 ratio=0.2, nms_radius=0.1, max_points=8000, k1=30, k2=20, select_scene=None):
        self.inlier_threshold, self.num_node, self.use_mutual = inlier_threshold, num_node, use_mutual
        self.d_thre, self.num_iterations, self.ratio = d_thre, num_iterations, ratio
        self.max_points, self.nms_radius, self.k1, self.k2 = max_points, nms_radius, k1, k2

    # ---- scripts/SC2_PCR/SC2_PCR.py:281-302 --------------------------------------------------------------------
    def match_pair(self, src_keypts, tgt_keypts, src_features, tgt_features):
        N_src, N_tgt = src_features.shape[1], tgt_features.shape[1]
        dev = src_features.device
        if self.num_node == "all":
            src_sel, tgt_sel = None, None
        else:                                                    # with replacement, as the reference (:289-290)
            src_sel = host_to_device(np.random.choice(N_src, self.num_node), dev)      # pinned block, non-blocking copy
            tgt_sel = host_to_device(np.random.choice(N_tgt, self.num_node), dev)
        _, arg = pdist_min(src_features[0], tgt_features[0], "SquareL2", rows_a=src_sel, rows_b=tgt_sel)
        arg = arg.long()
        src_rows = src_sel if src_sel is not None else torch.arange(N_src, device=dev)
        tgt_rows = tgt_sel[arg] if tgt_sel is not None else arg
        return src_keypts[:, src_rows], tgt_keypts[:, tgt_rows]

    # ---- :304-381 ------------------------------------------------------------------------------------------------
    def SC2_PCR(self, src_keypts, tgt_keypts):
        lib = _lib.require_gpu()
        if src_keypts.shape[0] != 1:
            raise NotImplementedError("batch size 1 only (as the reference's pick_seeds / post_refinement)")
        src = src_keypts[0, :self.max_points].to(torch.float32).contiguous()
        tgt = tgt_keypts[0, :self.max_points].to(torch.float32).contiguous()
        n = src.shape[0]
        dev = src.device
        st = _lib.stream()
        n_seeds = int(n * self.ratio)
        if n_seeds < 1:
            raise ValueError("too few correspondences for SC2-PCR")
        k1, k2 = (self.k1, self.k2) if self.k1 <= n else (4, 4)                      # :75-77
        thr = 0.10 if self.inlier_threshold == 0.10 else 1.2
        if ONE_CALL and SPARSE_CONFIDENCE:
            # every stage below in ONE native call (same kernels, same results): two allocations, no torch operation between
            # the stages -- the loop over pairs was bound by this thread, not by the device
            fields, off = {}, 0
            for name, count, dtype, shape in (("out", 16, torch.float32, (1, 4, 4)), ("labels", n, torch.float32, (1, n)),
                                              ("conf", n, torch.float32, None), ("seeds", n_seeds, torch.int64, None),
                                              ("knn", n_seeds * k1, torch.int32, (n_seeds, k1)),
                                              ("seed_trans", n_seeds * 12, torch.float32, (n_seeds, 12)),
                                              ("fitness", n_seeds, torch.float32, None), ("best", 1, torch.int32, None)):
                fields[name] = (off, count, dtype, shape)
                off += (count * dtype.itemsize + 255) // 256 * 256
            buf = torch.empty(off, dtype=torch.uint8, device=dev)
            scratch = torch.empty(lib.gcl_sc2_register_scratch_bytes(n), dtype=torch.uint8, device=dev)
            base = buf.data_ptr()
            at = lambda name: base + fields[name][0]
            _lib.check(lib.gcl_sc2_register(_lib.ptr(src), _lib.ptr(tgt), n, float(self.d_thre), int(self.num_iterations),
                                            float(self.nms_radius), n_seeds, k1, k2, float(self.inlier_threshold), thr, 20,
                                            _lib.ptr(scratch), at("conf"), at("seeds"), at("knn"), at("seed_trans"),
                                            at("fitness"), at("best"), at("out"), at("labels"), st), "gcl_sc2_register")
            self.last = _Stages(buf, fields)
            self._labels = self.last["labels"]
            return self.last["out"]
        self._labels = None
        # confidence of every correspondence (:337-345)
        conf = torch.ones(n, dtype=torch.float32, device=dev)
        partial = torch.empty(lib.gcl_sc2_chunks() * n, dtype=torch.float32, device=dev)
        done = torch.zeros(1, dtype=torch.int32, device=dev)
        if SPARSE_CONFIDENCE:      # the matrix's non-zero entries kept from one build: bitwise the dense products' result
            scratch = torch.empty(lib.gcl_sc2_confidence_scratch_bytes(n), dtype=torch.uint8, device=dev)
            _lib.check(lib.gcl_sc2_confidence_sparse(_lib.ptr(src), _lib.ptr(tgt), n, float(self.d_thre),
                                                     int(self.num_iterations), _lib.ptr(partial), _lib.ptr(conf),
                                                     _lib.ptr(done), _lib.ptr(scratch), st), "gcl_sc2_confidence_sparse")
        else:
            _lib.check(lib.gcl_sc2_confidence(_lib.ptr(src), _lib.ptr(tgt), n, float(self.d_thre),
                                              int(self.num_iterations), _lib.ptr(partial), _lib.ptr(conf), _lib.ptr(done),
                                              st), "gcl_sc2_confidence")
        # seeds: local maxima first, by confidence (:32-58); ties -> lowest index
        is_max = torch.ones(n, dtype=torch.int32, device=dev)
        _lib.check(lib.gcl_sc2_local_max(_lib.ptr(src), _lib.ptr(conf), n, float(self.nms_radius), _lib.ptr(is_max),
                                         st), "gcl_sc2_local_max")
        seeds = torch.sort(-(conf * is_max.float()), stable=True)[1][:n_seeds].contiguous()
        # k1 most compatible correspondences of every seed under the second-order measure (:353-361, :85-86)
        bits = torch.empty(n * ((n + 63) // 64), dtype=torch.int64, device=dev)
        knn = torch.empty((n_seeds, k1), dtype=torch.int32, device=dev)
        _lib.check(lib.gcl_sc2_seed_knn(_lib.ptr(src), _lib.ptr(tgt), n, _lib.ptr(seeds), n_seeds, float(self.d_thre),
                                        k1, _lib.ptr(bits), _lib.ptr(knn), st), "gcl_sc2_seed_knn")
        # one hypothesis per seed and its inlier count (:88-161)
        trans = torch.empty((n_seeds, 12), dtype=torch.float32, device=dev)
        fitness = torch.empty(n_seeds, dtype=torch.float32, device=dev)
        _lib.check(lib.gcl_sc2_seed_trans(_lib.ptr(src), _lib.ptr(tgt), n, _lib.ptr(knn), n_seeds, k1, k2,
                                          float(self.d_thre), int(self.num_iterations), float(self.inlier_threshold),
                                          _lib.ptr(trans), _lib.ptr(fitness), st), "gcl_sc2_seed_trans")
        best = torch.sort(-fitness, stable=True)[1][0]
        T = trans[best].clone()
        # post refinement over all correspondences (:238-279)
        rpart = torch.empty(lib.gcl_sc2_refine_partial_len(), dtype=torch.float64, device=dev)
        state = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.gcl_sc2_refine(_lib.ptr(src), _lib.ptr(tgt), n, thr, 20, _lib.ptr(rpart), _lib.ptr(state),
                                      _lib.ptr(T), st), "gcl_sc2_refine")
        out = torch.zeros((1, 4, 4), dtype=torch.float32, device=dev)
        out[0, :3, :] = T.view(3, 4)
        out[0, 3, 3] = 1.0
        self.last = dict(conf=conf, seeds=seeds, knn=knn, seed_trans=trans, fitness=fitness, best=best)
        return out

    # ---- :383-410 ------------------------------------------------------------------------------------------------
    def estimator(self, src_keypts, tgt_keypts, src_features, tgt_features):
        src_corr, tgt_corr = self.match_pair(src_keypts, tgt_keypts, src_features, tgt_features)
        pred_trans = self.SC2_PCR(src_corr, tgt_corr)
        if self._labels is not None and src_corr.shape[1] <= self.max_points:      # made by the registration call itself
            return pred_trans, self._labels, src_corr, tgt_corr
        warped = src_corr @ pred_trans[:, :3, :3].transpose(1, 2) + pred_trans[:, None, :3, 3]
        distance = torch.sum((warped - tgt_corr) ** 2, dim=-1) ** 0.5
        pred_labels = (distance < self.inlier_threshold).float()
        return pred_trans, pred_labels, src_corr, tgt_corr


MAX_CORRESPONDENCES = 8192      # SC_MAXN of csrc/sc2pcr.hip: the scratch size functions answer 0 beyond it


def split_batch(n_pairs, pair_bytes, max_batch_bytes):
    """Consecutive sub-batches [(b0, b1), ...] of ``n_pairs`` pairs whose scratch (``pair_bytes`` each) stays within
    ``max_batch_bytes``; a sub-batch has at least one pair, whatever the limit.  Pure host arithmetic."""
    per = max(1, int(max_batch_bytes) // max(1, int(pair_bytes)))
    return [(b0, min(n_pairs, b0 + per)) for b0 in range(0, n_pairs, per)]


class _BatchStages:
    """``BatchMatcher.last``: ``last[b][name]`` is pair b's view of stage ``name`` (the names of ``Matcher.last``), cut to the
    pair's own extent; the views are made when asked for."""

    def __init__(self, pairs):
        self._pairs = pairs          # per pair: (dict name -> [pairs of its sub-batch, ...] tensor, row, n, n_seeds)

    def __len__(self):
        return len(self._pairs)

    def __getitem__(self, b):
        views, row, n, n_seeds = self._pairs[b]

        class _One:
            def __getitem__(_, name):
                v = views[name][row]
                if name == "out":
                    return v.view(1, 4, 4)
                if name == "labels":
                    return v[:n].view(1, n)
                if name == "conf":
                    return v[:n]
                return v if name == "best" else v[:n_seeds]

            def keys(_):
                return views.keys()

        return _One()


class BatchMatcher(Matcher):
    """``Matcher`` for a batch of pairs: ``SC2_PCR`` / ``estimator`` take [B, n, ...] tensors and make ONE
    ``gcl_sc2_register_batch`` call -- the launches of one registration with the pair as the grids' z dimension -- whose
    results equal ``Matcher``'s on every pair alone bit for bit (the two entries launch the same kernel bodies).
    SCRATCH: ~ 8 n^2 bytes per pair (528 MB at n = 8000); a batch that would need more than ``max_batch_bytes`` runs as
    consecutive sub-batches on one scratch block."""

    accepts_batch = True             # scripts/eval_batch.eval_pairs(..., batch_registration=True) asks for these two
    draw_takes_sizes = True

    def __init__(self, *args, max_batch_bytes=8 << 30, **kwargs):
        super().__init__(*args, **kwargs)
        self.max_batch_bytes = int(max_batch_bytes)
        self.last = None

    def draw_seed(self, n_src, n_tgt):
        """The host draws ``Matcher.match_pair`` makes for one pair with ``n_src`` / ``n_tgt`` feature rows, in its order:
        None for ``num_node == 'all'``, else the (source rows, target rows) for ``estimator(seeds=...)``."""
        if self.num_node == "all":
            return None
        return np.random.choice(n_src, self.num_node), np.random.choice(n_tgt, self.num_node)

    def plan(self, n_cap, counts=None, n_pairs=None):
        """Host half of ``SC2_PCR``: per pair the count after the ``max_points`` cut and ``int(n * ratio)`` seeds, and the
        batch's (k1, k2).  Raises ``ValueError`` for a pair without a seed and for a batch whose pairs disagree on the
        reference's ``k1 > n -> (4, 4)`` rule (:75-77): one call has one k1."""
        if counts is None:
            counts = [n_cap] * n_pairs
        counts = [int(c) for c in counts]
        if n_pairs is not None and len(counts) != n_pairs:
            raise ValueError(f"{n_pairs} pairs but {len(counts)} counts")
        if any(c < 0 or c > n_cap for c in counts):
            raise ValueError(f"counts must lie in [0, {n_cap}], got {counts}")
        if min(n_cap, self.max_points) > MAX_CORRESPONDENCES:
            raise ValueError(f"a registration takes at most {MAX_CORRESPONDENCES} correspondences per pair; got {n_cap} with "
                             f"max_points = {self.max_points}: lower max_points")
        counts = [min(c, self.max_points) for c in counts]
        n_seeds = [int(c * self.ratio) for c in counts]
        if min(n_seeds) < 1:
            raise ValueError(f"too few correspondences for SC2-PCR: counts {counts} give {n_seeds} seeds")
        small = [self.k1 > c for c in counts]
        if any(small) and not all(small):
            raise ValueError(f"pairs with fewer than k1 = {self.k1} correspondences use (k1, k2) = (4, 4) and cannot share a "
                             f"call with pairs that do not: counts {counts}; register the two groups separately")
        k1, k2 = (4, 4) if small[0] else (self.k1, self.k2)
        return counts, n_seeds, k1, k2

    def SC2_PCR(self, src_keypts, tgt_keypts, counts=None):
        B = src_keypts.shape[0]
        if B < 1:
            raise ValueError("SC2_PCR needs at least one pair")
        counts, n_seeds, k1, k2 = self.plan(src_keypts.shape[1], counts, B)      # refusals before any GPU work
        lib = _lib.require_gpu()
        src = src_keypts[:, :self.max_points].to(torch.float32).contiguous()
        tgt = tgt_keypts[:, :self.max_points].to(torch.float32).contiguous()
        n_cap, dev, st = src.shape[1], src.device, _lib.stream()
        thr = 0.10 if self.inlier_threshold == 0.10 else 1.2
        subs = split_batch(B, lib.gcl_sc2_register_batch_scratch_bytes(1, n_cap), self.max_batch_bytes)
        # ONE output block: out and labels for the whole batch, then every sub-batch's stages at its own S = max(n_seeds)
        fields, off = [], 0

        def place(count, dtype):
            nonlocal off
            at = off
            off += (count * dtype.itemsize + 255) // 256 * 256
            return at, count, dtype

        head = dict(out=place(B * 16, torch.float32), labels=place(B * n_cap, torch.float32),
                    conf=place(B * n_cap, torch.float32), best=place(B, torch.int32))
        for b0, b1 in subs:
            S, nb = max(n_seeds[b0:b1]), b1 - b0
            fields.append((S, dict(seeds=place(nb * S, torch.int64), knn=place(nb * S * k1, torch.int32),
                                   seed_trans=place(nb * S * 12, torch.float32), fitness=place(nb * S, torch.float32))))
        buf = torch.empty(off, dtype=torch.uint8, device=dev)
        scratch = torch.empty(lib.gcl_sc2_register_batch_scratch_bytes(max(b1 - b0 for b0, b1 in subs), n_cap),
                              dtype=torch.uint8, device=dev)
        view = lambda f, *shape: buf[f[0]:f[0] + f[1] * f[2].itemsize].view(f[2]).view(*shape)
        out, labels = view(head["out"], B, 16), view(head["labels"], B, n_cap)
        conf, best = view(head["conf"], B, n_cap), view(head["best"], B)
        c_counts, c_seeds = (ctypes.c_int32 * B)(*counts), (ctypes.c_int32 * B)(*n_seeds)
        i32 = ctypes.sizeof(ctypes.c_int32)
        pairs = []
        for (b0, b1), (S, f) in zip(subs, fields):
            nb = b1 - b0
            v = dict(out=out[b0:b1], labels=labels[b0:b1], conf=conf[b0:b1], best=best[b0:b1],
                     seeds=view(f["seeds"], nb, S), knn=view(f["knn"], nb, S, k1),
                     seed_trans=view(f["seed_trans"], nb, S, 12), fitness=view(f["fitness"], nb, S))
            _lib.check(lib.gcl_sc2_register_batch(
                _lib.ptr(src[b0:b1]), _lib.ptr(tgt[b0:b1]), nb, n_cap, ctypes.byref(c_counts, b0 * i32),
                ctypes.byref(c_seeds, b0 * i32), float(self.d_thre), int(self.num_iterations), float(self.nms_radius),
                k1, k2, float(self.inlier_threshold), thr, 20, _lib.ptr(scratch), _lib.ptr(v["conf"]), _lib.ptr(v["seeds"]),
                _lib.ptr(v["knn"]), _lib.ptr(v["seed_trans"]), _lib.ptr(v["fitness"]), _lib.ptr(v["best"]),
                _lib.ptr(v["out"]), _lib.ptr(v["labels"]), st), "gcl_sc2_register_batch")
            pairs += [(v, b - b0, counts[b], n_seeds[b]) for b in range(b0, b1)]
        self.last = _BatchStages(pairs)
        self.counts = counts
        self._labels = labels
        return out.view(B, 4, 4)

    def _match_into(self, pairs, seeds, src_corr, tgt_corr):
        """``Matcher.match_pair`` for every ``(src_keypts, tgt_keypts, src_features, tgt_features)`` of ``pairs`` ([n, ...]
        tensors, ragged) under the draws ``seeds`` in ONE ``pdist_min_batch`` call: pair b's correspondences go to the first
        rows of ``src_corr[b]`` / ``tgt_corr[b]`` ([B, n_cap, 3]; rows beyond its count are left alone), written by the search
        itself when the points are float32, else by indexing with its arg-minima.  One copy brings all the draws over."""
        dev = src_corr.device
        drawn = [np.asarray(r, dtype=np.int64) for sel in seeds if sel is not None for r in sel]
        rows, at = (host_to_device(np.concatenate(drawn), dev), 0) if drawn else (None, 0)
        fused = all(p[0].dtype == torch.float32 and p[1].dtype == torch.float32 for p in pairs) and \
            src_corr.dtype == torch.float32 and tgt_corr.dtype == torch.float32
        problems, sels = [], []
        for b, ((sk, tk, sf, tf), sel) in enumerate(zip(pairs, seeds)):
            src_sel = tgt_sel = None
            if sel is not None:
                src_sel, tgt_sel = rows[at:at + len(sel[0])], rows[at + len(sel[0]):at + len(sel[0]) + len(sel[1])]
                at += len(sel[0]) + len(sel[1])
            n = sf.shape[0] if src_sel is None else src_sel.shape[0]
            sels.append((src_sel, tgt_sel, n))
            problems.append((sf, tf, src_sel, tgt_sel, sk, tk, src_corr[b, :n], tgt_corr[b, :n]) if fused
                            else (sf, tf, src_sel, tgt_sel))
        out = pdist_min_batch(problems, "SquareL2")
        if not fused:
            for b, ((sk, tk, _, _), (src_sel, tgt_sel, n)) in enumerate(zip(pairs, sels)):
                arg = out[b][1].long()
                src_corr[b, :n] = sk if src_sel is None else sk[src_sel]
                tgt_corr[b, :n] = tk[tgt_sel[arg] if tgt_sel is not None else arg]
        return [n for _, _, n in sels]

    def match_pairs(self, pairs, seeds=None):
        """``Matcher.match_pair`` for a list of RAGGED pairs ``(src_keypts, tgt_keypts, src_features, tgt_features)`` ([n, ...]
        or [1, n, ...] tensors) in one native call.  Returns ``(src [B, n_cap, 3], tgt [B, n_cap, 3], counts)`` (float32; a
        pair's rows beyond its count are never written): what ``SC2_PCR(src, tgt, counts=counts)`` takes.  The draws of an
        integer ``num_node`` are made first, in pair order -- the stream of B ``match_pair`` calls in a row -- unless ``seeds``
        (per pair what ``draw_seed`` returned) gives them."""
        pairs = [tuple(x[0] if x.dim() == 3 else x for x in p) for p in pairs]
        if len(pairs) < 1:
            raise ValueError("match_pairs needs at least one pair")
        if seeds is None:
            seeds = [self.draw_seed(sf.shape[0], tf.shape[0]) for _, _, sf, tf in pairs]
        if len(seeds) != len(pairs):
            raise ValueError(f"{len(pairs)} pairs but {len(seeds)} seeds")
        counts = [sf.shape[0] if sel is None else len(sel[0]) for (_, _, sf, _), sel in zip(pairs, seeds)]
        dev = pairs[0][2].device
        pairs = [(sk.to(torch.float32), tk.to(torch.float32), sf, tf) for sk, tk, sf, tf in pairs]
        src = torch.empty((len(pairs), max(counts), 3), dtype=torch.float32, device=dev)
        tgt = torch.empty_like(src)
        self._match_into(pairs, seeds, src, tgt)
        return src, tgt, counts

    def estimator(self, src_keypts, tgt_keypts, src_features, tgt_features, seeds=None):
        """``Matcher.estimator`` on [B, N, ...] tensors: the pairs' feature 1-NN searches as ONE call that writes the
        correspondences (one pair: ``Matcher.match_pair``'s calls), ONE registration call.  ``seeds``: per
        pair what ``draw_seed`` returned, for a caller that made the draws already (in its own order of host draws); None:
        drawn here, in pair order -- the draws of B ``Matcher.estimator`` calls in a row."""
        B = src_keypts.shape[0]
        N_src, N_tgt = src_features.shape[1], tgt_features.shape[1]
        if seeds is None:
            seeds = [self.draw_seed(N_src, N_tgt) for _ in range(B)]
        if len(seeds) != B:
            raise ValueError(f"{B} pairs but {len(seeds)} seeds")
        n = N_src if self.num_node == "all" else int(self.num_node)
        self.plan(n, None, B)                                                    # refusals before any GPU work
        dev = src_features.device
        src_corr = torch.empty((B, n, 3), dtype=src_keypts.dtype, device=dev)
        tgt_corr = torch.empty((B, n, 3), dtype=tgt_keypts.dtype, device=dev)
        if B == 1:                                                               # Matcher.match_pair with the given draws
            sel = seeds[0]
            src_sel, tgt_sel = (None, None) if sel is None else (host_to_device(sel[0], dev), host_to_device(sel[1], dev))
            _, arg = pdist_min(src_features[0], tgt_features[0], "SquareL2", rows_a=src_sel, rows_b=tgt_sel)
            arg = arg.long()
            src_corr[0] = src_keypts[0] if src_sel is None else src_keypts[0, src_sel]
            tgt_corr[0] = tgt_keypts[0, tgt_sel[arg] if tgt_sel is not None else arg]
        else:                                                                    # the B searches and their gathers: one call
            self._match_into([(src_keypts[b], tgt_keypts[b], src_features[b], tgt_features[b]) for b in range(B)], seeds,
                             src_corr, tgt_corr)
        pred_trans = self.SC2_PCR(src_corr, tgt_corr)
        if n <= self.max_points:                                                 # made by the registration call itself
            return pred_trans, self._labels, src_corr, tgt_corr
        labels = torch.empty((B, n), dtype=torch.float32, device=dev)
        for b in range(B):                                                       # Matcher.estimator's own expression, per pair
            T, sc, tc = pred_trans[b:b + 1], src_corr[b:b + 1], tgt_corr[b:b + 1]
            warped = sc @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]
            labels[b] = (torch.sum((warped - tc) ** 2, dim=-1) ** 0.5 < self.inlier_threshold).float()[0]
        return pred_trans, labels, src_corr, tgt_corr
