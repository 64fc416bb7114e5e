"""numpy restatement of the correspondence set open3d's RANSAC registration runs on with ``mutual_filter=True``
(include/gcl_amd.h, gcl_mutual_correspondences), built on ``eth_eval_oracle.mutual``, and the feature constructions the
tests of the mutual filter use.

    M = [(i, nn01[i]) for ascending i if nn10[nn01[i]] == i]                       (eth_eval_oracle.mutual)
    |M| >= min_count:  rows xyz0[i_k] / xyz1[j_k], zero rows from |M| on, count = (|M|, |M|)
    otherwise:         rows xyz0[i] / xyz1[nn01[i]] for every source i, count = (m0, |M|)

The second branch is open3d's "too few correspondences after mutual filter, fall back to original correspondences" (written
from memory of its Registration.cpp: open3d is not available where the tests run); ``min_count`` is ``ransac_n`` there.  A
target index outside [0, m1) is never mutual; in the fall-back its target row is zero, as the header states.

A 1-NN is DECISIVE for the list when the rule reads it: every entry of nn01, and nn10 at the targets some source points to.
``tables`` returns, with the two tables, the smallest relative gap (second best - best) / second best of the squared
distances over the decisive searches: with a gap of 1e-3 an fp32 search (relative error ~ 1e-6 for these widths and
magnitudes) cannot decide differently from the fp64 one.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eth_eval_oracle as EO                                           # noqa: E402

WIDTH = 32


def correspondences(nn01, nn10, xyz0, xyz1, min_count):
    """(src float32 [m0, 3], tgt float32 [m0, 3], count int [2]) by the rule above."""
    nn01 = np.asarray(nn01, dtype=np.int64)
    xyz0, xyz1 = np.asarray(xyz0, dtype=np.float32), np.asarray(xyz1, dtype=np.float32)
    m0, m1 = len(nn01), len(nn10)
    pairs = EO.mutual(nn01, nn10)
    src, tgt = np.zeros((m0, 3), dtype=np.float32), np.zeros((m0, 3), dtype=np.float32)
    if len(pairs) >= min_count:
        src[:len(pairs)], tgt[:len(pairs)] = xyz0[pairs[:, 0]], xyz1[pairs[:, 1]]
        return src, tgt, np.array([len(pairs), len(pairs)])
    ok = (nn01 >= 0) & (nn01 < m1)
    src[:] = xyz0
    tgt[ok] = xyz1[nn01[ok]]
    return src, tgt, np.array([m0, len(pairs)])


def loop_list(nn01, nn10):
    """The mutual list by a plain loop, written without eth_eval_oracle (the check of the check)."""
    out = []
    for i, j in enumerate(nn01):
        if j < 0 or j >= len(nn10):
            continue
        if nn10[j] == i:
            out.append((i, int(j)))
    return out


def _rel_gap(D, rows):
    """Smallest (second - best) / second over the given rows of a squared-distance matrix with >= 2 columns."""
    part = np.partition(D[rows], 1, axis=1)
    return float(((part[:, 1] - part[:, 0]) / part[:, 1]).min())


def tables(F0, F1):
    """(nn01 int64 [m0], nn10 int64 [m1], smallest relative gap of the decisive searches) in fp64."""
    D = EO.sqdist_rows(F0, F1, np.arange(len(F0)))
    nn01, nn10 = D.argmin(1), D.argmin(0)
    gap = min(_rel_gap(D, np.arange(len(F0))), _rel_gap(D.T, np.unique(nn01)))
    return nn01, nn10, gap


def planted_features(seed, n=300):
    """F0 N(0, 1) [n, 32] and F1 with F1[perm] = F0 + N(0, 0.01): every source is mutual with its own copy.
    Returns (F0, F1, perm)."""
    rng = np.random.RandomState(seed)
    F0 = rng.normal(size=(n, WIDTH)).astype(np.float32)
    perm = rng.permutation(n)
    F1 = np.empty_like(F0)
    F1[perm] = F0 + rng.normal(scale=0.01, size=F0.shape).astype(np.float32)
    return F0, F1, perm


FUNNEL_M0, FUNNEL_M1, FUNNEL_SINK, FUNNEL_HALVED = 40, 50, 7, 3


def funnel_features(seed, e):
    """40 sources x 50 targets.  Sources N(0, 0.1), row FUNNEL_HALVED scaled by 0.5; targets of norm 100 except row
    FUNNEL_SINK = 0: every source's nearest target is the sink, whose nearest source is the halved one -- ONE mutual pair.
    ``e`` isolated matched pairs far away: source 39 - k and target 10 + k both at 1000 e_k.  |M| = 1 + e.
    Returns (F0, F1)."""
    rng = np.random.RandomState(seed)
    F0 = rng.normal(scale=0.1, size=(FUNNEL_M0, WIDTH)).astype(np.float32)
    F0[FUNNEL_HALVED] *= 0.5
    F1 = rng.normal(size=(FUNNEL_M1, WIDTH))
    F1 = (100.0 * F1 / np.linalg.norm(F1, axis=1, keepdims=True)).astype(np.float32)
    F1[FUNNEL_SINK] = 0.0
    for k in range(e):
        F0[FUNNEL_M0 - 1 - k] = 0.0
        F0[FUNNEL_M0 - 1 - k, k] = 1000.0
        F1[10 + k] = F0[FUNNEL_M0 - 1 - k]
    return F0, F1


def random_tables(seed, m0, m1):
    """Integer tables with many mutual pairs, many broken ones and out-of-range entries (-1 and m1) in nn01."""
    rng = np.random.RandomState(seed)
    nn01 = rng.randint(0, m1, m0)
    nn10 = rng.randint(0, m0, m1)
    for i in np.nonzero(rng.rand(m0) < 0.5)[0]:         # make about half of the sources mutual (later writes may break some)
        nn10[nn01[i]] = i
    bad = rng.rand(m0) < 0.15
    nn01[bad] = np.where(rng.rand(int(bad.sum())) < 0.5, -1, m1)
    return nn01.astype(np.int32), nn10.astype(np.int32)
