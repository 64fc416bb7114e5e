"""Feature-match recall of a scene of fragments (interface of generalization_ETH/evaluate.py), device-resident.

The reference's functions keep their names and meaning; what they do off the GPU or through third parties runs here in
HIP kernels (csrc/match.hip, csrc/loss.hip):

  find_nearest_voxel_feature  :110-122  pytorch3d knn_points, K = 1       -> gcl_nn3_rowmin (+ the row gather, same call)
  calculate_M                 :63-77    two sklearn KDTrees, Python loop  -> 2 x gcl_nn_rowmin + gcl_mutual_match
  inlier ratio under gtTrans  :160-169  numpy on the host                 -> gcl_mutual_match (same launch)
  scene loop                  :263-284  the network twice per PAIR        -> once per FRAGMENT, results read once per scene

No file formats are read here (PLY fragments, keypoint index files: dataset I/O): the inputs are
arrays.  Points and keypoints are searched in fp32 (the reference hands pytorch3d the float64 arrays of open3d); the
distance is evaluated in the difference form, good to a few 2^-24 relative at any offset from the origin.
"""
import ctypes
import os

import numpy as np
import torch

import gcl_amd.MinkowskiEngine as ME
from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device
from gcl_amd.lib.metrics import mutual_jobs, nn3_min, pdist_min, pdist_min_batch

DESC_WIDTHS = (16, 32, 64)      # what gcl_nn_rowmin searches


def loadlog(gtpath):
    """``gt.log`` of a scene as {'i_j': 4x4 float64} (generalization_ETH/evaluate.py:46-61)."""
    with open(os.path.join(gtpath, "gt.log")) as f:
        content = f.readlines()
    result = {}
    i = 0
    while i < len(content):
        line = content[i].replace("\n", "").split("\t")[0:3]
        trans = np.zeros([4, 4])
        for r in range(4):
            trans[r] = [float(x) for x in content[i + 1 + r].replace("\n", "").split("\t")[0:4]]
        i = i + 5
        result[f"{int(line[0])}_{int(line[1])}"] = trans
    return result


def fragment_input(xyz, voxel_size, device):
    """One cloud's half of ``prepare_pcd_to_input`` (:80-107): ``(sinput, xyz_th)`` -- the voxelised cloud as a
    SparseTensor of ones on ``device`` and the kept points (first point of every voxel, host tensor, input dtype)."""
    xyz = torch.as_tensor(np.asarray(xyz) if not isinstance(xyz, torch.Tensor) else xyz).cpu()
    _, sel = ME.utils.sparse_quantize(xyz / voxel_size, return_index=True)
    xyz_th = xyz[sel]
    coords = torch.floor(xyz_th / voxel_size)
    feats = torch.ones((len(coords), 1))
    coords_batch, feats_batch = ME.utils.sparse_collate([coords], [feats])
    sinput = ME.SparseTensor(feats_batch.to(device), coordinates=coords_batch.to(device))
    return sinput, xyz_th


def prepare_pcd_to_input(xyz_0, xyz_1, voxel_size, device):
    """:80-107 with the reference's two globals as arguments: ``(sinput0, sinput1, xyz_0_th, xyz_1_th)``."""
    sinput0, xyz_0_th = fragment_input(xyz_0, voxel_size, device)
    sinput1, xyz_1_th = fragment_input(xyz_1, voxel_size, device)
    return sinput0, sinput1, xyz_0_th, xyz_1_th


def _points(x, device):
    """float32 [n, 3] on ``device`` from an array or tensor of any float dtype (small host arrays: pinned, non-blocking)."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.to(torch.float32).contiguous()
    arr = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    return host_to_device(arr, device)


def _current_device():
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def find_nearest_voxel_feature(full, partial, features):
    """``features[nn]`` with nn = the nearest point of ``full`` [n, 3] for every point of ``partial`` [m, 3] (:110-122);
    search and row gather are one native call.  Ties go to the lowest index."""
    dev = features.device
    return nn3_min(_points(partial, dev), _points(full, dev), features)[2]


def _check_width(c):
    if c not in DESC_WIDTHS:
        raise ValueError(f"descriptor width must be 16, 32 or 64 (the limit of gcl_nn_rowmin), got {c}")


def _as_desc(x, device):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.detach().to(torch.float32).contiguous()
    return _points(x, device)


class FragmentMatch:
    """What ``match_fragments`` enqueued for one pair; everything stays on the device until ``result()`` is called.
    ``pairs`` int32 [m0, 2] (the first ``stats[0]`` rows are the mutual pairs, ascending in the source index),
    ``stats`` int32 [2] = (mutual pairs, inliers), ``nn01`` / ``nn10`` the two arg-minima."""

    def __init__(self, pairs, stats, nn01, nn10):
        self.pairs, self.stats, self.nn01, self.nn10 = pairs, stats, nn01, nn10

    def result(self):
        """(pairs int64 [K, 2] on the device, number of inliers): ONE read of the two counters."""
        k, inl = self.stats.tolist()
        return self.pairs[:k].long(), inl


def _mutual(nn01, nn10, kp_s, kp_t, T, tau, out):
    lib = _lib.require_gpu()
    m0, m1 = nn01.shape[0], nn10.shape[0]
    dev = nn01.device
    pairs = torch.empty((m0, 2), dtype=torch.int32, device=dev)
    stats = out if out is not None else torch.empty(2, dtype=torch.int32, device=dev)
    if stats.dtype != torch.int32 or stats.numel() != 2:
        raise ValueError("match_fragments: out must be an int32 tensor of two elements")
    _lib.check(lib.gcl_mutual_match(_lib.ptr(nn01, torch.int32), m0, _lib.ptr(nn10, torch.int32), m1,
                                    _lib.ptr(kp_s, torch.float32), _lib.ptr(kp_t, torch.float32),
                                    _lib.ptr(T, torch.float32), float(tau), _lib.ptr(pairs), _lib.ptr(stats),
                                    _lib.stream()), "gcl_mutual_match")
    return FragmentMatch(pairs, stats, nn01, nn10)


def calculate_M(source_desc, target_desc):
    """The mutually closest pairs in feature space (:63-77): int64 [K, 2] on the device, ascending in the source index.
    Nearest neighbours are exact fp32 searches with ties to the lowest index (a KD-tree's tie order is unspecified)."""
    dev = source_desc.device if isinstance(source_desc, torch.Tensor) and source_desc.is_cuda else _current_device()
    s, t = _as_desc(source_desc, dev), _as_desc(target_desc, dev)
    _check_width(s.shape[1])
    if t.shape[1] != s.shape[1]:
        raise ValueError(f"descriptor widths differ: {s.shape[1]} and {t.shape[1]}")
    if s.shape[0] == 0 or t.shape[0] == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=dev)
    _, nn01 = pdist_min(s, t, "SquareL2")
    _, nn10 = pdist_min(t, s, "SquareL2")
    return _mutual(nn01, nn10, None, None, None, 0.0, None).result()[0]


def fragment_descriptors(model, xyz, keypts, voxel_size):
    """Descriptors of one fragment's keypoints (:138-145 for one cloud): ONE forward pass over the voxelised fragment and
    ONE 3-D nearest-voxel search that also gathers the rows.  float32 [len(keypts), n_out] on the model's device."""
    if model.training:
        raise RuntimeError("fragment_descriptors needs model.eval() (the reference evaluates with running statistics)")
    dev = next(model.parameters()).device
    with torch.cuda.device(dev), torch.no_grad():
        sinput, voxels = fragment_input(xyz, voxel_size, dev)
        F = model(sinput).F.detach()
        return find_nearest_voxel_feature(voxels, keypts, F)


def _transform12(gtTrans, device):
    """float32 [12] = rows of [R | t] on ``device`` from a [4, 4] / [3, 4] array or tensor."""
    if gtTrans is None:
        return None
    if isinstance(gtTrans, torch.Tensor) and gtTrans.is_cuda:
        return gtTrans.reshape(-1)[:12].to(torch.float32).contiguous()
    T = np.asarray(gtTrans.numpy() if isinstance(gtTrans, torch.Tensor) else gtTrans, dtype=np.float64)
    return host_to_device(np.ascontiguousarray(T.reshape(-1)[:12], dtype=np.float32), device)


def match_fragments(kp_s, kp_t, desc_s, desc_t, gtTrans, tau1=0.1, out=None):
    """Enqueue one pair's matching (:158-169): the two feature-space 1-NN searches and the mutual filter with the count of
    mutual pairs whose keypoints lie within ``tau1`` once the TARGET keypoints are moved by ``gtTrans`` (None: no count).
    ``out``: an int32 [2] device tensor (a row of a scene's table) that receives (mutual pairs, inliers).
    Returns a ``FragmentMatch``; nothing is read back."""
    dev = desc_s.device
    _check_width(desc_s.shape[1])
    if desc_t.shape[1] != desc_s.shape[1]:
        raise ValueError(f"descriptor widths differ: {desc_s.shape[1]} and {desc_t.shape[1]}")
    kp_s, kp_t = _points(kp_s, dev), _points(kp_t, dev)
    if kp_s.shape[0] != desc_s.shape[0] or kp_t.shape[0] != desc_t.shape[0]:
        raise ValueError("match_fragments: one descriptor row per keypoint is required")
    if desc_s.shape[0] == 0 or desc_t.shape[0] == 0:
        raise ValueError("match_fragments: a fragment without keypoints")
    _, nn01 = pdist_min(desc_s, desc_t, "SquareL2")
    _, nn10 = pdist_min(desc_t, desc_s, "SquareL2")
    return _mutual(nn01, nn10, kp_s, kp_t, _transform12(gtTrans, dev), tau1, out)


def match_fragments_batch(jobs, tau1=0.1, outs=None):
    """``match_fragments`` for a list of pairs ``(kp_s, kp_t, desc_s, desc_t, gtTrans)`` in a fixed number of launches: both
    directions of every pair are the searches of ONE ``pdist_min_batch``, the mutual filters ONE ``gcl_mutual_match_batch``
    (one workgroup per pair).  ``outs``: per pair the int32 [2] tensor that receives (mutual pairs, inliers) -- rows of a
    scene's table.  Same refusals, and per pair the same ``FragmentMatch``, bit for bit."""
    lib = _lib.require_gpu()
    P = len(jobs)
    if P < 1:
        raise ValueError("match_fragments_batch needs at least one pair")
    if outs is not None and len(outs) != P:
        raise ValueError(f"{P} pairs but {len(outs)} outputs")
    dev = jobs[0][2].device
    checked = []
    for kp_s, kp_t, desc_s, desc_t, gtTrans in jobs:
        _check_width(desc_s.shape[1])
        if desc_t.shape[1] != desc_s.shape[1]:
            raise ValueError(f"descriptor widths differ: {desc_s.shape[1]} and {desc_t.shape[1]}")
        kp_s, kp_t = _points(kp_s, dev), _points(kp_t, dev)
        if kp_s.shape[0] != desc_s.shape[0] or kp_t.shape[0] != desc_t.shape[0]:
            raise ValueError("match_fragments: one descriptor row per keypoint is required")
        if desc_s.shape[0] == 0 or desc_t.shape[0] == 0:
            raise ValueError("match_fragments: a fragment without keypoints")
        checked.append((kp_s, kp_t, desc_s, desc_t, _transform12(gtTrans, dev)))
    nn = pdist_min_batch([(j[2], j[3]) for j in checked] + [(j[3], j[2]) for j in checked], "SquareL2")
    pairs = torch.empty((sum(j[2].shape[0] for j in checked), 2), dtype=torch.int32, device=dev)
    stats = outs if outs is not None else list(torch.empty((P, 2), dtype=torch.int32, device=dev))
    table, result, at = [], [], 0
    for k, (kp_s, kp_t, desc_s, desc_t, T) in enumerate(checked):
        if stats[k].dtype != torch.int32 or stats[k].numel() != 2:
            raise ValueError("match_fragments: out must be an int32 tensor of two elements")
        m0, m1 = desc_s.shape[0], desc_t.shape[0]
        table.append(dict(nn01=nn[k][1], nn10=nn[P + k][1], xyz0=kp_s, xyz1=kp_t, T=T, pairs=pairs[at:at + m0], count=stats[k],
                          m0=m0, m1=m1))
        result.append(FragmentMatch(pairs[at:at + m0], stats[k], nn[k][1], nn[P + k][1]))
        at += m0
    recs, jobs_dev = mutual_jobs(table, dev)
    _lib.check(lib.gcl_mutual_match_batch(ctypes.addressof(recs), _lib.ptr(jobs_dev), P, float(tau1), _lib.stream()),
               "gcl_mutual_match_batch")
    return result


def scene_summary(table, tau2=0.05):
    """The reference's aggregation (:270-282) of a per-pair table [P, 3] = (num_inliers, inlier_ratio, gt_flag)."""
    result = np.asarray(table, dtype=np.float64).reshape(-1, 3)
    gt_match = int(np.sum(result[:, 2] == 1))
    correct_match = int(np.sum(result[:, 1] > tau2))
    recall = float(correct_match / gt_match) * 100 if gt_match else float("nan")
    kept = np.sum(np.where(result[:, 1] > tau2, result[:, 0], np.zeros(result.shape[0])))
    ave_num_inliers = float(kept / correct_match) if correct_match else 0.0
    return dict(recall=recall, correct_match=correct_match, gt_match=gt_match, ave_num_inliers=ave_num_inliers)


def evaluate_scene(fragments, keypoints, gt_log, model=None, descriptors=None, voxel_size=0.05, tau1=0.1, tau2=0.05,
                   matcher=None, max_batch_bytes=1 << 30):
    """Feature-match recall of one scene (the loop of :258-284).

    ``fragments``: the clouds [N_i, 3] (unused when ``descriptors`` is given), ``keypoints``: [K_i, 3] per fragment,
    ``gt_log``: ``loadlog``'s dict.  Descriptors are computed ONCE per fragment (``fragment_descriptors``; the reference
    runs the network twice per pair) or taken from ``descriptors`` ([K_i, C] per fragment).  Every pair id1 < id2 named
    by ``gt_log`` is matched into one int32 [P, 2] table, which is read ONCE -- the pairs go in chunks whose search scratch
    stays within ``max_batch_bytes``, each chunk ONE ``match_fragments_batch`` (a chunk of one pair: ``match_fragments``); a
    pair the log does not name counts (0, 0, gt_flag 0), as in the reference.

    Returns ``recall`` (percent), ``correct_match``, ``gt_match``, ``ave_num_inliers`` and ``table`` float64 [P, 3] =
    (num_inliers, inlier_ratio, gt_flag) per pair in the loop's order, with the reference's arithmetic: the ratio goes
    through its 8-decimal text form (:198, :274), a pair is correct when ratio > ``tau2``.  Two divisions by zero of the
    reference are DEFINED here: a pair with zero mutual matches has ratio 0, and a scene with zero correct matches has
    ``ave_num_inliers`` 0.0 (a scene without any ground-truth pair has recall NaN, as numpy's 0 / 0 there).

    With a ``matcher`` every ground-truth pair is also registered on its keypoints and descriptors -- by open3d's
    feature-matching RANSAC as the reference does (:171-186) with ``gcl_amd.lib.ransac.FeatureRansac.eth()``, or by SC2-PCR
    with a ``Matcher`` (scripts/SC2_PCR.py) -- and ``pred_log`` holds
    ``(id1, id2, inverse of the estimate as 4x4 float64)`` in the reference's log order (:188-196); the estimates leave the
    device in one further copy.
    """
    n_frag = len(keypoints)
    if descriptors is None:
        if model is None:
            raise ValueError("evaluate_scene needs a model or precomputed descriptors")
        descriptors = [fragment_descriptors(model, fragments[i], keypoints[i], voxel_size) for i in range(n_frag)]
        dev = descriptors[0].device if n_frag else _current_device()
    else:
        if len(descriptors) != n_frag:
            raise ValueError("one descriptor array per fragment is required")
        first = descriptors[0] if n_frag else None
        dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda else _current_device()
        descriptors = [_as_desc(d, dev) for d in descriptors]
    with torch.cuda.device(dev):
        kps = [_points(k, dev) for k in keypoints]
        ids = [(a, b) for a in range(n_frag) for b in range(a + 1, n_frag)]
        gt_rows = [p for p, (a, b) in enumerate(ids) if f"{a}_{b}" in gt_log]
        counts = torch.zeros((max(1, len(ids)), 2), dtype=torch.int32, device=dev)
        T_all = None
        if gt_rows:       # every ground-truth transformation in one copy
            T_host = np.stack([np.asarray(gt_log["%d_%d" % ids[p]], dtype=np.float64).reshape(-1)[:12] for p in gt_rows])
            T_all = host_to_device(np.ascontiguousarray(T_host, dtype=np.float32), dev)
        estimates = []
        lib, g0 = _lib.require_gpu(), 0
        while g0 < len(gt_rows):                               # chunks of pairs under the scratch limit, at least one pair each
            g1, need = g0, 0
            while g1 < len(gt_rows):
                m0, m1 = (int(descriptors[i].shape[0]) for i in ids[gt_rows[g1]])
                need += 4 * (lib.gcl_nn_rowmin_scratch_len(m0, m1) + lib.gcl_nn_rowmin_scratch_len(m1, m0))
                if g1 > g0 and need > int(max_batch_bytes):
                    break
                g1 += 1
            chunk = [(g, gt_rows[g]) + ids[gt_rows[g]] for g in range(g0, g1)]
            if len(chunk) == 1:
                g, p, a, b = chunk[0]
                match_fragments(kps[a], kps[b], descriptors[a], descriptors[b], T_all[g], tau1, out=counts[p])
            else:
                match_fragments_batch([(kps[a], kps[b], descriptors[a], descriptors[b], T_all[g]) for g, p, a, b in chunk], tau1,
                                      outs=[counts[p] for g, p, a, b in chunk])
            if matcher is not None:
                for g, p, a, b in chunk:
                    T_est = matcher.estimator(kps[a][None], kps[b][None], descriptors[a][None], descriptors[b][None])[0]
                    estimates.append(T_est[0])
            g0 = g1
        counts_host = counts.cpu().numpy()                     # the scene's ONE read of the match counts
        T_est_host = torch.stack(estimates).cpu().numpy().astype(np.float64) if estimates else None
    table = np.zeros((len(ids), 3), dtype=np.float64)
    for p in gt_rows:
        n_mutual, n_inl = int(counts_host[p, 0]), int(counts_host[p, 1])
        ratio = n_inl / n_mutual if n_mutual else 0.0
        table[p] = (n_inl, float(f"{ratio:.8f}"), 1)
    out = scene_summary(table, tau2)
    out["table"] = table
    out["pairs"] = ids
    if matcher is not None:
        out["pred_log"] = [(ids[p][0], ids[p][1], np.linalg.inv(T_est_host[g])) for g, p in enumerate(gt_rows)]
    return out


def write_log(path, pred_log):
    """Append ``pred_log`` entries in the reference's text form (:188-196)."""
    with open(path, "a+") as f:
        for id1, id2, trans in pred_log:
            f.write(f"{id1}\t {id2}\t  37\n")
            for r in range(4):
                f.write(f"{trans[r, 0]}\t {trans[r, 1]}\t {trans[r, 2]}\t {trans[r, 3]}\t \n")
