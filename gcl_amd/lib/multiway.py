"""Multiway registration on the MI355X kernels (csrc/multiway.hip, csrc/posegraph.h): the ground-truth poses of a frame's
neighbourhood as the complement pair loaders make them (lib/complement_data_loader.py:407-516 and its nuScenes twin) -- an
ICP for every pair of the clouds on a side, open3d's ``get_information_matrix_from_point_clouds`` for every pair, a pose graph
of odometry edges and uncertain loop closures, and open3d's ``global_optimization`` (Levenberg-Marquardt with a line process,
edges pruned at 0.25).

The semantics are RESTATED from open3d's published source (open3d is not a dependency) in DESIGN.md "Multiway registration"
and in numpy in tests/multiway_oracle.py.  Everything is fp64 on the device.  Results stay on the device unless stated, no
call in the chain waits for the host, and a pair's matrix and a graph's result are bitwise the same alone, anywhere in a batch
and on every run.
"""
import ctypes

import numpy as np
import torch

from gcl_amd import _lib
from gcl_amd.lib.eval import host_to_device
from gcl_amd.lib.fpfh import _offsets_host, _points
from gcl_amd.lib.icp import _distance, registration_icp_batch, voxelise_clouds

MAX_NODES, MAX_EDGES = 8, 28          # PG_MAX_NODES, PG_MAX_EDGES
DEFAULT_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                        min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0,
                        lower_scale_factor=1.0 / 3.0)          # open3d's GlobalOptimizationConvergenceCriteria


# ---- information matrices -----------------------------------------------------------------------------------------------
def information_matrix_batch(xyz0, offsets0, xyz1, offsets1, max_correspondence_distance, transformation):
    """open3d's ``get_information_matrix_from_point_clouds`` for B pairs in the layout of ``registration_icp_batch``.
    ``transformation``: [B, 4, 4] (host array or device tensor).  Returns device float64 [B, 6, 6] (rotation part first);
    ``[:, 5, 5]`` is the number of correspondences.  The target's grid is built here, at this distance."""
    xyz0, xyz1 = _points(xyz0, "xyz0"), _points(xyz1, "xyz1")
    d = _distance(max_correspondence_distance)
    off0, off1 = _offsets_host(offsets0, xyz0.shape[0]), _offsets_host(offsets1, xyz1.shape[0])
    if off0.size != off1.size:
        raise ValueError(f"{off0.size - 1} sources but {off1.size - 1} targets")
    B = off0.size - 1
    if xyz0.device != xyz1.device:
        raise ValueError(f"xyz0 on {xyz0.device} but xyz1 on {xyz1.device}")
    dev = xyz0.device
    if torch.is_tensor(transformation):
        T = transformation.detach().to(torch.float64)
        if tuple(T.shape) == (4, 4):
            T = T[None]
        if tuple(T.shape) != (B, 4, 4):
            raise ValueError(f"transformation must be [B, 4, 4] with B = {B}, got {tuple(T.shape)}")
        T = T.reshape(B, 16).contiguous().to(dev)
    else:
        T = np.asarray(transformation, dtype=np.float64)
        if T.shape == (4, 4):
            T = T[None]
        if T.shape != (B, 4, 4) or not np.isfinite(T).all():
            raise ValueError(f"transformation must be finite [B, 4, 4] with B = {B}, got {T.shape}")
        T = host_to_device(np.array(T.reshape(B, 16)), dev)               # a copy: the caller's array may be read-only
    lib = _lib.require_gpu()
    n0, n1 = xyz0.shape[0], xyz1.shape[0]
    off_dev = host_to_device(np.concatenate([off0, off1]), dev)
    off0_dev, off1_dev = off_dev[:B + 1], off_dev[B + 1:]
    skeys = order = None
    if n1:
        keys = torch.empty(n1, dtype=torch.int64, device=dev)
        _lib.check(lib.gcl_fpfh_cell_keys(_lib.ptr(xyz1), n1, _lib.ptr(off1_dev), B, d, _lib.ptr(keys), _lib.stream()),
                   "gcl_fpfh_cell_keys")
        skeys, order = torch.sort(keys)              # plumbing, as in registration_icp_batch
    info = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    scratch = torch.empty(max(lib.gcl_info_scratch_bytes(n0, n1, B), 1), dtype=torch.uint8, device=dev)
    i64p = ctypes.POINTER(ctypes.c_int64)
    _lib.check(lib.gcl_info_matrix_batch(_lib.ptr(xyz0) if n0 else None, off0.ctypes.data_as(i64p), _lib.ptr(off0_dev),
                                         _lib.ptr(xyz1) if n1 else None, off1.ctypes.data_as(i64p), _lib.ptr(off1_dev), B,
                                         _lib.ptr(skeys), _lib.ptr(order), _lib.ptr(T), d, _lib.ptr(scratch), _lib.ptr(info),
                                         _lib.stream()), "gcl_info_matrix_batch")
    return info


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """The one-pair form: device float64 [6, 6]."""
    return information_matrix_batch(source, None, target, None, max_correspondence_distance, transformation)[0]


# ---- pose graphs --------------------------------------------------------------------------------------------------------------
class GlobalOptimizationResult:
    """Device tensors of a batch of optimised graphs: ``poses`` float64 [total_nodes, 4, 4], ``confidence`` float64
    [total_edges] (the line process of the last pass an edge took part in), ``kept`` int32 [total_edges], ``stats`` float64
    [G, 3] (linear solves of pass 1, of pass 2, the final residual) and ``status`` int32 [G] (0; 1: no edge carries a
    correspondence; 2: a non-finite input; 3: the solver broke down; 1 .. 3 return the input poses with every edge kept).
    ``node_offsets`` / ``edge_offsets`` are the host offsets of the graphs."""

    def __init__(self, poses, confidence, kept, stats, status, node_offsets, edge_offsets):
        self.poses, self.confidence, self.kept, self.stats, self.status = poses, confidence, kept, stats, status
        self.node_offsets, self.edge_offsets = node_offsets, edge_offsets


def check_structure(node_counts, edge_lists, reference_node=0):
    """Raises ValueError unless every graph has 1 .. 8 nodes, at most 28 edges (s, t) with 0 <= s < t < n, and the odometry
    edge i -> i + 1 for every i.  Host integers only: nothing is launched."""
    if len(node_counts) != len(edge_lists) or not len(node_counts):
        raise ValueError("one edge list per graph and at least one graph")
    for g, (n, edges) in enumerate(zip(node_counts, edge_lists)):
        n = int(n)
        if not 1 <= n <= MAX_NODES:
            raise ValueError(f"graph {g}: {n} nodes, not in 1 .. {MAX_NODES}")
        if len(edges) > MAX_EDGES:
            raise ValueError(f"graph {g}: {len(edges)} edges, above {MAX_EDGES}")
        if not 0 <= int(reference_node) < n:
            raise ValueError(f"graph {g}: reference node {reference_node} not in 0 .. {n - 1}")
        seen = set()
        for s, t in edges:
            s, t = int(s), int(t)
            if not (0 <= s < n and 0 <= t < n):
                raise ValueError(f"graph {g}: edge ({s}, {t}) names a node outside 0 .. {n - 1}")
            if s >= t:
                raise ValueError(f"graph {g}: edge ({s}, {t}) must have source < target")
            seen.add((s, t))
        for i in range(n - 1):
            if (i, i + 1) not in seen:
                raise ValueError(f"graph {g}: the odometry edge {i} -> {i + 1} is missing")


def _params(max_correspondence_distance, edge_prune_threshold, preference_loop_closure, reference_node, criteria):
    c = dict(DEFAULT_CRITERIA)
    for k, v in (criteria or {}).items():
        if k not in c:
            raise ValueError(f"unknown convergence criterion {k!r}")
        c[k] = v
    if int(c["max_iteration"]) != c["max_iteration"] or not 0 <= c["max_iteration"] <= 1000:
        raise ValueError("max_iteration must be an integer in 0 .. 1000")
    if int(c["max_iteration_lm"]) != c["max_iteration_lm"] or not 1 <= c["max_iteration_lm"] <= 100:
        raise ValueError("max_iteration_lm must be an integer in 1 .. 100")
    p = [_distance(max_correspondence_distance), float(edge_prune_threshold), float(preference_loop_closure), int(reference_node),
         int(c["max_iteration"]), c["min_relative_increment"], c["min_relative_residual_increment"], c["min_right_term"],
         c["min_residual"], int(c["max_iteration_lm"]), c["upper_scale_factor"], c["lower_scale_factor"]]
    p = np.array(p, dtype=np.float64)
    if not np.isfinite(p).all():
        raise ValueError("the optimisation's parameters must be finite")
    return p


def _optimize(nodes, node_off, edges, edge_off, edge_T, edge_info, uncertain, G, total_nodes, total_edges, params):
    """The launch on device tensors; the structure has been validated."""
    lib = _lib.require_gpu()
    dev = nodes.device
    poses = torch.empty((total_nodes, 4, 4), dtype=torch.float64, device=dev)
    confidence = torch.empty(total_edges, dtype=torch.float64, device=dev)
    kept = torch.empty(total_edges, dtype=torch.int32, device=dev)
    stats = torch.empty((G, 3), dtype=torch.float64, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    e = lambda t: _lib.ptr(t) if total_edges else None
    _lib.check(lib.gcl_posegraph_optimize_batch(_lib.ptr(nodes), _lib.ptr(node_off), e(edges), _lib.ptr(edge_off), e(edge_T),
                                                e(edge_info), e(uncertain), G, total_nodes, total_edges,
                                                params.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.ptr(poses),
                                                e(confidence), e(kept), _lib.ptr(stats), _lib.ptr(status), _lib.stream()),
               "gcl_posegraph_optimize_batch")
    return poses, confidence, kept, stats, status


def _f64(t, shape, name, dev):
    """``t`` (device tensor or host array) as a contiguous device float64 [shape[0], prod(shape[1:])]."""
    if not torch.is_tensor(t):
        t = host_to_device(np.ascontiguousarray(t, dtype=np.float64), dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return t.detach().to(torch.float64).reshape(shape[0], -1).contiguous()


def global_optimization_batch(nodes, edges, edge_transformation, edge_information, uncertain, node_offsets=None,
                              edge_offsets=None, max_correspondence_distance=0.075, edge_prune_threshold=0.25,
                              preference_loop_closure=1.0, reference_node=0, criteria=None):
    """open3d's ``global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option)`` for a batch of
    graphs as flat arrays.  ``nodes`` [total_nodes, 4, 4], ``edge_transformation`` [total_edges, 4, 4] and
    ``edge_information`` [total_edges, 6, 6] are device tensors (or host arrays, copied); ``edges`` [total_edges, 2] (source,
    target, counted within the graph), ``uncertain`` [total_edges], ``node_offsets`` / ``edge_offsets`` [G + 1] (None: one
    graph) are HOST integers and are validated before anything is launched: a ``ValueError`` names what is wrong.  ``criteria``
    overrides entries of ``DEFAULT_CRITERIA``.  Returns a ``GlobalOptimizationResult``; nothing is read back."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    u = np.asarray(uncertain).reshape(-1)
    total_edges = len(e)
    if len(u) != total_edges:
        raise ValueError(f"{total_edges} edges but {len(u)} uncertain flags")
    total_nodes = int(nodes.shape[0])
    n_off = _offsets_host(node_offsets, total_nodes)
    e_off = np.array([0, total_edges], dtype=np.int64) if edge_offsets is None else np.asarray(edge_offsets, dtype=np.int64)
    if e_off.ndim != 1 or e_off.size != n_off.size or e_off[0] != 0 or e_off[-1] != total_edges or (np.diff(e_off) < 0).any():
        raise ValueError(f"edge_offsets must ascend from 0 to {total_edges} over {n_off.size - 1} graphs")
    G = n_off.size - 1
    check_structure(np.diff(n_off), [e[e_off[g]:e_off[g + 1]] for g in range(G)], reference_node)
    params = _params(max_correspondence_distance, edge_prune_threshold, preference_loop_closure, reference_node, criteria)
    _lib.require_gpu()
    dev = nodes.device if torch.is_tensor(nodes) else torch.device("cuda", torch.cuda.current_device())
    nodes = _f64(nodes, (total_nodes, 4, 4), "nodes", dev)
    edge_T = _f64(edge_transformation, (total_edges, 4, 4), "edge_transformation", dev)
    edge_info = _f64(edge_information, (total_edges, 6, 6), "edge_information", dev)
    ints = np.concatenate([n_off, e_off, e.reshape(-1), u.astype(bool).astype(np.int64)]).astype(np.int32)
    ints = host_to_device(ints, dev)
    node_off, edge_off = ints[:G + 1], ints[G + 1:2 * G + 2]
    edges_dev, unc = ints[2 * G + 2:2 * G + 2 + 2 * total_edges], ints[2 * G + 2 + 2 * total_edges:]
    out = _optimize(nodes, node_off, edges_dev, edge_off, edge_T, edge_info, unc, G, total_nodes, total_edges, params)
    return GlobalOptimizationResult(*out, n_off, e_off)


class FullRegistrationResult(GlobalOptimizationResult):
    """A ``GlobalOptimizationResult`` with the chain's intermediates: ``icp`` (the ``BatchICPResult`` of all pairs),
    ``information`` float64 [total_edges, 6, 6] and ``nodes`` float64 [total_nodes, 4, 4] (the composed start)."""


def full_registration_batch(graphs, max_distance=0.2, info_distance=0.075, max_iteration=200):
    """The reference's ``full_registration`` for a batch of graphs.  Each graph is ``{"clouds": n device [N_i, 3] tensors,
    "init": float64 [n, n, 4, 4] (host)}``, the entries ``s < t`` being the reference's ``M`` of that pair (cloud s moved into
    cloud t's frame).  All pairs of all graphs go through ONE ``registration_icp_batch`` from ``init``, one grid build and
    one information launch set at ``info_distance``; a set-up kernel composes the graphs (node k = the inverse of the chained
    consecutive ICPs; consecutive pairs certain, the others uncertain) and one launch optimises them (prune threshold 0.25,
    reference node 0, ``max_correspondence_distance = info_distance``).  Nothing is read back."""
    if not len(graphs):
        raise ValueError("at least one graph")
    src, tgt, inits, counts = [], [], [], []
    for g, gr in enumerate(graphs):
        clouds = [_points(c, f"graph {g} cloud {i}") for i, c in enumerate(gr["clouds"])]
        n = len(clouds)
        if not 1 <= n <= MAX_NODES:
            raise ValueError(f"graph {g}: {n} clouds, not in 1 .. {MAX_NODES}")
        init = np.asarray(gr["init"], dtype=np.float64)
        if init.shape != (n, n, 4, 4):
            raise ValueError(f"graph {g}: init must be [{n}, {n}, 4, 4], got {init.shape}")
        for s in range(n):
            for t in range(s + 1, n):
                src.append(clouds[s])
                tgt.append(clouds[t])
                inits.append(init[s, t])
        counts.append(n)
    pairs = len(src)
    if pairs == 0:
        raise ValueError("no graph has two clouds: nothing to register")
    if not np.isfinite(np.stack(inits)).all():
        raise ValueError("init must be finite")
    d_info = _distance(info_distance)
    params = _params(d_info, 0.25, 1.0, 0, None)
    n_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    e_off = np.concatenate([[0], np.cumsum([n * (n - 1) // 2 for n in counts])]).astype(np.int64)
    off0 = np.concatenate([[0], np.cumsum([len(c) for c in src])]).astype(np.int64)
    off1 = np.concatenate([[0], np.cumsum([len(c) for c in tgt])]).astype(np.int64)
    xyz0, xyz1 = torch.cat(src), torch.cat(tgt)
    icp = registration_icp_batch(xyz0, off0, xyz1, off1, max_distance, np.stack(inits), max_iteration)
    info = information_matrix_batch(xyz0, off0, xyz1, off1, d_info, icp.transformation)
    lib = _lib.require_gpu()
    dev = xyz0.device
    G, total_nodes, total_edges = len(counts), int(n_off[-1]), int(e_off[-1])
    offs = host_to_device(np.concatenate([n_off, e_off]).astype(np.int32), dev)
    node_off, edge_off = offs[:G + 1], offs[G + 1:]
    nodes = torch.empty((total_nodes, 16), dtype=torch.float64, device=dev)
    edges = torch.empty((total_edges, 2), dtype=torch.int32, device=dev)
    unc = torch.empty(total_edges, dtype=torch.int32, device=dev)
    edge_T = icp.transformation.reshape(total_edges, 16)
    _lib.check(lib.gcl_multiway_compose(_lib.ptr(node_off), _lib.ptr(edge_off), G, total_nodes, total_edges, _lib.ptr(edge_T),
                                        _lib.ptr(nodes), _lib.ptr(edges), _lib.ptr(unc), _lib.stream()), "gcl_multiway_compose")
    out = _optimize(nodes, node_off, edges, edge_off, edge_T, info.reshape(total_edges, 36), unc, G, total_nodes, total_edges,
                    params)
    r = FullRegistrationResult(*out, n_off, e_off)
    r.icp, r.information, r.nodes = icp, info, nodes.reshape(total_nodes, 4, 4)
    return r


def _pair_init(velo2cam, pos_s, pos_t):
    """lib/complement_data_loader.py:410-411."""
    return (velo2cam @ pos_s.T @ np.linalg.inv(pos_t.T) @ np.linalg.inv(velo2cam)).T


def multiway_registration(xyz_curr, xyz_cmpls, pos_curr, pos_cmpls, velo2cam, num_complement_one_side, icp_voxel_size=0.05):
    """The loaders' ``multiway_registration`` without its file cache.  ``xyz_curr``: the raw centre scan, float32 [P, 3] host
    array; ``xyz_cmpls``: the ``2 * num_complement_one_side`` raw neighbour scans, left side first; ``pos_curr`` /
    ``pos_cmpls``: their 4 x 4 poses; ``velo2cam``: 4 x 4.  One voxeliser pass downsamples every scan (the centre once, shared
    by both sides), ``init`` is the reference's formula in host numpy, and both sides run as two graphs of one
    ``full_registration_batch``.  Returns the list ``inv(P_0) @ P_i`` of the left side, then of the right side: host float64
    4 x 4 matrices.  Host reads: the voxeliser's counts, then the poses.

    A list of samples (every argument but ``velo2cam``, ``num_complement_one_side`` and ``icp_voxel_size`` a list of equal
    length) gives a batch -- as many samples as the voxeliser's 64-cloud table holds -- and a list of such lists comes back."""
    k = int(num_complement_one_side)
    if not 1 <= k < MAX_NODES:
        raise ValueError(f"num_complement_one_side must be in 1 .. {MAX_NODES - 1}, got {num_complement_one_side}")
    batched = isinstance(xyz_curr, (list, tuple))
    samples = list(zip(xyz_curr, xyz_cmpls, pos_curr, pos_cmpls)) if batched else [(xyz_curr, xyz_cmpls, pos_curr, pos_cmpls)]
    if not 1 <= len(samples) <= 64 // (1 + 2 * k):
        raise ValueError(f"1 .. {64 // (1 + 2 * k)} samples per call (64 clouds share the voxeliser's table)")
    voxel = float(icp_voxel_size)
    if not (0.0 < voxel < 3.0e38):
        raise ValueError(f"icp_voxel_size must be positive and finite, got {voxel}")
    velo2cam = np.asarray(velo2cam, dtype=np.float64)
    if velo2cam.shape != (4, 4) or not np.isfinite(velo2cam).all():
        raise ValueError("velo2cam must be a finite 4 x 4 matrix")
    raw, inits = [], []
    for xc, xs, pc, ps in samples:
        if len(xs) != 2 * k or len(ps) != 2 * k:
            raise ValueError(f"{2 * k} complement scans and poses a sample, got {len(xs)} and {len(ps)}")
        for x in [xc] + list(xs):
            x = np.asarray(x, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != 3:
                raise ValueError(f"a scan must be [P, 3], got {x.shape}")
            raw.append(x)
        poses = [np.asarray(p, dtype=np.float64) for p in [pc] + list(ps)]
        if any(p.shape != (4, 4) or not np.isfinite(p).all() for p in poses):
            raise ValueError("poses must be finite 4 x 4 matrices")
        for side in (poses[:1] + poses[1:1 + k], poses[:1] + poses[1 + k:]):
            init = np.tile(np.eye(4), (k + 1, k + 1, 1, 1))
            for s in range(k + 1):
                for t in range(s + 1, k + 1):
                    init[s, t] = _pair_init(velo2cam, side[s], side[t])
            inits.append(init)
    xyz, starts = voxelise_clouds(raw, voxel)                                # host read 1: the row counts
    graphs = []
    for i in range(len(samples)):
        c = [xyz[starts[(1 + 2 * k) * i + j]:starts[(1 + 2 * k) * i + j + 1]] for j in range(1 + 2 * k)]
        graphs.append({"clouds": c[:1] + c[1:1 + k], "init": inits[2 * i]})
        graphs.append({"clouds": c[:1] + c[1 + k:], "init": inits[2 * i + 1]})
    P = full_registration_batch(graphs).poses.cpu().numpy()                  # host read 2: the poses
    out = []
    for i in range(len(samples)):
        Ms = []
        for side in (2 * i, 2 * i + 1):
            Q = P[(k + 1) * side:(k + 1) * (side + 1)]
            Ms += [np.linalg.inv(Q[0]) @ Q[j] for j in range(1, k + 1)]
        out.append(Ms)
    return out if batched else out[0]
