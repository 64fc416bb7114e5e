"""Feature-match recall: the HIP path beside what torch alone could do on the same box, in one process.

  nn3_min            5000 x 200 000 and 5000 x 1 000 000   vs  chunked torch.cdist(...).min(1), both compute modes
  match_fragments    5000 x 5000 x 32                      vs  one torch.cdist, two argmins, the mutual test, the count, .tolist()
  evaluate_scene     16 synthetic fragments, ResUNetFatBN  vs  the reference's loop shape: the network twice per PAIR, torch
                                                               nearest voxel, torch matching, one read per pair

Every figure: one warm run, then five repeats of enough calls to fill ~0.3 s each, timed with a host clock around a device
synchronise; the median and the minimum of the five are printed.  The torch nearest-voxel search is also checked against
the HIP result (share of queries with the same index, and whose point is nearer in fp64): torch.cdist's default mode uses
|q|^2 + |p|^2 - 2 q.p.

    python3 tools/micro/eth_eval_probe.py [--out FILE] [--fragments 16] [--frag-points 10000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from gcl_amd import synthetic
from gcl_amd.generalization_ETH import evaluate as E
from gcl_amd.lib.metrics import nn3_min
from gcl_amd.model import load_model

DEV = torch.device("cuda:0")
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn, repeats=5, window=0.3, max_iters=200):
    """(median, minimum) seconds per call over ``repeats`` windows of whole calls, after a warm run."""
    fn()
    torch.cuda.synchronize()
    iters = 1
    if max_iters > 1:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        iters = int(max(1, min(max_iters, window / max(time.perf_counter() - t0, 1e-6))))
    per_call = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / iters)
    return float(np.median(per_call)), float(np.min(per_call)), iters


def report(name, fn, **kw):
    med, low, iters = timed(fn, **kw)
    say(f"{name:<58s} median {med * 1e3:10.3f} ms   min {low * 1e3:10.3f} ms   ({iters} calls x 5)")
    return med


def torch_nn(Q, P, mode, chunk=16384):
    """Running (min, argmin) over chunks of P of torch.cdist: the [m, chunk] matrix stays under 330 MB at m = 5000."""
    best = torch.full((len(Q),), float("inf"), device=Q.device)
    arg = torch.zeros(len(Q), dtype=torch.int64, device=Q.device)
    for j0 in range(0, len(P), chunk):
        v, i = torch.cdist(Q, P[j0:j0 + chunk], compute_mode=mode).min(1)
        better = v < best
        best = torch.where(better, v, best)
        arg = torch.where(better, i + j0, arg)
    return best, arg


def torch_match(kp_s, kp_t, ds, dt, T, tau):
    D = torch.cdist(ds, dt)
    nn01, nn10 = D.argmin(1), D.argmin(0)
    src = torch.arange(len(ds), device=ds.device)
    keep = nn10[nn01] == src
    moved = kp_t[nn01] @ T[:3, :3].t() + T[:3, 3]
    inl = keep & (torch.sqrt(((kp_s - moved) ** 2).sum(1)) < tau)
    return torch.stack([keep.sum(), inl.sum()]).tolist()


def nn3_section():
    rng = np.random.RandomState(0)
    for n in (200_000, 1_000_000):
        # a 5 cm voxel surface cloud's scale: points over a 60 m x 60 m x 10 m block, away from the origin like a real scan
        P = torch.from_numpy((rng.uniform(0, 1, (n, 3)) * [60, 60, 10] + [100, -80, 0]).astype(np.float32)).to(DEV)
        Q = (P[torch.from_numpy(rng.randint(0, n, 5000)).to(DEV)] + 0.02).contiguous()
        F = torch.randn((n, 32), device=DEV)
        say(f"-- nearest voxel, 5000 x {n}")
        report("gcl_nn3_rowmin (nn3_min)", lambda: nn3_min(Q, P))
        report("gcl_nn3_rowmin + fused gather of 32 floats (nn3_min)", lambda: nn3_min(Q, P, F))
        report("torch.cdist chunks, default mode (mm expansion)", lambda: torch_nn(Q, P, "use_mm_for_euclid_dist_if_necessary"))
        report("torch.cdist chunks, donot_use_mm_for_euclid_dist", lambda: torch_nn(Q, P, "donot_use_mm_for_euclid_dist"))
        arg = nn3_min(Q, P)[1].long()
        d64 = lambda idx: ((Q.double() - P[idx].double()) ** 2).sum(1)
        for mode in ("use_mm_for_euclid_dist_if_necessary", "donot_use_mm_for_euclid_dist"):
            theirs = torch_nn(Q, P, mode)[1]
            same = (theirs == arg).float().mean().item()
            farther = (d64(theirs) > d64(arg)).float().mean().item()
            nearer = (d64(theirs) < d64(arg)).float().mean().item()
            say(f"   torch {mode}: same index as the HIP search for {100 * same:.2f} % of the queries; its point is "
                f"farther (fp64) for {100 * farther:.2f} %, nearer for {100 * nearer:.2f} %")
        del P, Q, F


def match_section():
    rng = np.random.RandomState(1)
    ds = torch.nn.functional.normalize(torch.randn((5000, 32), device=DEV), dim=1)
    dt = ds[torch.randperm(5000, device=DEV)] + 0.05 * torch.randn((5000, 32), device=DEV)
    dt = torch.nn.functional.normalize(dt, dim=1).contiguous()
    kp_s = torch.from_numpy(rng.uniform(-20, 20, (5000, 3)).astype(np.float32)).to(DEV)
    kp_t = torch.from_numpy(rng.uniform(-20, 20, (5000, 3)).astype(np.float32)).to(DEV)
    T = torch.eye(4, device=DEV)
    say("-- one pair, 5000 x 5000 keypoints, 32-wide descriptors (both end with the two counters on the host)")
    report("match_fragments + result()", lambda: E.match_fragments(kp_s, kp_t, ds, dt, T, 0.1).stats.tolist())
    table = torch.zeros((64, 2), dtype=torch.int32, device=DEV)
    report("match_fragments into a table row (no read)", lambda: E.match_fragments(kp_s, kp_t, ds, dt, T, 0.1, out=table[3]))
    report("torch: cdist, two argmins, mutual test, count, tolist", lambda: torch_match(kp_s, kp_t, ds, dt, T, 0.1))


def make_scene(n_frag, frag_points, n_keys=5000, seed=3):
    """``n_frag`` overlapping x-windows of one box-surface world, each in a frame of its own; 5000 keypoints per fragment
    drawn from its points (ETH's keypoint files are indices into the fragment)."""
    rng = np.random.RandomState(seed)
    width = 4.0
    n_world = int(frag_points * (n_frag + width - 1) / width)
    world = synthetic.make_box_cloud(seed, n_points=n_world, cube=16.0, n_boxes=24).astype(np.float64)
    lo, hi = world[:, 0].min(), world[:, 0].max()
    step = (hi - lo) / (n_frag + width - 1)
    frags, keys, poses, gt = [], [], [], {}
    for i in range(n_frag):
        a = rng.normal(size=(3, 3))
        q, r = np.linalg.qr(a)
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = q, rng.uniform(-3, 3, 3)
        poses.append(pose)
        inside = world[(world[:, 0] >= lo + i * step) & (world[:, 0] <= lo + (i + width) * step)]
        inv = np.linalg.inv(pose)
        pts = (inside @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        frags.append(pts)
        keys.append(pts[rng.choice(len(pts), min(n_keys, len(pts)), replace=False)])
    for i in range(n_frag):
        for j in range(i + 1, n_frag):
            if j - i < width:
                gt[f"{i}_{j}"] = np.linalg.inv(poses[i]) @ poses[j]
    return frags, keys, gt


def reference_shaped_scene(model, frags, keys, gt, voxel=0.05, tau1=0.1, tau2=0.05):
    """The loop of generalization_ETH/evaluate.py:263-284 with torch in place of pytorch3d / sklearn / numpy: both fragments
    voxelised and run through the network for EVERY pair, nearest voxel by chunked cdist, matching by torch_match, one read
    per pair."""
    rows = []
    with torch.no_grad():
        for a in range(len(frags)):
            for b in range(a + 1, len(frags)):
                s0, s1, v0, v1 = E.prepare_pcd_to_input(frags[a], frags[b], voxel, DEV)
                F0, F1 = model(s0).F, model(s1).F
                ka, kb = torch.from_numpy(keys[a]).to(DEV), torch.from_numpy(keys[b]).to(DEV)
                da = F0[torch_nn(ka, v0.to(DEV), "use_mm_for_euclid_dist_if_necessary")[1]]
                db = F1[torch_nn(kb, v1.to(DEV), "use_mm_for_euclid_dist_if_necessary")[1]]
                if f"{a}_{b}" not in gt:
                    rows.append((0, 0.0, 0))
                    continue
                T = torch.from_numpy(gt[f"{a}_{b}"]).float().to(DEV)
                n_mut, n_inl = torch_match(ka, kb, da, db, T, tau1)
                rows.append((n_inl, n_inl / n_mut if n_mut else 0.0, 1))
    return E.scene_summary(rows, tau2)


def scene_section(n_frag, frag_points):
    frags, keys, gt = make_scene(n_frag, frag_points)
    torch.manual_seed(0)
    model = load_model("ResUNetFatBN")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(DEV).eval()
    n_vox = [len(E.fragment_input(f, 0.05, DEV)[1]) for f in frags]
    say(f"-- scene: {n_frag} fragments of {min(map(len, frags))} - {max(map(len, frags))} points ({min(n_vox)} - {max(n_vox)} voxels "
        f"at 5 cm), {len(keys[0])} keypoints each, {n_frag * (n_frag - 1) // 2} pairs of which {len(gt)} in the log; "
        "ResUNetFatBN, random weights")
    ours = E.evaluate_scene(frags, keys, gt, model=model)
    report("evaluate_scene (network once per fragment, one read)", lambda: E.evaluate_scene(frags, keys, gt, model=model),
           max_iters=3)
    descs = [E.fragment_descriptors(model, f, k, 0.05) for f, k in zip(frags, keys)]
    report("  of which: the pair loop alone (descriptors given)",
           lambda: E.evaluate_scene(None, keys, gt, descriptors=descs), max_iters=20)
    kept = {}
    report("reference loop shape in torch (network twice per pair)",
           lambda: kept.update(reference_shaped_scene(model, frags, keys, gt)), max_iters=1)
    theirs = kept
    say(f"   recall / correct / ave inliers: HIP path {ours['recall']:.1f} % / {ours['correct_match']} / "
        f"{ours['ave_num_inliers']:.1f}; torch loop {theirs['recall']:.1f} % / {theirs['correct_match']} / "
        f"{theirs['ave_num_inliers']:.1f} (an untrained network: the figures say nothing about a model)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fragments", type=int, default=16)
    ap.add_argument("--frag-points", type=int, default=10000)
    ap.add_argument("--skip-scene", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    say(f"eth_eval_probe on {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    with torch.cuda.device(DEV):
        nn3_section()
        match_section()
        if not args.skip_scene:
            scene_section(args.fragments, args.frag_points)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
