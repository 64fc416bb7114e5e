"""SC2-PCR registration, every stage as raw bytes: a dump to compare two builds of the library bit for bit.

Writes into ONE .npz the bytes (uint8 arrays) of ``out``, ``labels``, ``conf``, ``seeds``, ``knn``, ``seed_trans``, ``fitness``
and ``best`` of

  * each golden problem tests/golden/sc2pcr_s*.npz, alone through ``Matcher``            (keys golden<i>/single/<stage>)
  * the same problems as one ``BatchMatcher`` batch                                      (keys golden<i>/batch/<stage>)
  * the planted problems of tests/test_gpu_sc2_batch.py at n = 5, 29, 64, 65, 129, 256, 257, 1001 (``planted_case`` of
    tests/ransac_oracle.py, that file's seeds), alone through ``Matcher``                (keys planted<n>/single/<stage>)
  * the same planted problems through ``BatchMatcher``: n = 5, 29 as one batch and the others as a second -- pairs below
    k1 = 30 use (k1, k2) = (4, 4) and cannot share a call with pairs that do not          (keys planted<n>/batch/<stage>)

Only the Python interface is used, so the tool runs unchanged on any commit that has ``Matcher`` and ``BatchMatcher``.

    python3 tools/micro/sc2_stage_dump.py --out A.npz
    python3 tools/micro/sc2_stage_dump.py --compare A.npz B.npz        # every differing key; exit status 1 if there is one
"""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

STAGES = ("out", "labels", "conf", "seeds", "knn", "seed_trans", "fitness", "best")
CFG = dict(inlier_threshold=0.6, d_thre=0.1, num_iterations=20, ratio=0.2, nms_radius=0.6, max_points=8000, k1=30, k2=20)
PLANTED = (5, 29, 64, 65, 129, 256, 257, 1001)


def _raw(t):
    return np.frombuffer(t.detach().contiguous().cpu().numpy().tobytes(), np.uint8)


def dump(path, dev):
    import torch
    import ransac_oracle as RO
    from gcl_amd.scripts.SC2_PCR import BatchMatcher, Matcher
    problems = []
    for i, p in enumerate(sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sc2pcr_s*.npz")))):
        z = np.load(p)
        assert all(float(z[k]) == CFG[k] for k in CFG), p
        problems.append((f"golden{i}", "golden", z["src"], z["tgt"]))
    for n in PLANTED:      # test_word_tile_and_chunk_edges_in_one_batch / test_a_batch_below_k1_uses_the_four_nearest
        src, tgt = RO.planted_case((200 if n < CFG["k1"] else 100) + n, n, 0.5, noise=0.05)[:2]
        problems.append((f"planted{n}", "below k1" if n < CFG["k1"] else "planted", src, tgt))
    res = {}
    with torch.cuda.device(dev):
        for name, _, src, tgt in problems:
            m = Matcher(num_node="all", use_mutual=False, **CFG)
            T = m.SC2_PCR(torch.from_numpy(src).to(dev)[None], torch.from_numpy(tgt).to(dev)[None])
            for k in STAGES:
                res[f"{name}/single/{k}"] = _raw(T if k == "out" else m._labels if k == "labels" else m.last[k])
        for group in ("golden", "below k1", "planted"):
            sel = [p for p in problems if p[1] == group]
            n_cap = max(len(p[2]) for p in sel)
            src = np.full((len(sel), n_cap, 3), np.nan, np.float32)
            tgt = np.full((len(sel), n_cap, 3), np.nan, np.float32)
            for b, (_, _, s, t) in enumerate(sel):
                src[b, :len(s)], tgt[b, :len(t)] = s, t
            m = BatchMatcher(num_node="all", use_mutual=False, **CFG)
            m.SC2_PCR(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), counts=[len(p[2]) for p in sel])
            for b, (name, _, _, _) in enumerate(sel):
                for k in STAGES:
                    res[f"{name}/batch/{k}"] = _raw(m.last[b][k])
        torch.cuda.synchronize()
    np.savez(path, **res)
    print(f"{len(res)} arrays of {len(problems)} problems -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"only in one dump: {k}")
    for k in sorted(set(A.files) & set(B.files)):
        if A[k].shape != B[k].shape or not np.array_equal(A[k], B[k]):
            n = int((A[k] != B[k]).sum()) if A[k].shape == B[k].shape else -1
            print(f"differs: {k} ({n} of {A[k].size} bytes)")
            bad.append(k)
    print(f"{len(set(A.files) & set(B.files))} common keys, {len(bad)} differing")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="sc2_stage_dump.npz")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out, a.device)


if __name__ == "__main__":
    main()
