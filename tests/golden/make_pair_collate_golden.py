"""Generates tests/golden/pair_collate.npz by IMPORTING the reference's own ``collate_pair_fn`` (lib/data_loaders.py:26-79).

Run:  python tests/golden/make_pair_collate_golden.py      (needs the reference checkout make_golden.py names; arrays only)

``lib/data_loaders.py`` imports under the empty stub modules of ``make_golden._import_reference``; the one third-party call on
this path, ``ME.utils.sparse_collate`` (:59-60), is served by this repository's own ``gcl_amd.MinkowskiEngine.utils`` (so the
golden pins the reference's bookkeeping -- which pairs are dropped, how the start indices move -- not that function).

Three pairs, the second WITHOUT a match: it must vanish from pcd0 / pcd1 / T_gt / len_batch while the start indices of the
third pair move past its rows.  ``correspondences`` is stored as the reference returns it (int32, ``.int()``).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _import_reference      # noqa: E402


def main():
    _import_reference()
    from gcl_amd.MinkowskiEngine import utils as me_utils
    sys.modules["MinkowskiEngine"].utils = me_utils
    from lib.data_loaders import collate_pair_fn
    rng = np.random.RandomState(31)
    sizes = [(40, 50), (30, 20), (25, 35)]
    items, store = [], {}
    for b, (n0, n1) in enumerate(sizes):
        c0 = rng.permutation(1000)[:n0, None] * np.array([[1, 0, 0]]) + rng.randint(-20, 20, (n0, 3)) * np.array([[0, 1, 1]])
        c1 = rng.permutation(1000)[:n1, None] * np.array([[1, 0, 0]]) + rng.randint(-20, 20, (n1, 3)) * np.array([[0, 1, 1]])
        xyz0 = ((c0 + rng.rand(n0, 3)) * 0.3).astype(np.float32)
        xyz1 = ((c1 + rng.rand(n1, 3)) * 0.3).astype(np.float32)
        n_m = 0 if b == 1 else 60
        m = [(int(i), int(j)) for i, j in zip(rng.randint(0, n0, n_m), rng.randint(0, n1, n_m))]
        T = np.eye(4)
        T[:3] = rng.normal(size=(3, 4))
        items.append((torch.from_numpy(xyz0), torch.from_numpy(xyz1), torch.from_numpy(c0).int(), torch.from_numpy(c1).int(),
                      torch.ones(n0, 1), torch.ones(n1, 1), m, T))
        store.update({f"xyz0_{b}": xyz0, f"xyz1_{b}": xyz1, f"coords0_{b}": c0.astype(np.int32), f"coords1_{b}": c1.astype(np.int32),
                      f"matches_{b}": np.asarray(m, dtype=np.int64).reshape(-1, 2), f"trans_{b}": T})
    out = collate_pair_fn(items)
    for k, v in out.items():
        store["out_" + k] = np.asarray(v) if k == "len_batch" else v.numpy()
    path = os.path.join(HERE, "pair_collate.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), {k: v.shape for k, v in store.items() if k.startswith("out_")})


if __name__ == "__main__":
    main()
