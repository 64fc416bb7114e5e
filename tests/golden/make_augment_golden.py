"""Generates tests/golden/augment_s0.npz by IMPORTING the reference's own ``M``, ``sample_random_trans`` and
``follow_presampled_trans`` (lib/colocation_data_loader.py:33-50).

Run:  python tests/golden/make_augment_golden.py      (needs the reference checkout make_golden.py names; arrays only)

``lib/colocation_data_loader.py`` imports under the empty stub modules of ``make_golden._import_reference``.  What is written:
the seed, a centre and a neighbour cloud (float32, <= 2 000 points each, as a scan file holds them), the rotation ranges of
two consecutive draws from ONE generator (360, and the ``np.pi / 4`` the datasets pass, :352), the reference's ``T0`` of either
draw, ``Tc = follow_presampled_trans(neighbour, T0)``, the generator's state after the draws, and a ground-truth transform
before and after ``list_M[i] = T0 @ list_M[i] @ np.linalg.inv(Tc)`` (:358, evaluated here with the reference's expression).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _import_reference      # noqa: E402

SEED = 0


def main():
    _import_reference()
    from lib.colocation_data_loader import M, follow_presampled_trans, sample_random_trans
    assert np.allclose(M(np.array([0.0, 0.0, 2.0]), np.pi / 2) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    from gcl_amd import synthetic
    scene = synthetic.make_scene(5, n_boxes=10)
    shift = np.array([12.0, -7.0, 1.5])
    center = (synthetic.raycast(scene, np.array([0.0, 0.0, 0.0]), 11)[::7][:2000] + shift).astype(np.float32)
    nghb = (synthetic.raycast(scene, np.array([6.0, 0.3, 0.0]), 12)[::7][:1900] + shift).astype(np.float32)
    randg = np.random.RandomState()
    randg.seed(SEED)
    ranges = np.array([360.0, np.pi / 4])
    T0s = np.stack([sample_random_trans(center, randg, r) for r in ranges])
    Tcs = np.stack([follow_presampled_trans(nghb, T0) for T0 in T0s])
    state = randg.get_state()
    M_in = np.eye(4)
    M_in[:3, :3] = M(np.array([0.1, -0.2, 1.0]), 0.05)
    M_in[:3, 3] = [6.0, 0.3, 0.02]
    M_out = np.stack([T0 @ M_in @ np.linalg.inv(Tc) for T0, Tc in zip(T0s, Tcs)])
    path = os.path.join(HERE, "augment_s0.npz")
    np.savez_compressed(path, seed=SEED, center=center, nghb=nghb, ranges=ranges, T0=T0s, Tc=Tcs, state_key=state[1],
                        state_pos=state[2], state_gauss=np.array([state[3], state[4]]), M_in=M_in, M_out=M_out)
    print("wrote", path, os.path.getsize(path), center.shape, nghb.shape)


if __name__ == "__main__":
    main()
