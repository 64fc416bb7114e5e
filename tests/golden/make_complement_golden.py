"""Generates tests/golden/complement_s0.npz by IMPORTING the reference's own ``sample_random_trans`` and
``PointDataset.apply_transform`` (lib/complement_data_loader.py:33-38, :65-70).

Run:  python tests/golden/make_complement_golden.py      (needs the reference checkout make_golden.py names; arrays only)

``lib/complement_data_loader.py`` imports under the empty stub modules of ``make_golden._import_reference``.  What is written:
one raw sample of tests/complement_scenes.py (two centre scans of 1 200 points, 1 500 + 500 complement points, their
transforms), and what the reference's functions make of it in ``__getitem__``'s order (:576-628): the complement scans after
``apply_transform(xyz_k, M_k)``; for three rotation ranges drawn from ONE generator (the KITTI loader's ``np.pi * 2``, the
``np.pi / 4`` of both loaders, and 360 for a real turn) ``T0`` / ``T1`` of ``sample_random_trans``, the centre scans and the
complement scans moved by them, ``np.max((xyz ** 2).sum(-1))`` and the crop mask ``(xyz_cmpl ** 2).sum(-1) < max``; the same
without a rotation; the generator's state after the draws; and the scale of :656-658 for 24 seeds of ``random`` (NaN: not
scaled), evaluated here with the reference's expression.  Prints how many complement points lie inside the margin in which
tests/test_oracle_complement.py lets two float32 evaluation orders disagree about the crop.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _import_reference      # noqa: E402

SEED = 0
RANGES = (np.pi * 2, np.pi / 4, 360.0)
FRAME = np.array([30.0, -20.0, 1.0])
MIN_SCALE, MAX_SCALE = 0.8, 1.2


def main():
    _import_reference()
    from lib.complement_data_loader import PointDataset, sample_random_trans
    import complement_oracle as CO
    import complement_scenes as CS
    apply_transform = lambda pts, T: PointDataset.apply_transform(None, pts, T)
    s = CS.make_sample(9, (500, 600, 400), (500,), n_centre=1200, shift=FRAME)
    out = {"seed": SEED, "ranges": np.array(RANGES), "xyz0": s["xyz0"], "xyz1": s["xyz1"], "min_max_scale": np.array([MIN_SCALE, MAX_SCALE])}
    stage1 = []
    for k in (0, 1):
        out[f"cmpl{k}"] = np.concatenate(s[f"cmpl{k}"])
        out[f"cmpl{k}_sizes"] = np.array([len(x) for x in s[f"cmpl{k}"]])
        out[f"list_M{k}"] = np.stack(s[f"list_M{k}"])
        stage1.append([apply_transform(x, M) for x, M in zip(s[f"cmpl{k}"], s[f"list_M{k}"])])
        out[f"stage1_{k}"] = np.concatenate(stage1[k])
        assert out[f"stage1_{k}"].dtype == np.float32

    def crop(centre, moved):
        max_d = np.max((centre ** 2).sum(-1))
        cat = np.concatenate(moved, axis=0)
        return max_d, (cat ** 2).sum(-1) < max_d

    for k in (0, 1):
        out[f"max_plain_{k}"], out[f"keep_plain_{k}"] = crop(s[f"xyz{k}"], stage1[k])
    randg = np.random.RandomState()
    randg.seed(SEED)
    Ts = [[sample_random_trans(s["xyz0"], randg, r), sample_random_trans(s["xyz1"], randg, r)] for r in RANGES]
    state = randg.get_state()
    out.update(T=np.array(Ts), state_key=state[1], state_pos=state[2])
    inside = 0
    for i in range(len(RANGES)):
        for k in (0, 1):
            T = Ts[i][k]
            centre = apply_transform(s[f"xyz{k}"], T)
            moved = [apply_transform(c, T) for c in stage1[k]]
            out[f"centre_{i}_{k}"], out[f"stage2_{i}_{k}"] = centre, np.concatenate(moved)
            out[f"max_{i}_{k}"], out[f"keep_{i}_{k}"] = crop(centre, moved)
            # the margin, from the reference's own numbers
            b1 = np.concatenate([CO.stage_bound(x, M) for x, M in zip(s[f"cmpl{k}"], s[f"list_M{k}"])])
            b2 = CO.stage_bound(out[f"stage1_{k}"], T, b1)
            bc = CO.stage_bound(s[f"xyz{k}"], T)
            margin = CO.range_bound(out[f"stage2_{i}_{k}"], b2) + CO.range_bound(centre, bc).max()
            inside += int((np.abs(CO.range2_f64(out[f"stage2_{i}_{k}"]) - CO.range2_f64(centre).max()) <= margin).sum())
    scales = []
    for seed in range(24):
        random.seed(seed)
        scale = np.nan
        if random.random() < 0.95:
            scale = MIN_SCALE + (MAX_SCALE - MIN_SCALE) * random.random()
        scales.append(scale)
    out["scales"] = np.array(scales)
    path = os.path.join(HERE, "complement_s0.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "complement points inside the crop margin (reference alone):", inside)


if __name__ == "__main__":
    main()
