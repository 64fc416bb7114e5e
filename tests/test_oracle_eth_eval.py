"""The feature-match-recall oracle (tests/eth_eval_oracle.py) against independent implementations, the scene's log reader,
and the argument checks of the new C-ABI entries -- all without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/eth_eval_oracle.py
import eth_eval_oracle as EO                                           # noqa: E402


def _distinct_descriptors(seed, m0, m1, c):
    """Random rows whose nearest neighbour is unambiguous: every fp64 best / runner-up gap above 1e-9, both ways."""
    rng = np.random.RandomState(seed)
    a, b = rng.normal(size=(m0, c)), rng.normal(size=(m1, c))
    b[: min(m0, m1) // 2] = a[: min(m0, m1) // 2] + 0.05 * rng.normal(size=(min(m0, m1) // 2, c))     # many mutual pairs
    return a, b


@pytest.mark.parametrize("m0,m1,c", [(40, 40, 3), (300, 211, 32), (97, 350, 16)])
def test_mutual_pairs_match_the_kdtree_recipe(m0, m1, c):
    """calculate_M's recipe (generalization_ETH/evaluate.py:63-77): a KD-tree query each way, keep i when the target's
    nearest source is i again."""
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    a, b = _distinct_descriptors(m0 + c, m0, m1, c)
    _, nn01, gap01 = EO.nn(a, b, with_gap=True)
    _, nn10, gap10 = EO.nn(b, a, with_gap=True)
    assert gap01.min() > 1e-9 and gap10.min() > 1e-9, "test data must have unambiguous nearest neighbours"
    ours = EO.mutual(nn01, nn10)
    _, s_idx = KDTree(b).query(a, 1)
    _, t_idx = KDTree(a).query(b, 1)
    theirs = np.array([[i, s_idx[i][0]] for i in range(len(s_idx)) if t_idx[s_idx[i]] == i]).reshape(-1, 2)
    assert len(ours) >= min(m0, m1) // 4
    assert np.array_equal(ours, theirs)
    assert np.all(np.diff(ours[:, 0]) > 0)


def test_mutual_filter_drops_out_of_range_entries():
    nn01 = np.array([2, -1, 0, 7, 1])
    nn10 = np.array([2, 4, 0])
    assert EO.mutual(nn01, nn10).tolist() == [[0, 2], [2, 0], [4, 1]]
    assert EO.mutual(np.zeros(0, dtype=np.int64), nn10).shape == (0, 2)


def test_nn3_matches_ckdtree():
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    rng = np.random.RandomState(3)
    p = rng.uniform(-20, 20, (5000, 3))
    q = rng.uniform(-21, 21, (700, 3))
    d2, arg, gap = EO.nn(q, p, with_gap=True)
    assert gap.min() > 1e-9
    dist, idx = cKDTree(p).query(q, 1)
    assert np.array_equal(arg, idx)
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    # ties: the lowest index
    p2 = np.concatenate([p[:10], p[:10]])
    assert np.array_equal(EO.nn(p[:10], p2)[1], np.arange(10))


def test_inlier_count_and_scene_aggregation():
    rng = np.random.RandomState(5)
    kp1 = rng.uniform(-5, 5, (6, 3))
    th = 0.7
    T = np.eye(4)
    T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    T[:3, 3] = [1.0, -2.0, 0.5]
    kp0 = kp1 @ T[:3, :3].T + T[:3, 3]
    kp0[1] += [0.0, 0.2, 0.0]
    kp0[4] += [0.09, 0.0, 0.0]
    pairs = np.stack([np.arange(6), np.arange(6)], 1)
    assert EO.inliers(pairs, kp0, kp1, T, 0.1) == 5
    assert EO.inliers(pairs[:0], kp0, kp1, T, 0.1) == 0
    table = [EO.pair_row(100, 30), EO.pair_row(50, 2), EO.pair_row(0, 0), EO.pair_row(10, 10, in_log=False), EO.pair_row(40, 20)]
    s = EO.scene(table, 0.05)
    assert s == dict(recall=50.0, correct_match=2, gt_match=4, ave_num_inliers=25.0)
    assert EO.scene([EO.pair_row(0, 0)])["ave_num_inliers"] == 0.0 and EO.scene([EO.pair_row(0, 0)])["recall"] == 0.0
    from gcl_amd.generalization_ETH.evaluate import scene_summary
    assert scene_summary(table, 0.05) == s


def test_loadlog_round_trips_a_written_log(tmp_path):
    from gcl_amd.generalization_ETH.evaluate import loadlog, write_log
    rng = np.random.RandomState(1)
    want = {}
    with open(tmp_path / "gt.log", "w") as f:
        for (a, b) in [(0, 1), (0, 3), (2, 31)]:
            T = np.eye(4)
            T[:3] = rng.normal(size=(3, 4))
            want[f"{a}_{b}"] = T
            f.write(f"{a}\t {b}\t 32\n")
            for r in range(4):
                f.write("\t".join(repr(float(x)) for x in T[r]) + "\t\n")
    got = loadlog(str(tmp_path))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == (4, 4) and np.array_equal(got[k], want[k])
    # the prediction log is written in the same form
    write_log(str(tmp_path / "sub.log"), [(0, 1, want["0_1"]), (2, 31, want["2_31"])])
    os.replace(tmp_path / "sub.log", tmp_path / "gt.log")
    again = loadlog(str(tmp_path))
    assert sorted(again) == ["0_1", "2_31"] and np.array_equal(again["2_31"], want["2_31"])


def test_new_entries_check_their_arguments_without_gpu():
    from gcl_amd import _lib
    _lib.build()
    lib = _lib.load()
    p8 = ctypes.c_void_p(8)
    # sizes are host arithmetic: no scratch for a single chunk, two words per (chunk, query) otherwise
    assert lib.gcl_nn3_scratch_len(0, 100) == 0 and lib.gcl_nn3_scratch_len(100, 0) == 0
    assert lib.gcl_nn3_scratch_len(5, 200) == 0
    big = lib.gcl_nn3_scratch_len(5000, 200000)
    assert big >= 2 * 2 * 5000 and big % (2 * 5000) == 0
    # m == 0: nothing to do, no launch
    assert lib.gcl_nn3_rowmin(None, 0, p8, 10, None, 0, None, None, None, None, None) == 0
    rc = lib.gcl_nn3_rowmin(None, 10, p8, 10, None, 0, None, p8, p8, None, None)
    assert rc == -1 and b"null" in lib.gcl_last_error()
    rc = lib.gcl_nn3_rowmin(p8, 10, p8, 10, None, 0, None, p8, None, None, None)
    assert rc == -1 and b"null" in lib.gcl_last_error()
    rc = lib.gcl_nn3_rowmin(p8, 5000, p8, 200000, None, 0, None, p8, p8, None, None)
    assert rc == -1 and b"scratch" in lib.gcl_last_error()
    rc = lib.gcl_nn3_rowmin(p8, 10, p8, 10, p8, 32, None, p8, p8, None, None)
    assert rc == -1 and b"feat and desc" in lib.gcl_last_error()
    rc = lib.gcl_nn3_rowmin(p8, 10, p8, 10, None, 32, None, p8, p8, p8, None)
    assert rc == -1 and b"feat and desc" in lib.gcl_last_error()
    rc = lib.gcl_nn3_rowmin(p8, 10, p8, 10, p8, 0, None, p8, p8, p8, None)
    assert rc == -1 and b"width" in lib.gcl_last_error()
    for n in (0, -3):
        rc = lib.gcl_nn3_rowmin(p8, 10, p8, n, None, 0, None, p8, p8, None, None)
        assert rc == -1 and b"no points" in lib.gcl_last_error()
    rc = lib.gcl_mutual_match(None, 10, p8, 10, None, None, None, 0.1, p8, p8, None)
    assert rc == -1 and b"null" in lib.gcl_last_error()
    rc = lib.gcl_mutual_match(p8, 10, p8, 10, None, None, None, 0.1, p8, None, None)
    assert rc == -1 and b"stats" in lib.gcl_last_error()
    rc = lib.gcl_mutual_match(p8, 10, None, 10, None, None, None, 0.1, p8, p8, None)
    assert rc == -1 and b"nn10" in lib.gcl_last_error()
    rc = lib.gcl_mutual_match(p8, 10, p8, 10, p8, None, p8, 0.1, p8, p8, None)
    assert rc == -1 and b"keypoint" in lib.gcl_last_error()
    rc = lib.gcl_mutual_match(p8, -1, p8, 10, None, None, None, 0.1, p8, p8, None)
    assert rc == -1 and b"negative" in lib.gcl_last_error()


def test_python_surface_rejects_what_the_kernels_cannot_take():
    import torch
    from gcl_amd.generalization_ETH import evaluate as E
    with pytest.raises(ValueError, match="16, 32 or 64"):
        E._check_width(48)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            E.calculate_M(np.zeros((4, 32), dtype=np.float32), np.zeros((4, 32), dtype=np.float32))
        from gcl_amd.lib.metrics import nn3_min
        with pytest.raises(RuntimeError, match="GPU"):
            nn3_min(torch.zeros(4, 3), torch.zeros(4, 3))


def test_far_grid_data_defeats_the_expansion_form():
    """The far-from-origin case of the GPU test tells the two arithmetic forms apart: |q|^2 + |p|^2 - 2 q.p in fp32 picks a
    point beyond min * (1 + 1e-6) for most queries, the difference form in fp32 (numpy here) for none."""
    q, p = EO.far_grid_case()
    d2, _ = EO.nn(q, p)
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    wrong = EO.expansion_form_fp32(q, p)
    assert (((q64 - p64[wrong]) ** 2).sum(1) > d2 * (1 + 1e-6)).mean() > 0.5
    diff = (q[:, None, :] - p[None, :, :]) ** 2
    right = ((diff[..., 0] + diff[..., 1]) + diff[..., 2]).argmin(1)
    assert np.all(((q64 - p64[right]) ** 2).sum(1) <= d2 * (1 + 1e-6))


def test_scene_case_is_what_the_gpu_test_takes_it_for():
    """Planted descriptors: every logged pair is correct and its inlier count is the number of shared keypoints; the rolled
    copy matches nothing."""
    from gcl_amd import synthetic
    sc = EO.scene_case(synthetic.make_box_cloud(11, n_points=8000, cube=8.0))
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    assert sorted(sc["gt_log"]) == ["0_1", "0_2", "1_2", "1_3", "2_3"] and min(sc["shared"][p] for p in pairs if p != (0, 3)) >= 20
    table = EO.scene_table(sc["keypoints"], sc["descriptors"], sc["gt_log"])
    assert [int(r[0]) for r in table] == [sc["shared"][p] if p != (0, 3) else 0 for p in pairs]
    s = EO.scene(table)
    assert s["recall"] == 100.0 and s["correct_match"] == s["gt_match"] == 5
    for a, b in zip(sc["descriptors"], sc["shuffled"]):
        assert sorted(map(tuple, a)) == sorted(map(tuple, b)) and not np.array_equal(a, b)
    t2 = EO.scene_table(sc["keypoints"], sc["shuffled"], sc["gt_log"])
    assert EO.scene(t2) == dict(recall=0.0, correct_match=0, gt_match=5, ave_num_inliers=0.0)
