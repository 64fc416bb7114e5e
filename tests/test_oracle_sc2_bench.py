"""The SC2-PCR benchmark's host half and fixtures, without a GPU: the numpy restatement of the per-pair statistics
(tests/sc2_bench_oracle.py) against the reference's recorded values (tests/golden/sc2_bench_s*.npz, written by
make_sc2_bench_golden.py from the reference's TransformationLoss / ClassificationLoss / transform), the chunk former against
``BatchMatcher.plan``'s rules, the two summaries against the reference's expressions, and the argument checks of the two new
C-ABI entries (they come before any launch)."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sc2_bench_oracle as SO                                          # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = sorted(glob.glob(os.path.join(G, "sc2_bench_s[0-2].npz")))
INT_COLS = [0, 3, 5]


def test_goldens_hold_the_cases_the_kernel_must_survive():
    assert len(GOLDENS) == 3
    z = [np.load(p) for p in GOLDENS]
    ref = np.concatenate([x["stats_ref"] for x in z])
    counts = np.concatenate([x["counts"] for x in z])
    assert {1, 257, 700} <= set(z[0]["counts"].tolist()), "counts 1, 257 and 700 share a batch"
    assert ((ref[:, 5] == 0) & (ref[:, 3] > 0) & (ref[:, 6:9] == 0).all(1)).any(), "a pair with no predicted inlier"
    assert (ref[:, 3] == 0).any(), "a pair with no gt inlier"
    assert (ref[:, 0] == 0).any() and (ref[:, 0] == 1).any(), "a failed and a successful pair"
    assert counts.min() == 1 and counts.max() >= 1000
    # the generator's guard bands, re-checked on what it stored: no distance within 1e-4 thr of the threshold (fp32 and
    # float64, both transformations), RE / TE not within 1e-3 relative of theirs
    for x in z:
        thr = float(x["inlier_threshold"])
        for b, n in enumerate(x["counts"]):
            for T in (x["gt_trans"][b], x["pred_trans"][b]):
                for dt in (np.float32, np.float64):
                    d = SO.distances(x["src"][b, :n], x["tgt"][b, :n], T, dt).astype(np.float64)
                    assert (np.abs(d - thr) > 1e-4 * thr).all()
            for col, key in ((0, "re_thre"), (1, "te_thre")):
                for v in (x["stats_f64"][b, col], x["stats_ref"][b, col + 1]):
                    assert abs(v - float(x[key])) > 1e-3 * float(x[key])


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_numpy_restatement_reproduces_the_reference(path):
    x = np.load(path)
    got = SO.batch_stats(x["src"], x["tgt"], x["counts"], x["pred_trans"], x["gt_trans"], float(x["inlier_threshold"]),
                         float(x["re_thre"]), float(x["te_thre"]))
    ref, f64 = x["stats_ref"], x["stats_f64"]
    assert (got[:, INT_COLS] == ref[:, INT_COLS]).all(), "success and the two inlier counts are exact"
    for k, col in enumerate((1, 2, 9)):
        assert np.allclose(got[:, col], f64[:, k], rtol=1e-9, atol=0), (col, got[:, col], f64[:, k])
        assert (np.abs(got[:, col] - ref[:, col]) <= 2 * np.abs(ref[:, col] - f64[:, k]) + 1e-9).all(), col
    assert np.abs(got[:, [4, 6, 7, 8]] - ref[:, [4, 6, 7, 8]]).max() <= 1e-6


def test_chunk_former_obeys_the_plan_rules():
    from gcl_amd.scripts.SC2_PCR import BatchMatcher
    from gcl_amd.scripts.SC2_PCR_bench import form_chunks
    m = BatchMatcher(inlier_threshold=0.1, num_node="all", d_thre=0.1, num_iterations=10, ratio=0.1, nms_radius=0.1,
                     max_points=500, k1=30, k2=20)
    counts = [300, 900, 29, 12, 400, 4, 0, 30, 31, 700, 650, 600, 550, 9, 500]
    chunks = form_chunks(counts, 4, m.k1, m.ratio, m.max_points)
    assert [i for _, idx in chunks for i in idx] == list(range(len(counts))), "every pair once, in order"
    assert chunks == [("full", [0, 1]), ("small", [2, 3]), ("full", [4]), ("fail", [5]), ("fail", [6]),
                      ("full", [7, 8, 9, 10]), ("full", [11, 12]), ("fail", [13]), ("full", [14])]
    for kind, idx in chunks:
        cs = [counts[i] for i in idx]
        if kind == "fail":
            assert len(idx) == 1
            with pytest.raises(ValueError, match="too few"):
                m.plan(max(cs + [1]), cs, len(cs))
            continue
        assert len(idx) <= 4
        cut, n_seeds, k1, k2 = m.plan(max(cs), cs, len(cs))            # raises if the chunk breaks a rule
        assert (k1, k2) == ((4, 4) if kind == "small" else (30, 20)) and min(n_seeds) >= 1 and max(cut) <= 500
    # the max_points cut decides the class, as in plan: 900 correspondences cut to 20 are 'small'
    assert form_chunks([900, 25], 8, 30, 0.2, 20) == [("small", [0, 1])]
    assert form_chunks([50, 60, 70], 1, 30, 0.2, 8000) == [("full", [0]), ("full", [1]), ("full", [2])]
    assert form_chunks([], 8, 30, 0.2, 8000) == []


def test_summaries_match_the_reference_expressions():
    from gcl_amd.scripts.SC2_PCR_bench import summarize_pairs, summarize_scenes
    rng = np.random.RandomState(5)
    tables = {}
    for k, n in enumerate((7, 1, 12)):
        st = rng.uniform(0, 50, (n, 12))
        st[:, 0] = rng.randint(0, 2, n)
        st[:, 11] = k
        tables[f"scene{k}"] = st
    tables["scene0"][0, 0], tables["scene1"][0, 0], tables["scene2"][3, 0] = 1, 1, 1
    # test_KITTI.py:110-118
    allp = np.concatenate(list(tables.values()), axis=0)
    average, correct = allp.mean(0), allp[allp[:, 0] == 1].mean(0)
    s = summarize_pairs(allp)
    assert s["n_pairs"] == 20 and s["success_rate"] == average[0] and s["re"] == correct[1] and s["te"] == correct[2]
    for name, col in (("input_inlier_num", 3), ("input_inlier_ratio", 4), ("output_inlier_num", 5), ("precision", 6),
                      ("recall", 7), ("f1", 8), ("model_time", 9), ("data_time", 10)):
        assert s[name] == average[col], name
    # test_3DMatch.py:119-143
    scene_vals = np.zeros([3, 12])
    for k, st in enumerate(tables.values()):
        correct_pair = np.where(st[:, 0] == 1)
        scene_vals[k] = st.mean(0)
        scene_vals[k, 1] = st[correct_pair].mean(0)[1]
        scene_vals[k, 2] = st[correct_pair].mean(0)[2]
    r = summarize_scenes(tables)
    assert r["scenes"] == list(tables) and (r["scene_vals"] == scene_vals).all() and (r["average"] == scene_vals.mean(0)).all()
    assert (r["all_stats"] == allp).all() and r["allpair"] == s
    # no successful pair: RE / TE are NaN, nothing raises
    none = allp.copy()
    none[:, 0] = 0
    s0 = summarize_pairs(none)
    assert s0["success_rate"] == 0 and np.isnan(s0["re"]) and np.isnan(s0["te"])


def test_new_entries_check_their_arguments_before_any_launch():
    from gcl_amd import _lib
    lib = _lib.load()
    p8 = ctypes.c_void_p(8)
    assert lib.gcl_nn_rowmin_any_scratch_len(0, 5, 33) == 0 and lib.gcl_nn_rowmin_any_scratch_len(5, 5, 129) == 0
    # the interleaved copy of B is padded to 40 channels; 5000 x 5000 runs in several chunks (partial results on top)
    assert lib.gcl_nn_rowmin_any_scratch_len(10, 8, 33) == 4 * 2 * 40
    assert lib.gcl_nn_rowmin_any_scratch_len(5000, 5000, 33) > 2500 * 2 * 40
    assert lib.gcl_nn_rowmin_any_scratch_len(64, 8, 128) == 4 * 2 * 128
    for c in (0, 129, -3):
        rc = lib.gcl_nn_rowmin_any(p8, None, 10, p8, None, 10, c, 0, p8, p8, p8, None)
        assert rc == -1 and b"1 .. 128" in lib.gcl_last_error(), c
    rc = lib.gcl_nn_rowmin_any(p8, None, 10, p8, None, 10, 33, 0, None, p8, p8, None)
    assert rc == -1 and b"scratch" in lib.gcl_last_error()
    rc = lib.gcl_nn_rowmin_any(p8, None, 0, p8, None, 10, 33, 0, p8, p8, p8, None)
    assert rc == -1 and b"empty" in lib.gcl_last_error()
    # the old entry keeps its refusal of every other width
    rc = lib.gcl_nn_rowmin(p8, None, 10, p8, None, 10, 48, 0, p8, p8, p8, None)
    assert rc == -1 and b"16, 32 or 64" in lib.gcl_last_error()
    # statistics: null tables and negative sizes are refused, an empty batch is no launch
    rc = lib.gcl_registration_stats(p8, p8, 2, 10, None, p8, p8, 0.1, 15.0, 30.0, None, None, None, None)
    assert rc == -1 and b"null" in lib.gcl_last_error()
    rc = lib.gcl_registration_stats(None, p8, 2, 10, None, p8, p8, 0.1, 15.0, 30.0, p8, None, None, None)
    assert rc == -1 and b"src_corr" in lib.gcl_last_error()
    rc = lib.gcl_registration_stats(p8, p8, -1, 10, None, p8, p8, 0.1, 15.0, 30.0, p8, None, None, None)
    assert rc == -1 and b"negative" in lib.gcl_last_error()
    assert lib.gcl_registration_stats(p8, p8, 0, 10, None, p8, p8, 0.1, 15.0, 30.0, p8, None, None, None) == 0


def test_bench_module_fails_loudly_without_gpu():
    import torch
    from gcl_amd.scripts.SC2_PCR_bench import eval_per_pair, registration_stats
    if torch.cuda.is_available():
        return                                  # tests/test_gpu_sc2_bench.py runs both there
    with pytest.raises(RuntimeError, match="GPU"):
        registration_stats(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), None, torch.eye(4)[None], torch.eye(4)[None], 0.1, 15, 30)
    with pytest.raises(RuntimeError, match="GPU"):
        eval_per_pair([], None, dict(inlier_threshold=0.1, re_thre=15, te_thre=30))
