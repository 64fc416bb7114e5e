"""Host-side (CPU) logic of the product package: ME.utils, hashes, synthetic input contracts, model registry."""
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import synthetic
from gcl_amd.MinkowskiEngine import utils as U
from gcl_amd.util import misc
from oracle import loss_oracle as LO

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_quantize_first_occurrence_and_floor():
    xyz = np.array([[0.2, 0.2, 0.2], [-0.1, 0.0, 0.0], [0.9, 0.9, 0.9], [-0.9, 0.5, 0.5], [1.0, 0.0, 0.0]])
    c, idx = U.sparse_quantize(xyz, return_index=True)
    assert idx.tolist() == [0, 1, 4]                      # rows 2 and 3 fall into voxels seen earlier
    assert c.tolist() == [[0, 0, 0], [-1, 0, 0], [1, 0, 0]] and c.dtype == np.int32
    ct, it = U.sparse_quantize(torch.from_numpy(xyz), return_index=True)
    assert it.tolist() == [0, 1, 4] and ct.dtype == torch.int32
    assert U.sparse_quantize(np.zeros((0, 3))).shape == (0, 3)


def test_collate_and_batched_coordinates():
    a, b = np.array([[1, 2, 3]]), np.array([[4, 5, 6], [7, 8, 9]])
    C = U.batched_coordinates([a, b])
    assert C.dtype == torch.int32 and C.tolist() == [[0, 1, 2, 3], [1, 4, 5, 6], [1, 7, 8, 9]]
    C2, F2 = U.sparse_collate([a, b], [np.ones((1, 1)), np.zeros((2, 1))])
    assert torch.equal(C, C2) and F2[:, 0].tolist() == [1.0, 0.0, 0.0]


def test_hashes_match_reference_goldens():
    z = np.load(os.path.join(G, "hash.npz"))
    M = int(z["M"])
    split = np.split(z["index"], np.cumsum(z["group"])[:-1])
    assert np.array_equal(misc._exhaustive_hash(split, M), z["exhaustive"])
    assert np.array_equal(misc._neg_hash(z["i1"], z["i2"], M), z["neg"])
    assert np.array_equal(misc._hash(z["arr"], 97), z["hash_arr"])
    assert np.array_equal(synthetic.exhaustive_hash(z["index"], z["group"], M), z["exhaustive"])


def test_synthetic_train_batch_contract():
    s = synthetic.make_train_sample(5, num_neighborhood=2, n_boxes=10)
    b = synthetic.collate_train([s, synthetic.make_train_sample(6, num_neighborhood=2, n_boxes=10)])
    C = b["sinput_C"]
    assert C.dtype == torch.int32 and C.shape[1] == 4 and b["sinput_F"].shape == (len(C), 1)
    assert C[:, 0].max().item() == 2 * 3 - 1                       # batch id increments per cloud
    key = O_pack(C.numpy())
    assert len(np.unique(key)) == len(key), "coordinates are unique within the batch"
    g, idx, fl = b["group"].numpy(), b["index"].numpy(), b["finest_flag"].numpy()
    assert g.sum() == len(idx) == len(fl) and g.min() >= 2 and g.max() <= 5 + 5 * 2
    starts = np.concatenate([[0], np.cumsum(g)[:-1]])
    assert (np.add.reduceat(fl.astype(int), starts) == 1).all(), "exactly one finest member per group"
    assert idx.max() < len(C) and sum(b["batch_lengths"]) == len(C)
    split = np.split(idx, np.cumsum(g)[:-1])
    assert np.array_equal(b["index_hash"], LO.exhaustive_hash(split, len(C)))
    f16 = synthetic.collate_train([synthetic.make_train_sample(5, num_neighborhood=6, n_boxes=10, group_mode="fixed16")])
    assert (f16["group"] == 16).all() and len(f16["group"]) > 0


def O_pack(C):
    from oracle.me_oracle import pack_keys
    return pack_keys(C)


def test_eval_pair_contract_and_registry():
    p = synthetic.make_eval_pair(0, n_boxes=10)
    for k in (0, 1):
        assert p[f"sinput{k}_C"].shape[1] == 4 and (p[f"sinput{k}_C"][:, 0] == 0).all()
        assert len(p[f"pcd{k}"][0]) == len(p[f"sinput{k}_C"]) == len(p[f"sinput{k}_F"])
    from gcl_amd.model import load_model
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    assert sum(p.numel() for p in m.parameters()) == 8753408
    fat = load_model("ResUNetFatBN")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    assert fat.conv1_tr.kernel.shape == (32 + 128, 128)


def test_prefetched_draws_follow_the_serial_random_stream():
    """train_steps() draws batch i+1 on a helper thread; the draws must equal those of a serial loop."""
    import types
    import numpy as np
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, draw_selections, make_config
    tr = object.__new__(FinestContrastiveLossTrainer)
    tr.config = make_config(batch_size=2, num_pos_per_batch=8, num_hn_samples_per_batch=16)
    seen = []
    tr.train_step = types.MethodType(lambda self, b, draws=None: seen.append(draws) or len(seen), tr)
    batches = [{"group": list(range(40 + i)), "sinput_C": list(range(500 + 7 * i))} for i in range(5)]
    np.random.seed(3)
    out = list(tr.train_steps(batches))
    np.random.seed(3)
    ref = [draw_selections(len(b["group"]), len(b["sinput_C"]), 16, 32) for b in batches]
    assert out == [1, 2, 3, 4, 5]
    for got, want in zip(seen, ref):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_train_steps_groups_iter_size_batches_and_keeps_the_random_stream():
    """config.iter_size = 2: one optimizer step per two consecutive batches (lib/colocation_trainer.py:838), the draws of
    every batch still made in batch order; a trailing odd batch is dropped like ``len(loader) // iter_size``."""
    import types
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, draw_selections, make_config
    tr = object.__new__(FinestContrastiveLossTrainer)
    tr.config = make_config(batch_size=2, num_pos_per_batch=8, num_hn_samples_per_batch=16, iter_size=2)
    seen = []
    tr.train_step = types.MethodType(lambda self, b, draws=None: seen.append((b, draws)) or len(seen), tr)
    batches = [{"group": list(range(40 + i)), "sinput_C": list(range(500 + 7 * i))} for i in range(5)]
    np.random.seed(3)
    assert list(tr.train_steps(batches)) == [1, 2]
    np.random.seed(3)
    ref = [draw_selections(len(b["group"]), len(b["sinput_C"]), 16, 32) for b in batches[:4]]
    flat = [d for _, ds in seen for d in ds]
    assert [len(b) for b, _ in seen] == [2, 2] and seen[1][0][0] is batches[2]
    for got, want in zip(flat, ref):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_generator_groups_equal_the_oracle_restatement():
    """The synthetic generator's vectorised group builder (cKDTree) against oracle/colocation_oracle.py, the per-point
    restatement of get_matching_indices_colocation (util/pointcloud.py:69-132) -- with the reference's float64
    transform of the neighbour clouds and with the float32 centre-frame points the device builder receives."""
    from oracle.colocation_oracle import colocation_groups
    xyz, cmpl, _, _, group, index, finest, list_M = synthetic.make_train_sample(13, 0.3, num_neighborhood=2, n_boxes=8)
    r = synthetic.sample_search_radius(13, 0.3, 2)
    for cf in (None, [synthetic._apply(list_M[j], x) for j, x in enumerate(cmpl)]):
        og, oi, of = colocation_groups(xyz, cmpl, list_M, r, K=5, nghb_cf=cf)
        assert og == list(group) and oi == list(index) and of == list(finest)
    assert len(group) > 100


def test_native_legacy_choice_is_numpy_bit_for_bit():
    """gcl_host_legacy_choice (host code of the C-ABI library, no GPU): np.random.choice(n, k, replace=False) of the global
    RandomState -- same indices AND the same stream position afterwards -- so that a seeded training run still draws
    what the reference draws (lib/colocation_trainer.py:457, :506-507)."""
    from gcl_amd.lib.colocation_trainer import draw_selections, legacy_choice
    for seed, n, k in [(0, 530321, 1024), (1, 5000, 5000), (2, 19699, 1024), (3, 4096, 1), (4, 100000, 0), (5, 70001, 77),
                       (6, 65536, 100), (7, 65537, 100), (8, 8192, 1024), (9, 8192, 1025), (10, 4099, 512), (11, 1 << 20, 3)]:
        np.random.seed(seed)
        np.random.rand(seed * 5)                 # an arbitrary position inside the 624-word state block
        a, ra = np.random.choice(n, k, replace=False), np.random.rand(3)
        np.random.seed(seed)
        np.random.rand(seed * 5)
        b, rb = legacy_choice(n, k), np.random.rand(3)
        assert np.array_equal(a, b) and np.array_equal(ra, rb), (seed, n, k)
    np.random.seed(11)
    got = draw_selections(20000, 530000, 1024, 1024)
    np.random.seed(11)
    want = (np.random.choice(20000, 1024, replace=False), np.random.choice(530000, 1024, replace=False),
            np.random.choice(530000, 1024, replace=False))
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want))


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus 2` without a launcher on a box with fewer than 2 devices: non-zero exit, no JSON line
    (it used to time one GPU and print it)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GCL_BENCH_SINGLE_DEVICE")}
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices visible")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_secondary_figures_cannot_take_the_headline_down():
    """bench.py measures configs[1] / configs[4] (`secondary`) in a CHILD process (round 5: a memory fault in a new kernel
    there once ended the process before the headline line was printed).  Whatever the child does -- here: no GPU, so it
    cannot even measure -- the parent gets a dict back, never an exception, and the child prints exactly one JSON line."""
    import importlib.util
    import json
    import subprocess
    import torch
    if torch.cuda.is_available():
        pytest.skip("meaningful on a box without a GPU (on a GPU box the -m gpu tests and the bench itself cover it)")
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    res = bench.secondary_in_child(timeout_s=240)
    assert isinstance(res, dict) and "error" in res
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--secondary-worker"], capture_output=True, text=True,
                       timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "error" in json.loads(lines[0])


def test_counter_figures_are_quoted_only_for_the_sources_they_were_collected_on(tmp_path, monkeypatch):
    """profiles/pmc_summary.json is stamped with a hash of the training step's kernel sources (_lib.source_hash); bench.py's
    roofline quotes `traffic` / `mfma_busy` from it only when its own sources carry the same hash (VERDICT round 4, weak #9:
    a pasted number must not outlive the kernels it was measured on)."""
    import importlib.util
    import json
    from gcl_amd import _lib
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    h = _lib.source_hash()
    assert len(h) == 16 and h == _lib.source_hash()
    committed = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))
    assert "_csrc_sha16" in committed
    prof = [("k_conv_fwd_dma<2,true,false>", 0.15, None, 1000000, 128, 128, 70000, 70000, 27)]
    for stamp, quoted in ((h, True), ("0" * 16, False)):
        root = tmp_path / stamp
        (root / "profiles").mkdir(parents=True)
        json.dump({"_csrc_sha16": stamp, "k_conv_fwd_dma<2,true,false>": {"hbm_bytes_per_launch": 123456, "mfma_busy": 0.25}},
                  open(root / "profiles" / "pmc_summary.json", "w"))
        monkeypatch.setattr(bench, "ROOT", str(root))
        r = bench.roofline_of(prof, "fp16x3")
        assert (r["traffic"], r["mfma_busy"]) == ((123456, 0.25) if quoted else (None, None)), (stamp, r["traffic"])
        assert ("collected on these kernel sources" in r["note"]) == quoted


def test_bench_dump_outputs_are_float_arrays_within_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: what the last timed step computed (loss, its three parts, the voxel count, the model's state
    after the update) as <name>.npy in float32 / float64 within 64 MB; over the budget, a seeded sample of each large array
    that takes the same positions in every run."""
    import importlib.util
    from gcl_amd.model import load_model
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    torch.manual_seed(0)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    loss, parts = torch.tensor(1.5), (torch.tensor(0.5), torch.tensor(0.25), torch.tensor(0.75))
    bench.dump_outputs(str(tmp_path / "all"), loss, parts, 530321, model)
    files = {p.name: np.load(p) for p in (tmp_path / "all").iterdir()}
    sd = {k: v for k, v in model.state_dict().items() if v.is_floating_point()}
    assert set(files) == {"loss.npy", "loss_parts.npy", "active_voxels.npy"} | {f"state.{k}.npy" for k in sd}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_LIMIT_BYTES == 64 * 1000 * 1000
    assert float(files["loss.npy"]) == 1.5 and files["loss_parts.npy"].tolist() == [0.5, 0.25, 0.75]
    assert float(files["active_voxels.npy"]) == 530321
    assert all(np.array_equal(files[f"state.{k}.npy"], v.numpy()) for k, v in sd.items())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4_000_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, parts, 530321, model)
    a = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    b = {p.name: np.load(p) for p in (tmp_path / "b").iterdir()}
    assert a.keys() == files.keys() and sum(x.nbytes for x in a.values()) <= 4_000_000
    assert all(np.array_equal(a[k], b[k]) for k in a)
    k = "state.block4.conv1.kernel.npy"
    assert a[k].size < files[k].size and np.isin(a[k], files[k]).all()


def test_registration_stage_views_and_host_copies():
    """Host pieces of the one-call registration path (gcl_amd/scripts/SC2_PCR.py) and of the eval loop's copies: the stage
    views carve typed tensors out of ONE byte buffer at the recorded offsets; host_to_device is the identity off the GPU."""
    import numpy as np
    import torch
    from gcl_amd.scripts.SC2_PCR import _Stages
    from gcl_amd.lib.eval import host_to_device
    fields, off = {}, 0
    for name, count, dtype, shape in (("out", 16, torch.float32, (1, 4, 4)), ("seeds", 5, torch.int64, None),
                                      ("knn", 6, torch.int32, (2, 3)), ("best", 1, torch.int32, None)):
        fields[name] = (off, count, dtype, shape)
        off += (count * dtype.itemsize + 255) // 256 * 256
    buf = torch.zeros(off, dtype=torch.uint8)
    st = _Stages(buf, fields)
    st["out"][0, 3, 3] = 1.0
    st["seeds"][:] = torch.arange(5)
    st["knn"][1, 2] = 7
    buf[fields["best"][0]:fields["best"][0] + 4].view(torch.int32)[0] = 3
    assert st["out"].shape == (1, 4, 4) and float(buf[60:64].view(torch.float32)[0]) == 1.0
    assert st["seeds"].dtype == torch.int64 and st["seeds"].tolist() == [0, 1, 2, 3, 4]
    assert st["knn"].shape == (2, 3) and int(st["knn"][1, 2]) == 7 and int(st["best"]) == 3 and st["best"].dim() == 0
    assert set(st.keys()) == {"out", "seeds", "knn", "best"}
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    t = host_to_device(a, "cpu")
    assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and np.array_equal(t.numpy(), a)


def test_module_walk_cache_sees_a_replaced_submodule():
    """ResUNet2._module_list caches the module walk of the inference guards (``any(m.training ...)``): a sub-module
    REPLACED under the same name (same counts everywhere) must invalidate it -- a replaced norm layer left in training
    mode has to stop the eval plan."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.model import load_model
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    m.eval()
    first = m._module_list()
    assert m._module_list() is first                       # cached
    assert not any(x.training for x in first)
    new = ME.MinkowskiBatchNorm(32, momentum=0.05)          # fresh modules are in training mode
    m.block1.norm1 = new
    mods = m._module_list()
    assert mods is not first and any(x is new for x in mods) and any(x.training for x in mods)
    n = m._n_parameters()
    m.block1.conv1.kernel = torch.nn.Parameter(m.block1.conv1.kernel.detach().clone())       # same count, new identity
    assert m._module_list() is not mods and m._n_parameters() == n


def test_twin_eval_pair_contract():
    """synthetic.make_twin_eval_pair (bench.py secondary, configs[4]): unique voxels per cloud, the shared part of cloud 0 moved
    by T_gt IS in cloud 1 with the same input feature, and (up to a handful of chance coincidences) no voxel of cloud 0's
    unrelated part maps onto cloud 1."""
    from gcl_amd import synthetic
    p = synthetic.make_twin_eval_pair(7, 0.4, n_boxes=15)
    C0, C1 = p["sinput0_C"].numpy(), p["sinput1_C"].numpy()
    assert len(np.unique(C0, axis=0)) == len(C0) and len(np.unique(C1, axis=0)) == len(C1) and len(C0) == len(C1)
    sh = np.round(p["T_gt"].numpy()[:3, 3] / 0.3).astype(np.int64)
    assert (sh % 8 == 0).all() and np.allclose(p["T_gt"].numpy()[:3, :3], np.eye(3))
    key1 = {tuple(c): i for i, c in enumerate(C1[:, 1:].tolist())}
    twins = [(i, key1[tuple((c + sh).tolist())]) for i, c in enumerate(C0[:, 1:].astype(np.int64)) if tuple((c + sh).tolist()) in key1]
    assert p["shared_voxels"] <= len(twins) <= 1.005 * p["shared_voxels"] and 0.35 * len(C0) < len(twins) < 0.45 * len(C0)
    i0, i1 = np.array(twins).T
    same_f = (p["sinput0_F"].numpy()[i0] == p["sinput1_F"].numpy()[i1]).reshape(-1)
    assert int(same_f.sum()) >= p["shared_voxels"]
    moved = p["pcd0"][0].numpy()[i0[same_f]] + p["T_gt"].numpy()[:3, 3]
    assert np.abs(moved - p["pcd1"][0].numpy()[i1[same_f]]).max() < 1e-4
    # metric points sit in their voxels (the float32 shift puts a point on a voxel face over the edge now and then)
    assert (np.floor(p["pcd1"][0].numpy() / 0.3).astype(np.int32) == C1[:, 1:]).all(axis=1).mean() > 0.99


def test_raw_sample_is_what_make_train_sample_voxelises():
    """synthetic.make_raw_sample (the input of build_batch_gpu / train_from_scans) replays make_train_sample's draws: voxelising
    its clouds gives the sample's coordinates, and raw_sample_jitter the centre cloud's feature jitter."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd import synthetic
    raw = synthetic.make_raw_sample(33, 0.3, num_neighborhood=2, n_boxes=8)
    xyz_th, xyz_cmpl_th, coords, feats, group, index, finest, list_M = synthetic.make_train_sample(33, 0.3, num_neighborhood=2, n_boxes=8)
    assert len(raw["xyz"]) == 3 and all(np.allclose(a, b) for a, b in zip(raw["list_M"], list_M))
    for c, x in enumerate(raw["xyz"]):
        q, sel = ME.utils.sparse_quantize(x / 0.3, return_index=True)
        assert np.array_equal(np.floor(x[sel] / 0.3).astype(np.int32), coords[c])
    assert abs(raw["radius"] - synthetic.sample_search_radius(33, 0.3, 2)) < 1e-12
    j = synthetic.raw_sample_jitter([raw])(0, len(coords[0]))
    want = feats[0] - 1.0
    assert (j is None and not want.any()) or np.allclose(j, want, atol=1e-7)
    assert synthetic.raw_sample_jitter([raw])(0, len(coords[0])) is None or \
        np.array_equal(synthetic.raw_sample_jitter([raw])(0, len(coords[0])), j)          # a raw sample can be fed again
