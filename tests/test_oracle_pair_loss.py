"""Pins tests/pair_loss_oracle.py (the CPU restatement of the pair family's losses) against golden vectors captured
from the reference's own code (tests/golden/make_pair_golden.py imported lib/trainer.py), and the host-side pieces of
the pair trainers that need no GPU: the np.random draw order, the count precondition, the pair batch."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/pair_loss_oracle.py
import pair_loss_oracle as PO                                          # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRIPLET = sorted(glob.glob(os.path.join(G, "triplet_*.npz")))
HARDEST = sorted(glob.glob(os.path.join(G, "hardest_triplet_*.npz")))
CONTRASTIVE = sorted(glob.glob(os.path.join(G, "contrastive_rand_*.npz")))


def load_features(z, dtype=torch.float32):
    """The fixtures keep the features as int16 on a 2^-14 grid: F = q / F_scale, exact in fp32."""
    s = float(z["F_scale"])
    return [(torch.from_numpy(z[k]).to(dtype) / s) for k in ("F0_q", "F1_q")]


def close(v, ref):
    v = v.detach() if torch.is_tensor(v) else v
    return abs(float(v) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))


def grads_close(t, ref):
    return np.allclose(t.grad.numpy(), ref, rtol=1e-5, atol=1e-7)


def triplet_draws(z):
    return (z["pos_sel"] if bool(z["subsampled"]) else None, z["rand_inds"], z["negatives"])


def hardest_draws(z):
    return (z["sel0"], z["sel1"]) + triplet_draws(z)


def test_fixture_set_is_complete():
    assert len(TRIPLET) == 4 and len(HARDEST) == 4 and len(CONTRASTIVE) == 3
    # across the set every mask has kept and dropped entries (the generator asserts the same for the hinges)
    both = lambda a: bool(a.any() and (~a).any())
    assert any(both(np.load(p)["rand_mask"]) for p in TRIPLET)
    assert any(both(np.load(p)["mask0"]) for p in HARDEST) and any(both(np.load(p)["mask1"]) for p in HARDEST)
    assert any(both(np.load(p)["keep"]) for p in CONTRASTIVE)
    assert all(float(np.load(p)["gap"]) >= 5e-6 for p in HARDEST)


@pytest.mark.parametrize("path", TRIPLET, ids=os.path.basename)
def test_triplet_loss_golden(path):
    z = np.load(path)
    F0, F1 = (f.requires_grad_(True) for f in load_features(z))
    loss, pos_dist, neg_dist, mask = PO.triplet(F0, F1, z["pairs"], triplet_draws(z), float(z["margin"]))
    assert close(loss, z["loss"]) and close(pos_dist, z["pos_dist"]) and close(neg_dist, z["neg_dist"])
    assert np.array_equal(mask, z["rand_mask"])
    loss.backward()
    assert grads_close(F0, z["grad0"]) and grads_close(F1, z["grad1"])


@pytest.mark.parametrize("path", HARDEST, ids=os.path.basename)
def test_hardest_triplet_loss_golden(path):
    z = np.load(path)
    F0, F1 = (f.requires_grad_(True) for f in load_features(z))
    o = PO.hardest_triplet(F0, F1, z["pairs"], hardest_draws(z), float(z["margin"]))
    assert close(o["loss"], z["loss"]) and close(o["pos_dist"], z["pos_dist"]) and close(o["neg_dist"], z["neg_dist"])
    for k in ("rand_mask", "mask0", "mask1", "neg01", "neg10"):
        assert np.array_equal(o[k], z[k]), k
    o["loss"].backward()
    assert grads_close(F0, z["grad0"]) and grads_close(F1, z["grad1"])


@pytest.mark.parametrize("path", CONTRASTIVE, ids=os.path.basename)
def test_contrastive_random_negative_loss_golden(path):
    z = np.load(path)
    F0, F1 = (f.requires_grad_(True) for f in load_features(z))
    pos, neg, keep = PO.contrastive_random_negative(F0, F1, z["pairs"], z["candidates"], float(z["neg_thresh"]))
    assert close(pos, z["pos"]) and close(neg, z["neg"])
    assert np.array_equal(keep, z["keep"]) and np.array_equal(z["candidates"][keep], z["neg_pairs"])
    (pos + neg).backward()
    assert grads_close(F0, z["grad0"]) and grads_close(F1, z["grad1"])


def test_seeded_draw_helpers_reproduce_the_recorded_draws():
    from gcl_amd.lib import trainer as T
    same = lambda a, b: (a is None and b is None) or np.array_equal(a, b)
    for path in TRIPLET:
        z = np.load(path)
        np.random.seed(int(z["np_seed"]))
        got = T.draw_triplet_selections(z["F1_q"].shape[0], len(z["pairs"]), int(z["num_pos"]), int(z["num_rand"]))
        assert all(same(a, b) for a, b in zip(got, triplet_draws(z))), path
    for path in HARDEST:
        z = np.load(path)
        np.random.seed(int(z["np_seed"]))
        got = T.draw_hardest_triplet_selections(z["F0_q"].shape[0], z["F1_q"].shape[0], len(z["pairs"]), int(z["num_pos"]),
                                                int(z["num_hn"]), int(z["num_rand"]))
        assert all(same(a, b) for a, b in zip(got, hardest_draws(z))), path
    for path in CONTRASTIVE:
        z = np.load(path)
        np.random.seed(int(z["np_seed"]))
        got = T.draw_rand_negative_pairs(len(z["pairs"]), z["F0_q"].shape[0], z["F1_q"].shape[0])
        assert got.dtype == np.int64 and np.array_equal(got, z["candidates"]), path


def test_unequal_random_triplet_counts_raise_value_error():
    """min(P, num_rand_triplet) anchors are paired one to one with min(N1, num_rand_triplet) negatives: unequal counts are
    an error that says so (the reference dies of a numpy broadcast error there)."""
    from gcl_amd.lib import trainer as T
    F0, F1 = torch.zeros(50, 32), torch.zeros(40, 32)
    pairs = np.stack([np.arange(20), np.arange(20)], 1)
    for fn in (T.triplet_loss, T.hardest_triplet_loss):
        with pytest.raises(ValueError, match="must be equal"):
            fn(F0, F1, pairs, num_rand_triplet=30)          # 20 anchors, 30 negatives
    batch = {"sinput0_C": torch.zeros(50, 4), "sinput1_C": torch.zeros(40, 4), "correspondences": torch.from_numpy(pairs)}
    from gcl_amd.lib.colocation_trainer import make_config
    cfg = make_config(batch_size=1, triplet_num_rand=30)
    assert (cfg.triplet_num_pos, cfg.triplet_num_hn, cfg.triplet_num_rand) == (256, 512, 30)
    assert make_config().triplet_num_rand == 1024
    for cls in (T.TripletLossTrainer, T.HardestTripletLossTrainer):
        tr = cls.__new__(cls)
        tr.config = cfg
        with pytest.raises(ValueError, match="must be equal"):
            tr.draw_for(batch)


def test_new_losses_have_no_cpu_path():
    """CPU tensors are an error, never a quiet fall-back to torch ops."""
    from gcl_amd.lib import trainer as T
    F0, F1 = torch.zeros(50, 32), torch.zeros(40, 32)
    pairs = np.stack([np.arange(20), np.arange(20)], 1)
    for call in (lambda: T.triplet_loss(F0, F1, pairs, num_rand_triplet=20),
                 lambda: T.hardest_triplet_loss(F0, F1, pairs, num_rand_triplet=20),
                 lambda: T.contrastive_random_negative_loss(F0, F1, pairs)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_make_train_pair_correspondences_are_within_the_radius_and_complete():
    from gcl_amd import synthetic as S
    vs, mult = 0.3, 1.5
    b = S.make_train_pair(5, voxel_size=vs, max_points=700)
    for k in ("sinput0_C", "sinput0_F", "sinput1_C", "sinput1_F", "correspondences", "T_gt", "len_batch"):
        assert k in b
    pairs = b["correspondences"]
    assert pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2 and len(pairs) > 100
    n0, n1 = len(b["sinput0_C"]), len(b["sinput1_C"])
    assert b["len_batch"] == [[n0, n1]] and n0 <= 700 and n1 <= 700
    assert b["sinput0_F"].shape == (n0, 1) and b["sinput1_F"].shape == (n1, 1)
    T = b["T_gt"].double().numpy()
    c0 = (b["sinput0_C"][:, 1:].double().numpy() + 0.5) * vs
    c1 = (b["sinput1_C"][:, 1:].double().numpy() + 0.5) * vs
    moved = c0 @ T[:3, :3].T + T[:3, 3]
    d = np.sqrt(((moved[:, None, :] - c1[None, :, :]) ** 2).sum(2))           # brute force [n0, n1]
    want = np.argwhere(d <= vs * mult)
    got = pairs.numpy()
    assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want)      # within the radius AND complete
    assert np.bincount(got[:, 0]).max() > 1                                   # one anchor, several partners


def test_invalid_arguments_are_rejected_before_any_launch():
    """Argument validation comes before any HIP call, so it runs without a GPU (as tests/test_abi.py does for the rest)."""
    import ctypes
    from gcl_amd import _lib as L
    lib = L.load()
    p8 = ctypes.c_void_p(8)
    err = lambda: lib.gcl_last_error()
    assert lib.gcl_pair_key_table(p8, 10, 5, p8, 48, None) == -1 and b"power of two" in err()
    assert lib.gcl_pair_key_table(p8, 100, 5, p8, 128, None) == -1 and b"power of two" in err()
    assert lib.gcl_pair_key_table(None, 10, 5, p8, 64, None) == -1 and b"null" in err()
    assert lib.gcl_pair_key_table(p8, 10, 0, p8, 64, None) == -1 and b"seed" in err()
    assert lib.gcl_pair_key_mask(p8, 2, p8, None, 10, 10, 5, p8, 64, None, p8, None) == -1 and b"col" in err()
    assert lib.gcl_pair_key_mask(p8, 0, None, p8, 10, 10, 5, p8, 64, None, p8, None) == -1 and b"candidate rows" in err()
    assert lib.gcl_pair_key_mask(p8, 0, p8, None, 5, 10, 5, p8, 64, None, p8, None) == -1 and b"fewer rows" in err()
    assert lib.gcl_triplet_fwd(p8, 5, p8, 5, 65, p8, p8, p8, None, 4, 0.4, p8, p8, None) == -1 and b"feature width" in err()
    assert lib.gcl_triplet_fwd(p8, 5, p8, 5, 32, p8, None, p8, None, 4, 0.4, p8, p8, None) == -1 and b"null" in err()
    assert lib.gcl_triplet_bwd(p8, 5, p8, 5, 32, p8, p8, p8, None, 4, p8, p8, None, p8, p8, None) == -1 and b"null" in err()
    assert lib.gcl_pair_terms_fwd(p8, 5, p8, 5, 32, p8, None, 4, 7, 0.0, 0.0, p8, p8, None) == -1 and b"mode" in err()
    assert lib.gcl_pair_terms_bwd(p8, 5, p8, 5, 32, p8, None, 4, 3, 0.0, 1e-7, p8, p8, p8, p8, p8, None) == -1 \
        and b"no backward" in err()
    assert lib.gcl_pair_terms_fwd(p8, 5, p8, 5, 0, p8, None, 4, 0, 0.0, 0.0, p8, p8, None) == -1 and b"feature width" in err()
    assert lib.gcl_triplet_scratch_len(0) == 0 and lib.gcl_triplet_scratch_len(1000) == 3000
    assert lib.gcl_pair_terms_scratch_len(-3) == 0 and lib.gcl_pair_terms_scratch_len(1000) == 1000
