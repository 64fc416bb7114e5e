"""gcl_amd/lib/augment.py against the reference's own draws (tests/golden/augment_s0.npz, written by
tests/golden/make_augment_golden.py from ``sample_random_trans`` / ``follow_presampled_trans``): the same rotations from the
same generator in the same order, the translation a fp64 centroid gives, and the ground truth followed through them."""
import os
import random

import numpy as np
import pytest

from gcl_amd.lib import augment

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_s0.npz"))


def _replay():
    randg = np.random.RandomState()
    randg.seed(int(G["seed"]))
    return randg, [augment.sample_rotation(randg, float(r)) for r in G["ranges"]]


def test_rotations_match_the_reference_and_leave_the_generator_where_it_does():
    randg, Rs = _replay()
    assert len(Rs) == 2
    for R, T0, Tc in zip(Rs, G["T0"], G["Tc"]):
        # two fp64 evaluations (Rodrigues / expm) of one matrix with entries <= 1: a cap, not a measurement
        assert np.abs(R - T0[:3, :3]).max() <= 1e-12
        assert np.array_equal(Tc[:3, :3], T0[:3, :3])          # the neighbour follows the centre's rotation
        augment.checked_rotation(R)
    assert np.abs(Rs[0] - np.eye(3)).max() > 0.1                # 360: a real turn; np.pi / 4 "degrees": a fraction of one
    assert 0 < np.abs(Rs[1] - np.eye(3)).max() < 0.01
    state = randg.get_state()
    assert state[0] == "MT19937" and np.array_equal(state[1], G["state_key"]) and state[2] == int(G["state_pos"])
    assert [state[3], state[4]] == G["state_gauss"].tolist()


def test_translation_from_an_fp64_centroid_is_within_the_float32_mean_s_error():
    """The reference's centroid is a float32 np.mean; ours is a fp64 sum.  Float32 recursive summation of P terms is off by at
    most (P - 1) 2^-24 max|x| per component, carried through R: (P - 1) 2^-24 max|x| sum_j |R_ij|."""
    _, Rs = _replay()
    for cloud, Ts in ((G["center"], G["T0"]), (G["nghb"], G["Tc"])):
        P = len(cloud)
        assert 1000 < P <= 2000 and cloud.dtype == np.float32
        centroid = cloud.astype(np.float64).sum(axis=0) / P
        for R, T in zip(Rs, Ts):
            t = R @ -centroid
            bound = (P - 1) * 2.0 ** -24 * np.abs(cloud).max() * np.abs(R).sum(axis=1)
            print("translation error", np.abs(t - T[:3, 3]), "bound", bound)
            assert (np.abs(t - T[:3, 3]) <= bound).all()


def test_list_M_composition_is_the_reference_s_bit_for_bit():
    for T0, Tc, want in zip(G["T0"], G["Tc"], G["M_out"]):
        got = augment.follow_list_M(T0, G["M_in"], Tc)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        scaled = augment.follow_list_M(T0, G["M_in"], Tc, 0.9)
        assert np.array_equal(scaled[:3, :3], want[:3, :3]) and np.array_equal(scaled[:3, 3], 0.9 * want[:3, 3])
        # a pair's transform goes the other way round: cloud 0 -> cloud 1 (lib/data_loaders.py:479)
        assert np.array_equal(augment.follow_pair_trans(Tc, T0, G["M_in"]), want)


def test_draw_scale_makes_the_reference_s_two_draws():
    """lib/colocation_data_loader.py:362-364: ``random.random() < 0.95`` and then ``min + (max - min) * random.random()``."""
    seen = set()
    for seed in range(60):
        a, b = random.Random(seed), random.Random(seed)
        got = augment.draw_scale(a, 0.8, 1.2)
        if b.random() < 0.95:
            assert got == 0.8 + (1.2 - 0.8) * b.random() and 0.8 <= got < 1.2
        else:
            assert got is None
        assert a.getstate() == b.getstate()
        seen.add(got is None)
    assert seen == {True, False}
    random.seed(5)
    want = random.random() < 0.95 and 0.8 + 0.4 * random.random()
    random.seed(5)
    assert augment.draw_scale(random, 0.8, 1.2) == want


def test_bad_keys_are_named():
    with pytest.raises(ValueError, match="rotation"):
        augment.checked_rotation(np.eye(3) * 1.001)
    with pytest.raises(ValueError, match="rotation"):
        augment.checked_rotation(np.eye(4))
    R = np.eye(3)
    R[0, 1] = 5e-7                      # |R^T R - I| = 5e-7: inside the 1e-6 the builders accept
    augment.checked_rotation(R)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            augment.checked_scale(bad)
