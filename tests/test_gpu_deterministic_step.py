"""``deterministic_loss_backward``: the product path.  Two fresh trainers in ONE process -- the same seed, the same batches,
the same draws -- run three optimizer steps with the flag set; after every step the loss, every parameter, every BatchNorm
running statistic and every momentum buffer of the two are equal bit for bit (``torch.equal``).

FinestContrastiveLossTrainer with the default switches and with ``use_group_circle_loss``, on the small batches of
tests/test_gpu_trajectory.py's generator; HardestContrastiveLossTrainer and TripletLossTrainer on a small scan pair.  The flag
is off by default, and with ``use_hard_negative=False`` (a debug path of torch operators ending in ``index_add_``) it is
refused, not silently ignored."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 3
POS, HN = 64, 256


def _snapshot(tr, loss):
    out = {"loss": loss.detach().clone()}
    for k, v in tr.model.state_dict().items():                       # parameters, running_mean / running_var, step counters
        out["state." + k] = v.detach().clone()
    for i, p in enumerate(tr.model.parameters()):
        b = tr.optimizer.state[p].get("momentum_buffer")
        assert b is not None
        out[f"momentum.{i}"] = b.detach().clone()
    return out


def _assert_equal(a, b, what):
    assert a.keys() == b.keys()
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, (what, len(diff), diff[:6])
    assert all(torch.isfinite(v.float()).all() for v in a.values()), what


def _run_twice(make, batches, draws):
    """Two trainers one after the other, each from torch.manual_seed(0): the snapshots after every step."""
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        tr = make()
        snaps = []
        for i in range(STEPS):
            loss = tr.train_step(batches[i % len(batches)], draws[i])[0]
            snaps.append(_snapshot(tr, loss))
        torch.cuda.synchronize()
        runs.append(snaps)
    for i in range(STEPS):
        _assert_equal(runs[0][i], runs[1][i], f"step {i}")
    # the steps did something: the parameters moved, and the loss saw the flag's path (a finite, non-zero value)
    moved = [k for k in runs[0][0] if k.startswith("state.") and not torch.equal(runs[0][0][k], runs[0][STEPS - 1][k])]
    assert len(moved) > 10 and float(runs[0][0]["loss"]) != 0


_CACHE = {}


def _gcl_batches():
    if "gcl" not in _CACHE:
        from gcl_amd import synthetic
        _CACHE["gcl"] = [synthetic.collate_train([synthetic.make_train_sample(s, num_neighborhood=1, n_boxes=10)])
                         for s in (31, 32)]
    return _CACHE["gcl"]


def _pair_batch():
    if "pair" not in _CACHE:
        from gcl_amd import synthetic
        _CACHE["pair"] = synthetic.make_train_pair(3, voxel_size=0.3, max_points=1500)
    return _CACHE["pair"]


@pytest.mark.parametrize("circle", (False, True))
def test_finest_contrastive_trainer_repeats_bit_for_bit(circle):
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    batches = _gcl_batches()
    cfg = make_config(batch_size=1, num_pos_per_batch=POS, num_hn_samples_per_batch=HN, use_group_circle_loss=circle,
                      deterministic_loss_backward=True)
    make = lambda: FinestContrastiveLossTrainer(cfg, device=DEV)
    np.random.seed(5)
    probe = make()
    draws = [probe._draw_for(batches[i % len(batches)]) for i in range(STEPS)]
    _run_twice(make, batches, draws)


@pytest.mark.parametrize("name", ("HardestContrastiveLossTrainer", "TripletLossTrainer"))
def test_pair_trainers_repeat_bit_for_bit(name):
    from gcl_amd.lib import trainer as T
    from gcl_amd.lib.colocation_trainer import make_config
    batch = _pair_batch()
    cfg = make_config(batch_size=1, num_pos_per_batch=256, num_hn_samples_per_batch=256, triplet_num_pos=256,
                      triplet_num_hn=512, triplet_num_rand=1024, deterministic_loss_backward=True)
    make = lambda: getattr(T, name)(cfg, device=DEV)
    np.random.seed(5)
    probe = make()
    draws = [probe.draw_for(batch) for _ in range(STEPS)]
    _run_twice(make, [batch], draws)


def test_the_flag_is_off_by_default_and_refuses_the_random_negative_debug_path():
    from gcl_amd.lib.colocation_trainer import (DEFAULT_CONFIG, FinestContrastiveLossTrainer, finest_contrastive_loss,
                                                make_config)
    assert make_config().deterministic_loss_backward is False and DEFAULT_CONFIG["deterministic_loss_backward"] is False
    with pytest.raises(ValueError, match="use_hard_negative"):
        FinestContrastiveLossTrainer(make_config(deterministic_loss_backward=True, use_hard_negative=False), device=DEV)
    b = _gcl_batches()[0]
    F = torch.zeros(len(b["sinput_C"]), 32, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="use_hard_negative"):
        finest_contrastive_loss(F, b["group"], b["index"], b.get("index_hash"), b["finest_flag"], use_hard_negative=False,
                                deterministic_loss_backward=True)


def test_functional_losses_with_the_flag_give_the_same_gradient_twice_and_match_the_default_path():
    """finest_contrastive_loss / location_contrastive_loss / location_circle_loss with the keyword: two calls give the same dF
    bit for bit, and it agrees with the atomic path's to rounding (1e-5 rel-L2: the bound of the atomic path itself)."""
    from gcl_amd.lib import colocation_trainer as CT
    b = _gcl_batches()[0]
    n = len(b["sinput_C"])
    g = torch.Generator().manual_seed(3)
    F0 = torch.nn.functional.normalize(torch.randn(n, 32, generator=g), dim=1).to(DEV)
    np.random.seed(7)
    draws = CT.draw_selections(len(b["group"]), n, POS, HN)
    cdraws = CT.draw_circle_selections(len(b["group"]), POS)

    def grad(fn, det, **kw):
        F = F0.clone().requires_grad_(True)
        with torch.cuda.device(DEV):
            terms = fn(F, b["group"], b["index"], b.get("index_hash"), b["finest_flag"], deterministic_loss_backward=det, **kw)
            sum(terms[:3]).backward()
        return F.grad.clone()

    cases = ((CT.finest_contrastive_loss, dict(draws=draws)), (CT.location_contrastive_loss, dict(draws=draws)),
             (CT.location_circle_loss, dict(draws=cdraws, points=b["sinput_C"][:, 1:], batch_lengths=b.get("batch_lengths"))))
    for fn, kw in cases:
        if fn is CT.location_circle_loss and kw["batch_lengths"] is None:
            kw["batch_lengths"] = [n]
        a, a2, d = grad(fn, True, **kw), grad(fn, True, **kw), grad(fn, False, **kw)
        assert torch.equal(a, a2), fn.__name__
        err = float((a.double() - d.double()).norm() / d.double().norm())
        assert d.abs().sum() > 0 and err < 1e-5, (fn.__name__, err)
