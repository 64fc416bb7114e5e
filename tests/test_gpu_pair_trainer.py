"""The four pair trainers (gcl_amd/lib/trainer.py) on the GPU: one optimizer step against the fp64 oracle network
(oracle.me_oracle.resunet_forward, two training-mode passes of one state) + the CPU restatement of the losses
(tests/pair_loss_oracle.py) + plain SGD; gradient accumulation; no host synchronisation inside the loss.

Bounds of one step = the bounds test_resunet_forward_backward_vs_oracle holds ONE pass to (kernel gradients 2e-3,
BatchNorm parameters 1e-2, running statistics 1e-4 rel-L2; loss terms 1e-4 relative, that test's feature tolerance: the
losses are O(1)-Lipschitz in the features): a pair step is two such passes plus a loss whose own error is 1e-5, so it
gets no extra margin.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import me_oracle as O             # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/pair_loss_oracle.py
import pair_loss_oracle as PO                                          # noqa: E402

DEV = "cuda:0"
TRAINERS = ["ContrastiveLossTrainer", "HardestContrastiveLossTrainer", "TripletLossTrainer", "HardestTripletLossTrainer"]
CFG = dict(batch_size=1, num_pos_per_batch=256, num_hn_samples_per_batch=256, triplet_num_pos=256, triplet_num_hn=512,
           triplet_num_rand=1024, lr=0.1, momentum=0.8, weight_decay=1e-4)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def pair_batch(seed=3, max_points=1500):
    from gcl_amd import synthetic
    return synthetic.make_train_pair(seed, voxel_size=0.3, max_points=max_points)


def model_and_state(seed, k1):
    from gcl_amd.model import load_model
    torch.manual_seed(seed)
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=k1, D=3).to(DEV)
    with torch.no_grad():                      # non-trivial BN affine parameters
        for name, p in m.named_parameters():
            if name.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            elif name.endswith("bn.bias"):
                p.uniform_(-0.1, 0.1)
    st = {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items() if "num_batches" not in k}
    return m, st


def make_trainer(name, k1, model=None, **over):
    from gcl_amd.lib import trainer as T
    from gcl_amd.lib.colocation_trainer import make_config
    cfg = make_config(conv1_kernel_size=k1, **dict(CFG, **over))
    return getattr(T, name)(cfg, model=model, device=DEV)


_ORACLE = {}


def oracle_passes(k1, batch, st):
    """Two training-mode fp64 passes of ONE state (cloud 0 first: the running statistics are updated twice); cached per
    conv1_kernel_size -- the four trainers start from the same state and see the same batch."""
    if k1 not in _ORACLE:
        so = {k: v.clone().requires_grad_("running" not in k) for k, v in st.items()}
        F0 = O.resunet_forward(so, batch["sinput0_C"].numpy(), batch["sinput0_F"].double(), k1, True, True, 0.05)
        F1 = O.resunet_forward(so, batch["sinput1_C"].numpy(), batch["sinput1_F"].double(), k1, True, True, 0.05)
        _ORACLE[k1] = (so, F0, F1)
    return _ORACLE[k1]


def oracle_loss(name, F0, F1, pairs, draws, cfg, mined):
    """(scalar that is back-propagated, reported parts) from the restatement, at the product's mined rows."""
    if name == "ContrastiveLossTrainer":
        pos, neg, _ = PO.contrastive_random_negative(F0, F1, pairs, draws, cfg.neg_thresh)
        return pos + cfg.neg_weight * neg, (pos, neg)
    if name == "HardestContrastiveLossTrainer":
        o = PO.hardest_contrastive(F0, F1, pairs, draws, cfg.pos_thresh, cfg.neg_thresh, mined=mined)
        return o["pos"] + cfg.neg_weight * o["neg"], (o["pos"], o["neg"])
    if name == "TripletLossTrainer":
        loss, pd, nd, _ = PO.triplet(F0, F1, pairs, draws, cfg.neg_thresh)
        return loss, (pd, nd)
    o = PO.hardest_triplet(F0, F1, pairs, draws, cfg.neg_thresh, mined=mined)
    return o["loss"], (o["pos_dist"], o["neg_dist"])


def product_mined_rows(name, F0, F1, pairs, draws):
    """The rows the product's mining kernel picks on the product's own features (None for the trainers that do not mine)."""
    from gcl_amd.lib.metrics import pdist_min
    if "Hardest" not in name:
        return None
    sel0, sel1, pos_sel = draws[:3]
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)
    _, a01 = pdist_min(F0, F1, "L2", rows_a=up(sample[:, 0]), rows_b=up(sel1))
    _, a10 = pdist_min(F1, F0, "L2", rows_a=up(sample[:, 1]), rows_b=up(sel0))
    return np.asarray(sel1)[a01.cpu().numpy()], np.asarray(sel0)[a10.cpu().numpy()]


@pytest.mark.parametrize("k1", [5, 3])
@pytest.mark.parametrize("name", TRAINERS)
def test_one_step_vs_fp64_oracle(name, k1):
    """The pair is one whole scan pair (15 k + 17 k voxels, batch_size 1), not a cropped one.  A parameter gradient is a
    discontinuous function of the features wherever a ReLU argument crosses zero, and the fp32 network differs from the
    fp64 oracle by ~1e-6 in its pre-activations: among the ~1e6 of them of a pass about one sits that close to zero and
    lands on the other side.  What one such flip does to a gradient falls with the number of rows that share the
    parameter: on a 1500-voxel crop (30 rows on the coarsest level) ONE pass measured 3e-3 .. 1e-2 against this oracle
    for some (crop, conv1_kernel_size) and 2e-6 for others -- the single-pass comparison itself, not the pair step, whose
    two live passes equal the sum of two single passes to 3.5e-8 on every one of those inputs.  A whole scan has ten
    times the rows per level, as the clouds test_resunet_forward_backward_vs_oracle's bounds were set on."""
    batch = pair_batch(max_points=None)
    pairs = batch["correspondences"].numpy()
    model, st = model_and_state(0, k1)
    tr = make_trainer(name, k1, model)
    cfg = tr.config
    np.random.seed(11)
    draws = tr.draw_for(batch)
    seen = {}
    inner = tr.pair_loss

    def spy(F0, F1, pos_pairs, d):
        seen["F0"], seen["F1"] = F0.detach().clone(), F1.detach().clone()
        return inner(F0, F1, pos_pairs, d)

    tr.pair_loss = spy
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss, parts, n_rows = tr.train_step(batch, draws)
    assert n_rows == len(batch["sinput0_C"]) + len(batch["sinput1_C"])

    so, F0o, F1o = oracle_passes(k1, batch, st)
    e0, e1 = rel_l2(seen["F0"].cpu(), F0o.detach()), rel_l2(seen["F1"].cpu(), F1o.detach())
    print(f"[{name} k{k1}] features rel-L2 {e0:.2e} {e1:.2e}")
    assert e0 < 1e-4 and e1 < 1e-4
    mined = product_mined_rows(name, seen["F0"], seen["F1"], pairs, draws)
    if mined is not None:
        # an index is a discontinuous function of the features: the loss is evaluated at the PRODUCT's rows, each of which
        # must be within 1e-5 of the oracle's own row minimum
        sel0, sel1, pos_sel = draws[:3]
        sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel)]
        d01, _, _ = PO.mine(F0o, F1o, sample[:, 0], sel1)
        d10, _, _ = PO.mine(F1o, F0o, sample[:, 1], sel0)
        i0, i1 = torch.from_numpy(sample[:, 0].copy()), torch.from_numpy(sample[:, 1].copy())
        at01 = PO.dist(F0o.detach()[i0], F1o.detach()[torch.from_numpy(mined[0])]).numpy()
        at10 = PO.dist(F1o.detach()[i1], F0o.detach()[torch.from_numpy(mined[1])]).numpy()
        worst = max(float((at01 - d01).max()), float((at10 - d10).max()))
        print(f"[{name} k{k1}] mined rows: worst distance above the oracle's row minimum {worst:.2e}")
        assert worst <= 1e-5
    for p in so.values():
        p.grad = None
    lo, parts_o = oracle_loss(name, F0o, F1o, pairs, draws, cfg, mined)
    lo.backward(retain_graph=True)
    for what, got, ref in [("loss", loss, lo)] + [(f"part{i}", g, r) for i, (g, r) in enumerate(zip(parts, parts_o))]:
        got, ref = got.detach(), ref.detach()
        err = abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-30)
        print(f"[{name} k{k1}] {what}: {float(got):.8g} vs {float(ref):.8g} (rel {err:.2e})")
        assert err < 1e-4, what
    worst = {}
    for pname, p in model.named_parameters():
        e = rel_l2(p.grad.cpu(), so[pname].grad)
        kind = "bn" if ".bn." in pname else "kernel"
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e < (1e-2 if kind == "bn" else 2e-3), (pname, e)
        # ONE plain SGD step with the accumulated gradient (first step: the momentum buffer is the gradient itself)
        want = before[pname] - cfg.lr * (p.grad + cfg.weight_decay * before[pname])
        assert torch.allclose(p.detach(), want, rtol=1e-6, atol=1e-7), pname
    print(f"[{name} k{k1}] worst parameter-gradient rel-L2: {worst}")
    for bname, b in model.named_buffers():
        if "running" in bname:                 # BOTH updates, cloud 0 first
            assert rel_l2(b.cpu(), so[bname]) < 1e-4, bname


@pytest.mark.parametrize("name", TRAINERS)
def test_iter_size_two_accumulates_the_mean_gradient(name):
    """lr = 0: a step over two pair batches leaves in p.grad the mean of the two single-batch gradients -- one fp32 add per
    element apart, plus the order of the loss backward's atomics: 1e-5 rel-L2."""
    batches = [pair_batch(3), pair_batch(4)]
    model, _ = model_and_state(0, 5)
    tr = make_trainer(name, 5, model, lr=0.0, weight_decay=0.0, iter_size=2)
    np.random.seed(5)
    draws = [tr.draw_for(b) for b in batches]
    singles = []
    for b, d in zip(batches, draws):
        tr.train_step(b, d)
        singles.append([p.grad.detach().clone() for p in model.parameters()])
    loss, parts, _ = tr.train_step(batches, draws)
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).cpu()
    want = (flat(singles[0]).double() + flat(singles[1]).double()) / 2
    err = rel_l2(flat([p.grad for p in model.parameters()]), want)
    print(f"[{name}] accumulated vs mean of the single-batch gradients: rel-L2 {err:.2e}")
    assert err < 1e-5
    assert torch.isfinite(loss) and all(torch.isfinite(p) for p in parts)
    steps = list(tr.train_steps(batches + batches + batches[:1]))          # five batches: two steps, the fifth is dropped
    assert len(steps) == 2


@pytest.mark.parametrize("name", ["ContrastiveLossTrainer", "TripletLossTrainer", "HardestTripletLossTrainer"])
def test_loss_call_never_waits_for_the_host(name):
    """Four steps with torch's synchronisation debug mode armed around the loss call only: no device -> host copy, no stream
    wait.  (HardestContrastiveLossTrainer runs the existing contrastive_hardest_negative_loss unchanged, whose boolean-mask
    indexing does read a count back; moving it onto these kernels is a follow-up.)"""
    batch = pair_batch()
    model, _ = model_and_state(0, 5)
    tr = make_trainer(name, 5, model, lr=0.01)
    inner = tr.pair_loss
    caught = []

    def guarded(F0, F1, pos_pairs, d):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = inner(F0, F1, pos_pairs, d)
            caught.extend(w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return out

    tr.pair_loss = guarded
    np.random.seed(2)
    losses = [tr.train_step(batch)[0] for _ in range(4)]
    assert not caught, [str(w.message) for w in caught]
    assert all(np.isfinite(float(l)) for l in losses)
