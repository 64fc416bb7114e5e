"""Forward pass of the network's row-local head on the rows the loss reads (include/gcl_amd.h, "Touched rows": a list handed
to the plan BEFORE gcl_plan_forward; csrc/plan.hip).

The model, batch and lists of tests/test_gpu_head_touched_rows.py (ResUNetBN2C on one cloud of ~1.8 k voxels; 37 and 129 rows,
cap 128 and 256).  Every comparison of values is against the fp64 oracle: the pass on the rows of a list may be at most twice
as far from it as the dense pass is (the rule of the backward test).  Measured on an MI355X (rel-L2 against the oracle, dense
/ on the list): features of the listed rows 5.376e-07 / 5.376e-07 (37 rows) and 5.893e-07 / 5.893e-07 (129 rows); the rows of
conv1_tr and of final are bitwise the dense pass's at both lengths; over the 66 parameter tensors the largest ratio of the two
distances is 1.002 (final.kernel, 129 rows: 6.531e-07 -> 6.541e-07); the trainer's loss and its three parts are equal in both
orders, and the largest ratio over its parameter updates is 1.17 (final.bias: 1.01e-06 -> 1.19e-06).  The tests print all of it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_head_touched_rows import DEV, HEAD, _case, _dF, _rel_l2      # noqa: E402

gpu = pytest.mark.gpu
_CACHE = {}


def _a256(nbytes):
    return (nbytes + 255) // 256 * 256


def _pass(case, dF, rows=None, cap=None, before=True, state=None, buckets=None):
    """One training pass through the plan.  ``rows``: the list, announced before the forward pass or (``before=False``) only
    before the backward pass.  Returns a dict: F (the output), grads, the rows the head ran on in either pass, and -- for a
    forward pass on the list -- the compact tensors the pass parked in its arena."""
    import gcl_amd.MinkowskiEngine as ME
    lib = _lib.load()
    m, n = case["m"], case["n"]
    with torch.cuda.device(DEV):
        m.load_state_dict(state if state is not None else case["state0"])
        for p in m.parameters():
            p.grad = None
        x = ME.SparseTensor(case["F"], coordinates=case["C"], coordinate_manager=case["mgr"])
        plan = m.plan_for(x)
        assert plan is not None
        e = torch.zeros(0, dtype=torch.int64, device=DEV)
        goff = torch.zeros(1, dtype=torch.int64, device=DEV)
        if buckets is not None:
            plan.bucket_of_param, plan.on_bucket = buckets, (lambda b: None)
        try:
            if rows is not None and before:
                plan.touch_loss_rows(e, goff, e, rows.to(DEV), e, n, cap)
            out = m(x).F
            fwd_used = int(lib.gcl_plan_suffix_fwd_rows_used(plan.handle))
            F = out.detach().cpu().clone()
            saved = {}
            if fwd_used:      # arena order of the head on the list: input, conv1_tr, final, y, norm, then the dense output
                arena = out.grad_fn.run.arena
                o = out.data_ptr() - arena.data_ptr()
                view = lambda off, r, c: arena[off:off + r * c * 4].view(torch.float32).view(r, c).cpu().clone()
                o -= _a256(fwd_used * 4)
                saved["norm"] = view(o, fwd_used, 1)[:, 0]
                for name, c in (("y", 32), ("final", 32), ("conv1_tr", 64), ("x", 96)):
                    o -= _a256(fwd_used * c * 4)
                    saved[name] = view(o, fwd_used, c)
            elif rows is None:   # dense: conv1_tr, final, y (the output), norm
                arena = out.grad_fn.run.arena
                o = out.data_ptr() - arena.data_ptr()
                view = lambda off, r, c: arena[off:off + r * c * 4].view(torch.float32).view(r, c).cpu().clone()
                saved["norm"] = view(o + _a256(n * 32 * 4), n, 1)[:, 0]
                o -= _a256(n * 32 * 4)
                saved["final"] = view(o, n, 32)
                o -= _a256(n * 64 * 4)
                saved["conv1_tr"] = view(o, n, 64)
            if rows is not None and not before:
                plan.touch_loss_rows(e, goff, e, rows.to(DEV), e, n, cap)
            out.backward(dF.to(DEV))
            torch.cuda.synchronize()
        finally:
            plan.set_touched_rows(None, 0)
            plan.bucket_of_param = plan.on_bucket = None
        bwd_used = int(lib.gcl_plan_suffix_rows_used(plan.handle))
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
        return dict(F=F, grads=grads, fwd=fwd_used, bwd=bwd_used, saved=saved, plan=plan)


def _lists(case, k, seed):
    """dF of the loss's shape, its rows, cap, the dense pass and the oracle's gradients: once per (k, seed)."""
    key = (k, seed)
    if key not in _CACHE:
        n = case["n"]
        dF, rows = _dF(n, k, seed)
        cap = max(128, (k + 127) // 128 * 128)
        dense = _pass(case, dF)
        assert dense["fwd"] == 0 and dense["bwd"] == 0
        _CACHE[key] = dict(dF=dF, rows=rows, cap=cap, dense=dense, ref=_oracle_grads(case["so"], case["Fo"], dF))
    return _CACHE[key]


def _oracle_grads(so, Fo, dF):
    for v in so.values():
        v.grad = None
    Fo.backward(dF.double(), retain_graph=True)
    return {k: v.grad.clone() for k, v in so.items() if v.grad is not None}


def _check_features(tag, comp, dense, Fo, rows):
    """Rows outside the list exactly zero; on the list no further from the oracle than twice the dense pass."""
    r = rows.numpy()
    outside = np.ones(len(comp["F"]), bool)
    outside[r] = False
    assert not comp["F"][outside].any(), "a row outside the list is not zero"
    if len(r) == 0:
        return
    ref = Fo.detach()[r]
    e_dense, e_comp = _rel_l2(dense["F"][r], ref), _rel_l2(comp["F"][r], ref)
    print(f"[{tag}] features of the listed rows: rel-L2 vs fp64 oracle dense {e_dense:.3e}, on the list {e_comp:.3e}")
    assert e_comp <= 2 * e_dense, (e_dense, e_comp)


def _check_grads(tag, comp, dense, ref):
    worst = (0.0, None, 0.0, 0.0)
    for name, g in comp.items():
        assert torch.isfinite(g).all(), name
        e_dense, e_comp = _rel_l2(dense[name], ref[name]), _rel_l2(g, ref[name])
        if name in HEAD:
            print(f"[{tag}] {name}: rel-L2 vs fp64 oracle dense {e_dense:.3e}, on the list {e_comp:.3e}")
        if e_dense > 0 and e_comp / e_dense > worst[0]:
            worst = (e_comp / e_dense, name, e_dense, e_comp)
        assert e_comp <= 2 * e_dense, (name, e_dense, e_comp)
    print(f"[{tag}] largest e_comp / e_dense over {len(comp)} tensors: {worst[0]:.3f} ({worst[1]}: {worst[2]:.3e} -> {worst[3]:.3e})")


# ---------------------------------------------------------------------------------------------------------------
# 1. which path ran
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_a_list_before_the_forward_pass_takes_both_passes_and_none_or_a_long_one_neither():
    case = _case()
    n = case["n"]
    L = _lists(case, 37, 47)
    comp = _pass(case, L["dF"], L["rows"], L["cap"])
    assert comp["fwd"] == L["cap"] and comp["bwd"] == L["cap"]
    # the list was good for that pass only: a plain pass is bitwise the earlier plain pass
    again = _pass(case, L["dF"])
    assert again["fwd"] == 0 and again["bwd"] == 0
    # 2 cap >= n: not worth it, in either pass
    long_ = _pass(case, L["dF"], L["rows"], (n // 2 + 127) // 128 * 128)
    assert long_["fwd"] == 0 and long_["bwd"] == 0
    for got in (again, long_):
        assert torch.equal(got["F"], L["dense"]["F"])
        for name, g in L["dense"]["grads"].items():
            assert torch.equal(g, got["grads"][name]), name


# ---------------------------------------------------------------------------------------------------------------
# 2. + 3. output and gradients against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [37, 129])
def test_forward_on_the_list_output_and_gradients_against_the_oracle(k):
    case = _case()
    L = _lists(case, k, 10 + k)
    comp = _pass(case, L["dF"], L["rows"], L["cap"])
    assert comp["fwd"] == L["cap"] and comp["bwd"] == L["cap"]
    _check_features(f"{k} rows", comp, L["dense"], case["Fo"], L["rows"])
    _check_grads(f"{k} rows", comp["grads"], L["dense"]["grads"], L["ref"])
    # the parked tensors: y's live rows are the output's rows; conv1_tr shares the dense pass's max-abs slot, final does not
    r, s, d = L["rows"].numpy(), comp["saved"], L["dense"]["saved"]
    assert torch.equal(s["y"][:k], comp["F"][r]), "the arena layout the test assumes has changed"
    assert torch.equal(s["y"][:k], (s["final"] / s["norm"][:, None])[:k]), "the arena layout the test assumes has changed"
    for name, t in s.items():
        assert torch.isfinite(t).all(), name
    assert torch.equal(d["final"] / d["norm"][:, None], L["dense"]["F"]), "the arena layout the test assumes has changed"
    print(f"[{k} rows] conv1_tr rows bitwise equal to the dense pass: {torch.equal(s['conv1_tr'][:k], d['conv1_tr'][r])}; "
          f"final rows: {torch.equal(s['final'][:k], d['final'][r])}")


@gpu
def test_a_list_of_no_rows_gives_exact_zeros():
    case = _case()
    L = _lists(case, 0, 10)
    comp = _pass(case, L["dF"], L["rows"], L["cap"])
    assert comp["fwd"] == 128 and comp["bwd"] == 128
    assert not comp["F"].any()
    for name, g in comp["grads"].items():
        assert not g.any(), name
    for t in comp["saved"].values():
        assert torch.isfinite(t).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. padding rows: final(0) = bias = 0 is a zero row in front of the row normalisation
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_padding_rows_are_finite_and_inert_with_a_zero_bias():
    from oracle import me_oracle as O
    case = _case()
    n, k, cap = case["n"], 37, 128
    dF, rows = _dF(n, k, 47)
    state = {name: v.clone() for name, v in case["state0"].items()}
    state["final.bias"].zero_()
    if "zero_bias" not in _CACHE:
        so = {name: v.detach().clone().requires_grad_(v.requires_grad) for name, v in case["so"].items()}
        with torch.no_grad():
            so["final.bias"].zero_()
        Fo = O.resunet_forward(so, case["C"].cpu().numpy(), case["F"].cpu().double(), 3, True, True, 0.05)
        _CACHE["zero_bias"] = (so, Fo)
    so, Fo = _CACHE["zero_bias"]
    ref = _oracle_grads(so, Fo, dF)
    dense = _pass(case, dF, state=state)
    comp = _pass(case, dF, rows, cap, state=state)
    assert comp["fwd"] == cap and comp["bwd"] == cap
    s = comp["saved"]
    for name, t in s.items():
        assert torch.isfinite(t).all(), name
    assert torch.equal(s["y"][:k], comp["F"][rows.numpy()]), "the arena layout the test assumes has changed"
    assert not s["x"][k:].any() and not s["conv1_tr"][k:].any() and not s["final"][k:].any() and not s["y"][k:].any()
    assert bool((s["norm"][k:] == 1).all()) and bool((s["norm"][:k] > 0).all())
    assert torch.isfinite(comp["F"]).all()
    _check_features("zero bias", comp, dense, Fo, rows)
    _check_grads("zero bias", comp["grads"], dense["grads"], ref)


# ---------------------------------------------------------------------------------------------------------------
# 5. list before the forward pass / only before the backward pass
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_both_orders_agree_within_the_oracle_bound():
    case = _case()
    L = _lists(case, 129, 139)
    fwd = _pass(case, L["dF"], L["rows"], L["cap"])
    bwd = _pass(case, L["dF"], L["rows"], L["cap"], before=False)
    assert fwd["fwd"] == L["cap"] and fwd["bwd"] == L["cap"]
    assert bwd["fwd"] == 0 and bwd["bwd"] == L["cap"]
    assert torch.equal(bwd["F"], L["dense"]["F"])          # today's order: dense forward
    _check_grads("list before the forward", fwd["grads"], L["dense"]["grads"], L["ref"])
    _check_grads("list before the backward", bwd["grads"], L["dense"]["grads"], L["ref"])
    # the cat's gradient is what everything upstream is made of: the two orders agree as closely as either does with the oracle
    for name in fwd["grads"]:
        e_a, e_b = _rel_l2(fwd["grads"][name], L["ref"][name]), _rel_l2(bwd["grads"][name], L["ref"][name])
        assert _rel_l2(fwd["grads"][name], bwd["grads"][name]) <= e_a + e_b + 1e-30, name


# ---------------------------------------------------------------------------------------------------------------
# 6. a backward range that cuts the head of a pass that ran on the list
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_a_record_range_that_cuts_the_head_is_refused_and_bucket_segments_keep_the_forward_dense():
    case = _case()
    lib = _lib.load()
    n = case["n"]
    L = _lists(case, 37, 47)
    plan = L["dense"]["plan"]
    n_ops = len(plan.records)
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        case["m"].load_state_dict(case["state0"])
        plan.touch_loss_rows(e, torch.zeros(1, dtype=torch.int64, device=DEV), e, L["rows"].to(DEV), e, n, L["cap"])
        y = plan.run(case["F"], case["mgr"].native)
        assert lib.gcl_plan_suffix_fwd_rows_used(plan.handle) == L["cap"]
        run = y.grad_fn.run
        flat = torch.zeros(sum(p.numel() for p in plan.params), device=DEV)
        targets, off = [], 0
        for p in plan.params:
            targets.append(flat[off:off + p.numel()])
            off += p.numel()
        gp = (ctypes.c_void_p * len(targets))(*[t.data_ptr() for t in targets])
        dy = L["dF"].to(DEV)
        rc = lib.gcl_plan_backward(plan.handle, _lib.ptr(run.arena), _lib.ptr(dy), gp, n_ops - 2, n_ops, _lib.stream())
        msg = lib.gcl_last_error().decode()
        assert rc != 0 and "cuts the touched-row suffix" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert not flat.any()          # nothing was launched
        del y, run                     # the refused pass is un-parked with its output
    # the next plain pass works, bit for bit
    again = _pass(case, L["dF"])
    assert again["fwd"] == 0 and again["bwd"] == 0
    for name, g in L["dense"]["grads"].items():
        assert torch.equal(g, again["grads"][name]), name
    # gradient buckets that end inside the head: the host side keeps the list away from the forward pass, and the backward
    # pass (whose first segment cuts the head) runs the dense records
    names = [k for k, _ in case["m"].named_parameters()]
    buckets = {i: (0 if k.startswith("final.") else 1) for i, k in enumerate(names)}
    seg = _pass(case, L["dF"], L["rows"], L["cap"], buckets=buckets)
    assert seg["fwd"] == 0 and seg["bwd"] == 0
    assert torch.equal(seg["F"], L["dense"]["F"])
    for name, g in L["dense"]["grads"].items():
        assert torch.equal(g, seg["grads"][name]), name


# ---------------------------------------------------------------------------------------------------------------
# 7. the trainer's step
# ---------------------------------------------------------------------------------------------------------------
def _trainer_step(batch, draws, dense):
    """(loss, parts, parameter update, rows the head ran on) of ONE optimizer step from the seeded initial state.  The plan
    exists after a first step (recorded by the Tape); the state is put back behind it."""
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    lib = _lib.load()
    keys = ("sinput_C", "sinput_F", "group", "index", "finest_flag")
    torch.manual_seed(0)
    np.random.seed(0)
    tr = FinestContrastiveLossTrainer(make_config(batch_size=1, num_pos_per_batch=16, num_hn_samples_per_batch=32), device=DEV)
    init = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}

    def feed():
        b = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k in keys else v) for k, v in batch.items()}
        b = tr._prefetch_maps(b)
        b["_group_host"] = batch["group"]
        return b

    with torch.cuda.device(DEV):
        tr.train_step(feed(), draws)
        tr.model.load_state_dict(init)
        tr.optimizer.state.clear()
        if dense:
            tr._touched_cap = lambda *a: None
        loss, parts, _ = tr.train_step(feed(), draws)
        torch.cuda.synchronize()
    plan = tr.model._plan
    used = (int(lib.gcl_plan_suffix_fwd_rows_used(plan.handle)), int(lib.gcl_plan_suffix_rows_used(plan.handle)))
    step = {k: (p.detach() - init[k]).cpu().double() for k, p in tr.model.named_parameters()}
    vals = np.array([loss.item()] + [p.item() for p in parts], dtype=np.float64)
    return vals, step, used, tr, {k: v.cpu().double() for k, v in init.items() if "num_batches" not in k}


@gpu
def test_trainer_step_with_the_list_passed_forward_against_the_dense_step():
    from gcl_amd import synthetic
    from oracle import me_oracle, loss_oracle
    torch.manual_seed(0)
    np.random.seed(0)
    batch = synthetic.collate_train([synthetic.make_train_sample(3, num_neighborhood=2, n_boxes=12)])
    N, G = len(batch["sinput_C"]), len(batch["group"])
    rng = np.random.RandomState(5)
    draws = (rng.choice(G, min(G, 16), replace=False), rng.choice(N, 32, replace=False), rng.choice(N, 32, replace=False))
    v_comp, s_comp, used, tr, init = _trainer_step(batch, draws, dense=False)
    v_dense, s_dense, used_d, _, _ = _trainer_step(batch, draws, dense=True)
    assert used[0] > 0 and used[0] == used[1], f"the step did not pass the list forward: {used} (N = {N})"
    assert used_d == (0, 0)
    rel = np.abs(v_comp - v_dense) / np.maximum(np.abs(v_dense), 1e-30)
    print(f"(total, pos, finest, neg) on the list {v_comp}, dense {v_dense}, relative difference {rel}")
    assert np.all(rel <= 1e-6), (v_comp, v_dense, rel)
    # the fp64 oracle's step: same parameters, batch and draws; SGD's first step from an empty momentum buffer
    cfg = tr.config
    so = {k: v.clone().requires_grad_("running" not in k) for k, v in init.items()}
    Fo = me_oracle.resunet_forward(so, batch["sinput_C"].numpy(), batch["sinput_F"].double(), 5, True, True, 0.05)
    p, f, ng = loss_oracle.finest_contrastive_loss(Fo, batch["group"].numpy(), batch["index"].numpy(), batch["index_hash"],
                                                   batch["finest_flag"].numpy(), draws=draws)
    (tr.pos_weight * p + tr.finest_weight * f + tr.neg_weight * ng).backward()
    worst = (0.0, None)
    for name, d_comp in s_comp.items():
        ref = -cfg.lr * (so[name].grad + cfg.weight_decay * init[name])
        e_dense, e_comp = _rel_l2(s_dense[name], ref), _rel_l2(d_comp, ref)
        if e_dense > 0 and e_comp / e_dense > worst[0]:
            worst = (e_comp / e_dense, name, e_dense, e_comp)
        assert torch.isfinite(d_comp).all() and e_comp <= 2 * e_dense, (name, e_dense, e_comp)
    print(f"parameter updates: largest e_comp / e_dense {worst}")
