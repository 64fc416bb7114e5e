"""The loss gradient stays compact up to the first BatchNorm backward (include/gcl_amd.h: gcl_bn_bwd_reduce_rows,
gcl_bn_bwd_apply_rows, gcl_scatter_add_rows, gcl_row_slots; csrc/plan.hip: TState::rv).

Kernel level: n = 1003 rows, c = 32, c = 64 and c = 64 as the left slice of a pitch-96 compact tensor; lists of 0, 1 (row 0),
1 (row n - 1), 37 and 129 rows -- the longer ones hold row 0 and row n - 1 -- in cap = 128 / 256 entries whose padding is -1
and whose padding rows of g hold 1e30; with the ReLU's sign bits and without.  The sums are held against fp64 numpy at the
bounds tests/test_gpu_norm_kernels.py uses for gcl_bn_bwd_reduce (u = 2^-24: sum_g 2 u |want| + 2^-40 sum|terms|, sum_gx
3 u sum|g||xhat| + 2 u |want|), and against the dense entry on the zero-filled g: the list kernel runs the dense kernel's grid,
every thread on the rows it takes there, so the partials, the sums and max|g| are asserted bit for bit; dx within 1 ulp of
gcl_bn_bwd_apply's (the count of differing elements is printed), the compact dres bitwise the dense one's rows.  Measured on
an MI355X: worst |err| / bound 0.43 (sum_g) and 0.09 (sum_gx); no element of dx differs in any case; 64 of the 66 plan
gradients are bitwise the dense pass's (all but conv1_tr.kernel and final.kernel, the head's sums over fewer rows), the
largest ratio of the distances from the oracle is 1.002 (final.kernel, 129 rows).

Plan level: the model, cloud and lists of tests/test_gpu_head_forward_touched_rows.py (ResUNetBN2C, 1788 voxels; 37 / 0 / 129
rows in cap 128 / 128 / 256), the list set before the forward pass and before the backward pass: each of the 66 parameter
gradients at most twice as far from the fp64 oracle as the dense pass's.  The plan offers no view of the input gradient of
the two launches that now run plain with a scatter-add behind them; every gradient upstream of them is made of it, and the
tests print how many of the 66 tensors are bitwise the dense pass's (all of them when the list is set before the backward
pass means that dx was)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO                                                                     # noqa: E402
from test_gpu_head_touched_rows import DEV, _case, _rel_l2                                   # noqa: E402
from test_gpu_head_forward_touched_rows import _check_grads, _lists, _pass, _trainer_step    # noqa: E402

gpu = pytest.mark.gpu
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
N = 1003
AMAX_WORDS, AMAX_STRIDE = 512, 32
SHAPES = {"c32": (32, 0), "c64": (64, 0), "c64_of_96": (64, 96)}
LISTS = {"0": (0, None), "1_first": (1, 0), "1_last": (1, N - 1), "37": (37, None), "129": (129, None)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(entry, *args):
    lib = _lib.load()
    with torch.cuda.device(DEV):
        a = [_lib.ptr(x) if (x is None or torch.is_tensor(x)) else x for x in args]
        _lib.check(getattr(lib, entry)(*a, _lib.stream()), entry)
        torch.cuda.synchronize()


def _rows(k, only):
    """k distinct rows ascending (row 0 and row N - 1 among them from two rows on), in cap entries padded with -1."""
    r = np.random.default_rng(1000 + k)
    if k == 0:
        rows = np.zeros(0, np.int64)
    elif k == 1:
        rows = np.array([only], np.int64)
    else:
        rows = np.sort(np.concatenate([[0, N - 1], 1 + r.permutation(N - 2)[:k - 2]])).astype(np.int64)
    cap = max(128, (k + 127) // 128 * 128)
    lst = np.full(cap, -1, np.int32)
    lst[:k] = rows
    return rows, lst, cap


def _problem(c, k):
    r = np.random.default_rng(7 * c + k)
    sd = np.exp2(r.uniform(-2, 2, c))
    mu = r.uniform(-3, 3, c) * sd
    x = (r.standard_normal((N, c)) * sd + mu).astype(F32)
    mean = (mu + 0.1 * sd * r.uniform(-1, 1, c)).astype(F32)
    rstd = (r.uniform(0.9, 1.1, c) / sd).astype(F32)
    w = (r.uniform(0.5, 1.5, c) * np.where(np.arange(c) % 3 == 1, -1.0, 1.0)).astype(F32)
    bits = r.random((N, c)) < 0.6
    gk = (r.standard_normal((k, c)) * np.exp2(r.uniform(-10, -6, c))).astype(F32)
    return x, mean, rstd, w, bits, gk


def _slot(value=None):
    s = np.zeros(AMAX_WORDS, np.int32)
    if value is not None:
        s[5 * AMAX_STRIDE] = np.float32(value).view(np.int32)
    return _dev(s)


def _ulps(a, b):
    """Distance of two fp32 arrays in units in the last place (the integer order of their bit patterns)."""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------------------------
# 1. the two BatchNorm backward entries against fp64 numpy and against their dense twins
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "plain"])
@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bn_backward_on_a_row_list(shape, lst, relu):
    lib = _lib.load()
    (c, ld), (k, only) = SHAPES[shape], LISTS[lst]
    rows, rows_pad, cap = _rows(k, only)
    x, mean, rstd, w, bits, gk = _problem(c, k)
    compact = np.full((cap, ld or c), 1e30, F32)          # padding rows and the columns past c must not be read into a sum
    compact[:k, :c] = gk
    dense_g = np.zeros((N, c), F32)
    dense_g[rows] = gk
    gate = bits if relu else None
    xrange = np.stack([x.min(0), x.max(0)])
    d = {name: _dev(v) for name, v in dict(x=x, mean=mean, rstd=rstd, w=w, xrange=xrange, g=compact, dense_g=dense_g,
                                           rows=rows_pad).items()}
    mask = _dev(NO.pack_mask(bits, N, c).view(np.int64)) if relu else None
    n_scratch = lib.gcl_bn_scratch_len(N, c)
    nwg = n_scratch // (3 * c)

    def sums(entry):
        sg, sx = torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)
        scratch = torch.full((n_scratch,), float("nan"), dtype=torch.float64, device=DEV)
        slot = _slot()
        if entry == "rows":
            _call("gcl_bn_bwd_reduce_rows", d["x"], d["g"], ld, slots, mask, N, c, d["mean"], d["rstd"], relu, scratch, sg, sx,
                  d["xrange"], d["w"], slot)
        else:
            _call("gcl_bn_bwd_reduce_range", d["x"], d["dense_g"], 0, None, mask, N, c, d["mean"], d["rstd"], relu, scratch,
                  sg, sx, d["xrange"], d["w"], slot)
        return sg.cpu().numpy(), sx.cpu().numpy(), scratch.cpu().numpy(), slot.cpu().numpy()

    slots = torch.full((N,), 12345, dtype=torch.int32, device=DEV)
    _call("gcl_row_slots", d["rows"], cap, N, slots)
    want_slots = np.full(N, -1, np.int32)
    want_slots[rows] = np.arange(k)
    assert np.array_equal(slots.cpu().numpy(), want_slots)
    sg, sx, part, slot = sums("rows")
    sg_d, sx_d, part_d, slot_d = sums("dense")
    want_g, want_gx, abs_gx = NO.bn_bwd_sums(x, dense_g, gate, mean, rstd)
    sum_abs = np.abs(NO._gated(dense_g, gate)).sum(0)
    err_g, err_gx = np.abs(sg - want_g), np.abs(sx - want_gx)
    bound_g, bound_gx = 2 * U * np.abs(want_g) + 2.0 ** -40 * sum_abs, 3 * U * abs_gx + 2 * U * np.abs(want_gx)
    gmax = part.reshape(3, c, nwg)[2].max(1)
    print(f"[{shape} {lst} relu={relu}] sum_g worst |err| / bound {np.max(err_g / np.maximum(bound_g, 1e-300)):.3f}, sum_gx "
          f"{np.max(err_gx / np.maximum(bound_gx, 1e-300)):.3f}; sums bitwise the dense entry's: "
          f"{sg.tobytes() == sg_d.tobytes() and sx.tobytes() == sx_d.tobytes()}; partials bitwise: {part.tobytes() == part_d.tobytes()}")
    assert np.isfinite(sg).all() and np.isfinite(sx).all() and np.isfinite(part).all()
    assert (err_g <= bound_g).all() and (err_gx <= bound_gx).all()
    assert np.array_equal(gmax, part_d.reshape(3, c, nwg)[2].max(1)), "max|g| differs from the dense entry's"
    assert np.array_equal(gmax, np.abs(NO._gated(dense_g, gate)).max(0)), "max|g| differs from numpy's"
    assert part.tobytes() == part_d.tobytes() and sg.tobytes() == sg_d.tobytes() and sx.tobytes() == sx_d.tobytes()
    assert slot.tobytes() == slot_d.tobytes(), "the bound of max|dx| differs from the dense entry's"
    if k == 0:
        assert not sg.any() and not sx.any() and not gmax.any()

    # the apply pass on the sums the list kernel left
    sgd, sxd = _dev(sg), _dev(sx)
    for image in (0, 1):
        dx, dx_d = torch.full((N, c), float("nan"), device=DEV), torch.full((N, c), float("nan"), device=DEV)
        dres = torch.full((cap, c), -7777.25, device=DEV)
        dres_d = torch.full((N, c), float("nan"), device=DEV)
        want_dx, _, _ = NO.bn_bwd_apply(x, dense_g, gate, mean, rstd, w, sg, sx, N)
        am, am_d = (_slot(F32(np.abs(want_dx).max() * 1.25 + 1e-30)) for _ in range(2)) if image else (_slot(), _slot())
        img, img_d = ((torch.zeros((N, 2 * c), dtype=torch.int16, device=DEV) for _ in range(2)) if image else (None, None))
        _call("gcl_bn_bwd_apply_rows", d["x"], d["g"], ld, slots, mask, N, c, d["mean"], d["rstd"], d["w"], sgd, sxd, relu, dx,
              dres, am, img)
        _call("gcl_bn_bwd_apply_planes", d["x"], d["dense_g"], 0, None, mask, N, c, d["mean"], d["rstd"], d["w"], sgd, sxd, relu,
              dx_d, dres_d, am_d, img_d)
        a, b = dx.cpu().numpy(), dx_d.cpu().numpy()
        assert np.isfinite(a).all()
        dist = _ulps(a, b)
        print(f"[{shape} {lst} relu={relu} image={image}] dx elements that differ from gcl_bn_bwd_apply's: {int((dist > 0).sum())} "
              f"of {a.size}, at most {int(dist.max())} ulp")
        assert dist.max() <= 1
        assert np.array_equal(dres.cpu().numpy()[:k], dres_d.cpu().numpy()[rows]), "compact dres is not the dense one's rows"
        assert (dres.cpu().numpy()[k:] == -7777.25).all(), "a padding row of the compact dres was written"
        assert torch.equal(am.cpu(), am_d.cpu())
        if image:
            assert torch.equal(img.cpu(), img_d.cpu()), "the plane image of dx differs from the dense entry's"


@gpu
@pytest.mark.parametrize("src_ld,dst_ld", [(32, 32), (96, 32), (64, 96)])
def test_scatter_add_rows_is_one_fp32_addition_per_listed_element(src_ld, dst_ld):
    c, k = 32, 129
    rows, rows_pad, cap = _rows(k, None)
    r = np.random.default_rng(src_ld + dst_ld)
    src = r.standard_normal((cap, src_ld)).astype(F32)          # the padding rows hold values that must go nowhere
    dst = r.standard_normal((N, dst_ld)).astype(F32)
    want = dst.copy()
    want[rows, :c] = dst[rows, :c] + src[:k, :c]
    out = _dev(dst)
    _call("gcl_scatter_add_rows", _dev(src), src_ld, _dev(rows_pad), cap, c, N, out, dst_ld)
    assert out.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 2. the plan: 66 gradients against the fp64 oracle, the list set in front of either pass
# ---------------------------------------------------------------------------------------------------------------
def _bitwise(tag, comp, dense):
    same = [name for name, g in comp.items() if torch.equal(g, dense[name])]
    print(f"[{tag}] gradients bitwise the dense pass's: {len(same)} of {len(comp)}"
          + ("" if len(same) == len(comp) else f"; not: {sorted(set(comp) - set(same))}"))
    return len(same)


@gpu
@pytest.mark.parametrize("before", [True, False], ids=["list_before_forward", "list_before_backward"])
@pytest.mark.parametrize("k", [37, 0, 129])
def test_plan_gradients_with_the_gradient_compact_up_to_the_first_batchnorm(k, before):
    case = _case()
    L = _lists(case, k, 10 + k)
    assert L["cap"] == {37: 128, 0: 128, 129: 256}[k] and 1500 < case["n"] < 2100
    comp = _pass(case, L["dF"], L["rows"], L["cap"], before=before)
    assert comp["bwd"] == L["cap"] and comp["fwd"] == (L["cap"] if before else 0), "the pass did not run on the list"
    assert len(comp["grads"]) == 66
    tag = f"{k} rows, list before the {'forward' if before else 'backward'} pass"
    _bitwise(tag, comp["grads"], L["dense"]["grads"])
    if k == 0:
        for name, g in comp["grads"].items():
            assert not g.any(), name
        return
    _check_grads(tag, comp["grads"], L["dense"]["grads"], L["ref"])
    # the pass sized itself with a counted run of the head on this plan: a second pass is the first
    again = _pass(case, L["dF"], L["rows"], L["cap"], before=before)
    assert again["bwd"] == L["cap"]
    for name, g in comp["grads"].items():
        assert torch.equal(g, again["grads"][name]), name


@gpu
def test_a_long_list_runs_the_dense_records_bit_for_bit():
    case = _case()
    n = case["n"]
    L = _lists(case, 37, 47)
    for before in (True, False):
        got = _pass(case, L["dF"], L["rows"], (n // 2 + 127) // 128 * 128, before=before)      # 2 cap >= n
        assert got["fwd"] == 0 and got["bwd"] == 0
        for name, g in L["dense"]["grads"].items():
            assert torch.equal(g, got["grads"][name]), name
    plain = _pass(case, L["dF"])
    for name, g in L["dense"]["grads"].items():
        assert torch.equal(g, plain["grads"][name]), name


# ---------------------------------------------------------------------------------------------------------------
# 3. the trainer's step on the smoke batch
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_trainer_step_loss_equal_and_updates_within_twice_the_dense_error():
    from gcl_amd import synthetic
    from oracle import me_oracle, loss_oracle
    torch.manual_seed(0)
    np.random.seed(0)
    batch = synthetic.collate_train([synthetic.make_train_sample(3, num_neighborhood=2, n_boxes=12)])
    n, groups = len(batch["sinput_C"]), len(batch["group"])
    rng = np.random.RandomState(5)
    draws = (rng.choice(groups, min(groups, 16), replace=False), rng.choice(n, 32, replace=False), rng.choice(n, 32, replace=False))
    v_comp, s_comp, used, tr, init = _trainer_step(batch, draws, dense=False)
    v_dense, s_dense, used_d, _, _ = _trainer_step(batch, draws, dense=True)
    assert used[0] > 0 and used[0] == used[1] and used_d == (0, 0), (used, used_d)
    print(f"(total, pos, finest, neg) on the list {v_comp}, dense {v_dense}")
    assert np.array_equal(v_comp, v_dense), (v_comp, v_dense)
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
