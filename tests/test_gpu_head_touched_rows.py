"""Backward pass of the network's row-local head on the rows the loss touched (include/gcl_amd.h, "Touched rows";
csrc/plan.hip: gcl_touched_rows, gcl_gather_rows, gcl_scatter_rows, gcl_plan_set_touched_rows).

The list builder against numpy.unique, the two row moves exactly, and a ResUNetBN2C pass whose output gradient is
non-zero on a few rows, with and without the list: everything upstream of the head bitwise equal, the three head tensors
(conv1_tr.kernel, final.kernel, final.bias: sums over fewer rows in other groups) no further from the fp64 oracle than
twice the dense pass's distance.  The suffix rule itself needs no GPU (last test)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEV = "cuda:0"
gpu = pytest.mark.gpu
HEAD = ("conv1_tr.kernel", "final.kernel", "final.bias")


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.linalg.norm(a - b))


# ---------------------------------------------------------------------------------------------------------------
# list builder
# ---------------------------------------------------------------------------------------------------------------
def _touched(index, goff, sel, rows_a, rows_b, n, cap):
    lib = _lib.require_gpu()
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(DEV)
    index, goff, sel, rows_a, rows_b = t(index), t(goff), t(sel), t(rows_a), t(rows_b)
    scratch = torch.empty(lib.gcl_touched_rows_scratch_len(n), dtype=torch.int32, device=DEV)
    rows = torch.full((cap + 8,), 77, dtype=torch.int32, device=DEV)       # 8 guard words behind the list
    count = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.gcl_touched_rows(_lib.ptr(index), len(index), _lib.ptr(goff), len(goff) - 1, _lib.ptr(sel), len(sel),
                                        _lib.ptr(rows_a), len(rows_a), _lib.ptr(rows_b), len(rows_b), n, _lib.ptr(scratch),
                                        _lib.ptr(rows), cap, _lib.ptr(count), _lib.stream()), "gcl_touched_rows")
        torch.cuda.synchronize()
    assert rows[cap:].tolist() == [77] * 8, "wrote behind the list"
    return rows[:cap].cpu().numpy(), int(count.item())


@gpu
@pytest.mark.parametrize("case", ["duplicates", "empty", "every_row"])
def test_touched_row_list_equals_numpy_unique(case):
    n = 1000
    rng = np.random.RandomState(4)
    # 40 groups over a shuffled index array (rows shared between groups: duplicates inside the index array too)
    sizes = rng.randint(1, 9, 40)
    goff = np.concatenate([[0], np.cumsum(sizes)])
    index = rng.randint(0, n, goff[-1])
    if case == "duplicates":
        sel = rng.choice(40, 12, replace=False)
        a, b = rng.randint(0, n, 50), rng.randint(0, n, 50)
        a[:10] = index[goff[sel[0]]]                 # the same row from three sources
        b[:5] = a[:5]
        cap = 256
    elif case == "empty":
        sel, a, b, cap = np.zeros(0, int), np.zeros(0, int), np.zeros(0, int), 128
    else:
        sel, a, b, cap = np.arange(40), rng.permutation(n), np.arange(n)[::-1].copy(), 1024
    members = np.concatenate([index[goff[g]:goff[g + 1]] for g in sel] + [np.zeros(0, int)])
    want = np.unique(np.concatenate([members, a, b])).astype(np.int32)
    rows, count = _touched(index, goff, sel, a, b, n, cap)
    assert count == len(want)
    assert np.array_equal(rows[:count], want) and np.all(rows[count:] == -1)


@gpu
def test_touched_row_list_skips_ids_outside_their_array_and_cuts_at_cap():
    n = 1000
    index, goff = np.array([5, 2000, -3, 999, 7]), np.array([0, 2, 5])
    rows, count = _touched(index, goff, [1, 0, 9, -1], [1 << 40, 3], [-1, 3, 0], n, 128)
    want = [0, 3, 5, 7, 999]
    assert count == 5 and rows[:5].tolist() == want and np.all(rows[5:] == -1)
    # more rows than the caller's bound: the first `cap`, the true count (the caller can tell)
    rows, count = _touched(np.zeros(0, int), np.array([0]), [], np.arange(0, 600, 2), [], n, 128)
    assert count == 300 and rows.tolist() == list(range(0, 256, 2))


# ---------------------------------------------------------------------------------------------------------------
# gather / scatter
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,ld,off", [(32, 32, 0), (96, 96, 0), (32, 96, 64), (96, 128, 32)])
def test_gather_and_scatter_rows_are_exact(c, ld, off):
    """cap = 300 (no multiple of the 256-thread block, more than one block), -1 entries, one index past the end and one far
    negative: gathered as `pad`, skipped by the scatter -- checked on a destination with 16 guard rows behind it."""
    lib = _lib.require_gpu()
    n, cap = 1000, 300
    rng = np.random.RandomState(c + ld)
    rows = np.full(cap, -1, np.int32)
    rows[:257] = np.sort(rng.choice(n, 257, replace=False))
    rows[100], rows[200] = n + 3, -7
    g = torch.Generator().manual_seed(ld)
    wide = torch.randn(n, ld, generator=g)
    src = wide.to(DEV)
    rows_d = torch.from_numpy(rows).to(DEV)
    live = (rows >= 0) & (rows < n)
    with torch.cuda.device(DEV):
        for pad in (0.0, 1.0):
            out = torch.full((cap + 1, c), 9.0, device=DEV)
            _lib.check(lib.gcl_gather_rows(ctypes.c_void_p(src.data_ptr() + 4 * off), ld, n, _lib.ptr(rows_d), cap, c, pad,
                                           _lib.ptr(out), _lib.stream()), "gcl_gather_rows")
            want = torch.full((cap, c), pad)
            want[live] = wide[rows[live]][:, off:off + c]
            assert torch.equal(out[:cap].cpu(), want) and bool((out[cap] == 9.0).all())
        # a column of scalars (the row norms): c = 1
        col = torch.full((cap,), 9.0, device=DEV)
        _lib.check(lib.gcl_gather_rows(_lib.ptr(src), ld, n, _lib.ptr(rows_d), cap, 1, 1.0,
                                       _lib.ptr(col), _lib.stream()), "gcl_gather_rows")
        want = torch.ones(cap)
        want[live] = wide[rows[live], 0]
        assert torch.equal(col.cpu(), want)
        # scatter into columns [off, off + c) of a zero-filled [n (+ 16 guard rows), ld] tensor
        comp = torch.randn(cap, c, generator=g)
        dst = torch.zeros(n + 16, ld, device=DEV)
        _lib.check(lib.gcl_scatter_rows(_lib.ptr(comp.to(DEV)), _lib.ptr(rows_d), cap, c, n,
                                        ctypes.c_void_p(dst.data_ptr() + 4 * off), ld, _lib.stream()), "gcl_scatter_rows")
        want = torch.zeros(n + 16, ld)
        want[rows[live].astype(np.int64), off:off + c] = comp[live]
        assert torch.equal(dst.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------
# plan level: ResUNetBN2C on one cloud, dF non-zero on 37 / 0 / 129 rows
# ---------------------------------------------------------------------------------------------------------------
_CASE, _CASE_PLANES = {}, {}


def _case(cache=_CASE, oracle=None):
    """Model, maps, recorded plan and the fp64 oracle's graph: made once, shared by the plan-level tests, never changed.
    ``oracle``: an earlier case whose model has the same parameters, and whose oracle graph this one shares."""
    if cache:
        return cache
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd import synthetic
    from gcl_amd.MinkowskiEngine import native
    from gcl_amd.model import load_model
    from oracle import me_oracle as O
    xyz = synthetic.make_box_cloud(0, 5000)            # the parity tests' box cloud, voxel 0.3: 1788 voxels
    C = ME.utils.batched_coordinates([ME.utils.sparse_quantize(xyz / 0.3)])
    feats = torch.ones(len(C), 1)
    torch.manual_seed(0)
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3, D=3).to(DEV)
    with torch.no_grad():                              # non-trivial BatchNorm affine parameters
        for name, p in m.named_parameters():
            if name.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            elif name.endswith("bn.bias"):
                p.uniform_(-0.1, 0.1)
    st = {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items() if "num_batches" not in k}
    m.train()
    if oracle is not None:
        assert st.keys() == oracle["st"].keys() and all(torch.equal(v, oracle["st"][k]) for k, v in st.items())
        so, Fo = oracle["so"], oracle["Fo"]
    else:
        so = {k: v.clone().requires_grad_("running" not in k) for k, v in st.items()}
        Fo = O.resunet_forward(so, C.numpy(), feats.double(), 3, True, True, 0.05)
    with torch.cuda.device(DEV):
        Cd, Fd = C.to(DEV), feats.to(DEV)
        mgr = ME.CoordinateManager.build_native(Cd, m.native_map_specs())
        state0 = {k: v.clone() for k, v in m.state_dict().items()}
        m(ME.SparseTensor(Fd, coordinates=Cd, coordinate_manager=mgr)).F.sum().backward()      # recorded by the Tape
        assert isinstance(m._plan, native.NetworkPlan), getattr(m, "_plan_error", None)
        m.load_state_dict(state0)
    cache.update(m=m, state0=state0, st=st, so=so, Fo=Fo, C=Cd, F=Fd, mgr=mgr, n=len(C))
    return cache


def _dF(n, k, seed):
    """Gradient of the output that is non-zero on k rows spread over the cloud."""
    g = torch.Generator().manual_seed(seed)
    dF = torch.zeros(n, 32)
    rows = torch.randperm(n, generator=g)[:k].sort().values
    dF[rows] = torch.randn(k, 32, generator=g)
    return dF, rows


def _backward(case, dF, rows=None, cap=None, before_forward=False):
    """One training pass through the plan; ``rows``: announce them first -- behind the forward pass, or in front of it.
    Returns ({name: gradient}, rows the head ran on in the backward pass, the plan)."""
    import gcl_amd.MinkowskiEngine as ME
    lib = _lib.load()
    m = case["m"]
    with torch.cuda.device(DEV):
        m.load_state_dict(case["state0"])
        for p in m.parameters():
            p.grad = None
        x = ME.SparseTensor(case["F"], coordinates=case["C"], coordinate_manager=case["mgr"])
        plan = m.plan_for(x)
        assert plan is not None
        e = torch.zeros(0, dtype=torch.int64, device=DEV)
        goff = torch.zeros(1, dtype=torch.int64, device=DEV)
        if rows is not None and before_forward:
            plan.touch_loss_rows(e, goff, e, rows.to(DEV), e, case["n"], cap)
        out = m(x).F
        if rows is not None and not before_forward:
            plan.touch_loss_rows(e, goff, e, rows.to(DEV), e, case["n"], cap)
        out.backward(dF.to(DEV))
        torch.cuda.synchronize()
        used = int(lib.gcl_plan_suffix_rows_used(plan.handle))
        return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}, used, plan


@gpu
@pytest.mark.parametrize("k", [37, 0, 129])
def test_head_backward_on_touched_rows(k):
    case = _case()
    n = case["n"]
    assert 1500 < n < 2100
    dF, rows = _dF(n, k, 10 + k)
    cap = max(128, (k + 127) // 128 * 128)          # 37 -> 128, 0 -> 128 (a list of -1 only), 129 -> 256: crosses a 128 boundary
    dense, used, _ = _backward(case, dF)
    assert used == 0
    comp, used, plan = _backward(case, dF, rows, cap)
    assert used == cap, "the pass did not take the touched-row path"
    assert _lib.load().gcl_plan_touched_suffix(plan.handle) == len(plan.records) - 4      # conv1_tr, relu, final, rownorm
    for name in dense:
        if name not in HEAD:
            assert torch.equal(dense[name], comp[name]), name
    # the three head tensors against the fp64 oracle: at most twice the dense pass's error (the margin for another summation order)
    so, Fo = case["so"], case["Fo"]
    for v in so.values():
        v.grad = None
    Fo.backward(dF.double(), retain_graph=True)
    for name in HEAD:
        ref = so[name].grad
        e_dense, e_comp = _rel_l2(dense[name], ref), _rel_l2(comp[name], ref)
        print(f"[{k} rows] {name}: rel-L2 vs fp64 oracle dense {e_dense:.3e}, touched rows {e_comp:.3e}")
        assert e_comp <= 2 * e_dense, (name, e_dense, e_comp)
        if k == 0:
            assert not comp[name].any() and not dense[name].any()
    # the list was good for that pass only: the next one runs dense again, bit for bit
    again, used, _ = _backward(case, dF)
    assert used == 0
    for name in dense:
        assert torch.equal(dense[name], again[name]), name


@gpu
def test_head_on_touched_rows_reads_plane_images(monkeypatch):
    """The same cloud and model with plane images from 64 channels on (PRESPLIT_MIN_C = 64 while a fresh model records its
    plan): conv1_tr (96 -> 64) reads its input and its output gradient as plane images in the head as well."""
    from gcl_amd.MinkowskiEngine import ops
    lib = _lib.load()
    if not _CASE_PLANES:
        with monkeypatch.context() as mp:
            mp.setattr(ops, "PRESPLIT_MIN_C", 64)
            _case(_CASE_PLANES, oracle=_case())
    case = _CASE_PLANES
    n, k, cap = case["n"], 37, 128
    dF, rows = _dF(n, k, 10 + k)
    dense, used, _ = _backward(case, dF)
    assert used == 0
    comp, used, plan = _backward(case, dF, rows, cap)
    assert used == cap and lib.gcl_plan_suffix_rows_used(plan.handle) == cap, "the pass did not take the touched-row path"
    for name in dense:
        if name not in HEAD:
            assert torch.equal(dense[name], comp[name]), name
    fwd, used, plan = _backward(case, dF, rows, cap, before_forward=True)
    assert lib.gcl_plan_suffix_fwd_rows_used(plan.handle) == cap and used == cap, "the forward pass did not run on the list"
    so, Fo = case["so"], case["Fo"]
    for v in so.values():
        v.grad = None
    Fo.backward(dF.double(), retain_graph=True)
    for name in HEAD:
        ref = so[name].grad
        e_dense, e_comp, e_fwd = _rel_l2(dense[name], ref), _rel_l2(comp[name], ref), _rel_l2(fwd[name], ref)
        print(f"[planes from 64] {name}: rel-L2 vs fp64 oracle dense {e_dense:.3e}, list before the backward pass {e_comp:.3e}, "
              f"before the forward pass {e_fwd:.3e}")
        assert e_comp <= 2 * e_dense, (name, e_dense, e_comp)
        assert e_fwd <= 2 * e_dense, (name, e_dense, e_fwd)


@gpu
def test_long_lists_and_plans_without_a_row_local_head_run_dense():
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import native
    case = _case()
    n = case["n"]
    lib = _lib.load()
    dF, rows = _dF(n, 37, 3)
    dense, _, plan = _backward(case, dF)
    # 2 cap >= n_rows: not worth it
    cap = (n // 2 + 127) // 128 * 128
    got, used, _ = _backward(case, dF, rows, cap)
    assert used == 0
    for name in dense:
        assert torch.equal(dense[name], got[name]), name
    # a plan that ends in a 3^3 convolution (the network's first two records) has no such suffix and ignores a list
    recs = [dict(r) for r in plan.records[:2]]
    assert recs[1]["K"] == 27 and recs[1]["kind"] == _lib.OP_CONVBN
    n_tensors = max(max(r["x"], r["x2"], r["y"]) for r in recs) + 1
    sub = native.NetworkPlan(recs, n_tensors, plan.params, plan.bn_buffers[:2], plan.bn_modules[:2], [recs[1]["w"]],
                             plan.spec_keys, recs[1]["cout"])
    assert lib.gcl_plan_touched_suffix(sub.handle) == 2
    g = torch.Generator().manual_seed(8)
    dY = torch.zeros(n, recs[1]["cout"])
    dY[rows] = torch.randn(len(rows), recs[1]["cout"], generator=g)
    outs = []
    with torch.cuda.device(DEV):
        for announce in (False, True):
            y = sub.run(case["F"], case["mgr"].native)
            if announce:
                e = torch.zeros(0, dtype=torch.int64, device=DEV)
                sub.touch_loss_rows(e, torch.zeros(1, dtype=torch.int64, device=DEV), e, rows.to(DEV), e, n, 128)
            grads = torch.autograd.grad(y, [plan.params[recs[0]["w"]], plan.params[recs[1]["w"]]], dY.to(DEV))
            torch.cuda.synchronize()
            assert lib.gcl_plan_suffix_rows_used(sub.handle) == 0
            outs.append([t.cpu().clone() for t in grads])
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and all(bool(a.any()) for a in outs[0])


# ---------------------------------------------------------------------------------------------------------------
# the suffix rule (host only)
# ---------------------------------------------------------------------------------------------------------------
def test_touched_row_suffix_of_record_lists():
    from test_plan_host import _create, _mini_records, _op
    lib = _lib.load()

    def suffix(records, **kw):
        h = _create(records, **kw)
        assert h, lib.gcl_last_error()
        h = ctypes.c_void_p(h)
        s = lib.gcl_plan_touched_suffix(h)
        lib.gcl_plan_destroy(h)
        return s

    # ResUNetBN2C's shape: ... cat, 1x1 conv, relu, 1x1 conv + bias, row normalise -> the four records behind the cat
    rec = _mini_records()
    assert suffix(rec) == 6
    # without the row normalisation (normalize_feature = False) the suffix is the three records behind the cat
    assert suffix(rec[:9], n_tensors=10) == 6
    # no kernel_size-1 head: the last record is a 3^3 convolution + BatchNorm -> no suffix; nor behind a transposed one
    assert suffix(rec[:3], n_tensors=4, n_params=9, worder=(3, 6)) == 3
    assert suffix(rec[:5], n_tensors=6, n_params=15, worder=(3, 6, 9, 12)) == 5
    # `final` as convolution + BatchNorm (statistics over all rows: not row-local): the row normalisation alone
    rec = _mini_records()
    rec[8].update(kind=_lib.OP_CONVBN, bias=-1, bn_w=17, bn_b=18, bn=5)
    assert suffix(rec, n_params=19) == 9
    # the first head convolution's input read a second time (a cat in front of the row normalisation): the chain ends at
    # that cat, and the 1x1 convolutions in front of it stay dense
    rec = _mini_records()
    rec.insert(9, _op(kind=_lib.OP_CAT, x=9, x2=6, y=11, cin=32, cout=96))
    rec[10].update(x=11, y=10, cin=96, cout=96)
    assert suffix(rec, n_tensors=12) == 10
    # the ReLU's output read by a second record: the run of row-local records starts at `final`, whose input has two readers,
    # so the suffix is cut to the row normalisation
    rec = _mini_records()
    rec.insert(8, _op(kind=_lib.OP_CAT, x=8, x2=5, y=11, cin=64, cout=96))
    assert suffix(rec, n_tensors=12) == 10
