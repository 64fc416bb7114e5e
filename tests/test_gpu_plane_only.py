"""Tensors the training plan keeps as a plane image only (include/gcl_amd.h, "Plane-only tensors"; csrc/plan.hip:
analyse_graph; csrc/norm.hip: k_bn_apply / k_bn_bwd_apply with a NULL fp32 output).

Host level (no GPU): ResUNetBN2C's record list written out by hand -- the reader analysis names the 4 forward and 8 backward
tensors, and the dry sizing shrinks by exactly their blocks, at presplit 128 and 64.

Kernel level: n = 1003 rows (no multiple of the 256-thread block's 64 rows of 128 channels, several blocks), c = 128 and 256,
with / without a residual (forward: the operand, backward: dres) and with / without ReLU.  The call with a NULL fp32 output
against the call with one: image, sign bits, dres and the max-abs slot torch.equal, the canary where the plan's arena would
hold the fp32 block (in front of the image) untouched, and NULL without an image is GCL_ERR_ARG.

Plan level: ResUNetBN2C on the 1788-voxel cloud of tests/test_gpu_head_touched_rows.py, presplit 128 and 64, dense and with a
list of 37 / 129 rows handed over before the forward pass; one fixed output gradient through the default plan and through the
same plan with every fp32 twin kept: features, loss, the 66 gradients and the running statistics bitwise equal, a second pass
equal to the first, the set of plane-only tensors, and the arena smaller by exactly their blocks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gcl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_plan_host import _op                                                        # noqa: E402
from test_gpu_head_touched_rows import DEV, _CASE_PLANES, _case, _dF                  # noqa: E402
from test_gpu_head_forward_touched_rows import _pass                                  # noqa: E402

gpu = pytest.mark.gpu
N = 1003
AMAX_WORDS, AMAX_STRIDE = 512, 32
FWD_128 = {"block3.norm1", "block4.norm1", "block4.norm2", "block4_tr.norm1"}
BWD_128 = {"block3.norm1", "block3.norm2", "block4.norm1", "block4.norm2", "norm4", "norm4_tr", "block4_tr.norm1",
           "block4_tr.norm2"}


# ---------------------------------------------------------------------------------------------------------------
# 1. the reader analysis and the dry sizing (host only)
# ---------------------------------------------------------------------------------------------------------------
def _resunet_records():
    """ResUNetBN2C (channels 32 / 64 / 128 / 256, decoder 64 / 64 / 64 / 128, 3^3 first layer on one input channel) as
    model/resunet.py's _forward records it.  Returns (records, names of the CONVBN records, n_tensors, n_params, worder)."""
    C = _lib.OP_CONVBN
    ch, tr = [None, 32, 64, 128, 256], [None, 64, 64, 64, 128]
    keys = [(1, 3, 1), (1, 3, 2), (2, 3, 1), (2, 3, 2), (4, 3, 1), (4, 3, 2), (8, 3, 1), (1, 1, 1)]
    rec, names, worder = [], {}, []
    state = dict(t=0, p=0, bn=0)

    def new(kind):
        state[kind] += 1
        return state[kind] - (0 if kind == "t" else 1)

    def convbn(name, x, cin, cout, lin, lout, key, transpose=0, x2=-1, relu=0):
        w, bw, bb = new("p"), new("p"), new("p")
        if cin > 4:
            worder.append(w)
        y = new("t")
        names[len(rec)] = name
        rec.append(_op(kind=C, x=x, x2=x2, y=y, level_in=lin, level_out=lout, cin=cin, cout=cout, map=keys.index(key),
                       transpose=transpose, K=27, w=w, bn_w=bw, bn_b=bb, bn=new("bn"), relu=relu, momentum=0.05))
        return y

    def block(name, x, c, lvl):
        key = (1 << lvl, 3, 1)
        y = convbn(f"{name}.norm1", x, c, c, lvl, lvl, key, relu=1)
        return convbn(f"{name}.norm2", y, c, c, lvl, lvl, key, x2=x, relu=1)

    out, width, skips = 0, 1, {}
    for l in (1, 2, 3, 4):
        lin, lout = max(l - 2, 0), l - 1
        out = convbn(f"norm{l}", out, width, ch[l], lin, lout, (1 << lin, 3, 1 if l == 1 else 2))
        out = skips[l] = block(f"block{l}", out, ch[l], lout)
        width = ch[l]
    for l in (4, 3, 2):
        out = convbn(f"norm{l}_tr", out, width, tr[l], l - 1, l - 2, (1 << (l - 2), 3, 2), transpose=1)
        out = block(f"block{l}_tr", out, tr[l], l - 2)
        y = new("t")
        rec.append(_op(kind=_lib.OP_CAT, x=out, x2=skips[l - 1], y=y, level_in=l - 2, level_out=l - 2, cin=tr[l],
                       cout=tr[l] + ch[l - 1]))
        out, width = y, tr[l] + ch[l - 1]
    w = new("p")
    worder.append(w)
    y = new("t")
    rec.append(_op(kind=_lib.OP_CONV, x=out, y=y, cin=width, cout=tr[1], map=7, K=1, w=w))
    out = new("t")
    rec.append(_op(kind=_lib.OP_RELU, x=y, y=out, cin=tr[1], cout=tr[1]))
    w, b = new("p"), new("p")
    worder.append(w)
    y = new("t")
    rec.append(_op(kind=_lib.OP_CONV, x=out, y=y, cin=tr[1], cout=32, map=7, K=1, w=w, bias=b))
    out = new("t")
    rec.append(_op(kind=_lib.OP_ROWNORM, x=y, y=out, cin=32, cout=32))
    return rec, names, state["t"] + 1, state["p"], worder, keys


def _host_maps(keys, rows=(1788, 640, 210, 70)):
    d = _lib.MapsDesc()
    d.n_levels, d.n_maps = 4, len(keys)
    for l, n in enumerate(rows):
        d.n_rows[l] = n
    for i, (t, ks, st) in enumerate(keys):
        m = d.maps[i]
        li = t.bit_length() - 1
        lo = li + (1 if st == 2 else 0)
        m.t_in, m.kernel_size, m.stride, m.K, m.level_in, m.level_out = t, ks, st, ks ** 3, li, lo
        m.n_in, m.n_out = d.n_rows[li], d.n_rows[lo]
        m.n_pairs = 8 * m.n_out
        for k in range(m.K + 1):
            m.seg_off[k] = k * 1024
    return d


def _flags(lib, h, n_ops):
    flags = (ctypes.c_int32 * n_ops)()
    count = lib.gcl_plan_plane_only(h, flags, n_ops)
    fwd, bwd = [i for i in range(n_ops) if flags[i] & 1], [i for i in range(n_ops) if flags[i] & 2]
    assert count == len(fwd) + len(bwd)
    return fwd, bwd


@pytest.mark.parametrize("presplit", [128, 64])
def test_reader_analysis_and_dry_sizing_of_a_resunet_record_list(presplit):
    lib = _lib.load()
    rec, names, n_tensors, n_params, worder, keys = _resunet_records()
    arr = (_lib.PlanOp * len(rec))()
    for a, r in zip(arr, rec):
        for k, v in r.items():
            setattr(a, k, v)
    wo = (ctypes.c_int32 * len(worder))(*worder)
    h = lib.gcl_plan_create(arr, len(rec), n_tensors, n_params, wo, len(worder), presplit)
    assert h, lib.gcl_last_error()
    h = ctypes.c_void_p(h)
    assert lib.gcl_plan_touched_suffix(h) == len(rec) - 4
    fwd, bwd = _flags(lib, h, len(rec))
    print(f"presplit {presplit}: forward {[names[i] for i in fwd]}, backward {[names[i] for i in bwd]}")
    if presplit == 128:
        assert {names[i] for i in fwd} == FWD_128 and {names[i] for i in bwd} == BWD_128
    else:      # the 64-wide records join; what a residual, an ME.cat or the 1x1 head reads stays fp32
        assert FWD_128 < {names[i] for i in fwd} and BWD_128 < {names[i] for i in bwd}
        assert "block2.norm1" in {names[i] for i in fwd} and "norm2" not in {names[i] for i in bwd}      # norm2: cin 32
        assert not {"block2.norm2", "block2_tr.norm2", "norm2", "norm2_tr"} & {names[i] for i in fwd}
        # the gradient of block2_tr's output (the cat the touched-row suffix reads) and of its residual can arrive compact
        assert not {"block2_tr.norm2", "norm2_tr"} & {names[i] for i in bwd}
        assert "block2_tr.norm1" in {names[i] for i in bwd}
    for i in fwd + bwd:
        assert rec[i]["kind"] == _lib.OP_CONVBN and rec[i]["cout"] >= presplit
    assert lib.gcl_plan_plane_only(h, (ctypes.c_int32 * 3)(), 3) < 0
    d = _host_maps(keys)
    blocks = sum(d.n_rows[rec[i]["level_out"]] * rec[i]["cout"] * 4 for i in fwd + bwd)
    default = lib.gcl_plan_arena_bytes(h, ctypes.byref(d))
    assert lib.gcl_plan_set_keep_fp32(h, 1) == 0
    assert _flags(lib, h, len(rec)) == ([], [])
    kept = lib.gcl_plan_arena_bytes(h, ctypes.byref(d))
    assert lib.gcl_plan_set_keep_fp32(h, 0) == 0
    assert default > 0 and kept - default == blocks, (default, kept, blocks)
    assert lib.gcl_plan_arena_bytes(h, ctypes.byref(d)) == default
    lib.gcl_plan_destroy(h)


# ---------------------------------------------------------------------------------------------------------------
# 2. the two apply kernels with a NULL fp32 output
# ---------------------------------------------------------------------------------------------------------------
CANARY = -7777.25
CANARY_BITS = int(np.float32(CANARY).view(np.int32))


def _slot(value):
    s = np.zeros(AMAX_WORDS, np.int32)
    s[5 * AMAX_STRIDE] = np.float32(value).view(np.int32)
    return torch.from_numpy(s).to(DEV)


def _problem(c, seed):
    g = torch.Generator().manual_seed(seed)
    sd = torch.exp2(torch.rand(c, generator=g) * 4 - 2)
    x = torch.randn(N, c, generator=g) * sd + (torch.rand(c, generator=g) * 6 - 3) * sd
    mean, rstd = x.mean(0), 1.0 / x.std(0)
    w = (torch.rand(c, generator=g) + 0.5) * torch.where(torch.arange(c) % 3 == 1, -1.0, 1.0)
    b = torch.rand(c, generator=g) * 0.2 - 0.1
    other = torch.randn(N, c, generator=g)          # the residual (forward) / the output gradient (backward)
    return [t.contiguous().to(DEV) for t in (x, mean, rstd, w, b, other)]


def _arena(c, mask_words):
    """[guard | fp32 block (canary) | image | sign bits | dres | guard] in one buffer, as the plan lays them out."""
    words = [64, N * c, N * c, 2 * mask_words, N * c, 64]
    buf = torch.full((sum(words),), CANARY, device=DEV)
    off = np.concatenate([[0], np.cumsum(words)])
    return buf, [buf[off[i]:off[i + 1]] for i in range(len(words))]


def _raw(lib, entry, *args):
    with torch.cuda.device(DEV):
        a = [_lib.ptr(x) if (x is None or torch.is_tensor(x)) else x for x in args]
        rc = getattr(lib, entry)(*a, _lib.stream())
        torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "plain"])
@pytest.mark.parametrize("residual", [1, 0], ids=["residual", "no_residual"])
@pytest.mark.parametrize("c", [128, 256])
def test_forward_apply_with_a_null_fp32_output(c, residual, relu):
    lib = _lib.load()
    x, mean, rstd, w, b, res = _problem(c, 11 * c + 2 * residual + relu)
    res = res if residual else None
    mask_words = lib.gcl_bn_mask_len(N, c)
    want = (x - mean) * rstd * w + b + (res if residual else 0)
    bound = float(want.abs().max()) * 1.25
    out = {}
    for null in (False, True):
        buf, (g0, y, img, mask, _, g1) = _arena(c, mask_words)
        slot = _slot(bound)
        rc = _raw(lib, "gcl_bn_apply_planes", x, N, c, mean, rstd, w, b, res, relu, None if null else y, 0,
                  mask if relu else None, slot, img)
        assert rc == 0, lib.gcl_last_error()
        assert bool((g0 == CANARY).all()) and bool((g1 == CANARY).all())
        out[null] = (img.view(torch.int32).clone(), mask.view(torch.int32).clone(), slot.clone(), y.clone())      # bits, not floats
    for a, b_, what in zip(out[True][:3], out[False][:3], ("plane image", "sign bits", "max-abs slot")):
        assert torch.equal(a, b_), what
    assert bool((out[True][3] == CANARY).all()), "the call with a NULL y wrote where the fp32 block would be"
    assert not bool((out[False][3] == CANARY).any()) and bool((out[True][0] != CANARY_BITS).any())
    assert bool((out[True][1] == CANARY_BITS).all()) != bool(relu)
    # NULL without an image: refused on the host
    buf, (_, y, img, mask, _, _) = _arena(c, mask_words)
    assert _raw(lib, "gcl_bn_apply_planes", x, N, c, mean, rstd, w, b, res, relu, None, 0, mask if relu else None,
                _slot(bound), None) == -1
    assert b"NULL" in lib.gcl_last_error() and bool((buf == CANARY).all())


@gpu
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "plain"])
@pytest.mark.parametrize("residual", [1, 0], ids=["residual", "no_residual"])
@pytest.mark.parametrize("c", [128, 256])
def test_backward_apply_with_a_null_fp32_output(c, residual, relu):
    lib = _lib.load()
    x, mean, rstd, w, _, dy = _problem(c, 13 * c + 2 * residual + relu)
    dy = dy * 2.0 ** -8
    mask_words = lib.gcl_bn_mask_len(N, c)
    g = torch.Generator().manual_seed(c + relu)
    bits = torch.randint(-2 ** 62, 2 ** 62, (mask_words,), generator=g, dtype=torch.int64).to(DEV) if relu else None
    sum_g = dy.sum(0).contiguous()
    sum_gx = (dy * (x - mean) * rstd).sum(0).contiguous()
    bound = float(((w * rstd).abs() * (dy.abs().max(0).values + sum_g.abs() / N
                                       + ((x - mean) * rstd).abs().max(0).values * sum_gx.abs() / N)).max()) * 1.25
    out = {}
    for null in (False, True):
        buf, (g0, dx, img, _, dres, g1) = _arena(c, mask_words)
        slot = _slot(bound)
        rc = _raw(lib, "gcl_bn_bwd_apply_planes", x, dy, 0, None, bits, N, c, mean, rstd, w, sum_g, sum_gx, relu,
                  None if null else dx, dres if residual else None, slot, img)
        assert rc == 0, lib.gcl_last_error()
        assert bool((g0 == CANARY).all()) and bool((g1 == CANARY).all())
        out[null] = (img.view(torch.int32).clone(), dres.view(torch.int32).clone(), slot.clone(), dx.clone())      # bits, not floats
    for a, b_, what in zip(out[True][:3], out[False][:3], ("plane image", "dres", "max-abs slot")):
        assert torch.equal(a, b_), what
    assert bool((out[True][3] == CANARY).all()), "the call with a NULL dx wrote where the fp32 block would be"
    assert not bool((out[False][3] == CANARY).any()) and bool((out[True][0] != CANARY_BITS).any())
    assert bool((out[True][1] == CANARY_BITS).all()) != bool(residual)
    buf, (_, dx, img, _, dres, _) = _arena(c, mask_words)
    assert _raw(lib, "gcl_bn_bwd_apply_planes", x, dy, 0, None, bits, N, c, mean, rstd, w, sum_g, sum_gx, relu, None,
                dres if residual else None, _slot(bound), None) == -1
    assert b"NULL" in lib.gcl_last_error() and bool((buf == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------
# 3. the plan against itself with every fp32 twin kept
# ---------------------------------------------------------------------------------------------------------------
def _plan_case(presplit):
    if presplit == 128:
        return _case()
    from gcl_amd.MinkowskiEngine import ops
    if not _CASE_PLANES:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, "PRESPLIT_MIN_C", 64)
            _case(_CASE_PLANES, oracle=_case())
    return _CASE_PLANES


def _run(case, keep, dF, rows, cap):
    plan = case["m"]._plan
    plan.set_keep_fp32(keep)
    try:
        got = _pass(case, dF, rows, cap)
    finally:
        plan.set_keep_fp32(False)
    stats = {k: v.detach().cpu().clone() for k, v in case["m"].state_dict().items() if "running" in k}
    loss = (got["F"].double() * dF.double()).sum()
    return got, stats, loss


@gpu
@pytest.mark.parametrize("k", [0, 37, 129], ids=["dense", "list_37", "list_129"])
@pytest.mark.parametrize("presplit", [128, 64])
def test_plan_without_the_fp32_twins_is_bitwise_the_plan_with_them(presplit, k):
    lib = _lib.load()
    case = _plan_case(presplit)
    n = case["n"]
    assert 1500 < n < 2100
    dF, rows = _dF(n, k if k else 37, 10 + k)          # one output gradient for every pass of the case
    cap = max(128, (k + 127) // 128 * 128)
    rows, cap = (rows, cap) if k else (None, None)
    plan = case["m"]._plan
    assert plan.handle and plan.records
    # which tensors, and how much arena
    names = [name for name, _ in case["m"].named_parameters()]
    label = lambda i: names[plan.records[i]["bn_w"]][:-len(".bn.weight")]
    fwd, bwd = plan.plane_only()
    print(f"presplit {presplit}: forward {[label(i) for i in fwd]}, backward {[label(i) for i in bwd]}")
    if presplit == 128:
        assert {label(i) for i in fwd} == FWD_128 and len(fwd) == 4
        assert {label(i) for i in bwd} == BWD_128 and len(bwd) == 8
    else:
        assert len(fwd) > 4 and len(bwd) > 8
    desc = case["mgr"].native.desc
    blocks = sum(int(desc.n_rows[plan.records[i]["level_out"]]) * plan.records[i]["cout"] * 4 for i in fwd + bwd)
    default = lib.gcl_plan_arena_bytes(plan.handle, ctypes.byref(desc))
    plan.set_keep_fp32(True)
    try:
        assert plan.plane_only() == ([], [])
        kept = lib.gcl_plan_arena_bytes(plan.handle, ctypes.byref(desc))
    finally:
        plan.set_keep_fp32(False)
    print(f"arena: {kept} bytes with the twins, {default} without, {blocks} bytes of skipped blocks")
    assert default > 0 and kept - default == blocks
    # the passes
    a, a_stats, a_loss = _run(case, False, dF, rows, cap)
    b, b_stats, b_loss = _run(case, True, dF, rows, cap)
    again, again_stats, _ = _run(case, False, dF, rows, cap)
    want_rows = cap if k else 0
    for got in (a, b, again):
        assert got["fwd"] == want_rows and got["bwd"] == want_rows, "the pass did not run where the case says"
    assert len(a["grads"]) == 66 and len(a_stats) >= 2 * 21
    assert torch.isfinite(a["F"]).all() and bool(a["F"].any())
    for other, other_stats in ((b, b_stats), (again, again_stats)):
        assert torch.equal(a["F"], other["F"])
        for name, g in a["grads"].items():
            assert torch.isfinite(g).all() and torch.equal(g, other["grads"][name]), name
        for name, v in a_stats.items():
            assert torch.equal(v, other_stats[name]), name
    assert a_loss == b_loss
    assert any(bool(g.any()) for g in a["grads"].values())
