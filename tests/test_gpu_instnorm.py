"""The segmented InstanceNorm of csrc/instnorm.hip (gcl_in_fwd / gcl_in_bwd) and its Python surface.

1. Bitwise against the per-cloud loop: for each cloud, on its contiguous rows, gcl_bn_stats -> gcl_bn_apply ->
   gcl_bn_bwd_reduce -> gcl_bn_bwd_apply with eps 1e-8 -- what ops._InstanceNormFn did before the segmented kernels.  mean,
   rstd, y, dx, dres, the per-cloud sum_g / sum_gx and the two published amax values are torch.equal.  Shapes: cloud sizes
   [1, 63, 64, 65, 700, 50001] at c 32 (one chunk, the chunk edges, 782 chunk sums: past reduce_runs' four-chain loop),
   [131073, 5] at c 32 (128-row chunks), [1, 2, 255, 257, 1000] at c 4 / 64 / 256 (one row lane, rstep 16, rstep 4); each with
   relu 0 / 1 x residual none / given.  The contiguous runs pass rows = NULL.
2. Any row order: the first shape merged by a seeded interleave that keeps each cloud's rows in order, and with the clouds
   in descending order: every row and every table bitwise the contiguous run's.  Fully shuffled rows change the order of
   the sums: against tests/norm_oracle.py per cloud in fp64, y 2e-6 rel-L2, dx 1e-5 rel-L2 without the 1-voxel cloud, the
   affine map's gradients 1e-5 (the bounds of tests/test_gpu_parity.py's InstanceNorm test).  The oracle's backward takes
   the kernel's own ReLU gate (y > 0), as tests/test_gpu_norm_kernels.py does: y is judged separately.
3. Empty cloud: batch indices {0, 2, 3} give, for those clouds, the bits of the dense indexing {0, 1, 2}; the empty cloud's
   table rows are not written.
4. Module level: ME.MinkowskiInstanceNorm(64) on interleaved coordinates, residual + ReLU, forward and backward against the
   fp64 per-cloud formula; a second forward builds no new cloud tables.
5. Model level: a ResUNetIN2C training step's loss, output features and every parameter gradient, torch.equal with
   ops.instance_norm replaced by a copy of the per-cloud autograd function.  The loss kernels add their feature gradient with
   floating-point atomics (csrc/loss.hip), so two backward passes of ONE path already differ (measured: all 66 parameter
   gradients, by up to 5e-8, with either InstanceNorm); the loss gradient is therefore taken once, from the first run, and
   the same tensor is sent back through the network in both runs -- everything the network computes is compared bitwise.
6. Determinism: the first shape twice, identical bits.
Outputs are pre-filled with NaN, the scratch has exactly gcl_in_scratch_len doubles and a guard that must come back."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from torch.autograd.function import once_differentiable

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO                                               # noqa: E402

from gcl_amd import _lib                                               # noqa: E402

DEV = "cuda:0"
EPS = 1e-8
GUARD, SENT = 64, -7777.25
FIRST = ((1, 63, 64, 65, 700, 50001), 32)
SHAPES = [FIRST, ((131073, 5), 32), ((1, 2, 255, 257, 1000), 4), ((1, 2, 255, 257, 1000), 64), ((1, 2, 255, 257, 1000), 256)]
OUT = ("mean", "rstd", "y", "dx", "dres", "sum_g", "sum_gx", "amax_y", "amax_dx")


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def _data(sizes, c):
    """x, dy, residual [n, c] (clouds contiguous, in index order; every cloud with a mean and a spread of its own), w, b."""
    g = torch.Generator().manual_seed(1000 * c + sum(sizes))
    n = sum(sizes)
    x = torch.randn(n, c, generator=g)
    r0 = 0
    for i, m in enumerate(sizes):
        x[r0:r0 + m] = x[r0:r0 + m] * (0.5 + i) + (i - 2) * 0.75
        r0 += m
    dy, res = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    return tuple(t.to(DEV) for t in (x, dy, res, w, b))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _amax(slot):
    return slot.view(-1, 32)[:, 0].max().view(1).view(torch.float32).clone()


def _tables(cloud_of_row, n_clouds):
    """seg_off, rows, row_cloud (device) of a host vector of cloud indices: a stable grouping of the rows by cloud."""
    lab = torch.as_tensor(cloud_of_row, dtype=torch.int64)
    order = torch.sort(lab, stable=True)[1]
    seg = torch.zeros(n_clouds + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.bincount(lab, minlength=n_clouds), 0)
    return seg.to(DEV), order.to(torch.int32).to(DEV), lab.to(torch.int32).to(DEV)


def _segmented(x, dy, res, w, b, cloud_of_row, n_clouds, relu, identity=False):
    lib = _lib.load()
    n, c = x.shape
    seg_off, rows, row_cloud = _tables(cloud_of_row, n_clouds)
    if identity:
        assert torch.equal(rows.cpu(), torch.arange(n, dtype=torch.int32))
        rows = None
    o = dict(mean=_nan(n_clouds, c), rstd=_nan(n_clouds, c), y=_nan(n, c), dx=_nan(n, c), dres=_nan(n, c) if res is not None else None,
             sum_g=_nan(n_clouds, c), sum_gx=_nan(n_clouds, c))
    slot_y, slot_dx = (torch.zeros(512, dtype=torch.int32, device=DEV) for _ in range(2))
    mask = torch.empty(lib.gcl_bn_mask_len(n, c), dtype=torch.int64, device=DEV) if relu else None
    st = _lib.stream()
    ln = lib.gcl_in_scratch_len(n, n_clouds, c)
    scratch = [torch.full((ln + GUARD,), SENT, dtype=torch.float64, device=DEV) for _ in range(2)]
    _lib.check(lib.gcl_in_fwd(_lib.ptr(x), n, c, _lib.ptr(seg_off), _lib.ptr(rows), _lib.ptr(row_cloud), n_clouds, EPS,
                              _lib.ptr(w), _lib.ptr(b), _lib.ptr(res), int(relu), _lib.ptr(scratch[0]), _lib.ptr(o["mean"]),
                              _lib.ptr(o["rstd"]), _lib.ptr(o["y"]), _lib.ptr(mask), _lib.ptr(slot_y), st), "gcl_in_fwd")
    _lib.check(lib.gcl_in_bwd(_lib.ptr(x), _lib.ptr(dy), n, c, _lib.ptr(seg_off), _lib.ptr(rows), _lib.ptr(row_cloud), n_clouds,
                              _lib.ptr(o["mean"]), _lib.ptr(o["rstd"]), _lib.ptr(w), int(relu), _lib.ptr(mask),
                              _lib.ptr(scratch[1]), _lib.ptr(o["sum_g"]), _lib.ptr(o["sum_gx"]), _lib.ptr(o["dx"]),
                              _lib.ptr(o["dres"]), _lib.ptr(slot_dx), st), "gcl_in_bwd")
    torch.cuda.synchronize()
    for s in scratch:
        assert bool((s[ln:] == SENT).all()), "a write past gcl_in_scratch_len doubles"
    o["amax_y"], o["amax_dx"] = _amax(slot_y), _amax(slot_dx)
    return o


def _per_cloud_loop(x, dy, res, w, b, sizes, relu):
    """The reference: every cloud through the public BatchNorm entries on its contiguous rows."""
    lib = _lib.load()
    n, c = x.shape
    ns = len(sizes)
    o = dict(mean=_nan(ns, c), rstd=_nan(ns, c), y=_nan(n, c), dx=_nan(n, c), dres=_nan(n, c) if res is not None else None,
             sum_g=_nan(ns, c), sum_gx=_nan(ns, c))
    slot_y, slot_dx = (torch.zeros(512, dtype=torch.int32, device=DEV) for _ in range(2))
    st = _lib.stream()
    r0 = 0
    for s, m in enumerate(sizes):
        sl = slice(r0, r0 + m)
        scratch = torch.empty(lib.gcl_bn_scratch_len(m, c), dtype=torch.float64, device=DEV)
        mask = torch.empty(lib.gcl_bn_mask_len(m, c), dtype=torch.int64, device=DEV) if relu else None
        _lib.check(lib.gcl_bn_stats(_lib.ptr(x[sl]), m, c, EPS, 0.0, None, None, _lib.ptr(scratch), _lib.ptr(o["mean"][s]),
                                    _lib.ptr(o["rstd"][s]), st), "gcl_bn_stats")
        _lib.check(lib.gcl_bn_apply(_lib.ptr(x[sl]), m, c, _lib.ptr(o["mean"][s]), _lib.ptr(o["rstd"][s]), _lib.ptr(w), _lib.ptr(b),
                                    _lib.ptr(res[sl]) if res is not None else None, int(relu), _lib.ptr(o["y"][sl]),
                                    _lib.ptr(mask), _lib.ptr(slot_y), st), "gcl_bn_apply")
        _lib.check(lib.gcl_bn_bwd_reduce(_lib.ptr(x[sl]), _lib.ptr(dy[sl]), None, _lib.ptr(mask), m, c, _lib.ptr(o["mean"][s]),
                                         _lib.ptr(o["rstd"][s]), int(relu), _lib.ptr(scratch), _lib.ptr(o["sum_g"][s]),
                                         _lib.ptr(o["sum_gx"][s]), st), "gcl_bn_bwd_reduce")
        _lib.check(lib.gcl_bn_bwd_apply(_lib.ptr(x[sl]), _lib.ptr(dy[sl]), None, _lib.ptr(mask), m, c, _lib.ptr(o["mean"][s]),
                                        _lib.ptr(o["rstd"][s]), _lib.ptr(w), _lib.ptr(o["sum_g"][s]), _lib.ptr(o["sum_gx"][s]),
                                        int(relu), _lib.ptr(o["dx"][sl]), _lib.ptr(o["dres"][sl]) if res is not None else None,
                                        _lib.ptr(slot_dx), st), "gcl_bn_bwd_apply")
        r0 += m
    torch.cuda.synchronize()
    o["amax_y"], o["amax_dx"] = _amax(slot_y), _amax(slot_dx)
    return o


def _labels(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


@functools.lru_cache(maxsize=None)
def _contiguous(sizes, c, relu, with_res):
    x, dy, res, w, b = _data(sizes, c)
    return _segmented(x, dy, res if with_res else None, w, b, _labels(sizes), len(sizes), relu, identity=True)


def _same(got, want, keys=OUT):
    for k in keys:
        if want[k] is None:
            assert got[k] is None
            continue
        assert not torch.isnan(want[k]).any(), k
        assert torch.equal(got[k], want[k]), (k, (got[k] != want[k]).sum().item())


# ---- 1. bitwise against the per-cloud loop --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("sizes,c", SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"c{v}")
def test_bitwise_the_per_cloud_loop(sizes, c, relu, with_res):
    x, dy, res, w, b = _data(sizes, c)
    want = _per_cloud_loop(x, dy, res if with_res else None, w, b, sizes, relu)
    _same(_contiguous(sizes, c, relu, with_res), want)


# ---- 2. any row order ------------------------------------------------------------------------------------------------------
def _merged(sizes, lab):
    """src[j]: the row of the contiguous layout that row j of the layout ``lab`` (cloud of each row) holds, every cloud's
    rows kept in their order."""
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    seen = np.zeros(len(sizes), dtype=np.int64)
    src = np.empty(len(lab), dtype=np.int64)
    for cl in range(len(sizes)):
        at = np.nonzero(lab == cl)[0]
        src[at] = starts[cl] + np.arange(len(at))
        seen[cl] = len(at)
    assert (seen == np.asarray(sizes)).all()
    return torch.from_numpy(src).to(DEV)


@pytest.mark.parametrize("order", ["interleaved", "descending"])
def test_rows_in_any_order_keep_the_bits(order):
    sizes, c = FIRST
    if order == "interleaved":
        lab = np.random.RandomState(7).permutation(_labels(sizes))
    else:
        lab = _labels(sizes)[::-1].copy()
    src = _merged(sizes, lab)
    x, dy, res, w, b = _data(sizes, c)
    got = _segmented(x[src].contiguous(), dy[src].contiguous(), res[src].contiguous(), w, b, lab, len(sizes), 1)
    want = _contiguous(sizes, c, 1, True)
    _same(got, want, ("mean", "rstd", "sum_g", "sum_gx", "amax_y", "amax_dx"))
    for k in ("y", "dx", "dres"):
        assert torch.equal(got[k], want[k][src]), k


def test_shuffled_rows_against_the_fp64_oracle():
    sizes, c = FIRST
    x, dy, res, w, b = _data(sizes, c)
    perm = torch.from_numpy(np.random.RandomState(8).permutation(sum(sizes))).to(DEV)
    lab = _labels(sizes)[perm.cpu().numpy()]
    xs, gs, rs = x[perm].contiguous(), dy[perm].contiguous(), res[perm].contiguous()
    got = _segmented(xs, gs, rs, w, b, lab, len(sizes), 1)
    xs, gs, rs, w, b = (t.cpu().numpy() for t in (xs, gs, rs, w, b))
    y, dx = np.empty(xs.shape), np.empty(xs.shape)
    dw, db = np.zeros(c), np.zeros(c)
    gate = got["y"].cpu().numpy() > 0
    for cl, m in enumerate(sizes):
        at = np.nonzero(lab == cl)[0]
        mean, rstd, _, _ = NO.bn_stats(xs[at], EPS, 0.0)
        y[at] = NO.bn_apply(xs[at], mean, rstd, w, b, rs[at], True)[0]
        sg, sx, _ = NO.bn_bwd_sums(xs[at], gs[at], gate[at], mean, rstd)
        dx[at] = NO.bn_bwd_apply(xs[at], gs[at], gate[at], mean, rstd, w, sg, sx, m)[0]
        dw, db = dw + sx, db + sg
    keep = lab != 0                                              # cloud 0 has one voxel: variance 0, gradient scaled by 1e4
    e = dict(y=rel_l2(got["y"].cpu(), y), dx=rel_l2(got["dx"].cpu().numpy()[keep], dx[keep]),
             dw=rel_l2(got["sum_gx"].sum(0).cpu(), dw), db=rel_l2(got["sum_g"].sum(0).cpu(), db))
    print("shuffled rows, rel-L2:", e)
    assert e["y"] < 2e-6 and e["dx"] < 1e-5 and e["dw"] < 1e-5 and e["db"] < 1e-5, e
    assert torch.equal(got["dres"], torch.where(got["y"] > 0, torch.from_numpy(gs).to(DEV), torch.zeros((), device=DEV)))


# ---- 3. empty cloud --------------------------------------------------------------------------------------------------------
def test_an_empty_cloud_is_skipped():
    sizes, c = (255, 257, 1000), 64
    x, dy, res, w, b = _data(sizes, c)
    dense = _segmented(x, dy, res, w, b, _labels(sizes), 3, 1, identity=True)
    lab = np.asarray([0, 2, 3])[_labels(sizes)]
    got = _segmented(x, dy, res, w, b, lab, 4, 1, identity=True)
    _same(got, dense, ("y", "dx", "dres", "amax_y", "amax_dx"))
    for k in ("mean", "rstd", "sum_g", "sum_gx"):
        assert torch.equal(got[k][[0, 2, 3]], dense[k]), k
        assert bool(torch.isnan(got[k][1]).all()), k + ": the empty cloud's row was written"


# ---- 4. module level -------------------------------------------------------------------------------------------------------
def test_module_on_interleaved_coordinates():
    import gcl_amd.MinkowskiEngine as ME
    g = torch.Generator().manual_seed(12)
    sizes, c = [700, 33, 1500, 1], 64
    lab = torch.from_numpy(np.random.RandomState(9).permutation(_labels(sizes)))
    n = len(lab)
    C = torch.stack([lab, torch.arange(n), torch.zeros(n, dtype=torch.int64), lab], 1).to(torch.int32).to(DEV)
    x = (torch.randn(n, c, generator=g) * 2 + 0.5).to(DEV).requires_grad_(True)
    r = torch.randn(n, c, generator=g).to(DEV).requires_grad_(True)
    wgt = torch.randn(n, c, generator=g).to(DEV)
    norm = ME.MinkowskiInstanceNorm(c, dimension=3).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(1, c, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(1, c, generator=g) * 0.1)
    xs = ME.SparseTensor(x, coordinates=C)
    rs = ME.SparseTensor(r, coordinate_map_key=xs.coordinate_map_key, coordinate_manager=xs.coordinate_manager)
    y = norm(xs, residual=rs, relu=True).F
    (y * wgt).sum().backward()
    xd, rd = x.detach().double().requires_grad_(True), r.detach().double().requires_grad_(True)
    wd, bd = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    out = torch.zeros(n, c, dtype=torch.float64, device=DEV)
    for cl in range(len(sizes)):
        at = torch.nonzero(lab == cl)[:, 0].to(DEV)
        seg = xd[at]
        mu = seg.mean(0, keepdim=True)
        var = ((seg - mu) ** 2).mean(0, keepdim=True)
        out = out.index_add(0, at, (seg - mu) / torch.sqrt(var + 1e-8) * wd + bd)
    yr = torch.relu(out + rd)
    (yr * wgt.double()).sum().backward()
    keep = (lab != 3).numpy()                                    # the 1-voxel cloud: variance 0, gradient scaled by 1e4
    e = dict(y=rel_l2(y.detach().cpu(), yr.detach().cpu()), dx=rel_l2(x.grad.cpu().numpy()[keep], xd.grad.cpu().numpy()[keep]),
             dres=rel_l2(r.grad.cpu(), rd.grad.cpu()), dw=rel_l2(norm.weight.grad.cpu(), wd.grad.cpu()),
             db=rel_l2(norm.bias.grad.cpu(), bd.grad.cpu()))
    print("module, rel-L2:", e)
    assert e["y"] < 2e-6 and e["dx"] < 1e-5 and e["dres"] < 2e-6 and e["dw"] < 1e-5 and e["db"] < 1e-5, e
    # a second forward on the same manager reuses the cached tables
    mgr = xs.coordinate_manager
    before = dict(mgr._cloud_rows)
    assert list(before) == [1] and before[1][3] == 4
    y2 = norm(xs, residual=rs, relu=True).F
    assert list(mgr._cloud_rows) == [1] and mgr._cloud_rows[1] is before[1]
    assert torch.equal(y2, y)


# ---- 5. model level --------------------------------------------------------------------------------------------------------
class _PerCloudInstanceNormFn(torch.autograd.Function):
    """The autograd function InstanceNorm ran on before the segmented kernels: a loop over clouds (row segments), each through
    the BatchNorm entries on its row range."""

    @staticmethod
    def forward(ctx, x, weight, bias, segments, eps, residual, relu):
        from gcl_amd.MinkowskiEngine import ops
        lib = _lib.require_gpu()
        x = x.contiguous()
        n, c = x.shape
        dev = x.device
        ns = len(segments)
        mean = torch.empty((ns, c), dtype=torch.float32, device=dev)
        rstd = torch.empty((ns, c), dtype=torch.float32, device=dev)
        res = residual.contiguous() if residual is not None else None
        y = torch.empty_like(x)
        w, b = weight.detach().contiguous().view(-1), bias.detach().contiguous().view(-1)
        ops._LAST_BN_AMAX = slot = ops.amax_slot(dev) if ops.PRECISION == "fp16x3" else None
        masks = []
        st = _lib.stream()
        for s, (r0, rows) in enumerate(segments):
            xs = x[r0:r0 + rows]
            scratch = torch.empty(lib.gcl_bn_scratch_len(rows, c), dtype=torch.float64, device=dev)
            _lib.check(lib.gcl_bn_stats(_lib.ptr(xs, torch.float32), rows, c, float(eps), 0.0, None, None,
                                        _lib.ptr(scratch), _lib.ptr(mean[s]), _lib.ptr(rstd[s]), st), "gcl_bn_stats")
            mask = torch.empty(lib.gcl_bn_mask_len(rows, c), dtype=torch.int64, device=dev) if relu else None
            masks.append(mask)
            _lib.check(lib.gcl_bn_apply(_lib.ptr(xs), rows, c, _lib.ptr(mean[s]), _lib.ptr(rstd[s]), _lib.ptr(w),
                                        _lib.ptr(b), _lib.ptr(res[r0:r0 + rows]) if res is not None else None,
                                        int(relu), _lib.ptr(y[r0:r0 + rows]), _lib.ptr(mask), _lib.ptr(slot), st),
                       "gcl_bn_apply")
        ctx.save_for_backward(x, weight, mean, rstd, *[m for m in masks if m is not None])
        ctx.segments, ctx.relu, ctx.has_res = segments, bool(relu), residual is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from gcl_amd.MinkowskiEngine import ops
        lib = _lib.load()
        x, weight, mean, rstd, *masks = ctx.saved_tensors
        n, c = x.shape
        dev = x.device
        dy = dy.contiguous()
        ns = len(ctx.segments)
        sum_g = torch.empty((ns, c), dtype=torch.float32, device=dev)
        sum_gx = torch.empty((ns, c), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        w = weight.detach().contiguous().view(-1)
        slot = ops.amax_slot(dev) if ops.PRECISION == "fp16x3" else None
        st = _lib.stream()
        for s, (r0, rows) in enumerate(ctx.segments):
            xs, gs = x[r0:r0 + rows], dy[r0:r0 + rows]
            mask = masks[s] if ctx.relu else None
            scratch = torch.empty(lib.gcl_bn_scratch_len(rows, c), dtype=torch.float64, device=dev)
            _lib.check(lib.gcl_bn_bwd_reduce(_lib.ptr(xs), _lib.ptr(gs), None, _lib.ptr(mask), rows, c,
                                             _lib.ptr(mean[s]), _lib.ptr(rstd[s]), int(ctx.relu), _lib.ptr(scratch),
                                             _lib.ptr(sum_g[s]), _lib.ptr(sum_gx[s]), st), "gcl_bn_bwd_reduce")
            _lib.check(lib.gcl_bn_bwd_apply(_lib.ptr(xs), _lib.ptr(gs), None, _lib.ptr(mask), rows, c,
                                            _lib.ptr(mean[s]), _lib.ptr(rstd[s]), _lib.ptr(w), _lib.ptr(sum_g[s]),
                                            _lib.ptr(sum_gx[s]), int(ctx.relu), _lib.ptr(dx[r0:r0 + rows]),
                                            _lib.ptr(dres[r0:r0 + rows]) if dres is not None else None,
                                            _lib.ptr(slot), st), "gcl_bn_bwd_apply")
        if slot is not None:
            ops.tag_amax(dx, slot)
        return dx, sum_gx.sum(0).view_as(weight), sum_g.sum(0).view_as(weight), None, None, dres, None


def _per_cloud_instance_norm(x, weight, bias, clouds, eps=1e-8, residual=None, relu=False):
    from gcl_amd.MinkowskiEngine import ops
    seg_off, rows, _, _ = clouds
    assert torch.equal(rows.cpu(), torch.arange(rows.shape[0], dtype=torch.int32)), "the loop needs contiguous clouds"
    off = seg_off.tolist()
    segments = [(off[i], off[i + 1] - off[i]) for i in range(len(off) - 1)]
    ops.tape_guard("MinkowskiInstanceNorm", x, residual)
    y = _PerCloudInstanceNormFn.apply(x, weight, bias, segments, eps, residual, relu)
    if ops._LAST_BN_AMAX is not None:
        ops.tag_amax(y, ops._LAST_BN_AMAX)
    return y


def test_model_step_is_bitwise_the_per_cloud_path(monkeypatch):
    from gcl_amd import synthetic
    from gcl_amd.MinkowskiEngine import ops
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    batch = synthetic.make_train_batch(79, batch_size=1, num_neighborhood=1, n_boxes=12)
    assert len(torch.unique(batch["sinput_C"][:, 0])) == 2
    torch.manual_seed(3)
    tr = FinestContrastiveLossTrainer(make_config(model="ResUNetIN2C", batch_size=1, num_pos_per_batch=64,
                                                  num_hn_samples_per_batch=128), device=DEV)
    tr.model.train()
    np.random.seed(4)
    draws = tr._draw_for(batch)
    calls = []

    def step(dF=None):
        for p in tr.model.parameters():
            p.grad = None
        with torch.cuda.device(DEV):
            loss, parts, F_out = tr.forward_loss(batch, draws, fused_total=True)
            if dF is None:
                dF = torch.autograd.grad(loss, F_out, retain_graph=True)[0]
            F_out.backward(dF)
        torch.cuda.synchronize()
        return [loss.detach().clone(), F_out.detach().clone()] + [p.detach().clone() for p in parts], \
            {k: p.grad.detach().clone() for k, p in tr.model.named_parameters()}, dF

    shipped = step()

    def counted(*a, **k):
        calls.append(1)
        return _per_cloud_instance_norm(*a, **k)

    monkeypatch.setattr(ops, "instance_norm", counted)
    looped = step(shipped[2])
    assert len(calls) >= 14, "the per-cloud copy did not run"
    for a, b in zip(shipped[0], looped[0]):
        assert torch.equal(a, b)
    assert shipped[1].keys() == looped[1].keys() and "block1.norm1.weight" in shipped[1]
    for k in shipped[1]:
        assert torch.isfinite(shipped[1][k]).all(), k
        assert torch.equal(shipped[1][k], looped[1][k]), k


# ---- 6. determinism --------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    sizes, c = FIRST
    x, dy, res, w, b = _data(sizes, c)
    again = _segmented(x, dy, res, w, b, _labels(sizes), len(sizes), 1, identity=True)
    _same(again, _contiguous(sizes, c, 1, True))
