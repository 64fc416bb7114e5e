"""Pins tests/norm_oracle.py (the fp64 references of the kernels of csrc/norm.hip) against torch's autograd, asserts the
conditions that tests/test_gpu_norm_kernels.py promises for its generated inputs, and evaluates the kernels' expressions
in numpy fp32 on the same inputs: the bounds of the GPU file must be satisfiable by correct fp32 arithmetic without fused
multiply-adds (the compiler's contractions only remove roundings)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO                                               # noqa: E402
import test_gpu_norm_kernels as GK                                     # noqa: E402  (case tables and generators only)

F32, F64, U = np.float32, np.float64, 2.0 ** -24
EPS, MOM = NO._f32(GK.EPS), NO._f32(GK.MOM)


# ---- the oracle against autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("c,n,res,relu", [(4, 7, False, False), (12, 33, True, True), (32, 130, False, True)])
def test_oracle_equals_autograd(c, n, res, relu, training):
    g = torch.Generator().manual_seed(c * 1000 + n)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, r, gy = rnd(n, c) * 2 + 1, (rnd(n, c) if res else None), rnd(n, c)
    w, b, rm, rv = rnd(c), rnd(c), rnd(c), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, b))
    ro = r.clone().requires_grad_(True) if res else None
    rmo, rvo = rm.clone(), rv.clone()
    yo = torch.nn.functional.batch_norm(xo, rmo, rvo, wo, bo, training, MOM, EPS)
    if res:
        yo = yo + ro
    if relu:
        yo = torch.relu(yo)
    yo.backward(gy)

    xn, wn, bn, gn = x.numpy(), w.numpy(), b.numpy(), gy.numpy()
    rn = r.numpy() if res else None
    if training:
        mean, rstd, new_rm, new_rv = NO.bn_stats(xn, EPS, MOM, rm.numpy(), rv.numpy())
        assert np.abs(new_rm - rmo.numpy()).max() <= 1e-12 and np.abs(new_rv - rvo.numpy()).max() <= 1e-12
    else:
        mean, rstd = rm.numpy(), 1.0 / np.sqrt(rv.numpy() + EPS)
    y, mag = NO.bn_apply(xn, mean, rstd, wn, bn, rn, relu)
    assert np.abs(y - yo.detach().numpy()).max() <= 1e-12 and (mag >= np.abs(y) - 1e-12).all()
    gate = (y > 0) if relu else None
    sum_g, sum_gx, abs_gx = NO.bn_bwd_sums(xn, gn, gate, mean, rstd)
    assert (abs_gx >= np.abs(sum_gx) - 1e-12).all()
    z = np.zeros(c)
    dx, dres, mag = NO.bn_bwd_apply(xn, gn, gate, mean, rstd, wn, sum_g if training else z, sum_gx if training else z, n)
    assert np.abs(dx - xo.grad.numpy()).max() <= 1e-12 and (mag >= np.abs(dx) - 1e-12).all()
    assert np.abs(sum_gx - wo.grad.numpy()).max() <= 1e-12          # dweight
    assert np.abs(sum_g - bo.grad.numpy()).max() <= 1e-12           # dbias
    if res:
        assert np.abs(dres - ro.grad.numpy()).max() <= 1e-12


def test_stats_of_one_row_and_from_partials():
    x = np.array([[1.5, -2.0, 0.25, 3.0]])
    mean, rstd, rm, rv = NO.bn_stats(x, EPS, MOM, np.zeros(4), np.ones(4))
    assert (mean == x[0]).all() and np.allclose(rstd, 1 / np.sqrt(EPS), rtol=1e-15)
    assert np.allclose(rv, 1 - MOM, rtol=1e-15)            # the variance is 0: moves toward 0 by the momentum
    c, nt = 8, 3
    n = GK.tiles_n(nt)
    xs, _, _ = GK.gen_x(c, n, "tiles")
    part = GK.tile_partials(xs, nt)
    a, b = NO.bn_stats(xs, EPS, MOM, np.zeros(c), np.ones(c)), NO.bn_stats_from_partials(part, n, EPS, MOM, np.zeros(c), np.ones(c))
    for u, v in zip(a, b[:4]):                             # fp32 tile sums: a few 1e-7 of the mean / the variance
        assert np.allclose(u, v, rtol=2e-5, atol=2e-6)
    assert (b[4] == np.stack([xs.min(0), xs.max(0)])).all()


def test_row_normalize_and_sgd_oracles_equal_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, 16, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(9, 16, generator=g, dtype=torch.float64)
    y = x / torch.norm(x, p=2, dim=1, keepdim=True)
    y.backward(dy)
    yn, norm = NO.row_normalize_fwd(x.detach().numpy())
    dx, mag = NO.row_normalize_bwd(yn, dy.numpy(), norm)
    assert np.abs(yn - y.detach().numpy()).max() <= 1e-14 and np.abs(dx - x.grad.numpy()).max() <= 1e-12
    assert (mag >= np.abs(dx) - 1e-12).all()
    lr, mom, wd = (NO._f32(v) for v in (0.1, 0.8, 1e-4))
    p = torch.nn.Parameter(torch.randn(50, generator=g, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd)
    mine, buf = p.detach().numpy().copy(), None
    for step in range(3):
        p.grad = torch.randn(50, generator=g, dtype=torch.float64)
        mine, buf, _, _ = NO.sgd_step(mine, p.grad.numpy(), buf, lr, mom, wd, step == 0)
        opt.step()
        assert np.abs(mine - p.detach().numpy()).max() <= 1e-14
    assert np.abs(NO.col_sum(dy.numpy()) - dy.sum(0).numpy()).max() <= 1e-14


# ---- the mask -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c", [(37, 12), (1, 4), (64, 4), (65, 4), (3, 1024)])
def test_mask_round_trip(n, c):
    """(37, 12): 111 quads, the second group of words is used up to bit 46; (1, 4): one bit of four words."""
    bits = np.random.default_rng(n * c).random((n, c)) < 0.5
    words = NO.pack_mask(bits, n, c)
    assert words.dtype == np.uint64 and len(words) == NO.mask_len(n, c) == -(-n * (c // 4) // 64) * 4
    assert (NO.unpack_mask(words, n, c) == bits).all()
    used = n * (c // 4) - (len(words) // 4 - 1) * 64       # bits of the last group of four words that stand for a quad
    if used < 64:
        assert (words[-4:] >> np.uint64(used) == 0).all()
    one = np.zeros((n, c), bool)
    e, comp = n * (c // 4) - 1, 2                          # the last quad's third channel
    one.reshape(-1, 4)[e, comp] = True
    w = NO.pack_mask(one, n, c)
    assert w[(e >> 6) * 4 + comp] == np.uint64(1) << np.uint64(e & 63) and np.count_nonzero(w) == 1


# ---- the plane image -------------------------------------------------------------------------------------------------------
def test_planes_image_layout_and_value():
    y = (np.random.default_rng(0).standard_normal((5, 64)) * 3).astype(F32)
    amax = np.abs(y).max()
    s = NO.amax_scale(amax)
    assert 2.0 ** 13 <= amax * s < 2.0 ** 14 and np.log2(s) == int(np.log2(s))
    assert NO.amax_scale(0.0) == 1 and NO.amax_scale(np.float32(3.1e38)) == 1
    img = NO.planes_image(y, amax, ld=96, fill=0x7B7B)
    assert img.shape == (5, 3, 2, 32) and (img[:, 2] == 0x7B7B).all()
    flat = img.reshape(-1)
    row, ch = 3, 45
    unit = row * 96 * 2 + (ch // 32) * 64 + ch % 32
    hi, lo = flat[unit:unit + 1].view(np.float16)[0], flat[unit + 32:unit + 33].view(np.float16)[0]
    assert hi == np.float16(y[row, ch] * s)
    back = (F64(hi) + F64(lo) / 2048) / s
    assert abs(back - y[row, ch]) <= 2.0 ** -21 * amax     # hi + lo / 2^11 carries 22 bits of the scaled value


# ---- conditions of the GPU file's inputs -----------------------------------------------------------------------------------
def _rows_per_wg(n):
    rows = 1024
    while rows > 64 and n // rows < 1024:
        rows >>= 1
    return rows


def test_case_tables_reach_the_branches():
    nwg = {(-(-n // _rows_per_wg(n)), _rows_per_wg(n)) for _, n in GK.STATS_CASES}
    assert {(k, 64) for k in (1, 2, 255, 256, 257, 1023, 1024, 1025)} <= nwg and (1025, 128) in nwg
    assert {c for c, _ in GK.STATS_CASES} == {4, 8, 16, 32, 64, 128, 256, 512, 1024}
    for c in GK.ODD:
        outcomes = {GK.apply_hoisted(c, n) for cc, n in GK.APPLY_CASES if cc == c}
        assert outcomes == {True, False}, c
    for c in GK.POW2:
        assert all(GK.apply_hoisted(c, n) for cc, n in GK.APPLY_CASES if cc == c)
    total4 = sorted(n * (c // 4) for c, n in GK.APPLY_CASES)
    S = GK.APPLY_S
    assert total4[0] < S and S in total4 and any(S < t < 2 * S for t in total4) and any(t > 2 * S for t in total4)
    assert not GK.apply_hoisted(96, 87400) and 87400 * 24 > 2 * S and GK.apply_grid(96, 87400) == 4096
    assert GK.tiles_n(2049) * 32 * 4 <= 34 * 2 ** 20       # the largest tensor
    # SGD: vector and scalar bodies, the tail, a second sweep of 128 x 256 threads
    sweep = 128 * 256
    assert any(s % 4 for s in GK.SGD_SIZES) and any(s // 4 > sweep for s in GK.SGD_SIZES) and any(s > 2 * sweep and s % 4 for s in GK.SGD_SIZES)


@pytest.mark.parametrize("c,n", GK.STATS_CASES)
def test_stats_inputs_have_mean_within_ten_deviations(c, n):
    if n == 1:
        return                                             # one row: ss / n - m^2 is exactly 0 (fp32 squares are exact in fp64)
    x = GK.gen_x(c, n, "stats")[0].astype(F64)
    assert (np.abs(x.mean(0)) <= 10 * x.std(0)).all()
    g = GK.gen_bwd(c, n)
    bits, y = g[5], g[6]
    assert ((y > 0) == bits).all() and ((y[~bits] == 0).any() or n * c < 64)
    if n >= 63:
        frac = bits.mean(0)
        assert (frac >= 0.1).all() and (frac <= 0.9).all()


@pytest.mark.parametrize("c,nt", GK.TILES_CASES)
def test_tile_inputs_have_mean_within_ten_deviations(c, nt):
    n, x, w, _ = GK.gen_tiles(c, nt)
    x = x.astype(F64)
    assert n % GK.TILE != 0 and -(-n // GK.TILE) == nt
    assert (np.abs(x.mean(0)) <= 10 * x.std(0)).all() and (w < 0).any() and (w > 0).any()


@pytest.mark.parametrize("c,n", GK.APPLY_CASES)
def test_apply_inputs_have_both_signs(c, n):
    """At least 10 % of a channel's elements on each side of the ReLU from 64 rows on; over the whole tensor below that (a
    channel of 5 rows cannot promise tenths), no claim below 40 elements."""
    x, mean, rstd, w, b, res = GK.gen_apply(c, n)
    if n >= 63:                                            # mean and rstd are inputs here; the generator is the same
        for xs in (x.astype(F64), GK.gen_bwd(c, n)[0].astype(F64)):
            assert (np.abs(xs.mean(0)) <= 10 * xs.std(0)).all()
    for r in (None, res):
        pos = NO.bn_apply(x, mean, rstd, w, b, r, False)[0] > 0
        frac = pos.mean(0) if n >= 64 else np.array([pos.mean()]) if n * c >= 40 else np.array([0.5])
        assert (frac >= 0.1).all() and (frac <= 0.9).all(), (frac.min(), frac.max())
    if n >= 64:
        bits = GK.gen_bwd(c, n)[5].mean(0)
        assert (bits >= 0.1).all() and (bits <= 0.9).all()


# ---- the kernels' expressions in numpy fp32 ----------------------------------------------------------------------------------
# measured worst |err| / (u x magnitude) over EMU_SHAPES (and ROWNORM_C x {257}), next to the bound it stands under
MEASURED = {              # bound
    "y": 3.44,            # 6
    "dx": 3.83,           # 12
    "sum_gx": 0.27,       # 3 (relative to sum |g||xhat| + |want|; 2 more on |want|)
    "rownorm_fwd": 2.50,  # log2(c) + 6
    "rownorm_bwd": 2.36,  # log2(c) + 8
    "sgd_buf": 1.69,      # 3
    "sgd_p": 2.31,        # 2 (+ lr x buf's error, counted in this figure)
}
EMU_SHAPES = [(4, 1000), (32, 1000), (96, 257), (256, 257), (1024, 257)]


def emu_apply(x, mean, rstd, w, b, res, relu):
    o = (x - mean) * rstd * w + b
    if res is not None:
        o = o + res
    return np.maximum(o, F32(0)) if relu else o


def emu_bwd_apply(x, g, gate, mean, rstd, w, sg, sx, n):
    inv_n = F32(1) / F32(n)
    g = np.where(gate, g, F32(0)) if gate is not None else g
    return w * rstd * (g - sg * inv_n - (x - mean) * rstd * sx * inv_n)


def emu_sum_gx(x, g, gate, mean, rstd):
    g = np.where(gate, g, F32(0)) if gate is not None else g
    xhat = (x - mean) * rstd                               # fp32, two roundings
    return (g.astype(F64) * xhat.astype(F64)).sum(0).astype(F32)


def _lane_sum(prod):
    """[n, c] products -> [n]: x + y + z + w in a lane, then the xor butterfly over c / 4 lanes (a balanced tree)."""
    n, c = prod.shape
    q = prod.reshape(n, c // 4, 4)
    a = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def emu_rownorm_fwd(x):
    nr = np.sqrt(_lane_sum(x * x))
    return x / nr[:, None], nr


def emu_rownorm_bwd(y, dy, nr):
    s = _lane_sum(y * dy)
    return (dy - y * s[:, None]) / nr[:, None]


def _ratio(got, want, mag):
    return float((np.abs(got.astype(F64) - want) / (U * np.maximum(mag, 1e-300))).max())


def fp32_emulation_ratios():
    worst = dict.fromkeys(MEASURED, 0.0)
    for c, n in EMU_SHAPES:
        x, mean, rstd, w, b, res = GK.gen_apply(c, n)
        for r in (None, res):
            for relu in (0, 1):
                want, mag = NO.bn_apply(x, mean, rstd, w, b, r, relu)
                worst["y"] = max(worst["y"], _ratio(emu_apply(x, mean, rstd, w, b, r, relu), want, mag))
        x, mean, rstd, w, g, bits, _, sums = GK.gen_bwd(c, n)
        for gate in (None, bits):
            for s in (sums, np.zeros_like(sums)):
                want, _, mag = NO.bn_bwd_apply(x, g, gate, mean, rstd, w, s[0], s[1], n)
                worst["dx"] = max(worst["dx"], _ratio(emu_bwd_apply(x, g, gate, mean, rstd, w, s[0], s[1], n), want, mag))
            _, want, abs_gx = NO.bn_bwd_sums(x, g, gate, mean, rstd)
            got = emu_sum_gx(x, g, gate, mean, rstd)
            assert (np.abs(got - want) <= 3 * U * abs_gx + 2 * U * np.abs(want)).all()
            worst["sum_gx"] = max(worst["sum_gx"], _ratio(got, want, abs_gx + np.abs(want)))
    for c in GK.ROWNORM_C:
        x, dy = GK.gen_rownorm(c, 257)
        y, nr = emu_rownorm_fwd(x)
        want_y, want_n = NO.row_normalize_fwd(x)
        k = np.log2(c)
        assert _ratio(y, want_y, np.abs(want_y)) <= k + 6 and _ratio(nr, want_n, want_n) <= k + 6
        worst["rownorm_fwd"] = max(worst["rownorm_fwd"], _ratio(y, want_y, np.abs(want_y)))
        want_dx, mag = NO.row_normalize_bwd(y, dy, nr)
        r = _ratio(emu_rownorm_bwd(y, dy, nr), want_dx, mag)
        assert r <= k + 8
        worst["rownorm_bwd"] = max(worst["rownorm_bwd"], r)
    for lr, mom, wd in GK.SGD_SETTINGS:
        lr32, mom32, wd32 = F32(lr), F32(mom), F32(wd)
        for p, g, buf in GK.gen_sgd((1023, 5000), "emu"):
            for first in (1, 0):
                d = g + wd32 * p
                nb = d if first else mom32 * buf + d
                npp = p - lr32 * nb
                want_p, want_b, b_bound, p_bound = NO.sgd_step(p, g, buf, lr, mom, wd, first)
                assert (np.abs(nb - want_b) <= b_bound).all() and (np.abs(npp - want_p) <= p_bound).all()
                worst["sgd_buf"] = max(worst["sgd_buf"], _ratio(nb, want_b, b_bound / (3 * U)))
                worst["sgd_p"] = max(worst["sgd_p"], _ratio(npp, want_p, (p_bound - NO._f32(lr) * b_bound) / (2 * U)))
    return worst


def test_fp32_emulation_stays_inside_the_bounds():
    worst = fp32_emulation_ratios()
    print({k: round(v, 2) for k, v in worst.items()})
    assert worst["y"] <= 6 and worst["dx"] <= 12 and worst["sum_gx"] <= 3
    assert worst["sgd_buf"] <= 3
    for k, v in worst.items():                             # the figures recorded above are this run's (reproducible inputs)
        assert MEASURED[k] is not None and abs(v - MEASURED[k]) <= 0.1 * max(1.0, MEASURED[k]), (k, v, MEASURED[k])
