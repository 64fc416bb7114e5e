"""Every kernel of csrc/norm.hip, called through the C ABI and compared ELEMENT BY ELEMENT with the fp64 references of
tests/norm_oracle.py.  The conditions promised for the generated inputs, and an fp32 evaluation of the kernels'
expressions against the same bounds, are asserted on the CPU in tests/test_oracle_norm.py.

Branches reached, per entry point
  gcl_bn_stats, gcl_col_sum (k_bn_reduce<false>, reduce_runs)
      widths 4 .. 1024: rstep 256 (more than the 64 rows of a workgroup) .. 1; n 1, 63, 64, 65, 127 (one workgroup, loop
      and tail), 200, 1000; at c 4 and 32 nwg 255 / 256 / 257 and 1023 / 1024 / 1025 (64 rows per workgroup: both sides
      of reduce_runs' four-chain loop) and n = 131075 (128 rows per workgroup, nwg 1025); running statistics given / NULL
  gcl_bn_stats_from_tiles_range (k_bn_stats_direct, reduce_min_max)
      nt 1, 2, 255, 256, 257 at c 5, 32, 256; nt 1023, 1024, 1025, 2049 at c 5, 32; ragged last tile; add_amax x
      max_with x relu; negative weights
  gcl_bn_apply / _ld / _planes (k_bn_apply<true>, <false>)
      hoisted: every power-of-two width 4 .. 1024, and 12 / 96 / 160 at the n where g * 256 is a multiple of c / 4;
      plain: 12 / 96 / 160 at the other n, and c = 96 at n = 87400 (g = 4096, second trip of the plain body);
      total4 = S (c 1024, n 4096), second quads partly valid (n 4100), second trip (n 8193);
      y_ld 0 and c + 32; residual; ReLU with the mask; slot given / NULL; image (c a multiple of 32) with both pitches
  gcl_bn_bwd_reduce / _ld / _range (k_bn_reduce<true>, k_bn_bwd_final)
      widths and n of gcl_bn_stats; gate none / mask words / y; dy_ld 0, c + 4, 2 c; bound slot given (third run of
      partials) / NULL
  gcl_bn_bwd_apply / _ld / _planes (k_bn_bwd_apply<true>, <false>)
      widths and n of the apply pass; gate none / mask / y; dres given / NULL; dy_ld 0, c + 4, 2 c, also with an image;
      sums arbitrary and zero (eval mode)
  gcl_row_normalize_fwd / _bwd   widths 4 .. 256 (lpr 1 .. 64), n 1 .. 1000, rows scaled 1e-3, 1, 1e3; slot given / NULL;
      one all-zero row
  gcl_sgd_multi   float4 body (all pointers 16-byte aligned) and scalar body (p, g or buf off by 4 or 8 bytes), the scalar
      tail (sizes 1, 3, 5, 7, 1023, 131079, 300001), a second and third grid-stride sweep (131072 floats = one sweep
      of quads x 4; 300001), nine tensors and 300 tensors in one launch, first = 1 / 0
  gcl_split_planes   against the CPU construction at c 32 n 1, c 128 n 257, and c 256 as the leading columns of 320

Buffers.  Every output has GUARD elements after it (a slice also its columns past c) that must come back bit for bit;
outputs are pre-filled with NaN (mask words, images: a pattern) so that a word the kernel did not write fails the
comparison.  Scratch has exactly gcl_bn_scratch_len doubles, plus guards.  Every statistics / reduce entry runs twice and
must repeat itself bit for bit.

Bounds, u = 2^-24 (one fp32 rounding, relative), the constant is the count of roundings:
  mean, sum_g, col_sum   2 u |want| + 2^-40 sum|terms|: fp64 accumulation of fp32 terms (n <= 2^18 terms: 2^18 x 2^-53 = 2^-35
                         relative to sum|terms| at the very worst, 2^-40 for sums kept as a tree of short chains) and ONE
                         rounding to fp32 (1 u; 2 u asked)
  rstd, running pair     4 u relative: fp64 throughout, one rounding to fp32 (1 u); running: the fp32 state is an input,
                         one rounding of the result.  Holds while |mean| <= 10 std (ss / n - m^2 cancels 7 bits of 53);
                         beyond that the fp32 tile partials of the convolution epilogue are not designed to serve.
  sum_gx                 3 u sum |g||xhat| + 2 u |want|: xhat = (x - mu) rs has 2 roundings, the product with g is exact
                         in fp64; 1 u for the final rounding
  y                      6 u (|(x - mu) rs w| + |b| + |res|): subtract, two products, add b, add residual = 5 roundings
  dx                     12 u |w rs| (|g| + |sum_g| / n + |xhat| |sum_gx| / n): inv_n (1), w rs (1), sg inv_n (1), x - mu, rs, sx,
                         inv_n (4), two subtractions (2), final product (1) = 10 at most on any one term
  row normalise          forward (log2(c) + 6) u: the sum of squares takes a product (1), 3 adds in the lane and log2(c / 4)
                         butterfly adds = log2(c) + 2 on positive terms, halved by the square root; sqrt (1), divide (1):
                         log2(c) / 2 + 3 on y, one less on norm.  backward (log2(c) + 8) u (|dy| + |y| sum |y||dy|) / norm: the
                         dot product as above (log2(c) + 2), y s (1), subtract (1), divide (1)
  SGD                    buf 3 u (|g| + wd |p| + m |buf|): wd p, + g, m buf + d (the last two count twice on the larger term);
                         p 2 u (|p| + lr |buf'|) + lr x buf's bound
dres, the mask, the amax slots and the plane images are exact (bit for bit), computed from the kernel's own y / dx."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO                                               # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
EPS, MOM = 1e-5, 0.05
GUARD = 96
SENT = {torch.float32: -7777.25, torch.float64: -7777.25, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x7B7B7B7B,
        torch.int16: 0x7B7B}
UNWRITTEN = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int64: 0x3C3C3C3C3C3C3C3C,
             torch.int32: 0x3C3C3C3C, torch.int16: 0x7B7B}
AMAX_WORDS, AMAX_STRIDE = 512, 32

# ---- case tables (tests/test_oracle_norm.py asserts their conditions) ----------------------------------------------------
POW2 = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
ODD = (12, 96, 160)                                        # c / 4 = 3, 24, 40: g * 256 is not always a multiple
N_STATS = (1, 63, 64, 65, 127, 200, 1000)
N_STATS_BIG = (16320, 16384, 16385, 65472, 65536, 65537, 131075)
STATS_CASES = [(c, n) for c in POW2 for n in N_STATS] + [(c, n) for c in (4, 32) for n in N_STATS_BIG]
TILE = 128
TILES_CASES = [(c, nt) for c in (5, 32, 256) for nt in (1, 2, 255, 256, 257)] + \
              [(c, nt) for c in (5, 32) for nt in (1023, 1024, 1025, 2049)]
N_APPLY = (1, 5, 64, 257, 1000)
N_APPLY_EXTRA = {12: (256,), 96: (32,), 160: (32,)}         # hoisted at these; the CPU file asserts both bodies per width
APPLY_LARGE = [(1024, 4096), (1024, 4100), (1024, 8193), (96, 87400)]
APPLY_CASES = [(c, n) for c in POW2 + ODD for n in N_APPLY + N_APPLY_EXTRA.get(c, ())] + APPLY_LARGE
FULL_CROSS_MAX = 1100000                                   # elements up to which a case runs the whole cross of its switches
ROWNORM_C = (4, 8, 16, 32, 64, 128, 256)
ROWNORM_N = (1, 3, 64, 257, 1000)
SGD_SIZES = (1, 3, 4, 5, 7, 1023, 131072, 131079, 300001)
SGD_LAYOUTS = {"aligned": (0, 0, 0), "p+1": (1, 0, 0), "g+1": (0, 1, 0), "buf+2": (0, 0, 2)}
SGD_SETTINGS = ((0.1, 0.8, 1e-4), (0.1, 0.0, 0.0))
APPLY_S = 4096 * 256


def tiles_n(nt):
    return (nt - 1) * TILE + 37                            # ragged last tile


def apply_grid(c, n):
    return min(-(-n * (c // 4) // 256), 4096)


def apply_hoisted(c, n):
    return (apply_grid(c, n) * 256) % (c // 4) == 0


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gen_x(c, n, tag):
    """Channels of standard deviation 2^-2 .. 2^2 and mean within 3 of them."""
    r = rng("x", c, n, tag)
    sd = np.exp2(r.uniform(-2, 2, c))
    mu = r.uniform(-3, 3, c) * sd
    return (r.standard_normal((n, c)) * sd + mu).astype(F32), mu, sd


def gen_w(r, c):
    """Weights of magnitude 0.5 .. 1.5, every third one negative."""
    return (r.uniform(0.5, 1.5, c) * np.where(np.arange(c) % 3 == 1, -1.0, 1.0)).astype(F32)


def gen_given_stats(r, mu, sd):
    """mean and rstd as INPUTS: near the channel's, not equal."""
    return (mu + 0.1 * sd * r.uniform(-1, 1, len(mu))).astype(F32), (r.uniform(0.9, 1.1, len(mu)) / sd).astype(F32)


def gen_apply(c, n):
    x, mu, sd = gen_x(c, n, "apply")
    r = rng("apply", c, n)
    mean, rstd = gen_given_stats(r, mu, sd)
    w = gen_w(r, c)
    b = r.uniform(-0.2, 0.2, c).astype(F32)
    res = (0.5 * r.standard_normal((n, c))).astype(F32)
    return x, mean, rstd, w, b, res


def gen_bwd(c, n):
    x, mu, sd = gen_x(c, n, "bwd")
    r = rng("bwd", c, n)
    mean, rstd = gen_given_stats(r, mu, sd)
    w = gen_w(r, c)
    g = (r.standard_normal((n, c)) * np.exp2(r.uniform(-10, -6, c))).astype(F32)
    bits = r.random((n, c)) < 0.6
    # a y whose signs are those bits; some of the gated-off elements are exactly 0 (y > 0 is false there)
    mag = r.uniform(0.1, 1.0, (n, c))
    y = np.where(bits, mag, np.where(r.random((n, c)) < 0.3, 0.0, -mag)).astype(F32)
    sums = ((r.standard_normal((2, c)) * np.sqrt(n)) * np.abs(g).max(0)).astype(F32)
    return x, mean, rstd, w, g, bits, y, sums


def gen_tiles(c, nt):
    n = tiles_n(nt)
    x, _, _ = gen_x(c, n, "tiles")
    r = rng("tiles", c, nt)
    w = gen_w(r, c)
    b = r.uniform(-0.2, 0.2, c).astype(F32)
    return n, x, w, b


def tile_partials(x, nt):
    """The convolution epilogue's partials, made on the CPU in fp32: [4][c][nt] sum, sum of squares, minimum, maximum per
    128-row tile; padded rows contribute 0 to the sums, +3e38 to the minimum and -3e38 to the maximum."""
    n, c = x.shape
    pad = nt * TILE - n
    xz = np.concatenate([x, np.zeros((pad, c), F32)]).reshape(nt, TILE, c)
    lo = np.concatenate([x, np.full((pad, c), 3.0e38, F32)]).reshape(nt, TILE, c).min(1)
    hi = np.concatenate([x, np.full((pad, c), -3.0e38, F32)]).reshape(nt, TILE, c).max(1)
    part = np.stack([xz.sum(1, dtype=F32), (xz * xz).sum(1, dtype=F32), lo, hi])
    return np.ascontiguousarray(part.transpose(0, 2, 1))


def gen_rownorm(c, n):
    r = rng("rownorm", c, n)
    scale = r.choice([1e-3, 1.0, 1e3], (n, 1))
    x = (r.standard_normal((n, c)) * scale).astype(F32)
    dy = r.standard_normal((n, c)).astype(F32)
    return x, dy


def gen_sgd(sizes, tag):
    r = rng("sgd", tag, len(sizes))
    return [(r.standard_normal(s).astype(F32), (0.01 * r.standard_normal(s)).astype(F32),
             (0.01 * r.standard_normal(s)).astype(F32)) for s in sizes]


# ---- buffers -------------------------------------------------------------------------------------------------------------
class Buf:
    """A device buffer of ``shape`` followed by GUARD sentinel elements; host() checks the guard and returns the body."""

    def __init__(self, shape, dtype=torch.float32, fill=None, init=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.size = int(np.prod(self.shape))
        self.t = torch.empty(self.size + GUARD, dtype=dtype, device=DEV)
        self.t[self.size:] = SENT[dtype]
        if init is not None:
            self.t[:self.size] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(DEV)
        else:
            self.t[:self.size] = UNWRITTEN[dtype] if fill is None else fill

    def host(self):
        h = self.t.cpu()
        assert bool((h[self.size:] == SENT[self.t.dtype]).all()), "a guard element after the buffer changed"
        return h[:self.size].numpy().reshape(self.shape)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from gcl_amd import _lib as L
    return L, L.load()


def _call(entry, *args):
    L, lib = _lib()
    with torch.cuda.device(DEV):
        a = [x.t if isinstance(x, Buf) else x for x in args]
        a = [L.ptr(x) if (x is None or torch.is_tensor(x)) else x for x in a]
        L.check(getattr(lib, entry)(*a, L.stream()), entry)
        torch.cuda.synchronize()


def _slot(value=None):
    """An amax slot: 16 entries (word 32 i), zero or holding ``value`` in one of them; every other word is a sentinel."""
    s = np.full(AMAX_WORDS, SENT[torch.int32], dtype=np.int32)
    s[::AMAX_STRIDE] = 0
    if value is not None:
        s[5 * AMAX_STRIDE] = np.float32(value).view(np.int32)
    return Buf(AMAX_WORDS, torch.int32, init=s), s


def _slot_value(buf, before):
    h = buf.host()
    keep = np.ones(AMAX_WORDS, bool)
    keep[::AMAX_STRIDE] = False
    assert (h[keep] == before[keep]).all(), "a word of the slot that is no entry changed"
    return h[::AMAX_STRIDE].max().view(F32), h


def _scratch(n, c):
    _, lib = _lib()
    return Buf(lib.gcl_bn_scratch_len(n, c), torch.float64)


def _within(got, want, bound, what):
    """|got - want| <= bound element by element; names the worst element."""
    got = np.asarray(got)
    err = np.abs(got.astype(F64) - want)
    assert np.isfinite(got).all(), f"{what}: a value is not finite (not written?)"
    ratio = err / np.maximum(bound, 1e-300)
    i = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    print(f"  {what}: worst |err| / bound {ratio.max():.3f} at {i}")
    assert (err <= bound).all(), (what, i, float(got[i]), float(np.asarray(want)[i]), float(err[i]), float(np.asarray(bound)[i]))


def _same(a, b, what):
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"{what}: not bit for bit"


# ---- A. gcl_bn_stats, gcl_col_sum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", STATS_CASES)
def test_bn_stats_and_col_sum(c, n):
    x, _, _ = gen_x(c, n, "stats")
    r = rng("running", c, n)
    rm0, rv0 = r.standard_normal(c).astype(F32), r.uniform(0.5, 1.5, c).astype(F32)
    want_mean, want_rstd, want_rm, want_rv = NO.bn_stats(x, EPS, MOM, rm0, rv0)
    if n == 1:                                             # the variance is 0: the running one moves toward 0 by the momentum
        assert np.allclose(want_rv, (1 - NO._f32(MOM)) * rv0.astype(F64), rtol=1e-15)
    sum_abs = np.abs(x.astype(F64)).sum(0)
    xd = _dev(x)
    runs = []
    for running in (True, False, True):                    # the first and the last: the same call twice
        mean, rstd, sc = Buf(c), Buf(c), _scratch(n, c)
        rm, rv = (Buf(c, init=rm0), Buf(c, init=rv0)) if running else (None, None)
        _call("gcl_bn_stats", xd, n, c, EPS, MOM, rm, rv, sc, mean, rstd)
        sc.host()
        runs.append((mean.host(), rstd.host(), rm.host() if running else None, rv.host() if running else None))
    for k in range(4):
        _same(runs[0][k], runs[2][k], "gcl_bn_stats twice")
    _same(runs[0][0], runs[1][0], "mean without running statistics")
    _same(runs[0][1], runs[1][1], "rstd without running statistics")
    mean, rstd, rm, rv = runs[0]
    _within(mean, want_mean, 2 * U * np.abs(want_mean) + 2.0 ** -40 * sum_abs / n, "mean")
    _within(rstd, want_rstd, 4 * U * want_rstd, "rstd")
    _within(rm, want_rm, 4 * U * np.abs(want_rm), "running_mean")
    _within(rv, want_rv, 4 * U * want_rv, "running_var")
    sums = []
    for _ in range(2):
        out, sc = Buf(c), _scratch(n, c)
        _call("gcl_col_sum", xd, n, c, sc, out)
        sc.host()
        sums.append(out.host())
    _same(sums[0], sums[1], "gcl_col_sum twice")
    want = NO.col_sum(x)
    _within(sums[0], want, 2 * U * np.abs(want) + 2.0 ** -40 * sum_abs, "col_sum")


# ---- B. gcl_bn_stats_from_tiles_range ----------------------------------------------------------------------------------------
def _apply_max(x, mean, rstd, w, b, relu):
    """max|y| of gcl_bn_apply without residual, from its slot.  A width that is no multiple of 4 is padded with channels
    that give y = 0 (x = mean = w = b = 0): the maximum over the real channels."""
    n, c = x.shape
    cp = -(-c // 4) * 4
    pad = lambda v, fill=0.0: np.concatenate([v, np.full(cp - c, fill, F32)])
    xp = np.concatenate([x, np.zeros((n, cp - c), F32)], axis=1)
    y, (slot, s0) = Buf((n, cp)), _slot()
    _call("gcl_bn_apply", _dev(xp), n, cp, _dev(pad(mean)), _dev(pad(rstd, 1.0)), _dev(pad(w)), _dev(pad(b)), None, int(relu),
          y, Buf(NO.mask_len(n, cp), torch.int64) if relu else None, slot)
    v, _ = _slot_value(slot, s0)
    assert v == np.abs(y.host()).max()
    return v


@pytest.mark.parametrize("c,nt", TILES_CASES)
def test_bn_stats_from_tiles_range(c, nt):
    n, x, w, b = gen_tiles(c, nt)
    part = tile_partials(x, nt)
    r = rng("running", c, nt)
    rm0, rv0 = r.standard_normal(c).astype(F32), r.uniform(0.5, 1.5, c).astype(F32)
    want_mean, want_rstd, want_rm, want_rv, want_range = NO.bn_stats_from_partials(part, n, EPS, MOM, rm0, rv0)
    _same(want_range, np.stack([x.min(0), x.max(0)]), "the oracle's range is the tensor's")
    sum_abs = np.abs(part[0].astype(F64)).sum(1)
    res_amax, partner = F32(1.375), {0: None, 1: None}
    pd, wd, bd = _dev(part), _dev(w), _dev(b)
    first = None
    for relu in (0, 1):
        for add in (False, True):
            for mx in (False, True):
                mean, rstd, xr = Buf(c), Buf(c), Buf((2, c))
                rm, rv = Buf(c, init=rm0), Buf(c, init=rv0)
                slot, s0 = _slot()
                a_slot, a0 = _slot(res_amax)
                _call("gcl_bn_stats_from_tiles_range", pd, nt, n, c, EPS, MOM, rm, rv, mean, rstd, xr, wd, bd, relu,
                      a_slot if add else None, None, slot)
                got = (mean.host(), rstd.host(), rm.host(), rv.host(), xr.host())
                _same(a_slot.host(), a0, "the residual's slot is read only")
                if first is None:
                    first = got
                    _within(got[0], want_mean, 2 * U * np.abs(want_mean) + 2.0 ** -40 * sum_abs / n, "mean")
                    _within(got[1], want_rstd, 4 * U * want_rstd, "rstd")
                    _within(got[2], want_rm, 4 * U * np.abs(want_rm), "running_mean")
                    _within(got[3], want_rv, 4 * U * want_rv, "running_var")
                    _same(got[4], want_range, "xrange")
                for k in range(5):
                    _same(got[k], first[k], "statistics do not depend on the bound's switches (and repeat)")
                if partner[relu] is None:                  # max|y| of the apply pass on the statistics the kernel published
                    partner[relu] = _apply_max(x, got[0], got[1], w, b, relu)
                y_max = partner[relu]
                bound, _ = _slot_value(slot, s0)
                want = F32(y_max + res_amax) if add else y_max
                # the partner's slot value: once above, once below this tensor's bound
                if mx:
                    for other in (F32(want * F32(1.5)), F32(want * F32(0.5))):
                        slot, s0 = _slot()
                        m_slot, m0 = _slot(other)
                        a_slot, _ = _slot(res_amax)
                        _call("gcl_bn_stats_from_tiles_range", pd, nt, n, c, EPS, MOM, None, None, Buf(c), Buf(c), None, wd, bd,
                              relu, a_slot if add else None, m_slot, slot)
                        _same(m_slot.host(), m0, "the partner's slot is read only")
                        bound, _ = _slot_value(slot, s0)
                        assert bound == max(want, other), (relu, add, float(bound), float(want), float(other))
                else:
                    assert bound == want, (relu, add, float(bound), float(want))
    # without a slot nothing of the bound is computed: xrange stays as it was
    xr = Buf((2, c))
    _call("gcl_bn_stats_from_tiles_range", pd, nt, n, c, EPS, MOM, None, None, Buf(c), Buf(c), xr, None, None, 0, None, None, None)
    assert np.isnan(xr.host()).all()


# ---- C. gcl_bn_apply / _ld / _planes -----------------------------------------------------------------------------------------
def _cross(n, c, full, few):
    return full if n * c <= FULL_CROSS_MAX else few


def _img_host(img, n, ld):
    return img.host().view(np.uint16).reshape(n, ld // 32, 2, 32)


@pytest.mark.parametrize("c,n", APPLY_CASES)
def test_bn_apply(c, n):
    """Above FULL_CROSS_MAX elements (the four large cases) four combinations that together use every switch both ways."""
    x, mean, rstd, w, b, res = gen_apply(c, n)
    can_img = c % 32 == 0
    full = [(rs, relu, ld, slot, img) for rs in (0, 1) for relu in (0, 1) for ld in (0, c + 32) for slot in (0, 1)
            for img in ((0, 1) if can_img else (0,)) if slot or not img]
    few = [(1, 1, 0, 1, 0), (0, 0, c + 32, 0, 0), (1, 1, c + 32, 1, int(can_img)), (0, 1, 0, 1, int(can_img))]
    d = {k: _dev(v) for k, v in dict(x=x, mean=mean, rstd=rstd, w=w, b=b, res=res).items()}
    wants, first = {}, {}
    for use_res, relu, ld, use_slot, use_img in _cross(n, c, full, few):
        if (use_res, relu) not in wants:
            wants[use_res, relu] = NO.bn_apply(x, mean, rstd, w, b, res if use_res else None, relu)
        want, mag = wants[use_res, relu]
        width = ld or c
        y = Buf((n, width), fill=SENT[torch.float32]) if ld else Buf((n, c))
        mask = Buf(NO.mask_len(n, c), torch.int64) if relu else None
        slot, s0 = _slot(F32(np.abs(want).max() * 1.25) if use_img else None) if use_slot else (None, None)
        img = Buf((n, width * 2), torch.int16) if use_img else None
        args = (d["x"], n, c, d["mean"], d["rstd"], d["w"], d["b"], d["res"] if use_res else None, relu, y)
        if use_img:
            _call("gcl_bn_apply_planes", *args, ld, mask, slot, img)
        elif ld:
            _call("gcl_bn_apply_ld", *args, ld, mask, slot)
        else:
            _call("gcl_bn_apply", *args, mask, slot)
        yh = y.host()
        if ld:
            assert (yh[:, c:] == SENT[torch.float32]).all(), "a column past c of the slice changed"
            yh = np.ascontiguousarray(yh[:, :c])
        what = f"y res={use_res} relu={relu} ld={ld} slot={use_slot} image={use_img}"
        if (use_res, relu) not in first:
            first[use_res, relu] = yh
            _within(yh, want, 6 * U * mag, what)
        else:
            _same(yh, first[use_res, relu], what + " against the first variant")
        if relu:
            _same(mask.host().view(np.uint64), NO.pack_mask(yh > 0, n, c), "mask")
        if use_slot:
            v, sh = _slot_value(slot, s0)
            if use_img:
                _same(sh, s0, "the slot of an image is read only")
                _same(_img_host(img, n, width), NO.planes_image(yh, v, width, fill=SENT[torch.int16]), "plane image")
            else:
                assert v == np.abs(yh).max(), (what, float(v), float(np.abs(yh).max()))


# ---- D. gcl_bn_bwd_reduce / _ld / _range ---------------------------------------------------------------------------------------
def _in_slice(g, ld):
    """g as the leading columns of an [n, ld] tensor whose other columns hold 1e30."""
    if not ld:
        return g
    out = np.full((g.shape[0], ld), 1e30, F32)
    out[:, :g.shape[1]] = g
    return out


@pytest.mark.parametrize("c,n", STATS_CASES)
def test_bn_bwd_reduce(c, n):
    x, mean, rstd, w, g, bits, y, _ = gen_bwd(c, n)
    xrange = np.stack([x.min(0), x.max(0)])
    d = {k: _dev(v) for k, v in dict(x=x, mean=mean, rstd=rstd, w=w, y=y, xrange=xrange).items()}
    d["mask"] = _dev(NO.pack_mask(bits, n, c).view(np.int64))
    gd = {ld: _dev(_in_slice(g, ld)) for ld in (0, c + 4, 2 * c)}

    def run(ld, gate, use_slot):
        sg, sx, sc = Buf(c), Buf(c), _scratch(n, c)
        slot, s0 = _slot() if use_slot else (None, None)
        yv, mv, relu = (d["y"] if gate == "y" else None), (d["mask"] if gate == "mask" else None), int(gate != "none")
        tail = (n, c, d["mean"], d["rstd"], relu, sc, sg, sx)
        if use_slot:
            _call("gcl_bn_bwd_reduce_range", d["x"], gd[ld], ld, yv, mv, *tail, d["xrange"], d["w"], slot)
        elif ld:
            _call("gcl_bn_bwd_reduce_ld", d["x"], gd[ld], ld, yv, mv, *tail)
        else:
            _call("gcl_bn_bwd_reduce", d["x"], gd[ld], yv, mv, *tail)
        sc.host()
        return sg.host(), sx.host(), (_slot_value(slot, s0)[0] if use_slot else None)

    for gates in (("none",), ("mask", "y")):
        base = run(0, gates[0], True)
        variants = [(0, gates[0], True)] + [(ld, gt, (i + j) % 2 == 0) for i, gt in enumerate(gates)
                                            for j, ld in enumerate((0, c + 4, 2 * c))]
        for ld, gt, use_slot in variants:
            got = run(ld, gt, use_slot)
            what = f"gate={gt} dy_ld={ld} slot={use_slot} against gate={gates[0]} dy_ld=0 with a slot"
            _same(got[0], base[0], "sum_g " + what)
            _same(got[1], base[1], "sum_gx " + what)
            if use_slot:
                assert got[2] == base[2], "dx bound " + what
        gate = None if gates[0] == "none" else bits
        want_g, want_gx, abs_gx = NO.bn_bwd_sums(x, g, gate, mean, rstd)
        sum_abs = np.abs(NO._gated(g, gate)).sum(0)
        _within(base[0], want_g, 2 * U * np.abs(want_g) + 2.0 ** -40 * sum_abs, f"sum_g gate={gates[0]}")
        _within(base[1], want_gx, 3 * U * abs_gx + 2 * U * np.abs(want_gx), f"sum_gx gate={gates[0]}")
        # the bound of max|dx| against the apply pass on the sums the kernel published
        dx = Buf((n, c))
        _call("gcl_bn_bwd_apply", d["x"], gd[0], None, d["mask"] if gate is not None else None, n, c, d["mean"], d["rstd"],
              d["w"], _dev(base[0]), _dev(base[1]), int(gate is not None), dx, None, None)
        dmax = np.abs(dx.host()).max()
        assert base[2] >= dmax, (gates[0], float(base[2]), float(dmax))
        if n >= 129:
            assert base[2] <= 4 * dmax, (gates[0], float(base[2]), float(dmax))


# ---- E. gcl_bn_bwd_apply / _ld / _planes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", APPLY_CASES)
def test_bn_bwd_apply(c, n):
    """Above FULL_CROSS_MAX elements (the four large cases) six combinations that together use every switch every way."""
    x, mean, rstd, w, g, bits, y, sums = gen_bwd(c, n)
    can_img = c % 32 == 0
    lds = (0, c + 4, 2 * c)
    full = [(gate, dres, ld, zero, img) for gate in ("none", "mask", "y") for dres in (1, 0) for ld in lds
            for zero in (0, 1) for img in ((0, 1) if can_img else (0,))]
    few = [("none", 1, 0, 0, 0), ("mask", 1, c + 4, 0, int(can_img)), ("y", 0, 2 * c, 1, 0), ("mask", 0, 0, 1, int(can_img)),
           ("y", 1, c + 4, 0, 0), ("none", 0, 2 * c, 0, int(can_img))]
    d = {k: _dev(v) for k, v in dict(x=x, mean=mean, rstd=rstd, w=w, y=y).items()}
    d["mask"] = _dev(NO.pack_mask(bits, n, c).view(np.int64))
    gd = {ld: _dev(_in_slice(g, ld)) for ld in lds}
    sd = {0: _dev(sums), 1: _dev(np.zeros_like(sums))}
    wants, first = {}, {}
    for gate, use_dres, ld, zero, use_img in _cross(n, c, full, few):
        relu = int(gate != "none")
        if (relu, zero) not in wants:
            s = sums * (1 - zero)
            wants[relu, zero] = NO.bn_bwd_apply(x, g, bits if relu else None, mean, rstd, w, s[0], s[1], n)
        want_dx, want_dres, mag = wants[relu, zero]
        dx, dres = Buf((n, c)), (Buf((n, c)) if use_dres else None)
        slot, s0 = _slot(F32(np.abs(want_dx).max() * 1.25) if use_img else None)
        img = Buf((n, c * 2), torch.int16) if use_img else None
        yv, mv = (d["y"] if gate == "y" else None), (d["mask"] if gate == "mask" else None)
        tail = (n, c, d["mean"], d["rstd"], d["w"], sd[zero][0], sd[zero][1], relu, dx, dres, slot)
        if use_img:
            _call("gcl_bn_bwd_apply_planes", d["x"], gd[ld], ld, yv, mv, *tail, img)
        elif ld:
            _call("gcl_bn_bwd_apply_ld", d["x"], gd[ld], ld, yv, mv, *tail)
        else:
            _call("gcl_bn_bwd_apply", d["x"], gd[ld], yv, mv, *tail)
        dxh = dx.host()
        what = f"dx gate={gate} dres={use_dres} dy_ld={ld} zero sums={zero} image={use_img}"
        if (relu, zero) not in first:
            first[relu, zero] = dxh
            _within(dxh, want_dx, 12 * U * mag, what)
        else:
            _same(dxh, first[relu, zero], what + " against the first variant")
        if use_dres:
            _same(dres.host(), want_dres.astype(F32), "dres is the gated g")
        v, sh = _slot_value(slot, s0)
        if use_img:
            _same(sh, s0, "the slot of an image is read only")
            _same(_img_host(img, n, c), NO.planes_image(dxh, v), "plane image")
        else:
            assert v == np.abs(dxh).max(), (what, float(v), float(np.abs(dxh).max()))
    # no slot at all
    dx = Buf((n, c))
    _call("gcl_bn_bwd_apply", d["x"], gd[0], None, None, n, c, d["mean"], d["rstd"], d["w"], sd[0][0], sd[0][1], 0, dx, None, None)
    _same(dx.host(), first[0, 0], "dx without a slot")


# ---- gcl_split_planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,ld", [(32, 1, 0), (128, 257, 0), (256, 129, 320)])
def test_split_planes_is_the_documented_construction(c, n, ld):
    """ld = 320: the 256 leading columns of a 320-wide tensor whose other columns are 0 -- what the in-place image of a
    column slice is compared with in test_batch_norm_plane_images_from_the_producer."""
    r = rng("planes", c, n)
    x = (r.standard_normal((n, c)) * np.exp2(r.uniform(-12, 3, (n, 1)))).astype(F32)      # rows far below the maximum too
    x[0, 0] = 0.0
    width = ld or c
    full = np.zeros((n, width), F32)
    full[:, :c] = x
    for value in (np.abs(x).max(), F32(np.abs(x).max() * 3.0)):
        slot, s0 = _slot(value)
        img = Buf((n, width * 2), torch.int16, fill=0x3C3C)
        _call("gcl_split_planes", _dev(full), n, width, slot, img)
        _same(slot.host(), s0, "slot")
        _same(_img_host(img, n, width), NO.planes_image(x, value, width, fill=0), "plane image")


# ---- F. row-wise L2 normalisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWNORM_N)
@pytest.mark.parametrize("c", ROWNORM_C)
def test_row_normalize(c, n):
    x, dy = gen_rownorm(c, n)
    y, norm = Buf((n, c)), Buf(n)
    _call("gcl_row_normalize_fwd", _dev(x), n, c, y, norm)
    yh, nh = y.host(), norm.host()
    want_y, want_norm = NO.row_normalize_fwd(x)
    k = np.log2(c)
    _within(yh, want_y, (k + 6) * U * np.abs(want_y), "y")
    _within(nh, want_norm, (k + 6) * U * want_norm, "norm")
    want_dx, mag = NO.row_normalize_bwd(yh, dy, nh)       # the kernel's own y and norm are the backward's inputs
    outs = []
    for use_slot in (True, False):
        dx = Buf((n, c))
        slot, s0 = _slot() if use_slot else (None, None)
        _call("gcl_row_normalize_bwd", _dev(yh), _dev(dy), _dev(nh), n, c, dx, slot)
        outs.append(dx.host())
        if use_slot:
            assert _slot_value(slot, s0)[0] == np.abs(outs[0]).max()
    _same(outs[0], outs[1], "dx with and without a slot")
    _within(outs[0], want_dx, (k + 8) * U * mag, "dx")


def test_row_normalize_zero_row_is_nan_in_that_row_only():
    c, n, z = 32, 65, 17
    x, _ = gen_rownorm(c, n)
    x[z] = 0.0
    y, norm = Buf((n, c)), Buf(n)
    _call("gcl_row_normalize_fwd", _dev(x), n, c, y, norm)
    t = y.t.cpu()
    assert bool((t[y.size:] == SENT[torch.float32]).all())
    yh, nh = t[:y.size].numpy().reshape(n, c), norm.host()
    assert np.isnan(yh[z]).all() and nh[z] == 0.0
    others = np.arange(n) != z
    want_y, want_norm = NO.row_normalize_fwd(x[others])
    _within(yh[others], want_y, (np.log2(c) + 6) * U * np.abs(want_y), "y of the other rows")
    _within(nh[others], want_norm, (np.log2(c) + 6) * U * want_norm, "norm of the other rows")


# ---- G. gcl_sgd_multi -------------------------------------------------------------------------------------------------------------------
def _sgd_layout(sizes, shifts):
    """Offsets (in floats) of p, g, buf of every tensor in one flat buffer: each region starts at a multiple of 4 floats plus
    its role's shift and is followed by at least GUARD floats that belong to nobody."""
    offs, cur = [], 0
    for i, s in enumerate(sizes):
        row = []
        for role in range(3):
            sh = shifts[i % len(shifts)][role] if isinstance(shifts, list) else shifts[role]
            start = -(-cur // 4) * 4 + sh
            row.append(start)
            cur = start + s + GUARD
        offs.append(row)
    return offs, -(-cur // 4) * 4


def _sgd_run(data, sizes, shifts, lr, mom, wd):
    """first = 1 on NaN momentum buffers, then first = 0 with a second gradient.  -> per step the lists of p and buf."""
    offs, total = _sgd_layout(sizes, shifts)
    flat = np.full(total, SENT[torch.float32], F32)
    for (p, g, _), (op, og, ob), s in zip(data, offs, sizes):
        flat[op:op + s], flat[og:og + s], flat[ob:ob + s] = p, g, np.nan
    owned = np.zeros(total, bool)
    for (op, _, ob), s in zip(offs, sizes):
        owned[op:op + s] = owned[ob:ob + s] = True
    t = torch.from_numpy(flat).to(DEV)
    assert t.data_ptr() % 16 == 0
    table = torch.tensor([[t.data_ptr() + 4 * o for o in row] for row in offs], dtype=torch.int64, device=DEV)
    sz = torch.tensor(list(sizes), dtype=torch.int64, device=DEV)
    steps = []
    for first in (1, 0):
        if not first:                                      # a second gradient: the first one's third buffer column
            for (_, _, g2), (_, og, _), s in zip(data, offs, sizes):
                flat[og:og + s] = g2
                t[og:og + s] = torch.from_numpy(g2).to(DEV)
        _call("gcl_sgd_multi", table, sz, len(sizes), lr, mom, wd, first)
        h = t.cpu().numpy()
        assert h[~owned].tobytes() == flat[~owned].tobytes(), "a float outside every p and buf changed (guards, gradients)"
        steps.append(([h[op:op + s].copy() for (op, _, _), s in zip(offs, sizes)],
                      [h[ob:ob + s].copy() for (_, _, ob), s in zip(offs, sizes)]))
        flat = h.copy()
    return steps


def _sgd_check(data, steps, lr, mom, wd, what):
    ps, bufs = [d[0] for d in data], [None] * len(data)
    for step, first in enumerate((1, 0)):
        for i, d in enumerate(data):
            g = d[1] if first else d[2]
            want_p, want_b, b_bound, p_bound = NO.sgd_step(ps[i], g, bufs[i], lr, mom, wd, first)
            got_p, got_b = steps[step][0][i], steps[step][1][i]
            assert np.isfinite(got_b).all() and np.isfinite(got_p).all(), f"{what}: tensor {i} step {step} not finite"
            eb, ep = np.abs(got_b.astype(F64) - want_b), np.abs(got_p.astype(F64) - want_p)
            assert (eb <= b_bound).all(), (what, "buf", i, step, int((eb - b_bound).argmax()))
            assert (ep <= p_bound).all(), (what, "p", i, step, int((ep - p_bound).argmax()))
            ps[i], bufs[i] = got_p, got_b                  # the next step starts from the kernel's own state


@pytest.mark.parametrize("lr,mom,wd", SGD_SETTINGS)
def test_sgd_multi_layouts(lr, mom, wd):
    data = gen_sgd(SGD_SIZES, "nine")
    runs = {name: _sgd_run(data, SGD_SIZES, sh, lr, mom, wd) for name, sh in SGD_LAYOUTS.items()}
    _sgd_check(data, runs["aligned"], lr, mom, wd, "aligned")
    for name in SGD_LAYOUTS:
        for step in range(2):
            for which, role in enumerate(("p", "buf")):
                for i, s in enumerate(SGD_SIZES):
                    assert runs[name][step][which][i].tobytes() == runs["aligned"][step][which][i].tobytes(), \
                        f"layout {name}: {role} of the tensor of {s} elements differs from the aligned layout at step {step}"


def test_sgd_multi_300_small_tensors():
    sizes = [i % 9 + 1 for i in range(300)]
    data = gen_sgd(sizes, "many")
    lr, mom, wd = SGD_SETTINGS[0]
    steps = _sgd_run(data, sizes, list(SGD_LAYOUTS.values()), lr, mom, wd)
    _sgd_check(data, steps, lr, mom, wd, "300 tensors")
