"""fp64 references of the operations of csrc/norm.hip (numpy, CPU only), one plain function per operation, arguments in
the order of the C entry points.  tests/test_oracle_norm.py pins them against torch's autograd; the GPU tests of
tests/test_gpu_norm_kernels.py compare every kernel with them element by element.

Mean and rstd are INPUTS of the apply and backward references, as they are of the entry points: each kernel is judged
on its own arithmetic, not on its predecessor's rounding.  ``eps`` and ``momentum`` cross the C ABI as fp32, so the
references take them at their fp32 values."""
import numpy as np

F64 = np.float64
U = 2.0 ** -24                                             # unit roundoff of fp32


def _d(a):
    return None if a is None else np.asarray(a, dtype=F64)


def _f32(v):
    return float(np.float32(v))


# ---- statistics ---------------------------------------------------------------------------------------------------------
def _finish_stats(mean, var, n, eps, momentum, running_mean, running_var):
    rstd = 1.0 / np.sqrt(var + _f32(eps))
    if running_mean is None:
        return mean, rstd, None, None
    m = _f32(momentum)
    unb = var * (n / (n - 1.0)) if n > 1 else var          # torch refuses n = 1; the kernels keep the biased value (0)
    return mean, rstd, (1.0 - m) * _d(running_mean) + m * mean, (1.0 - m) * _d(running_var) + m * unb


def bn_stats(x, eps, momentum, running_mean=None, running_var=None):
    """-> mean, rstd, new running_mean, new running_var (None, None without running statistics).  Two-pass variance."""
    x = _d(x)
    n = x.shape[0]
    mean = x.sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    return _finish_stats(mean, var, n, eps, momentum, running_mean, running_var)


def bn_stats_from_partials(partial, n, eps, momentum, running_mean=None, running_var=None):
    """partial: fp32 [4][c][nt] -- per tile and channel the sum, the sum of squares, the minimum and the maximum of x.
    Sums exactly what the kernel reads (so E[x^2] - mean^2, in fp64).  -> mean, rstd, running pair, xrange [2][c]."""
    p = _d(partial)
    mean = p[0].sum(1) / n
    var = np.maximum(p[1].sum(1) / n - mean * mean, 0.0)
    xrange = np.stack([np.asarray(partial)[2].min(1), np.asarray(partial)[3].max(1)])
    return _finish_stats(mean, var, n, eps, momentum, running_mean, running_var) + (xrange,)


def col_sum(x):
    return _d(x).sum(0)


# ---- apply --------------------------------------------------------------------------------------------------------------
def bn_apply(x, mean, rstd, w, b, residual=None, relu=False):
    """-> y, magnitude |(x - mu) rs w| + |b| + |res| (what the roundings of the fp32 expression are relative to)."""
    t = (_d(x) - _d(mean)) * _d(rstd) * _d(w)
    y, mag = t + _d(b), np.abs(t) + np.abs(_d(b))
    if residual is not None:
        y, mag = y + _d(residual), mag + np.abs(_d(residual))
    return (np.maximum(y, 0.0) if relu else y), mag


# ---- backward -----------------------------------------------------------------------------------------------------------
def _gated(g, gate):
    return _d(g) if gate is None else np.where(np.asarray(gate, dtype=bool), _d(g), 0.0)


def bn_bwd_sums(x, g, gate, mean, rstd):
    """gate: boolean [n, c] (the ReLU's y > 0) or None.  -> sum_g, sum_gx, sum |g| |xhat|."""
    g = _gated(g, gate)
    xhat = (_d(x) - _d(mean)) * _d(rstd)
    return g.sum(0), (g * xhat).sum(0), (np.abs(g) * np.abs(xhat)).sum(0)


def bn_bwd_apply(x, g, gate, mean, rstd, w, sum_g, sum_gx, n):
    """-> dx, dres (the gated g), magnitude |w rs| (|g| + |sum_g| / n + |xhat| |sum_gx| / n)."""
    g = _gated(g, gate)
    xhat = (_d(x) - _d(mean)) * _d(rstd)
    wrs, sg, sx = _d(w) * _d(rstd), _d(sum_g), _d(sum_gx)
    dx = wrs * (g - sg / n - xhat * sx / n)
    mag = np.abs(wrs) * (np.abs(g) + np.abs(sg) / n + np.abs(xhat) * np.abs(sx) / n)
    return dx, g, mag


# ---- ReLU sign bits -----------------------------------------------------------------------------------------------------
def mask_len(n, c):
    return (n * (c // 4) + 63) // 64 * 4


def pack_mask(y_positive, n, c):
    """boolean [n, c] -> uint64 [mask_len]: element quad e (four consecutive channels of the flat tensor) -> bit e & 63 of
    the words (e >> 6) * 4 + component.  Bits past the last quad are 0."""
    q = np.asarray(y_positive, dtype=bool).reshape(n * (c // 4), 4)
    groups = mask_len(n, c) // 4
    padded = np.zeros((groups * 64, 4), dtype=np.uint64)
    padded[:q.shape[0]] = q
    bit = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(groups, 64, 4) * bit[None, :, None]).sum(1, dtype=np.uint64).reshape(-1)      # distinct bits: sum = or


def unpack_mask(words, n, c):
    e = np.arange(n * (c // 4), dtype=np.int64)
    w = np.asarray(words, dtype=np.uint64)
    out = np.empty((len(e), 4), dtype=bool)
    for comp in range(4):
        out[:, comp] = ((w[(e >> 6) * 4 + comp] >> (e & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    return out.reshape(n, c)


# ---- row-wise L2 normalisation -------------------------------------------------------------------------------------------
def row_normalize_fwd(x):
    """-> y = x / ||x||, norm.  No epsilon: an all-zero row gives NaN, as in the kernel and the model it follows."""
    x = _d(x)
    norm = np.sqrt((x * x).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / norm[:, None], norm


def row_normalize_bwd(y, dy, norm):
    """-> dx = (dy - y (y . dy)) / norm, magnitude (|dy| + |y| sum |y| |dy|) / norm."""
    y, dy, norm = _d(y), _d(dy), _d(norm)[:, None]
    dx = (dy - y * (y * dy).sum(1, keepdims=True)) / norm
    mag = (np.abs(dy) + np.abs(y) * (np.abs(y) * np.abs(dy)).sum(1, keepdims=True)) / norm
    return dx, mag


# ---- SGD ----------------------------------------------------------------------------------------------------------------
def sgd_step(p, g, buf, lr, momentum, wd, first):
    """torch.optim.SGD's update (dampening 0, no Nesterov).  ``buf`` is not read when ``first``.
    -> new p, new buf, bound of buf's fp32 error (3 roundings), bound of p's (2 roundings + lr x buf's)."""
    p, g = _d(p), _d(g)
    lr, momentum, wd = _f32(lr), _f32(momentum), _f32(wd)
    d = g + wd * p
    if first:
        nb, bmag = d, np.abs(g) + wd * np.abs(p)
    else:
        nb, bmag = momentum * _d(buf) + d, np.abs(g) + wd * np.abs(p) + momentum * np.abs(_d(buf))
    np_ = p - lr * nb
    bbound = 3 * U * bmag
    return np_, nb, bbound, 2 * U * (np.abs(p) + lr * np.abs(nb)) + lr * bbound


# ---- amax slots and fp16 plane images (csrc/common.h) ----------------------------------------------------------------------
def amax_scale(amax):
    """The power-of-two scale that maps amax into [2^13, 2^14); 1 for 0, negative, NaN and >= 3e38."""
    amax = np.float32(amax)
    if not (amax > 0) or not (amax < np.float32(3.0e38)):
        return np.float32(1.0)
    _, e = np.frexp(amax)
    return np.float32(np.ldexp(1.0, int(np.clip(14 - e, -100, 100))))


def split_f16(sv):
    """fp32 -> hi = fp16(sv), lo = fp16((sv - hi) 2^11); the difference and its scaling are exact in fp32."""
    sv = np.asarray(sv, dtype=np.float32)
    hi = sv.astype(np.float16)
    lo = ((sv - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def planes_image(y_fp32, slot_value, ld=0, fill=0):
    """The fp16 hi / lo image of fp32 [n, c] (c a multiple of 32) at row pitch ``ld`` channels (0 = c), as uint16
    [n, ld / 32, 2, 32]: 16-bit unit row * ld * 2 + slice * 64 + plane * 32 + ch % 32.  Slices past c hold ``fill``."""
    y = np.asarray(y_fp32, dtype=np.float32)
    n, c = y.shape
    ld = ld or c
    assert c % 32 == 0 and ld % 32 == 0 and ld >= c
    hi, lo = split_f16(y * amax_scale(slot_value))
    img = np.full((n, ld // 32, 2, 32), fill, dtype=np.uint16)
    img[:, :c // 32, 0, :] = hi.view(np.uint16).reshape(n, c // 32, 32)
    img[:, :c // 32, 1, :] = lo.view(np.uint16).reshape(n, c // 32, 32)
    return img
