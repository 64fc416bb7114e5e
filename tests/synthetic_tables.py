"""Synthetic neighbour tables, the two data sets and the two kinds of check shared by tests/test_gpu_stem_kernels.py and
tests/test_gpu_generic_conv.py.  Plain numpy; nothing here needs a GPU.

A table is nbr[K][n_out] int32: entry -1 (absent) with probability 0.6, else a row of x, uniform in [0, n_in).  Forced
into every table, as far as K and n_out leave room:

    * the last offset K - 1 is present in every row that has neighbours at all (so an off-by-one at a K border drops
      terms of every row and of a whole dW[k]);
    * one offset is absent in every row (K >= 2);
    * some output rows have no neighbour at all (n_out >= 4; they take precedence over the all-present offset, the two
      demands exclude each other on those rows);
    * the first and the last output row are populated.

The convolution over such a table is one GEMM over the gathered matrix A[v][k * Cin + c] = x[nbr[k][v]][c] (0 where
absent): y = A W, dW = A^T dY, and sum |terms| = |A| |W|.  With small-integer data the fp64 GEMM is exact (every partial
sum is an integer far below 2^53), so its result cast to int64 IS the int64 result; the tests assert the kernels' premise
(sum |products| < 2^24: every fp32 product and partial sum exact in any order) on it.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
P_ABSENT = 0.6
OCC_RUN = 37            # occupancy mix "runs": the flag alternates in runs of 37 rows


def make_table(K, n_out, n_in, seed, flags=None):
    """(nbr, info).  flags: per-row occupancy flags (n_in == n_out); a row's neighbours are then drawn among the rows of its
    own flag, as the rows of one cloud are (the occupancy kernels assume every row an unflagged row gathers is 1.0)."""
    rng = np.random.RandomState(seed)
    if flags is None:
        full = rng.randint(0, n_in, (K, n_out))
        full[K - 1, 0], full[K - 1, n_out - 1] = n_in - 1, 0          # entries over the whole of x
    else:
        assert n_in == n_out
        full = np.empty((K, n_out), np.int64)
        for f in (0, 1):
            cols = np.nonzero(flags == f)[0]
            if len(cols):
                full[:, cols] = cols[rng.randint(0, len(cols), (K, len(cols)))]
    nbr = np.where(rng.rand(K, n_out) < P_ABSENT, -1, full)
    nbr[K - 1] = full[K - 1]
    k_absent = (K - 1) // 2 if K >= 2 else None
    if k_absent is not None:
        nbr[k_absent] = -1
    empty = np.zeros(0, np.int64)
    if n_out >= 4:
        empty = np.unique(np.concatenate([[1], rng.randint(1, n_out - 1, max(1, n_out // 16))]))
        nbr[:, empty] = -1
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    # what was forced is there
    present = nbr >= 0
    assert present[:, 0].any() and present[:, n_out - 1].any()
    assert k_absent is None or not present[k_absent].any()
    assert present[K - 1].sum() == n_out - len(empty) and (len(empty) > 0) == (n_out >= 4)
    assert not present[:, empty].any() and nbr.max() < n_in and nbr.min() >= -1
    return nbr, dict(k_absent=k_absent, k_full=K - 1, empty=empty)


def occupancy_flags(mix, n):
    """not_ones[v] of an occupancy mix: "zeros" (every row occupancy), "ones" (every row walks the table), "runs"."""
    if mix == "zeros":
        return np.zeros(n, np.int32)
    if mix == "ones":
        return np.ones(n, np.int32)
    assert mix == "runs", mix
    return ((np.arange(n) // OCC_RUN) % 2 == 0).astype(np.int32)


def presence_words(nbr):
    """Bit k of a row's words = offset k present (what gcl_presence_bits computes; tests/test_gpu_parity.py checks that)."""
    K, n = nbr.shape
    w = np.zeros((n, (K + 31) // 32), np.uint32)
    for k in range(K):
        w[:, k // 32] |= (nbr[k] >= 0).astype(np.uint32) << np.uint32(k % 32)
    return w


def draw(rng, shape, kind, scale=1.0):
    """fp32 data of a set: "int" small integers |v| <= 2, "gauss" standard normal times `scale`."""
    if kind == "int":
        return rng.randint(-2, 3, shape).astype(np.float32)
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def gathered(nbr, x):
    """A[v][k * Cin + c] = x[nbr[k][v]][c], 0 where absent; fp64.  nbr None: K = 1, row v reads row v."""
    x = np.asarray(x, np.float64)
    if nbr is None:
        return x.copy()
    K, n_out = nbr.shape
    g = np.where((nbr >= 0)[:, :, None], x[np.maximum(nbr, 0)], 0.0)          # [K, n_out, Cin]
    return np.ascontiguousarray(g.transpose(1, 0, 2)).reshape(n_out, K * x.shape[1])


def first_difference(got, want):
    bad = np.argwhere(~(got == want))
    if len(bad) == 0:
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at {i}: {got[i]!r} != {want[i]!r}"


def assert_exact(got, ref, mag, what):
    """Integer data: `ref` (fp64 GEMM of integer operands) is integral, its sum |products| `mag` is below 2^24, and the
    kernel's fp32 result equals it as int64, element for element."""
    assert float(mag.max()) < 2.0 ** 24, (what, float(mag.max()))
    ref_i = ref.astype(np.int64)
    assert np.array_equal(ref_i.astype(np.float64), ref), what
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements left unwritten"
    g = got.astype(np.float64)
    assert np.array_equal(g, ref_i), f"{what}: {first_difference(g, ref_i.astype(np.float64))}"


def fp64_errors(got, ref, mag, depth, what):
    """Gaussian data: (relative L2 against fp64, worst |got - ref| / (depth * 2^-24 * sum |terms|)).  Where the bound is 0
    (no term at all) the element must be exactly 0."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements left unwritten"
    g = got.astype(np.float64)
    err = np.abs(g - ref)
    bound = depth * U * mag
    none = bound == 0
    assert not g[none].any(), f"{what}: an element without terms is not an exact zero"
    ratio = float((err[~none] / bound[~none]).max()) if (~none).any() else 0.0
    rel = float(np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30))
    return rel, ratio
