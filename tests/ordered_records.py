"""What the tests of the ordered loss backward share (test infrastructure, numpy on the CPU): the serial replay of a record
list, which is the contract of gcl_ordered_row_sum (include/gcl_amd.h), and the per-row fp64 sums of a list."""
import numpy as np


def values(rng, n, c):
    """float32 [n, c] with random signs and magnitudes 2^-20 .. 2^20: sums of them depend on the order of the additions"""
    return (rng.choice([-1.0, 1.0], (n, c)) * np.exp2(rng.uniform(-20, 20, (n, c)))).astype(np.float32)


def serial(rec_row, rec_val, df, order=None):
    """dF[row] = fl(.. fl(fl(dF[row] + v_1) + v_2) .. + v_k) in fp32 over the records in list order (``order``: another order
    of the list); records with a row outside [0, len(df)) are skipped."""
    out = np.array(df, dtype=np.float32, copy=True)
    n_rows = len(out)
    for i in (range(len(rec_row)) if order is None else order):
        r = int(rec_row[i])
        if 0 <= r < n_rows:
            out[r] = out[r] + rec_val[i]              # float32 + float32: one rounding per addition
    return out


def named(rec_row, n_rows):
    ok = (rec_row >= 0) & (rec_row < n_rows)
    return ok, np.bincount(rec_row[ok], minlength=n_rows)


def row_sums64(rec_row, rec_val, n_rows):
    """the per-row sum of the records in fp64"""
    ok, _ = named(rec_row, n_rows)
    out = np.zeros((n_rows, rec_val.shape[1]))
    np.add.at(out, rec_row[ok], rec_val[ok].astype(np.float64))
    return out
