"""gcl_ordered_row_sum alone, against a numpy loop that adds np.float32 values one after the other in list order: the
comparison is EXACT.  Values have random signs and magnitudes from 2^-20 to 2^20, so that a row's sum depends on the order
of its additions -- asserted on the CPU for the rows with many records (ascending against descending order and against
np.sum), otherwise the exact comparison would prove nothing about order.

The kernel takes a row's record ids in windows of L = gcl_ordered_row_sum_window() consecutive ids (a bitmap in LDS), 64 ids
per bitmap word, 256 records per block of its counting kernels: the counts and the hub sizes sit on both sides of each."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ordered_records import serial, values                             # noqa: E402

DEV = "cuda:0"
WIDTHS = (1, 4, 31, 32, 33, 64)


def _lib():
    from gcl_amd import _lib as L
    return L, L.require_gpu()


def window():
    return int(_lib()[1].gcl_ordered_row_sum_window())


def run(rec_row, rec_val, df, n_rows=None):
    L, lib = _lib()
    n_rec, c = len(rec_row), df.shape[1]
    n_rows = len(df) if n_rows is None else n_rows
    with torch.cuda.device(DEV):
        row_d = torch.from_numpy(np.ascontiguousarray(rec_row, dtype=np.int32)).to(DEV)
        val_d = torch.from_numpy(np.ascontiguousarray(rec_val, dtype=np.float32)).to(DEV)
        df_d = torch.from_numpy(df.copy()).to(DEV)
        ns = int(lib.gcl_ordered_row_sum_scratch_len(n_rec, n_rows))
        assert ns == (2 + 2 * n_rows + 3 * n_rec if n_rec > 0 and n_rows > 0 else 0)
        scratch = torch.full((max(ns, 1),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # stale words: the call fills what it reads
        nul = lambda t: L.ptr(t) if n_rec else None
        L.check(lib.gcl_ordered_row_sum(nul(row_d), nul(val_d), n_rec, c, n_rows, L.ptr(scratch), L.ptr(df_d), L.stream()),
                "gcl_ordered_row_sum")
        torch.cuda.synchronize()
    return df_d.cpu().numpy()


def random_list(rng, n_rec, n_rows, c):
    """n_rec records over n_rows rows: row 0 and row n_rows - 1 named (when the list has two records), about a tenth of the
    records with row -1 or a row >= n_rows, some rows named several times, at least a third named by nobody."""
    rows = rng.randint(0, max(1, n_rows // 2), n_rec).astype(np.int64)
    bad = rng.rand(n_rec) < 0.1
    rows[bad] = rng.choice([-1, -5, n_rows, n_rows + 7, 2 ** 31 - 1], int(bad.sum()))
    if n_rec >= 2:
        a, b = rng.choice(n_rec, 2, replace=False)
        rows[a], rows[b] = 0, n_rows - 1
    return rows.astype(np.int32), values(rng, n_rec, c)


def counts():
    L = window()
    return sorted({0, 1, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, 2 * L + 1})


@pytest.mark.parametrize("c", WIDTHS)
def test_random_lists_at_every_count_exactly(c):
    for n_rec in counts():
        rng = np.random.RandomState(1000 * c + n_rec)
        n_rows = 97
        rec_row, rec_val = random_list(rng, n_rec, n_rows, c)
        df = values(rng, n_rows, c)
        want = serial(rec_row, rec_val, df)
        got = run(rec_row, rec_val, df)
        assert np.array_equal(got, want), (c, n_rec, int((got != want).any(1).sum()))
        named = np.zeros(n_rows, dtype=bool)
        ok = (rec_row >= 0) & (rec_row < n_rows)
        named[rec_row[ok]] = True
        assert got[~named].tobytes() == df[~named].tobytes()              # rows nobody names: bit for bit
        if n_rec >= 2:
            assert named[0] and named[n_rows - 1] and (~named).sum() * 3 >= n_rows
        if n_rec >= 64:
            assert (~ok).any() and (rec_row < 0).any() and (rec_row >= n_rows).any()
        # the same input again: the same bytes
        assert run(rec_row, rec_val, df).tobytes() == got.tobytes()


def hub_list(rng, k, c, n_rows=50, hub=17, spread=1):
    """One row (``hub``) named by k records whose ids are ``spread`` apart, every other row named once, the single records
    standing before, between and behind the hub's; some skipped records mixed in."""
    others = [r for r in range(n_rows) if r != hub]
    n_rec = k * spread + len(others) + 9
    rows = np.full(n_rec, -1, dtype=np.int64)
    first = 5
    hub_ids = first + spread * np.arange(k)
    rows[hub_ids] = hub
    free = np.setdiff1d(np.arange(n_rec), hub_ids)
    rows[rng.choice(free, len(others), replace=False)] = others
    rows[rows == -1] = rng.choice([-1, n_rows, n_rows + 3], int((rows == -1).sum()))
    return rows.astype(np.int32), values(rng, n_rec, c), hub_ids


@pytest.mark.parametrize("c", (1, 32, 33, 64))
def test_hub_row_at_the_window_edges_exactly(c):
    L = window()
    for k, spread in ((1, 1), (2, 1), (L, 1), (L + 1, 1), (3 * L + 5, 1), (70, L // 4 + 1), (5, 2 * L + 3)):
        rng = np.random.RandomState(7 * c + k + spread)
        rec_row, rec_val, hub_ids = hub_list(rng, k, c, spread=spread)
        n_rows, hub = 50, 17
        df = values(rng, n_rows, c)
        want = serial(rec_row, rec_val, df)
        if k >= 64:           # the order of the additions shows in the result: else an exact match says nothing about it
            down = serial(rec_row, rec_val, df, order=range(len(rec_row) - 1, -1, -1))
            assert (want[hub] != down[hub]).any(), "ascending and descending serial sums agree"
            flat = df[hub] + np.sum(rec_val[hub_ids], axis=0, dtype=np.float32)
            assert (want[hub] != flat).any(), "the serial sum equals np.sum"
        got = run(rec_row, rec_val, df)
        bad = np.nonzero((got != want).any(1))[0]
        assert np.array_equal(got, want), (c, k, spread, bad[:8])
        assert (np.bincount(rec_row[(rec_row >= 0) & (rec_row < n_rows)], minlength=n_rows) == np.where(
            np.arange(n_rows) == hub, k, 1)).all()
        assert run(rec_row, rec_val, df).tobytes() == got.tobytes()


def test_every_record_names_one_row_and_rows_past_n_rows_are_skipped():
    """3000 records on ONE row (three windows), the others skipped: n_rows below the length of dF leaves the rest of dF alone."""
    rng = np.random.RandomState(3)
    c, n_rec = 32, 3000
    rec_row = np.where(rng.rand(n_rec) < 0.8, 3, 6).astype(np.int32)
    rec_val = values(rng, n_rec, c)
    df = values(rng, 8, c)
    got = run(rec_row, rec_val, df, n_rows=5)                                # row 6 is >= n_rows: skipped
    want = serial(np.where(rec_row == 3, 3, -1), rec_val, df)
    assert np.array_equal(got, want) and got[[0, 1, 2, 4, 5, 6, 7]].tobytes() == df[[0, 1, 2, 4, 5, 6, 7]].tobytes()
    down = serial(np.where(rec_row == 3, 3, -1), rec_val, df, order=range(n_rec - 1, -1, -1))
    assert (want[3] != down[3]).any()
