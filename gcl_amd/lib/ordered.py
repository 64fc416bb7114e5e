"""The loss backward without float atomics (``deterministic_loss_backward``): record lists and the ordered row sum.

A loss backward entry of the library adds its contributions into dF with float atomics, whose order -- and with it the
rounding of every row that receives more than one -- changes from run to run.  Its ``*_emit`` twin writes the same values
as records at fixed positions; ``gcl_ordered_row_sum`` adds them row by row in ascending position (include/gcl_amd.h,
DESIGN.md section 6).  The helpers here allocate the lists and run the reduction; the autograd functions of
``lib/colocation_trainer.py`` and ``lib/trainer.py`` call the emit entries themselves."""
import numpy as np
import torch

from gcl_amd import _lib


def records(n_rec, c, device):
    """``(rec_row int32 [n_rec], rec_val float32 [n_rec, c])``, uninitialised: every emit entry fills ``rec_row`` itself."""
    return (torch.empty(int(n_rec), dtype=torch.int32, device=device),
            torch.empty((int(n_rec), int(c)), dtype=torch.float32, device=device))


def ordered_row_sum(rec_row, rec_val, dF):
    """dF[row] = (..((dF[row] + v_1) + v_2) .. + v_k) over the row's records in ascending position, for every named row."""
    lib = _lib.load()
    n_rec, (n_rows, c) = int(rec_row.shape[0]), dF.shape
    ns = int(lib.gcl_ordered_row_sum_scratch_len(n_rec, n_rows))
    if ns == 0:
        return dF
    scratch = torch.empty(ns, dtype=torch.int32, device=dF.device)
    _lib.check(lib.gcl_ordered_row_sum(_lib.ptr(rec_row, torch.int32), _lib.ptr(rec_val, torch.float32), n_rec, c, n_rows,
                                       _lib.ptr(scratch), _lib.ptr(dF, torch.float32), _lib.stream()), "gcl_ordered_row_sum")
    return dF


def members_bound(group, pos_sel, index):
    """A host-known bound of the sum of the selected groups' sizes (what sizes the record list of the two group losses):
    the sum itself when the group sizes are on the host, else the length of ``index``, which bounds it when no group is
    selected twice.  Never reads the device."""
    pos_sel = np.asarray(pos_sel)
    if not (torch.is_tensor(group) and group.is_cuda):
        return int(np.asarray(group)[pos_sel].sum())
    if len(np.unique(pos_sel)) != len(pos_sel):
        raise ValueError("deterministic_loss_backward: a group is selected twice and the group sizes are on the device only; "
                         "pass the sizes as a host tensor")
    return int(index.shape[0])
