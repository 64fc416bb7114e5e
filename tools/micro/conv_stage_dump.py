"""Convolution forward / weight gradient, every kernel path as raw bytes: a dump to compare two builds of the library bit for bit.

Writes into ONE .npz the bytes (uint8 arrays) of

  * ``y``, the BatchNorm tile partials and max|y| of every entry of CASES in tests/test_gpu_conv_instances.py
                                                                                      (keys fwd<i>/<y | partials | amax>)
  * the inference layer of tests/test_gpu_conv_epilogue.py (2051 rows, 128 -> 128, GCL_CONV_TALL) without and with the fused
    epilogue, through the offset-group launches (scratch handed over) and the sixteen-wave kernel
                                                                                      (keys infer/<groups | tall>/<plain | fused>)
  * ``dW`` of every entry of CASES in tests/test_gpu_dw_instances.py                  (keys dw<i>)
  * one gcl_conv_bwd_weight_rows launch (40967 rows, 64 x 32)                         (key rows/dw)
  * one first-layer forward + weight gradient (530003 rows, K = 27, 1 -> 32: more 64-row tiles than the 1024 workgroups of
    the weight gradient take eight each)                                              (keys stem/y, stem/dw)

The case tables and input builders are those of the two test files, and every launch goes through the C ABI (``_lib``), so
the file runs unchanged in a checkout of any commit that has those tests; ``GCL_LIB_PATH`` selects another build of the
library with the same exports.

    python3 tools/micro/conv_stage_dump.py --out A.npz
    python3 tools/micro/conv_stage_dump.py --compare A.npz B.npz        # every differing key; exit status 1 if there is one
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def _raw(t):
    return np.frombuffer(t.detach().contiguous().cpu().numpy().tobytes(), np.uint8)


def dump(path):
    import torch
    import test_gpu_conv_epilogue as CE
    import test_gpu_conv_instances as CI
    import test_gpu_dw_instances as DW
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd import _lib
    lib = _lib.require_gpu()
    dev = CI.DEV
    res = {}
    for i, (prec, cin, cout, conv, n, form, epi, flags, _nb) in enumerate(CI.CASES):
        y, stats, amax = CI.problem(n, conv, cin, cout).run(prec, form, epi, flags)
        res[f"fwd{i}/y"] = _raw(y)
        if stats is not None:
            res[f"fwd{i}/partials"] = _raw(stats)
        if amax is not None:
            res[f"fwd{i}/amax"] = _raw(torch.as_tensor(amax, dtype=torch.float32))
    CI._PROBLEMS.clear()
    p = CE.layer(2051, 128, 128)
    gs_len = lib.gcl_conv_fwd_groups_scratch_len(p.n, 27, p.cin, p.cout)
    assert gs_len > 0
    for kernel in ("groups", "tall"):
        scratch = torch.empty(gs_len, dtype=torch.float32, device=dev) if kernel == "groups" else None
        res[f"infer/{kernel}/plain"] = _raw(p.launch("rows", CE.TALL, partials=False, scratch=scratch)[0])
        y, _, amax = p.launch("rows", CE.TALL, scale=True, bias=True, res="own", relu=1, amax=True, partials=False, scratch=scratch)
        res[f"infer/{kernel}/fused"] = _raw(y)
        res[f"infer/{kernel}/fused_amax"] = _raw(torch.as_tensor(amax, dtype=torch.float32))
    for i, case in enumerate(DW.CASES):
        lname, ca, cb, prec, pl = case[:5]
        q = DW.problem(lname, ca, cb)
        res[f"dw{i}"] = _raw(q.run(prec, pl, q.L.side))
    DW._PROBLEMS.clear()
    g = torch.Generator().manual_seed(5)
    with torch.cuda.device(dev):
        n, ca, cb = 40967, 64, 32
        a, b = torch.randn(n, ca, generator=g).to(dev), (torch.randn(n, cb, generator=g) * 3e-3).to(dev)
        aa, ba = ME.ops.amax_slot(a.device), ME.ops.amax_slot(a.device)
        _lib.check(lib.gcl_amax(_lib.ptr(a), a.numel(), _lib.ptr(aa), 1, _lib.stream()), "gcl_amax")
        _lib.check(lib.gcl_amax(_lib.ptr(b), b.numel(), _lib.ptr(ba), 1, _lib.stream()), "gcl_amax")
        ln = lib.gcl_conv_bwd_weight_rows_scratch_len(ca, cb, 4, n)
        assert ln > 0
        scratch, dw = torch.empty(ln, device=dev), torch.empty(ca, cb, device=dev)
        _lib.check(lib.gcl_conv_bwd_weight_rows(_lib.ptr(a), _lib.ptr(b), n, ca, cb, 4, _lib.ptr(aa), _lib.ptr(ba),
                                                _lib.ptr(scratch), _lib.ptr(dw), _lib.stream()), "gcl_conv_bwd_weight_rows")
        res["rows/dw"] = _raw(dw)
        n, K, cin, cout = 530003, 27, 1, 32
        x, w = torch.randn(n, cin, generator=g).to(dev), (0.1 * torch.randn(K, cin, cout, generator=g)).to(dev)
        dy = (torch.randn(n, cout, generator=g) * 3e-3).to(dev)
        nbr = torch.randint(-1, n, (K, n), generator=g, dtype=torch.int32).to(dev)
        y = torch.empty(n, cout, device=dev)
        _lib.check(lib.gcl_stem_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(nbr), n, K, cin, cout, _lib.ptr(y), None, None,
                                    _lib.stream()), "gcl_stem_fwd")
        scratch = torch.empty(lib.gcl_stem_bwd_weight_scratch_len(K, cin, cout, n), device=dev)
        dw = torch.empty(K, cin, cout, device=dev)
        _lib.check(lib.gcl_stem_bwd_weight(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(nbr), n, K, cin, cout, _lib.ptr(scratch),
                                           _lib.ptr(dw), None, None, _lib.stream()), "gcl_stem_bwd_weight")
        torch.cuda.synchronize()
        res["stem/y"], res["stem/dw"] = _raw(y), _raw(dw)
    np.savez(path, **res)
    print(f"{len(res)} arrays -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"only in one dump: {k}")
    for k in sorted(set(A.files) & set(B.files)):
        if A[k].shape != B[k].shape or not np.array_equal(A[k], B[k]):
            n = int((A[k] != B[k]).sum()) if A[k].shape == B[k].shape else -1
            print(f"differs: {k} ({n} of {A[k].size} bytes)")
            bad.append(k)
    print(f"{len(set(A.files) & set(B.files))} common keys, {len(bad)} differing")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="conv_stage_dump.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out)


if __name__ == "__main__":
    main()
