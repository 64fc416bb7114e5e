"""The pair family's losses on the GPU (csrc/pairloss.hip): against the golden vectors captured from the reference's own
code, and kernel by kernel through the C ABI against the CPU restatement (tests/pair_loss_oracle.py, fp64).

Bounds: returned values within 2e-6 abs and gradients within 1e-5 rel-L2 of the reference's output -- what
test_fcgf_hardest_contrastive_loss_golden holds the sibling loss to (same arithmetic class: fp32 distances of 32-term
rows, a mean of a few thousand O(1) terms); masks and mined rows exactly; the forward value bitwise equal between calls.
"""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/pair_loss_oracle.py
import pair_loss_oracle as PO                                          # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
TRIPLET = sorted(glob.glob(os.path.join(G, "triplet_*.npz")))
HARDEST = sorted(glob.glob(os.path.join(G, "hardest_triplet_*.npz")))
CONTRASTIVE = sorted(glob.glob(os.path.join(G, "contrastive_rand_*.npz")))


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def features(z):
    s = float(z["F_scale"])
    return [(torch.from_numpy(z[k]).float() / s).to(DEV).requires_grad_(True) for k in ("F0_q", "F1_q")]


def triplet_draws(z):
    return (z["pos_sel"] if bool(z["subsampled"]) else None, z["rand_inds"], z["negatives"])


def near(v, ref, what):
    v = v.detach()
    err = abs(float(v) - float(ref))
    print(f"  {what}: {float(v):.9g} vs {float(ref):.9g} (|diff| {err:.2e})")
    return err < 2e-6


# ---------------------------------------------------------------------------------------------------------------
# (b) the three losses against the reference's own outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", TRIPLET, ids=os.path.basename)
def test_triplet_loss_golden(path):
    from gcl_amd.lib.trainer import triplet_loss
    z = np.load(path)
    F0, F1 = features(z)
    kw = dict(num_pos=int(z["num_pos"]), num_hn_samples=int(z["num_hn"]), num_rand_triplet=int(z["num_rand"]),
              neg_thresh=float(z["margin"]))
    det = {}
    loss, pos_dist, neg_dist = triplet_loss(F0, F1, z["pairs"], draws=triplet_draws(z), details=det, **kw)
    assert not pos_dist.requires_grad and not neg_dist.requires_grad and pos_dist.is_cuda and neg_dist.is_cuda
    assert near(loss, z["loss"], "loss") and near(pos_dist, z["pos_dist"], "pos_dist") and near(neg_dist, z["neg_dist"], "neg_dist")
    assert np.array_equal(det["rand_mask"].cpu().numpy().astype(bool), z["rand_mask"])
    loss.backward()
    e0, e1 = rel_l2(F0.grad.cpu(), z["grad0"]), rel_l2(F1.grad.cpu(), z["grad1"])
    print(f"  gradient rel-L2: {e0:.2e} {e1:.2e}")
    assert e0 < 1e-5 and e1 < 1e-5
    again = triplet_loss(F0.detach(), F1.detach(), z["pairs"], draws=triplet_draws(z), **kw)
    assert all(torch.equal(a, b.detach()) for a, b in zip(again, (loss, pos_dist, neg_dist))), "forward value must be bitwise reproducible"
    np.random.seed(int(z["np_seed"]))                 # unseeded call: the draws come out in the reference's order
    l2, p2, n2 = triplet_loss(F0.detach(), F1.detach(), torch.from_numpy(z["pairs"]), **kw)
    assert near(l2, z["loss"], "loss (own draws)") and near(p2, z["pos_dist"], "pos_dist") and near(n2, z["neg_dist"], "neg_dist")


@pytest.mark.parametrize("path", HARDEST, ids=os.path.basename)
def test_hardest_triplet_loss_golden(path):
    from gcl_amd.lib.trainer import hardest_triplet_loss
    z = np.load(path)
    F0, F1 = features(z)
    kw = dict(num_pos=int(z["num_pos"]), num_hn_samples=int(z["num_hn"]), num_rand_triplet=int(z["num_rand"]),
              neg_thresh=float(z["margin"]))
    draws = (z["sel0"], z["sel1"]) + triplet_draws(z)
    det = {}
    loss, pos_dist, neg_dist = hardest_triplet_loss(F0, F1, z["pairs"], draws=draws, details=det, **kw)
    assert not pos_dist.requires_grad and not neg_dist.requires_grad and pos_dist.is_cuda and neg_dist.is_cuda
    for k in ("neg01", "neg10"):                      # the mined rows: the generator made sure none of them is a near tie
        assert np.array_equal(det[k].cpu().numpy(), z[k]), k
    for k in ("rand_mask", "mask0", "mask1"):
        assert np.array_equal(det[k].cpu().numpy().astype(bool), z[k]), k
    assert near(loss, z["loss"], "loss") and near(pos_dist, z["pos_dist"], "pos_dist") and near(neg_dist, z["neg_dist"], "neg_dist")
    loss.backward()
    e0, e1 = rel_l2(F0.grad.cpu(), z["grad0"]), rel_l2(F1.grad.cpu(), z["grad1"])
    print(f"  gradient rel-L2: {e0:.2e} {e1:.2e}")
    assert e0 < 1e-5 and e1 < 1e-5
    again = hardest_triplet_loss(F0.detach(), F1.detach(), z["pairs"], draws=draws, **kw)
    assert all(torch.equal(a, b.detach()) for a, b in zip(again, (loss, pos_dist, neg_dist))), "forward value must be bitwise reproducible"
    np.random.seed(int(z["np_seed"]))
    l2, p2, n2 = hardest_triplet_loss(F0.detach(), F1.detach(), torch.from_numpy(z["pairs"]), **kw)
    assert near(l2, z["loss"], "loss (own draws)") and near(p2, z["pos_dist"], "pos_dist") and near(n2, z["neg_dist"], "neg_dist")


@pytest.mark.parametrize("path", CONTRASTIVE, ids=os.path.basename)
def test_contrastive_random_negative_loss_golden(path):
    from gcl_amd.lib.trainer import contrastive_random_negative_loss, generate_rand_negative_pairs
    z = np.load(path)
    F0, F1 = features(z)
    n0, n1 = len(F0), len(F1)
    cand, keep = generate_rand_negative_pairs(z["pairs"], max(n0, n1), n0, n1, draws=z["candidates"], device=DEV)
    assert np.array_equal(cand.cpu().numpy(), z["candidates"])
    assert np.array_equal(keep.cpu().numpy().astype(bool), z["keep"])
    assert np.array_equal(cand.cpu().numpy()[keep.cpu().numpy().astype(bool)], z["neg_pairs"])     # what the reference returns
    pos, neg = contrastive_random_negative_loss(F0, F1, z["pairs"], float(z["neg_thresh"]), draws=z["candidates"])
    assert near(pos, z["pos"], "pos") and near(neg, z["neg"], "neg")
    (pos + neg).backward()
    e0, e1 = rel_l2(F0.grad.cpu(), z["grad0"]), rel_l2(F1.grad.cpu(), z["grad1"])
    print(f"  gradient rel-L2: {e0:.2e} {e1:.2e}")
    assert e0 < 1e-5 and e1 < 1e-5
    again = contrastive_random_negative_loss(F0.detach(), F1.detach(), z["pairs"], float(z["neg_thresh"]), draws=z["candidates"])
    assert torch.equal(again[0], pos.detach()) and torch.equal(again[1], neg.detach())
    np.random.seed(int(z["np_seed"]))
    p2, n2 = contrastive_random_negative_loss(F0.detach(), F1.detach(), torch.from_numpy(z["pairs"]), float(z["neg_thresh"]))
    assert near(p2, z["pos"], "pos (own draws)") and near(n2, z["neg"], "neg (own draws)")


# ---------------------------------------------------------------------------------------------------------------
# (c) kernel level, through the C ABI
# ---------------------------------------------------------------------------------------------------------------
def _lib():
    from gcl_amd import _lib as L
    return L, L.require_gpu()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def key_mask(ap, seed, pos, col=0, b=None, arg=None):
    L, lib = _lib()
    n_pos = len(pos)
    cap = 64
    while cap < 2 * n_pos:
        cap *= 2
    table = torch.empty((cap, 2), dtype=torch.int64, device=DEV)
    pos_d = dev(pos) if n_pos else None
    L.check(lib.gcl_pair_key_table(L.ptr(pos_d), n_pos, seed, L.ptr(table), cap, None), "table")
    m = len(ap)
    keep = torch.full((m,), 7, dtype=torch.uint8, device=DEV)
    ap_d = dev(ap)
    b_d = dev(b) if b is not None else None
    arg_d = dev(arg, torch.int32) if arg is not None else None
    b_out = torch.full((m,), -5, dtype=torch.int64, device=DEV) if b is not None else None
    L.check(lib.gcl_pair_key_mask(L.ptr(ap_d), col, L.ptr(b_d), L.ptr(arg_d), 0 if b is None else len(b), m, seed,
                                  L.ptr(table), cap, L.ptr(b_out), L.ptr(keep), None), "mask")
    torch.cuda.synchronize()
    return keep.cpu().numpy(), (b_out.cpu().numpy() if b_out is not None else None)


@pytest.mark.parametrize("n_pos,n_rows,seed", [(0, 50, 50), (700, 40, 40), (5000, 3000, 3000),
                                               (3000, 3_000_000_000, 3_000_000_011)])
def test_key_mask_equals_np_isin(n_pos, n_rows, seed):
    """keep = ~np.isin(a + b * seed, p0 + p1 * seed) on random tables: no positives at all, duplicated positives (700 draws
    from a 40 x 40 grid), and row ids whose product with the seed lies far beyond 2^31 (int64 keys)."""
    rng = np.random.RandomState(n_pos + 1)
    lo = max(0, n_rows - 5000)                     # large ids: a narrow band below n_rows, so that candidates hit positives
    pos = rng.randint(lo, n_rows, (n_pos, 2), dtype=np.int64)
    m = 4097
    cand = rng.randint(lo, n_rows, (m, 2), dtype=np.int64)
    if n_pos:
        cand[::3] = pos[rng.randint(0, n_pos, len(cand[::3]))]          # a third of the candidates ARE positives
    want = PO.keep_mask(cand[:, 0], cand[:, 1], pos, seed)
    got, _ = key_mask(cand, seed, pos)
    assert np.array_equal(got.astype(bool), want)
    assert n_pos == 0 or (want.any() and (~want).any())
    # the same candidates as (column of ap, row of b), directly and through an arg-minimum list, on either side
    perm = rng.permutation(m)
    inv = np.argsort(perm)
    for col in (0, 1):
        other = np.ascontiguousarray(cand[:, 1 - col])
        got, b_out = key_mask(cand, seed, pos, col=col, b=other)
        assert np.array_equal(got.astype(bool), want) and np.array_equal(b_out, other)
        got, b_out = key_mask(cand, seed, pos, col=col, b=other[perm], arg=inv)
        assert np.array_equal(got.astype(bool), want) and np.array_equal(b_out, other)
    if seed > 2 ** 31:
        assert int(cand[:, 1].max()) * seed > 2 ** 62


def unit_rows(seed, n, c):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, c, generator=g)
    return f / f.norm(dim=1, keepdim=True)


def run_triplet(F0, F1, ap, neg, tag, keep, margin, g=1.0):
    L, lib = _lib()
    m, c = len(ap), F0.shape[1]
    F0d, F1d = F0.to(DEV).contiguous(), F1.to(DEV).contiguous()
    ap_d, neg_d, tag_d = dev(ap.reshape(-1, 2)), dev(neg), dev(tag, torch.uint8)
    keep_d = dev(keep, torch.uint8) if keep is not None else None
    work = torch.empty(int(lib.gcl_triplet_scratch_len(m)), dtype=torch.float32, device=DEV)
    assert work.numel() == 3 * m
    out = torch.full((L.TRIPLET_OUT,), -3.0, device=DEV)
    nul = lambda t: L.ptr(t) if m else None
    L.check(lib.gcl_triplet_fwd(L.ptr(F0d), len(F0d), L.ptr(F1d), len(F1d), c, nul(ap_d), nul(neg_d), nul(tag_d),
                                nul(keep_d) if keep is not None else None, m, margin, nul(work), L.ptr(out), None), "fwd")
    d0, d1 = torch.zeros_like(F0d), torch.zeros_like(F1d)
    gd = torch.tensor([g], dtype=torch.float32, device=DEV)
    L.check(lib.gcl_triplet_bwd(L.ptr(F0d), len(F0d), L.ptr(F1d), len(F1d), c, nul(ap_d), nul(neg_d), nul(tag_d),
                                nul(keep_d) if keep is not None else None, m, nul(work), L.ptr(out), L.ptr(gd), L.ptr(d0),
                                L.ptr(d1), None), "bwd")
    torch.cuda.synchronize()
    return out.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy()


def triplet_case(seed, c, m, n0=300, n1=260):
    rng = np.random.RandomState(seed)
    F0, F1 = unit_rows(seed, n0, c), unit_rows(seed + 1, n1, c)
    ap = np.stack([rng.randint(0, n0, m), rng.randint(0, n1, m)], 1).astype(np.int64)
    side = rng.randint(0, 2, m)
    neg = np.where(side == 1, rng.randint(0, n0, m), rng.randint(0, n1, m)).astype(np.int64)
    sets = rng.randint(0, 3, m)
    keep = rng.rand(m) < 0.7
    return F0, F1, ap, neg, side, sets, keep


def triplet_reference(F0, F1, ap, neg, side, keep, margin, g):
    D0, D1 = F0.double().requires_grad_(True), F1.double().requires_grad_(True)
    h, dp, dn = PO.triplet_terms(D0, D1, ap, neg, side, margin)
    k = torch.from_numpy(np.asarray(keep, dtype=bool))
    loss = h[k].mean()
    if k.any():
        (g * loss).backward()
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
    return float(loss.detach()), z(D0), z(D1), dp.detach().numpy(), dn.detach().numpy()


@pytest.mark.parametrize("c", [16, 20, 32, 64])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 5000])
def test_triplet_terms_vs_restatement(c, m):
    F0, F1, ap, neg, side, sets, keep = triplet_case(11 * c + m, c, m)
    margin, g = 0.4, 0.7
    tag = (side | (sets << 1)).astype(np.uint8)
    out, d0, d1 = run_triplet(F0, F1, ap, neg, tag, keep, margin, g)
    loss, r0, r1, dp, dn = triplet_reference(F0, F1, ap, neg, side, keep, margin, g)
    assert out[1] == keep.sum()
    if keep.sum() == 0:
        assert np.isnan(out[0]) and not d0.any() and not d1.any()
    else:
        assert abs(out[0] - loss) < 2e-6, (out[0], loss)
        e0, e1 = rel_l2(d0, r0), rel_l2(d1, r1)
        assert (e0 < 1e-5 or not r0.any()) and (e1 < 1e-5 or not r1.any()), (e0, e1)
    for s in range(3):                                     # the per-set statistics
        o = out[2 + 6 * s: 8 + 6 * s]
        a, k = sets == s, (sets == s) & keep
        assert o[0] == k.sum() and o[1] == a.sum()
        for got, sel, d in ((o[2], k, dp), (o[3], k, dn), (o[4], a, dp), (o[5], a, dn)):
            assert (np.isnan(got) and not sel.any()) or abs(got - d[sel].mean()) < 2e-6
    if m:                                                  # no keep mask = every triplet
        out2, _, _ = run_triplet(F0, F1, ap, neg, tag, None, margin, g)
        ref2 = triplet_reference(F0, F1, ap, neg, side, np.ones(m, bool), margin, g)[0]
        assert out2[1] == m and abs(out2[0] - ref2) < 2e-6


def test_triplet_all_masked_gives_nan_and_zero_gradient():
    F0, F1, ap, neg, side, sets, _ = triplet_case(5, 32, 777)
    out, d0, d1 = run_triplet(F0, F1, ap, neg, (side | (sets << 1)).astype(np.uint8), np.zeros(777, bool), 0.4)
    assert np.isnan(out[0]) and out[1] == 0
    assert not d0.any() and not d1.any() and np.isfinite(d0).all() and np.isfinite(d1).all()


def test_triplet_out_of_range_rows_are_dropped_not_read():
    F0, F1, ap, neg, side, sets, keep = triplet_case(6, 32, 400)
    bad = np.arange(0, 400, 7)
    ap2, neg2 = ap.copy(), neg.copy()
    ap2[bad[::3], 0] = 10 ** 12
    neg2[bad[1::3]] = -1
    ap2[bad[2::3], 1] = 260 + 300                          # valid in neither cloud
    out, d0, d1 = run_triplet(F0, F1, ap2, neg2, (side | (sets << 1)).astype(np.uint8), keep, 0.4)
    k2 = keep.copy()
    k2[bad] = False
    loss, r0, r1, _, _ = triplet_reference(F0, F1, ap, neg, side, k2, 0.4, 1.0)
    assert out[1] == k2.sum() and abs(out[0] - loss) < 2e-6
    assert rel_l2(d0, r0) < 1e-5 and rel_l2(d1, r1) < 1e-5


def test_triplet_every_anchor_identical():
    """5000 triplets with ONE anchor row: every channel of that row of dF0 is a sum of 5000 float atomics in an arbitrary
    order.  Per element the bound is the worst case of an arbitrarily ordered fp32 sum, m * 2^-24 * sum_i |term_i|, with the
    terms from the fp64 restatement; every other row (one or a few atomics each) is held to 1e-5 rel-L2."""
    m, c, margin = 5000, 32, 0.4
    F0, F1, ap, neg, _, sets, _ = triplet_case(8, c, m)
    ap[:, 0] = 17
    side = np.zeros(m, dtype=np.int64)
    neg = np.random.RandomState(9).randint(0, len(F1), m).astype(np.int64)
    out, d0, d1 = run_triplet(F0, F1, ap, neg, (sets << 1).astype(np.uint8), None, margin)
    D0, D1 = F0.double(), F1.double()
    A, P, N = D0[17][None], D1[torch.from_numpy(ap[:, 1])], D1[torch.from_numpy(neg)]
    dp, dn = PO.dist(A, P), PO.dist(A, N)
    active = (dp + margin - dn > 0).double()[:, None]
    terms = active * ((A - P) / dp[:, None] - (A - N) / dn[:, None]) / m          # contribution of triplet i to dF0[17]
    ref, bound = terms.sum(0).numpy(), (m * 2.0 ** -24 * terms.abs().sum(0)).numpy()
    err = np.abs(d0[17] - ref)
    print(f"  anchor row: max |err| {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
    assert (err <= bound).all()
    assert not np.delete(d0, 17, axis=0).any()
    loss, _, r1, _, _ = triplet_reference(F0, F1, ap, neg, side, np.ones(m, bool), margin, 1.0)
    assert abs(out[0] - loss) < 2e-6 and rel_l2(d1, r1) < 1e-5


MODES = {0: "sq", 1: "sq_pos", 2: "neg", 3: "dist"}


def run_pairs(F0, F1, pairs, keep, mode, thresh, eps, g=1.0, backward=True):
    L, lib = _lib()
    m, c = len(pairs), F0.shape[1]
    F0d, F1d = F0.to(DEV).contiguous(), F1.to(DEV).contiguous()
    p_d = dev(pairs.reshape(-1, 2))
    keep_d = dev(keep, torch.uint8) if keep is not None else None
    work = torch.empty(int(lib.gcl_pair_terms_scratch_len(m)), dtype=torch.float32, device=DEV)
    out = torch.full((2,), -3.0, device=DEV)
    nul = lambda t: L.ptr(t) if m else None
    kp = nul(keep_d) if keep is not None else None
    L.check(lib.gcl_pair_terms_fwd(L.ptr(F0d), len(F0d), L.ptr(F1d), len(F1d), c, nul(p_d), kp, m, mode, thresh, eps,
                                   nul(work), L.ptr(out), None), "fwd")
    d0, d1 = torch.zeros_like(F0d), torch.zeros_like(F1d)
    if backward:
        gd = torch.tensor([g], dtype=torch.float32, device=DEV)
        L.check(lib.gcl_pair_terms_bwd(L.ptr(F0d), len(F0d), L.ptr(F1d), len(F1d), c, nul(p_d), kp, m, mode, thresh, eps,
                                       nul(work), L.ptr(out), L.ptr(gd), L.ptr(d0), L.ptr(d1), None), "bwd")
    torch.cuda.synchronize()
    return out.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy()


@pytest.mark.parametrize("mode,thresh,eps", [(0, 0.0, 0.0), (1, 1.9, 0.0), (2, 1.4, 1e-4), (2, 1.4, 1e-7), (3, 0.0, 1e-7)])
@pytest.mark.parametrize("c", [16, 32, 64])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 5000])
def test_pair_terms_vs_restatement(mode, thresh, eps, c, m):
    rng = np.random.RandomState(7 * c + m + mode)
    n0, n1 = 310, 270
    F0, F1 = unit_rows(c + m, n0, c), unit_rows(c + m + 1, n1, c)
    pairs = np.stack([rng.randint(0, n0, m), rng.randint(0, n1, m)], 1).astype(np.int64)
    keep = rng.rand(m) < 0.6
    g = 1.3
    out, d0, d1 = run_pairs(F0, F1, pairs, keep, mode, thresh, eps, g, backward=mode != 3)
    D0, D1 = F0.double().requires_grad_(True), F1.double().requires_grad_(True)
    terms = PO.pair_term(D0, D1, pairs[keep], MODES[mode], thresh, eps)
    assert out[1] == keep.sum()
    if keep.sum() == 0:
        assert np.isnan(out[0]) and not d0.any() and not d1.any()
        return
    assert abs(out[0] - float(terms.mean())) < 2e-6
    if m >= 63 and mode in (1, 2):
        assert (terms > 0).any() and (terms == 0).any(), "the case must hold active and inactive hinges"
    if mode != 3:
        (g * terms.mean()).backward()
        assert rel_l2(d0, D0.grad.numpy()) < 1e-5 and rel_l2(d1, D1.grad.numpy()) < 1e-5
    out2, _, _ = run_pairs(F0, F1, pairs, None, mode, thresh, eps, backward=False)
    assert out2[1] == m and abs(out2[0] - float(PO.pair_term(F0.double(), F1.double(), pairs, MODES[mode], thresh, eps).mean())) < 2e-6


def test_invalid_arguments_are_rejected_with_a_message():
    L, lib = _lib()
    p8 = ctypes.c_void_p(8)
    err = lambda: lib.gcl_last_error()
    assert lib.gcl_pair_key_table(p8, 10, 5, p8, 48, None) == -1 and b"power of two" in err()
    assert lib.gcl_pair_key_table(p8, 100, 5, p8, 128, None) == -1 and b"power of two" in err()
    assert lib.gcl_pair_key_table(None, 10, 5, p8, 64, None) == -1 and b"null" in err()
    assert lib.gcl_pair_key_table(p8, 10, 0, p8, 64, None) == -1 and b"seed" in err()
    assert lib.gcl_pair_key_mask(p8, 2, p8, None, 10, 10, 5, p8, 64, None, p8, None) == -1 and b"col" in err()
    assert lib.gcl_pair_key_mask(p8, 0, None, p8, 10, 10, 5, p8, 64, None, p8, None) == -1 and b"candidate rows" in err()
    assert lib.gcl_pair_key_mask(p8, 0, p8, None, 5, 10, 5, p8, 64, None, p8, None) == -1 and b"fewer rows" in err()
    assert lib.gcl_triplet_fwd(p8, 5, p8, 5, 65, p8, p8, p8, None, 4, 0.4, p8, p8, None) == -1 and b"feature width" in err()
    assert lib.gcl_triplet_fwd(p8, 5, p8, 5, 32, p8, None, p8, None, 4, 0.4, p8, p8, None) == -1 and b"null" in err()
    assert lib.gcl_triplet_bwd(p8, 5, p8, 5, 32, p8, p8, p8, None, 4, p8, p8, None, p8, p8, None) == -1 and b"null" in err()
    assert lib.gcl_pair_terms_fwd(p8, 5, p8, 5, 32, p8, None, 4, 7, 0.0, 0.0, p8, p8, None) == -1 and b"mode" in err()
    assert lib.gcl_pair_terms_bwd(p8, 5, p8, 5, 32, p8, None, 4, 3, 0.0, 1e-7, p8, p8, p8, p8, p8, None) == -1 \
        and b"no backward" in err()
    assert lib.gcl_pair_terms_fwd(p8, 5, p8, 5, 0, p8, None, 4, 0, 0.0, 0.0, p8, p8, None) == -1 and b"feature width" in err()
    assert lib.gcl_triplet_scratch_len(0) == 0 and lib.gcl_triplet_scratch_len(1000) == 3000
    assert lib.gcl_pair_terms_scratch_len(-3) == 0 and lib.gcl_pair_terms_scratch_len(1000) == 1000
