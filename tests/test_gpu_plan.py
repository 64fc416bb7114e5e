"""The native step runtime (csrc/plan.hip, gcl_amd/MinkowskiEngine/native.py) against the per-operator path:
``gcl_maps_build`` against CoordinateManager's own launches (bit-exact tables), ``gcl_plan_forward / _backward`` against
the Tape (bitwise-equal features, gradients, losses and parameters over several optimizer steps), the tape guards of
ADVICE round 2, and the two-rank data-parallel step with the bucket all-reduce started between backward segments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(seed, n=4000, batch=2, extent=24):
    """Unique int32 coords [N,4]: a thin sheet (LiDAR-like) plus a blob, negative coordinates included."""
    rng = np.random.RandomState(seed)
    cs = []
    for b in range(batch):
        pts = rng.randint(-extent, extent, (n, 3))
        pts[: n // 2, 2] = rng.randint(-1, 1, n // 2)
        c = np.unique(pts, axis=0)
        rng.shuffle(c)
        cs.append(np.concatenate([np.full((len(c), 1), b), c], axis=1))
    return np.concatenate(cs).astype(np.int32)


def _model(k1=5):
    from gcl_amd.model import load_model
    torch.manual_seed(5)
    return load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=k1, D=3).to(DEV)


@pytest.mark.parametrize("seed,n,batch", [(0, 4000, 2), (1, 300, 1), (2, 20000, 3)])
def test_native_maps_equal_the_per_operator_maps(seed, n, batch):
    """ONE gcl_maps_build call == the launches CoordinateManager issues from Python: coordinates of every level, kernel
    maps, transposed maps, pair counts, mask-sorted tables (table, order, tile masks) and pair lists, bit for bit."""
    import gcl_amd.MinkowskiEngine as ME
    C = torch.from_numpy(_cloud(seed, n, batch)).to(DEV)
    specs = _model().native_map_specs()
    with torch.cuda.device(DEV):
        ref = ME.CoordinateManager(C).prefetch([s for s in specs if s[1] > 1])
        nat = ME.CoordinateManager.build_native(C, specs)
        assert nat.native is not None and nat.native.desc.arena_used <= nat.native.arena.numel()
        for t in (1, 2, 4, 8):
            assert torch.equal(ref.get_coords(t), nat.get_coords(t)), t
        for t_in, ks, stride, tables, pairs in (s[:5] for s in specs):
            if ks == 1:
                a, b = ref.identity_pairs(len(C)), nat.identity_pairs(len(C))
                assert torch.equal(a[0], b[0]) and a[2] == b[2]
                continue
            ka, kb = ref.get_kernel_map(t_in, ks, stride), nat.get_kernel_map(t_in, ks, stride)
            assert torch.equal(ka.nbr, kb.nbr) and ka.counts == kb.counts and ka.n_pairs == kb.n_pairs
            assert (ka.nbr_t is None) == (kb.nbr_t is None)
            if ka.nbr_t is not None:
                assert torch.equal(ka.nbr_t, kb.nbr_t)
            for tr in tables:
                for u, v in zip(ka.sorted_table(transposed=tr), kb.sorted_table(transposed=tr)):
                    assert torch.equal(u, v), (t_in, ks, stride, tr)
            if pairs:
                pa, pb = ka.pairs(), kb.pairs()
                assert pa[2] == pb[2] and torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
        # inference specs: no pair lists, presence words of the first layer's table (bit k of row v = nbr[k][v] >= 0)
        ispecs = _model().native_map_specs(training=False)
        assert not any(s[4] for s in ispecs) and sum(len(s) > 5 for s in ispecs) == 1
        inf = ME.CoordinateManager.build_native(C, ispecs).native
        for i, sp in enumerate(ispecs):
            d = inf.desc.maps[i]
            assert bool(d.presence) == (len(sp) > 5) and d.n_pairs == 0
            if len(sp) > 5:
                K, n_out = int(d.K), int(d.n_out)
                words = (K + 31) // 32
                got = inf.view(d.presence, (n_out, words), torch.int32).cpu().numpy().view(np.uint32)
                nb = inf.view(d.nbr, (K, n_out), torch.int32).cpu().numpy()
                want = np.zeros((n_out, words), np.uint32)
                for k in range(K):
                    want[:, k // 32] |= (nb[k] >= 0).astype(np.uint32) << np.uint32(k % 32)
                assert np.array_equal(got, want)


@pytest.mark.parametrize("seed,n,batch", [(0, 4000, 2), (1, 300, 1), (2, 20000, 3)])
def test_kernel_map_3_from_5_equals_the_probed_map(seed, n, batch):
    """gcl_kernel_map_3_from_5 (the shortcut of gcl_maps_build: the 3^3 stride-1 map of the input table as
    27 rows of its 5^3 map) == the map the probing pass builds: neighbour table and pair counts, bit
    for bit."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd import _lib
    lib = _lib.load()
    C = torch.from_numpy(_cloud(seed, n, batch)).to(DEV)
    with torch.cuda.device(DEV):
        mgr = ME.CoordinateManager(C)
        k5, k3 = mgr.get_kernel_map(1, 5, 1), mgr.get_kernel_map(1, 3, 1)
        nbr3 = torch.full_like(k3.nbr, -7)
        counts3 = torch.full((27,), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.gcl_kernel_map_3_from_5(_lib.ptr(k5.nbr), _lib.ptr(k5._counts_dev), len(C), _lib.ptr(nbr3),
                                               _lib.ptr(counts3), _lib.stream()), "gcl_kernel_map_3_from_5")
        assert torch.equal(nbr3, k3.nbr)
        assert counts3.tolist() == list(k3.counts)


def test_native_maps_reject_bad_coordinates():
    import gcl_amd.MinkowskiEngine as ME
    specs = _model().native_map_specs()
    C = torch.from_numpy(_cloud(3, 500, 1)).to(DEV)
    dup = torch.cat([C, C[:3]])
    with torch.cuda.device(DEV):
        with pytest.raises(ValueError, match="duplicate"):
            ME.CoordinateManager.build_native(dup, specs)
        far = C.clone()
        far[0, 1] = 40000
        with pytest.raises(ValueError, match="packable"):
            ME.CoordinateManager.build_native(far, specs)
        with pytest.raises(ValueError, match="not part of the native map build"):
            ME.CoordinateManager.build_native(C, specs).get_kernel_map(2, 5, 1)


@pytest.mark.parametrize("k1", [5, 3])
def test_plan_pass_equals_the_tape_bitwise(k1):
    """One forward + backward pass: the recorded NetworkPlan (ONE gcl_plan_forward, ONE gcl_plan_backward) gives the
    same features, parameter gradients and running statistics as the Tape / per-operator path on the same maps -- bit
    for bit -- both with gradients handed to autograd and with seated (written in place) gradients."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import native
    C = torch.from_numpy(_cloud(7, 5000, 2)).to(DEV)
    g = torch.Generator().manual_seed(1)
    F = torch.ones(len(C), 1, device=DEV)
    dF = torch.randn(len(C), 32, generator=g).to(DEV)
    with torch.cuda.device(DEV):
        m = _model(k1)
        state0 = {k: v.clone() for k, v in m.state_dict().items()}
        mgr = ME.CoordinateManager.build_native(C, m.native_map_specs())

        def run(expect_plan, seat=False):
            m.load_state_dict(state0)
            for p in m.parameters():
                p.grad = None
            m.train()
            x = ME.SparseTensor(F, coordinates=C, coordinate_manager=mgr)
            plan = m.plan_for(x)
            assert (plan is not None) == expect_plan
            if seat:
                seats = [torch.full_like(p, 7.0) for p in m.parameters()]       # stale contents must be overwritten
                plan.grad_targets = seats
            out = m(x).F
            out.backward(dF)
            if seat:
                plan.grad_targets = None
                assert all(p.grad is None for p in m.parameters())
                grads = seats
            else:
                grads = [p.grad for p in m.parameters()]
            torch.cuda.synchronize()
            return out.detach().clone(), [t.clone() for t in grads], {k: v.clone() for k, v in m.state_dict().items()}

        assert m._plan is None
        ref = run(False)                     # recorded by the Tape; becomes the plan
        assert isinstance(m._plan, native.NetworkPlan), getattr(m, "_plan_error", None)
        assert len(m._plan.records) == 28      # 21 conv+BN, 3 cat, 2 heads, relu, row normalise
        for seat in (False, True):
            got = run(True, seat)
            assert torch.equal(ref[0], got[0]), "features"
            for (name, _), a, b in zip(m.named_parameters(), ref[1], got[1]):
                assert torch.equal(a, b), name
            for k in ref[2]:
                assert torch.equal(ref[2][k], got[2][k]), k
        # a second pass while the first one still waits for its backward: arenas are per pass, nothing is overwritten
        x = ME.SparseTensor(F, coordinates=C, coordinate_manager=mgr)
        m.load_state_dict(state0)
        o1 = m(x).F
        keep = o1.detach().clone()
        o2 = m(ME.SparseTensor(F * 2, coordinates=C, coordinate_manager=mgr)).F
        assert torch.equal(o1.detach(), keep) and not torch.equal(o2.detach(), keep)
        (o1.sum() + o2.sum()).backward()
        torch.cuda.synchronize()


@pytest.mark.parametrize("k1", [5, 3])
def test_inference_plan_equals_the_per_operator_eval_path(k1):
    """model.eval() under torch.no_grad(): ONE gcl_maps_build + ONE gcl_plan_forward_eval (every conv + BatchNorm
    (+ residual)(+ ReLU) a single fused launch, packed kernels persistent across passes) gives bitwise the features of the
    per-operator eval path -- on the traced first pass, on later passes, on other clouds, after the parameters changed
    (a training step with FusedSGD, which bumps the parameter versions), and through forward_clouds' batching."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import native
    from gcl_amd.scripts.test_kitti import forward_clouds
    clouds = [torch.from_numpy(_cloud(s, 4000 + 500 * s, 1)).to(DEV) for s in (11, 12, 13)]
    feats = [torch.ones(len(c), 1, device=DEV) for c in clouds]
    with torch.cuda.device(DEV):
        m = _model(k1)
        # make the running statistics and the affine parameters non-trivial
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                    mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
                    mod.weight.copy_(0.5 + torch.rand(mod.num_features, generator=g))
                    mod.bias.copy_(0.1 * torch.randn(mod.num_features, generator=g))
        m.eval()

        def reference(C, F):
            old, native.PLAN_ENABLED = native.PLAN_ENABLED, False
            try:
                with torch.no_grad():
                    return m(ME.SparseTensor(F, coordinates=C)).F.clone()
            finally:
                native.PLAN_ENABLED = old

        refs = [reference(c, f) for c, f in zip(clouds, feats)]
        with torch.no_grad():
            assert m._plan is None
            first = m(ME.SparseTensor(feats[0], coordinates=clouds[0])).F.clone()          # traced pass
            assert isinstance(m._plan, native.NetworkPlan), getattr(m, "_plan_error", None)
            assert torch.equal(first, refs[0])
            for c, f, r in zip(clouds, feats, refs):                                       # plan passes
                assert torch.equal(m(ME.SparseTensor(f, coordinates=c)).F, r)
            batched = forward_clouds(m, [(f, c) for f, c in zip(feats, clouds)])
            for got, r in zip(batched, refs):
                assert torch.equal(got, r)
            # the same sets through forward_clouds_stream (maps of the coming sets built on a side stream by a helper
            # thread): single clouds from host memory, then mixed set sizes -- bit for bit the same features, in order
            from gcl_amd.scripts.test_kitti import forward_clouds_stream
            host = [(f.cpu(), c.cpu()) for f, c in zip(feats, clouds)]
            for rep in range(2):
                got = list(forward_clouds_stream(m, ([fc] for fc in host), device=DEV))
                assert len(got) == len(refs) and all(len(g) == 1 and torch.equal(g[0], r) for g, r in zip(got, refs))
            sets = [[(feats[0], clouds[0]), (feats[1], clouds[1])], [(feats[2], clouds[2])], [(feats[1], clouds[1]), (feats[0], clouds[0])]]
            got = list(forward_clouds_stream(m, sets, device=DEV, depth=1))
            want = [[refs[0], refs[1]], [refs[2]], [refs[1], refs[0]]]
            assert all(len(g) == len(w) and all(torch.equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))
        # parameters change behind the persistent packed kernels: one optimizer step through the fused SGD kernel
        from gcl_amd.lib.optim import FusedSGD
        m.train()
        opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.8, weight_decay=1e-4)
        out = m(ME.SparseTensor(feats[1], coordinates=clouds[1])).F
        out.square().mean().backward()
        opt.step()
        m.eval()
        with torch.no_grad():
            after = m(ME.SparseTensor(feats[2], coordinates=clouds[2])).F
            assert not torch.equal(after, refs[2])
            assert torch.equal(after, reference(clouds[2], feats[2]))


@pytest.mark.parametrize("n", [1, 37, 300])
def test_plan_on_tiny_clouds(n):
    """Edge sizes (one voxel, fewer rows than a 32-row wave tile / a 128-row workgroup tile, coarse levels of one or two
    rows): the native maps + plan -- training pass and inference pass -- equal the per-operator path bit for bit."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import native
    rng = np.random.RandomState(n)
    pts = np.unique(rng.randint(-5, 5, (4 * n + 8, 3)), axis=0)[:n]
    C = torch.from_numpy(np.concatenate([np.zeros((len(pts), 1), int), pts], 1).astype(np.int32)).to(DEV)
    F = torch.ones(len(C), 1, device=DEV)
    dF = torch.randn(len(C), 32, generator=torch.Generator().manual_seed(n)).to(DEV)
    with torch.cuda.device(DEV):
        m = _model(3)
        state0 = {k: v.clone() for k, v in m.state_dict().items()}

        def train_pass(plan_on):
            m.load_state_dict(state0)
            m.train()
            for p in m.parameters():
                p.grad = None
            old, native.PLAN_ENABLED = native.PLAN_ENABLED, plan_on
            try:
                mgr = ME.CoordinateManager.build_native(C, m.native_map_specs()) if plan_on else ME.CoordinateManager(C)
                out = m(ME.SparseTensor(F, coordinates=C, coordinate_manager=mgr)).F
                out.backward(dF)
            finally:
                native.PLAN_ENABLED = old
            torch.cuda.synchronize()
            return out.detach().clone(), [p.grad.clone() for p in m.parameters()]

        ref = train_pass(False)
        train_pass(True)                      # recorded by the Tape on native maps
        got = train_pass(True)                # through the plan
        assert isinstance(m._plan, native.NetworkPlan), getattr(m, "_plan_error", None)
        assert torch.equal(ref[0], got[0])
        for (name, _), a, b in zip(m.named_parameters(), ref[1], got[1]):
            assert torch.equal(a, b), name
        m.load_state_dict(state0)
        m.eval()
        with torch.no_grad():
            e_plan = m(ME.SparseTensor(F, coordinates=C)).F.clone()
            old, native.PLAN_ENABLED = native.PLAN_ENABLED, False
            try:
                e_ref = m(ME.SparseTensor(F, coordinates=C)).F.clone()
            finally:
                native.PLAN_ENABLED = old
        assert torch.equal(e_plan, e_ref)


def _train(cfg_kw, n_steps, plan, batches, iter_size=1, seed=3):
    from gcl_amd.MinkowskiEngine import native
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config, prefetch_to_device
    keys = ("sinput_C", "sinput_F", "group", "index", "finest_flag")
    host = [{k: v for k, v in b.items() if k in keys} for b in batches]
    old = native.PLAN_ENABLED
    native.PLAN_ENABLED = plan
    try:
        torch.manual_seed(seed)
        np.random.seed(seed)
        tr = FinestContrastiveLossTrainer(make_config(iter_size=iter_size, **cfg_kw), device=DEV)
        seq = [host[i % len(host)] for i in range(n_steps * iter_size)]
        losses = [l.item() for l, _, _ in tr.train_steps(prefetch_to_device(seq, DEV, keys))]
        torch.cuda.synchronize()
        used = isinstance(tr.model._plan, native.NetworkPlan)
        return losses, torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).cpu(), used, \
            {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    finally:
        native.PLAN_ENABLED = old


@pytest.mark.parametrize("iter_size", [1, 2])
def test_training_steps_with_the_plan_equal_the_per_operator_path(iter_size):
    """VERDICT round 2, item 1 "done" criterion: 5 optimizer steps through train_steps (H2D prefetch, native map build on
    the side stream, plan forward / backward, fused SGD) give bitwise-equal losses and parameters to the same run with
    GCL_PLAN off (Python map build, Tape, autograd-assigned gradients) -- with lr = 0, where every step is a deterministic
    function of its batch and draws (losses, BatchNorm running statistics: exact equality).  With lr > 0 the loss
    backward's float atomics (the one order-dependent piece of a step, as the reference's index_add on CUDA) feed back
    through the parameters, so the two runs are compared at 1e-5; the gradients themselves are compared bit for bit, without
    atomics in the way, by test_plan_pass_equals_the_tape_bitwise."""
    from gcl_amd import synthetic
    batches = [synthetic.collate_train([synthetic.make_train_sample(s, num_neighborhood=2, n_boxes=10)]) for s in (41, 42, 43)]
    kw = dict(batch_size=1, num_pos_per_batch=64, num_hn_samples_per_batch=128, lr=0.0, weight_decay=0.0)
    a = _train(kw, 5, False, batches, iter_size)
    b = _train(kw, 5, True, batches, iter_size)
    assert not a[2] and b[2], "the second run must have gone through the plan"
    assert a[0] == b[0], (a[0], b[0])
    assert torch.equal(a[1], b[1])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k                # running statistics, num_batches_tracked
    # parameters that move: the first steps are deterministic up to the loss backward's atomics -> compare at 1e-6
    kw["lr"], kw["weight_decay"] = 0.05, 1e-4
    a = _train(kw, 4, False, batches, iter_size)
    a2 = _train(kw, 4, False, batches, iter_size)            # the same path twice: what the atomics alone do to a run
    b = _train(kw, 4, True, batches, iter_size)
    noise = float((a[1] - a2[1]).abs().max())
    diff = float((a[1] - b[1]).abs().max())
    print(f"iter_size {iter_size}: max |param difference| per-operator vs itself {noise:.3e}, vs plan {diff:.3e}; losses "
          f"{a[0]} / {b[0]}")
    # hardest-negative mining is discontinuous, so last-bit differences of the atomics can grow to ~1e-3 within a few
    # steps (the same path against itself shows it): this part only checks that the plan trains the same way
    assert b[2] and np.allclose(a[0], b[0], rtol=5e-3, atol=1e-4), (a[0], b[0])
    assert diff <= max(20 * noise, 5e-3 * float(a[1].abs().max()))


def test_tape_equals_per_layer_autograd_and_frozen_bn_leaves_the_tape():
    """the whole-network Tape == the per-layer autograd path bit for bit; a BatchNorm in eval mode
    inside a training model (frozen-BN fine-tuning) makes forward leave the Tape instead of silently cutting the
    gradient, and consumers the Tape does not know fail loudly."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd.MinkowskiEngine import ops
    C = torch.from_numpy(_cloud(9, 3000, 1)).to(DEV)
    F = torch.ones(len(C), 1, device=DEV)
    dF = torch.randn(len(C), 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.cuda.device(DEV):
        m = _model()
        state0 = {k: v.clone() for k, v in m.state_dict().items()}

        def grads(tape, freeze=False):
            m.load_state_dict(state0)
            m.train()
            if freeze:
                m.block2.norm1.eval()
            for p in m.parameters():
                p.grad = None
            old, ops.TAPE_ENABLED = ops.TAPE_ENABLED, tape
            try:
                out = m(ME.SparseTensor(F, coordinates=C)).F
                out.backward(dF)
            finally:
                ops.TAPE_ENABLED = old
            return [None if p.grad is None else p.grad.clone() for p in m.parameters()]

        a, b = grads(True), grads(False)
        for (name, _), u, v in zip(m.named_parameters(), a, b):
            assert u is not None and torch.equal(u, v), name
        fa, fb = grads(True, freeze=True), grads(False, freeze=True)
        for (name, _), u, v in zip(m.named_parameters(), fa, fb):
            assert u is not None and v is not None and torch.equal(u, v), name
        assert float(fa[0].abs().max()) > 0          # conv1.kernel sits upstream of the frozen layer: gradient arrives
        with ops.tape() as tp:
            y, _ = ops.sparse_conv(torch.ones(len(C), 32, device=DEV), m.block1.conv1.kernel,
                                   ME.CoordinateManager(C).get_kernel_map(1, 3, 1), len(C), False, None, None)
            with pytest.raises(RuntimeError, match="Tape"):
                bn = m.block1.norm1.bn
                ops.batch_norm(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, 0.05, 1e-5)


def test_two_ranks_on_one_device_overlap_the_decoder_bucket(tmp_path):
    """configs[3] first-run safety: a FRESH child process per rank (torch.distributed.run,
    gloo, both ranks on cuda:0) runs bench.py's N = 2 path for 3 steps with the plan: FlatDDP buckets are started by
    ``bucket_ready`` between the plan's backward segments (decoder bucket first, before the encoder records run), both
    ranks end with identical finite parameters, and they equal a single-process run fed the averaged gradients."""
    env = dict(os.environ, GCL_BENCH_SINGLE_DEVICE="1", GCL_DDP_SELFTEST="1", MASTER_ADDR="127.0.0.1")
    env.pop("RANK", None)
    out = str(tmp_path)
    env["GCL_DDP_SELFTEST_DIR"] = out
    r = None
    for attempt in (0, 1):      # the run takes 10 - 15 s; ONE retry if the two-process rendezvous on a shared device stalls
        # (seen once in ~40 runs of round 4: 900 s of silence, five clean repeats after it); --standalone: the launcher binds
        # its own free rendezvous port
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", "2", os.path.join(ROOT, "tools", "ddp_selftest.py")]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
            break
        except subprocess.TimeoutExpired:
            if attempt == 1:
                raise
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = [json.load(open(os.path.join(out, f"rank{k}.json"))) for k in (0, 1)]
    assert rec[0]["param_sha"] == rec[1]["param_sha"] and rec[0]["finite"] and rec[1]["finite"]
    assert rec[0]["plan_used"] and rec[1]["plan_used"]
    for k in (0, 1):
        assert rec[k]["launch_order"] and rec[k]["launch_order"][0] == rec[k]["n_buckets"] - 1, rec[k]
        assert rec[k]["first_bucket_before_record"] > 0, "decoder bucket started before the encoder records ran"
        # averaged-gradient reference = the same batches accumulated in one process; the runs differ by summation order (and
        # the loss backward's atomics), which hardest-negative mining can amplify to ~1e-4 within 3 steps; a missing
        # average or a stale bucket would show at ~1e-2
        assert rec[k]["max_abs_diff_vs_averaged_single_process"] <= 1e-3 * rec[k]["max_abs_param"], rec[k]


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` WITHOUT a launcher must start two ranks itself (child
    torch.distributed.run; here both on cuda:0 over gloo through the GCL_BENCH_SINGLE_DEVICE test hook) and print a line
    with n_gpus == 2 -- never a silent 1-GPU number.  Without the hook, on this 1-GPU box, the same command must refuse."""
    env = dict(os.environ, GCL_BENCH_SINGLE_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--resident",
           "--batches", "1", "--no-kernel-events"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks"]["rccl_ranks"] == 2 and rec["ranks"]["backend"] == "gloo"
    assert len(rec["ranks"]["voxels_per_step_per_rank"]) == 2 and rec["config"]["parallelism"] == "dp2"
    if torch.cuda.device_count() < 2:
        env.pop("GCL_BENCH_SINGLE_DEVICE")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "refusing" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_plain_run_times_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    """A plain `bench.py` run prints one JSON line with the headline keys, times exactly --steps steps and measures none of
    the --full figures (roofline, cpu_baseline, secondary); --dump-outputs writes the last timed step's loss (the line's own
    `config.loss`), its parts and the model's state after the update as float arrays.  A second run with the same arguments
    has the same inputs exactly and, the dumped step starting from the seeded initial state, the same outputs up to the
    rounding of the loss backward's float atomics."""
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GCL_BENCH_SINGLE_DEVICE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batches", "2",
           "--dump-outputs"]
    r = subprocess.run(cmd + [str(out)], env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r2 = subprocess.run(cmd + [str(tmp_path / "again")], env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    rec = json.loads(lines[0])
    assert all(k in rec for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"))
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["full"] is False
    assert rec["roofline"] is None and "secondary" not in rec and "cpu_baseline" not in rec
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert {"loss.npy", "loss_parts.npy", "active_voxels.npy", "state.conv1.kernel.npy"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert float(files["loss.npy"]) == rec["config"]["loss"]
    # the last of 2 + 3 steps over two batches in rotation ran on the first batch
    assert float(files["active_voxels.npy"]) == rec["config"]["voxels_per_batch_rank0"][0]
    assert all(np.isfinite(a).all() for a in files.values())
    rec2 = json.loads([ln for ln in r2.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec2["config"]["voxels_per_batch_rank0"] == rec["config"]["voxels_per_batch_rank0"]
    again = {p.name: np.load(p) for p in (tmp_path / "again").iterdir()}
    assert again.keys() == files.keys() and float(again["active_voxels.npy"]) == float(files["active_voxels.npy"])
    bad = [k for k in files if not np.allclose(again[k], files[k], rtol=1e-5, atol=1e-6)]
    assert not bad, [(k, float(np.abs(again[k].astype(np.float64) - files[k]).max())) for k in bad[:5]]


def test_frozen_parameter_keeps_the_step_off_the_plan():
    """with one convolution frozen (requires_grad=False, fine-tuning) a training step must not
    go through the plan -- it writes every record's gradient through raw pointers and the trainer seats p.grad for all
    of model.parameters(), so SGD (weight decay, momentum) would move the frozen tensor.  The step stays on the Tape:
    p.grad of the frozen kernel stays None, it keeps its bits, every other parameter still trains."""
    import gcl_amd.MinkowskiEngine as ME
    from gcl_amd import synthetic
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    with torch.cuda.device(DEV):
        cfg = make_config(batch_size=1)
        trainer = FinestContrastiveLossTrainer(cfg, device=torch.device(DEV))
        keys = ("sinput_C", "sinput_F", "group", "index", "finest_flag")
        batches = [{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in
                    synthetic.make_train_batch(300 + j, batch_size=1, num_neighborhood=2, n_boxes=12).items() if k in keys}
                   for j in range(2)]
        frozen = trainer.model.block2.conv1.kernel
        frozen.requires_grad_(False)
        before = frozen.detach().clone()
        other = trainer.model.block2.conv2.kernel.detach().clone()
        np.random.seed(0)
        steps = trainer.train_steps(iter([batches[0], batches[1], batches[0], batches[1]]))
        for _ in range(4):
            loss, _, _ = next(steps)
            assert torch.isfinite(loss).item()
            plan = trainer.model.__dict__.get("_plan")
            if plan:                                  # recorded by step 1, but never handed out while a tensor is frozen
                probe_mgr = ME.CoordinateManager.build_native(batches[0]["sinput_C"], trainer.model.native_map_specs())
                x = ME.SparseTensor(batches[0]["sinput_F"], coordinates=batches[0]["sinput_C"], coordinate_manager=probe_mgr)
                assert trainer.model.plan_for(x) is None
        steps.close()
        torch.cuda.synchronize()
        assert frozen.grad is None and torch.equal(frozen, before)
        assert not torch.equal(trainer.model.block2.conv2.kernel, other)
        # un-frozen again, the same model goes back to the plan
        frozen.requires_grad_(True)
        x = ME.SparseTensor(batches[0]["sinput_F"], coordinates=batches[0]["sinput_C"], coordinate_manager=probe_mgr)
        assert trainer.model.plan_for(x) is not None
