"""Headline benchmark: active voxels / second through ResUNetBN2C fwd + GCL loss + bwd + SGD step
(BASELINE.json metric; workload = configs[2], the GCL training step at KITTI 0.3 m, bs = 4 x 7 clouds).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    (N > 1: launched by torch.distributed.run, one rank per GPU, RCCL gradient all-reduce over xGMI)

One "step" = SURVEY.md 8(d)'s t_step on one synthetic batch: host -> device copy of the batch (pinned memory, issued one
step ahead on a copy stream: what a loader does), SparseTensor / coordinate-map build, kernel maps, 23 sparse convs +
21 BNs forward, finest-contrastive loss, backward, (gradient all-reduce,) SGD step.  The timed region rotates over
``--batches`` (default 4) DISTINCT pre-generated batches, so coordinates, hash tables and cache contents change every
step.  Rank 0 prints ONE JSON line.  A plain run does only what that line's headline needs: batches, warm-up, the K timed
steps.  ``--full`` adds the figures that cost time of their own: `roofline` prices the dominant HIP kernel (per-launch
times measured by events on the launch stream in the last timed step) against the pipe it actually runs on -- the fp16
MFMA pipe for the fp16x3 convolutions (every fp32 product = 3 fp16 MFMA terms), HBM for bandwidth-bound kernels;
`cpu_baseline` times the C / OpenMP restatement of MinkowskiEngine's CPU path (oracle/me_cpu.c, kind "port") on the
SAME first batch, all usable host cores; `secondary` measures configs[1] / configs[4] in a child process.
``--dump-outputs DIR`` writes what the last timed step computed (loss, its three parts, the step's voxel count, the
model's parameters and BatchNorm statistics after its SGD update) as DIR/<name>.npy, after the clock has stopped.  That
step starts from the seeded initial model and optimizer state (put back with the clock stopped), so that its outputs
are the same in every run to rounding: the loss backward's float atomics differ in the last bit from run to run, and
over many steps training amplifies that.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
F32_MATRIX_PEAK_TFS = 157.3   # MI355X_MICROARCH.md: dense f32 matrix peak (spec)
F16_MFMA_PEAK_TFS = 2500.0    # MI355X_MICROARCH.md: dense bf16 / fp16 MFMA peak (spec, no sparsity)
MFMA_TERMS = {"fp16x3": 3, "bf16x3": 3, "bf16x6": 6, "f32": 1}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)      # ~0.9 s timed: short regions ride the clock ramp of a cold box
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--batches", type=int, default=4, help="distinct pre-generated batches the steps rotate over")
    ap.add_argument("--group-mode", default="fixed16", choices=["fixed16", "radius"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--resident", action="store_true",
                    help="diagnostic: keep the batches in HBM (no H2D in the step); the line is then NOT the headline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the configs[1] / configs[4] measurements appended as `secondary` (N = 1 only)")
    ap.add_argument("--full", action="store_true",
                    help="also measure roofline (kernel events in the last timed step), cpu_baseline and secondary; a "
                         "plain run times the headline only (--no-* switch single figures off again)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, < 64 MB); that "
                         "step starts from the seeded initial state, so the outputs repeat from run to run")
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--secondary-worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def usable_cores():
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota (os.cpu_count() reports the
    whole host and over-subscribes a quota-limited container by an order of magnitude)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except Exception:
            pass
    return max(1, min(n, 64))


def _gen_sample(job):
    from gcl_amd import synthetic
    seed, group_mode = job
    return synthetic.make_train_sample(seed, group_mode=group_mode)


def make_batches(rank, n, batch_size, group_mode):
    """``n`` distinct synthetic batches of this rank (seeds 100 + rank + 1000 j), generated by worker processes BEFORE
    anything touches the GPU (the generator is numpy / scipy loader work and is not timed).  Batch j is
    synthetic.make_train_batch(seed_j, batch_size, group_mode=group_mode): its samples (each seeded on its own,
    seed_j * 1000 + b) are one job each, so that all of the batches' samples are generated at once, and are collated here."""
    from gcl_amd import synthetic
    seeds = [100 + rank + 1000 * j for j in range(n)]
    jobs = [(s * 1000 + b, group_mode) for s in seeds for b in range(batch_size)]
    workers = max(1, min(len(jobs), usable_cores() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))))
    profiled = "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or \
        any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ)
    if workers == 1 or profiled:       # under rocprofv3 the GPU is initialised before main(): no forked workers then
        samples = [_gen_sample(j) for j in jobs]
    else:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(workers) as pool:
            samples = pool.map(_gen_sample, jobs)
    return [synthetic.collate_train(samples[j * batch_size:(j + 1) * batch_size]) for j in range(n)]


DUMP_LIMIT_BYTES = 64 * 1000 * 1000


def dump_outputs(out_dir, loss, parts, n_vox, model):
    """What the last timed step computed, as out_dir/<name>.npy: ``loss`` and ``loss_parts`` (pos, finest, neg; float32),
    ``active_voxels`` (float64) and ``state.<key>`` for every floating-point entry of the model's state dict after the
    step's SGD update (parameters and BatchNorm running statistics, float32).  Above DUMP_LIMIT_BYTES in all, every array
    of more than 4096 values is replaced by the same fraction of its flattened values (indices drawn from a seeded
    generator, sorted), so that the same arguments always dump the same positions."""
    arrays = {"loss": np.asarray(loss.detach().float().cpu().numpy(), dtype=np.float32),
              "loss_parts": np.array([p.item() for p in parts], dtype=np.float32),
              "active_voxels": np.array(float(n_vox), dtype=np.float64)}
    for k, v in model.state_dict().items():
        if v.is_floating_point():
            arrays[f"state.{k}"] = v.detach().float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        frac = 0.9 * DUMP_LIMIT_BYTES / total
        rng = np.random.RandomState(0)
        for k in sorted(arrays):
            a = arrays[k].reshape(-1)
            if a.size > 4096:
                arrays[k] = a[np.sort(rng.choice(a.size, max(4096, int(a.size * frac)), replace=False))]
        total = sum(a.nbytes for a in arrays.values())
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)
    log(f"dumped {len(arrays)} arrays ({total / 1e6:.1f} MB) of the last timed step to {out_dir}")


def cpu_baseline_worker():
    """The C / OpenMP restatement of ME's CPU path (oracle/me_cpu.c: hash map -> kernel maps -> gather / GEMM /
    scatter-add per offset; BatchNorm, ReLU, loss in torch-CPU fp32) on the SAME batch the GPU line starts with
    (seed 100, bs 4 x 7 clouds, groups fixed16): coordinate + kernel maps, forward, loss, backward.  All usable cores.
    Bounded: one untimed warm-up step, then at most 8 steps / ~20 s of timed CPU work."""
    from gcl_amd import synthetic
    from oracle import loss_oracle, me_cpu, me_oracle
    args = parse()
    cores = int(os.environ.get("GCL_CPU_BASELINE_CORES", "0")) or usable_cores()      # (diagnostic override: thread-count sweeps)
    torch.set_num_threads(cores)
    me_cpu.lib().me_set_num_threads(cores)
    batch = synthetic.make_train_batch(100, batch_size=args.batch_size, group_mode=args.group_mode)
    C, F = batch["sinput_C"].numpy(), batch["sinput_F"].float()
    st = me_oracle.random_state(0, dtype=torch.float32)
    n_done, t_total = -1, 0.0      # step -1: untimed warm-up (round 6: the first step pays the first touch of ~10 GB of saved
    np.random.seed(0)              # activations and the library load -- 17 s against 5.7 s warm on the GPU box's host; the GPU line is warm too)
    while t_total < 20.0 and n_done < 8:
        leaves = {k: v.clone().requires_grad_("running" not in k) for k, v in st.items()}
        t0 = time.perf_counter()
        mgr = me_cpu.CoordinateManager(C)          # coordinate + kernel maps are part of the step
        out = me_oracle.resunet_forward(leaves, C, F, 5, True, True, 0.05, mgr=mgr)
        pos, fin, neg = loss_oracle.finest_contrastive_loss(out, batch["group"].numpy(), batch["index"].numpy(),
                                                            batch["index_hash"], batch["finest_flag"].numpy(),
                                                            max_pos_cluster=256 * args.batch_size,
                                                            max_hn_samples=256 * args.batch_size)
        (pos + fin + neg).backward()
        if n_done >= 0:
            t_total += time.perf_counter() - t0
        n_done += 1
    return {"value": round(len(C) * n_done / t_total, 1), "unit": "active voxels/s", "cores": cores, "kind": "port",
            "sample": f"{n_done} step(s) on the GPU line's first batch (seed 100, bs {args.batch_size} x 7 clouds, "
                      f"{len(C)} voxels): maps + fwd + loss + bwd, C/OpenMP restatement of ME's CPU gather-GEMM-scatter "
                      f"(oracle/me_cpu.c, fp32) + torch-CPU BatchNorm / loss, {t_total:.1f} s after one untimed warm-up step; glibc malloc "
                      f"without mmap / trim (the child's environment, bench.cpu_baseline)"}


def cpu_baseline(args, timeout_s=300):
    """Runs the worker in a child process (never touches the GPU) under a hard wall-clock limit.
    The child's glibc malloc keeps its memory (no mmap per large block, no trimming, one arena): with the defaults the
    autograd backward pass of this 530 k-voxel step returns and re-faults gigabytes of temporaries per step and spends 13 of
    its 15 s in the kernel's page-fault path (measured on the GPU box's host, tools/micro/cpu_baseline_profile.py: 16.2 ->
    1.9 s per step) -- that is the allocator, not the algorithm the baseline stands for."""
    import subprocess
    try:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", MALLOC_ARENA_MAX="1", MALLOC_TRIM_THRESHOLD_="100000000000",
                   MALLOC_MMAP_THRESHOLD_="100000000000")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", "--batch-size",
                            str(args.batch_size), "--group-mode", args.group_mode], capture_output=True,
                           text=True, timeout=timeout_s, env=env)
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:   # report, never hang the benchmark line
        return {"value": None, "unit": "active voxels/s", "cores": usable_cores(), "kind": "port",
                "sample": f"CPU baseline did not finish within {timeout_s} s ({type(e).__name__})"}


def secondary_in_child(timeout_s=360):
    """The configs[1] / configs[4] figures from a CHILD process (never an exec; started after the headline region, the GPU is
    idle by then): the headline line must not depend on them -- neither on an exception nor on a fault that ends the process
    that runs them."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--secondary-worker"], capture_output=True, text=True,
                           timeout=timeout_s)
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"secondary worker exited with code {r.returncode}: {r.stderr.strip()[-300:]}"}
        return json.loads(lines[-1])
    except Exception as e:
        return {"error": f"{type(e).__name__}: {e}"}


def spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment: run
    `python -m torch.distributed.run --standalone --local-addr 127.0.0.1 --nnodes=1 --nproc-per-node N bench.py <argv>`
    as a child process (one rank per GPU, RCCL), forward its output and return its exit code.  With fewer than N devices
    visible the line is refused -- a 1-GPU number must never be printed under `n_gpus: N`.  (GCL_BENCH_SINGLE_DEVICE=1, a
    test hook the driver never sets, puts every rank on cuda:0 with gloo to exercise this code path on a 1-GPU box.)"""
    import subprocess
    single = os.environ.get("GCL_BENCH_SINGLE_DEVICE") == "1"
    # The launcher below is started as a CHILD process (subprocess.run), never by replacing this one (exec), so whether
    # counting devices initialises the HIP runtime in this parent does not matter.
    n_dev = torch.cuda.device_count()
    if not single and n_dev < args.gpus:
        print(f"bench.py: --gpus {args.gpus} requested but only {n_dev} device(s) are visible; refusing to time fewer "
              f"GPUs than the line would claim", file=sys.stderr, flush=True)
        return 2
    # --standalone: the launcher binds its own free rendezvous port (no bind / release / re-bind window for another process)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), os.path.abspath(__file__)] + sys.argv[1:]
    log("no launcher in the environment: starting " + " ".join(cmd))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def roofline_of(prof, precision, aux_names=(), ms_per_step=None):
    """Roofline of the dominant kernel from the per-launch event records of the last timed step.  ``aux_names``: kernels
    whose launches run on the plan's second stream BESIDE the main stream's kernels (the weight gradients): their event
    intervals overlap main-stream work (they roughly double when two streams share the chip), so they are listed but do
    not compete for "dominant" -- the step time is the main stream's chain, and by exclusive time (GCL_PLAN_AUX=0 runs,
    profiles/) the forward / input-gradient kernel stays the largest."""
    agg = {}
    terms = MFMA_TERMS.get(precision, 3)
    log("per-launch timings of the last timed step (events on the launch stream):")
    for name, e0, e1, pairs, cin, cout, n_in, n_out, K in prof:
        ms = e0.elapsed_time(e1) if e1 is not None else e0          # plan records carry the measured ms directly
        by = pairs * (cin + cout) * 4.0 + pairs * 8.0                      # algorithmic bytes of a launch
        fl = 2.0 * pairs * cin * cout
        comp = (n_in * cin + n_out * cout) * 4.0 + K * cin * cout * 4.0 + pairs * 8.0      # compulsory bytes
        log(f"  {name:36s} pairs={pairs:9d} {cin:3d}->{cout:3d}  {ms * 1e3:7.1f} us  "
            f"{fl / (ms * 1e-3) / 1e12:6.1f} TFLOP/s  {by / (ms * 1e-3) / 1e9:7.0f} GB/s")
        a = agg.setdefault(name, [0.0, 0.0, 0.0, 0, 0.0])
        a[0] += ms
        a[1] += by
        a[2] += fl
        a[3] += 1
        a[4] += comp
    dom = max((k for k in agg if k not in aux_names), key=lambda k: agg[k][0])
    ms, by, fl, cnt, comp = agg[dom]
    gbs, tfs = by / (ms * 1e-3) / 1e9, fl / (ms * 1e-3) / 1e12
    traffic = mfma_busy = step_traffic = None
    pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
    pmc_note = "no profiles/pmc_summary.json"
    if os.path.exists(pmc):
        from gcl_amd import _lib
        allrec = json.load(open(pmc))
        # the counter passes are separate runs (tools/collect_profiles.sh): their figures are quoted only when they were
        # collected on the kernel sources this process is timing (sha256 stamp), otherwise null
        if allrec.get("_csrc_sha16") == _lib.source_hash():
            rec = allrec.get(dom.replace(" ", ""), {})
            traffic, mfma_busy = rec.get("hbm_bytes_per_launch"), rec.get("mfma_busy")
            # every kernel's counter bytes x its launches, per step of the profiled command
            n_prof = float(allrec.get("_steps", 10))
            step_traffic = sum(v["hbm_bytes_per_launch"] * v["launches"] for k, v in allrec.items()
                               if isinstance(v, dict) and "hbm_bytes_per_launch" in v and "launches" in v) / n_prof
            pmc_note = f"profiles/pmc_summary.json, collected on these kernel sources (sha16 {allrec['_csrc_sha16']})"
        else:
            pmc_note = (f"profiles/pmc_summary.json was collected on other kernel sources (sha16 {allrec.get('_csrc_sha16')} != "
                        f"{_lib.source_hash()}): traffic / mfma_busy not quoted")
    split = "split" in dom or "k_conv_fwd_dma" in dom                # the fp16 / bf16 split-MFMA convolution kernels
    peak_tf = F16_MFMA_PEAK_TFS if split else F32_MATRIX_PEAK_TFS
    pipe_tfs = tfs * (terms if split else 1)
    # which roof bounds the kernel: its algorithmic intensity against the ridge of the pipe it runs on
    mfma_bound = (fl * (terms if split else 1)) / by > peak_tf * 1e12 / (HBM_PEAK_GBS * 1e9) or \
        pipe_tfs / peak_tf > gbs / HBM_PEAK_GBS
    out = {"bound": "mfma" if mfma_bound else "hbm", "kernel": dom,
           "achieved": round(pipe_tfs if mfma_bound else gbs, 2), "peak": peak_tf if mfma_bound else HBM_PEAK_GBS,
           "unit": "TFLOP/s" if mfma_bound else "GB/s",
           "frac": round(pipe_tfs / peak_tf if mfma_bound else gbs / HBM_PEAK_GBS, 4),
           "traffic": traffic, "launches": cnt, "avg_launch_us": round(ms * 1e3 / cnt, 2),
           # counter bytes / launch time against the HBM peak: what the fabric really moved for this kernel (the algorithmic
           # figure above counts every gather, also those an L2 serves)
           "frac_traffic": round(traffic / (ms * 1e-3 / cnt) / (HBM_PEAK_GBS * 1e9), 4) if traffic else None,
           "step_traffic_GB": round(step_traffic / 1e9, 2) if step_traffic else None,
           "step_frac_traffic": (round(step_traffic / (ms_per_step * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
                                 if step_traffic and ms_per_step else None),
           "algorithmic_GBps": round(gbs, 1), "algorithmic_fp32_TFLOPs": round(tfs, 2),
           "mfma_terms_per_product": terms if split else 1, "peak_pipe_TFs": peak_tf,
           "frac_pipe": round(pipe_tfs / peak_tf, 4), "frac_hbm": round(gbs / HBM_PEAK_GBS, 4),
           "frac_vs_f32_matrix_peak": round(tfs / F32_MATRIX_PEAK_TFS, 4), "mfma_busy": mfma_busy,
           "avg_algorithmic_MB_per_launch": round(by / cnt / 1e6, 3),
           "compulsory_MB_per_launch": round(comp / cnt / 1e6, 3),
           "note": "algorithmic = exact sparse work of the layer (pairs*(Cin+Cout)*4+8 B, 2*pairs*Cin*Cout flop, SURVEY 8d); "
                   "achieved (mfma) = algorithmic flop x MFMA terms per fp32 product / launch time, priced against the "
                   "dense fp16 MFMA peak (the pipe the kernel runs on); frac_vs_f32_matrix_peak is the same launch "
                   "against the exact-f32 MFMA peak (can exceed 1: not the kernel's roof); traffic / mfma_busy: separate "
                   "rocprofv3 --pmc passes of this command -- " + pmc_note + "; frac_traffic = traffic / avg launch time / "
                   "HBM peak; step_traffic_GB = sum over ALL kernels of a step of their counter bytes (main, weight-gradient "
                   "and map streams), step_frac_traffic = that / ms_per_step / HBM peak",
           "kernel_ms_last_step": {k: round(v[0], 3) for k, v in agg.items() if k not in aux_names},
           "overlapped_aux_stream_kernel_ms_last_step": {k: round(v[0], 3) for k, v in agg.items() if k in aux_names}}
    if aux_names:
        out["note"] += ("; overlapped_aux_stream_kernel_ms_last_step: the weight-gradient launches, which run on a second "
                        "stream beside the main stream's kernels -- their event intervals include the time they share the "
                        "chip (about twice their exclusive duration) and they are not candidates for the dominant kernel")
    return out


def _gen_secondary(job):
    from gcl_amd import synthetic
    kind, seed, arg = job
    if kind == "pair":
        return synthetic.make_eval_pair(seed, baseline=arg)
    if kind == "twin":
        return synthetic.make_twin_eval_pair(seed, arg)
    return synthetic.make_raw_sample(seed)


def secondary_inputs(twin_share=0.5, raw_batches=2, batch_size=4):
    """The synthetic inputs of `secondary`, generated by forked workers BEFORE the process touches the GPU (numpy ray casts:
    ~50 s on one core): 8 eval pairs, 8 twin pairs, ``raw_batches`` x ``batch_size`` raw training samples (7 scans each)."""
    jobs = [("pair", 100 + s, 15.0 + 5.0 * (s % 6)) for s in range(8)] + [("twin", 200 + s, twin_share) for s in range(8)] + \
           [("raw", 100 + 1000 * j + b, None) for j in range(raw_batches) for b in range(batch_size)]
    workers = max(1, min(len(jobs), usable_cores()))
    if workers == 1:
        res = [_gen_secondary(j) for j in jobs]
    else:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(workers) as pool:
            res = pool.map(_gen_secondary, jobs)
    raws = res[16:]
    return {"pairs": res[:8], "twins": res[8:16], "twin_share": twin_share,
            "raw_batches": [raws[j * batch_size:(j + 1) * batch_size] for j in range(raw_batches)]}


def end_to_end_from_scans(dev, raw_batches, steps=20, warmup=8):
    """The training step fed from RAW scans (missing #2 of VERDICT round 5; reference: the DataLoader pull inside the iteration,
    lib/colocation_trainer.py:838-846, over __getitem__ + collate, lib/colocation_data_loader.py:315-475): host -> device copy
    of the raw points (pinned), voxelisation, co-location groups (the reference's radius groups), collate on a loader stream
    a step ahead (gcl_amd.lib.colocation_data_gpu.train_from_scans), then the headline's step."""
    from gcl_amd import synthetic
    from gcl_amd.lib.colocation_data_gpu import build_batch_gpu, train_from_scans
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config
    torch.manual_seed(0)
    np.random.seed(0)
    bs = len(raw_batches[0])
    trainer = FinestContrastiveLossTrainer(make_config(batch_size=bs), device=dev)
    out = {"raw_points_per_sample": int(np.mean([sum(len(x) for x in s["xyz"]) for b in raw_batches for s in b])),
           "clouds_per_sample": len(raw_batches[0][0]["xyz"]), "batch_size": bs, "groups": "radius (the reference's)"}
    with torch.cuda.device(dev):
        # the loader alone: build_batch_gpu back to back, pinned staging + H2D of the raw points included
        for _ in range(2):
            b = build_batch_gpu(raw_batches[0], 0.3, dev, jitter=synthetic.raw_sample_jitter(raw_batches[0]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 6
        for i in range(reps):
            b = build_batch_gpu(raw_batches[i % len(raw_batches)], 0.3, dev,
                                jitter=synthetic.raw_sample_jitter(raw_batches[i % len(raw_batches)]))
        torch.cuda.synchronize()
        out["loader_alone_ms_per_sample"] = round((time.perf_counter() - t0) / reps / bs * 1e3, 3)
        out["voxels_per_batch"] = int(len(b["sinput_C"]))
        out["groups_per_batch"] = int(len(b["group"]))
        del b
        depth = 2 + max(1, int(os.environ.get("GCL_PREFETCH_DEPTH", "2")))
        feed = (raw_batches[i % len(raw_batches)] for i in range(warmup + steps + depth))
        it = train_from_scans(trainer, feed, voxel_size=0.3, jitter=synthetic.raw_sample_jitter)
        for _ in range(warmup):
            next(it)
        torch.cuda.synchronize()
        t0, nv = time.perf_counter(), 0
        for _ in range(steps):
            loss, _, n = next(it)
            nv += n
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        it.close()
    out["ms_per_step"] = round(dt / steps * 1e3, 3)
    out["active_voxels_per_s"] = round(nv / dt, 1)
    out["steps"], out["loss"] = steps, float(loss.item())
    return out


def secondary_configs(dev, budget_s=2.0, inputs=None):
    """BASELINE configs[1] and configs[4] on the driver's clock (N = 1, after the headline region, in a child process):
      configs[1]  forward-only feature extraction (eval mode) on 8 synthetic KITTI-shaped pairs (~18 k voxels per cloud), B pairs
                  per forward pass (scripts/test_kitti.py:141-152 runs one cloud per pass; forward_clouds gives bitwise-equal
                  features for any B) -> active voxels/s, each figure at most ``budget_s`` seconds of timed work;
      configs[4]  the packaged eval loop eval_pairs (2 x forward, find_corr with the 5000 x 5000 feature 1-NN, random_sample,
                  SC2-PCR, RTE / RRE meters; scripts/test_kitti.py:129-227) -> pairs/s on pairs that HAVE true
                  correspondences (synthetic.make_twin_eval_pair: with a random-init network unrelated views give none, and a
                  registration of pure outliers -- what rounds 1-5 timed, success 0 -- walks an empty compatibility matrix):
                  median of 5 repeats of >= 1 s each with the spread, the success rate and the MEASURED inlier share of the
                  putative correspondences next to it; the registration alone (Matcher.SC2_PCR, 8000 correspondences) at inlier
                  shares 0.05 / 0.3 / 0.6; the feature 1-NN kernel alone (events on the launch stream)."""
    import gcl_amd.MinkowskiEngine as ME  # noqa: F401
    from gcl_amd import synthetic
    from gcl_amd.lib.eval import find_corr
    from gcl_amd.lib.metrics import pdist_min
    from gcl_amd.model import load_model
    from gcl_amd.scripts.SC2_PCR import Matcher
    from gcl_amd.scripts.test_kitti import eval_pairs, forward_clouds, forward_clouds_stream
    torch.manual_seed(0)
    np.random.seed(0)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    model.eval()
    inputs = inputs or secondary_inputs()
    pairs, twins, TWIN_SHARE = inputs["pairs"], inputs["twins"], inputs["twin_share"]
    dpairs = [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in p.items()} for p in pairs]
    matcher = Matcher(inlier_threshold=0.6, num_node=8000, use_mutual=False, d_thre=0.1, num_iterations=20, ratio=0.2,
                      nms_radius=0.6, max_points=8000, k1=30, k2=20)
    out = {"pairs": len(pairs), "voxels_per_cloud": round(float(np.mean([len(p["sinput0_C"]) for p in pairs])), 1),
           "note": "synthetic KITTI-shaped pairs @0.3 m, random-init ResUNetBN2C-32 (eval mode, fp16x3); configs[1] figures <= "
                   f"{budget_s:.0f} s of timed work each; reference context: 7 pairs/s end to end with SC2-PCR on an RTX 3090 "
                   "(README.md:193, other hardware, real data)"}

    def timed(fn, units, budget=budget_s):
        fn()                                            # warm-up (maps of these clouds, allocator)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > budget or n >= 50:
                break
        return units * n / (time.perf_counter() - t0)

    def median_of(fn, units, repeats=5, budget=1.0):
        rates = sorted(timed(fn, units, budget) for _ in range(repeats))
        return {"median": round(rates[len(rates) // 2], 2), "min": round(rates[0], 2), "max": round(rates[-1], 2),
                "repeats": repeats, "seconds_per_repeat": budget}

    # as in the headline run: what exists so far leaves the cyclic collector's reach (a full collection over the pairs' arrays
    # inside a 1 s repeat is a 30 % outlier of that repeat)
    import gc
    gc.collect()
    gc.freeze()
    with torch.no_grad(), torch.cuda.device(dev):
        fwd = {}
        for B in (1, 8):
            def run(B=B):
                for c0 in range(0, 8, B):
                    forward_clouds(model, [(d[f"sinput{k}_F"], d[f"sinput{k}_C"]) for d in dpairs[c0:c0 + B] for k in (0, 1)])
            nv = sum(len(d["sinput0_C"]) + len(d["sinput1_C"]) for d in dpairs)
            fwd[f"pairs_per_forward={B}"] = round(timed(run, nv), 1)

        LOOP = 4       # the pipelined loops below run over 4 x 8 pairs per timed call (the reference's loop is over a dataset)

        def run_stream():      # the reference's loop shape (pair after pair, scripts/test_kitti.py:141-152), maps built ahead
            for _ in forward_clouds_stream(model, ([(d[f"sinput{k}_F"], d[f"sinput{k}_C"]) for k in (0, 1)]
                                                   for d in dpairs * LOOP), device=dev):
                pass
        fwd["pairs_per_forward=1, loop over pairs (forward_clouds_stream: maps built ahead on a side stream, passes on 3 streams)"] = \
            round(timed(run_stream, nv * LOOP), 1)
        out["configs[1] forward-only active voxels/s"] = fwd

        def corr_only():
            for c0 in range(0, 8, 8):
                feats = forward_clouds(model, [(d[f"sinput{k}_F"], d[f"sinput{k}_C"]) for d in dpairs for k in (0, 1)])
                for j, p in enumerate(pairs):
                    find_corr(p["pcd0"][0], p["pcd1"][0], feats[2 * j], feats[2 * j + 1], subsample_size=5000)
        loop = {"no registration (2 x fwd + find_corr), batch_pairs=8": round(timed(corr_only, len(pairs)), 2)}
        # what the registrations of this workload are given: the share of find_corr's 5000 matches per pair that are true
        # under T_gt (scripts/test_kitti.py:154-155, threshold = the matcher's inlier_threshold), one untimed pass
        probe = eval_pairs(model, twins, matcher, device=dev, batch_pairs=8, collect=True)
        share = float(np.mean([np.mean(np.asarray(d) < matcher.inlier_threshold) for d in probe["dists_nn"]]))
        loop["workload"] = (f"8 twin pairs (synthetic.make_twin_eval_pair: {TWIN_SHARE:.0%} of each cloud's voxels shared with "
                            f"the other cloud, {float(np.mean([len(p['sinput0_C']) for p in twins])):.0f} voxels per cloud), "
                            f"4 x 8 pairs per timed call")
        loop["measured inlier share of the putative correspondences"] = round(share, 4)
        for B in (1, 8):
            res = {}

            def run_eval(B=B, res=res):
                res["last"] = eval_pairs(model, twins * LOOP, matcher, device=dev, batch_pairs=B)
            rate = median_of(run_eval, len(twins) * LOOP)
            rate["success_rate"] = round(float(res["last"]["success_rate"]), 4)
            rate["rte_avg_m"] = round(float(res["last"]["rte_avg"]), 4)
            loop[f"with SC2-PCR, batch_pairs={B}"] = rate
        # the pure-outlier workload of rounds 1-5 (unrelated ray casts, success 0), kept for continuity with BENCH_r01..r05
        loop["with SC2-PCR, batch_pairs=8, ZERO-inlier pairs (rounds 1-5's workload, success 0)"] = round(
            timed(lambda: eval_pairs(model, pairs * LOOP, matcher, device=dev, batch_pairs=8), len(pairs) * LOOP, 1.0), 2)
        out["configs[4] eval_pairs pairs/s"] = loop
        reg = {}
        for sh in (0.05, 0.3, 0.6):      # tools/sc2pcr_profile.py's problem: 8000 correspondences, outliers uniform in the scene
            rng = np.random.RandomState(0)
            n = 8000
            src = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
            src[:, 2] *= 0.1
            ang = np.deg2rad(15.0)
            R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
            tgt = (src @ R.T + np.array([5.0, 1.0, 0.3]) + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
            bad = rng.rand(n) >= sh
            tgt[bad] = rng.uniform(-40, 40, (int(bad.sum()), 3)).astype(np.float32)
            s_, t_ = torch.from_numpy(src).to(dev)[None], torch.from_numpy(tgt).to(dev)[None]
            T = matcher.SC2_PCR(s_, t_)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                T = matcher.SC2_PCR(s_, t_)
            e1.record()
            torch.cuda.synchronize()
            ok = bool(np.abs(T[0, :3, :3].cpu().numpy() - R).max() < 5e-3)
            reg[f"inlier share {sh}"] = {"us": round(e0.elapsed_time(e1) / 20 * 1e3, 1), "recovered": ok}
        out["SC2-PCR registration alone (Matcher.SC2_PCR, 8000 correspondences) us per registration"] = reg
        nn = {}
        g = torch.Generator().manual_seed(0)
        for m in (1024, 5000):
            A = torch.nn.functional.normalize(torch.randn(m, 32, generator=g), dim=1).to(dev)
            Bm = torch.nn.functional.normalize(torch.randn(m, 32, generator=g), dim=1).to(dev)
            pdist_min(A, Bm, "SquareL2")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                pdist_min(A, Bm, "SquareL2")
            e1.record()
            torch.cuda.synchronize()
            nn[f"{m}x{m}x32"] = round(e0.elapsed_time(e1) / 20 * 1e3, 1)
        out["feature 1-NN (gcl_nn_rowmin) us per call"] = nn
    if inputs.get("raw_batches"):
        try:
            out["end_to_end from raw scans (configs[2] fed by the device loader)"] = end_to_end_from_scans(dev, inputs["raw_batches"])
        except Exception as e:      # a figure of its own: never takes the others down
            out["end_to_end from raw scans (configs[2] fed by the device loader)"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def plan_profile_records(plan, precision):
    """Per-launch records of the whole-network plan's profiled pass (events recorded by csrc/plan.hip on the launch
    stream around every convolution launch) in the tuple layout roofline_of reads, with the kernel instance each launch
    ran (same naming as rocprofv3's kernel trace)."""
    from gcl_amd import _lib
    from gcl_amd.MinkowskiEngine import ops
    lib = _lib.load()
    prec = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 4}[precision]
    out = []
    for kind, ms, pairs, cin, cout, n_in, n_out, K in plan.profile_records():
        cin, cout, K = int(cin), int(cout), int(K)
        if kind == 3:
            name = f"k_bwd_weight_rows<{cin // 32},{cout // 32}>"      # kernel_size 1: both operands streamed once
        elif kind == 2:
            if min(cin, cout) <= 4:
                name = "k_stem_bwd_weight"
            else:
                tile = f"{64 if cin % 64 == 0 else 32},{64 if cout % 64 == 0 else 32}"
                pl = cin >= ops.PRESPLIT_MIN_C and cout >= ops.PRESPLIT_MIN_C
                name = f"k_conv_bwd_weight_split<{tile},{prec},{'true' if pl else 'false'}>"
                if pl and cin % 128 == 0 and cout % 128 == 0 and os.environ.get("GCL_DW_WG128", "1") != "0":
                    name = "k_conv_bwd_weight_wg128"          # 128 x 128 block per workgroup, rows shared by its four waves
        else:
            nb = lib.gcl_conv_fwd_nb(int(n_out), cout, prec)
            pre = "true" if cin >= ops.PRESPLIT_MIN_C else "false"
            name = f"k_conv_fwd_split<{nb},{prec},{pre},{'true' if kind == 1 else 'false'}>"
            if prec == 4 and os.environ.get("GCL_FWD_DMA", "1") != "0" and \
                    (pre == "true" or os.environ.get("GCL_FWD_DMA_ROWS", "1") != "0"):           # LDS-DMA staging
                name = f"k_conv_fwd_dma<{nb},{pre},{'true' if kind == 1 else 'false'}>"
        out.append((name, ms, None, int(pairs), cin, cout, int(n_in), int(n_out), K))
    return out


def main():
    args = parse()
    if args.cpu_baseline_worker:
        print(json.dumps(cpu_baseline_worker()), flush=True)
        return
    if args.secondary_worker:
        torch.set_num_threads(max(1, min(16, usable_cores())))
        dev = torch.device("cuda:0")
        try:
            inputs = secondary_inputs()         # forked workers: before anything touches the GPU
            torch.cuda.set_device(dev)
            res = secondary_configs(dev, inputs=inputs)
        except Exception as e:
            res = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps(res), flush=True)
        return
    if args.gpus > 1 and "RANK" not in os.environ:
        # Invoked without a launcher (`python bench.py --gpus N`): start the N ranks ourselves.  Nothing in this process
        # has touched the GPU yet (importing torch and counting devices do not initialise HIP), and the launcher runs as
        # a CHILD process -- never an exec -- whose JSON line and exit code are forwarded.
        raise SystemExit(spawn_ranks(args))
    rank_env, world_env = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world_env:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world_env}: every GPU of the line must be a rank")
    # torch's CPU thread pool defaults to the HOST's core count; inside a CPU-quota'd container every small CPU op (the
    # eval loop's 3x3 algebra, index arithmetic) then pays an oversubscribed OpenMP barrier -- measured 34 ms per eval pair
    torch.set_num_threads(max(1, usable_cores() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))))
    # ---- synthetic batches of this rank (weak scaling: every rank gets its own bs=4 batches), made before the GPU is
    # touched (worker processes are forked) ------------------------------------------------------------------------------
    t_gen = time.perf_counter()
    batches = make_batches(rank_env, max(1, args.batches), args.batch_size, args.group_mode)
    log(f"rank {rank_env}: {len(batches)} batches generated in {time.perf_counter() - t_gen:.1f} s: "
        f"{[len(b['sinput_C']) for b in batches]} voxels")

    from gcl_amd import ddp
    # test hooks for a 1-GPU box (never set by the driver): run the N>1 code path with every rank on cuda:0 and gloo
    if os.environ.get("GCL_BENCH_SINGLE_DEVICE") == "1":
        rank, world, local = ddp.init_from_env(backend="gloo")
        local = 0
    else:
        rank, world, local = ddp.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the process group has {world} rank(s)")
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    import torch.distributed as dist
    from gcl_amd.lib.colocation_trainer import FinestContrastiveLossTrainer, make_config, prefetch_to_device
    from gcl_amd.MinkowskiEngine import ops

    torch.manual_seed(0)
    np.random.seed(rank)
    keys = ("sinput_C", "sinput_F", "group", "index", "finest_flag")
    host = []
    for b in batches:       # pinned host memory: the H2D copies of the timed region are asynchronous DMA
        hb = {k: (v.pin_memory() if isinstance(v, torch.Tensor) else v) for k, v in b.items() if k in keys}
        host.append(hb)
    h2d_bytes = sum(v.numel() * v.element_size() for v in host[0].values() if isinstance(v, torch.Tensor))
    if args.resident:
        host = [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in hb.items()} for hb in host]
    cfg = make_config(batch_size=args.batch_size)
    trainer = FinestContrastiveLossTrainer(cfg, device=dev, ddp=ddp.FlatDDP() if world > 1 else None)
    # --dump-outputs: the seeded initial state, put back before the last timed step (see the loop)
    state0 = ({k: v.detach().clone() for k, v in trainer.model.state_dict().items()} if args.dump_outputs else None)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def feed(n, start=0):
        seq = (host[(start + i) % len(host)] for i in range(n))
        return seq if args.resident else prefetch_to_device(seq, dev, keys)

    # Setup, not a step: everything built so far (modules, batches, the imported libraries' objects) is moved out of the
    # cyclic garbage collector's reach.  Otherwise the interpreter's first full collection lands ~58 steps into the run
    # and, on a box whose image is still being paged in, takes 75 - 120 ms walking objects it has never touched
    # (measured per step with GCL_BENCH_STEP_TIMES=1: one 74.6 / 117.6 ms step among 15.8 ms ones; 21.1 vs 16.2 ms per
    # step for --steps 20 --warmup 5 on a fresh box).  Young objects are still collected as usual.
    import gc
    gc.collect()
    gc.freeze()
    # ONE epoch loop over warm-up + timed steps (the trainer's helpers stay one or two steps ahead across the boundary,
    # as they are anywhere else in an epoch); the timed region is bracketed by barrier + synchronize on both sides
    # the helpers work GCL_PREFETCH_DEPTH steps ahead: feed that many batches beyond the timed region, so that its last steps
    # still submit H2D / map / draw work for successors like every step of a long epoch does (the clock stops after
    # `steps`; the surplus batches are never trained on)
    depth = max(1, int(os.environ.get("GCL_PREFETCH_DEPTH", "2")))
    steps = trainer.train_steps(feed(args.warmup + args.steps + depth))
    for _ in range(args.warmup):
        loss, _, _ = next(steps)
    sync()
    log("warmup done")
    t0, c0 = time.perf_counter(), time.thread_time()
    # the trainer's epoch loop: the H2D copy of every batch and all K x 3 np.random draws happen inside the timed region
    # (copy stream / helper thread, one step ahead).  Per-launch events (roofline) are recorded during the LAST timed
    # step only: recording ~300 events per step costs ~3 ms of host time, which would otherwise perturb every step
    n_vox = 0
    step_trace = os.environ.get("GCL_BENCH_STEP_TIMES") == "1"     # diagnostic: per-step GPU interval and host time
    step_events, step_host, step_mem = [], [], []
    kernel_events = args.full and not args.no_kernel_events          # roofline: a --full figure
    for it in range(args.steps):
        if it == args.steps - 1 and state0 is not None:
            # --dump-outputs: the loss backward's float atomics differ in the last bit from run to run and training
            # amplifies that over the steps, so the last step starts from the seeded initial parameters, BatchNorm
            # statistics and optimizer state (momentum buffers rebuilt by the step, as in a first step): its outputs then
            # depend on its batch and draws alone.  The steps already queued finish on the clock; it is stopped only while
            # the state is put back (the drain costs the last step its overlap with the previous one: ~1 % on ms_per_step)
            sync()
            p0, pc0 = time.perf_counter(), time.thread_time()
            with torch.no_grad():
                trainer.model.load_state_dict(state0)       # in place: version bumps void the packed-weight caches
            trainer.optimizer.state.clear()
            sync()
            t0, c0 = t0 + time.perf_counter() - p0, c0 + time.thread_time() - pc0
        if it == args.steps - 1 and kernel_events:
            ops.PROFILE = []
            plan = getattr(trainer.model, "_plan", None)
            if hasattr(plan, "profile_next"):       # the whole-network plan times its own launches (events in C)
                plan.profile_next = True
        loss, parts, n = next(steps)
        n_vox += n
        if step_trace:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            step_events.append(e)
            step_host.append(time.perf_counter())
            step_mem.append(torch.cuda.memory_stats().get("num_device_alloc", 0))
        if os.environ.get("GCL_BENCH_TRACE_LOSS") == "1":      # diagnostic (adds a host sync per step)
            log(f"step {it}: loss {loss.item():.6f} parts {[round(p.item(), 5) for p in parts]}")
    t_enqueue, t_cpu = time.perf_counter() - t0, time.thread_time() - c0
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0
    sync()
    dt = time.perf_counter() - t0
    steps.close()                      # drops the look-ahead batches (outside the timed region)
    if step_trace:
        gpu = [step_events[i].elapsed_time(step_events[i + 1]) for i in range(len(step_events) - 1)]
        host = [(step_host[i + 1] - step_host[i]) * 1e3 for i in range(len(step_host) - 1)]
        for i0 in range(0, len(gpu), 10):
            log(f"steps {i0:3d}..: gpu ms " + " ".join(f"{v:5.1f}" for v in gpu[i0:i0 + 10]) + "  | host ms " +
                " ".join(f"{v:5.1f}" for v in host[i0:i0 + 10]) + "  | device allocations so far " +
                " ".join(str(v) for v in step_mem[i0:i0 + 10]))
    log(f"timed region done: {dt / args.steps * 1e3:.2f} ms/step (host finished enqueuing after "
        f"{t_enqueue / args.steps * 1e3:.2f} ms/step, of which the enqueuing thread was on a CPU for "
        f"{t_cpu / args.steps * 1e3:.2f} ms/step: the rest is waiting for the GPU through its helpers)")
    prof, ops.PROFILE = ops.PROFILE, None
    plan = getattr(trainer.model, "_plan", None)
    plan_used = hasattr(plan, "profile_records")
    if plan_used and not prof and kernel_events:
        prof = plan_profile_records(plan, ops.PRECISION)
    if args.dump_outputs and rank == 0:
        torch.cuda.synchronize()
        dump_outputs(args.dump_outputs, loss, parts, n, trainer.model)
    for name, (w, c, k) in getattr(trainer, "_helper_times", {}).items():
        if k:
            log(f"helper thread '{name}': {w / k * 1e3:.2f} ms wall, {c / k * 1e3:.2f} ms CPU per step ({k} steps)")
    ranks = None
    if world > 1:
        stats = torch.tensor([dt, float(n_vox), dt_local], dtype=torch.float64,
                             device=dev if dist.get_backend() == "nccl" else "cpu")
        allst = [torch.zeros_like(stats) for _ in range(world)]
        dist.all_gather(allst, stats)
        allst = torch.stack(allst).cpu()
        dt, total_vox = float(allst[:, 0].max()), float(allst[:, 1].sum())
        ranks = {"backend": dist.get_backend(), "rccl_ranks": world,
                 "voxels_per_step_per_rank": [round(v / args.steps, 1) for v in allst[:, 1].tolist()],
                 "ms_per_step_per_rank_before_barrier": [round(v / args.steps * 1e3, 3) for v in allst[:, 2].tolist()],
                 "straggler_max_over_mean": round(float(allst[:, 2].max() / allst[:, 2].mean()), 4)}
    else:
        total_vox = float(n_vox)
    if not torch.isfinite(loss).item():
        raise SystemExit("non-finite loss in the benchmark")

    if rank != 0:
        if world > 1:
            dist.barrier()
        return

    aux = set()
    if plan_used and getattr(plan, "_aux", None) is not None:
        aux = {r[0] for r in (prof or []) if r[0].startswith(("k_conv_bwd_weight", "k_stem_bwd_weight", "k_bwd_weight_rows"))}
    roofline = roofline_of(prof, ops.PRECISION, aux, ms_per_step=dt / args.steps * 1e3) if prof else None
    out = {
        "metric": "active voxels/sec thru ResUNetBN2C fwd+bwd+GCL loss, KITTI 0.3m",
        "value": round(total_vox / dt, 1), "unit": "active voxels/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if ops.PRECISION != "bf16x3" else "f32 via bf16x3 split (reduced: ~1.5e-5)",
        "arithmetic": ops.PRECISION, "data": "synthetic", "full": args.full,
        "config": {"workload": "configs[2]: GCL training step (finest_contrastive_loss), ResUNetBN2C-32 conv1 k=5, "
                               f"KITTI-shaped ray-cast clouds @0.3 m, bs={args.batch_size} x 7 clouds per GPU, "
                               f"positive groups '{args.group_mode}'",
                   "timed_region": ("inputs resident in HBM (diagnostic)" if args.resident else
                                    f"H2D of every batch inside the step (pinned, copy stream, {h2d_bytes / 1e6:.1f} MB "
                                    f"per batch), {len(host)} distinct batches in rotation"),
                   "voxels_per_batch_rank0": [len(b["sinput_C"]) for b in batches],
                   "global_batch": args.batch_size * world, "parallelism": f"dp{world}", "loss": float(loss.item()),
                   "host_enqueue_ms_per_step": round(t_enqueue / args.steps * 1e3, 3),
                   "host_cpu_ms_per_step_enqueuing_thread": round(t_cpu / args.steps * 1e3, 3),
                   "step_runtime": "native plan (gcl_maps_build + gcl_plan_forward/backward)" if plan_used
                                   else "per-operator launches from Python"},
        "roofline": roofline,
    }
    if ranks is not None:
        want = "gloo" if os.environ.get("GCL_BENCH_SINGLE_DEVICE") == "1" else "nccl"
        if ranks["rccl_ranks"] != args.gpus or ranks["backend"] != want:
            raise SystemExit(f"--gpus {args.gpus}: the collective ran on {ranks['rccl_ranks']} rank(s) over "
                             f"'{ranks['backend']}' (expected {args.gpus} over '{want}')")
        out["ranks"] = ranks
    if args.full and world == 1 and not args.no_secondary:
        out["secondary"] = secondary_in_child()
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()


if __name__ == "__main__":
    main()
