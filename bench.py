#!/usr/bin/env python3
"""bench.py -- headline benchmark: 3D hex BwdTrans sum-factorisation, fp64, nq = 8, on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path (one sf_bwdtrans_hex_f64 launch) over this rank's batch of
elements, inputs resident in HBM.  The element batch is embarrassingly parallel: ranks own disjoint
element ranges, there is NO data-path collective; torch.distributed (RCCL) carries only the barrier,
the MAX of the elapsed time, the SUM of the result checksum and the count of ranks.

Launching.  One process per GPU.  Under a launcher (WORLD_SIZE set) `--gpus` must equal WORLD_SIZE or
the run exits non-zero.  Without a launcher, `--gpus N` with N > 1 starts the N ranks itself
(`python -m torch.distributed.run` as a child process, before this process makes any GPU call) and
exits with the child's code; it refuses when the box has fewer than N GPUs.  `n_gpus` in the JSON line
is the number of ranks the collectives actually reduced over, never the flag.

Workload.  N = 1: 1 048 576 elements (BASELINE configs[2], the config the metric's target is quoted
on).  N > 1: BASELINE configs[4], a 10 000 000-element batch sharded over the ranks ("strong"); with
`--full` rank 0 then times the SAME batch alone on its GPU (it fits: 68 GB) for `speedup_vs_1gpu_same_batch`.
`--elements-per-gpu` selects weak scaling instead.

Metric (BASELINE.json): GDOF/s = 1e-9 * nelmt * nm^3 / t   (benchmark05/benchmark05.cc:1408; DOF =
input modes).  Roofline: HBM, algorithmic bytes 8*(nm^3 + nq^3) per element.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps, writes its outputs
(`--dump-outputs`) and prints the line: the headline keys, "roofline" and "checksum_norm".  `--full` adds
what takes runs of its own, after the timed region: "cpu_baseline" (oracle port timed on the host's cores
by rank 0, every N), the graph-replayed group timings and the golden-norm check (N=1), "extra" (nq sweep
2..10 and the 2D quad orders, N=1 only; `--no-extra` drops it) and the single-GPU run of the same batch
(N>1, strong).  One protocol per number: `value` / `ms_per_step` / `roofline.frac` = mean of the timed
steps by wall clock; `roofline.kernel_ms` = the same launches between HIP events; `ms_min_of_40` and every
`*_min` = the fastest of 40 graph-replayed groups; `frac` / `*_mean` in the sweeps = the mean over them.

`--dump-outputs DIR` writes, after the timed steps, what the last step computed on rank 0: `DIR/hex_out.npy`,
float64, shape (S, nq^3) = the output rows of S elements of rank 0's batch ([k][j][i] within a row), and
`DIR/hex_out_elements.npy`, float64, the element indices of those rows.  S covers the whole batch when it fits
DUMP_BYTES, else the first and last DUMP_EDGE elements plus a fixed seeded sample of the rest.  Inputs are
seeded, so the same arguments give the same inputs in every run.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X datasheet HBM3E peak (/opt/skills/guides/MI355X_MICROARCH.md)
NQ = 8
GOLDEN_NORM_1M = 17134.76235  # benchmark05/nq8x8x8.log:45 (nelmt 1 048 576, sin/cos data)
CONFIG4_ELEMENTS = 10_000_000  # BASELINE.json configs[4]
QUAD_ORDERS = (2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 26, 28, 30, 32)  # benchmark04/run.sh:5-6 + 20 / 24 / 26 / 28 / 30
DUMP_BYTES = 32 << 20   # --dump-outputs: at most this many bytes of output rows
DUMP_EDGE = 512         # elements always dumped at each end of the batch (chunk / dispatch seams)
DUMP_SEED = 20260401    # seeds the sample of the interior elements


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="number of ranks = GPUs (default: WORLD_SIZE under a launcher, else 1)")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--elements-per-gpu", type=int, default=0,
                    help="weak scaling: elements owned by each rank (N = 1 default: 1 048 576)")
    ap.add_argument("--total-elements", type=int, default=0,
                    help="strong scaling: shard this many elements over the ranks "
                         "(N > 1 default: 10 000 000 = BASELINE config 4)")
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baseline, the order sweeps, the group timings, the golden-norm check "
                         "and (N > 1) the single-GPU run of the same batch")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the order sweeps")
    ap.add_argument("--no-single-gpu-reference", action="store_true",
                    help="with --full, N > 1, strong scaling: skip rank 0's solo run of the same batch")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    return ap.parse_args(argv)


def dump_elements(nelmt, nq):
    """Element indices (sorted, unique) whose output rows --dump-outputs writes: all of them when they fit
    DUMP_BYTES, else the first and last DUMP_EDGE plus a sample of the rest drawn with DUMP_SEED."""
    import numpy as np
    cap = max(1, DUMP_BYTES // (8 * nq ** 3))
    if nelmt <= cap:
        return np.arange(nelmt, dtype=np.int64)
    edge = min(DUMP_EDGE, cap // 4)
    rng = np.random.default_rng(DUMP_SEED)
    mid = edge + rng.choice(nelmt - 2 * edge, size=cap - 2 * edge, replace=False)
    return np.unique(np.concatenate([np.arange(edge), mid, np.arange(nelmt - edge, nelmt)])).astype(np.int64)


def dump_outputs(path, out, nelmt, nq, torch):
    """Rows of the output buffer (this rank's batch, as the last step left it) -> path/hex_out.npy and the
    element index of every row -> path/hex_out_elements.npy."""
    import numpy as np
    idx = dump_elements(nelmt, nq)
    rows = out.view(nelmt, nq ** 3).index_select(0, torch.from_numpy(idx).to(out.device))
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "hex_out.npy"), rows.cpu().numpy().astype(np.float64))
    np.save(os.path.join(path, "hex_out_elements.npy"), idx.astype(np.float64))


def resolve_world(args, environ):
    """(world, must_spawn).  Raises SystemExit when --gpus contradicts the launcher."""
    env_world = environ.get("WORLD_SIZE")
    if env_world is None:
        n = 1 if args.gpus is None else args.gpus
        if n < 1:
            raise SystemExit(f"bench.py: --gpus {n} is not a rank count")
        return n, n > 1
    world = int(env_world)
    if args.gpus is not None and args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; "
                         "refusing to report a number for a different GPU count")
    return world, False


def pick_workload(args, world):
    """(scaling, total elements, elements per rank or None)."""
    if args.total_elements > 0 and args.elements_per_gpu > 0:
        raise SystemExit("bench.py: give --total-elements or --elements-per-gpu, not both")
    if args.total_elements > 0:
        return "strong", args.total_elements, None
    if args.elements_per_gpu > 0:
        return "weak", world * args.elements_per_gpu, args.elements_per_gpu
    if world == 1:
        return "weak", 1 << 20, 1 << 20
    return "strong", CONFIG4_ELEMENTS, None


KFD_NODES = "/sys/class/kfd/kfd/topology/nodes"


def visible_gpu_count(environ=None, nodes_dir=KFD_NODES):
    """GPUs this process would see, counted WITHOUT a HIP / HSA call: KFD topology nodes with simd_count > 0
    (CPU nodes report 0), narrowed by ROCR_VISIBLE_DEVICES and then HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES
    the way the runtime applies them (a list of indices or GPU-<uuid> names; parsing stops at the first entry that
    names no device).  None when the topology is not readable (not a ROCm box, or sysfs hidden)."""
    environ = os.environ if environ is None else environ
    try:
        names = sorted(os.listdir(nodes_dir), key=lambda v: int(v) if v.isdigit() else 1 << 30)
    except OSError:
        return None
    gpus = []
    for name in names:
        props = {}
        try:
            with open(os.path.join(nodes_dir, name, "properties")) as fh:
                for line in fh:
                    key, _, val = line.strip().partition(" ")
                    props[key] = val.strip()
        except OSError:
            continue
        if int(props.get("simd_count", "0") or 0) > 0:
            gpus.append(props.get("unique_id", ""))
    count = len(gpus)
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        if var == "CUDA_VISIBLE_DEVICES" and "HIP_VISIBLE_DEVICES" in environ:
            continue
        if var not in environ:
            continue
        kept = 0
        for item in environ[var].split(","):
            item = item.strip()
            if item.isdigit() and int(item) < count:
                kept += 1
            elif item.upper().startswith("GPU-") and var == "ROCR_VISIBLE_DEVICES":
                kept += 1
            else:
                break
        count = kept
    return count


def gpu_handles_open():
    """Device files of the GPU driver this process holds open (/dev/kfd, /dev/dri/renderD*): non-empty once a
    HIP / HSA call has initialised the runtime."""
    held = []
    try:
        for fd in os.listdir("/proc/self/fd"):
            try:
                target = os.readlink(os.path.join("/proc/self/fd", fd))
            except OSError:
                continue
            if target == "/dev/kfd" or target.startswith("/dev/dri/"):
                held.append(target)
    except OSError:
        pass
    return held


def spawn_ranks(n, argv, call=subprocess.call):
    """No launcher: start the N ranks as a child `torch.distributed.run`.  This process makes no GPU call and does
    not import torch: the GPUs are counted from the KFD topology in sysfs, and the spawn is refused if the process
    nevertheless holds the GPU driver's device files (a child started from an initialised parent is what this pool
    forbids)."""
    backend = os.environ.get("SF_BENCH_BACKEND", "nccl")
    have = visible_gpu_count()
    if backend == "nccl" and have is not None and have < n:
        raise SystemExit(f"bench.py: --gpus {n} but this box has {have} GPU(s); one rank per GPU "
                         "(set SF_BENCH_BACKEND=gloo to rehearse with ranks sharing a GPU)")
    held = gpu_handles_open()
    if held:
        raise SystemExit(f"bench.py: refusing to start ranks from a process that has initialised the GPU ({held[0]} is open)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    passed = [a for a in argv]
    if not any(a == "--gpus" or a.startswith("--gpus=") for a in passed):
        passed += ["--gpus", str(n)]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return call(cmd + passed, env=env)


def time_steps(fn, steps, warmup, torch, dist, use_dist):
    """W untimed steps, then exactly K timed steps bracketed by barrier + synchronize.
    Returns (wall seconds of this rank, HIP-event seconds on the launch stream)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return t1 - t0, ev0.elapsed_time(ev1) * 1e-3


def cpu_baseline(nq, seconds):
    """Oracle (-O3/AVX2/FMA build, OpenMP over elements, register-blocked sweeps) on the full 1 Mi-element
    batch of the headline config, bounded by `seconds` of CPU work."""
    import oracle
    nm = nq - 1
    sample = 1 << 20
    cores = oracle.usable_cpus()      # not omp_get_max_threads(): the box grants a CPU share
    builds = [True] + (["avx512"] if oracle.host_has_avx512() else [])
    for fast in [False] + builds:
        oracle.set_threads(cores, fast=fast)
    b = oracle.fill_basis(nm, nq)
    x = oracle.fill_random(sample * nm ** 3, 0x5F3759DF)
    form = "blocked" if oracle.has_blocked(nq) else "vector"
    import numpy as np
    out = np.zeros(sample * nq ** 3)   # allocated and touched once, as the device buffers are: no page faults in the timing

    def one_pass(fast):
        t0 = time.perf_counter()
        oracle.bwdtrans_hex((nq,) * 3, sample, b, b, b, x, form=form, fast=fast, out=out)
        return time.perf_counter() - t0

    # two passes of every vector width the host lists, then the rest of the budget on the faster build
    trial = {fast: min(one_pass(fast), one_pass(fast)) for fast in builds}
    fast = min(trial, key=trial.get)
    best, spent, reps = trial[fast], 2.0 * sum(trial.values()), 2
    while spent < seconds and reps < 200:
        dt = one_pass(fast)
        best = min(best, dt)
        spent += dt
        reps += 1
    flops = 2.0 * (nq * nm ** 3 + nq ** 2 * nm ** 2 + nq ** 3 * nm) * sample / best
    flags = "-O3 -mavx512f -mprefer-vector-width=512 -mfma" if fast == "avx512" else "-O3 -mavx2 -mfma"
    width = "AVX-512 (8-wide)" if fast == "avx512" else "AVX2 (4-wide)"
    return {"value": round(1e-9 * sample * nm ** 3 / best, 4), "unit": "GDOF/s",
            "cores": oracle.max_threads(fast=fast), "kind": "port",
            "gflop_s": round(flops * 1e-9, 1),
            "builds_tried_gdof_s": {("avx512" if k == "avx512" else "avx2"): round(1e-9 * sample * nm ** 3 / v, 4)
                                    for k, v in trial.items()},
            "sample": f"hex nq={nq}, {sample} elements (the full headline batch), seeded random data, min of "
                      f"{reps} passes ({spent:.1f} s of CPU work), oracle/bwdtrans_ref.c "
                      f"oracle_bwdtrans_hex_{form} (3-sweep form, "
                      f"{'register-blocked ' + width + ' i-vectors' if form == 'blocked' else 'CPU loop order'}), "
                      f"{flags}, OpenMP over elements, {cores} threads granted, output buffer allocated once"}


def _store(dist):
    try:
        return dist.distributed_c10d._get_default_store()
    except Exception:
        return None


def wait_for_rank0(dist, key):
    """Block (on the rendezvous store's socket, not spinning in a collective) until rank 0 has set `key`; without
    a store the caller's barrier does the waiting."""
    import datetime
    store = _store(dist)
    if store is not None:
        try:
            store.wait([key], datetime.timedelta(minutes=30))
        except Exception:
            pass


def release_ranks(dist, key):
    store = _store(dist)
    if store is not None:
        try:
            store.set(key, "1")
        except Exception:
            pass


def single_gpu_reference(sf, torch, dev, nq, total, steps):
    """Rank 0 alone over the whole strong-scaling batch (fits one 288 GB GPU): GDOF/s, or None."""
    nm = nq - 1
    need = 8 * total * (nm ** 3 + nq ** 3)
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.92 * free:
        return None
    b = sf.fill_basis(nm, nq, dev)
    x = sf.fill_random(total * nm ** 3, 0x5F3759DF, 0, dev)
    out = torch.empty(total * nq ** 3, dtype=torch.float64, device=dev)
    for _ in range(2):
        sf.bwdtrans_hex((nq,) * 3, b, b, b, x, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sf.bwdtrans_hex((nq,) * 3, b, b, b, x, out=out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del x, out
    torch.cuda.empty_cache()
    return 1e-9 * total * nm ** 3 * steps / dt


def main():
    args = parse()
    world, must_spawn = resolve_world(args, os.environ)
    if must_spawn:
        sys.exit(spawn_ranks(world, sys.argv[1:]))

    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback for the product path)")
    # one process per GPU; SF_BENCH_BACKEND=gloo (rehearsal: several ranks may then share a GPU,
    # the scalar reductions go through CPU tensors) -- default nccl = RCCL over xGMI
    backend = os.environ.get("SF_BENCH_BACKEND", "nccl")
    ndev = max(1, torch.cuda.device_count())
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} ranks but {ndev} GPU(s): one rank per GPU")
    local = local % ndev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rdev = dev if backend == "nccl" else torch.device("cpu")   # where the reduced scalars live
    # SF_BENCH_FORCE_DIST=1 (under a launcher): run the collectives even with ONE rank -- exercises the RCCL
    # communicator, barrier, all-reduces and all-gather on a one-GPU box
    use_dist = world > 1 or (os.environ.get("SF_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    sf = ge.load_package()
    from gpu_benchmarking_amd import shard

    nq, nm = args.nq, args.nq - 1
    scaling, total, per_gpu = pick_workload(args, world)
    if per_gpu is None:
        lo, hi = shard.element_range(total, world, rank)
    else:
        lo, hi = rank * per_gpu, (rank + 1) * per_gpu
    nelmt = hi - lo

    b = sf.fill_basis(nm, nq, dev)
    # seeded, per-value-distinct data; the global element index seeds the stream so every rank
    # generates exactly its shard of the one global array
    x = sf.fill_random(nelmt * nm ** 3, 0x5F3759DF, lo * nm ** 3, dev)
    out = torch.empty(nelmt * nq ** 3, dtype=torch.float64, device=dev)

    def step():
        sf.bwdtrans_hex((nq,) * 3, b, b, b, x, out=out)

    wall, evs = time_steps(step, args.steps, args.warmup, torch, dist, use_dist)
    tmax = torch.tensor([wall, evs], dtype=torch.float64, device=rdev)
    # checksum, rank count and element count all come out of the same SUM all-reduce
    sums = torch.tensor([sf.sumsq(out), 1.0, float(nelmt)], dtype=torch.float64, device=rdev)
    mine = torch.tensor([float(nelmt), evs, wall], dtype=torch.float64, device=rdev)
    per_rank = [torch.zeros_like(mine) for _ in range(world)]
    if use_dist:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        dist.all_gather(per_rank, mine)
    else:
        per_rank = [mine]
    wall_max = float(tmax[0])
    ranks_reduced, elements_reduced = int(round(float(sums[1]))), int(round(float(sums[2])))
    if ranks_reduced != world or elements_reduced != total:
        raise SystemExit(f"bench.py: collectives reduced over {ranks_reduced} ranks / {elements_reduced} "
                         f"elements, expected {world} / {total}")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, nelmt, nq, torch)
    result = None
    bytes_per_elmt = 8 * (nm ** 3 + nq ** 3)
    if rank == 0:
        dof = total * nm ** 3
        # per GPU, kernel level: algorithmic bytes of ITS launch / ITS average launch duration (HIP events on the
        # launch stream)
        per_gpu_gbs = [float(p[0]) * bytes_per_elmt / (float(p[1]) / args.steps) * 1e-9 for p in per_rank]
        slowest = min(range(world), key=lambda r: per_gpu_gbs[r])
        kernel_s = float(per_rank[slowest][1]) / args.steps
        # the line's roofline figure follows from the driver-checkable ms_per_step (wall clock, MAX over ranks,
        # launch overhead and barriers included): one GPU's algorithmic bytes per step / that time
        achieved = float(per_rank[slowest][0]) * bytes_per_elmt / (wall_max / args.steps) * 1e-9
        traffic = shard.recorded_traffic(ROOT, 3, nq, int(per_rank[slowest][0]))
        result = {
            "metric": "GDOF/s for 3D hex sum-factorisation, fp64, nq=2..10 sweep",
            "metric_detail": f"value = the nq={nq} order (the one north_star's target is quoted on); the "
                             "per-order sweep 2..10 is in extra.hex_sweep, its min / geomean in roofline "
                             "(bench.py --full)",
            "value": round(1e-9 * dof * args.steps / wall_max, 3),
            "unit": "GDOF/s",
            "n_gpus": ranks_reduced, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * wall_max / args.steps, 5),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"benchmark05 3D hex BwdTrans nq={nq}x{nq}x{nq}, "
                                   f"{total} elements over {world} GPU(s) ({nelmt} on rank 0), fp64, "
                                   f"seeded random modes, cos basis"
                                   + (" [BASELINE configs[4]]" if total == CONFIG4_ELEMENTS and world > 1 else ""),
                       "nq": nq, "elements_per_gpu": nelmt, "total_elements": total,
                       "parallelism": f"element-range sharding x{world}, no data-path collective",
                       "backend": "rccl" if backend == "nccl" else backend},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": traffic["bytes"] if traffic else None,
                         "traffic_source": traffic["source"] if traffic else
                         "not recorded for this shape (PMC passes are separate rocprofv3 runs, profiles/README.md)",
                         "traffic_over_algorithmic": traffic["over_algorithmic"] if traffic else None,
                         "frac_protocol": "achieved = one GPU's algorithmic bytes per step / ms_per_step (mean of the "
                                          "timed steps, host wall clock, MAX over ranks); kernel_ms / frac_kernel_events "
                                          "= the same bytes / the mean launch duration between HIP events on the launch "
                                          "stream (what rocprofv3's AverageNs measures)",
                         "kernel": "sf::hex_wave_kernel", "bytes_per_element": bytes_per_elmt,
                         "kernel_ms": round(kernel_s * 1e3, 5),
                         "frac_kernel_events": round(per_gpu_gbs[slowest] / HBM_PEAK_GBS, 4),
                         # one step = one library call; a batch above 1 Mi elements is enqueued as several dispatches
                         "dispatches_per_step": shard.hex_dispatches_per_call(nq, int(per_rank[slowest][0]))},
            "checksum_norm": math.sqrt(float(sums[0])),
        }
        if world > 1:
            result["roofline"]["per_gpu_frac"] = [round(g / HBM_PEAK_GBS, 4) for g in per_gpu_gbs]
            result["roofline"]["per_gpu_wall_ms_per_step"] = [round(1e3 * float(p[2]) / args.steps, 5) for p in per_rank]
            result["roofline"]["note"] = ("per_gpu_frac: each GPU's own launches between HIP events; achieved / frac: "
                                          "the slowest GPU's bytes over the job's ms_per_step")
            if backend != "nccl":
                result["rehearsal"] = f"backend {backend}: ranks may share a GPU; not a scaling measurement"

    if args.full and world > 1 and scaling == "strong" and not args.no_single_gpu_reference:
        # rank 0 alone over the same batch, the others wait (asleep on the rendezvous store, then at the barrier)
        if rank != 0:
            wait_for_rank0(dist, "solo_done")
        if rank == 0:
            del x, out
            x = out = None
            solo = single_gpu_reference(sf, torch, dev, nq, total, max(2, min(args.steps, 10)))
            if solo:
                result["single_gpu_same_batch_gdof_s"] = round(solo, 3)
                result["speedup_vs_1gpu_same_batch"] = round(result["value"] / solo, 3)
            release_ranks(dist, "solo_done")
        dist.barrier()

    if args.full and rank == 0 and world == 1:
        # the same launches under the sweep's protocol (groups of 8 replayed from a HIP graph, HIP events):
        # mean and minimum over 40 groups next to the eager wall-clock mean that `value` is
        mean_ms, min_ms, _ = grouped_ms(torch, step)
        result["ms_mean_of_40_groups"] = round(mean_ms, 5)
        result["ms_min_of_40"] = round(min_ms, 5)
        # parity sanity on the reference's own data: golden norm of benchmark05/nq8x8x8.log:45
        if nq == 8:
            xs = sf.fill_sincos(1 << 20, nm ** 3, dev)
            os_ = sf.bwdtrans_hex((nq,) * 3, b, b, b, xs)
            norm = math.sqrt(sf.sumsq(os_))
            result["golden_norm_check"] = {"got": norm, "reference": GOLDEN_NORM_1M,
                                           "ok": abs(norm - GOLDEN_NORM_1M) <= 5.5e-10 * norm}
            del xs, os_
        del x, out
        x = out = None
        if not args.no_extra:
            result["extra"] = extras(sf, torch, dev, shard)
            fr = [v["frac_mean"] for v in result["extra"]["hex_sweep"].values()]
            worst = min(result["extra"]["hex_sweep"].items(), key=lambda kv: kv[1]["frac_mean"])
            result["roofline"]["sweep_min"] = round(min(fr), 4)
            result["roofline"]["sweep_min_nq"] = int(worst[0])
            result["roofline"]["sweep_geomean"] = round(math.exp(sum(math.log(f) for f in fr) / len(fr)), 4)
            result["roofline"]["sweep_protocol"] = "from frac_mean of extra.hex_sweep (mean over 40 graph-replayed groups)"
            # second denominator: the device's own measured stream rate (benchmark02's x += y,
            # 24 B/element), next to the 8 TB/s datasheet figure
            stream = measured_stream_gbs(sf, torch, dev)
            result["roofline"]["measured_stream_gb_s"] = round(stream, 1)
            result["roofline"]["frac_of_measured_stream"] = round(
                result["roofline"]["achieved"] / stream, 4)
    if args.full and not args.no_cpu_baseline:
        # the oracle on this box's host cores, in the same run (north_star), AFTER the timed region; for N > 1 the
        # other ranks wait at the barrier as they do for rank 0's solo run
        if use_dist and rank != 0:
            wait_for_rank0(dist, "cpu_done")   # asleep on a socket: the host cores belong to rank 0's OpenMP team
        if rank == 0:
            del x, out
            result["cpu_baseline"] = cpu_baseline(nq, args.cpu_seconds)
            result["vs_reference_published"] = {
                "value": round(result["value"] / 26.389, 2),
                "note": "reference's best variant, 26.389 GDOF/s on an unstated NVIDIA GPU "
                        "(benchmark05/nq8x8x8.log:46); not an MI355X number, so vs_baseline is null"}
            if use_dist:
                release_ranks(dist, "cpu_done")
        if use_dist:
            dist.barrier()
    if rank == 0:
        if use_dist:
            result["config"]["collectives"] = f"{backend} communicator of {dist.get_world_size()} rank(s)"
        print(json.dumps(result), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def measured_stream_gbs(sf, torch, dev, n=1 << 28, reps=10):
    """benchmark02 on this device: x += y over 2 x 2 GiB, best of `reps` (HIP events)."""
    x, y = sf.fill_vecadd(n, dev)
    sf.vector_add(x, y)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sf.vector_add(x, y)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return 24.0 * n / best * 1e-6


def traffic_ratio(shard, dim, nq, nelmt):
    """Measured HBM bytes / algorithmic bytes of this shape from the committed PMC passes (None: not recorded, or
    recorded on other kernel sources)."""
    rec = shard.recorded_traffic(ROOT, dim, nq, nelmt)
    return rec["over_algorithmic"] if rec and "STALE" not in rec["source"] else None


def grouped_ms(torch, fn, reps=40, inner=8):
    """(mean, min, replayed) milliseconds per launch over `reps` groups of `inner` back-to-back launches, each
    group between two HIP events and replayed from a HIP graph when stream capture works: the low orders run for
    ~10 us, where eager launches mostly measure the host's launch cadence."""
    fn()
    torch.cuda.synchronize()
    graph = None
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(inner):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        graph = g
    except Exception:                      # capture unsupported here: eager launches
        torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if graph is not None:
            graph.replay()
        else:
            for _ in range(inner):
                fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return sum(times) / len(times), min(times), graph is not None


def extras(sf, torch, dev, shard, nelmt=1 << 20, reps=40):
    """BASELINE configs 1 and 3 on one GPU: the hex nq = 2..10 sweep and the quad orders of the reference's
    run.sh (+ 20 / 24 / 26 / 28 / 30), `reps` groups of 8 launches (the reference's n_tests = 40; HIP events), each
    order with the MEAN over the groups (`frac_mean`, what `frac` and the sweep summary are) and the best group
    (`frac_min`, the reference's min-of-40 protocol) as fractions of the 8 TB/s HBM roofline."""
    replayed = [True]
    out = {"protocol": f"{nelmt} elements, {reps} groups of 8 back-to-back launches (HIP events; the groups are "
                       "HIP-graph replays when stream capture succeeds); *_mean = mean over the groups, *_min = the "
                       "fastest group; frac = frac_mean",
           "hex_sweep": {}, "quad": {}}

    def entry(dim, nq, dof, nbytes, fn):
        mean_ms, min_ms, graphed = grouped_ms(torch, fn, reps)
        replayed[0] = replayed[0] and graphed
        gbs_mean, gbs_min = nbytes / mean_ms * 1e-6, nbytes / min_ms * 1e-6
        return {"gdof_s": round(dof / mean_ms * 1e-6, 2), "gdof_s_min": round(dof / min_ms * 1e-6, 2),
                "gb_s": round(gbs_mean, 1), "frac": round(gbs_mean / HBM_PEAK_GBS, 4),
                "frac_mean": round(gbs_mean / HBM_PEAK_GBS, 4), "frac_min": round(gbs_min / HBM_PEAK_GBS, 4),
                "traffic_over_algorithmic": traffic_ratio(shard, dim, nq, nelmt)}

    for nq in range(2, 11):
        nm = nq - 1
        b = sf.fill_basis(nm, nq, dev)
        x = sf.fill_random(nelmt * nm ** 3, 1, 0, dev)
        o = torch.empty(nelmt * nq ** 3, dtype=torch.float64, device=dev)
        out["hex_sweep"][str(nq)] = entry(3, nq, nelmt * nm ** 3, nelmt * 8 * (nm ** 3 + nq ** 3),
                                          lambda: sf.bwdtrans_hex((nq,) * 3, b, b, b, x, out=o))
        del x, o
    for nq in QUAD_ORDERS:
        nm = nq - 1
        b = sf.fill_basis(nm, nq, dev)
        x = sf.fill_random(nelmt * nm ** 2, 1, 0, dev)
        o = torch.empty(nelmt * nq ** 2, dtype=torch.float64, device=dev)
        out["quad"][str(nq)] = entry(2, nq, nelmt * nm ** 2, nelmt * 8 * (nm ** 2 + nq ** 2),
                                     lambda: sf.bwdtrans_quad((nq, nq), b, b, x, out=o))
        del x, o
    out["hip_graph_replay"] = replayed[0]
    return out


if __name__ == "__main__":
    main()
