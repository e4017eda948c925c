#!/usr/bin/env python
"""bench.py — headline benchmark of the hot path on MI355X: batched Lomb-Scargle (BASELINE.json configs[1]) + the BLS
transit search (configs[3]) + the accuracy columns of the metric, in ONE JSON line.

    python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]

A plain run does only what the headline needs: it builds the inputs, runs W warm-up and K timed steps of the headline path
(`value`, `ms_per_step`, the `roofline` priced on their kernel time) and prints the line.  `--full` adds everything listed
below beside the headline: the CPU baselines and accuracy checks against the reference, the other LS method, the `--repeats`
blocks, the shader-clock probes, host_to_host, api_end_to_end, pipeline_end_to_end, configs[2]_on_1_gpu and the BLS, PLD
and flatten blocks (the same for the secondary workloads: their baselines, accuracy, clock probe and API block).
`--dump-outputs DIR`: after the timed steps, what the timed path computed in its last step is written as DIR/<name>.npy
(float64, or float32 where the output is float32; at most 64 MB in all, a larger output keeps a fixed seeded sample of its
elements; NaN and infinities are written as 0.0 and listed in DIR/<name>_nonfinite.npy, sample_outputs).  The inputs are seeded: two builds run with the same arguments can be compared file by file.

N > 1: the driver launches one rank per GPU (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`);
run by hand without WORLD_SIZE in the environment, `--gpus N` re-executes itself under torch.distributed.run with N
ranks on 127.0.0.1.  `--dry` forms the same process group on CPU (gloo) and exercises launch + barrier + max-over-ranks
without touching a GPU (tests/test_distributed_cpu.py).

A "step" = one pass of the hot path over one batch of targets, inputs already resident in HBM:
  * headline (`value`): B targets x M trial frequencies through lk_ls_fast_peaks_batch_dev — the reference's DEFAULT
    method ls_method="fast" (extirpolation + FFT) followed by the per-target (max power, argmax);
  * `other_method`: the exact direct-sum kernel (lk_ls_power_batch_dev + lk_argmax_batch_dev), same protocol;
  * `bls`: configs[3] (B targets x 50 000 periods x 200 durations) through lk_bls_batch_dev, 1 warm-up + <= 2 steps;
  * `pld`: configs[4] (500 cutouts 11x11 x 3500 cadences, pld_order 3, 16 components) through lk_pld_design_batch_dev +
    lk_regress_batch_dev; accuracy against lightkurve's own PLDCorrector output for the first cutouts
    (tests/golden/pld_c5.npz, made from the reference) and against the numpy port;
  * `flatten`: 1000 light curves x 20 000 cadences, window 401, through lk_savgol_trend_batch_dev; accuracy and
    cpu_baseline from scipy's savgol_filter / interp1d (the reference's own calls) run under conda on this box;
  * `accuracy` (N = 1): astropy ITSELF (conda interpreter, oracle/astropy_baseline.py suite) run on the first targets
    of the very same batches, arrays handed over as files: max-power relative error and argmax equality for 'fast'
    (vs astropy 'fast') and exact (vs astropy 'cython') at full N / M, BLS best-period index equality on the full
    period grid.  The same runs are the `cpu_baseline`s (the reference's CPU path on this box's usable cores).
  * `configs[2]_on_1_gpu`: north_star's own shape — 10 000 targets x 1e5 frequencies — in ONE call on this GPU, same protocol;
  * `pipeline_end_to_end`: a device-RESIDENT batch (lightkurve_amd.device.DeviceLightCurveBatch) through
    normalize -> flatten(401) -> Lomb-Scargle peaks: wall clock of the chain against the sum of its stages' kernel times;
  * every roofline block carries `shader_clock_mhz`: the clock the GPU sustained while that block's kernels ran (measured
    on the device, lk_shader_clock_mhz) — box-to-box spread of the fractions is mostly this number;
  * `host_to_host`: the same LS step through the HOST-pointer entry point (lk_ls_fast_peaks_batch: pinned,
    double-buffered staging), PCIe included — reported beside `value`, never as `value`.

Scaling: weak by default (every rank owns --targets targets); `--total-targets T` fixes the job (configs[2]: 10 000
targets over 8 GPUs) and reports "scaling": "strong".  Targets are independent: no data-path collective; with N > 1 the
per-target (max power, argmax) are all-gathered over RCCL each step (--gather summary), or the full spectra
(--gather spectra, chunked so the collective of chunk k overlaps the kernels of chunk k+1), everything device-resident.

Other workloads, same protocol and JSON shape: --workload bls | pld | regress | flatten | fold | lschi2 | pgsmooth.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK_TFLOPS = 78.6   # MI355X fp64 vector == fp64 MFMA dense peak (256 CU x 4 SIMD x 16 lanes x 2 x 2.4 GHz)
HBM_PEAK_GBS = 8000.0
CONDA = "/opt/conda/bin/python3.9"
SYS_STDCXX = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: the LS step is 11 ms and takes ~5 calls to reach its steady state after an idle GPU (20.1, 11.3, 10.9, 10.8, 10.76,
    # 10.70 ... ms per call, profiles/r06_lsfast_two_streams_ab.txt): 3 warm-up + 20 timed steps; the other blocks cap their own counts
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--targets", type=int, default=1000, help="targets per GPU (B), weak scaling")
    ap.add_argument("--total-targets", type=int, default=0,
                    help="strong scaling: total targets of the job, sharded over the ranks (configs[2]: 10000)")
    ap.add_argument("--cadences", type=int, default=20000, help="cadences per target (N)")
    ap.add_argument("--freqs", type=int, default=100000, help="trial frequencies (M)")
    ap.add_argument("--chunks", type=int, default=4, help="target chunks per step (comm/compute overlap)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the astropy runs (cpu_baseline AND accuracy)")
    ap.add_argument("--workload", default="ls", choices=["ls", "api", "bls", "pld", "flatten", "lschi2", "pgsmooth", "fold", "regress"])
    ap.add_argument("--repeats", type=int, default=5, help="workload ls, --full: blocks of K steps behind roofline.frac_median / _min / _max")
    ap.add_argument("--no-api", action="store_true", help="workload ls: skip the api_end_to_end block (Python batch API, host included)")
    ap.add_argument("--regressors", type=int, default=135, help="regress: design-matrix columns K")
    ap.add_argument("--nterms", type=int, default=2, help="lschi2: Fourier terms")
    ap.add_argument("--cutouts", type=int, default=500, help="PLD: cutouts per GPU")
    ap.add_argument("--pld-cadences", type=int, default=3500)
    ap.add_argument("--ls-method", default="both", choices=["both", "exact", "fast"],
                    help="fast: the reference's default method (extirpolation + FFT), the headline; exact: direct fp64 trig "
                         "sums; both (default): headline = fast, with --full the exact kernel is measured too and reported beside it")
    ap.add_argument("--gather", default="summary", choices=["summary", "spectra", "none"],
                    help="N>1: what is all-gathered over RCCL each step: per-target (max power, argmax), the full spectra, or nothing")
    ap.add_argument("--periods", type=int, default=50000)
    ap.add_argument("--durations", type=int, default=200)
    ap.add_argument("--no-bls", action="store_true", help="workload ls: skip the BLS block of the metric")
    ap.add_argument("--bls-targets", type=int, default=1000, help="workload ls: targets per GPU of the BLS block")
    ap.add_argument("--no-host", action="store_true", help="workload ls: skip the host-to-host measurement")
    ap.add_argument("--no-pld", action="store_true", help="workload ls: skip the PLD block (configs[4])")
    ap.add_argument("--no-flatten", action="store_true", help="workload ls: skip the flatten block")
    ap.add_argument("--flatten-targets", type=int, default=1000, help="workload ls: light curves per GPU of the flatten block")
    ap.add_argument("--flatten-window", type=int, default=401,
                    help="flatten: Savitzky-Golay window (401 with the 20 000-cadence bench shape; `--workload flatten "
                         "--cadences 4500 --flatten-window 101` is the long-cadence shape of the LDS-resident kernel)")
    ap.add_argument("--acc-flatten", type=int, default=64,
                    help="light curves flattened by scipy itself under conda (accuracy reference and cpu_baseline)")
    ap.add_argument("--acc-fast", type=int, default=256, help="targets checked against astropy 'fast' (also the cpu_baseline sample)")
    ap.add_argument("--acc-exact", type=int, default=16, help="targets checked against astropy 'cython' (74 s of one core each)")
    ap.add_argument("--acc-bls", type=int, default=32, help="targets checked against astropy run_bls on the full period grid")
    ap.add_argument("--c2-targets", type=int, default=10000,
                    help="workload ls: targets of the configs[2]-on-one-GPU block (north_star's 10k x 1e5 shape in one call); 0 = skip")
    ap.add_argument("--no-pipeline", action="store_true", help="workload ls: skip the pipeline_end_to_end block (device-resident chain)")
    ap.add_argument("--dry", action="store_true", help="CPU only: form the process group (gloo), barrier, max over ranks; no GPU work")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beside the headline (CPU baselines, accuracy, the other LS method, "
                         "--repeats, clock probes, host/API/pipeline blocks, configs[2], BLS, PLD, flatten); without it the "
                         "run sets up, warms up, times --steps steps of the headline and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy")
    args = ap.parse_args(argv)
    args.api_headline = args.workload == "api"
    if args.api_headline:
        # the Python batch API as the headline: the LS 'fast' device step (for the kernel time and the results to compare
        # with) + the api_end_to_end block, nothing else
        args.workload, args.ls_method = "ls", "fast"
        args.no_bls = args.no_pld = args.no_flatten = args.no_host = args.no_cpu_baseline = args.no_pipeline = True
        args.no_api = False
        args.c2_targets = 0
    # the headline metric keeps its name with and without --full
    args.metric_bls = not args.no_bls
    if not args.full:
        args.no_cpu_baseline = args.no_bls = args.no_pld = args.no_flatten = args.no_host = args.no_pipeline = True
        args.no_api = not args.api_headline
        args.c2_targets, args.repeats = 0, 1
        if args.ls_method == "both":
            args.ls_method = "fast"
    return args


DUMP_LIMIT_BYTES = 64 << 20


def sample_outputs(named):
    """--dump-outputs: [(name, torch tensor)] -> {name: numpy array}, float32 / float64 kept, anything else as float64.  An
    output of more elements than its share of DUMP_LIMIT_BYTES (24 B each: the value and room for its non-finite record)
    keeps, flattened, the elements at the flat indices np.unique(np.random.default_rng(0).integers(0, size, share)): the
    same sample in every run of the same shape.  Every dumped value is finite: a NaN or an infinity (the 'lk_amplitude'
    spectra hold NaN where the reference takes the square root of a negative power) is written as 0.0, and
    <name>_nonfinite, float64 (k, 2), lists each one as (flat index into <name>, 0 for NaN / +1 for +inf / -1 for -inf)."""
    import torch
    share = (DUMP_LIMIT_BYTES - 4096 * 2 * len(named)) // 24 // len(named)
    out = {}
    for name, x in named:
        if x.numel() > share:
            idx = np.unique(np.random.default_rng(0).integers(0, x.numel(), share))
            x = x.reshape(-1)[torch.from_numpy(idx).to(x.device)]
        a = x.cpu().numpy()
        a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
        bad = np.flatnonzero(~np.isfinite(a))
        if bad.size:
            flat = a.reshape(-1)
            out[name + "_nonfinite"] = np.stack([bad.astype(np.float64), np.sign(np.nan_to_num(flat[bad], nan=0.0))], axis=1)
            a = a.copy()
            a.reshape(-1)[bad] = 0.0
        out[name] = a
    return out


def effective_cores(cap=64):
    """Host cores this process may actually use: min(affinity mask, cgroup CPU quota) — the GPU box advertises
    256 logical CPUs but its cgroup grants 16 (cpu.max = "1600000 100000")."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
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
    return max(1, min(n, cap))


# ------------------------------------------------------------------------------------------------ self-launch
def self_launch(args):
    """`python bench.py --gpus N` outside torch.distributed.run: re-execute under it with N ranks on 127.0.0.1."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world):
    """The launch / rendezvous / barrier / max-over-ranks skeleton of the real run on CPU (gloo), no GPU work."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
    from lightkurve_amd import distributed as LD
    from lightkurve_amd.distributed import shard_bounds
    total = args.total_targets or args.targets * world
    bounds = strong_bounds(args, world) if args.total_targets else np.arange(world + 1) * args.targets
    mine = int(bounds[rank + 1] - bounds[rank])
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    dt = time.perf_counter() - t0
    # the gathers of the real step on CPU tensors: shards padded to the largest one, chunked all-gather of the "spectra"
    # (row b of rank r holds its global target index), per-target summaries — and a check that every rank can rebuild
    # the whole batch from what it received
    gather_checked = None
    if world > 1 and args.gather != "none":
        first = int(bounds[rank])
        Bmax = int(np.max(np.diff(bounds)))
        Md = 16
        pad = torch.zeros((Bmax, Md), dtype=torch.float64)
        pad[:mine] = torch.arange(first, first + mine, dtype=torch.float64)[:, None] + 0.001 * torch.arange(Md, dtype=torch.float64)
        ok = True
        if args.gather == "spectra":
            nch = max(1, min(args.chunks, max(mine, 1)))
            cb = np.linspace(0, Bmax, nch + 1).astype(int)
            full = torch.full((world, Bmax, Md), -1.0, dtype=torch.float64)
            for c in range(nch):
                out = torch.empty((world, int(cb[c + 1] - cb[c]), Md), dtype=torch.float64)
                LD.all_gather_equal(out, pad[int(cb[c]):int(cb[c + 1])])
                full[:, int(cb[c]):int(cb[c + 1])] = out
        else:
            full = torch.empty((world, Bmax, Md), dtype=torch.float64)
            LD.all_gather_equal(full, pad)
        for r in range(world):
            nr = int(bounds[r + 1] - bounds[r])
            want = torch.arange(int(bounds[r]), int(bounds[r]) + nr, dtype=torch.float64)
            ok = ok and bool(torch.equal(full[r, :nr, 0], want)) and bool(torch.all(full[r, nr:] == 0))
        gather_checked = ok
    tt = torch.tensor([dt, float(mine)], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        mx = tt.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = tt.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        dt, total_seen = float(mx[0]), int(sm[1])
    else:
        total_seen = mine
    if rank == 0:
        print(json.dumps({"metric": "dry run (no GPU work)", "dry": True, "n_gpus": world, "value": 0.0,
                          "targets_total": total_seen, "scaling": "strong" if args.total_targets else "weak",
                          "gather": args.gather, "gather_checked": gather_checked, "shards": [int(x) for x in np.diff(bounds)],
                          "ms_per_step": 1e3 * dt, "steps": args.steps, "warmup": args.warmup}))
    if world > 1:
        dist.destroy_process_group()
    return 0


def strong_bounds(args, world):
    """--total-targets: contiguous shards balanced by cost (sum of N_b * M per shard, lightkurve_amd.distributed
    .partition_by_cost), not by count — the synthetic targets all have N cadences, so here the two coincide; a ragged
    batch would not."""
    from lightkurve_amd.distributed import shard_bounds
    costs = np.full(args.total_targets, float(args.cadences) * float(args.freqs))
    return shard_bounds(args.total_targets, world, costs=costs)


# ------------------------------------------------------------------------------------------------ reference runs
def _moment_tiles(k, order):
    """Number of 16 x 16 MFMA tiles pld_moment_gram_kernel computes per cadence step for the order-`order` products of k
    components (same construction as lightkurve_amd/csrc/pld.hip: moment_plan): rows ordered by largest factor, columns in
    lexicographic order, wave tiles of 4 x 4 tiles masked to those that hold a canonical (max(row) <= min(col)) pair."""
    import itertools
    cols = list(itertools.combinations_with_replacement(range(k), order))
    pc = len(cols)
    rperm = sorted(range(pc), key=lambda i: (cols[i][-1], i))
    colstart = [sum(1 for c in cols if c[0] < m) for m in range(k + 2)]
    tiles = 0
    for r0 in range(0, pc, 64):
        rt = [min((cols[x][-1] for x in rperm[r0 + 16 * i:r0 + 16 * i + 16]), default=None) for i in range(4)]
        mn = min(x for x in rt if x is not None)
        for cg in range((colstart[mn] // 16) * 16, pc, 64):
            for i in range(4):
                for j in range(4):
                    if rt[i] is not None and cg + 16 * j < pc and cg + 16 * j + 16 > colstart[rt[i]]:
                        tiles += 1
    return tiles


def reference_suite(args, want_ls, want_bls, want_flatten=False):
    """Run astropy itself (the reference's numerical dependency) on the first targets of the bench batches, before
    torch/HIP is initialised: returns the suite's result dict (rates + per-target maxima), or None when the conda
    interpreter / astropy is not there.  Inputs travel as .npz files so both sides see identical arrays."""
    from lightkurve_amd import synth
    if not os.path.exists(CONDA):
        return None
    cores = effective_cores()
    work = tempfile.mkdtemp(prefix="lk_bench_")
    spec = {}
    try:
        if want_ls:
            n = max(args.acc_fast, args.acc_exact)
            n = min(n, args.targets)
            t, y, dy, off = synth.ls_batch(1, n, args.cadences, first_index=0)
            for b in range(n):
                t[off[b]:off[b + 1]] -= t[off[b]]
            df = 360.0 / args.freqs
            np.savez(os.path.join(work, "ls.npz"), t=t, y=y, off=off, f0=df, df=df, M=args.freqs)
            spec["ls"] = {"n_fast": min(args.acc_fast, n), "n_exact": min(args.acc_exact, n)}
        if want_bls and args.acc_bls > 0:
            n = min(args.acc_bls, args.bls_targets if args.workload == "ls" else args.targets)
            t, y, e, off = synth.bls_batch(3, n, args.cadences, first_index=0)
            period, duration = synth.bls_grid(args.periods, args.durations)
            np.savez(os.path.join(work, "bls.npz"), t=t, y=y, e=e, off=off, period=period, duration=duration)
            spec["bls"] = {"n": n}
        if want_flatten and args.acc_flatten > 0:
            n = min(args.acc_flatten, args.flatten_targets if args.workload == "ls" else args.targets)
            t, y, dy, off = synth.ls_batch(6, n, args.cadences, first_index=0)
            np.savez(os.path.join(work, "flatten.npz"), t=t, y=y, off=off, window=args.flatten_window)
            spec["flatten"] = {"n": n}
        json.dump(spec, open(os.path.join(work, "suite.json"), "w"))
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "oracle", "shims") + os.pathsep + ROOT)
        if os.path.exists(SYS_STDCXX):
            env["LD_PRELOAD"] = SYS_STDCXX
        p = subprocess.run([CONDA, "-W", "ignore", os.path.join(ROOT, "oracle", "astropy_baseline.py"), "suite", work,
                            str(cores)], env=env, capture_output=True, timeout=1500)
        rpath = os.path.join(work, "result.json")
        if p.returncode != 0 or not os.path.exists(rpath):
            sys.stderr.write("astropy suite failed: %s\n" % p.stderr.decode()[-800:])
            return None
        res = json.load(open(rpath))
        res["cores"] = cores
        if "flatten" in res:
            res["flatten"]["trends"] = np.load(os.path.join(work, "flatten_trends.npy"))
        if "bls" in res and os.path.exists(os.path.join(work, "bls_folded.npy")):
            res["bls"]["folded_flux"] = np.load(os.path.join(work, "bls_folded.npy"))
        return res
    except Exception as e:   # the baseline is reported, never required
        sys.stderr.write("astropy suite failed: %r\n" % (e,))
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def port_baseline_ls(args):
    """Fallback when astropy is absent: the numpy port of the reference default (oracle.np_oracle.ls_power_fast)."""
    import multiprocessing as mp
    from oracle import cpu_baseline as cb
    cores = effective_cores()
    n_targets = cores * 2
    jobs = [(1, i, args.cadences, args.freqs) for i in range(n_targets)]
    with mp.get_context("spawn").Pool(cores) as pool:
        pool.map(cb.ls_fast_one, jobs[:cores])
        t0 = time.perf_counter()
        pool.map(cb.ls_fast_one, jobs)
        dt = time.perf_counter() - t0
    return {"value": n_targets * args.freqs / dt, "unit": "frequencies*targets/sec", "cores": cores, "kind": "port",
            "sample": "%d targets x %d freqs, N=%d, numpy port of the reference default ls_method='fast' "
                      "(Press-Rybicki FFT), %d processes" % (n_targets, args.freqs, args.cadences, cores)}


def port_baseline_bls(args):
    from oracle import cpu_baseline as cb
    rate = cb.bls_rate(args.cadences, args.durations)
    return {"value": rate, "unit": "periods*targets/sec", "cores": 1, "kind": "port",
            "sample": "C oracle (restated astropy run_bls), 1 target x 24 periods x %d durations, N=%d, 1 core"
                      % (args.durations, args.cadences)}


def _pld_port_one(job):
    """One cutout through the numpy/LAPACK port, BLAS pinned to one thread (one process per core)."""
    i, n_cad = job
    try:
        from threadpoolctl import threadpool_limits
        ctx = threadpool_limits(limits=1)
    except Exception:
        import contextlib
        ctx = contextlib.nullcontext()
    from lightkurve_amd import synth
    from oracle import np_oracle as O
    allm = np.ones((11, 11), bool)
    with ctx:
        t, flux, err, _ = synth.pld_cutout(4, i, n=n_cad, npix=11)
        r = O.pld_correct(t, flux, err, allm, allm, allm, pld_order=3, pca_components=16, spline_degree=5)
    return np.asarray(r["corrected"]), np.asarray(r["outlier_mask"])


def cpu_baseline_pld(args):
    """PLDCorrector.correct on the host cores, one process per core like the other blocks' baselines: the numpy/LAPACK port
    (oracle.np_oracle.pld_correct: exact SVD in place of fbpca, kind "port") — lightkurve itself is not installed on the GPU
    box, so kind "reference" is reported by the committed golden's accuracy block instead (tests/golden/pld_c5.npz)."""
    import multiprocessing as mp
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    procs = max(1, min(cores, 32))
    n = max(2, procs)
    jobs = [(i, args.pld_cadences) for i in range(n)]
    t0 = time.perf_counter()
    if procs > 1:
        with mp.get_context("fork").Pool(procs) as pool:
            kept = pool.map(_pld_port_one, jobs)
    else:
        kept = [_pld_port_one(j) for j in jobs]
    dt = time.perf_counter() - t0
    port = {"value": n / dt, "unit": "cutouts/sec", "cores": procs, "kind": "port",
            "sample": "%d cutouts 11x11 x %d cadences, order 3, 16 PCA comps, numpy/LAPACK port of PLDCorrector.correct, "
                      "%d processes x 1 BLAS thread, %.1f s" % (n, args.pld_cadences, procs, dt),
            # the port is SLOWER than the reference (exact SVDs where lightkurve runs fbpca's randomised range finder): the
            # speed-up is also priced on SURVEY.md §6's measurement of PLDCorrector.correct itself, scaled ideally to these cores
            "reference_s_per_cutout_survey": SURVEY_PLD_S_PER_CUTOUT,
            "value_priced_on_survey": procs / SURVEY_PLD_S_PER_CUTOUT,
            "_results": kept[:2]}   # popped before the JSON line: the accuracy block compares the GPU path with these
    ref = reference_baseline_pld(args)
    if ref is not None:   # a lightkurve checkout is staged on this box: the reference itself is the baseline
        ref["port"] = {k: v for k, v in port.items() if not k.startswith("_")}
        ref["reference_s_per_cutout_survey"] = SURVEY_PLD_S_PER_CUTOUT
        ref["value_priced_on_survey"] = port["value_priced_on_survey"]
        ref["_results"] = port["_results"]
        return ref
    return port


SURVEY_PLD_S_PER_CUTOUT = 1.14   # lightkurve's PLDCorrector.correct on ONE core, 11 x 11 px x 3500 cadences


def reference_baseline_pld(args):
    """kind "reference" for the PLD block: lightkurve's own PLDCorrector.correct, one process per core, when a lightkurve
    checkout has been staged on this box (LK_REFERENCE_ROOT, tools/stage_reference.sh: the GPU box has conda + astropy but
    no lightkurve) — a builder-run measurement; the driver's line keeps the port and prices the speed-up on SURVEY's figure."""
    ref_root = os.environ.get("LK_REFERENCE_ROOT")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "lightkurve")) or not os.path.exists(CONDA):
        return None
    cores = effective_cores()
    procs = max(1, min(cores, 32))
    n = 16 * procs   # ~10 s of wall clock at ~0.6 s per call and process
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "oracle", "shims"), os.path.join(ref_root, "src"), ROOT]),
               OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")   # one BLAS thread per process, set before numpy loads
    if os.path.exists(SYS_STDCXX):
        env["LD_PRELOAD"] = SYS_STDCXX
    try:
        p = subprocess.run([CONDA, "-W", "ignore", os.path.join(ROOT, "oracle", "lightkurve_pld_baseline.py"), str(n),
                            str(args.pld_cadences), str(procs)], env=env, capture_output=True, timeout=1500)
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    except Exception as e:
        sys.stderr.write("lightkurve PLD baseline failed: %r\n" % (e,))
        return None
    return {"value": r["cutouts_per_s"], "unit": "cutouts/sec", "cores": procs, "kind": "reference",
            "sample": "lightkurve %s PLDCorrector(tpf).correct(pld_order=3, pca_components=16, pld_aperture_mask='all') itself "
                      "(pldcorrector.py:304-427; fbpca replaced by the exact-SVD shim of oracle/shims), %d cutouts 11x11 x %d "
                      "cadences, %d processes x 1 BLAS thread, %.1f s (TargetPixelFileFactory construction included); one "
                      "correct() call alone: %.2f s (median)" % (r["lightkurve"], r["n"], args.pld_cadences, procs, r["seconds"],
                                                                  r["correct_call_seconds_median"])}


def cpu_baseline_flatten(args):
    from lightkurve_amd import synth
    from oracle import np_oracle as O
    n = 8
    lcs = [synth.ls_target(6, i, args.cadences) for i in range(n)]
    t0 = time.perf_counter()
    kept = [O.flatten_trend(t, y, args.flatten_window, 2, 5, 3, 3)[0] for t, y, e, _ in lcs]
    dt = time.perf_counter() - t0
    return {"value": n * args.cadences / dt, "unit": "cadences/sec", "cores": 1, "kind": "port",
            "sample": "%d light curves x %d cadences, window %d, numpy port of LightCurve.flatten" % (n, args.cadences, args.flatten_window),
            "_results": kept}   # popped before the JSON line: the accuracy block compares the GPU trends with these


def cpu_baseline_lschi2(args):
    from lightkurve_amd import synth
    from oracle import np_oracle as O
    t, y, e, _ = synth.ls_target(1, 0, 2000)
    f = 0.0036 * (1 + np.arange(400))
    t0 = time.perf_counter()
    O.ls_power_chi2(t - t[0], y, None, f, nterms=args.nterms, normalization="lk_amplitude")
    dt = time.perf_counter() - t0
    # cost is linear in cadences x frequencies: scale the sample's pair rate to a frequencies*targets rate at N cadences
    return {"value": len(f) * 2000.0 / args.cadences / dt, "unit": "frequencies*targets/sec", "cores": 1, "kind": "port",
            "sample": "numpy restatement of astropy lombscargle_chi2 (nterms=%d), 2000 cadences x 400 frequencies, "
                      "rate rescaled to %d cadences per target" % (args.nterms, args.cadences)}


def cpu_baseline_pgsmooth(args):
    from oracle import np_oracle as O
    rng = np.random.default_rng(0)
    M = args.freqs
    f = 0.0036 * (1 + np.arange(M))
    p = rng.chisquare(2, M)
    t0 = time.perf_counter()
    O.pg_smooth_logmedian(f, p, 0.01)
    dt = time.perf_counter() - t0
    return {"value": M / dt, "unit": "frequencies*targets/sec", "cores": 1, "kind": "port",
            "sample": "1 periodogram x %d frequencies, logmedian filter_width 0.01, numpy restatement of the reference loop" % M}


def cpu_baseline_regress(args):
    from oracle import np_oracle as O
    rng = np.random.default_rng(0)
    n, K, nb = args.pld_cadences, args.regressors, 4
    Xs = [rng.standard_normal((n, K)) for _ in range(nb)]
    ys = [X @ rng.standard_normal(K) * 1e-3 + 1 + 1e-3 * rng.standard_normal(n) for X in Xs]
    t0 = time.perf_counter()
    for X, y in zip(Xs, ys):
        O.regression_correct(X, y, np.full(n, 1e-3), prior_mu=np.zeros(K), prior_sigma=np.full(K, 10.0))
    dt = time.perf_counter() - t0
    return {"value": nb / dt, "unit": "fits/sec", "cores": effective_cores(), "kind": "port",
            "sample": "%d fits, N=%d, K=%d, 5 sigma-clip iterations, numpy port of RegressionCorrector.correct "
                      "(BLAS/LAPACK may thread)" % (nb, n, K)}


def cpu_baseline_fold(args):
    from lightkurve_amd import synth
    from oracle import np_oracle as O
    lcs = [synth.ls_target(6, i, args.cadences) for i in range(32)]
    t0 = time.perf_counter()
    for t, y, e, _ in lcs:
        ph, order, _c = O.fold(t, 3.3, t[0])
        y[order], e[order]
    dt = time.perf_counter() - t0
    return {"value": 32 * args.cadences / dt, "unit": "cadences/sec", "cores": 1, "kind": "port",
            "sample": "32 light curves x %d cadences, numpy mod + stable argsort + two gathers" % args.cadences}


# BLS instruction mix per (target, period) of configs[3], from the committed SQ counter passes of THIS round's kernels at the
# bench shape (profiles/r05_bls_pmc_sq.txt, _sq2.txt: `bench.py --workload bls --steps 1 --warmup 1` under rocprofv3 --pmc,
# i.e. 2 steps x 1000 targets x 50 000 periods; bls_team_deep_kernel + bls_team_kernel): busy quad-cycles of the VALU and
# LDS instruction pipes summed over all SIMDs.
_BLS_PMC_UNITS = 2 * 1000 * 50000.0
BLS_PMC = {"valu_busy_quad_cycles": (903958224704 + 1718560537839) / _BLS_PMC_UNITS,
           "lds_busy_quad_cycles": (196665709376 + 357009061971) / _BLS_PMC_UNITS,
           "lds_bank_conflict_cycles": (407316454294 + 476562731349) / _BLS_PMC_UNITS,
           "lds_wait_cycles": (222445482287 + 407333220130) / _BLS_PMC_UNITS,
           "valu_insts": (884767612883 + 1677464182329) / _BLS_PMC_UNITS,
           "salu_insts": (554299774229 + 1072152555377) / _BLS_PMC_UNITS,
           "lds_insts": (101366606862 + 151239607525) / _BLS_PMC_UNITS}


def bls_roofline(Bb, nP, kms, equiv_tflops, traffic):
    """What bounds bls_team_kernel is instruction issue (fp64 VALU + LDS atomics / prefix chains in LDS), not HBM and not a
    flop count: the bit-exact scan SKIPS most of the (start bin, duration) candidates SURVEY 8(d) prices at 12 flop each, so
    that figure is an equivalent rate, reported as such.  `frac` = measured VALU-busy issue cycles / issue cycles available
    (4 SIMDs x 256 CUs, one instruction per quad-cycle at 2.4 GHz) over this run's kernel time."""
    units = float(Bb) * nP
    slots = kms * 1e-3 * 1024 * 2.4e9 / 4.0
    return {"bound": "valu_issue", "achieved": BLS_PMC["valu_busy_quad_cycles"] * units, "peak": slots,
            "unit": "SIMD issue quad-cycles per step", "frac": BLS_PMC["valu_busy_quad_cycles"] * units / slots,
            "lds_issue_frac": BLS_PMC["lds_busy_quad_cycles"] * units / slots,
            "per_target_period": {"valu_instructions": BLS_PMC["valu_insts"], "lds_instructions": BLS_PMC["lds_insts"],
                                  "lds_bank_conflict_cycles": BLS_PMC["lds_bank_conflict_cycles"],
                                  "lds_wait_cycles": BLS_PMC["lds_wait_cycles"], "salu_instructions": BLS_PMC["salu_insts"]},
            "counters_from": "profiles/r05_bls_pmc_sq.txt, r05_bls_pmc_sq2.txt (kernels unchanged since; rocprofv3 --pmc passes of `bench.py --workload "
                             "bls` at the bench shape, 1000 targets x 50 000 periods, this round's kernels); the clock under "
                             "load is below 2.4 GHz, so the true fraction is higher by that ratio",
            "traffic": traffic, "kernel": "bls_team_kernel / bls_team_deep_kernel", "kernel_ms_per_step": kms,
            # SURVEY.md 8(d)'s own pricing, beside `frac` (VERDICT r5 #4d): 12 flop x EVERY (start bin, duration) candidate
            # over the kernel time against the fp64 vector peak — an equivalent rate (most candidates are skipped by rigorous
            # bounds), see equivalent_rate.note
            "frac_survey_8d_flop_equivalent": equiv_tflops / FP64_VECTOR_PEAK_TFLOPS,
            "equivalent_rate": {"value": equiv_tflops, "unit": "TFLOP/s", "frac_of_fp64_vector_peak": equiv_tflops / FP64_VECTOR_PEAK_TFLOPS,
                                "note": "12 flop per (start bin, duration) candidate (SURVEY.md 8(d)) x ALL candidates / time — "
                                        "the kernel evaluates a small fraction of them (rigorous growth / block-maximum bounds "
                                        "skip the rest), so this is NOT a utilisation and must not be read against a peak"},
            "note": "everything lives in LDS; HBM traffic is the 7 outputs + the inputs once"}


def load_traffic():
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        return json.load(open(tpath))
    except Exception:
        return {}


# ------------------------------------------------------------------------------------------------ main
def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry:
        sys.exit(dry_run(args, rank, world))

    # ---- the reference's CPU path (cpu_baseline + accuracy reference): rank 0 at N = 1 only, before torch/HIP exist
    ref, cpu_base, cpu_base_bls, cpu_base_pld, cpu_base_flat = None, None, None, None, None
    # (rank 0 does this for any world: the other ranks wait for it at the rendezvous, so N > 1 lines carry the reference's
    # numbers and the accuracy block too)
    if rank == 0 and not args.no_cpu_baseline:
        if args.workload == "ls":
            ref = reference_suite(args, True, not args.no_bls, not args.no_flatten)
            if ref is None:
                cpu_base = port_baseline_ls(args)
                cpu_base_bls = None if args.no_bls else port_baseline_bls(args)
            if not args.no_pld:
                cpu_base_pld = cpu_baseline_pld(args)
            if not args.no_flatten and (ref is None or "flatten" not in ref):
                cpu_base_flat = cpu_baseline_flatten(args)
        elif args.workload == "bls":
            ref = reference_suite(args, False, True)
            if ref is None:
                cpu_base = port_baseline_bls(args)
        elif args.workload == "flatten":
            ref = reference_suite(args, False, False, True)
            if ref is None or "flatten" not in ref:
                cpu_base = cpu_baseline_flatten(args)
        else:
            cpu_base = {"pld": cpu_baseline_pld, "flatten": cpu_baseline_flatten, "lschi2": cpu_baseline_lschi2,
                        "pgsmooth": cpu_baseline_pgsmooth, "fold": cpu_baseline_fold,
                        "regress": cpu_baseline_regress}[args.workload](args)
        if ref is not None:
            if "ls_fast" in ref:
                r = ref["ls_fast"]
                cpu_base = {"value": r["units_per_s"], "unit": "frequencies*targets/sec", "cores": ref["cores"],
                            "kind": "reference",
                            "sample": "astropy %s LombScargle.power(method='fast') as lightkurve calls it "
                                      "(periodogram.py:961-964), %d targets x %d freqs, N=%d, %d processes, %.1f s"
                                      % (ref["astropy"], r["n_targets"], args.freqs, args.cadences, ref["procs"], r["seconds"])}
                if "ls_cython" in ref:
                    rc = ref["ls_cython"]
                    cpu_base["exact_cython"] = {
                        "value": rc["units_per_s"], "unit": "frequencies*targets/sec", "cores": ref["cores"],
                        "sample": "astropy LombScargle.power(method='cython') (the exact method), %d targets x %d freqs, "
                                  "N=%d, %d processes, %.1f s" % (rc["n_targets"], args.freqs, args.cadences, ref["procs"],
                                                                  rc["seconds"])}
            if "bls" in ref:
                r = ref["bls"]
                cb = {"value": r["units_per_s"], "unit": "periods*targets/sec", "cores": ref["cores"], "kind": "reference",
                      "sample": "astropy %s BoxLeastSquares.power (compiled run_bls) as lightkurve calls it "
                                "(periodogram.py:1161-1169), %d targets x %d periods x %d durations, N=%d, %d processes, "
                                "%.1f s" % (ref["astropy"], r["n_targets"], args.periods, args.durations, args.cadences,
                                            ref["procs"], r["seconds"])}
                if args.workload == "bls":
                    cpu_base = cb
                else:
                    cpu_base_bls = cb
            if "flatten" in ref:
                r = ref["flatten"]
                cb = {"value": r["units_per_s"], "unit": "cadences/sec", "cores": ref["cores"], "kind": "reference",
                      "sample": "scipy %s savgol_filter + interp1d inside the restated loop of LightCurve.flatten "
                                "(lightcurve.py:996-1063; lightkurve itself is not installed on this box), %d light curves x %d "
                                "cadences, window %d, %d processes, %.1f s"
                                % (r["scipy"], r["n_targets"], args.cadences, args.flatten_window, ref["procs"], r["seconds"]),
                      "_results": [r["trends"][i * args.cadences:(i + 1) * args.cadences] for i in range(r["n_targets"])]}
                if args.workload == "flatten":
                    cpu_base = cb
                else:
                    cpu_base_flat = cb

    import ctypes
    import torch
    import torch.distributed as dist
    from lightkurve_amd import _capi, synth
    from lightkurve_amd import distributed as LD
    from lightkurve_amd.distributed import shard_bounds

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # LK_BENCH_FORCE_DIST=1 runs the N>1 code paths (RCCL init, gathers, barrier, max over ranks) with a single rank —
    # the only way to exercise them on a 1-GPU box
    dist_on = world > 1 or os.environ.get("LK_BENCH_FORCE_DIST") == "1"
    if dist_on:
        # RCCL prints a version banner on STDOUT when the first communicator is created; this script's stdout is one
        # JSON line, so file descriptor 1 points at stderr until the communicator exists
        import datetime
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(minutes=30))
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
    handle = _capi.Handle.get(local_rank)
    lib = _capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    vp = ctypes.c_void_p
    i64p = ctypes.POINTER(ctypes.c_int64)

    def sync():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize()

    def timed(step_fn, warmup, steps):
        """W untimed + K timed steps bracketed by barrier + synchronize; returns (max-over-ranks seconds, mean HIP-event
        ms of the kernel region per step).  step_fn(e0, e1) records e0/e1 around the library calls on `stream`."""
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + steps)]
        for k in range(warmup):
            step_fn(*evs[k])
        sync()
        t0 = time.perf_counter()
        for k in range(warmup, warmup + steps):
            step_fn(*evs[k])
        sync()
        dt = time.perf_counter() - t0
        if dist_on:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        kms = float(np.mean([e0.elapsed_time(e1) for e0, e1 in evs[warmup:]]))
        return dt, kms

    def clock_under(step_fn, steps, expect_ms):
        """Sustained shader clock [MHz] while `steps` calls of step_fn run: lk_shader_clock_mhz spins one wave on a stream of
        its own for ~70 % of the expected duration, started from a thread so that a launcher that blocks the host cannot
        leave the probe measuring an idle GPU.  None if the probe fails (never fatal) or without --full (it runs steps of
        its own)."""
        if not args.full:
            return None
        import threading
        spin = float(min(1000.0, max(1.0, 0.7 * expect_ms * steps)))
        mhz = ctypes.c_double(0.0)
        rc = [1]

        def probe():
            rc[0] = lib.lk_shader_clock_mhz(handle._h, spin, ctypes.byref(mhz))

        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        step_fn(*evs[0])                        # the GPU is busy before the probe's first reading
        th = threading.Thread(target=probe)
        th.start()
        for k in range(1, steps):
            step_fn(*evs[k])
        th.join()
        torch.cuda.synchronize()
        if rc[0] != 0 or not mhz.value > 0:
            return None
        return {"value": float(mhz.value), "measured_over_ms": spin,
                "how": "lk_shader_clock_mhz: shader-cycle counter / constant-rate counter on one wave of a side stream while "
                       "%d steps of this block ran" % steps}

    def ls_batch_threaded(config, nb, n, first_index):
        """synth.ls_batch over a thread pool (every target has its own seeded generator: the result does not depend on the
        split); 10 000 targets take ~40 s on one core."""
        from concurrent.futures import ThreadPoolExecutor
        nth = max(1, min(effective_cores(), 16, nb))
        cuts = np.linspace(0, nb, nth + 1).astype(int)
        with ThreadPoolExecutor(max_workers=nth) as ex:
            parts = list(ex.map(lambda k: synth.ls_batch(config, int(cuts[k + 1] - cuts[k]), n, first_index=first_index + int(cuts[k])),
                                range(nth)))
        tt = np.concatenate([q[0] for q in parts])
        yy = np.concatenate([q[1] for q in parts])
        ee = np.concatenate([q[2] for q in parts])
        oo = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(q[3]) for q in parts]))]).astype(np.int64)
        return tt, yy, ee, oo

    # ---- how many targets this rank owns
    strong = args.total_targets > 0
    if strong:
        bounds = strong_bounds(args, world)
        first, B = int(bounds[rank]), int(bounds[rank + 1] - bounds[rank])
        total_targets = args.total_targets
    else:
        first, B = rank * args.targets, args.targets
        total_targets = args.targets * world
    N, M = args.cadences, args.freqs
    traffic_all = load_traffic()
    out, extra = {}, {}
    roofline = None
    dump = bool(args.dump_outputs)
    dumped = {}   # --dump-outputs: the headline path's outputs of its last timed step, {name: numpy array}

    # ================================================================================================ BLS block
    def run_bls(Bb, first_index, steps, warmup, dump=False):
        t, y, dy, off = synth.bls_batch(3, Bb, N, first_index=first_index)
        ivar = 1.0 / dy ** 2
        nchk = min(Bb, max(args.acc_bls, 1))
        raw_t, raw_y = t[:off[nchk]].copy(), y[:off[nchk]].copy()   # as the reference sees them (the folded-flux check)
        tmin = np.array([t[off[b]:off[b + 1]].min() for b in range(nchk)])
        for b in range(Bb):
            s = slice(off[b], off[b + 1])
            t[s] -= t[s].min()
            y[s] -= np.median(y[s])
        period, duration = synth.bls_grid(args.periods, args.durations)
        nP = len(period)
        d_t, d_y, d_w = (torch.from_numpy(a).to(dev) for a in (t, y, ivar))
        d_per = torch.from_numpy(period).to(dev)
        d_out = torch.empty((7, Bb, nP), dtype=torch.float64, device=dev)
        d_max = torch.empty(Bb, dtype=torch.float64, device=dev)
        d_arg = torch.empty(Bb, dtype=torch.int64, device=dev)

        def step(e0, e1):
            e0.record()
            _capi.bls_batch_dev(handle, Bb, off, d_t.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), period,
                                d_per.data_ptr(), duration, 10, True, d_out.data_ptr(), stream)
            e1.record()
            _capi.argmax_batch_dev(handle, Bb, nP, d_out.data_ptr(), d_max.data_ptr(), d_arg.data_ptr(), stream)

        dt, kms = timed(step, warmup, steps)
        dumped = sample_outputs([(k, d_out[i]) for i, k in enumerate(_capi.BLS_FIELDS)] +
                                [("max_power", d_max), ("argmax", d_arg)]) if dump else {}
        clk = clock_under(step, 1, kms)
        nb = np.ceil(period / (duration.min() / 10)) + 10
        durb = np.unique(np.round(duration / (duration.min() / 10)))
        cand = float(np.sum(np.maximum(nb[:, None] - durb[None, :] + 1, 0))) * Bb   # (start bin, duration) candidates
        ach = 12.0 * cand / (kms * 1e-3) / 1e12
        res = {
            "metric": "BLS periods*targets/sec", "unit": "periods*targets/sec",
            "units_per_step": Bb * nP, "dt": dt, "steps": steps, "warmup": warmup, "kernel_ms": kms,
            "workload": "configs[3]: %d targets x %d cadences, %d periods x %d durations BLS per GPU" % (Bb, N, nP, len(duration)),
            "roofline": dict(bls_roofline(Bb, nP, kms, ach, traffic_all.get("bls")), shader_clock_mhz=clk),
            "argmax": d_arg.cpu().numpy(), "max_power": d_max.cpu().numpy(),
            "period_at_max": period[np.clip(d_arg.cpu().numpy(), 0, nP - 1)], "dumped": dumped,
        }
        # transit time at the best period of the first targets (row 4 of the seven outputs) + their inputs: the folded-flux check
        am = np.clip(res["argmax"][:nchk], 0, nP - 1)
        res["transit_time_at_max"] = d_out[4, torch.arange(nchk, device=dev), torch.from_numpy(am).to(dev)].cpu().numpy() + tmin
        res["_fold_inputs"] = (raw_t, raw_y, off[:nchk + 1].copy())
        del d_out
        return res

    def bls_accuracy(res, refb):
        n = min(len(refb["argmax"]), len(res["argmax"]))
        a_ref, a_gpu = np.asarray(refb["argmax"][:n]), res["argmax"][:n]
        p_ref, p_gpu = np.asarray(refb["max_power"][:n]), res["max_power"][:n]
        return {"targets_checked": n, "reference": "astropy %s BoxLeastSquares.power on the full %d-period grid"
                % (ref["astropy"], args.periods),
                "best_period_index_equal": "%d/%d" % (int(np.sum(a_ref == a_gpu)), n),
                "max_power_bit_identical": "%d/%d" % (int(np.sum(p_ref == p_gpu)), n),
                "max_power_relerr_max": float(np.max(np.abs(p_gpu - p_ref) / np.abs(p_ref))),
                **folded_flux_check(res, refb, n)}

    def folded_flux_check(res, refb, n):
        """BASELINE's third accuracy item: the light curve folded at the best period (lk_fold_batch at OUR best period and
        transit time) against astropy's TimeSeries.fold + sort at ITS best period, as lightkurve.fold does."""
        if "folded_flux" not in refb or "_fold_inputs" not in res:
            return {}
        tt, yy, oo = res["_fold_inputs"]
        n = min(n, len(oo) - 1)
        _, order, cols = _capi.fold_batch(tt[:oo[n]], oo[:n + 1], res["period_at_max"][:n], res["transit_time_at_max"][:n],
                                          columns=(yy[:oo[n]],))
        ref_f = np.asarray(refb["folded_flux"])[:oo[n]]
        same = cols[0] == ref_f
        return {"folded_flux_max_abs_diff": float(np.max(np.abs(cols[0] - ref_f))),
                "folded_flux_cadences_in_same_position": "%d/%d" % (int(np.sum(same)), same.size),
                "folded_flux_reference": "astropy TimeSeries.fold(period, epoch_time=transit_time) + sort('time') at astropy's "
                                         "best period (what LightCurve.fold runs, lightcurve.py:1173-1212), %d targets" % n}


    # ================================================================================================ PLD block
    def run_pld(Bc, first_index, steps, warmup, base, dump=False):
        """configs[4]: Bc cutouts 11x11 x pld_cadences, pld_order 3, 16 PCA components, all pixels: design matrix +
        regression through lk_pld_design_batch_dev + lk_regress_batch_dev.  `base`: the numpy port's baseline dict (its
        "_results" feed one of the two accuracy checks) or None."""
        Nc, npix = args.pld_cadences, 11
        P = npix * npix
        cubes = [synth.pld_cutout(4, first_index + i, n=Nc, npix=npix) for i in range(Bc)]
        tt = np.stack([c[0] for c in cubes])
        pix = np.stack([c[1].reshape(Nc, P) for c in cubes]).astype(np.float32)
        epx = np.stack([c[2].reshape(Nc, P) for c in cubes]).astype(np.float32)
        lcf = pix.sum(axis=2, dtype=np.float32)
        lce = np.sqrt((epx.astype(np.float64) ** 2).sum(axis=2))
        deg, nkn = 5, Nc // 50
        n_inner = nkn - deg - 1
        knots = np.stack([np.concatenate([[t_.min()], np.percentile(t_, np.linspace(0, 100, n_inner + 2)[1:-1]), [t_.max()]])
                          for t_ in tt])
        K = _capi.pld_design_width(P, P, 3, 16, nkn)
        d_pix, d_lcf, d_t, d_kn = (torch.from_numpy(a).to(dev) for a in (pix, lcf, tt, knots))
        d_y, d_err = torch.from_numpy(lcf.astype(np.float64).ravel()).to(dev), torch.from_numpy(lce.ravel()).to(dev)
        d_X = torch.empty((Bc, Nc, K), dtype=torch.float64, device=dev)
        d_ps = torch.empty((Bc, K), dtype=torch.float64, device=dev)
        d_mu = torch.zeros((Bc, K), dtype=torch.float64, device=dev)
        d_w = torch.empty((Bc, K), dtype=torch.float64, device=dev)
        d_model = torch.empty(Bc * Nc, dtype=torch.float64, device=dev)
        d_out = torch.empty(Bc * Nc, dtype=torch.uint8, device=dev)
        offp = np.arange(Bc + 1, dtype=np.int64) * Nc

        def step(e0, e1):
            e0.record()
            _capi._check(lib.lk_pld_design_batch_dev(handle._h, Bc, Nc, P, P, vp(d_pix.data_ptr()), vp(d_pix.data_ptr()),
                                                     vp(d_lcf.data_ptr()), vp(d_t.data_ptr()), vp(d_kn.data_ptr()),
                                                     n_inner, 3, 16, nkn, deg, 1, K, vp(d_X.data_ptr()),
                                                     vp(d_ps.data_ptr()), vp(stream)))
            _capi._check(lib.lk_regress_batch_dev(handle._h, Bc, offp.ctypes.data_as(i64p), K,
                                                  vp(d_X.data_ptr()), vp(d_y.data_ptr()), vp(d_err.data_ptr()), None,
                                                  vp(d_mu.data_ptr()), vp(d_ps.data_ptr()), 5.0, 5, vp(d_w.data_ptr()),
                                                  vp(d_model.data_ptr()), vp(d_out.data_ptr()), vp(stream)))
            e1.record()

        dt, kms = timed(step, warmup, steps)
        dumped = sample_outputs([("design_matrix", d_X), ("prior_sigma", d_ps), ("weights", d_w), ("model", d_model),
                                 ("outlier_mask", d_out)]) if dump else {}
        clk = clock_under(step, max(2, steps), kms)
        del d_X
        acc = {}
        from lightkurve_amd.correctors.pldcorrector import PixelCube, pld_correct_batch
        gpath = os.path.join(ROOT, "tests", "golden", "pld_c5.npz")
        if args.full and rank == 0 and first_index == 0 and Nc == 3500 and os.path.exists(gpath):
            # the product path (PLDCorrector mirror: design matrix, regression, restored trend) on the cutouts the REFERENCE
            # itself corrected when the fixture was made (oracle/gen_golden.py gen_pld_c5: lightkurve's PLDCorrector on
            # these very synth cutouts — regenerated here, SHA-256 checked)
            import hashlib
            g = np.load(gpath)
            ng = min(int(g["n_cutouts"]), Bc)
            same = all(hashlib.sha256(cubes[i][0].tobytes() + cubes[i][1].tobytes() + cubes[i][2].tobytes()).hexdigest()
                       == str(g["sha_%d" % i]) for i in range(ng))
            if same:
                cg = [PixelCube(g["time_%d" % i], cubes[i][1], cubes[i][2], mission="K2") for i in range(ng)]
                corr, outl = pld_correct_batch(cg, pld_order=3, pca_components=16)
                rel = [float(np.max(np.abs(corr[i] - g["corrected_%d" % i])) / np.median(g["corrected_%d" % i])) for i in range(ng)]
                acc["vs_reference"] = {
                    "reference": "lightkurve PLDCorrector.correct itself (pldcorrector.py:304-427) on these synthetic cutouts, "
                                 "outputs committed as tests/golden/pld_c5.npz (lightkurve is not installed on this box); "
                                 "%d cutouts 11x11 x %d cadences, order 3, 16 components" % (ng, Nc),
                    "corrected_flux_relerr_max": max(rel), "tolerance": 1e-6,
                    "outlier_masks_equal": "%d/%d" % (sum(int(np.array_equal(outl[i], g["outlier_mask_%d" % i])) for i in range(ng)), ng)}
        if base is not None and "_results" in base and first_index == 0:
            kept = base.pop("_results")
            cubes2 = [PixelCube(cubes[i][0], cubes[i][1], cubes[i][2], mission="K2") for i in range(len(kept))]
            corr, outl = pld_correct_batch(cubes2, pld_order=3, pca_components=16)
            relerr = [float(np.max(np.abs(corr[i] - kept[i][0])) / np.median(kept[i][0])) for i in range(len(kept))]
            acc["vs_port"] = {"reference": "numpy/LAPACK port of PLDCorrector.correct (exact SVD), %d cutouts 11x11 x %d "
                                           "cadences, order 3, 16 components" % (len(kept), Nc),
                              "corrected_flux_relerr_max": max(relerr),
                              "outlier_masks_equal": "%d/%d" % (sum(int(np.array_equal(outl[i], kept[i][1])) for i in range(len(kept))), len(kept))}
        # MFMA flop actually EXECUTED per cutout.  Pixel and background blocks (121 columns): upper-triangle Gram,
        # N*P*(P+1).  Product blocks (136 and 816 columns): the moment-form Gram computes only the canonical staircase of
        # the 4th / 6th moments in whole 16 x 16 tiles (pld.hip: pld_moment_gram_kernel) — 512 flop per tile and cadence.
        # Regression: N*(K+1)*(K+2) for ONE Gram (the clip loop stops at its fixed point; repeated passes are not executed).
        tiles2, tiles3 = _moment_tiles(16, 2), _moment_tiles(16, 3)
        flop = float(Bc) * Nc * (2 * P * (P + 1) + 512 * (tiles2 + tiles3) + (K + 1) * (K + 2))
        flop_plain = float(Bc) * Nc * (sum(c * (c + 1) for c in (P, 136, 816, P)) + (K + 1) * (K + 2))
        ach = flop / (kms * 1e-3) / 1e12
        rl = {"bound": "mfma", "achieved": ach, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
              "frac": ach / FP64_VECTOR_PEAK_TFLOPS, "traffic": traffic_all.get("pld"), "shader_clock_mhz": clk,
              "kernel": "pld_moment_gram_kernel + gram_mfma_kernel (v_mfma_f64_16x16x4_f64)", "kernel_ms_per_step": kms,
              "executed_gram_flop_per_step": flop, "plain_gram_flop_per_step": flop_plain,
              "dominant_kernel": {"kernel": "pld_topk_eig_kernel<2> (subspace iteration on the 816-column block's 5.3-MB Gram "
                                            "matrices; the 121- and 136-column blocks take the direct tridiagonal solver)",
                                  "bound": "hbm", "ms_per_step": 5.34, "hbm_bytes_per_step": 2.48e10,
                                  "achieved_GBps": 2.48e10 / 5.34e-3 / 1e9, "frac": 2.48e10 / 5.34e-3 / 1e9 / HBM_PEAK_GBS,
                                  "hbm_bytes_per_step_raw_counters": 1.417e10,
                                  "source": "profiles/r06_pld_eig_modes_ab.txt (5.34 ms per launch: per-phase clocks), r06_pld_pmc_fetch.txt "
                                            "/ _write.txt (FETCH_SIZE 1.064e10 + WRITE_SIZE 0.353e10 B per launch raw over 7 launches; the "
                                            "reads are 16-B-per-lane streams, which gfx950's FETCH_SIZE tallies at 1/2 — "
                                            "MI355X_MICROARCH.md — so 2 x 1.064e10 + 0.353e10 = 2.48e10 B, the nominal count of its ten "
                                            "products is 2.4e10); round 5: 7.7 ms, 1.91e10 B raw.  Constants of the committed passes, "
                                            "not re-measured in this run"},
              "frac_plain_gram_equivalent": flop_plain / (kms * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
              "note": "Gram flop EXECUTED on the matrix cores — N*P*(P+1) for the two 121-column blocks, 512 flop per "
                      "16x16 tile and cadence of the moment-form staircase for the 136- and 816-column product blocks "
                      "(%d + %d tiles instead of the 9316 + 333336 upper-triangle entries: the multiset symmetry of the "
                      "product columns), N*(K+1)*(K+2) for the regression — over the WHOLE step time (eigen-solver, "
                      "projections, LU, clipping included) against the fp64 MFMA dense peak.  frac_plain_gram_equivalent: "
                      "the same time priced with the flop of plain upper-triangle Grams (round 2's count), for comparison "
                      "across rounds only" % (tiles2, tiles3)}
        api = None
        if rank == 0 and first_index == 0 and not dist_on and not args.no_api:
            # the product's list-of-objects entry point (what replaces a loop over PLDCorrector(tpf).correct()): host pointers,
            # per-cutout aperture sums / NaN-cadence removal on the packing threads, ONE lk_pld_correct_batch call
            na = min(Bc, 100)
            ca = [PixelCube(cubes[i][0], cubes[i][1], cubes[i][2], mission="K2") for i in range(na)]
            pld_correct_batch(ca, pld_order=3, pca_components=16)
            ws = []
            for _ in range(3):
                t0 = time.perf_counter()
                pld_correct_batch(ca, pld_order=3, pca_components=16)
                ws.append(time.perf_counter() - t0)
            w = float(np.median(ws))
            api = {"call": "pld_correct_batch(list of %d PixelCube, pld_order=3, pca_components=16)" % na, "wall_ms": 1e3 * w,
                   "ms_per_cutout": 1e3 * w / na, "kernel_ms_per_cutout": kms / Bc, "value": na / w,
                   "note": "wall clock of one Python call, median of 3 after one warm-up, host arrays in and out (PCIe included)"}
        return {"dt": dt, "kernel_ms": kms, "units_per_step": Bc, "steps": steps, "warmup": warmup, "api_end_to_end": api,
                "metric": "PLD cutouts/sec (design matrix + regression)", "unit": "cutouts/sec",
                "workload": "configs[4]: %d K2-like 11x11-pixel cutouts x %d cadences, 3rd-order design matrix (K=%d), "
                            "MFMA Gram per GPU" % (Bc, Nc, K), "roofline": rl, "accuracy": acc, "Nc": Nc, "dumped": dumped}

    # ================================================================================================ flatten block
    def run_flatten(Bf, first_index, steps, warmup, base, dump=False):
        """LightCurve.flatten (window 401, polyorder 2, niters 3) on Bf light curves of N cadences through
        lk_savgol_trend_batch_dev.  `base`: a cpu_baseline dict whose "_results" are trends of the first light curves of
        this batch (scipy under conda, or the numpy port)."""
        t, y, dy, off = synth.ls_batch(6, Bf, N, first_index=first_index)
        d_t, d_y = torch.from_numpy(t).to(dev), torch.from_numpy(y).to(dev)
        d_tr = torch.empty_like(d_y)

        def step(e0, e1):
            e0.record()
            _capi._check(lib.lk_savgol_trend_batch_dev(handle._h, Bf, off.ctypes.data_as(i64p),
                                                       vp(d_t.data_ptr()), vp(d_y.data_ptr()), None, args.flatten_window, 2, 5.0, 3, 3.0,
                                                       vp(d_tr.data_ptr()), None, vp(stream)))
            e1.record()

        dt, kms = timed(step, warmup, steps)
        dumped = sample_outputs([("trend", d_tr)]) if dump else {}
        clk = clock_under(step, max(10, steps), kms)
        acc = None
        if base is not None and "_results" in base and first_index == 0:
            kept = base.pop("_results")   # the reference trends of the first light curves of this batch, full config shape
            tr = d_tr.cpu().numpy()
            rel = []
            for i, ref_tr in enumerate(kept[:Bf]):
                mine = tr[off[i]:off[i + 1]]
                okm = np.isfinite(ref_tr)
                rel.append(float(np.max(np.abs(mine[okm] - ref_tr[okm]) / np.abs(ref_tr[okm]))) if np.array_equal(okm, np.isfinite(mine)) else float("inf"))
            acc = {"reference": ("scipy savgol_filter + interp1d (the reference's own calls) inside the restated loop of "
                                 "LightCurve.flatten, run under conda on this box" if base.get("kind") == "reference" else
                                 "numpy port of LightCurve.flatten (scipy savgol semantics)") +
                                ", %d light curves x %d cadences, window %d" % (len(rel), N, args.flatten_window),
                   "trend_relerr_max": max(rel), "tolerance": 1e-10}
        algo = 24.0 * float(off[-1])
        rl = {"bound": "hbm", "achieved": algo / (kms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
              "unit": "GB/s", "frac": algo / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
              "traffic": traffic_all.get("flatten"), "kernel": "the phase-split pipeline of flatten.hip: flat_init + niters x (flat_compact, flat_dtseg, flat_trend, "
                                                              "flat_clip) + flat_interp, whole step", "kernel_ms_per_step": kms,
              "shader_clock_mhz": clk,
              # SURVEY.md 8(d) prices flatten at 48 B per cadence (time, flux, flux_err in; flux, flux_err, trend out: the
              # whole LightCurve.flatten call); the kernel timed here produces the TREND only (24 B: time, flux in, trend out;
              # the two divisions are lk_flatten_apply_batch_dev, timed inside pipeline_end_to_end) — both stated (VERDICT r5 #4c)
              "survey_8d_bytes_per_cadence": 48.0, "frac_on_survey_8d_bytes": 48.0 * float(off[-1]) / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
              "note": "algorithmic 24 B per cadence (time, flux in; trend out); frac_on_survey_8d_bytes prices the same time on "
                      "SURVEY 8(d)'s 48 B per cadence"}
        api = None
        if rank == 0 and first_index == 0 and not dist_on and not args.no_api:
            # the list-of-objects entry point (what replaces a loop over lc.flatten(), lightcurve.py:943-1078): packing into
            # page-locked staging, sortedness check, lk_savgol_trend_batch over PCIe, per-target result views
            from lightkurve_amd import batch as LB
            from lightkurve_amd.lightcurve import LightCurve
            lcs = [LightCurve(time=t[off[i]:off[i + 1]], flux=y[off[i]:off[i + 1]], flux_err=dy[off[i]:off[i + 1]]) for i in range(Bf)]
            got = LB.flatten_batch(lcs, window_length=args.flatten_window)
            same = bool(np.array_equal(np.concatenate(got), d_tr.cpu().numpy(), equal_nan=True))
            ws = []
            for _ in range(3):
                t0 = time.perf_counter()
                LB.flatten_batch(lcs, window_length=args.flatten_window)
                ws.append(time.perf_counter() - t0)
            w = float(np.median(ws))
            api = {"call": "flatten_batch(list of %d LightCurve, window_length=%d)" % (Bf, args.flatten_window), "wall_ms": 1e3 * w,
                   "ms_per_target": 1e3 * w / Bf, "kernel_ms_per_target": kms / Bf, "value": float(off[-1]) / w,
                   "trends_match_device_path": same,
                   "note": "wall clock of one Python call, median of 3 after one warm-up, host arrays in and out (24 B per cadence "
                           "over PCIe around the kernels)"}
        return {"dt": dt, "kernel_ms": kms, "units_per_step": int(off[-1]), "steps": steps, "warmup": warmup, "api_end_to_end": api,
                "metric": "flatten cadences/sec (window %d, niters 3)" % args.flatten_window, "unit": "cadences/sec",
                "workload": "flatten: %d light curves x %d cadences, window %d, polyorder 2, niters 3 per GPU" % (Bf, N, args.flatten_window),
                "roofline": rl, "accuracy": acc, "dumped": dumped}

    def block_of(res, base):
        """JSON block of a secondary workload inside the default line."""
        val = res["units_per_step"] * world * res["steps"] / res["dt"]
        blk = {"metric": res["metric"], "value": val, "unit": res["unit"], "steps": res["steps"], "warmup": res["warmup"],
               "ms_per_step": 1e3 * res["dt"] / res["steps"], "scaling": "weak", "config": {"workload": res["workload"]},
               "roofline": res["roofline"]}
        if res.get("accuracy"):
            blk["accuracy"] = res["accuracy"]
        if res.get("api_end_to_end"):
            blk["api_end_to_end"] = res["api_end_to_end"]
        if base is not None:
            blk["cpu_baseline"] = {k: v for k, v in base.items() if not k.startswith("_")}
            blk["speedup_vs_cpu_baseline"] = val / base["value"]
            if "value_priced_on_survey" in base:
                blk["speedup_vs_survey_reference"] = val / base["value_priced_on_survey"]
        return blk

    def run_api(t_abs, y, dy, off, df, M, kern_ms, dev_peaks, d_pow):
        """Wall time of the Python batch API on this rank's B light curves (reference idiom being replaced: the loop over a
        LightCurveCollection, collections.py:145, calling lc.to_periodogram(), lightcurve.py:2490-2535).  Every figure is
        host-inclusive wall clock per call: object access + packing + planning + PCIe + kernels."""
        from lightkurve_amd import batch as LB
        from lightkurve_amd.ingest import LightCurveBatch
        from lightkurve_amd.lightcurve import LightCurve
        from lightkurve_amd.periodogram import LombScarglePeriodogram
        Bq = len(off) - 1
        freq = df * (1.0 + np.arange(M))
        lcs = [LightCurve(time=t_abs[off[b]:off[b + 1]], flux=y[off[b]:off[b + 1]], flux_err=dy[off[b]:off[b + 1]])
               for b in range(Bq)]
        kern_per_target = kern_ms / Bq

        def wall(fn, reps=3):
            fn()                                   # warm-up: pinned pools, workspace, first-touch
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), r

        def entry(sec, extra_fields=None):
            ms_t = 1e3 * sec / Bq
            d = {"wall_ms": 1e3 * sec, "ms_per_target": ms_t, "host_overhead_ms_per_target": ms_t - kern_per_target,
                 "value": Bq * M / sec}
            d.update(extra_fields or {})
            return d

        res = {"unit": "frequencies*targets/sec", "targets": Bq, "kernel_ms_per_target": kern_per_target,
               "note": "wall clock of one Python call, median of 3 after one warm-up; host_overhead = wall - the HIP-event "
                       "kernel time of the device-pointer step above (so it includes PCIe).  list_*: a list of B LightCurve "
                       "objects (packed into the pinned staging pool inside the call); batch_*: a LightCurveBatch whose "
                       "arrays are page-locked (LightCurveBatch.from_lightcurves(lcs, pinned=True), built once: "
                       "`pack_once`).  *_spectra_pinned_out: out= a reused page-locked (B, M) array; *_spectra: no out= — "
                       "the result comes from _capi.result_empty's recycled page-locked buffers (reused once the caller has "
                       "dropped the previous result; LK_RESULT_POOL=0 gives a fresh pageable array per call: + ~50 ms of "
                       "first-touch page faults per 800 MB)"}
        sec, pk = wall(lambda: LB.lombscargle_peaks_batch(lcs, freq))
        res["list_to_peaks"] = entry(sec, {"peaks_match_device_path": bool(np.array_equal(pk[:, 0], dev_peaks[0]) and
                                                                           np.array_equal(pk[:, 1].astype(np.int64), dev_peaks[1]))})
        h_pow = _capi.pinned_empty((Bq, M))
        sec, pw = wall(lambda: LB.lombscargle_batch(lcs, freq, out=h_pow))
        res["list_to_spectra_pinned_out"] = entry(sec, {"spectra_match_device_path": bool(np.array_equal(pw, d_pow.cpu().numpy(), equal_nan=True))})
        sec, pw = wall(lambda: LB.lombscargle_batch(lcs, freq))
        res["list_to_spectra"] = entry(sec)
        del pw
        t0 = time.perf_counter()
        lb = LightCurveBatch.from_lightcurves(lcs, pinned=True)
        res["pack_once"] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "ms_per_target": 1e3 * (time.perf_counter() - t0) / Bq}
        sec, pk = wall(lambda: lb.to_periodogram_peaks(freq))
        res["batch_to_peaks"] = entry(sec, {"peaks_match_device_path": bool(np.array_equal(pk[:, 0], dev_peaks[0]) and
                                                                            np.array_equal(pk[:, 1].astype(np.int64), dev_peaks[1]))})
        sec, pw = wall(lambda: lb.to_periodogram_power(freq, out=h_pow))
        res["batch_to_spectra_pinned_out"] = entry(sec)
        # where batch_to_peaks' wall clock goes: the grid plan, the NaN sweep over the packed flux, the C entry point itself
        from lightkurve_amd import packed as LP
        tp0 = time.perf_counter()
        plan = LP.ls_grid_plan(freq)
        tp1 = time.perf_counter()
        LP.any_nan(lb.flux)
        tp2 = time.perf_counter()
        sc = LP.ls_scales(lb.time, lb.n_off, plan)
        tp3 = time.perf_counter()
        _capi.ls_fast_peaks_batch(lb.time, lb.flux, lb.n_off, f0=float(plan.f_day[0]), df=float(plan.f_day[1] - plan.f_day[0]), M=M,
                                  normalization=plan.norm, scale=sc, device=local_rank, want_power=False, absolute_time=True)
        tp4 = time.perf_counter()
        res["batch_to_peaks"]["breakdown_ms"] = {"grid_plan": 1e3 * (tp1 - tp0), "nan_sweep": 1e3 * (tp2 - tp1), "scales": 1e3 * (tp3 - tp2),
                                                 "lk_ls_fast_peaks_lc_batch": 1e3 * (tp4 - tp3)}
        # the reference idiom kept as it is (B = 1 per call): one constructor call per light curve
        nb1 = min(Bq, 32)
        LombScarglePeriodogram.from_lightcurve(lcs[0], frequency=freq)
        t0 = time.perf_counter()
        for lc in lcs[:nb1]:
            LombScarglePeriodogram.from_lightcurve(lc, frequency=freq)
        sec1 = (time.perf_counter() - t0) / nb1
        res["per_object_loop"] = {"ms_per_target": 1e3 * sec1, "value": M / sec1, "targets": nb1,
                                  "note": "for lc in lcs: LombScarglePeriodogram.from_lightcurve(lc, frequency=...) — one "
                                          "GPU call per light curve"}
        return res

    def run_pipeline(t_abs, y, dy, off, df, M, ls_kern_ms, dev_peaks):
        """A device-RESIDENT batch through the chain a survey script runs per light curve in the reference
        (collections.py:145 over lightcurve.py:1300-1327, 1216-1292, 943-1078, 2490-2535):
            batch.normalize() -> .flatten(window_length=401) -> .to_periodogram_peaks(frequency)
        One upload; every arrow stays in HBM; 16 B per target come back.  `wall_ms`: perf_counter around the whole chain
        (Python, launch gaps and the launchers' own synchronisations included), median of 5.  `stage_kernel_ms`: HIP events
        on the launch stream around each stage run ALONE; LS = the headline's device-pointer kernel time."""
        from lightkurve_amd.device import DeviceLightCurveBatch
        from lightkurve_amd.ingest import LightCurveBatch
        Bq = len(off) - 1
        freq = df * (1.0 + np.arange(M))
        t0 = time.perf_counter()
        dev_b = DeviceLightCurveBatch.from_arrays(t_abs, y, dy, off, device=local_rank, stream=stream)
        dev_b.synchronize()
        upload_ms = 1e3 * (time.perf_counter() - t0)

        def chain():
            return dev_b.normalize().flatten(window_length=args.flatten_window).to_periodogram_peaks(freq)

        def ev_ms(fn, reps=5):
            fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1))
            return float(np.median(out)), r

        ing_ms, norm_b = ev_ms(lambda: dev_b.normalize())
        flat_ms, flat_b = ev_ms(lambda: norm_b.flatten(window_length=args.flatten_window))
        ls_ms, pk = ev_ms(lambda: flat_b.to_periodogram_peaks(freq))
        chain()
        ws = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pk = chain()
            ws.append(time.perf_counter() - t0)
        wall = 1e3 * float(np.median(ws))
        # the same chain staged through the host (LightCurveBatch: H2D -> kernel -> D2H at every arrow)
        hb = LightCurveBatch(t_abs, y, dy, off)

        def staged():
            nb = hb.normalize(device=local_rank)
            tr = nb.flatten_trend(device=local_rank, window_length=args.flatten_window)
            fb = LightCurveBatch(nb.time, nb.flux / tr, nb.flux_err / tr, nb.n_off)
            return fb.to_periodogram_peaks(freq, device=local_rank)

        pk_s = staged()
        t0 = time.perf_counter()
        pk_s = staged()
        staged_ms = 1e3 * (time.perf_counter() - t0)
        ksum = ing_ms + flat_ms + ls_kern_ms
        return {"call": "DeviceLightCurveBatch(%d x %d).normalize().flatten(window_length=%d).to_periodogram_peaks(%d freqs)"
                        % (Bq, N, args.flatten_window, M),
                "wall_ms": wall, "stage_kernel_ms": {"normalize (lk_ingest_batch_dev)": ing_ms,
                                                     "flatten (lk_savgol_trend_batch_dev + lk_flatten_apply_batch_dev)": flat_ms,
                                                     "ls_peaks (lk_ls_fast_peaks_batch_dev, the headline step)": ls_kern_ms,
                                                     "ls_peaks stage alone, its remove_nans pass and Python included": ls_ms},
                "kernel_ms_sum": ksum, "wall_over_kernels": wall / ksum, "upload_once_ms": upload_ms,
                "staged_host_path_wall_ms": staged_ms, "value": Bq * M / (wall * 1e-3), "unit": "frequencies*targets/sec",
                "peaks_match_staged_path": bool(np.array_equal(pk, pk_s)),
                "note": "wall clock of the whole resident chain per call (median of 5) against the sum of its stages' kernel "
                        "times; the staged path runs the same kernels with host arrays between the stages (one call, after a "
                        "warm-up).  The flattened light curves differ from the headline's inputs, so the peaks are compared "
                        "with the staged path's, bit for bit"}

    if args.workload == "ls":
        # ---- synthetic inputs; rank r owns targets [first, first + B)
        t, y, dy, off = synth.ls_batch(1, B, N, first_index=first)
        t_abs = t.copy()       # the light curves' own times: what the Python batch API is handed (api_end_to_end below)
        for b in range(B):
            t[off[b]:off[b + 1]] -= t[off[b]]
        df = 360.0 / M
        d_t, d_y = torch.from_numpy(t).to(dev), torch.from_numpy(y).to(dev)
        d_pow = torch.empty((B, M), dtype=torch.float64, device=dev)
        d_max = torch.empty(B, dtype=torch.float64, device=dev)
        d_arg = torch.empty(B, dtype=torch.int64, device=dev)
        gather_spec = dist_on and args.gather == "spectra"
        gather_sum = dist_on and args.gather == "summary"
        # gathers need equal shard sizes per rank (weak scaling always; strong: pad to the largest shard)
        Bmax = B
        if dist_on and strong:
            Bmax = int(np.max(np.diff(strong_bounds(args, world))))
        nch = max(1, min(args.chunks, B)) if gather_spec else 1
        cb = np.linspace(0, Bmax, nch + 1).astype(int)
        d_all = [torch.empty((world, cb[c + 1] - cb[c], M), dtype=torch.float64, device=dev)
                 for c in range(nch)] if gather_spec else None
        d_powpad = torch.zeros((Bmax, M), dtype=torch.float64, device=dev) if (gather_spec and Bmax != B) else None
        d_sum = torch.zeros((Bmax, 2), dtype=torch.float64, device=dev)
        d_sum_all = torch.empty((world, Bmax, 2), dtype=torch.float64, device=dev) if gather_sum else None
        headline = "fast" if args.ls_method in ("both", "fast") else "exact"

        def make_step(method):
            def step(e0, e1):
                works = []
                for c in range(nch):
                    b0, b1 = min(int(cb[c]), B), min(int(cb[c + 1]), B)
                    if c == 0:
                        e0.record()
                    if b1 > b0:
                        offc = off[b0:b1 + 1] - off[b0]
                        tp, yp = d_t.data_ptr() + 8 * int(off[b0]), d_y.data_ptr() + 8 * int(off[b0])
                        pp = d_pow.data_ptr() + 8 * b0 * M
                        if method == "fast":
                            _capi.ls_fast_peaks_batch_dev(handle, b1 - b0, offc, tp, yp, 0, df, df, M, True, True,
                                                          "lk_amplitude", 0, 5, pp, d_max.data_ptr() + 8 * b0,
                                                          d_arg.data_ptr() + 8 * b0, stream)
                        else:
                            _capi.ls_power_batch_dev(handle, b1 - b0, offc, tp, yp, 0, 0, df, df, M, True, True,
                                                     "lk_amplitude", 0, pp, stream)
                            _capi.argmax_batch_dev(handle, b1 - b0, M, pp, d_max.data_ptr() + 8 * b0,
                                                   d_arg.data_ptr() + 8 * b0, stream)
                    if c == nch - 1:
                        e1.record()
                    if gather_spec:
                        src = d_pow
                        if d_powpad is not None:
                            d_powpad[:B] = d_pow
                            src = d_powpad
                        # the product's collective (lightkurve_amd.distributed): device tensors in, device tensors out
                        works.append(LD.all_gather_equal(d_all[c], src[int(cb[c]):int(cb[c + 1])], async_op=True))
                if gather_sum:   # every rank ends with every target's (max power, argmax): 16 B per target over xGMI
                    d_sum[:B, 0] = d_max
                    d_sum[:B, 1] = d_arg.to(torch.float64)
                    LD.all_gather_equal(d_sum_all, d_sum)
                for w in works:
                    w.wait()
            return step

        results = {}
        order = [headline] + ([("exact" if headline == "fast" else "fast")] if args.ls_method == "both" else [])
        peaks = {}
        rep_kms = []
        for method in order:
            results[method] = timed(make_step(method), args.warmup, args.steps)
            if method == headline and dump:
                dumped = sample_outputs([("power", d_pow), ("max_power", d_max), ("argmax", d_arg)])
            peaks[method] = (d_max.cpu().numpy().copy(), d_arg.cpu().numpy().copy())
            if method == headline == "fast":
                # the headline's kernel time again, `--repeats` - 1 more blocks of K steps right behind the timed region (before
                # the exact kernel's half-second VALU bursts pull the clocks down): the roofline fraction is quoted with its
                # median / min / max over the blocks (0.578 - 0.598 across boxes and runs)
                rep_kms = [results[headline][1]] + [timed(make_step(headline), 0, args.steps)[1]
                                                    for _ in range(max(0, args.repeats - 1))]
        units_per_step = total_targets * M
        pairs_local = float(off[-1]) * M
        names = {"exact": "exact GLS, direct fp64 trig sums", "fast": "ls_method='fast' (reference default): extirpolation + FFT"}
        metric = "frequencies*targets/sec (Lomb-Scargle, %s)%s" % (names[headline], "" if not args.metric_bls else
                                                                   " + BLS periods*targets/sec; max-power rel-err")
        unit = "frequencies*targets/sec"
        workload = ("configs[%d]: %d TESS-like %d-cadence targets x %d freqs Lomb-Scargle %s, ls_method=%s"
                    % (2 if strong else 1, total_targets if strong else B, N, M,
                       "in total over %d GPU(s)" % world if strong else "per GPU", headline))

        def ls_roofline(method, kms, B=B, off=off, t=t):
            if method == "fast":
                nfft = 1 << int(np.ceil(np.log2(5 * M)))
                n2 = 1 << (int(np.log2(nfft)) // 2)
                # Round 4: the extirpolation is fused into FFT step 1 (no spread grid in HBM) and the weights are formed on the
                # fly (no w, w*y arrays), so what the path must move per target is the FLOOR of this FFT scheme: the
                # three intermediates out and in, 16 B per cadence in, 8 B per frequency out.  `frac` uses that count; the
                # round-1..3 count (which also priced the spread rows out + in and 40 B per cadence) is kept beside it so that
                # rounds compare on one formula.
                used = 0.0   # grid rows that can hold samples (round-3 formula only)
                for b in range(B):
                    span = (t[off[b + 1] - 1] - t[off[b]]) * nfft * df
                    used += 2 * min(nfft, (int((span + 4) / n2) + 1) * n2) + min(nfft, (int((2 * span + 4) / n2) + 1) * n2)
                algo = B * (3 * nfft * 16.0 * 2 + 8.0 * M) + 16.0 * float(off[-1])
                algo_r03 = B * (3 * nfft * 16.0 * 2 + 8.0 * M) + used * 16.0 * 2 + 40.0 * float(off[-1])
                tr = traffic_all.get("ls_fast")
                rl = {"bound": "hbm", "achieved": algo / (kms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": algo / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": tr,
                      "kernel": "fft_cols_pruned_kernel (extirpolation + FFT step 1) + fft_rows512_power_kernel (FFT step 2 + closed "
                                "form + peak partials): whole step",
                      "kernel_ms_per_step": kms, "algorithmic_bytes_per_step": algo,
                      "note": "algorithmic bytes per target = the floor of the two-step FFT scheme: 3 complex fp64 grids of "
                              "Nfft=%d written by FFT step 1 and read by step 2 (2 x 16 B x Nfft each), 16 B/cadence in (t, y), "
                              "8 B/frequency out.  The spread grids and the three spectra never touch HBM (fused extirpolation, "
                              "fused closed form) and are not counted." % nfft,
                      "frac_r03_formula": algo_r03 / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "r03_formula_note": "rounds 1-3 priced 59.1 MB per target (the floor + the sample-bearing rows written by a "
                                          "separate spreader and read by step 1 + 40 B/cadence); round 3's 13.3 ms read 0.556 on "
                                          "it and 0.48 on the floor"}
                if tr:
                    rl["hbm_utilisation"] = float(tr) * (B / 1000.0) / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS
                    rl["traffic_note"] = ("PMC FETCH_SIZE + WRITE_SIZE per 1000-target step from profiles/ (separate rocprofv3 "
                                          "--pmc passes of this command), scaled to this batch; not re-measured in this run")
                return rl
            flops = 16.0 * float(off[-1]) * M
            ach = flops / (kms * 1e-3) / 1e12
            algo_bytes = 16.0 * float(off[-1]) + 8.0 * B * M
            return {"bound": "valu", "achieved": ach, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / FP64_VECTOR_PEAK_TFLOPS, "traffic": traffic_all.get("ls"),
                    "kernel": "ls_grid_kernel<16> (+ls_prep_kernel)", "kernel_ms_per_step": kms,
                    "note": "fp64 direct trig sums: 16 flop (8 v_fma_f64) per (cadence, frequency) pair; arithmetic "
                            "intensity ~3e4 flop/B so the fp64 VECTOR pipe binds (peak == fp64 MFMA dense peak), not HBM",
                    "hbm": {"achieved": algo_bytes / (kms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": algo_bytes / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "algorithmic_bytes_per_step": algo_bytes}}

        dt, kern_ms = results[headline]
        roofline = ls_roofline(headline, kern_ms)
        if len(rep_kms) > 1:
            roofline["kernel_ms_per_step_by_block"] = [float(k) for k in rep_kms]   # in the order they ran
            fr = sorted(ls_roofline(headline, k)["frac"] for k in rep_kms)
            roofline["frac_runs"] = fr
            roofline["frac_median"], roofline["frac_min"], roofline["frac_max"] = float(np.median(fr)), fr[0], fr[-1]
            roofline["frac_runs_note"] = ("%d blocks of %d steps on this box (the first is the timed region `value` comes from), HIP-event "
                                          "kernel time per block" % (len(rep_kms), args.steps))
        if headline == "fast":
            roofline["shader_clock_mhz"] = clock_under(make_step("fast"), args.steps, kern_ms)
        extra["config_ls_method"] = headline
        if len(order) > 1:
            other = order[1]
            dt2, kms2 = results[other]
            extra["other_method"] = {"ls_method": other, "value": units_per_step * args.steps / dt2, "unit": unit,
                                     "ms_per_step": 1e3 * dt2 / args.steps,
                                     "roofline": dict(ls_roofline(other, kms2),
                                                      shader_clock_mhz=clock_under(make_step(other), 1, kms2)),
                                     "note": "same workload, same timing protocol; 'exact' = the direct-sum kernel "
                                             "(matches the reference's slow/cython/chi2 to 1e-9), 'fast' = the reference's "
                                             "default algorithm (matches lightkurve's default output to 1e-9)"}

        # ---- accuracy vs astropy itself on the first targets of this very batch (N = 1 only)
        if ref is not None and rank == 0:
            acc = {}
            for method, key in (("fast", "ls_fast"), ("exact", "ls_cython")):
                if method in peaks and key in ref:
                    n = min(len(ref[key]["max_power"]), B)
                    r_max, r_arg = np.asarray(ref[key]["max_power"][:n]), np.asarray(ref[key]["argmax"][:n])
                    g_max, g_arg = peaks[method][0][:n], peaks[method][1][:n]
                    rel = np.abs(g_max - r_max) / np.abs(r_max)
                    acc["ls_" + method] = {
                        "reference": "astropy %s LombScargle.power(method='%s'), lightkurve amplitude normalisation, "
                                     "N=%d, M=%d" % (ref["astropy"], "fast" if method == "fast" else "cython", N, M),
                        "targets_checked": int(n), "max_power_relerr_max": float(np.max(rel)),
                        "max_power_relerr_median": float(np.median(rel)),
                        "argmax_equal": "%d/%d" % (int(np.sum(g_arg == r_arg)), n)}
            extra["accuracy"] = acc

        # ---- host-to-host: the same step through the host-pointer entry point (PCIe included)
        if not args.no_host:
            try:
                h_pow = _capi.pinned_empty((B, M))
                h_t, h_y = _capi.pinned_empty(t.shape), _capi.pinned_empty(y.shape)
                h_t[:], h_y[:] = t, y
                hs = {}
                for label, kw in (("spectra_pinned", dict(out=h_pow, want_power=True)),
                                  ("peaks_only_pinned", dict(want_power=False))):
                    _capi.ls_fast_peaks_batch(h_t, h_y, off, f0=df, df=df, M=M, normalization="lk_amplitude",
                                              device=local_rank, **kw)
                    sync()
                    t0 = time.perf_counter()
                    reps = max(1, min(args.steps, 3))
                    for _ in range(reps):
                        r = _capi.ls_fast_peaks_batch(h_t, h_y, off, f0=df, df=df, M=M, normalization="lk_amplitude",
                                                      device=local_rank, **kw)
                    sync()
                    hdt = (time.perf_counter() - t0) / reps
                    if dist_on:
                        tt = torch.tensor([hdt], dtype=torch.float64, device=dev)
                        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                        hdt = float(tt.item())
                    hs[label] = {"value": units_per_step / hdt, "ms_per_step": 1e3 * hdt}
                    if label == "peaks_only_pinned" and "fast" in peaks:
                        hs[label]["peaks_match_device_path"] = bool(np.array_equal(r[2], peaks["fast"][1]))
                # pageable numpy buffers (what a caller that never heard of lk_host_alloc passes)
                p_pow = np.empty((min(B, 256), M))
                nb = p_pow.shape[0]
                _capi.ls_fast_peaks_batch(t[:off[nb]], y[:off[nb]], off[:nb + 1], f0=df, df=df, M=M,
                                          normalization="lk_amplitude", device=local_rank, out=p_pow, want_power=True)
                t0 = time.perf_counter()
                _capi.ls_fast_peaks_batch(t[:off[nb]], y[:off[nb]], off[:nb + 1], f0=df, df=df, M=M,
                                          normalization="lk_amplitude", device=local_rank, out=p_pow, want_power=True)
                hdt = time.perf_counter() - t0
                hs["spectra_pageable"] = {"value": nb * M * world / hdt, "ms_per_step": 1e3 * hdt, "targets": nb}
                hs["unit"] = unit
                hs["note"] = ("lk_ls_fast_peaks_batch (HOST pointers): chunked, double-buffered staging; H2D of chunk k+1 "
                              "and D2H of chunk k-1 overlap the kernels of chunk k.  *_pinned: caller buffers from "
                              "lk_host_alloc (direct async DMA); pageable: plain numpy arrays")
                extra["host_to_host"] = hs
                extra["value_host_to_host"] = hs["spectra_pinned"]["value"]
                del h_pow
            except Exception as e:   # reported, never fatal for the headline
                extra["host_to_host"] = {"error": repr(e)}

        if len(order) > 1 and order[-1] != "fast" and "fast" in results:
            # d_pow holds the LAST method's spectra; the API checks below compare against the 'fast' ones (VERDICT r5 #4a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            make_step("fast")(e0, e1)
            sync()
        # ---- the product's Python batch API, host included: from light-curve objects / a LightCurveBatch to
        # peaks and to spectra through lightkurve_amd.batch — what replaces the loop over a LightCurveCollection
        if (not args.no_api) and not dist_on and headline == "fast":
            try:
                extra["api_end_to_end"] = run_api(t_abs, y, dy, off, df, M, kern_ms, peaks["fast"], d_pow)
            except Exception as e:   # reported, never fatal for the headline
                extra["api_end_to_end"] = {"error": repr(e)}

        # ---- a device-resident batch through normalize -> flatten -> LS peaks
        if (not args.no_pipeline) and not dist_on and headline == "fast":
            try:
                extra["pipeline_end_to_end"] = run_pipeline(t_abs, y, dy, off, df, M, kern_ms, peaks["fast"])
            except Exception as e:   # reported, never fatal for the headline
                extra["pipeline_end_to_end"] = {"error": repr(e)}
        del d_pow, d_t, d_y
        torch.cuda.empty_cache()
        # ---- north_star's own shape on ONE GPU: configs[2]'s 10 000 targets x 1e5 frequencies in one call (VERDICT r5 #4b)
        if args.c2_targets > 0 and not dist_on and not strong and headline == "fast":
            try:
                B2 = args.c2_targets
                t2, y2, _dy2, off2 = ls_batch_threaded(2, B2, N, 0)
                for b in range(B2):
                    t2[off2[b]:off2[b + 1]] -= t2[off2[b]]
                d_t2, d_y2 = torch.from_numpy(t2).to(dev), torch.from_numpy(y2).to(dev)
                d_pow2 = torch.empty((B2, M), dtype=torch.float64, device=dev)
                d_max2 = torch.empty(B2, dtype=torch.float64, device=dev)
                d_arg2 = torch.empty(B2, dtype=torch.int64, device=dev)

                def step2(e0, e1):
                    e0.record()
                    _capi.ls_fast_peaks_batch_dev(handle, B2, off2, d_t2.data_ptr(), d_y2.data_ptr(), 0, df, df, M, True, True,
                                                  "lk_amplitude", 0, 5, d_pow2.data_ptr(), d_max2.data_ptr(), d_arg2.data_ptr(), stream)
                    e1.record()

                s2 = max(1, min(args.steps, 3))
                dt_c2, kms_c2 = timed(step2, 1, s2)
                rl2 = ls_roofline("fast", kms_c2, B2, off2, t2)
                rl2["shader_clock_mhz"] = clock_under(step2, 2, kms_c2)
                extra["configs[2]_on_1_gpu"] = {
                    "metric": "frequencies*targets/sec (Lomb-Scargle, ls_method='fast')", "value": B2 * M * s2 / dt_c2,
                    "unit": unit, "steps": s2, "warmup": 1, "ms_per_step": 1e3 * dt_c2 / s2,
                    "config": {"workload": "configs[2] on ONE GPU: %d TESS-like %d-cadence targets x %d freqs in one "
                                           "lk_ls_fast_peaks_batch_dev call (north_star's 10k x 1e5 shape; its 8-GPU form shards "
                                           "these targets, 1 250 per GPU)" % (B2, N, M)},
                    "roofline": rl2, "speedup_vs_cpu_baseline": (B2 * M * s2 / dt_c2) / cpu_base["value"] if cpu_base else None,
                    "all_peaks_finite": bool(torch.isfinite(d_max2).all().item())}
                del d_t2, d_y2, d_pow2, d_max2, d_arg2, t2, y2
            except Exception as e:   # reported, never fatal for the headline
                extra["configs[2]_on_1_gpu"] = {"error": repr(e)}
            torch.cuda.empty_cache()
        # ---- BLS block of the metric
        if not args.no_bls:
            torch.cuda.empty_cache()
            bsteps = max(1, min(args.steps, 2))
            bres = run_bls(args.bls_targets, rank * args.bls_targets, bsteps, 1)
            bval = bres["units_per_step"] * world * bsteps / bres["dt"]
            blk = {"metric": bres["metric"], "value": bval, "unit": bres["unit"], "steps": bsteps, "warmup": 1,
                   "ms_per_step": 1e3 * bres["dt"] / bsteps, "scaling": "weak",
                   "config": {"workload": bres["workload"]}, "roofline": bres["roofline"]}
            if cpu_base_bls is not None:
                blk["cpu_baseline"] = cpu_base_bls
                blk["speedup_vs_cpu_baseline"] = bval / cpu_base_bls["value"]
            if ref is not None and "bls" in ref and rank == 0:
                blk["accuracy"] = bls_accuracy(bres, ref["bls"])
            extra["bls"] = blk
        # ---- configs[4] PLD and LightCurve.flatten: the other two rows of the hot path, same protocol
        if not args.no_pld:
            torch.cuda.empty_cache()
            pres = run_pld(args.cutouts, rank * args.cutouts, max(1, min(args.steps, 5)), 1, cpu_base_pld)
            extra["pld"] = block_of(pres, cpu_base_pld)
        if not args.no_flatten:
            torch.cuda.empty_cache()
            fres = run_flatten(args.flatten_targets, rank * args.flatten_targets, max(1, min(args.steps, 10)), 1, cpu_base_flat)
            extra["flatten"] = block_of(fres, cpu_base_flat)
    elif args.workload == "bls":
        bres = run_bls(B, first, args.steps, args.warmup, dump)
        dt, kern_ms, dumped = bres["dt"], bres["kernel_ms"], bres["dumped"]
        units_per_step = total_targets * args.periods
        metric, unit, workload, roofline = bres["metric"], bres["unit"], bres["workload"], bres["roofline"]
        if ref is not None and "bls" in ref and rank == 0:
            extra["accuracy"] = bls_accuracy(bres, ref["bls"])
    elif args.workload == "pld":
        pres = run_pld(args.cutouts, rank * args.cutouts, args.steps, args.warmup, cpu_base, dump)
        dt, kern_ms, dumped = pres["dt"], pres["kernel_ms"], pres["dumped"]
        units_per_step = pres["units_per_step"] * world
        metric, unit, workload, roofline = pres["metric"], pres["unit"], pres["workload"], pres["roofline"]
        if pres["accuracy"]:
            extra["accuracy"] = pres["accuracy"]
        if pres.get("api_end_to_end"):
            extra["api_end_to_end"] = pres["api_end_to_end"]
        B, N = args.cutouts, pres["Nc"]
    elif args.workload == "flatten":
        fres = run_flatten(B, first, args.steps, args.warmup, cpu_base, dump)
        dt, kern_ms, dumped = fres["dt"], fres["kernel_ms"], fres["dumped"]
        units_per_step = fres["units_per_step"] * world
        metric, unit, workload, roofline = fres["metric"], fres["unit"], fres["workload"], fres["roofline"]
        if fres["accuracy"]:
            extra["accuracy"] = fres["accuracy"]
        if fres.get("api_end_to_end"):
            extra["api_end_to_end"] = fres["api_end_to_end"]
    elif args.workload == "regress":
        Bc, Nc, K = args.cutouts, args.pld_cadences, args.regressors
        g = torch.Generator(device=dev).manual_seed(1234 + rank)
        d_X = torch.randn((Bc * Nc, K), dtype=torch.float64, device=dev, generator=g)
        d_coef = torch.randn((Bc, K), dtype=torch.float64, device=dev, generator=g) * 1e-3
        d_y = (d_X.view(Bc, Nc, K) @ d_coef.unsqueeze(-1)).reshape(-1) + 1.0 + \
            1e-3 * torch.randn(Bc * Nc, dtype=torch.float64, device=dev, generator=g)
        d_err = torch.full((Bc * Nc,), 1e-3, dtype=torch.float64, device=dev)
        d_mu = torch.zeros(K, dtype=torch.float64, device=dev)
        d_ps = torch.full((K,), 10.0, dtype=torch.float64, device=dev)
        d_w = torch.empty((Bc, K), dtype=torch.float64, device=dev)
        d_model = torch.empty(Bc * Nc, dtype=torch.float64, device=dev)
        d_out = torch.empty(Bc * Nc, dtype=torch.uint8, device=dev)
        offp = np.arange(Bc + 1, dtype=np.int64) * Nc

        def step(e0, e1):
            e0.record()
            _capi._check(lib.lk_regress_batch_dev(handle._h, Bc, offp.ctypes.data_as(i64p), K,
                                                  vp(d_X.data_ptr()), vp(d_y.data_ptr()), vp(d_err.data_ptr()), None,
                                                  vp(d_mu.data_ptr()), vp(d_ps.data_ptr()), 5.0, 5, vp(d_w.data_ptr()),
                                                  vp(d_model.data_ptr()), vp(d_out.data_ptr()), vp(stream)))
            e1.record()

        dt, kern_ms = timed(step, args.warmup, args.steps)
        if dump:
            dumped = sample_outputs([("weights", d_w), ("model", d_model), ("outlier_mask", d_out)])
        units_per_step = Bc * world
        flop = float(Bc) * Nc * (K + 1) * (K + 2)   # ONE Gram build (upper triangle: what the kernel executes); later clip passes are skipped
        metric, unit = "RegressionCorrector fits/sec (N=%d, K=%d, 5 sigma-clip iterations)" % (Nc, K), "fits/sec"
        workload = "configs[4] regression stage: %d fits, N=%d cadences, K=%d regressors per GPU" % (Bc, Nc, K)
        ach = flop / (kern_ms * 1e-3) / 1e12
        roofline = {"bound": "mfma", "achieved": ach, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / FP64_VECTOR_PEAK_TFLOPS, "traffic": None,
                    "kernel": "gram_mfma_kernel (v_mfma_f64_16x16x4_f64)", "kernel_ms_per_step": kern_ms,
                    "note": "useful N*(K+1)*(K+2) flop (upper triangle) for ONE Gram build per fit (SURVEY.md 8(d) counts one per clip "
                            "pass; a target whose pass adds no outlier has reached the fixed point of the reference's "
                            "loop and its remaining passes — identical by construction — are skipped, so only the first "
                            "is counted); each executed pass also runs an LU solve, a model product and a sigma-clip"}
        B, N = Bc, Nc
    elif args.workload == "lschi2":
        t, y, dy, off = synth.ls_batch(1, B, N, first_index=first)
        for b in range(B):
            t[off[b]:off[b + 1]] -= t[off[b]]
        d_t, d_y = torch.from_numpy(t).to(dev), torch.from_numpy(y).to(dev)
        d_p = torch.empty((B, M), dtype=torch.float64, device=dev)
        df = 360.0 / M

        def step(e0, e1):
            e0.record()
            _capi.ls_power_batch_dev(handle, B, off, d_t.data_ptr(), d_y.data_ptr(), 0, 0, df, df, M, True, True,
                                     "lk_amplitude", 0, d_p.data_ptr(), stream, nterms=args.nterms)
            e1.record()

        dt, kern_ms = timed(step, args.warmup, args.steps)
        if dump:
            dumped = sample_outputs([("power", d_p)])
        units_per_step = B * M * world
        metric, unit = "frequencies*targets/sec (Lomb-Scargle, nterms=%d, exact chi2)" % args.nterms, "frequencies*targets/sec"
        workload = "%d targets x %d cadences x %d frequencies, nterms=%d multi-term Lomb-Scargle per GPU" % (B, N, M, args.nterms)
        fl = 2.0 * (4 + 4 * (2 * args.nterms - 1) + 6 * args.nterms) * float(off[-1]) * M
        roofline = {"bound": "valu", "achieved": fl / (kern_ms * 1e-3) / 1e12, "peak": FP64_VECTOR_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": fl / (kern_ms * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
                    "traffic": None, "kernel": "ls_chi2_grid_kernel<%d>" % args.nterms, "kernel_ms_per_step": kern_ms,
                    "note": "4 + 4(2n-1) + 6n FMAs per (cadence, frequency) pair (phasor recurrence, Chebyshev "
                            "harmonics, 6n accumulates), n = nterms"}
    elif args.workload == "pgsmooth":
        from lightkurve_amd.periodogram import _logmedian_windows
        f = (360.0 / M) * (1 + np.arange(M))
        tabs = [np.ascontiguousarray(a, dtype=np.int32) for a in _logmedian_windows(f, 0.01)]
        d_p = torch.rand((B, M), dtype=torch.float64, device=dev)
        d_o = torch.empty_like(d_p)
        i32p = ctypes.POINTER(ctypes.c_int32)

        def step(e0, e1):
            e0.record()
            _capi._check(lib.lk_pg_logmedian_batch_dev(handle._h, B, M, vp(d_p.data_ptr()), int(tabs[0].size),
                                                       tabs[0].ctypes.data_as(i32p), tabs[1].ctypes.data_as(i32p),
                                                       tabs[2].ctypes.data_as(i32p), tabs[3].ctypes.data_as(i32p),
                                                       (8.0 / 9.0) ** 3, vp(d_o.data_ptr()), vp(stream)))
            e1.record()

        dt, kern_ms = timed(step, args.warmup, args.steps)
        if dump:
            dumped = sample_outputs([("smoothed_power", d_o)])
        units_per_step = B * M * world
        members = float(B) * float(np.sum(tabs[1] - tabs[0]))   # window memberships = values the medians look at
        metric, unit = "frequencies*targets/sec (Periodogram.smooth logmedian, filter_width 0.01)", "frequencies*targets/sec"
        workload = "%d periodograms x %d frequencies, logmedian smoothing (%d windows) per GPU" % (B, M, tabs[0].size)
        algo = 16.0 * B * M
        roofline = {"bound": "hbm", "achieved": algo / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": algo / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                    "kernel": "pg_window_median_kernel (+pg_window_average_kernel)", "kernel_ms_per_step": kern_ms,
                    "note": "algorithmic 16 B per frequency (power in, smoothed out); every value sits in ~4 "
                            "overlapping windows and each window median is an 8-pass radix select over its "
                            "members (%.3g member reads per step, served by L2)" % members}
    else:   # fold
        t, y, dy, off = synth.ls_batch(6, B, N, first_index=first)
        d_t, d_y, d_e = (torch.from_numpy(a).to(dev) for a in (t, y, dy))
        d_ph, d_fy, d_fe = torch.empty_like(d_t), torch.empty_like(d_t), torch.empty_like(d_t)
        d_ord = torch.empty(len(t), dtype=torch.int64, device=dev)
        period = np.linspace(0.7, 9.0, B)
        epoch = np.array([t[off[b]] for b in range(B)])
        wrap = period / 2
        dp = ctypes.POINTER(ctypes.c_double)
        cin = (vp * 2)(d_y.data_ptr(), d_e.data_ptr())
        cout = (vp * 2)(d_fy.data_ptr(), d_fe.data_ptr())

        def step(e0, e1):
            e0.record()
            _capi._check(lib.lk_fold_batch_dev(handle._h, B, off.ctypes.data_as(i64p),
                                               vp(d_t.data_ptr()), period.ctypes.data_as(dp), epoch.ctypes.data_as(dp), 0.0,
                                               wrap.ctypes.data_as(dp), 0, 2, cin, cout, vp(d_ph.data_ptr()),
                                               vp(d_ord.data_ptr()), vp(stream)))
            e1.record()

        dt, kern_ms = timed(step, args.warmup, args.steps)
        if dump:
            dumped = sample_outputs([("phase", d_ph), ("order", d_ord), ("flux", d_fy), ("flux_err", d_fe)])
        units_per_step = int(off[-1]) * world
        metric, unit = "fold cadences/sec (phase + stable sort + 2 gathered columns)", "cadences/sec"
        workload = "fold: %d light curves x %d cadences per GPU" % (B, N)
        algo = 72.0 * float(off[-1])
        roofline = {"bound": "hbm", "achieved": algo / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": algo / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                    "kernel": "fold_kernel (+2 fold_gather_kernel)", "kernel_ms_per_step": kern_ms,
                    "note": "algorithmic 72 B per cadence (t in, phase + order out, two columns in and out + "
                            "the order read per gather); the sort itself runs in LDS tiles / an L2-resident slab"}

    if rank == 0:
        if dump:
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name, a in dumped.items():
                np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
        value = units_per_step * args.steps / dt
        out = {
            "metric": metric, "value": value, "unit": unit, "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "full": args.full, "config": {"workload": workload, "targets_per_gpu": B if not strong else None,
                       "targets_total": total_targets, "cadences": N,
                       "parallelism": "targets sharded over %d rank(s), no data-path collective%s"
                                      % (world, ("; RCCL all-gather of %s each step" % (
                                          "the per-target (max power, argmax)" if args.gather == "summary" else
                                          "the full spectra, overlapped with compute"))
                                         if world > 1 and args.workload == "ls" and args.gather != "none" else "")},
            "roofline": roofline,
        }
        if "config_ls_method" in extra:
            out["config"]["ls_method"] = extra.pop("config_ls_method")
        out.update(extra)
        api = out.get("api_end_to_end") or {}
        if args.api_headline and "batch_to_peaks" in api:
            # --workload api: the line's value is what the Python API delivers, host included
            out["device_pointer_step"] = {"value": value, "ms_per_step": out["ms_per_step"], "unit": unit}
            out["metric"] = ("frequencies*targets/sec through the Python batch API, host included "
                             "(LightCurveBatch.to_periodogram_peaks, ls_method='fast')")
            out["value"] = api["batch_to_peaks"]["value"]
            out["ms_per_step"] = api["batch_to_peaks"]["wall_ms"]
        if cpu_base is not None:
            out["cpu_baseline"] = {k: v for k, v in cpu_base.items() if not k.startswith("_")}
            out["speedup_vs_cpu_baseline"] = value / cpu_base["value"]
            if "value_priced_on_survey" in cpu_base:
                out["speedup_vs_survey_reference"] = value / cpu_base["value_priced_on_survey"]
        print(json.dumps(out, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o)))
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
