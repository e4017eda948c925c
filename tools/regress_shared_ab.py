#!/usr/bin/env python
"""A/B of the shared-design-matrix regression against the per-target-matrix path on one problem: B = 1000 targets x N = 20 000
cadences x K = 17 columns (16 basis vectors and a constant), niters = 5.

    python tools/regress_shared_ab.py --out build/regress_shared_ab      # needs the GPU; ~1 min

runs three GPU steps, each under its own `timeout -k 10` and chained with `&&`:
  1. timing: lk_regress_shared_batch_dev and lk_regress_batch_dev (on X tiled B times ON THE DEVICE, the tiling not timed)
     alternate on the same data, every call between two HIP events on the stream, medians over --calls calls after warm-up;
     the outputs of the two paths are compared;
  2. rocprofv3 --kernel-trace --stats of the shared call alone (kernel trace only, no counters);
  3. the same of the per-target-matrix call alone;
then writes <out>/regress_shared_ab.txt: the two medians, the per-kernel tables and the Gram kernel's achieved bytes/s against
its own byte model.  profiles/regress_shared_ab.txt is a copy of that file.
"""
import argparse
import ctypes
import glob
import json
import os
import shlex
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_vp = ctypes.c_void_p


def make_problem(B, N, K, seed=21, noutl=20):
    """The generator of tests/test_regress_shared_gpu.py with `noutl` outliers per target."""
    t = np.linspace(0, 30, N)
    rng = np.random.default_rng(seed)
    cols = [np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(K - 1)]
    X = np.column_stack(cols + [np.ones(N)])
    W = rng.normal(0, 1e-3, (B, K))
    W[:, -1] = 1.0
    err = rng.uniform(0.5, 2.0, (B, N)) * 2e-4
    y = W @ X.T + rng.normal(0, 1, (B, N)) * err
    cm = np.ones((B, N), np.uint8)
    for b in range(B):
        y[b, rng.integers(0, N, noutl)] += rng.choice([-1, 1], noutl) * 0.01
        lo = int(rng.integers(0, N - N // 50 + 1))
        cm[b, lo:lo + N // 50] = 0
    return X, y, err, cm


def byte_model(B, N, K):
    """HBM bytes of ONE full Gram pass of each path (what the kernel must move, from the shapes)."""
    s = max(1, min(16, (N + 255) // 256))
    sl = ((N + s - 1) // s + 31) // 32 * 32
    S = (N + sl - 1) // sl
    NC = 16 * ((K * (K + 1) // 2 + 15) // 16 + (K + 15) // 16)
    ntb = (B + 15) // 16
    shared = B * N * (8 + 8 + 1 + 1) + N * K * 8 + ntb * 16 * S * NC * 8     # flux, error, two mask bytes | X once | partial sums
    Kp = 64 * ((K + 1 + 63) // 64)
    T = (K + 1 + 15) // 16
    parent = B * N * (8 * K + 8 + 8 + 1 + 1) + B * (16 * T) ** 2 * 8         # X per target | flux, error, masks | G tiles
    return dict(shared=shared, parent=parent, slices=S, Kp=Kp)


class Runner(object):
    def __init__(self, B, N, K, niters):
        import torch
        from lightkurve_amd import _capi
        self.torch, self.capi = torch, _capi
        self.B, self.N, self.K, self.niters = B, N, K, niters
        X, y, err, cm = make_problem(B, N, K)
        dev = torch.device("cuda:0")
        self.h = _capi.Handle.get(0)
        self.X = torch.from_numpy(X).to(dev)
        self.y, self.err, self.cm = (torch.from_numpy(a).to(dev) for a in (y, err, cm))
        self.out = {}
        for tag in ("shared", "parent"):
            self.out[tag] = dict(w=torch.empty((B, K), dtype=torch.float64, device=dev),
                                 model=torch.empty((B, N), dtype=torch.float64, device=dev),
                                 outl=torch.empty((B, N), dtype=torch.uint8, device=dev))
        self.X_tiled = None
        self.n_off = (np.arange(B + 1, dtype=np.int64) * N)

    def tile(self):
        if self.X_tiled is None:                       # B copies of X, made on the device, outside every timed window
            self.X_tiled = self.X.repeat(self.B, 1).contiguous()
            self.torch.cuda.synchronize()

    def shared(self):
        o = self.out["shared"]
        self.capi._check(self.capi._lib.lk_regress_shared_batch_dev(
            self.h._h, self.B, self.N, self.K, _vp(self.X.data_ptr()), _vp(self.y.data_ptr()), _vp(self.err.data_ptr()),
            _vp(self.cm.data_ptr()), None, None, 5.0, self.niters, _vp(o["w"].data_ptr()), _vp(o["model"].data_ptr()),
            _vp(o["outl"].data_ptr()), None, None))

    def parent(self):
        o = self.out["parent"]
        self.capi._check(self.capi._lib.lk_regress_batch_dev(
            self.h._h, self.B, self.n_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), self.K, _vp(self.X_tiled.data_ptr()),
            _vp(self.y.data_ptr()), _vp(self.err.data_ptr()), _vp(self.cm.data_ptr()), None, None, 5.0, self.niters,
            _vp(o["w"].data_ptr()), _vp(o["model"].data_ptr()), _vp(o["outl"].data_ptr()), None))

    def timed(self, fn):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)


def mode_time(args):
    r = Runner(args.B, args.N, args.K, args.niters)
    r.tile()
    for _ in range(args.warmup):
        r.shared()
        r.parent()
    r.torch.cuda.synchronize()
    ts, tp = [], []
    for _ in range(args.calls):                       # alternating: both see the same machine
        ts.append(r.timed(r.shared))
        tp.append(r.timed(r.parent))
    s, p = r.out["shared"], r.out["parent"]
    res = dict(B=args.B, N=args.N, K=args.K, niters=args.niters, calls=args.calls, warmup=args.warmup,
               shared_ms=ts, parent_ms=tp, shared_median_ms=float(np.median(ts)), parent_median_ms=float(np.median(tp)),
               masks_equal=bool(r.torch.equal(s["outl"], p["outl"])),
               clipped_per_target=float(s["outl"].sum().item()) / args.B,
               max_abs_model_diff=float((s["model"] - p["model"]).abs().max().item()),
               max_abs_coef_diff=float((s["w"] - p["w"]).abs().max().item()),
               flux_std=float(r.y.std(dim=1).mean().item()))
    with open(os.path.join(args.out, "timing.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_ms") or "median" in k}))


def mode_trace(args, which):
    r = Runner(args.B, args.N, args.K, args.niters)
    if which == "parent":
        r.tile()
    fn = getattr(r, which)
    for _ in range(args.trace_calls):
        fn()
    r.torch.cuda.synchronize()


def kernel_table(db, calls):
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), sum(end - start) / 1000.0, avg(end - start) / 1000.0, max(end - start) / 1000.0 "
                       "from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1.0
    lines = ["%-58s %7s %12s %10s %10s %7s" % ("kernel", "calls", "total_us", "avg_us", "max_us", "pct")]
    for name, n, t, a, m in rows:
        lines.append("%-58s %7d %12.1f %10.1f %10.1f %7.2f" % (name.split("(")[0][-58:], n, t, a, m, 100 * t / tot))
    lines.append("# all kernels: %.1f us over %d calls = %.1f us per call" % (tot, calls, tot / calls))

    def full_pass(pattern):        # a call's first pass is the full one (later passes skip converged targets): the `calls` longest
        d = [x[0] for x in con.execute("select (end - start) / 1000.0 from kernels where name like ? order by 1 desc limit ?",
                                       (pattern, calls)).fetchall()]
        return float(np.median(d)) if d else float("nan")

    def per_call(pattern):
        v = con.execute("select sum(end - start) / 1000.0 from kernels where name like ?", (pattern,)).fetchone()[0]
        return (v or 0.0) / calls
    return lines, full_pass, per_call


def summarise(args):
    tm = json.load(open(os.path.join(args.out, "timing.json")))
    bm = byte_model(args.B, args.N, args.K)
    out = ["# regression on one shared design matrix vs one matrix per target: B = %d, N = %d, K = %d, niters = %d"
           % (args.B, args.N, args.K, args.niters),
           "# tools/regress_shared_ab.py; MI355X; HIP events around each call, %d calls after %d warm-up calls, the two paths alternating"
           % (tm["calls"], tm["warmup"]), "",
           "## whole call (milliseconds, HIP events)",
           "lk_regress_shared_batch_dev          median %.3f   min %.3f   max %.3f" % (tm["shared_median_ms"], min(tm["shared_ms"]), max(tm["shared_ms"])),
           "lk_regress_batch_dev on tiled X      median %.3f   min %.3f   max %.3f" % (tm["parent_median_ms"], min(tm["parent_ms"]), max(tm["parent_ms"])),
           "ratio parent / shared                %.2f" % (tm["parent_median_ms"] / tm["shared_median_ms"]),
           "device memory of the design matrix   shared %.1f MB, tiled %.1f MB" % (args.N * args.K * 8 / 1e6, args.B * args.N * args.K * 8 / 1e6),
           "outputs: outlier masks equal: %s (%.1f clipped per target); max |model difference| %.3g (mean flux std %.3g); max |coefficient difference| %.3g"
           % (tm["masks_equal"], tm["clipped_per_target"], tm["max_abs_model_diff"], tm["flux_std"], tm["max_abs_coef_diff"]), ""]
    res = {}
    for which in ("shared", "parent"):
        dbs = sorted(glob.glob(os.path.join(args.out, "trace_" + which, "**", "*results.db"), recursive=True))
        if not dbs:
            out.append("## %s: no rocprofv3 result database found" % which)
            continue
        lines, full_pass, per_call = kernel_table(dbs[0], args.trace_calls)
        out.append("## rocprofv3 --kernel-trace --stats, %s path alone, %d calls (microseconds)" % (which, args.trace_calls))
        out.extend(lines)
        out.append("")
        res[which] = (full_pass, per_call)
    if "shared" in res and "parent" in res:
        fs, ps = res["shared"]
        fp, pp = res["parent"]
        g_s, g_p = fs("%gram_shared_kernel%"), fp("%gram_tri_kernel%")
        out += ["## Gram kernels against their byte models (one FULL pass = a call's first pass; median of the longest dispatch per call)",
                "gram_shared_kernel   %.1f us for %.1f MB (flux, error, two mask bytes per cadence; X once; %d-slice partial sums) = %.2f TB/s"
                % (g_s, bm["shared"] / 1e6, bm["slices"], bm["shared"] / g_s / 1e6),
                "gram_tri_kernel      %.1f us for %.1f MB (the tiled matrix and the same per-target arrays) = %.2f TB/s"
                % (g_p, bm["parent"] / 1e6, bm["parent"] / g_p / 1e6),
                "",
                "## Gram + model kernels per call (all passes, microseconds)",
                "shared: gram_shared_kernel %.1f + gram_shared_reduce_kernel %.1f + model_shared_kernel %.1f = %.1f"
                % (ps("%gram_shared_kernel%"), ps("%gram_shared_reduce%"), ps("%model_shared_kernel%"),
                   ps("%gram_shared_kernel%") + ps("%gram_shared_reduce%") + ps("%model_shared_kernel%")),
                "parent: gram_tri_kernel %.1f + gram_mfma_kernel (delta passes) %.1f + model_kernel %.1f = %.1f"
                % (pp("%gram_tri_kernel%"), pp("%gram_mfma_kernel%"), pp("%model_kernel%"),
                   pp("%gram_tri_kernel%") + pp("%gram_mfma_kernel%") + pp("%model_kernel%"))]
    path = os.path.join(args.out, "regress_shared_ab.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="build/regress_shared_ab")
    ap.add_argument("--mode", default="all", choices=["all", "time", "trace-shared", "trace-parent", "summary"])
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--K", type=int, default=17)
    ap.add_argument("--niters", type=int, default=5)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-calls", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    os.makedirs(args.out, exist_ok=True)
    if args.mode == "time":
        return mode_time(args)
    if args.mode in ("trace-shared", "trace-parent"):
        return mode_trace(args, args.mode.split("-")[1])
    if args.mode == "all":
        me = shlex.quote(os.path.abspath(__file__))
        common = "--out %s --B %d --N %d --K %d --niters %d --calls %d --warmup %d --trace-calls %d" % (
            shlex.quote(args.out), args.B, args.N, args.K, args.niters, args.calls, args.warmup, args.trace_calls)
        to = "timeout -k 10 %d" % args.step_timeout
        steps = ["%s %s %s --mode time %s" % (to, sys.executable, me, common)]
        for which in ("shared", "parent"):         # kernel trace only: no counters in the same run
            steps.append("%s rocprofv3 --kernel-trace --stats -d %s -o %s -- %s %s --mode trace-%s %s > %s 2>&1"
                         % (to, shlex.quote(os.path.join(args.out, "trace_" + which)), which, sys.executable, me, which, common,
                            shlex.quote(os.path.join(args.out, "trace_%s.log" % which))))
        rc = subprocess.call(["bash", "-c", " && ".join(steps)], cwd=tempfile.gettempdir())
        if rc != 0:
            raise SystemExit("a GPU step failed or ran out of time (exit status %d): nothing further was started" % rc)
    summarise(args)


if __name__ == "__main__":
    main()
