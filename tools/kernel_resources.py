#!/usr/bin/env python
"""Regenerate profiles/kernel_resources.md: registers, spills, scratch, occupancy and LDS of EVERY gfx950 kernel of liblkhip.so,
straight from the compiler (`hipcc -Rpass-analysis=kernel-resource-usage`, the flags of lightkurve_amd/csrc/Makefile).

DESIGN.md quotes spill counts; rounds 4-5 typed them by hand and they went stale.  Now they are quoted
from this table, which is a build product:

    python tools/kernel_resources.py            # rewrites profiles/kernel_resources.md (~1 min, 8 compiles in parallel)
    python tools/kernel_resources.py --check    # exit 1 if the committed table differs from what the sources compile to

tests/test_capi_symbols.py checks (without compiling) that the table names every __global__ kernel of the sources.
"""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lightkurve_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "kernel_resources.md")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = next((c for c in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "/usr/bin/c++filt") if os.path.exists(c)), "c++filt")
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("VGPRs Spill", "VGPR spill"), ("SGPRs Spill", "SGPR spill"),
          ("ScratchSize [bytes/lane]", "scratch B/lane"), ("Occupancy [waves/SIMD]", "waves/SIMD"),
          ("LDS Size [bytes/block]", "static LDS B"))


def flags_for(src):
    extra = ["-ffp-contract=off"] if os.path.basename(src) in ("bls.hip", "blsstats.hip", "pgsmooth.hip", "pixcube.hip", "select.hip", "fillgaps.hip", "interp.hip") else []    # as the Makefile
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra


def analyse(src):
    cmd = [HIPCC] + flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    if p.returncode != 0:
        raise SystemExit("compile failed: %s\n%s" % (" ".join(cmd), p.stderr[-2000:]))
    kernels, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line) or re.search(r"remark: .*?\bName: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            kernels.append(cur)
            continue
        if cur is None:
            continue
        for key, _ in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return kernels


def demangle(names):
    if not names or not os.path.exists(CXXFILT):
        return names
    p = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True)
    out = p.stdout.splitlines()
    return out if len(out) == len(names) else names


def short(name):
    """lk::flat_trend_kernel<true>(long const*, ...) -> flat_trend_kernel<true>"""
    name = re.sub(r"^void ", "", name)
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    return name[:cut].replace("lk::", "").replace("(anonymous namespace)::", "")


CLOSED_FORM = ("fft_rows512_power_kernel", "fft_rows_power_kernel", "lsf_power_kernel")


def closed_form_counts():
    """Static counts of the fp64 reciprocal / reciprocal-square-root instructions (the ones that issue at the transcendental
    rate; one per IEEE division or square root sequence) in the lsfast.hip kernels that hold the closed form, from -S."""
    src = os.path.join(CSRC, "lsfast.hip")
    cmd = [HIPCC] + flags_for(src) + ["--cuda-device-only", "-S", src, "-o", "-"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    if p.returncode != 0:
        raise SystemExit("compile failed: %s\n%s" % (" ".join(cmd), p.stderr[-2000:]))
    counts, cur = {}, None
    for line in p.stdout.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = counts.setdefault(m.group(1), [0, 0])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            op = line.split()[0] if line.split() else ""
            cur[0] += op.startswith("v_rcp_f64")
            cur[1] += op.startswith("v_rsq_f64")
    names = demangle(list(counts))
    rows = sorted((short(n), c) for n, c in zip(names, counts.values()) if short(n).split("<")[0] in CLOSED_FORM)
    lines = ["### lsfast.hip: closed-form kernels, fp64 reciprocals and reciprocal square roots (whole kernel, static)", "",
             "Every branch counts: all four normalisations, both `fit_mean` settings and the underflow fall-back of",
             "`gls_power_sums_lean`; what one output executes is in `profiles/lsfast_closed_form_ab.txt`.", "",
             "| kernel | v_rcp_f64 | v_rsq_f64 |", "|---|---:|---:|"]
    lines += ["| `%s` | %d | %d |" % (n, c[0], c[1]) for n, c in rows]
    return lines + [""]


def table():
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        extra = ex.submit(closed_form_counts)
        results = list(ex.map(lambda f: analyse(os.path.join(CSRC, f)), srcs))
    lines = ["# Kernel resources (generated by tools/kernel_resources.py — do not edit)", "",
             "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`, the flags of `lightkurve_amd/csrc/Makefile`.",
             "gfx950: 512 VGPRs per SIMD lane (a wave may use up to 512 with AGPRs), occupancy = waves per SIMD the register",
             "budget admits; scratch > 0 means spills (or a private array) in memory.", ""]
    for f, kernels in zip(srcs, results):
        lines += ["## %s" % f, "", "| kernel | " + " | ".join(h for _, h in FIELDS) + " |", "|---|" + "---:|" * len(FIELDS)]
        names = demangle([k["mangled"] for k in kernels])
        rows = sorted(zip((short(n) for n in names), kernels), key=lambda r: r[0])
        for name, k in rows:
            lines.append("| `%s` | " % name + " | ".join(str(k.get(key, "")) for key, _ in FIELDS) + " |")
        lines.append("")
        if f == "lsfast.hip":
            lines += extra.result()
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    new = table()
    if args.check:
        old = open(OUT).read() if os.path.exists(OUT) else ""
        if old != new:
            sys.stderr.write("profiles/kernel_resources.md is stale: run tools/kernel_resources.py\n")
            return 1
        print("profiles/kernel_resources.md is current")
        return 0
    with open(OUT, "w") as fh:
        fh.write(new)
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
