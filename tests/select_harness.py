"""Loader of tests/select_harness.hip: compiles the test-only driver of lightkurve_amd/csrc/block_select.hpp with hipcc
(no GPU needed for that) and wraps its C entry points.  A nonzero return of an entry point raises; nothing is retried."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "select_harness.hip")
CSRC = os.path.join(ROOT, "lightkurve_amd", "csrc")
ENTRY_POINTS = ("selh_route_count", "selh_prob_size", "selh_select", "selh_sort", "selh_reduce", "selh_sortable")

OP_KTH, OP_MEDIAN, OP_SAMPLED, OP_MEDIAN_SAMPLED, OP_NEAR, OP_HIST = range(6)
RED_EXSCAN, RED_SUM_DYN, RED_SUM_FAST, RED_COUNT_DYN, RED_COUNT_FAST = range(5)

PROB = np.dtype([("off", "<i8"), ("count", "<i8"), ("k", "<i8"), ("n", "<i4"), ("aux", "<i4"), ("guess", "<f8"),
                 ("width", "<f8")])


def route_names():
    """The SelRoute enum of block_select.hpp, in order: bit i of a route word is names[i]."""
    src = open(os.path.join(CSRC, "block_select.hpp")).read()
    body = re.search(r"enum SelRoute \{(.*?)\};", src, flags=re.S).group(1)
    names = re.findall(r"\bSEL_R_([A-Z0-9_]+)\b", re.sub(r"//[^\n]*", "", body))
    assert names[-1] == "COUNT"
    return [n.lower() for n in names[:-1]]


def compile_harness(outdir):
    """hipcc -> <outdir>/libselect_harness.so; returns its path."""
    out = os.path.join(str(outdir), "libselect_harness.so")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3",
           "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SOURCE, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("select harness does not compile:\n" + p.stdout)
    return out


class Problem:
    """One workgroup's input: values, an optional keep mask (bool, None = all kept), rank k, aux (want_next / qb), and the
    guess / width pair (block_median_near) or lo / hi (lds_hist_select)."""

    def __init__(self, values, keep=None, k=0, aux=0, guess=0.0, width=0.0):
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.keep = None if keep is None else np.ascontiguousarray(keep, dtype=bool)
        self.k, self.aux, self.guess, self.width = int(k), int(aux), float(guess), float(width)
        self.count = self.values.size if self.keep is None else int(np.count_nonzero(self.keep))

    def kept(self):
        return self.values if self.keep is None else self.values[self.keep]


def load(path):
    """dlopen the harness on the SAME HIP runtime liblkhip.so uses (one runtime per process: lightkurve_amd/_capi.py loads
    PyTorch's bundled copy first when there is one; a library opened before that on another copy would leave the later one
    without a device)."""
    from lightkurve_amd import _capi
    _capi._share_hip_runtime_with_torch()
    return ctypes.CDLL(path)


class Harness:
    def __init__(self, path):
        self.lib = load(path)
        self.names = route_names()
        assert self.lib.selh_route_count() == len(self.names) <= 32
        assert self.lib.selh_prob_size() == PROB.itemsize

    def bit(self, name):
        return 1 << self.names.index(name)

    def decode(self, word):
        return {n for i, n in enumerate(self.names) if (int(word) >> i) & 1}

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed with code %d (-1: a precondition of block_select.hpp was violated; else the HIP "
                               "error)" % (what, rc))

    @staticmethod
    def pack(problems):
        """Lay the problems out for selh_select once (reused over launches).  Problems that share the same values / keep arrays
        (several ranks of one data set) share one copy."""
        probs = np.zeros(len(problems), PROB)
        vals, masks, where, off = [], [], {}, 0
        any_mask = any(p.keep is not None for p in problems)
        for g, p in enumerate(problems):
            key = (id(p.values), id(p.keep))
            if key not in where:
                where[key] = off
                vals.append(p.values)
                masks.append(np.ones(p.values.size, np.uint8) if p.keep is None else p.keep.astype(np.uint8))
                off += p.values.size
            probs[g] = (where[key], p.count, p.k, p.values.size, p.aux, p.guess, p.width)
        v = np.concatenate(vals) if vals else np.zeros(0)
        m = np.concatenate(masks) if any_mask else None
        return v, m, probs

    def select(self, op, nt, cap, packed):
        """One launch over pack(problems).  Returns a dict of per-problem arrays: value, next, spacing, side_lo_min,
        side_lo_max, value_last / next_last (what the LAST thread of the workgroup got), flag (side_ran / ok / hist returned
        true), side_calls, untouched, route."""
        v, m, probs = packed
        G = probs.size
        outd = np.empty((G, 8))
        outi = np.empty((G, 4), np.int64)
        routes = np.empty(G, np.uint32)
        rc = self.lib.selh_select(ctypes.c_int(op), ctypes.c_int(nt), ctypes.c_int(cap), ctypes.c_int(G),
                                  ctypes.c_longlong(v.size), v.ctypes.data_as(ctypes.c_void_p),
                                  None if m is None else m.ctypes.data_as(ctypes.c_void_p),
                                  probs.ctypes.data_as(ctypes.c_void_p), outd.ctypes.data_as(ctypes.c_void_p),
                                  outi.ctypes.data_as(ctypes.c_void_p), routes.ctypes.data_as(ctypes.c_void_p))
        self._check(rc, "selh_select(op=%d, nt=%d, cap=%d)" % (op, nt, cap))
        return dict(value=outd[:, 0].copy(), next=outd[:, 1].copy(), spacing=outd[:, 2].copy(), side_lo_min=outd[:, 3].copy(),
                    side_lo_max=outd[:, 4].copy(), value_last=outd[:, 5].copy(), next_last=outd[:, 6].copy(),
                    flag=outi[:, 0].copy(), side_calls=outi[:, 1].copy(), untouched=outi[:, 2].copy(), route=routes)

    def sort(self, nt, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        G, S = keys.shape
        out = np.empty_like(keys)
        rc = self.lib.selh_sort(ctypes.c_int(nt), ctypes.c_int(S), ctypes.c_int(G), keys.ctypes.data_as(ctypes.c_void_p),
                                out.ctypes.data_as(ctypes.c_void_p))
        self._check(rc, "selh_sort(nt=%d, S=%d)" % (nt, S))
        return out

    def reduce(self, op, nt, xd=None, xi=None):
        """xd / xi: (G, nt).  Returns (per-thread doubles, per-thread int64, per-thread scan totals)."""
        ref = xd if xd is not None else xi
        G = ref.shape[0]
        assert ref.shape == (G, nt)
        xd = np.ascontiguousarray(np.zeros((G, nt)) if xd is None else xd, dtype=np.float64)
        xi = np.ascontiguousarray(np.zeros((G, nt)) if xi is None else xi, dtype=np.int64)
        od, oi, tot = np.empty((G, nt)), np.empty((G, nt), np.int64), np.empty((G, nt), np.int64)
        rc = self.lib.selh_reduce(ctypes.c_int(op), ctypes.c_int(nt), ctypes.c_int(G), xd.ctypes.data_as(ctypes.c_void_p),
                                  xi.ctypes.data_as(ctypes.c_void_p), od.ctypes.data_as(ctypes.c_void_p),
                                  oi.ctypes.data_as(ctypes.c_void_p), tot.ctypes.data_as(ctypes.c_void_p))
        self._check(rc, "selh_reduce(op=%d, nt=%d)" % (op, nt))
        return od, oi, tot

    def sortable(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        key, back = np.empty(x.size, np.uint64), np.empty(x.size)
        rc = self.lib.selh_sortable(ctypes.c_int(x.size), x.ctypes.data_as(ctypes.c_void_p),
                                    key.ctypes.data_as(ctypes.c_void_p), back.ctypes.data_as(ctypes.c_void_p))
        self._check(rc, "selh_sortable")
        return key, back


# ------------------------------------------------------------------------------------------------------------ inputs
# The value families, sizes and orders every select test feeds: the harness tests here and the production callers' tests
# (ingest, BLS input preparation) run the same ones.
SIZES = (1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 20_000, 30_000, 54_000, 64_000, 90_000, 200_001)
FAMILIES = ("gaussian", "lognormal", "negative", "mixed_zeros", "round1", "round2", "round3", "constant", "two_valued",
            "clusters", "third_neg_inf", "majority_pos_inf", "denormal", "full_range", "tiny_spread")


def family(name, n, rng):
    g = rng.standard_normal(n)
    i = np.arange(n)
    if name == "gaussian":
        return g
    if name == "lognormal":
        return np.exp(3 * g)
    if name == "negative":
        return -np.exp(g)
    if name == "mixed_zeros":           # both zeros present, values of both signs around them
        v = g.copy()
        v[i % 5 == 1] = 0.0
        v[i % 5 == 3] = -0.0
        return v
    if name in ("round1", "round2", "round3"):
        return np.round(g, int(name[-1]))
    if name == "constant":
        return np.full(n, 3.25)
    if name == "two_valued":            # 50/50: with an even count the two middle ranks are different values
        return np.where(i % 2 == 0, 1.0, 2.0)
    if name == "clusters":
        return np.where(i % 2 == 0, 1e-6 * g, 5 + 1e-6 * g)
    if name == "third_neg_inf":
        return np.where(i % 3 == 0, -np.inf, g)
    if name == "majority_pos_inf":
        return np.where(i % 5 < 3, np.inf, g)
    if name == "denormal":
        return rng.integers(0, 4096, n) * 5e-324
    if name == "full_range":            # hi - lo overflows
        return rng.uniform(-1.0, 1.0, n) * 1.7e308
    if name == "tiny_spread":
        return 1.0 + 1e-15 * rng.integers(0, 50, n)
    raise KeyError(name)


def ordered(v, order, rng):
    if order == "ascending":
        return np.sort(v)
    if order == "descending":
        return np.sort(v)[::-1].copy()
    return rng.permutation(v)


def production_batch(max_n=30_000, seed=99):
    """[(name, values)]: every family at every size up to max_n, shuffled, ascending and descending, plus the order that
    defeats the strided sample (8192 values, the 1024 sample positions see one class only) both ways round."""
    rng = np.random.default_rng(seed)
    out = []
    for fam in FAMILIES:
        for n in SIZES:
            if n > max_n:
                continue
            v = family(fam, n, rng)
            for order in ("shuffled", "ascending", "descending"):
                out.append(("%s/%s/%d" % (fam, order, n), ordered(v, order, rng)))
    i = np.arange(8192)
    out.append(("aliased_low", np.where(i % 8 == 0, rng.uniform(0, 1, 8192), rng.uniform(10, 11, 8192))))
    out.append(("aliased_high", np.where(i % 8 == 0, rng.uniform(10, 11, 8192), rng.uniform(0, 1, 8192))))
    return out


def reference_median(values):
    """numpy's median restated on the sorted values: s[(c-1)//2] for an odd count, else 0.5 * (s[c//2-1] + s[c//2])."""
    s = np.sort(np.asarray(values, dtype=np.float64))
    c = s.size
    if c == 0:
        return float("nan")
    if c & 1:
        return s[(c - 1) // 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * (s[c // 2 - 1] + s[c // 2])
