"""numpy model of the route decisions of block_select_sampled (lightkurve_amd/csrc/block_select.hpp): which of the header's
workgroup-uniform branches an input takes, named as the SelRoute enum names them.  It exists to PICK inputs for
tests/test_block_select_gpu.py on a machine without a GPU; it is not an oracle — the tests assert on the route word the device
reports.  `python tests/select_route_model.py` lists what the aimed inputs of that file take and searches seeds for the two routes
that need luck (the candidate radix select, the two-bin refinement)."""
import numpy as np

SEL_NB, SEL_LIST, SEL_SAMPLE = 1024, 64, 1024


def hist_select(c, cap, qa, qb, lo, hi, R):
    nc = len(c)
    ncp = (nc + 1) & ~1
    if not (hi > lo) or not np.isfinite(lo) or not np.isfinite(hi) or ncp + SEL_NB // 2 + SEL_LIST + 2 > cap or nc <= 0:
        R.add("hist_na")
        return False
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        scale = SEL_NB / (hi - lo)
        x = (c - lo) * scale
    b = np.clip(np.where(np.isfinite(x), x, 0).astype(np.int64), 0, SEL_NB - 1)
    sb = np.sort(b)
    want = {sb[q] for q in (qa, qb) if q >= 0}
    m = sum(int((b == w).sum()) for w in want)
    R.add("hist_done" if m <= SEL_LIST else "hist_ties")
    return m <= SEL_LIST


def route(v, keep, k, cap, want_next=True):
    v = np.asarray(v, float)
    n = len(v)
    keep = np.ones(n, bool) if keep is None else keep
    kv = v[keep]
    count = len(kv)
    R = set()
    if cap < 2 * SEL_SAMPLE:
        return {"cap_small_fallback"}
    if count <= min(cap, 2 * SEL_SAMPLE):
        R.add("all_in_lds")
        nb = want_next and k + 1 < count
        ok = hist_select(kv, cap, k, k + 1 if nb else -1, kv.min(), kv.max(), R)
        R.add("all_hist_ok" if ok else "all_sorted")
        return R
    idx = (np.arange(SEL_SAMPLE, dtype=np.int64) * n) // SEL_SAMPLE
    smp = np.sort(v[idx][keep[idx]])
    s_all = len(smp)
    if s_all < 64:
        return {"sample_small_fallback"}
    pos = (k + 0.5) * s_all / count
    sq = np.sqrt(s_all)
    delta = int(min(2 * sq + 6, max(1.2 * sq + 4, 2600.0 * s_all / (2.0 * count))))
    r_lo, r_hi = int(pos) - delta, int(pos) + delta
    lo = -np.inf if r_lo < 0 else smp[r_lo]
    hi = np.inf if r_hi >= s_all else smp[r_hi]
    R.add("bracket")
    if r_lo < 0:
        R.add("pivot_lo_inf")
    if r_hi >= s_all:
        R.add("pivot_hi_inf")
    n_less = int((kv < lo).sum())
    n_eqlo = int((kv == lo).sum())
    inside = kv[(kv > lo) & (kv < hi)]
    nc = len(inside)
    n_eqhi = int(((kv == hi) & (kv != lo)).sum())
    slo, shi = lo, hi
    if nc > cap:
        R.add("overflow")
        q0 = k - n_less - n_eqlo
        wa = 0 <= q0 < nc
        wb = want_next and k + 1 < count and 0 <= q0 + 1 < nc
        if not (wa or wb) or not np.isfinite(lo) or not np.isfinite(hi) or not hi > lo or cap < SEL_NB:
            return R | {"refine_na_fallback"}
        rf = q0 if wa else q0 + 1
        rl = q0 + 1 if wb else q0
        scale = SEL_NB / (hi - lo)
        b = np.clip(((inside - lo) * scale).astype(np.int64), 0, SEL_NB - 1)
        sb = np.sort(b)
        ba, bb = sb[rf], sb[rl]
        below = int((b < ba).sum())
        through = int((b <= bb).sum())
        if through - below > cap:
            return R | {"refine_ties_fallback"}
        R.add("refined")
        if bb != ba:
            R.add("refined_two_bins")
        inside = inside[(b >= ba) & (b <= bb)]
        n_less += n_eqlo + below
        n_eqlo = n_eqhi = 0
        nc = len(inside)
        slo = lo + ba / scale
        shi = lo + (bb + 1) / scale
    qa = k - n_less - n_eqlo
    qb = qa + 1
    need_a = 0 <= qa < nc
    need_b = want_next and k + 1 < count and 0 <= qb < nc
    hist_ok = False
    if need_a or need_b:
        hist_ok = hist_select(inside, cap, qa if need_a else -1, qb if need_b else -1, slo, shi, R)
        R.add("cand_hist_ok" if hist_ok else "cand_hist_refused")
    S2 = 2
    while S2 < nc:
        S2 <<= 1
    srt = (not hist_ok) and (need_a or need_b) and S2 <= cap
    if srt:
        R.add("cand_sorted")

    def at(r):
        q = r - n_less
        if q < 0:
            return "miss"
        if q < n_eqlo:
            R.add("rank_in_eqlo")
            return "eqlo"
        q -= n_eqlo
        if q < nc:
            R.add("rank_in_cand")
            if not (hist_ok or srt):
                R.add("cand_lds_radix")
            return "cand"
        q -= nc
        if q < n_eqhi:
            R.add("rank_in_eqhi")
            return "eqhi"
        return "miss"

    a = at(k)
    b = at(k + 1) if a != "miss" and want_next and k + 1 < count else a
    if "miss" in (a, b):
        R.add("miss_fallback")
    return R


def median_route(v, cap, keep=None):
    c = len(v) if keep is None else int(keep.sum())
    return route(v, keep, (c - 1) // 2, cap, c % 2 == 0)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import test_block_select_gpu as T
    for name, d, rank, exp in T.route_cases():
        for cap in T.ALL_CAPS:
            k, w = ((d.count - 1) // 2, d.count % 2 == 0) if rank == "median" else (rank[0], bool(rank[1]))
            got = route(d.values, d.keep, k, cap, w)
            flag = "" if cap not in exp else ("ok" if exp[cap] <= got else "MISSING %s" % sorted(exp[cap] - got))
            print("%-28s cap %4d %-8s %s" % (name, cap, flag, " ".join(sorted(got))))
    if "--search" in sys.argv:
        for cap, sizes in ((4896, (54_000, 56_000, 58_000)), (5880, (64_000, 66_000, 70_000))):
            for n in sizes:
                for seed in range(12):
                    if "cand_lds_radix" in median_route(T._uniform(seed, n), cap):
                        print("cand_lds_radix: (%d, %d, %d)" % (cap, n, seed))
        for cap, sizes in ((2048, (20_000, 40_000)), (4096, (60_000, 80_000)), (4896, (70_000, 90_000)), (5880, (80_000, 100_000))):
            for n in sizes:
                for seed in range(12):
                    if "refined_two_bins" in median_route(T._gauss(seed, n), cap):
                        print("refined_two_bins: (%d, %d, %d)" % (cap, n, seed))
