"""GPU: the workgroup order statistics of lightkurve_amd/csrc/block_select.hpp, driven directly through tests/select_harness.hip
and compared with numpy, on every route the header can take.

Reference: s = np.sort(values[keep]); rank k is s[k]; the median is s[(c-1)//2] for an odd count c, else
0.5 * (s[c//2-1] + s[c//2]); NaN for an empty set (and for the mean of -inf and +inf).  Nothing here has a tolerance: every result
is an order statistic or the IEEE mean of two and is compared with `==` — value equality, not bit pattern, so -0.0 and +0.0
compare equal (a select may return either zero of a tie) — and the NaN positions must be identical.
Precondition kept from the header's callers: no kept value is NaN (the harness refuses such input; it is not tested).

Each launch runs many independent problems, one workgroup each, and is run TWICE: every output must come back with identical
bits (the order of the candidates in LDS depends on atomics, the results must not).  Each problem also reports its route word
(the LK_SEL_ROUTE hooks of the header); test_every_route_is_reached_at_every_block_size_and_cap accounts for them.
tests/select_route_model.py's numpy model of the route decisions was used to pick the inputs of ROUTE_CASES; it is not an
oracle — the assertions are on the route word the device reports."""
import numpy as np
import pytest

from tests import select_harness as SH
from tests.select_harness import FAMILIES, SIZES, Problem, family, ordered

pytestmark = pytest.mark.gpu

NTS = (256, 512, 1024)
CAPS = (1024, 2048, 4096, 4896, 5880)
NAN = float("nan")


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return SH.Harness(SH.compile_harness(tmp_path_factory.mktemp("select_harness")))


# ------------------------------------------------------------------------------------------------------------ inputs
class Data:
    """One data set and its reference (the sorted kept values)."""

    def __init__(self, name, values, keep=None):
        self.name = name
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.keep = None if keep is None else np.ascontiguousarray(keep, dtype=bool)
        self.s = np.sort(self.values if keep is None else self.values[self.keep])
        self.count = self.s.size

    def rank(self, k):
        return self.s[k]

    def median(self):
        c = self.count
        if c == 0:
            return NAN
        if c & 1:
            return self.s[(c - 1) // 2]
        with np.errstate(invalid="ignore", over="ignore"):
            return 0.5 * (self.s[c // 2 - 1] + self.s[c // 2])

    def problem(self, k=0, aux=0, guess=0.0, width=0.0):
        p = Problem(self.values, self.keep, k, aux, guess, width)
        p.data = self
        return p


_GRID = []


def grid():
    """Every family x {shuffled, ascending, descending, shuffled with a random 10 % dropped} x every size, plus the edge sets."""
    if _GRID:
        return _GRID
    rng = np.random.default_rng(20240607)
    for fam in FAMILIES:
        for n in SIZES:
            v = family(fam, n, rng)
            for order in ("shuffled", "ascending", "descending"):
                _GRID.append(Data("%s/%s/%d" % (fam, order, n), ordered(v, order, rng)))
            _GRID.append(Data("%s/drop10/%d" % (fam, n), rng.permutation(v), rng.random(n) >= 0.1))
    n = 8192
    i = np.arange(n)
    for fam in ("gaussian", "round2", "lognormal"):
        v = family(fam, n, rng)
        _GRID.append(Data(fam + "/sample_positions_dropped", v, i % 8 != 0))   # 7168 kept, the strided sample is empty
        _GRID.append(Data(fam + "/only_sample_positions_kept", v, i % 8 == 0))  # 1024 kept: all in LDS under a sparse mask
    _GRID.append(Data("aliased", np.where(i % 8 == 0, rng.uniform(0, 1, n), rng.uniform(10, 11, n))))
    _GRID.append(Data("aliased_high", np.where(i % 8 == 0, rng.uniform(10, 11, n), rng.uniform(0, 1, n))))
    _GRID.append(Data("minus_and_plus_inf", [-np.inf, np.inf]))                   # the mean of the two is NaN
    _GRID.append(Data("infs_even", rng.permutation(np.repeat([-np.inf, np.inf], 3000))))
    _GRID.append(Data("nothing_kept", rng.standard_normal(5000), np.zeros(5000, bool)))
    _GRID.append(Data("one_kept_of_many", rng.standard_normal(30_000), np.arange(30_000) == 777))
    _GRID.append(Data("both_zeros_only", rng.permutation(np.repeat([-0.0, 0.0], 2500))))
    return _GRID


def same(got, ref):
    """value equality with identical NaN positions"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (got == ref) | (np.isnan(got) & np.isnan(ref))


SEEN = {}   # (nt, cap) -> OR of every route word this module saw


def launch(H, op, nt, cap, packed):
    """The launch, twice: identical bits in every output; every thread of a workgroup holds the same result."""
    a = H.select(op, nt, cap, packed)
    b = H.select(op, nt, cap, packed)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), "two runs of the same launch differ in %r" % key
    assert a["value"].tobytes() == a["value_last"].tobytes() and a["next"].tobytes() == a["next_last"].tobytes()
    SEEN[(nt, cap)] = SEEN.get((nt, cap), 0) | int(np.bitwise_or.reduce(a["route"]))
    return a


def report(H, problems, bad):
    return [(problems[g].data.name, problems[g].k) for g in np.flatnonzero(bad)[:8]]


# ------------------------------------------------------------------------------------------------------------ key transform
def test_sortable_keys_are_ordered_and_round_trip(H):
    tiny, dmin, dmax = 5e-324, np.finfo(np.float64).tiny, np.finfo(np.float64).max
    x = np.array([-np.inf, -dmax, -1.0, -dmin, -tiny, -0.0, 0.0, tiny, dmin, 1.0, dmax, np.inf])
    key, back = H.sortable(x)
    assert np.all(key[1:] > key[:-1]), "keys strictly increasing in numeric order, -0.0 before +0.0"
    assert back.tobytes() == x.tobytes(), "round trip is bit-exact"
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 63, 100_000, dtype=np.uint64) | (rng.integers(0, 2, 100_000, dtype=np.uint64) << np.uint64(63))
    r = bits.view(np.float64)
    r = r[~np.isnan(r)]
    key, back = H.sortable(r)
    assert back.tobytes() == r.tobytes()
    o = np.argsort(key, kind="stable")
    assert np.all(np.diff(r[o]) >= 0), "key order is numeric order"
    assert np.unique(key).size == np.unique(r.view(np.uint64)).size


# ------------------------------------------------------------------------------------------------------------ scan and sums
@pytest.mark.parametrize("nt", (64, 256, 512, 1024))
def test_scan_sums_and_counts(H, nt):
    """Integer-valued inputs: every partial sum is exact, so `==` holds whatever the tree order."""
    rng = np.random.default_rng(nt)
    G = 24
    xi = rng.integers(0, 1000, (G, nt))
    xi[rng.random((G, nt)) < 0.3] = 0
    xi[0] = 0
    xi[1] = 1
    xi[2, :-1] = 0
    _, scan, tot = H.reduce(SH.RED_EXSCAN, nt, xi=xi)
    assert np.array_equal(scan, np.cumsum(xi, axis=1) - xi)
    assert np.array_equal(tot, np.repeat(xi.sum(axis=1)[:, None], nt, axis=1))
    big = rng.integers(-2 ** 40, 2 ** 40, (G, nt))
    xd = big.astype(np.float64)
    for op in (SH.RED_SUM_DYN, SH.RED_SUM_FAST):
        od, _, _ = H.reduce(op, nt, xd=xd)
        assert np.array_equal(od, np.repeat(big.sum(axis=1)[:, None], nt, axis=1).astype(np.float64)), op
    for op in (SH.RED_COUNT_DYN, SH.RED_COUNT_FAST):
        _, oi, _ = H.reduce(op, nt, xi=big)
        assert np.array_equal(oi, np.repeat(big.sum(axis=1)[:, None], nt, axis=1)), op


# ------------------------------------------------------------------------------------------------------------ bitonic sort
SORT_SIZES = tuple(2 ** m for m in range(1, 14))


@pytest.mark.parametrize("nt", (64, 256, 512, 1024))
def test_bitonic_sort(H, nt):
    """Every power of two up to 8192 keys at every block size: S = nt, 2 nt, 4 nt (keys in registers), 8 nt and S < nt (the plain
    network) are all among them, as are the remaining ratios."""
    assert {nt, 2 * nt, 4 * nt, 8 * nt, nt // 2} <= set(SORT_SIZES)
    rng = np.random.default_rng(100 + nt)
    for S in SORT_SIZES:
        G = 6
        keys = rng.integers(0, 2 ** 63, (G, S), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (G, S), dtype=np.uint64)
        keys[1] = keys[1] % np.uint64(7)                                  # heavy duplicates
        keys[2, S // 2:] = ~np.uint64(0)                                  # trailing padding as the selects write it
        keys[3] = np.sort(keys[3])[::-1]
        keys[4] = np.sort(keys[4])
        keys[5, rng.integers(0, S, max(1, S // 3))] = ~np.uint64(0)       # padding keys anywhere
        out = H.sort(nt, keys)
        assert np.array_equal(out, np.sort(keys, axis=1)), (nt, S)
        assert H.sort(nt, keys).tobytes() == out.tobytes()


# ------------------------------------------------------------------------------------------------------------ radix select
def rank_list(count):
    if count == 0:
        return []
    return sorted({0, count - 1, (count - 1) // 2, count // 10, (37 * count) // 100, (9 * count) // 10})


@pytest.mark.parametrize("nt", NTS)
def test_radix_select_and_median_over_the_grid(H, nt):
    ds = grid()
    probs = [d.problem(k) for d in ds for k in rank_list(d.count)]
    out = launch(H, SH.OP_KTH, nt, 1024, H.pack(probs))
    ok = same(out["value"], [p.data.rank(p.k) for p in probs])
    assert ok.all(), report(H, probs, ~ok)
    probs = [d.problem() for d in ds]
    out = launch(H, SH.OP_MEDIAN, nt, 1024, H.pack(probs))
    ok = same(out["value"], [d.median() for d in ds])
    assert ok.all(), report(H, probs, ~ok)


# ------------------------------------------------------------------------------------------------------------ sampled select
def check_side(H, out, probs, values_lower_bound):
    """The collect pass of the bracket hands every kept value to the Side functor exactly once, always with the same `lo`.
    side_ran <=> that pass ran and no fallback followed it; then lo is <= the returned order statistic (after a bracket miss the
    answer may lie BELOW lo: the aliased orders).  flatten's segment-cut candidates rely on both."""
    ran = out["flag"] == 1
    bracket = (out["route"] & np.uint32(H.bit("bracket"))) != 0
    gave_up = (out["route"] & np.uint32(H.bit("miss_fallback") | H.bit("refine_na_fallback") | H.bit("refine_ties_fallback"))) != 0
    assert np.array_equal(ran, bracket & ~gave_up)
    counts = np.array([p.data.count for p in probs])
    assert np.array_equal(out["side_calls"][bracket], counts[bracket]), "Side called exactly `count` times"
    assert np.all(out["side_calls"][~bracket] == 0)
    assert np.all(out["side_lo_min"][bracket] == out["side_lo_max"][bracket])
    assert np.all(out["side_lo_min"][ran] <= values_lower_bound[ran])
    assert np.all(np.isfinite(out["spacing"]) & (out["spacing"] >= 0)), "spacing finite and >= 0"


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nt", NTS)
def test_sampled_median_over_the_grid(H, nt, cap):
    ds = grid()
    probs = [d.problem() for d in ds]
    out = launch(H, SH.OP_MEDIAN_SAMPLED, nt, cap, H.pack(probs))
    ok = same(out["value"], [d.median() for d in ds])
    assert ok.all(), report(H, probs, ~ok)
    lower = np.array([d.s[(d.count - 1) // 2] if d.count else NAN for d in ds])   # the lower middle rank: lo bounds IT
    check_side(H, out, probs, lower)
    if cap == 1024:
        kept = np.array([d.count > 0 for d in ds])
        assert np.all(out["route"][kept] == H.bit("cap_small_fallback"))


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nt", NTS)
def test_sampled_select_ranks_over_the_grid(H, nt, cap):
    """The median rank, k = 0, k = count - 1 and interior quantiles, each with and without want_next."""
    ds = grid()
    probs = [d.problem(k, aux=w) for d in ds for k in rank_list(d.count) for w in (0, 1)]
    out = launch(H, SH.OP_SAMPLED, nt, cap, H.pack(probs))
    ref = np.array([p.data.rank(p.k) for p in probs])
    ok = same(out["value"], ref)
    assert ok.all(), report(H, probs, ~ok)
    want = np.array([p.aux == 1 for p in probs])
    nxt = np.array([p.data.rank(min(p.k + 1, p.data.count - 1)) for p in probs])   # rank k + 1, or rank k again at the top
    ok = same(out["next"], nxt) | ~want
    assert ok.all(), report(H, probs, ~ok)
    check_side(H, out, probs, ref)


# ------------------------------------------------------------------------------------------------------------ routes
def _uniform(seed, n):
    return np.random.default_rng(seed).uniform(0, 1, n)


def _gauss(seed, n):
    return np.random.default_rng(seed).standard_normal(n)


def _masked_gauss():
    return Data("sample_positions_dropped", _gauss(21, 8192), np.arange(8192) % 8 != 0)


def _aliased():
    rng = np.random.default_rng(22)
    i = np.arange(8192)
    return Data("aliased", np.where(i % 8 == 0, rng.uniform(0, 1, 8192), rng.uniform(10, 11, 8192)))


def _two_clusters():
    rng = np.random.default_rng(23)
    return Data("two_clusters_90000", rng.permutation(np.concatenate([rng.normal(0, 1e-6, 45_000), rng.normal(5, 1e-6, 45_000)])))


def _majority_inf():
    rng = np.random.default_rng(24)
    v = rng.standard_normal(9001)
    v[rng.choice(9001, 5000, replace=False)] = np.inf
    return Data("majority_pos_inf_9001", v)


ALL_CAPS = (2048, 4096, 4896, 5880)
# (name, data, rank: "median" or (k, want_next), {cap: routes that MUST be in the route word})
ROUTE_CASES = []


def route_cases():
    if ROUTE_CASES:
        return ROUTE_CASES
    R = ROUTE_CASES.append
    on = lambda caps, *names: {c: set(names) for c in caps}   # noqa: E731
    R(("gauss_1000", Data("gauss_1000", _gauss(1, 1000)), "median", on(ALL_CAPS, "all_in_lds", "all_hist_ok", "hist_done")))
    R(("gauss_2048", Data("gauss_2048", _gauss(2, 2048)), "median",
       {2048: {"all_in_lds", "all_sorted", "hist_na"}, **on(ALL_CAPS[1:], "all_in_lds", "all_hist_ok")}))
    R(("gauss_2047", Data("gauss_2047", _gauss(3, 2047)), "median",
       {2048: {"all_in_lds", "all_sorted", "hist_na"}, **on(ALL_CAPS[1:], "all_in_lds", "all_hist_ok")}))
    R(("constant_100", Data("constant_100", np.full(100, 3.25)), "median", on(ALL_CAPS, "all_in_lds", "all_sorted", "hist_na")))
    R(("one_value", Data("one_value", [2.5]), "median", on(ALL_CAPS, "all_in_lds", "all_sorted", "hist_na")))
    R(("small_with_infs", Data("small_with_infs", np.where(np.arange(500) % 7 == 0, np.inf, np.where(np.arange(500) % 7 == 1, -np.inf, _gauss(4, 500)))),
       "median", on(ALL_CAPS, "all_in_lds", "all_sorted", "hist_na")))
    R(("two_valued_1000", Data("two_valued_1000", np.tile([1.0, 2.0], 500)), "median", on(ALL_CAPS, "all_in_lds", "all_sorted", "hist_ties")))
    for n in (2049, 5000):
        R(("gauss_%d" % n, Data("gauss_%d" % n, _gauss(n, n)), "median",
           on(ALL_CAPS, "bracket", "cand_hist_ok", "rank_in_cand", "hist_done")))
    for n in (20_000, 30_000):
        R(("gauss_%d" % n, Data("gauss_%d" % n, _gauss(n, n)), "median",
           {2048: {"bracket", "overflow", "refined", "cand_hist_ok"},
            **on(ALL_CAPS[1:], "bracket", "cand_hist_ok", "rank_in_cand", "hist_done")}))
    R(("round1_20000", Data("round1_20000", np.round(_gauss(6, 20_000), 1)), "median",
       on(ALL_CAPS[1:], "bracket", "cand_hist_refused", "cand_sorted", "hist_ties", "rank_in_cand")))
    R(("round2_20000", Data("round2_20000", np.round(_gauss(7, 20_000), 2)), "median",
       on(ALL_CAPS[1:], "bracket", "cand_hist_refused", "cand_sorted", "hist_ties", "rank_in_cand")))
    R(("round1_5000", Data("round1_5000", np.round(_gauss(8, 5000), 1)), "median",
       on(ALL_CAPS, "bracket", "cand_hist_refused", "cand_sorted", "hist_ties", "rank_in_cand")))
    R(("constant_5000", Data("constant_5000", np.full(5000, 3.25)), "median", on(ALL_CAPS, "bracket", "rank_in_eqlo")))
    R(("two_valued_6000", Data("two_valued_6000", np.tile([1.0, 2.0], 3000)), "median",
       on(ALL_CAPS, "bracket", "rank_in_eqlo", "rank_in_eqhi")))
    R(("majority_pos_inf_9001", _majority_inf(), "median", on(ALL_CAPS, "bracket", "rank_in_eqhi")))
    g20 = Data("gauss_20000_ends", _gauss(9, 20_000))
    R(("k_first", g20, (0, 1), on(ALL_CAPS, "bracket", "pivot_lo_inf")))
    R(("k_last", g20, (19_999, 1), on(ALL_CAPS, "bracket", "pivot_hi_inf")))
    g200 = Data("gauss_200001_ends", _gauss(10, 200_001))
    R(("k_first_of_200001", g200, (0, 1), on(ALL_CAPS, "bracket", "pivot_lo_inf", "overflow", "refine_na_fallback")))
    R(("k_last_of_200001", g200, (200_000, 0), on(ALL_CAPS, "bracket", "pivot_hi_inf", "overflow", "refine_na_fallback")))
    R(("aliased", _aliased(), "median", on(ALL_CAPS, "bracket", "miss_fallback")))
    R(("sample_positions_dropped", _masked_gauss(), "median", on(ALL_CAPS, "sample_small_fallback")))
    R(("two_clusters_90000", _two_clusters(), "median", on(ALL_CAPS, "bracket", "overflow", "refine_ties_fallback")))
    # (gaussian 50 000 overflows the 2048-value list only: at cap 4096 this draw leaves 4096 or fewer inside the bracket — model
    # and device agree — so 80 000 gaussian and 150 000 uniform values carry `overflow` + `refined` for the larger caps)
    R(("gauss_50000", Data("gauss_50000", _gauss(50_000, 50_000)), "median", on((2048,), "bracket", "overflow", "refined", "rank_in_cand")))
    R(("gauss_80000", Data("gauss_80000", _gauss(80_000, 80_000)), "median", on(ALL_CAPS, "bracket", "overflow", "refined", "rank_in_cand")))
    R(("uniform_150000", Data("uniform_150000", _uniform(11, 150_000)), "median", on(ALL_CAPS, "bracket", "overflow", "refined")))
    for name, d, rank, exp in searched_cases():
        R((name, d, rank, exp))
    return ROUTE_CASES


def searched_cases():
    """Inputs found by running the route model over seeds (tests/select_route_model.py --search): the candidate radix select needs a
    candidate count between the histogram's room and `cap` with a padded sort size above `cap`; the two-bin refinement needs the
    two middle ranks of an even count to straddle a bin edge."""
    out = []
    for cap, n, seed in LDS_RADIX_INPUTS:
        out.append(("uniform_%d_seed%d" % (n, seed), Data("uniform_%d_seed%d" % (n, seed), _uniform(seed, n)), "median",
                    {cap: {"bracket", "cand_hist_refused", "hist_na", "cand_lds_radix", "rank_in_cand"}}))
    for cap, n, seed in TWO_BIN_INPUTS:
        out.append(("gauss_%d_seed%d" % (n, seed), Data("gauss_%d_seed%d" % (n, seed), _gauss(seed, n)), "median",
                    {cap: {"bracket", "overflow", "refined", "refined_two_bins"}}))
    return out


LDS_RADIX_INPUTS = ((4896, 54_000, 5), (4896, 56_000, 7), (5880, 64_000, 2), (5880, 70_000, 0))   # (cap, n, seed)
TWO_BIN_INPUTS = ((2048, 20_000, 1), (2048, 40_000, 0), (4096, 60_000, 0), (4096, 80_000, 1), (4896, 70_000, 1), (4896, 90_000, 0),
                  (5880, 80_000, 1), (5880, 100_000, 3))


def run_route_cases(H, nt, cap):
    cases = [c for c in route_cases() if cap in c[3]]
    probs = []
    for name, d, rank, exp in cases:
        if rank == "median":
            probs.append(d.problem((d.count - 1) // 2, aux=1 if d.count % 2 == 0 else 0))
        else:
            probs.append(d.problem(rank[0], aux=rank[1]))
    out = launch(H, SH.OP_SAMPLED, nt, cap, H.pack(probs))
    return cases, probs, out


@pytest.mark.parametrize("cap", ALL_CAPS)
@pytest.mark.parametrize("nt", NTS)
def test_inputs_aimed_at_each_route_take_it_and_are_exact(H, nt, cap):
    cases, probs, out = run_route_cases(H, nt, cap)
    ref = np.array([p.data.rank(p.k) for p in probs])
    ok = same(out["value"], ref)
    assert ok.all(), report(H, probs, ~ok)
    for g, p in enumerate(probs):
        if p.aux:
            assert same(out["next"][g], p.data.rank(min(p.k + 1, p.data.count - 1))), cases[g][0]
    check_side(H, out, probs, ref)
    wrong = {}
    for g, (name, d, rank, exp) in enumerate(cases):
        got = H.decode(out["route"][g])
        if not exp[cap] <= got:
            wrong[name] = (sorted(exp[cap] - got), sorted(got))
    assert not wrong, "inputs that did not take the route they were picked for (missing, taken): %r" % wrong


# ------------------------------------------------------------------------------------------------------------ block_median_near
def near_cases():
    """(name, Data, guess, width, expect ok, route)"""
    out = []
    for n in (20_000, 20_001, 3000, 3001):
        d = Data("near_gauss_%d" % n, _gauss(30 + n, n))
        m = d.median()
        # (i) the window [guess - width, guess + width] covers both middle ranks
        if n >= 20_000:
            out.append(("covers_%d" % n, d, m + 0.01, 0.05, True, "near_ok"))       # ~800 values collected
        else:
            out.append(("covers_few_%d" % n, d, m + 1e-3, 0.02, True, "near_ok"))   # ~50 values: fewer than a block, S2 = nt
        out.append(("too_narrow_%d" % n, d, m + 0.5, 0.01, False, "near_gave_up"))  # (ii)
        out.append(("guess_below_%d" % n, d, m - 0.5, 0.01, False, "near_gave_up"))
        if n >= 20_000:
            out.append(("window_over_cap_%d" % n, d, m, 10.0, False, "near_gave_up"))  # (iii) all 20 000 inside, cap <= 5880
        # (iv)
        out.append(("zero_width_%d" % n, d, m, 0.0, False, "near_refused"))
        out.append(("negative_width_%d" % n, d, m, -1.0, False, "near_refused"))
        out.append(("nan_width_%d" % n, d, m, NAN, False, "near_refused"))
        out.append(("nan_guess_%d" % n, d, NAN, 1.0, False, "near_refused"))
        out.append(("inf_guess_%d" % n, d, np.inf, 1.0, False, "near_refused"))
        out.append(("minus_inf_guess_%d" % n, d, -np.inf, 1.0, False, "near_refused"))
    out.append(("nothing_kept", Data("near_nothing_kept", _gauss(40, 300), np.zeros(300, bool)), 0.0, 1.0, False, "near_refused"))
    # (v) many values exactly on both ends of the window 1.0 +- 0.5 (exact in binary): both ends are collected
    rng = np.random.default_rng(41)
    for extra in (0, 1):   # odd and even counts
        mid = rng.uniform(0.6, 1.4, 100 + extra)
        on_hi = np.concatenate([np.full(50, 0.1), np.full(100, 0.5), mid, np.full(300, 1.5), np.full(99, 2.0)])
        on_lo = np.concatenate([np.full(99, 0.1), np.full(300, 0.5), mid, np.full(100, 1.5), np.full(50, 2.0)])
        for nm, v, med in (("median_on_upper_end", on_hi, 1.5), ("median_on_lower_end", on_lo, 0.5)):
            d = Data("%s_%d" % (nm, v.size), rng.permutation(v))
            assert d.median() == med
            out.append(("%s_%d" % (nm, v.size), d, 1.0, 0.5, True, "near_ok"))
    # even count, the two middle ranks ON the two ends: 0.5 and 1.5, median 1.0
    v = np.concatenate([np.full(200, 0.5), np.full(200, 1.5)])
    out.append(("middle_ranks_on_both_ends", Data("near_both_ends", rng.permutation(v)), 1.0, 0.5, True, "near_ok"))
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nt", NTS)
def test_median_near(H, nt, cap):
    cases = near_cases()
    probs = [d.problem(guess=g, width=w) for _, d, g, w, _, _ in cases]
    out = launch(H, SH.OP_NEAR, nt, cap, H.pack(probs))
    for i, (name, d, g, w, ok, route) in enumerate(cases):
        assert bool(out["flag"][i]) == ok, (name, "ok", out["flag"][i])
        assert H.decode(out["route"][i]) == {route}, (name, H.decode(out["route"][i]))
        if ok:
            assert same(out["value"][i], d.median()), (name, out["value"][i], d.median())
            assert out["side_lo_min"][i] == out["side_lo_max"][i] == g - w <= out["value"][i]
        if route != "near_refused":
            assert out["side_calls"][i] == d.count, name


# ------------------------------------------------------------------------------------------------------------ lds_hist_select
def hist_cases(cap):
    """(name, candidates, qa, qb, lo, hi, expect true, route).  The candidates lie strictly inside (lo, hi), as the header
    requires; 400 of them leave room for the histogram at every cap."""
    rng = np.random.default_rng(50)
    out = []
    spread = (2 * np.arange(400) + 0.5) / 1024                         # one value per bin 0, 2, 4, ...: rank r sits in bin 2 r
    out.append(("different_bins", rng.permutation(spread), 200, 201, 0.0, 1.0, True, "hist_done"))
    trio = np.concatenate([spread[:397], (400 + np.array([0.1, 0.2, 0.3])) / 1024])   # ranks 200 .. 203 share bin 400
    out.append(("same_bin", rng.permutation(trio), 201, 202, 0.0, 1.0, True, "hist_done"))
    out.append(("only_qa", rng.permutation(spread), 123, -1, 0.0, 1.0, True, "hist_done"))
    out.append(("only_qb", rng.permutation(spread), -1, 321, 0.0, 1.0, True, "hist_done"))
    out.append(("first_and_last", rng.permutation(spread), 0, 399, 0.0, 1.0, True, "hist_done"))
    ties = np.concatenate([rng.uniform(0.01, 0.4, 150), np.full(100, 0.5), rng.uniform(0.6, 0.99, 150)])
    out.append(("ties_in_wanted_bin", rng.permutation(ties), 199, 200, 0.0, 1.0, False, "hist_ties"))
    out.append(("ties_in_other_bin", rng.permutation(ties), 10, 11, 0.0, 1.0, True, "hist_done"))
    sixty = np.concatenate([rng.uniform(0.01, 0.4, 150), np.full(64, 0.5), rng.uniform(0.6, 0.99, 150)])
    out.append(("list_exactly_full", rng.permutation(sixty), 150, 213, 0.0, 1.0, True, "hist_done"))
    few = rng.uniform(0.0, 1.0, 40)
    out.append(("bracket_much_wider", few, 19, 20, -1000.0, 1000.0, True, "hist_done"))   # every value in one middle bin
    edges = np.concatenate([[np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)], rng.uniform(0.2, 0.8, 60)])
    out.append(("values_next_to_the_ends", rng.permutation(edges), 0, 61, 0.0, 1.0, True, "hist_done"))   # first and last bin
    out.append(("huge_bracket", rng.permutation(spread), 200, 201, -1.7e308, 1.7e308, False, "hist_ties"))  # hi - lo overflows: one bin
    out.append(("infinite_bracket", few, 3, 4, -np.inf, np.inf, False, "hist_na"))
    room = cap - (1024 // 2 + 64 + 2)                                  # the largest even candidate count with room
    if room + 2 <= cap:
        out.append(("no_room", rng.uniform(0.0, 1.0, room + 1), 5, 6, 0.0, 1.0, False, "hist_na"))
        out.append(("last_that_fits", rng.uniform(0.0, 1.0, room & ~1), 5, 6, 0.0, 1.0, True, "hist_done"))
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nt", NTS)
def test_hist_select(H, nt, cap):
    cases = hist_cases(cap)
    data = [Data(c[0], c[1]) for c in cases]
    probs = [d.problem(k=c[2], aux=c[3], guess=c[4], width=c[5]) for d, c in zip(data, cases)]
    out = launch(H, SH.OP_HIST, nt, cap, H.pack(probs))
    for i, (name, v, qa, qb, lo, hi, ok, route) in enumerate(cases):
        assert bool(out["flag"][i]) == ok, name
        assert H.decode(out["route"][i]) == {route}, (name, H.decode(out["route"][i]))
        if ok:
            if qa >= 0:
                assert out["value"][i] == data[i].rank(qa), name
            if qb >= 0:
                assert out["next"][i] == data[i].rank(qb), name
        else:
            assert out["untouched"][i] == 1, "%s: a refused select must leave the candidates where they were" % name


# ------------------------------------------------------------------------------------------------------------ accounting
def reachable(H, cap):
    """Every route id but the ones `cap` rules out.  (sorted_ranks' S2 > cap branch has no id: it is dead, see the header.)"""
    names = set(H.names)
    if cap < 2048:
        return {"cap_small_fallback", "near_refused", "near_gave_up", "near_ok", "hist_na", "hist_ties", "hist_done"}
    names.discard("cap_small_fallback")
    if cap & (cap - 1) == 0:
        names.discard("cand_lds_radix")   # needs a padded sort size above cap with at most cap candidates: cap not a power of two
    return names


def test_every_route_is_reached_at_every_block_size_and_cap(H):
    """ORs the route words of the aimed inputs, of block_median_near and of lds_hist_select (run here) with whatever the other
    tests of this module saw.  Every id of the enum must be reached at each block size and at each cap that admits it."""
    lines, missing = [], {}
    for nt in NTS:
        for cap in CAPS:
            if cap >= 2048:
                run_route_cases(H, nt, cap)
            else:
                launch(H, SH.OP_MEDIAN_SAMPLED, nt, cap, H.pack([Data("g", _gauss(60, 3000)).problem()]))
            launch(H, SH.OP_NEAR, nt, cap, H.pack([d.problem(guess=g, width=w) for _, d, g, w, _, _ in near_cases()]))
            launch(H, SH.OP_HIST, nt, cap, H.pack([Data(c[0], c[1]).problem(k=c[2], aux=c[3], guess=c[4], width=c[5])
                                                    for c in hist_cases(cap)]))
            got = H.decode(SEEN[(nt, cap)])
            lines.append("nt %4d cap %4d: %2d routes  %s" % (nt, cap, len(got), " ".join(sorted(got))))
            if reachable(H, cap) - got:
                missing[(nt, cap)] = sorted(reachable(H, cap) - got)
            assert got <= reachable(H, cap), (nt, cap, sorted(got - reachable(H, cap)))
    union = set().union(*(H.decode(w) for w in SEEN.values()))
    print("\nroutes reached: %d of %d: %s" % (len(union), len(H.names), " ".join(n for n in H.names if n in union)))
    print("\n".join(lines))
    assert not missing, "routes never reached: %r" % missing
    assert union == set(H.names)
