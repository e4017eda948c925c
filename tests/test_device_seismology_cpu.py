"""CPU: the host side of the resident seismology chain (DevicePeriodogramBatch, lk_pg_deltanu_batch): the per-target
deltanu planner against the reference's own expressions, the new C-ABI symbols, and the loud failure without a GPU."""
import os
import re

import numpy as np
import pytest

import seismology_cases as cases
from lightkurve_amd import _capi, seismology
from lightkurve_amd.device import DevicePeriodogramBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lk_pg_snr_batch_dev", "lk_pg_acf_metric_batch_dev", "lk_pg_numax_pick_batch_dev", "lk_pg_deltanu_batch",
               "lk_pg_deltanu_batch_dev")


@pytest.mark.parametrize("grid", ["rg", "ms"])
def test_deltanu_plan_matches_the_reference_expressions(grid):
    """start, W, distance and the selected run of lags of seismology._deltanu_plan == the reference's lines evaluated per
    target with the full np.linspace mask: the five true numax values and 200 random ones inside the grid."""
    f = cases.GRIDS[grid]
    rng = np.random.default_rng(7 if grid == "rg" else 8)
    numaxs = np.concatenate([sum(cases.TRUE_NUMAX.values(), ()), rng.uniform(f[0] + 1.0, f[-1], 200)])
    plan = seismology._deltanu_plan(f, "uHz", numaxs)
    usable = 0
    for b, nm in enumerate(numaxs):
        ref = cases.reference_deltanu_plan(f, float(nm))
        assert plan["deltanu_emp"][b] == ref["deltanu_emp"] and plan["distance"][b] == ref["distance"]
        if ref["width"] < 2:
            assert plan["width"][b] == 0 and plan["start"][b] == -1
            continue
        usable += 1
        assert (plan["start"][b], plan["width"][b]) == (ref["start"], ref["width"])
        assert plan["stop"][b] == ref["lags"][-1] and plan["step"][b] == ref["lags"][1]
        idx = np.flatnonzero(ref["sel"])
        assert plan["sel_len"][b] == idx.size
        if idx.size:
            assert plan["sel_lo"][b] == idx[0] and idx[-1] - idx[0] + 1 == idx.size      # one run
    assert usable > 150


def test_deltanu_plan_marks_what_it_cannot_window():
    f = cases.GRIDS["rg"]
    plan = seismology._deltanu_plan(f, "uHz", np.array([np.nan, -3.0, 0.0, np.inf, 1.0, 120.0]))
    assert np.isnan(plan["deltanu_emp"][:4]).all() and np.isfinite(plan["deltanu_emp"][4:]).all()
    assert plan["width"][4] == 0 and plan["start"][4] == -1          # fwhm below one microhertz: an empty window
    assert plan["width"][5] == 880


def test_new_symbols_are_declared_and_typed():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lkhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lk_[a-z0-9_]+)\s*\(", src))
    typed = {s[0]: s for s in _capi.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared and name in typed, name
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert len(getattr(lib, name).argtypes) == len(typed[name][2])


def test_from_arrays_needs_a_gpu():
    """Like every resident constructor: no GPU, no object (there is no CPU fallback)."""
    f, power, _ = cases.batch("rg")
    if _capi.device_count() > 0:
        assert len(DevicePeriodogramBatch.from_arrays(f, power)) == 3
    else:
        with pytest.raises((RuntimeError, ValueError)):
            DevicePeriodogramBatch.from_arrays(f, power)
    with pytest.raises(ValueError):
        DevicePeriodogramBatch.from_arrays(f[:-1], power)


# ------------------------------------------------------------------------------------------------ the exact cases, on numpy alone
EXACT = [c for c in cases.CASES + cases.TRUNCATED_PAIR if c["h"] is not None]
OK_CASES = [c for c in cases.CASES + cases.TRUNCATED_PAIR if c["status"] == 0]


def test_case_table_holds_what_the_kernel_has_to_meet():
    names = [c["name"] for c in cases.CASES]
    assert len(set(names)) == len(names)
    n = {c["name"]: c["sel_len"] for c in cases.CASES}
    assert n["many_n299_distance_1"] == 299 and n["many_n999_distance_1"] == 999 and n["n2"] == 2 and n["n3_middle_highest"] == 3
    assert cases.CASE["many_n299_distance_n_plus_10"]["distance"] == 299 + 10 and cases.CASE["many_n999_distance_n_plus_10"]["distance"] == 999 + 10
    assert cases.CASE["many_n999_distance_1"]["maxima"] > 256                       # more than one trip of the compaction
    full, over = cases.CASE["w16384_lds_exactly_full"], cases.CASE["w16384_lds_one_lag_too_many"]
    assert full["W"] + 16 + full["sel_len"] == cases.LDS_DOUBLES == over["W"] + 16 + over["sel_len"] - 1
    last = cases.CASE["selection_to_last_lag"]
    assert last["sel_lo"] + last["sel_len"] == last["W"] and last["stop"] != (last["W"] - 1) * last["step"]
    assert last["winner"] == last["sel_len"] - 2
    edges = cases.CASE["maxima_at_slice_edges"]
    assert np.array_equal(cases.case_reference(edges)[0]["maxima"], [1, edges["sel_len"] - 2])
    for c in cases.CASES:
        if c["name"].startswith("production_lags"):                                # np.linspace(0, W fs, W)
            assert c["step"] == c["stop"] / (c["W"] - 1) and c["step"] not in (0.5, 1.0)
    for c in cases.CASES:
        if c["group"] != "refused" or c["name"] in ("understated_sel_len_alone", "w16384_lds_one_lag_too_many"):
            assert 0 <= c["start"] and c["start"] + c["W"] <= cases.M_EXACT, c["name"]
    assert cases.CASE["start_minus_1"]["start"] == -1 and cases.CASE["w1"]["W"] == 1 and cases.CASE["w16385"]["W"] == 16385
    c = cases.CASE["ends_past_the_row"]
    assert c["start"] + c["W"] == cases.M_EXACT + 1
    short, wide = cases.TRUNCATED_PAIR
    max_sel = max(short["plan_sel_len"], wide["plan_sel_len"])
    assert max_sel < short["sel_len"] and short["W"] + 16 + short["sel_len"] <= wide["W"] + 16 + max_sel       # fits beside it
    assert short["W"] + 16 + short["sel_len"] > short["W"] + 16 + short["plan_sel_len"]                        # and not alone


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c["name"])
def test_exact_window_is_exact_on_numpy(c):
    """The construction's promises, with ==: zero sum, C[sel] = A h, the slice ordered as h is."""
    p, h, lo, n = c["window"], c["h"], c["sel_lo"], c["sel_len"]
    assert len(h) == n and n <= lo and p.sum() == 0 and np.nanmean(p) == 0
    C, acf, lo_ref, n_ref = cases.reference_acf(p, c["emp"], c["step"], c["stop"])
    assert (lo_ref, n_ref) == (lo, n)
    assert np.array_equal(C[lo:lo + n], p[0] * h) and C[0] == p[0] ** 2 + np.sum(h ** 2) and C[0] < 2.0 ** 53
    assert np.array_equal(np.sign(np.diff(acf[lo:lo + n])), np.sign(np.diff(h)))


@pytest.mark.parametrize("c", OK_CASES, ids=lambda c: c["name"])
def test_case_is_what_its_name_claims(c):
    ref, x = cases.case_reference(c)
    h = c["h"]
    maxima = seismology._local_maxima_1d(h.astype(np.float64))
    assert np.array_equal(ref["maxima"], maxima) and len(maxima) == c["maxima"]
    assert len(ref["peaks"]) == c["survivors"] and ref["winner"] == c["winner"]
    assert ref["deltanu"] == cases.lags_of(c["W"], c["step"], c["stop"])[c["sel_lo"] + c["winner"]]
    # equally high maxima closer than ceil(distance): only in the group that is about them
    dist = int(min(np.ceil(c["distance"]), 2 ** 31 - 1))
    clash = any(h[a] == h[b] and b - a < dist for i, a in enumerate(maxima) for b in maxima[i + 1:])
    assert clash == (c["group"] == "equal")
    if c["group"] == "equal":
        assert np.array_equal(ref["peaks"], cases.find_peaks_stable(h, c["distance"]))
    else:
        assert np.array_equal(ref["peaks"], seismology._find_peaks(h, c["distance"]))
        assert np.array_equal(ref["peaks"], cases.find_peaks_stable(x, c["distance"]))
    d = np.abs(ref["lags"][ref["peaks"]] - c["emp"])
    assert (np.sum(d == d.min()) > 1) == c["tie"]
    if c["tie"]:
        assert ref["winner"] == ref["peaks"][0] and d[0] == d[1]
    try:
        from scipy.signal import find_peaks
    except ImportError:
        return
    assert np.array_equal(find_peaks(x, distance=c["distance"])[0], ref["peaks"])     # (equal heights: scipy agrees at this size)
    assert np.array_equal(find_peaks(h, distance=c["distance"])[0], ref["peaks"])


@pytest.mark.parametrize("c", [c for c in cases.CASES if c["status"] == 3], ids=lambda c: c["name"])
def test_status_3_cases_leave_the_reference_nothing(c):
    assert cases.case_reference(c)[0] is None
    _, acf, lo, n = cases.reference_acf(c["window"], c["emp"], c["step"], c["stop"])
    x = acf[lo:lo + n]
    if n >= 3 and c["distance"] >= 1:
        assert len(seismology._find_peaks(x, c["distance"])) == 0
        with pytest.raises(ValueError):
            np.argmin(np.abs(cases.lags_of(c["W"], c["step"], c["stop"])[lo:lo + n][:0] - c["emp"]))
    elif n >= 3:
        with pytest.raises(ValueError):          # scipy: `distance` must be >= 1; NaN fails in its integer conversion
            seismology._find_peaks(x, c["distance"])
    else:
        assert len(seismology._find_peaks(x, c["distance"])) == 0
    if c["name"] in ("constant_window", "one_nan"):
        assert np.isnan(x).all()
    if c["name"] == "monotone":
        assert np.all(np.diff(x) > 0)


@pytest.mark.parametrize("grid", ["rg", "ms"])
def test_production_ratio_never_keeps_two_peaks(grid):
    """With distance = floor(emp / 2 / fs) the slice is too short for two surviving maxima (they lie in [1, n - 2]): the
    two-survivor cases of the table therefore halve the distance, and the resident path can only show one survivor."""
    f = cases.GRIDS[grid]
    plan = seismology._deltanu_plan(f, "uHz", np.linspace(f[0] + 5.0, f[-1] - 5.0, 400))
    ok = plan["width"] >= 2
    assert ok.sum() > 300 and np.all(plan["sel_len"][ok] - 3 < plan["distance"][ok])
    pl = cases.reference_deltanu_plan(f, cases.PRODUCTION_NUMAX[grid])
    c = cases.CASE["production_lags_" + grid]
    assert (c["W"], c["emp"], c["distance"], c["step"], c["stop"]) == (pl["width"], pl["deltanu_emp"], pl["distance"], pl["lags"][1], pl["lags"][-1])
    assert 0 <= pl["start"] and pl["start"] + pl["width"] <= cases.M
