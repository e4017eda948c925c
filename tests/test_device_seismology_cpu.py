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
