"""No GPU: the ragged shared-design-matrix regression's declarations, the checks of DeviceLightCurveBatch.regression_correct /
.cbv_correct (rows= / cadenceno=) that come before any device call, and the reference-side clip margins of the generated cases
(regress_rows_cases.py) that test_regress_rows_gpu.py compares against."""
import os
import re

import numpy as np
import pytest

from lightkurve_amd import _capi
from lightkurve_amd import device as D

import regress_rows_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lk_regress_shared_rows_batch": 18, "lk_regress_shared_rows_batch_dev": 19, "lk_align_rows_batch": 8,
       "lk_align_rows_batch_dev": 9, "lk_ridge_prior_rows_batch": 8, "lk_ridge_prior_rows_batch_dev": 9,
       "lk_ridge_prior_rows_alphas_batch": 8, "lk_ridge_prior_rows_alphas_batch_dev": 9, "lk_fits_cadenceno_batch": 9,
       "lk_fits_cadenceno_batch_dev": 10}


def test_new_entry_points_are_declared_in_the_header_and_the_ctypes_table():
    text = open(os.path.join(ROOT, "include", "lkhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = {s[0]: s for s in _capi.SIGNATURES}
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m is not None and name in table, name
        assert len(m.group(1).split(",")) == nargs == len(table[name][2]), name
    # lk_fits_unpack_batch keeps its arguments: CADENCENO has an entry of its own
    assert len(table["lk_fits_unpack_batch"][2]) == 11 and len(table["lk_fits_unpack_batch_dev"][2]) == 12


def _batch_without_a_device(n_off, cadenceno=False):
    """A DeviceLightCurveBatch with offsets only: enough for the checks that run before the first device call."""
    b = object.__new__(D.DeviceLightCurveBatch)
    b.n_off = np.asarray(n_off, dtype=np.int64)
    b.d_cadenceno = object() if cadenceno else None
    return b


def test_the_uniform_message_is_untouched_without_rows_or_cadenceno():
    X = np.ones((100, 3))
    ragged = _batch_without_a_device([0, 100, 190])
    msg = ("regression_correct needs one cadence count for every target: this batch has between 90 and 100 cadences per target "
           "and the design matrix has 100 rows (regression_correct_batch takes ragged batches)")
    with pytest.raises(ValueError) as ei:
        ragged.regression_correct(X)
    assert str(ei.value) == msg
    with pytest.raises(ValueError) as ei:
        ragged.cbv_correct(np.ones((100, 16)))
    assert str(ei.value) == msg.replace("regression_correct needs", "cbv_correct needs")


def test_ragged_arguments_are_checked_before_any_device_call():
    X = np.ones((100, 3))
    b = _batch_without_a_device([0, 100, 190], cadenceno=True)
    grid = np.arange(100) + 7
    rows = np.r_[np.arange(100), np.arange(90)]
    with pytest.raises(ValueError, match="not both"):
        b.regression_correct(X, rows=rows, cadenceno=grid)
    for bad in (rows[:-1], rows.reshape(2, 95), rows.astype(float)):
        with pytest.raises(ValueError, match=r"rows must be an integer array of shape \(190,\)"):
            b.regression_correct(X, rows=bad)
    for bad in (np.r_[rows[:-1], 100], np.r_[-1, rows[1:]]):
        with pytest.raises(ValueError, match="indices into the 100 rows"):
            b.regression_correct(X, rows=bad)
    for bad in (grid[:-1], grid.astype(float), grid.reshape(10, 10)):
        with pytest.raises(ValueError, match=r"cadenceno .* integer array of shape \(100,\)"):
            b.regression_correct(X, cadenceno=bad)
        with pytest.raises(ValueError, match=r"cadenceno .* integer array of shape \(100,\)"):
            b.cbv_correct(np.ones((100, 16)), cadenceno=bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        b.regression_correct(X, cadenceno=np.r_[grid[:50], grid[49:-1]])
    # the ragged cadence mask: one entry per cadence of the batch
    for bad in (np.ones((2, 100), bool), np.ones(189, bool)):
        with pytest.raises(ValueError, match=r"cadence_mask is ragged.*\(190,\)"):
            b.regression_correct(X, cadence_mask=bad, rows=rows)
        with pytest.raises(ValueError, match=r"cadence_mask is ragged.*\(190,\)"):
            b.cbv_correct(np.ones((100, 16)), cadence_mask=bad, cadenceno=grid)
    # a batch without cadence numbers
    plain = _batch_without_a_device([0, 100, 190])
    with pytest.raises(ValueError, match="carries cadence numbers"):
        plain.regression_correct(X, cadenceno=grid)
    with pytest.raises(ValueError, match="carries cadence numbers"):
        plain.cbv_correct(np.ones((100, 16)), cadenceno=grid)
    with pytest.raises(ValueError, match="one penalty per target"):
        b.cbv_correct(np.ones((100, 16)), alpha=[1.0, 2.0, 3.0], cadenceno=grid)
    with pytest.raises(ValueError, match="both"):
        b.regression_correct(X, prior_mu=np.zeros(3), rows=rows)


@pytest.mark.parametrize("seed,B,N,K", C.CONFIGS)
def test_generated_cases_keep_their_clip_margins(seed, B, N, K):
    """problem() asserts margin > 1e-3 sd per target; the worst of each configuration is what the GPU tests' docstring quotes."""
    rg, refs = C.problem(seed, B, N, K)
    counts = np.diff(rg.n_off)
    assert len(refs) == B and counts.min() >= 325 and counts.max() == N and (counts < N).sum() >= B - (B + 4) // 5
    assert np.array_equal(counts[::5], np.full(len(counts[::5]), N))             # every fifth target keeps all rows
    assert rg.rows_b[1][0] >= N // 3 and rg.rows_b[2][-1] < N - N // 3           # whole leading / trailing slices absent
    assert all(np.all(np.diff(r) > 0) for r in rg.rows_b)
    worst = min(C.clip_margin(rg.X[r], rg.y[rg.sl(b)], rg.err[rg.sl(b)], rg.cm[rg.sl(b)]) for b, r in enumerate(rg.rows_b))
    assert 0.01 < worst < 0.1
    assert not rg.y.flags.writeable and not rg.X.flags.writeable


def test_cadenceno_array_helper():
    a = D._cadenceno_array(np.arange(5, dtype=np.int64), 5, "x")
    assert a.dtype == np.int32 and a.flags.c_contiguous
    with pytest.raises(ValueError, match="fit int32"):
        D._cadenceno_array(np.array([0, 2 ** 31]), 2, "x")
