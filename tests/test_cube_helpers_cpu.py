"""CPU: the host helpers of lightkurve_amd/cubes.py that every image method shares (``_per_cutout``, ``_first_finite_times``)
and the two import orders of cubes.py and device.py, each in a fresh interpreter."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lightkurve_amd.cubes import _first_finite_times, _per_cutout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_cutout_broadcasts_a_scalar_and_takes_one_value_per_cutout():
    for given, want in ((2.5, [2.5, 2.5, 2.5]), (np.array([1, 2, 3], dtype=np.int32), [1.0, 2.0, 3.0]),
                        (np.arange(6.0)[::2], [0.0, 2.0, 4.0])):
        got = _per_cutout("period", given, 3)
        assert got.dtype == np.float64 and got.shape == (3,) and got.flags.c_contiguous and got.tolist() == want


def test_per_cutout_names_the_argument_it_rejects():
    with pytest.raises(ValueError) as err:
        _per_cutout("period", np.ones(2), 3)
    assert str(err.value) == "period must be a scalar or one value per cutout (3), got shape (2,)"
    with pytest.raises(ValueError) as err:
        _per_cutout("duration", np.ones((3, 1)), 3)
    assert str(err.value) == "duration must be a scalar or one value per cutout (3), got shape (3, 1)"
    for bad in (np.inf, [1.0, -np.inf, 2.0], np.nan):
        with pytest.raises(ValueError) as err:
            _per_cutout("transit_time", bad, 3)
        assert str(err.value) == "transit_time must be finite"


def test_per_cutout_lets_nan_through_where_the_kernel_reports_it():
    got = _per_cutout("frequency", [1.0, np.nan, 3.0], 3, finite=False)
    assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, [1.0, np.nan, 3.0], equal_nan=True)
    assert np.isnan(_per_cutout("frequency", np.nan, 3, finite=False)).all()
    with pytest.raises(ValueError, match=r"frequency must be a scalar or one value per cutout \(3\), got shape \(2,\)"):
        _per_cutout("frequency", [1.0, np.nan], 3, finite=False)


def test_first_finite_times():
    nan, inf = np.nan, np.inf
    time = np.array([[nan, nan, 3.5, 4.0],
                     [nan, nan, nan, nan],
                     [inf, -inf, nan, 7.25],
                     [1.0, nan, 2.0, 3.0]])
    got = _first_finite_times(time)
    assert got.dtype == np.float64 and got.shape == (4,) and got.flags.c_contiguous
    assert np.array_equal(got, [3.5, nan, 7.25, 1.0], equal_nan=True)


@pytest.mark.parametrize("first, second", [("cubes", "device"), ("device", "cubes")])
def test_either_module_can_be_the_first_import(first, second):
    code = ("import sys; sys.path.insert(0, %r)\nimport lightkurve_amd.%s\nimport lightkurve_amd.%s\n"
            "assert lightkurve_amd.device.DevicePixelCubeBatch is lightkurve_amd.cubes.DevicePixelCubeBatch\n" % (ROOT, first, second))
    run = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0, run.stderr
