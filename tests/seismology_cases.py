"""Inputs of the resident seismology tests (test_device_seismology_cpu.py / _gpu.py): two grids of 3000 frequencies and
five synthetic oscillation spectra, and the reference's deltanu planning written with its own expressions."""
import numpy as np

from lightkurve_amd import seismology

M = 3000
GRIDS = {"rg": np.arange(50, 3050) * 0.1, "ms": np.arange(300, 3300) * 1.0}      # microhertz
TRUE_NUMAX = {"rg": (60.0, 120.0, 200.0), "ms": (1200.0, 2000.0)}


def spectrum(grid, numax, i):
    """Envelope of Lorentzian modes (radial, an l=2 neighbour, the l=1 ridge half way) times chi^2_2 noise, seed 100 + i."""
    f, ms = GRIDS[grid], grid == "ms"
    fs = f[1] - f[0]
    rng = np.random.default_rng(100 + i)
    dnu = 0.294 * numax ** 0.772
    fwhm = 0.25 * numax if ms else 0.66 * numax ** 0.88
    env = np.exp(-0.5 * ((f - numax) / (fwhm / 2.355)) ** 2)
    width = max(2 * fs, 0.02 * dnu)
    modes = np.zeros(M)
    for n in range(-12, 13):
        for off, h in ((0.0, 1.0), (-0.13 * dnu, 0.6), (0.5 * dnu, 0.8)):
            modes += h / (1 + ((f - (numax + n * dnu + off)) / width) ** 2)
    return (1 + 25 * env * modes) * rng.exponential(size=M)


def batch(grid):
    """(frequency, power[B, M], true numax[B]); spectrum k of a grid has seed 100 + k."""
    nm = TRUE_NUMAX[grid]
    return GRIDS[grid], np.stack([spectrum(grid, v, k) for k, v in enumerate(nm)]), np.array(nm)


def reference_deltanu_plan(frequency, numax):
    """What estimate_deltanu_acf2d derives from numax, by its own lines (seismology.py, deltanu_estimators.py:95-126): the
    window, the distance and the selection as the full mask over np.linspace.  Frequencies in microhertz."""
    fs = np.median(np.diff(frequency))
    deltanu_emp = 0.294 * numax ** 0.772
    fwhm = 0.25 * numax if frequency[-1] > 500.0 else 0.66 * numax ** 0.88
    window_width = 2 * int(np.floor(fwhm))
    start, W = seismology._window_start(frequency, numax, window_width, fs)
    lags = np.linspace(0.0, W * fs, W)
    sel = (lags > deltanu_emp - 0.25 * deltanu_emp) & (lags < deltanu_emp + 0.25 * deltanu_emp)
    return dict(start=start, width=W, deltanu_emp=deltanu_emp, distance=np.floor(deltanu_emp / 2.0 / fs), lags=lags, sel=sel)
