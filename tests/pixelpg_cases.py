"""The cases the CPU and GPU tests of the per-pixel periodograms share (tests/test_pixelpg_cpu.py, tests/test_pixelpg_gpu.py):
the cutouts of tests/ampimage_cases.py (``ampimage_cases.case(shape, N, 1)``), a frequency grid per cube length, and the numpy
mirror's answer, computed once.

What the case holds and the path it exercises: three cutouts (batch handling); NaN times and one whole-NaN cadence in cutout 0
(dropped cadences; every pixel of cutout 0 lacks the whole-NaN cadence, so all of it takes the correction path, cutouts 1 and 2
take the path without); an all-NaN pixel (n_used == 0); pixels with 3 and 2 values (the n_used < 4 rule); a pixel with a tenth of
its values NaN (the NaN correction); a variable neighbour 3 px from the star (the peak images).

Grid: np.linspace(1.5 / T, 0.25 / CADENCE, F), T the span of the finite times (the same for the three cutouts: the NaN times
of cutout 0 are never its first or last).  Below about one cycle per baseline the closed form's CC / SS lose digits in the
reference itself.  N = 7 is not used: its span admits no grid between 1.5 / T and a quarter of the sampling rate."""
import functools

import numpy as np

import ampimage_cases as A

CADENCE = A.CADENCE
SHAPES = A.SHAPES
NS = (20, 127, 128, 129, 300)
B = A.B
# the kernel works on tiles of 16 frequencies: one below, at and one above a tile, and a grid that spans three tiles
TILE_FS = (15, 16, 17, 40)
TILE_CASE = ((11, 11), 129)
UHZ_PER_CPD = 1e6 / 86400.0


def n_freq(N):
    return 5 if N == 20 else 37


def case(shape, N):
    """-> (time (B, N), flux (B, N, ny, nx) float32, flux_err) of ampimage_cases.  Read-only."""
    return A.case(shape, N, 1)[:3]


def grid(N, F=None):
    """The grid [1/d] of the cubes of N cadences."""
    time = A.case(SHAPES[0], N, 1)[0]
    t = time[np.isfinite(time)]
    return np.linspace(1.5 / (t.max() - t.min()), 0.25 / CADENCE, n_freq(N) if F is None else F)


def stack(per_cutout):
    return {k: np.stack([np.asarray(o[k]) for o in per_cutout]) for k in per_cutout[0] if k != "frequency"}


@functools.lru_cache(maxsize=None)
def mirror(shape, N, normalization="amplitude", F=None):
    """PixelCube.pixel_periodogram of every cutout of case() on grid(N, F), stacked -> dict of arrays with the batch axis (and
    ``frequency`` (F,) in 1/d).  'psd' takes the grid in microhertz, its default unit.  Read-only."""
    from lightkurve_amd.correctors import PixelCube
    time, flux, err = case(shape, N)
    f = grid(N, F) * (UHZ_PER_CPD if normalization == "psd" else 1.0)
    per = [PixelCube(time[b], flux[b], err[b]).pixel_periodogram(f, normalization) for b in range(B)]
    out = stack(per)
    out["frequency"] = per[0]["frequency"]
    for a in out.values():
        a.setflags(write=False)
    return out


def top_two_gap(power):
    """power (..., F, ny, nx) -> (largest - second largest) / largest of every pixel's finite powers over the F axis (the
    batch axes kept); NaN for a pixel with fewer than two."""
    p = np.moveaxis(np.asarray(power, dtype=np.float64), -3, -1)
    s = np.sort(np.where(np.isnan(p), -np.inf, p), axis=-1)
    with np.errstate(all="ignore"):
        gap = (s[..., -1] - s[..., -2]) / s[..., -1]
    return np.where(np.isfinite(s[..., -2]), gap, np.nan)
