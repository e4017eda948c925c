"""Deterministic cutouts for the background tests (test_background_cpu.py, test_background_gpu.py) and the plain restatement
of ``np.nanmedian(axis=1)`` the mirror ``PixelCube.estimate_background`` is held to.

A cutout is a Gaussian star on a per-cadence background ramp plus noise, float32.  Planted, by cadence index (a cutout of N
cadences has the features whose cadence it reaches; every cutout of a batch has them at the same cadences):

    0  pixel (0, 0) is NaN                                   the selected count flips between odd and even
    1  every pixel but the central one is NaN                no background value at all: NaN background
    2  +inf at pixel (0, nx - 1)
    3  -inf at pixel (ny - 1, 0)
    4  +inf at (0, nx - 1) and -inf at (ny - 1, 0)           the two-pixel mask below selects exactly these: inf + -inf = NaN
    5  pixels (0, 0) and (0, 1) are NaN                      the count flips back
    7  every pixel outside the central 3 x 3 is +inf         the median is +inf and sel - bkg = inf - inf = NaN in the scatter

Cutout 1 of every batch is quantised to small integers: the middle ranks sit inside runs of equal values.
"""
import functools

import numpy as np

from lightkurve_amd.correctors import PixelCube

SEED = 20261020
SHAPES = ((3, 4), (5, 5), (11, 11))          # npix = 25 and 121 are no multiples of 4: misaligned heads and tails in the staging
CADENCES = (1, 63, 64, 65, 130)              # 64 cadences are one tile of the small route
BATCHES = (1, 3)
MASKS = ("background", "all", "shared", "per cutout", "tiny")
ROUTE_CUT_NPIX = 224                         # cube_background_kernel up to here, cube_background_wide_kernel beyond (pixcube.hip)
CUT_SHAPES = ((14, 16), (15, 15))            # npix = 224 and 225: the last of the small route and the first of the wide one
LARGE_SHAPE, LARGE_N = (65, 65), 3           # more pixels than CUBE_MASK_MAX_NPIX: explicit masks only

ALL_NAN, INF_MEDIAN = 1, 7                   # the cadences of the table above that later tests name


def times(N):
    return 1000.0 + np.arange(N) / 48.0


@functools.lru_cache(maxsize=None)
def cutout_flux(shape, N, b):
    """float32 (N, ny, nx), read-only: cutout ``b`` of the batch of this shape and length."""
    ny, nx = shape
    rng = np.random.default_rng([SEED, ny, nx, N, b])
    yy, xx = np.indices(shape)
    cy, cx = (ny - 1) // 2, (nx - 1) // 2
    star = (900.0 + 100.0 * b) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 1.62)
    ramp = 40.0 + 0.25 * np.arange(N) + 3.0 * b
    flux = star[None] + ramp[:, None, None] + 2.0 * rng.standard_normal((N, ny, nx))
    if b == 1:
        flux = np.round(flux / 2.0)           # background values on a handful of integers
    flux = flux.astype(np.float32)
    plant = {0: [((0, 0), np.nan)], 2: [((0, nx - 1), np.inf)], 3: [((ny - 1, 0), -np.inf)],
             4: [((0, nx - 1), np.inf), ((ny - 1, 0), -np.inf)], 5: [((0, 0), np.nan), ((0, 1), np.nan)]}
    for i, items in plant.items():
        if i < N:
            for (y, x), v in items:
                flux[i, y, x] = v
    if ALL_NAN < N:
        keep = flux[ALL_NAN, cy, cx]
        flux[ALL_NAN] = np.nan
        flux[ALL_NAN, cy, cx] = keep
    if INF_MEDIAN < N:
        core = flux[INF_MEDIAN, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2].copy()
        flux[INF_MEDIAN] = np.inf
        flux[INF_MEDIAN, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = core
    flux.setflags(write=False)
    return flux


def cubes(shape, N, B, first=0):
    """The batch as host ``PixelCube``s (fresh objects over the shared read-only flux)."""
    out = []
    for b in range(first, first + B):
        flux = cutout_flux(shape, N, b)
        out.append(PixelCube(times(N), flux, np.full(flux.shape, 1.5, dtype=np.float32), targetid=100 + b))
    return out


def shared_mask(shape):
    """A bool (ny, nx) mask: the outer frame plus one inner pixel, so it holds the planted corners."""
    m = np.ones(shape, dtype=bool)
    m[1:-1, 1:-1] = False
    m[shape[0] // 2, 0] = False
    m[min(1, shape[0] - 1), min(1, shape[1] - 1)] = True
    return m


def per_cutout_masks(shape, B):
    """bool (B, ny, nx) of different sizes: every (b + 2)-th pixel from pixel b on."""
    npix = shape[0] * shape[1]
    m = np.zeros((B, npix), dtype=bool)
    for b in range(B):
        m[b, b::b + 2] = True
    return m.reshape((B,) + shape)


def tiny_masks(shape, B):
    """bool (B, ny, nx): cutout b gets ((b + 2) % 3) pixels - two (the +-inf corners), none, one, ..."""
    ny, nx = shape
    m = np.zeros((B,) + shape, dtype=bool)
    for b in range(B):
        k = (b + 2) % 3
        if k == 2:
            m[b, 0, nx - 1] = m[b, ny - 1, 0] = True
        elif k == 1:
            m[b, 0, 0] = True
    return m


def mask_spec(name, shape, B):
    """-> (what the batch call takes, what cutout b's mirror call takes)"""
    if name in ("background", "all"):
        return name, [name] * B
    if name == "shared":
        return shared_mask(shape), [shared_mask(shape)] * B
    per = per_cutout_masks(shape, B) if name == "per cutout" else tiny_masks(shape, B)
    return per, list(per)


def sorted_nanmedian_rows(sel):
    """The restatement: per row, sort the values that are not NaN, take the middle one or add the middle two and halve, in
    float32.  No value: NaN."""
    sel = np.asarray(sel, dtype=np.float32)
    out = np.full(sel.shape[0], np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i, row in enumerate(sel):
            v = np.sort(row[~np.isnan(row)])
            n = len(v)
            if n:
                out[i] = v[n // 2] if n % 2 else np.float32(v[n // 2 - 1] + v[n // 2]) / np.float32(2)
    return out


def restated_background(cube, mask):
    """``PixelCube.estimate_background`` restated: (flux, n_pixels, scatter) over the bool ``mask``."""
    sel = np.asarray(cube.flux, dtype=np.float32)[:, mask]
    flux = sorted_nanmedian_rows(sel)
    with np.errstate(all="ignore"):
        scatter = sorted_nanmedian_rows(np.abs(sel - flux[:, None]))
    return flux, np.sum(~np.isnan(sel), axis=1).astype(np.int32), scatter


@functools.lru_cache(maxsize=None)
def mirror(shape, N, B, name, first=0):
    """The mirror's answer for the batch, computed once and shared (read-only): a list of B dicts of
    ``PixelCube.estimate_background(mask, return_scatter=True)`` plus ``subtracted``, the float32 (N, ny, nx) flux of
    ``subtract_background``, and ``meta``, its meta."""
    out = []
    for cube, spec in zip(cubes(shape, N, B, first), mask_spec(name, shape, B)[1]):
        est = cube.estimate_background(spec, return_scatter=True)
        sub = cube.subtract_background(aperture_mask=spec)
        est["subtracted"], est["meta"] = sub.flux, sub.meta
        for v in est.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(est)
    return out
