"""Seeded synthetic scenes for the PSF fit with a pointing shift per cadence and a TABULATED PRF (PixelCube.psf_fit(prf=),
DevicePixelCubeBatch.psf_fit(prf=)), independent evaluations of the model and of its gradient, and a joint reference fit.

The scenes are psffit_cases.py's plan on prfphot_cases.py's tables: rendered WITH their true per-cadence shifts (uniform in
+-0.3 px) by the per-pixel ``prfphot_cases.prf_image`` at the stars' positions, photon-like noise e = sqrt(|img| + 4), float32;
the stars are at least 1.5 px apart and inside the cutout (psfphot_cases.star_grid).  ``prf_index`` of cutout b is b % n_prf.

A scene is a batch of cutouts of one shape:
  0  clean: nothing missing, every cadence ok with the defaults;
  1  NaN pixels, one cadence that is NaN throughout (too few pixels: status 2), flux_err of 0, NaN and inf, a NaN time, a NaN
     entry in shifts0 and a per-cutout mask that removes pixels;
  2  one star fewer than the batch's widest (S >= 2): the NaN padding sits in slot 0;
  3  (S >= 2) stars 0 and 1 at the same position: singular at every cadence, so the cutout's status is 1;
  4  (S >= 2) star 1 is 30.3137 px from the cutout, farther than any table reaches: its model and its derivative are zero on every
     pixel, status 3 at every cadence through the pivot cut.

The independent gradient (``prf_gradient_image``) is Keys' kernel's derivative written as the piecewise function of |x| — sign(x)
(4.5 x^2 - 5 |x|) up to 1, sign(x) (-1.5 x^2 + 5 |x| - 4) up to 2 — applied per pixel, in a plain loop, to a zero-padded table,
in the manner of ``prf_image``.  The reference fit is scipy.optimize.least_squares over (theta, dc, dr) jointly on a model
evaluated by ``prf_image``, with scipy's own finite-difference Jacobian: no variable projection, no derivative weights.
"""
import functools

import numpy as np

from prfphot_cases import TABLE_OF, keys, prf_image, prf_object, table
from psffit_cases import DEFAULTS, SETTINGS
from psfphot_cases import COLUMN, ROW, star_grid

# The thresholds of prffit.hip.  TILE: cadences per workgroup of cube_prffit_kernel (PSF_T); SHORT_TILE: the tile the launcher
# takes where TILE cadences do not fit LDS_MAX_BYTES.  LDS_ATTR_BYTES: above it the launcher raises the kernel's dynamic-LDS
# attribute before the launch.  LDS_MAX_BYTES: a cutout whose SHORT_TILE cadences need more is refused (LK_EINVAL), nothing launched.
TILE, SHORT_TILE = 16, 8
LDS_ATTR_BYTES = 64 * 1024
LDS_MAX_BYTES = 160 * 1024
TAPS_BYTES = 192                                            # sizeof(PrfGradTaps): the taps and derivative weights of one pair
SHAPES = (((3, 3), 1), ((5, 7), 2), ((11, 11), 4), ((11, 11), 8), ((13, 17), 3))
N_MAIN = 33
N_VALUES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
N_SHORT = (SHORT_TILE - 1, SHORT_TILE, SHORT_TILE + 1)


def padded(n):
    """n rounded up to 4 x an odd number: the pitch rule of the PSF kernels."""
    return 4 * (((n + 3) // 4) | 1)


def lds_bytes(shape, S, use_flux_err=True, tile=TILE):
    """The dynamic LDS of one workgroup of ``tile`` cadences, the launcher's own count (cube_prffit_launch: lds_bytes): per
    cadence the S model images, the two derivative images, theta (S + 1), the shift (2), the taps and the tile of flux and
    flux_err; per workgroup the flag (8) and the mask."""
    npix = shape[0] * shape[1]
    per_cadence = 8 * (padded(S * npix) + padded(2 * npix) + S + 3) + TAPS_BYTES * S + 4 * padded(npix) * (2 if use_flux_err else 1)
    return tile * per_cadence + 8 + npix


def tile_of(shape, S, use_flux_err=True):
    """The tile the launcher takes for S stars: TILE when it fits, else SHORT_TILE."""
    return TILE if lds_bytes(shape, S, use_flux_err, TILE) <= LDS_MAX_BYTES else SHORT_TILE


def keys_derivative(x):
    """d/dx of Keys' cubic convolution kernel, a = -1/2, as the piecewise function of |x|."""
    a, sg = abs(x), (1.0 if x > 0 else -1.0 if x < 0 else 0.0)
    if a <= 1.0:
        return sg * (4.5 * a * a - 5.0 * a)
    if a < 2.0:
        return sg * (-1.5 * a * a + 5.0 * a - 4.0)
    return 0.0


def prf_gradient_image(samples, oversample, shape, c, r):
    """(dP/dc, dP/dr) of ``prf_image``: per pixel, the kernel's derivative over the zero-padded table at that pixel's own offset;
    u = (ix - c) os + (Tx - 1) / 2 falls by os per pixel of c."""
    PAD = 2
    Ty, Tx = samples.shape
    pad = np.zeros((Ty + 2 * PAD, Tx + 2 * PAD))
    pad[PAD:PAD + Ty, PAD:PAD + Tx] = samples
    ny, nx = shape
    gc, gr = np.zeros((ny, nx)), np.zeros((ny, nx))
    for iy in range(ny):
        for ix in range(nx):
            u = (ix - c) * oversample + (Tx - 1) / 2.0
            v = (iy - r) * oversample + (Ty - 1) / 2.0
            if not (abs(u) < 1e9 and abs(v) < 1e9):
                continue
            i0, j0 = int(np.floor(u)), int(np.floor(v))
            tc = tr = 0.0
            for j in range(j0 - 1, j0 + 3):
                if not -PAD <= j < Ty + PAD:
                    continue
                for i in range(i0 - 1, i0 + 3):
                    if -PAD <= i < Tx + PAD:
                        tc += pad[j + PAD, i + PAD] * keys(v - j) * keys_derivative(u - i)
                        tr += pad[j + PAD, i + PAD] * keys_derivative(v - j) * keys(u - i)
            gc[iy, ix], gr[iy, ix] = -oversample * tc, -oversample * tr
    return gc, gr


# Seeds other than 0, picked so that the preconditions of test_prffit_cpu.py hold with the mirror alone
SEEDS = {((5, 7), 2, 33, "os4"): 1, ((11, 11), 8, 33, "os4"): 1, ((13, 17), 3, 33, "os7"): 1}   # (with seed 0 a step lands within 0.1 % of tol)


@functools.lru_cache(maxsize=None)
def scene(shape, S, N, key=None):
    """-> dict: time (B, N); flux, err (B, N, ny, nx) float32; star_col, star_row (B, S) absolute, NaN = no star; prf_index (B,)
    int32; true_shifts = (shift_col, shift_row) (B, N); shifts0 = the truth moved by up to 0.1 px, one NaN in cutout 1; mask (B,
    ny, nx) bool; true_flux (B, S, N); true_bkg (B,); key; B.  Read-only."""
    key = key or TABLE_OF[(shape, S)]
    samples, os_ = table(key)
    ny, nx = shape
    B = 5 if S >= 2 else 3
    rng = np.random.default_rng([SEEDS.get((shape, S, N, key), 0), ny, nx, S, N, os_])
    time = np.tile(1000.0 + np.arange(N) * 0.02, (B, 1))
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    err = np.empty_like(flux)
    star_col, star_row = np.full((B, S), np.nan), np.full((B, S), np.nan)
    prf_index = (np.arange(B) % len(samples)).astype(np.int32)
    true_shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))
    shifts0 = tuple(a + rng.uniform(-0.1, 0.1, (B, N)) for a in true_shifts)
    mask = np.ones((B, ny, nx), dtype=bool)
    true_flux, true_bkg = np.full((B, S, N), np.nan), 20.0 + 5.0 * np.arange(B)
    for b in range(B):
        c, r = star_grid(shape, S, rng)
        if b == 2 and S >= 2:
            c[0] = r[0] = np.nan                            # the padding first: slots 1 .. S - 1 become the rows 0 .. S - 2
        if b == 3:
            c[1], r[1] = c[0], r[0]
        if b == 4:
            c[1] = nx + 30.3137                             # (not a whole number of samples from the table's centre at shift 0)
        star_col[b], star_row[b] = COLUMN + c, ROW + r
        amp = rng.uniform(2000.0, 8000.0, S)
        f = amp[:, None] * (1.0 + 0.01 * np.sin(2 * np.pi * (np.arange(N)[None, :] / 37.0 + rng.uniform(0, 1, S)[:, None])))
        true_flux[b] = np.where(np.isnan(c)[:, None], np.nan, f)
        img = np.full((N, ny, nx), true_bkg[b])
        for n in range(N):
            for s in range(S):
                if not np.isnan(c[s]) and c[s] < nx + 10:
                    img[n] += f[s, n] * prf_image(samples[prf_index[b]], os_, shape, c[s] + true_shifts[0][b, n], r[s] + true_shifts[1][b, n])
        e = np.sqrt(np.abs(img) + 4.0)
        flux[b] = (img + e * rng.standard_normal(img.shape)).astype(np.float32)
        err[b] = e.astype(np.float32)
    # cutout 1: everything that can go wrong with a value
    bad = rng.random((N, ny, nx)) < (0.05 if ny * nx > 9 else 0.0)
    flux[1][bad] = np.nan
    flat_f, flat_e = flux[1].reshape(N, -1), err[1].reshape(N, -1)
    flat_f[N // 4, ny * nx - 2] = np.nan
    if N >= 3:
        flux[1, N // 2] = np.nan
        time[1, 2] = np.nan
    flat_e[0, 0], flat_e[N - 1, (ny * nx) // 2], flat_e[N // 3, ny * nx - 1] = 0.0, np.nan, np.inf
    if N >= 4:
        shifts0[0][1, N - 1] = np.nan
    mask[1, 0, 0] = False
    if ny * nx > 9:
        mask[1, ny - 1, nx // 2] = False
    for a in (time, flux, err, star_col, star_row, prf_index, mask, true_flux, true_bkg) + true_shifts + shifts0:
        a.setflags(write=False)
    return dict(time=time, flux=flux, err=err, star_col=star_col, star_row=star_row, prf_index=prf_index, true_shifts=true_shifts,
                shifts0=shifts0, mask=mask, true_flux=true_flux, true_bkg=true_bkg, key=key, B=B)


def reference_fit(samples, oversample, flux, err, star_col, star_row, start, theta0):
    """One cutout without missing values, one table [Ty, Tx] -> shifts (N, 2) and theta (N, S + 1): scipy.optimize.least_squares
    over (theta, dc, dr) jointly, per cadence, on (y - model) / e with ``prf_image`` and scipy's 2-point Jacobian, its three
    tolerances at 1e-14, from ``start`` (N, 2) and ``theta0`` (N, S + 1)."""
    from scipy.optimize import least_squares
    N, ny, nx = flux.shape
    S = len(star_col)
    out_u, out_t = np.empty((N, 2)), np.empty((N, S + 1))
    for n in range(N):
        y, sw = flux[n].astype(np.float64), 1.0 / err[n].astype(np.float64)

        def residuals(x):
            m = np.full((ny, nx), x[S])
            for s in range(S):
                m = m + x[s] * prf_image(samples, oversample, (ny, nx), star_col[s] + x[S + 1] - COLUMN, star_row[s] + x[S + 2] - ROW)
            return ((y - m) * sw).ravel()

        res = least_squares(residuals, np.concatenate([theta0[n], start[n]]), xtol=1e-14, ftol=1e-14, gtol=1e-14,
                            x_scale=np.concatenate([np.maximum(np.abs(theta0[n]), 1.0), [0.1, 0.1]]))
        out_u[n], out_t[n] = res.x[S + 1:], res.x[:S + 1]
    return out_u, out_t


def cutout_arguments(sc, b, start, masked):
    """The keywords of PixelCube.psf_fit for cutout b of a scene."""
    return dict(star_col=sc["star_col"][b], star_row=sc["star_row"][b], prf=prf_object(sc["key"]), prf_index=int(sc["prf_index"][b]),
                shifts0=(sc["shifts0"][0][b], sc["shifts0"][1][b]) if start else None,
                aperture_mask=sc["mask"][b] if masked else "all", column=COLUMN, row=ROW)


@functools.lru_cache(maxsize=None)
def mirror(shape, S, N, setting="default", start=False, masked=True, use_flux_err=True, key=None):
    """PixelCube.psf_fit(prf=) of every cutout of the scene -> list of dicts; shared, read-only."""
    from lightkurve_amd.correctors import PixelCube
    sc = scene(shape, S, N, key)
    return [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_fit(use_flux_err=use_flux_err, **SETTINGS[setting],
                                                                          **cutout_arguments(sc, b, start, masked))
            for b in range(sc["B"])]


def parameters(setting):
    p = dict(DEFAULTS)
    p.update(SETTINGS[setting])
    return p


# The routes.  (3, 3) with 1 star and (5, 7) with 2 sit below LDS_ATTR_BYTES on the TILE; (11, 11) with 4 stars, 122 369 bytes, sits
# above it on the TILE; (11, 11) with 8 stars and (13, 17) with 3 do not fit LDS_MAX_BYTES on the TILE (197 633 and 181 733 bytes)
# and take the SHORT_TILE (98 881 and 90 981 bytes).  Beyond it: TOO_LARGE, (13, 17) with 8 stars, 169 637 bytes on the SHORT_TILE.
TOO_LARGE = ((13, 17), 8)

# what the tests compare: (shape, S, N, setting, start, masked, use_flux_err, key)
CASES = ([(shape, S, N_MAIN, "default", False, True, True, None) for shape, S in SHAPES]
         + [(shape, S, N_MAIN, "fixed", True, False, True, None) for shape, S in SHAPES]
         + [(shape, S, N, "default", st, True, True, None) for shape, S in SHAPES[:2] for N in N_VALUES for st in (False, True)]
         + [((11, 11), 8, N, "default", False, True, True, None) for N in N_SHORT]
         + [((11, 11), 4, N_MAIN, setting, False, True, True, None) for setting in ("short", "near", "clamped")]
         + [((5, 7), 2, N_MAIN, setting, False, True, True, None) for setting in ("fixed", "short", "near", "clamped")]
         + [((11, 11), 4, N_MAIN, "default", False, False, False, None), ((5, 7), 2, N_MAIN, "fixed", True, True, False, None)])
CASES = list(dict.fromkeys(CASES))
# the mission-sized table: os = 50, 551 x 551
OS50_CASE = ((11, 11), 4, 9, "default", False, True, True, "os50")


def case_id(c):
    return "%dx%d-S%d-N%d-%s%s%s%s%s" % (c[0] + c[1:4] + ("-start" if c[4] else "", "-masks" if c[5] else "", "" if c[6] else "-unweighted",
                                                            "-" + c[7] if c[7] else ""))
