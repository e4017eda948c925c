"""Seeded synthetic scenes for the PSF fit with a pointing shift per cadence (PixelCube.psf_fit, DevicePixelCubeBatch.psf_fit) and
an independent reference fit.

Unlike the scenes of psfphot_cases.py these are rendered WITH their true per-cadence shifts (uniform in +-0.3 px), by the
per-pixel PSF of psfphot_cases.psf_image, with photon-like noise e = sqrt(|img| + 4); the stars are at least 1.5 px apart and
all inside the cutout (psfphot_cases.star_grid), so no compared iteration is ill-posed.  The reference is
scipy.optimize.least_squares over (theta, dc, dr) jointly on the sqrt(w)-scaled residuals of that per-pixel PSF: no variable
projection, no tables, no Cholesky.

A scene is a batch of cutouts of one shape, each made to exercise its own inputs:
  0  clean: nothing missing, every cadence ok with the defaults;
  1  NaN pixels, one cadence that is NaN throughout, flux_err of 0, NaN and inf, a NaN time, a NaN entry in shifts0 and a
     per-cutout mask that removes pixels;
  2  one star fewer than the batch's widest (S >= 2): the NaN padding sits in slot 0;
  3  (S >= 2) stars 0 and 1 at the same position: singular at every cadence, so the cutout's status is 1.
"""
import functools

import numpy as np

from psfphot_cases import COLUMN, ROW, psf_image, star_grid

# The thresholds of psffit.hip.  TILE: cadences per workgroup of cube_psffit_kernel (PSF_T).  LDS_ATTR_BYTES: above it the
# launcher raises the kernel's dynamic-LDS attribute before the launch.  LDS_MAX_BYTES: above it the launcher refuses the call
# (LK_EINVAL) and launches nothing.
TILE = 16
LDS_ATTR_BYTES = 64 * 1024
LDS_MAX_BYTES = 160 * 1024
N_VALUES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 65)
SHAPES = (((3, 3), 1), ((5, 7), 2), ((11, 11), 4), ((11, 11), 8), ((13, 17), 3))
DEFAULTS = dict(max_iter=10, tol=1e-7, max_step=0.5, max_shift=2.0)
# the parameter settings that reach statuses 4 and 5 and the clamp on well-posed cutouts, and the fixed-count form
SETTINGS = {"default": {}, "fixed": dict(tol=0.0, max_iter=8), "short": dict(max_iter=2), "near": dict(max_shift=0.1),
            "clamped": dict(max_step=0.05)}


def lds_bytes(shape, S, use_flux_err=True):
    """The dynamic LDS of one workgroup, the launcher's own count (cube_psffit_launch: lds_bytes): the tile of psf_photometry
    and two tables (factors, derivatives) per cadence."""
    ny, nx = shape
    npix = ny * nx
    pitch = 4 * (((npix + 3) // 4) | 1)
    return 2 * S * (nx + ny) * 8 * TILE + TILE * pitch * 4 * (2 if use_flux_err else 1) + npix


# Seeds other than 0, picked so that the preconditions of test_psffit_cpu.py hold (with seed 0 one step of the (5, 7) scene
# under max_step = 0.05 lands within 0.1 % of tol)
SEEDS = {((5, 7), 2, 65): 1}


@functools.lru_cache(maxsize=None)
def scene(shape, S, N):
    """-> dict: time (B, N); flux, err (B, N, ny, nx) float32; star_col, star_row (B, S) absolute, NaN = no star; sigma (B, 2);
    true_shifts = (shift_col, shift_row) (B, N); shifts0 = the truth moved by up to 0.1 px, one NaN in cutout 1; mask (B, ny,
    nx) bool; true_flux (B, S, N); true_bkg (B,).  Read-only."""
    ny, nx = shape
    B = 4 if S >= 2 else 3
    rng = np.random.default_rng([SEEDS.get((shape, S, N), 0), ny, nx, S, N])
    time = np.tile(1000.0 + np.arange(N) * 0.02, (B, 1))
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    err = np.empty_like(flux)
    star_col, star_row = np.full((B, S), np.nan), np.full((B, S), np.nan)
    sigma = np.array([[1.1, 0.9], [1.3, 1.3], [0.8, 1.2], [1.0, 1.1]])[:B]
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
        star_col[b], star_row[b] = COLUMN + c, ROW + r
        amp = rng.uniform(2000.0, 8000.0, S)
        f = amp[:, None] * (1.0 + 0.01 * np.sin(2 * np.pi * (np.arange(N)[None, :] / 37.0 + rng.uniform(0, 1, S)[:, None])))
        true_flux[b] = np.where(np.isnan(c)[:, None], np.nan, f)
        img = np.full((N, ny, nx), true_bkg[b])
        for n in range(N):
            for s in range(S):
                if not np.isnan(c[s]):
                    img[n] += f[s, n] * psf_image(shape, c[s] + true_shifts[0][b, n], r[s] + true_shifts[1][b, n], *sigma[b])
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
    for a in (time, flux, err, star_col, star_row, sigma, mask, true_flux, true_bkg) + true_shifts + shifts0:
        a.setflags(write=False)
    return dict(time=time, flux=flux, err=err, star_col=star_col, star_row=star_row, sigma=sigma, true_shifts=true_shifts,
                shifts0=shifts0, mask=mask, true_flux=true_flux, true_bkg=true_bkg, B=B)


def reference_fit(flux, err, star_col, star_row, sigma, start, theta0):
    """One cutout without missing values -> shifts (N, 2) and theta (N, S + 1): scipy.optimize.least_squares over (theta, dc,
    dr) jointly, per cadence, on (y - model) / e with the per-pixel PSF, its three tolerances at 1e-14, from ``start`` (N, 2)
    and ``theta0`` (N, S + 1)."""
    from scipy.optimize import least_squares
    N, ny, nx = flux.shape
    S = len(star_col)
    out_u, out_t = np.empty((N, 2)), np.empty((N, S + 1))
    for n in range(N):
        y, sw = flux[n].astype(np.float64), 1.0 / err[n].astype(np.float64)

        def residuals(x):
            m = np.full((ny, nx), x[S])
            for s in range(S):
                m = m + x[s] * psf_image((ny, nx), star_col[s] + x[S + 1] - COLUMN, star_row[s] + x[S + 2] - ROW, *sigma)
            return ((y - m) * sw).ravel()

        res = least_squares(residuals, np.concatenate([theta0[n], start[n]]), xtol=1e-14, ftol=1e-14, gtol=1e-14,
                            x_scale=np.concatenate([np.maximum(np.abs(theta0[n]), 1.0), [0.1, 0.1]]))
        out_u[n], out_t[n] = res.x[S + 1:], res.x[:S + 1]
    return out_u, out_t


def cutout_arguments(sc, b, start, masked):
    """The keywords of PixelCube.psf_fit for cutout b of a scene."""
    return dict(star_col=sc["star_col"][b], star_row=sc["star_row"][b], sigma=tuple(sc["sigma"][b]),
                shifts0=(sc["shifts0"][0][b], sc["shifts0"][1][b]) if start else None,
                aperture_mask=sc["mask"][b] if masked else "all", column=COLUMN, row=ROW)


@functools.lru_cache(maxsize=None)
def mirror(shape, S, N, setting="default", start=False, masked=True, use_flux_err=True):
    """PixelCube.psf_fit of every cutout of the scene -> list of dicts; shared, read-only."""
    from lightkurve_amd.correctors import PixelCube
    sc = scene(shape, S, N)
    return [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_fit(use_flux_err=use_flux_err, **SETTINGS[setting],
                                                                          **cutout_arguments(sc, b, start, masked))
            for b in range(sc["B"])]


# On both sides of LDS_ATTR_BYTES: (19, 19) needs 56 681 bytes with one star and 66 409 with two; just under LDS_MAX_BYTES:
# (33, 33) with one star, 157 761 bytes; beyond it: TOO_LARGE, (33, 33) with two stars, 174 657 bytes (refused).
LDS_CASES = [((19, 19), 1, TILE + 1, "default", False, True, True), ((19, 19), 2, TILE + 1, "default", False, True, True),
             ((33, 33), 1, TILE + 1, "default", False, True, True)]
TOO_LARGE = ((33, 33), 2)

# what the tests compare: (shape, S, N, setting, start, masked, use_flux_err)
N_MAIN = 65
CASES = ([(shape, S, N_MAIN, "default", False, True, True) for shape, S in SHAPES]
         + [(shape, S, N_MAIN, "fixed", True, False, True) for shape, S in SHAPES]
         + [((5, 7), 2, N, "default", st, True, True) for N in N_VALUES for st in (False, True)]
         + [((11, 11), 4, N_MAIN, setting, False, True, True) for setting in ("short", "near", "clamped")]
         + [((5, 7), 2, N_MAIN, setting, False, True, True) for setting in ("fixed", "short", "near", "clamped")]
         + [((11, 11), 4, N_MAIN, "default", False, False, False), ((5, 7), 2, N_MAIN, "fixed", True, True, False)] + LDS_CASES)
CASES = list(dict.fromkeys(CASES))
