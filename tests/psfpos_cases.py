"""Seeded synthetic scenes for the fit of the stars' positions per cutout (PixelCube.psf_positions,
DevicePixelCubeBatch.psf_positions) and an independent joint reference fit.

Like the scenes of psfwidth_cases.py these are rendered with true per-cadence shifts (uniform in +-0.3 px, handed to the fit
exactly) by the per-pixel PSF of psfphot_cases.psf_image at the cutout's true width (TRUE_SIGMA, handed to the fit exactly),
with photon-like noise e = sqrt(|img| + 4).  They are rendered at the TRUE positions; the fit starts at ``star_col`` /
``star_row`` = the truth plus a per-star, per-axis offset of 0.1 .. 0.3 px of either sign.  The reference is
scipy.optimize.least_squares over every cadence's theta and the fitted positions at once: no variable projection, no tables, no
Cholesky.

A scene is a batch of cutouts of one shape, each made to exercise its own inputs:
  0  clean: nothing missing, every cadence contributes; offsets of 0.1 .. 0.2 px;
  1  NaN pixels, one cadence that is NaN throughout, flux_err of 0, NaN and inf, a NaN time, a NaN shift, a per-cutout pixel mask
     and a cadence_mask that drops every third cadence; its offsets are the batch's largest, 0.27 .. 0.3 px, so
     SETTINGS["bounded"] (max_offset = 0.24) stops it with status 5 on its way to the truth;
  2  one star fewer than the batch's widest (S >= 2): the NaN padding sits in slot 0; offsets of 0.1 .. 0.2 px;
  3  (S >= 2) stars 0 and 1 at the same position, at the truth and at the start: every cadence is singular at every evaluation,
     so the status is 1.
``subset`` cases fit the stars of the even slots alone (2 of 4 at S = 4); the others are handed over at their true positions.
"""
import functools

import numpy as np

from psfphot_cases import COLUMN, ROW, psf_image, star_grid
from psffit_cases import LDS_ATTR_BYTES, LDS_CASES as FIT_LDS_CASES, LDS_MAX_BYTES, TILE, TOO_LARGE  # noqa: F401
from psfwidth_cases import N_LONG, N_VALUES, SHAPES, STEP_LANES, TRUE_SIGMA, render  # noqa: F401

DEFAULTS = dict(max_iter=20, tol=1e-6, max_step=0.25, max_offset=1.0)
# the fixed-count form, and the settings that reach statuses 4 and 5 and the clamp on well-posed cutouts.  bounded: max_offset
# lies between the offsets of the cutouts 0 and 2 (at most 0.2 px, plus the noise of the fit) and those of cutout 1 (0.27 px at
# least)
SETTINGS = {"default": {}, "fixed": dict(tol=0.0, max_iter=6), "short": dict(max_iter=2), "bounded": dict(max_offset=0.24),
            "clamped": dict(max_step=0.02)}

# Seeds other than 0, picked so that the preconditions of test_psfpos_cpu.py hold: (shape, S, N, shifted) -> seed
SEEDS = {}


def lds_bytes(shape, S, use_flux_err=True):
    """The dynamic LDS of one workgroup, the launcher's own count (cube_psfpos_launch: lds_bytes): psf_fit's tile and two tables
    per cadence, and the parked L^-1 C, (S + 1) x 2 S doubles per cadence."""
    ny, nx = shape
    npix = ny * nx
    pitch = 4 * (((npix + 3) // 4) | 1)
    return 2 * S * (nx + ny) * 8 * TILE + (S + 1) * 2 * S * 8 * TILE + TILE * pitch * 4 * (2 if use_flux_err else 1) + npix


@functools.lru_cache(maxsize=None)
def scene(shape, S, N, shifted=True):
    """-> dict: time (B, N); flux, err (B, N, ny, nx) float32; true_col, true_row (B, S) absolute, NaN = no star; star_col,
    star_row (B, S), the start: the truth plus the offsets; sigma (B, 2), the truth; shifts = (shift_col, shift_row) (B, N), the
    truth with one NaN in cutout 1, or None when the scene is rendered without shifts; mask (B, ny, nx) bool; cadence_mask (B,
    N) bool; true_flux (B, S, N); true_bkg (B,).  Read-only."""
    ny, nx = shape
    B = 4 if S >= 2 else 3
    rng = np.random.default_rng([SEEDS.get((shape, S, N, shifted), 0), ny, nx, S, N, int(shifted), 9])
    time = np.tile(1000.0 + np.arange(N) * 0.02, (B, 1))
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    err = np.empty_like(flux)
    true_col, true_row = np.full((B, S), np.nan), np.full((B, S), np.nan)
    sigma = TRUE_SIGMA[:B].copy()
    true_shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N))) if shifted else (np.zeros((B, N)), np.zeros((B, N)))
    mask = np.ones((B, ny, nx), dtype=bool)
    cadence_mask = np.ones((B, N), dtype=bool)
    true_flux, true_bkg = np.full((B, S, N), np.nan), 20.0 + 5.0 * np.arange(B)
    for b in range(B):
        c, r = star_grid(shape, S, rng)
        if b == 2 and S >= 2:
            c[0] = r[0] = np.nan                            # the padding first: slots 1 .. S - 1 are the stars 0 .. S - 2
        if b == 3:
            c[1], r[1] = c[0], r[0]
        true_col[b], true_row[b] = COLUMN + c, ROW + r
        flux[b], err[b], true_flux[b] = render(rng, shape, c, r, sigma[b], N, (true_shifts[0][b], true_shifts[1][b]), true_bkg[b])
    size = np.where(np.arange(B)[:, None, None] == 1, rng.uniform(0.27, 0.3, (B, S, 2)), rng.uniform(0.1, 0.2, (B, S, 2)))
    offset = size * rng.choice([-1.0, 1.0], (B, S, 2))
    if B > 3:
        offset[3, 1] = offset[3, 0]                         # the two stars at one position start at one position
    star_col, star_row = true_col + offset[:, :, 0], true_row + offset[:, :, 1]
    shifts = tuple(a.copy() for a in true_shifts) if shifted else None
    # cutout 1: everything that can go wrong with a value
    bad = rng.random((N, ny, nx)) < (0.05 if ny * nx > 9 else 0.0)
    flux[1][bad] = np.nan
    flat_f, flat_e = flux[1].reshape(N, -1), err[1].reshape(N, -1)
    flat_f[N // 4, ny * nx - 2] = np.nan
    if N >= 3:
        flux[1, N // 2] = np.nan
        time[1, 2] = np.nan
    flat_e[0, 0], flat_e[N - 1, (ny * nx) // 2], flat_e[N // 3, ny * nx - 1] = 0.0, np.nan, np.inf
    if N >= 4 and shifted:
        shifts[0][1, N - 1] = np.nan
    mask[1, 0, 0] = False
    if ny * nx > 9:
        mask[1, ny - 1, nx // 2] = False
    cadence_mask[1, 1::3] = False
    fit_subset = np.zeros((B, S), dtype=bool)
    fit_subset[:, 0::2] = True
    if S >= 2:
        fit_subset[2] = ~fit_subset[2]                      # cutout 2 has no star in slot 0: its odd slots instead
    for a in (time, flux, err, true_col, true_row, star_col, star_row, sigma, mask, cadence_mask, true_flux, true_bkg, fit_subset) \
            + true_shifts + (shifts or ()):
        a.setflags(write=False)
    return dict(time=time, flux=flux, err=err, true_col=true_col, true_row=true_row, star_col=star_col, star_row=star_row, sigma=sigma,
                shifts=shifts, true_shifts=true_shifts, mask=mask, cadence_mask=cadence_mask, true_flux=true_flux, true_bkg=true_bkg,
                fit_subset=fit_subset, B=B)


def start(sc, subset):
    """-> star_col, star_row (B, S) handed to the fit and fit_star (B, S) or None: with ``subset`` the stars that are not fitted
    sit at their true positions — but star 1 of cutout 3, which stays on star 0's start so that the cutout stays singular."""
    if not subset:
        return sc["star_col"], sc["star_row"], None
    fit = sc["fit_subset"]
    col, row = np.where(fit, sc["star_col"], sc["true_col"]), np.where(fit, sc["star_row"], sc["true_row"])
    if sc["B"] > 3:
        col[3, 1], row[3, 1] = sc["star_col"][3, 1], sc["star_row"][3, 1]
    return col, row, fit


@functools.lru_cache(maxsize=None)
def clean_cutout(seed, shape=(11, 11), S=4, N=33):
    """One clean cutout for the pulls, sigma as cutout ``seed % 4`` of a scene, starts 0.1 .. 0.3 px off -> the keywords of
    PixelCube and of psf_positions, and the truth."""
    rng = np.random.default_rng([seed, 78])
    sigma = TRUE_SIGMA[seed % 4]
    shifts = (rng.uniform(-0.3, 0.3, N), rng.uniform(-0.3, 0.3, N))
    c, r = star_grid(shape, S, rng)
    flux, err, _ = render(rng, shape, c, r, sigma, N, shifts, 20.0)
    off = rng.uniform(0.1, 0.3, (S, 2)) * rng.choice([-1.0, 1.0], (S, 2))
    return dict(time=1000.0 + np.arange(N) * 0.02, flux=flux, err=err, true_col=COLUMN + c, true_row=ROW + r,
                kw=dict(star_col=COLUMN + c + off[:, 0], star_row=ROW + r + off[:, 1], sigma=tuple(sigma), shifts=shifts, column=COLUMN,
                        row=ROW))


def reference_fit(flux, err, star_col, star_row, sigma, shifts, fit, theta0):
    """One cutout without missing values or empty slots -> (star_col, star_row (S,), theta (N, S + 1)): scipy.optimize.least_squares
    over every cadence's theta and the (column, row) of the stars with ``fit`` (S,) bool jointly, on (y - model) / e with the
    per-pixel PSF, its three tolerances at 1e-14; the stars that are not fitted stay frozen at ``star_col`` / ``star_row``."""
    from scipy.optimize import least_squares
    N, ny, nx = flux.shape
    S = len(star_col)
    y, sw = flux.astype(np.float64), 1.0 / err.astype(np.float64)
    fit = np.asarray(fit, dtype=bool)
    nfit = int(fit.sum())

    def positions(x):
        col, row = np.array(star_col, dtype=np.float64), np.array(star_row, dtype=np.float64)
        col[fit], row[fit] = x[-2 * nfit::2], x[-2 * nfit + 1::2]
        return col, row

    def residuals(x):
        theta = x[:-2 * nfit].reshape(N, S + 1)
        col, row = positions(x)
        out = np.empty((N, ny, nx))
        for n in range(N):
            m = np.full((ny, nx), theta[n, S])
            for s in range(S):
                m = m + theta[n, s] * psf_image((ny, nx), col[s] + shifts[0][n] - COLUMN, row[s] + shifts[1][n] - ROW, *sigma)
            out[n] = (y[n] - m) * sw[n]
        return out.ravel()

    v0 = np.stack([np.asarray(star_col)[fit], np.asarray(star_row)[fit]], axis=1).ravel()
    res = least_squares(residuals, np.concatenate([theta0.ravel(), v0]), xtol=1e-14, ftol=1e-14, gtol=1e-14,
                        x_scale=np.concatenate([np.maximum(np.abs(theta0.ravel()), 1.0), np.full(2 * nfit, 0.1)]))
    col, row = positions(res.x)
    return col, row, res.x[:-2 * nfit].reshape(N, S + 1)


def cutout_arguments(sc, b, masked, subset=False):
    """The keywords of PixelCube.psf_positions for cutout b of a scene."""
    col, row, fit = start(sc, subset)
    return dict(star_col=col[b], star_row=row[b], sigma=tuple(sc["sigma"][b]), fit_star=None if fit is None else fit[b],
                shifts=(sc["shifts"][0][b], sc["shifts"][1][b]) if sc["shifts"] is not None else None,
                cadence_mask=sc["cadence_mask"][b] if masked else None,
                aperture_mask=sc["mask"][b] if masked else "all", column=COLUMN, row=ROW)


@functools.lru_cache(maxsize=None)
def mirror(shape, S, N, setting="default", shifted=True, masked=True, use_flux_err=True, subset=False):
    """PixelCube.psf_positions of every cutout of the scene -> list of dicts; shared, read-only."""
    from lightkurve_amd.correctors import PixelCube
    sc = scene(shape, S, N, shifted)
    return [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_positions(use_flux_err=use_flux_err, **SETTINGS[setting],
                                                                                **cutout_arguments(sc, b, masked, subset))
            for b in range(sc["B"])]


# psf_fit's LDS cases, which the new count (+ 512 bytes with one star, + 1536 with two) still admits on the same sides of the
# two thresholds: (19, 19) with one star below LDS_ATTR_BYTES and with two above it, (33, 33) with one star just under
# LDS_MAX_BYTES; TOO_LARGE, (33, 33) with two stars, is refused
LDS_CASES = [(c[0], c[1], c[2], "default", True, True, True, False) for c in FIT_LDS_CASES]

# what the tests compare: (shape, S, N, setting, shifted, masked, use_flux_err, subset).  (11, 11) with 8 stars is compared with all
# its 16 positions free: the iteration contracts there at seed 0 (test_psfpos_cpu.py asserts it)
N_MAIN = 65
CASES = ([(shape, S, N_MAIN, "default", True, True, True, False) for shape, S in SHAPES]
         + [(shape, S, N_MAIN, "fixed", True, False, True, False) for shape, S in SHAPES]
         + [((5, 7), 2, N, "default", True, True, True, False) for N in N_VALUES + N_LONG]
         + [((11, 11), 4, N_MAIN, setting, True, True, True, False) for setting in ("short", "bounded", "clamped")]
         + [((5, 7), 2, N_MAIN, setting, True, True, True, False) for setting in ("fixed", "short", "bounded", "clamped")]
         + [((11, 11), 4, N_MAIN, "default", True, True, True, True), ((11, 11), 4, N_MAIN, "fixed", True, False, True, True),
            ((5, 7), 2, N_MAIN, "default", True, True, True, True)]
         + [((11, 11), 4, N_MAIN, "default", True, False, False, False), ((11, 11), 4, N_MAIN, "default", False, True, True, False),
            ((5, 7), 2, N_MAIN, "fixed", False, False, False, False)] + LDS_CASES)
CASES = list(dict.fromkeys(CASES))
