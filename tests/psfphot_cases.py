"""Seeded synthetic scenes for PSF photometry (PixelCube.psf_photometry, DevicePixelCubeBatch.psf_photometry) and an independent
reference fit.

The scenes are rendered with a PSF of their own: scipy.special.erf on the pixel edges written out per pixel, not the separable
tables of the mirror or the kernel.  The reference fit is np.linalg.lstsq on sqrt(w) A per cadence, the background column
included — no normal equations, no Cholesky.

A scene is a batch of cutouts of one shape, each made to exercise its own inputs:
  0  every star inside, photon-like noise, nothing missing;
  1  NaN pixels, one cadence that is NaN throughout, flux_err of 0, NaN and inf, a NaN time, (with shifts) a NaN shift, and a
     per-cutout mask that removes pixels;
  2  one star fewer than the batch's widest (S >= 2): the NaN padding sits in slot 0, so the cutout's stars are NOT the first
     slots and STAR_INDEX differs from the output row; its first star (slot 1; slot 0 for S = 1) is centred 0.9 px OUTSIDE the
     cutout's left edge;
  3  (S >= 2) stars 0 and 1 at the same position: singular at every cadence, so the cutout's status is 1.
"""
import functools

import numpy as np
from scipy.special import erf

# The thresholds of psfphot.hip.  TILE: cadences per workgroup of cube_psfphot_kernel (PSF_T).  LDS_ATTR_BYTES: above it the
# launcher raises the kernel's dynamic-LDS attribute before the launch (psf_launch: want_lds), another launch path, cut by shape,
# star count and shifts.  LDS_MAX_BYTES: above it the launcher refuses the call (LK_EINVAL) and launches nothing.
TILE = 16
LDS_ATTR_BYTES = 64 * 1024
LDS_MAX_BYTES = 160 * 1024
N_VALUES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 63, 64, 65, 130)
SHAPES = (((3, 3), 1), ((5, 7), 2), ((11, 11), 4), ((11, 11), 8), ((13, 17), 3))
COLUMN, ROW = 100.0, 200.0                                  # the cutouts' corner: positions are absolute


def lds_bytes(shape, S, shifts, use_flux_err=True):
    """The dynamic LDS of one workgroup, the launcher's own count (cube_psfphot_launch: lds_bytes)."""
    ny, nx = shape
    npix = ny * nx
    pitch = 4 * (((npix + 3) // 4) | 1)
    return S * (nx + ny) * 8 * (TILE if shifts else 1) + TILE * pitch * 4 * (2 if use_flux_err else 1) + npix


def psf_image(shape, c, r, sig_c, sig_r):
    """The pixel-integrated Gaussian centred on local (c, r), pixel (iy, ix) covering [ix - 1/2, ix + 1/2] x [iy - 1/2, iy + 1/2]."""
    ny, nx = shape
    iy, ix = np.mgrid[0:ny, 0:nx].astype(np.float64)
    gx = erf((ix + 0.5 - c) / (np.sqrt(2.0) * sig_c)) - erf((ix - 0.5 - c) / (np.sqrt(2.0) * sig_c))
    gy = erf((iy + 0.5 - r) / (np.sqrt(2.0) * sig_r)) - erf((iy - 0.5 - r) / (np.sqrt(2.0) * sig_r))
    return 0.25 * gx * gy


def star_grid(shape, S, rng):
    """S local positions at least ~1.5 px apart: a jittered lattice inside the cutout."""
    ny, nx = shape
    ncol = int(np.ceil(np.sqrt(S * nx / ny)))
    nrow = int(np.ceil(S / ncol))
    cells = [(i, j) for j in range(nrow) for i in range(ncol)][:S]
    col = np.array([(i + 0.5) * nx / ncol - 0.5 for i, _ in cells]) + rng.uniform(-0.2, 0.2, S)
    row = np.array([(j + 0.5) * ny / nrow - 0.5 for _, j in cells]) + rng.uniform(-0.2, 0.2, S)
    return col, row


@functools.lru_cache(maxsize=None)
def scene(shape, S, N, seed=0):
    """-> dict: time (B, N); flux, err (B, N, ny, nx) float32; star_col, star_row (B, S) absolute, NaN = no star; sigma (B, 2);
    shifts = (shift_col, shift_row) (B, N); mask (B, ny, nx) bool; true_flux (B, S, N); true_bkg (B,).  Read-only."""
    ny, nx = shape
    B = 4 if S >= 2 else 3
    rng = np.random.default_rng([seed, ny, nx, S, N])
    time = np.tile(1000.0 + np.arange(N) * 0.02, (B, 1))
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    err = np.empty_like(flux)
    star_col, star_row = np.full((B, S), np.nan), np.full((B, S), np.nan)
    sigma = np.array([[1.1, 0.9], [1.3, 1.3], [0.8, 1.2], [1.0, 1.1]])[:B]
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))
    mask = np.ones((B, ny, nx), dtype=bool)
    true_flux, true_bkg = np.full((B, S, N), np.nan), 20.0 + 5.0 * np.arange(B)
    for b in range(B):
        c, r = star_grid(shape, S, rng)
        if b == 2:
            if S >= 2:
                c[0] = r[0] = np.nan                        # the padding first: slots 1 .. S - 1 become the rows 0 .. S - 2
            c[1 if S >= 2 else 0] = -1.4                    # 0.9 px outside the left edge (which is at -0.5)
        if b == 3:
            c[1], r[1] = c[0], r[0]
        star_col[b], star_row[b] = COLUMN + c, ROW + r
        amp = rng.uniform(500.0, 5000.0, S)
        f = amp[:, None] * (1.0 + 0.01 * np.sin(2 * np.pi * (np.arange(N)[None, :] / 37.0 + rng.uniform(0, 1, S)[:, None])))
        true_flux[b] = np.where(np.isnan(c)[:, None], np.nan, f)
        img = np.full((N, ny, nx), true_bkg[b])
        for s in range(S):
            if not np.isnan(c[s]):
                img += f[s][:, None, None] * psf_image(shape, c[s], r[s], *sigma[b])[None]
        e = np.sqrt(np.abs(img) + 4.0)
        flux[b] = (img + e * rng.standard_normal(img.shape)).astype(np.float32)
        err[b] = e.astype(np.float32)
    # cutout 1: everything that can go wrong with a value
    bad = rng.random((N, ny, nx)) < 0.05
    flux[1][bad] = np.nan
    if N >= 3:
        flux[1, N // 2] = np.nan
        time[1, 2] = np.nan
    flat = err[1].reshape(N, -1)
    flat[0, 0], flat[N - 1, (ny * nx) // 2], flat[N // 3, ny * nx - 1] = 0.0, np.nan, np.inf
    if N >= 4:
        shifts[0][1, N - 1] = np.nan
        shifts[1][1, 1] = np.nan
    mask[1, 0, 0] = mask[1, ny - 1, nx // 2] = False
    for a in (time, flux, err, star_col, star_row, sigma, mask, true_flux, true_bkg) + shifts:
        a.setflags(write=False)
    return dict(time=time, flux=flux, err=err, star_col=star_col, star_row=star_row, sigma=sigma, shifts=shifts, mask=mask,
                true_flux=true_flux, true_bkg=true_bkg, B=B)


def reference_fit(time, flux, err, star_col, star_row, sigma, shifts=None, mask=None, use_flux_err=True):
    """One cutout, stars without NaN padding -> flux (S, N), flux_err (S, N), background (N,), chi2 (N,), n_used (N,): lstsq on
    sqrt(w) A with the independent PSF; NaN for a cadence with a non-finite time or shift or fewer than S + 2 used pixels.
    Rank-deficient cadences are NOT detected here (the tests compare them by status)."""
    N, ny, nx = flux.shape
    S = len(star_col)
    out_f, out_e = np.full((S, N), np.nan), np.full((S, N), np.nan)
    out_b, out_c, out_n = np.full(N, np.nan), np.full(N, np.nan), np.zeros(N, dtype=np.int32)
    m = np.ones((ny, nx), dtype=bool) if mask is None else mask
    for n in range(N):
        dc, dr = (0.0, 0.0) if shifts is None else (shifts[0][n], shifts[1][n])
        used = m & np.isfinite(flux[n])
        if use_flux_err:
            used &= np.isfinite(err[n]) & (err[n] > 0)
        out_n[n] = used.sum()
        if not (np.isfinite(time[n]) and np.isfinite(dc) and np.isfinite(dr)) or out_n[n] < S + 2:
            continue
        A = np.stack([psf_image((ny, nx), star_col[s] + dc - COLUMN, star_row[s] + dr - ROW, *sigma)[used] for s in range(S)]
                     + [np.ones(out_n[n])], axis=1)
        y = flux[n][used].astype(np.float64)
        sw = 1.0 / err[n][used].astype(np.float64) if use_flux_err else np.ones(out_n[n])
        theta = np.linalg.lstsq(A * sw[:, None], y * sw, rcond=None)[0]
        out_f[:, n], out_b[n] = theta[:S], theta[S]
        out_c[n] = np.sum((sw * (y - A.dot(theta))) ** 2)
        try:
            with np.errstate(invalid="ignore"):
                out_e[:, n] = np.sqrt(np.diag(np.linalg.inv((A * sw[:, None]).T.dot(A * sw[:, None]))))[:S]
        except np.linalg.LinAlgError:
            pass                                            # (a rank-deficient cadence: not compared)
    return out_f, out_e, out_b, out_c, out_n


def cutout_arguments(sc, b, shifts, masked):
    """The keywords of PixelCube.psf_photometry for cutout b of a scene."""
    return dict(star_col=sc["star_col"][b], star_row=sc["star_row"][b], sigma=tuple(sc["sigma"][b]),
                shifts=(sc["shifts"][0][b], sc["shifts"][1][b]) if shifts else None,
                aperture_mask=sc["mask"][b] if masked else "all", column=COLUMN, row=ROW)


@functools.lru_cache(maxsize=None)
def mirror(shape, S, N, shifts=False, masked=True, use_flux_err=True):
    """PixelCube.psf_photometry of every cutout of the scene -> list of dicts; shared, read-only."""
    from lightkurve_amd.correctors import PixelCube
    sc = scene(shape, S, N)
    return [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_photometry(use_flux_err=use_flux_err,
                                                                                **cutout_arguments(sc, b, shifts, masked))
            for b in range(sc["B"])]


# On both sides of LDS_ATTR_BYTES: (21, 21) with 4 stars needs 58 617 bytes without shifts and 78 777 with them; just under
# LDS_MAX_BYTES: (35, 35) with one star, 158 969 bytes; beyond it: TOO_LARGE, 168 272 bytes (test_psfphot_gpu.py: refused).
LDS_CASES = [((21, 21), 4, TILE + 1, False, True, True), ((21, 21), 4, TILE + 1, True, True, True), ((35, 35), 1, TILE + 1, False, True, True)]
TOO_LARGE = ((36, 36), 1)

# what the GPU file compares: (shape, S, N, shifts, masked, use_flux_err)
GPU_CASES = ([(shape, S, 130, False, True, True) for shape, S in SHAPES] + [(shape, S, 130, True, False, True) for shape, S in SHAPES]
             + [((5, 7), 2, N, sh, True, True) for N in N_VALUES for sh in (False, True)]
             + [((11, 11), 4, 130, False, False, False), ((5, 7), 2, 65, True, True, False)] + LDS_CASES)
GPU_CASES = list(dict.fromkeys(GPU_CASES))
