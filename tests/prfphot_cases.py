"""Seeded synthetic scenes for PSF photometry with a tabulated PRF (PixelCube.psf_photometry(prf=),
DevicePixelCubeBatch.psf_photometry(prf=)), in the manner of psfphot_cases.py, and an independent evaluation of the model.

The independent evaluation (``prf_image``) writes Keys' kernel as the piecewise function of |x| — 1.5 |x|^3 - 2.5 |x|^2 + 1 up to
1, -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2 up to 2 — and applies it per pixel, in a plain loop, to an explicitly zero-padded table at
the pixel's own offset (dx, dy); it shares neither the polynomial weights in f nor the shared fractional parts with the mirror
or the kernel.  The reference fit is np.linalg.lstsq on sqrt(w) A per cadence.  The scenes are rendered with ``prf_image`` at the
stars' catalogue positions (no shift), with photon-like noise.

Tables (``table(key)`` -> samples [2, Ty, Tx] float32 and the oversampling): smooth, positive, with a small seeded x y term so
that they are not separable; the second table of each key differs from the first, and ``prf_index`` of cutout b is b % 2.
  "os1"   os = 1, 5 x 5
  "os4"   os = 4, 33 x 41
  "os7"   os = 7, 50 x 57: Ty is even, so in y the star's centre lies between two samples
  "os50"  os = 50, 551 x 551 from TabulatedPRF.from_gaussian (one table; used by the from_gaussian test and one GPU test)

A scene is a batch of cutouts of one shape:
  0  every star inside, nothing missing;
  1  NaN pixels, one cadence that is NaN throughout, flux_err of 0, NaN and inf, a NaN time, (with shifts) a NaN shift, and a
     per-cutout mask that removes pixels;
  2  NaN-padded star slots (S >= 2: the padding sits in slot 0), and its first star centred 0.9 px OUTSIDE the cutout's left edge:
     the table's support overlaps the cutout only in part, so taps run off the table and off the cutout;
  3  (S >= 2) stars 0 and 1 at the same position: singular at every cadence, so the cutout's status is 1;
  4  (S >= 2) star 1 is 30 px from the cutout, farther than any table reaches: its model is zero on every pixel, status 3 at every
     cadence through the pivot cut, and the cutout's status is 1.
"""
import functools

import numpy as np

from psfphot_cases import COLUMN, ROW, star_grid

# The thresholds of prfphot.hip.  TILE: cadences per workgroup of cube_prfphot_kernel (PSF_T).  LDS_ATTR_BYTES: above it the
# launcher raises the kernel's dynamic-LDS attribute before the launch (prf_launch: want_lds).  LDS_MAX_BYTES: above it the
# launcher refuses the call (LK_EINVAL) and launches nothing.
TILE = 16
LDS_ATTR_BYTES = 64 * 1024
LDS_MAX_BYTES = 160 * 1024
TAPS_BYTES = 128                                            # sizeof(PrfTaps): the taps of one (cadence, star) pair
N_VALUES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 64, 65, 130)
SHAPES = (((3, 3), 1), ((5, 7), 2), ((11, 11), 4), ((11, 11), 8), ((13, 17), 3))
TABLE_OF = {((3, 3), 1): "os1", ((5, 7), 2): "os4", ((11, 11), 4): "os7", ((11, 11), 8): "os4", ((13, 17), 3): "os7"}


def lds_bytes(shape, S, shifts, use_flux_err=True):
    """The dynamic LDS of one workgroup, the launcher's own count (cube_prfphot_launch: lds_bytes)."""
    ny, nx = shape
    npix = ny * nx
    pitch = 4 * (((npix + 3) // 4) | 1)
    tile = TILE * pitch * 4 * (2 if use_flux_err else 1) + npix
    if not shifts:
        return S * npix * 8 + tile
    mpitch = 4 * (((S * npix + 3) // 4) | 1)
    return TILE * mpitch * 8 + TILE * S * TAPS_BYTES + tile


@functools.lru_cache(maxsize=None)
def table(key):
    """-> (samples [n_prf, Ty, Tx] float32, read-only; oversample)."""
    if key == "os50":
        from lightkurve_amd.correctors import TabulatedPRF
        prf = TabulatedPRF.from_gaussian(1.1, 0.9, 50, 5.5)
        assert prf.samples.shape == (1, 551, 551)
        return prf.samples, 50
    os_, Ty, Tx, sx, sy = {"os1": (1, 5, 5, 0.8, 0.9), "os4": (4, 33, 41, 1.2, 1.0), "os7": (7, 50, 57, 1.0, 0.9)}[key]
    rng = np.random.default_rng([77, os_, Ty, Tx])
    x = (np.arange(Tx) - (Tx - 1) / 2.0)[None, :] / os_
    y = (np.arange(Ty) - (Ty - 1) / 2.0)[:, None] / os_
    out = np.empty((2, Ty, Tx), dtype=np.float32)
    for k in range(2):
        a, b = rng.uniform(0.1, 0.3) * (1 if k == 0 else -1), rng.uniform(-0.1, 0.1)
        wide = 1.0 + 0.15 * k
        g = np.exp(-0.5 * ((x / (sx * wide)) ** 2 + (y / (sy * wide)) ** 2)) / (2 * np.pi * sx * sy * wide * wide)
        out[k] = g * (1.0 + a * x * y / (1.0 + x * x + y * y) + b * x / np.sqrt(1.0 + x * x))
    assert np.all(out > 0)
    out.setflags(write=False)
    return out, os_


def prf_object(key):
    from lightkurve_amd.correctors import TabulatedPRF
    return TabulatedPRF(*table(key))


def keys(x):
    """Keys' cubic convolution kernel, a = -1/2, as the piecewise function of |x|."""
    x = abs(x)
    if x <= 1.0:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x < 2.0:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def prf_image(samples, oversample, shape, c, r):
    """The model image of a star centred on local (c, r) from ONE table [Ty, Tx]: per pixel, the kernel over the zero-padded
    table at that pixel's own offset."""
    PAD = 2
    Ty, Tx = samples.shape
    pad = np.zeros((Ty + 2 * PAD, Tx + 2 * PAD))
    pad[PAD:PAD + Ty, PAD:PAD + Tx] = samples
    ny, nx = shape
    img = np.zeros((ny, nx))
    for iy in range(ny):
        for ix in range(nx):
            u = (ix - c) * oversample + (Tx - 1) / 2.0
            v = (iy - r) * oversample + (Ty - 1) / 2.0
            if not (abs(u) < 1e9 and abs(v) < 1e9):
                continue                                    # (no tap on the table; NaN: the cadence is not fitted)
            i0, j0 = int(np.floor(u)), int(np.floor(v))
            total = 0.0
            for j in range(j0 - 1, j0 + 3):
                if not -PAD <= j < Ty + PAD:
                    continue                                # beyond the padding: zero
                ky = keys(v - j)
                for i in range(i0 - 1, i0 + 3):
                    if -PAD <= i < Tx + PAD:
                        total += pad[j + PAD, i + PAD] * ky * keys(u - i)
            img[iy, ix] = total
    return img


@functools.lru_cache(maxsize=None)
def scene(shape, S, N, key=None, seed=0):
    """-> dict: time (B, N); flux, err (B, N, ny, nx) float32; star_col, star_row (B, S) absolute, NaN = no star; prf_index (B,)
    int32; shifts = (shift_col, shift_row) (B, N); mask (B, ny, nx) bool; key; B.  Read-only."""
    key = key or TABLE_OF.get((shape, S), "os4")
    samples, os_ = table(key)
    ny, nx = shape
    B = 5 if S >= 2 else 3
    rng = np.random.default_rng([seed, ny, nx, S, N, os_])
    time = np.tile(1000.0 + np.arange(N) * 0.02, (B, 1))
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    err = np.empty_like(flux)
    star_col, star_row = np.full((B, S), np.nan), np.full((B, S), np.nan)
    prf_index = (np.arange(B) % len(samples)).astype(np.int32)
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))
    mask = np.ones((B, ny, nx), dtype=bool)
    for b in range(B):
        c, r = star_grid(shape, S, rng)
        if b == 2:
            if S >= 2:
                c[0] = r[0] = np.nan
            c[1 if S >= 2 else 0] = -1.4
        if b == 3:
            c[1], r[1] = c[0], r[0]
        if b == 4:
            c[1] = nx + 30.0
        star_col[b], star_row[b] = COLUMN + c, ROW + r
        amp = rng.uniform(500.0, 5000.0, S)
        f = amp[:, None] * (1.0 + 0.01 * np.sin(2 * np.pi * (np.arange(N)[None, :] / 37.0 + rng.uniform(0, 1, S)[:, None])))
        img = np.full((N, ny, nx), 20.0 + 5.0 * b)
        for s in range(S):
            if not np.isnan(c[s]):
                img += f[s][:, None, None] * prf_image(samples[prf_index[b]], os_, shape, c[s], r[s])[None]
        e = np.sqrt(np.abs(img) + 4.0)
        flux[b] = (img + e * rng.standard_normal(img.shape)).astype(np.float32)
        err[b] = e.astype(np.float32)
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
    for a in (time, flux, err, star_col, star_row, prf_index, mask) + shifts:
        a.setflags(write=False)
    return dict(time=time, flux=flux, err=err, star_col=star_col, star_row=star_row, prf_index=prf_index, shifts=shifts, mask=mask,
                key=key, B=B)


def reference_fit(samples, oversample, time, flux, err, star_col, star_row, shifts=None, mask=None, use_flux_err=True):
    """One cutout, one table [Ty, Tx], stars without NaN padding -> flux (S, N), flux_err (S, N), background (N,), chi2 (N,),
    n_used (N,): lstsq on sqrt(w) A with ``prf_image``; NaN for a cadence with a non-finite time or shift or fewer than S + 2
    used pixels.  Rank-deficient cadences are NOT detected here (the tests compare them by status)."""
    N, ny, nx = flux.shape
    S = len(star_col)
    out_f, out_e = np.full((S, N), np.nan), np.full((S, N), np.nan)
    out_b, out_c, out_n = np.full(N, np.nan), np.full(N, np.nan), np.zeros(N, dtype=np.int32)
    m = np.ones((ny, nx), dtype=bool) if mask is None else mask
    still = None if shifts is not None else [prf_image(samples, oversample, (ny, nx), star_col[s] - COLUMN, star_row[s] - ROW)
                                              for s in range(S)]
    for n in range(N):
        dc, dr = (0.0, 0.0) if shifts is None else (shifts[0][n], shifts[1][n])
        used = m & np.isfinite(flux[n])
        if use_flux_err:
            used &= np.isfinite(err[n]) & (err[n] > 0)
        out_n[n] = used.sum()
        if not (np.isfinite(time[n]) and np.isfinite(dc) and np.isfinite(dr)) or out_n[n] < S + 2:
            continue
        images = still or [prf_image(samples, oversample, (ny, nx), star_col[s] + dc - COLUMN, star_row[s] + dr - ROW) for s in range(S)]
        A = np.stack([im[used] for im in images] + [np.ones(out_n[n])], axis=1)
        y = flux[n][used].astype(np.float64)
        sw = 1.0 / err[n][used].astype(np.float64) if use_flux_err else np.ones(out_n[n])
        theta = np.linalg.lstsq(A * sw[:, None], y * sw, rcond=None)[0]
        out_f[:, n], out_b[n] = theta[:S], theta[S]
        out_c[n] = np.sum((sw * (y - A.dot(theta))) ** 2)
        try:
            with np.errstate(all="ignore"):
                out_e[:, n] = np.sqrt(np.diag(np.linalg.inv((A * sw[:, None]).T.dot(A * sw[:, None]))))[:S]
        except np.linalg.LinAlgError:
            pass                                            # (a rank-deficient cadence: not compared)
    return out_f, out_e, out_b, out_c, out_n


def cutout_arguments(sc, b, shifts, masked):
    """The keywords of PixelCube.psf_photometry for cutout b of a scene."""
    return dict(star_col=sc["star_col"][b], star_row=sc["star_row"][b], prf=prf_object(sc["key"]), prf_index=int(sc["prf_index"][b]),
                shifts=(sc["shifts"][0][b], sc["shifts"][1][b]) if shifts else None,
                aperture_mask=sc["mask"][b] if masked else "all", column=COLUMN, row=ROW)


@functools.lru_cache(maxsize=None)
def mirror(shape, S, N, shifts=False, masked=True, use_flux_err=True):
    """PixelCube.psf_photometry(prf=) of every cutout of the scene -> list of dicts; shared, read-only."""
    from lightkurve_amd.correctors import PixelCube
    sc = scene(shape, S, N)
    return [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_photometry(use_flux_err=use_flux_err,
                                                                                **cutout_arguments(sc, b, shifts, masked))
            for b in range(sc["B"])]


# The launch above LDS_ATTR_BYTES: with shifts (11, 11) with 4 stars, 86 137 bytes, is the smallest of SHAPES that crosses it ((5,
# 7) with 2 stars needs 18 467); without shifts no shape of SHAPES does ((13, 17) with 3 stars: 34 709), and (21, 21) with 4 stars,
# 71 385 bytes, is the smallest square cutout with 4 stars that does.  Beyond LDS_MAX_BYTES: (13, 17) with 8 stars and shifts,
# 272 605 bytes, and without shifts (36, 36) with one star, 178 064 bytes.
LDS_CASES = [((21, 21), 4, TILE + 1, False, True, True)]
TOO_LARGE = (((13, 17), 8, True), ((36, 36), 1, False))

# what the GPU file compares: (shape, S, N, shifts, masked, use_flux_err)
GPU_CASES = ([(shape, S, 33, sh, not sh, err) for shape, S in SHAPES for sh in (False, True) for err in (True, False)]
             + [((5, 7), 2, N, sh, True, True) for N in N_VALUES for sh in (False, True)])
GPU_CASES = list(dict.fromkeys(GPU_CASES))
