"""The numpy restatement of the quadratic centroid and of the transit difference image, and the cases the CPU and GPU tests
share (tests/test_diffimage_cpu.py, tests/test_diffimage_gpu.py).  Nothing here calls the package: the contract is restated.

Quadratic centroid (lightkurve.utils.centroid_quadratic): z = data * mask; k = nanargmax(z); (yy, xx) = divmod(k, nx) clamped
so that the 3 x 3 patch stays inside; the least-squares quadratic through the patch by (A^T A)^-1 A^T (np.linalg.inv, NOT the
integer table the package hard-codes); det = 4 d f - e^2, |det| < 1e-6 -> NaN; col = column + xx - 1 + xm, row = row + yy - 1 +
ym.  An image without a value gives NaN and peak -1.

Difference image: class 1 where |x| < in_width D, 2 where out_inner D <= |x| < out_outer D, x = mod(t - t0 + P/2, P) - P/2;
per pixel the nan-aware float64 means of the float32 values per class, diff = mean_out - mean_in, diff_err = sqrt(sum_in e^2 /
n_in^2 + sum_out e^2 / n_out^2) over the same values."""
import functools

import numpy as np

CADENCE = 1.0 / 48.0
N_CENTROID = 130                      # not a multiple of 4 (wavefronts per workgroup) or of 64
SHAPES = ((7, 9), (9, 8), (3, 3))     # 63 pixels: fewer than a wavefront; 72: crosses the lane stride; 3 x 3: every patch clamped
N_DIFF = 700
DIFF_SHAPES = ((7, 9), (9, 8), (12, 11))   # 132 pixels: more than the 128 lanes of an accumulating workgroup; 700 cadences: 6 chunks
BOXES = ((3.1, 1.234, 0.15), (2.3, 0.9, 0.2), (40.0, -10.0, 0.15))      # (P, t0, D); the last has no transit inside the baseline

_A = np.array([[1, x, y, x * x, x * y, y * y] for y in range(3) for x in range(3)], dtype=np.float64)
FIT = np.linalg.inv(_A.T @ _A) @ _A.T


# ------------------------------------------------------------------------------------------------ restatement
def centroid_quadratic(data, mask=None, column=0, row=0):
    """-> (col, row, peak) of one (ny, nx) image."""
    with np.errstate(all="ignore"):
        z = np.asarray(data) if mask is None else np.asarray(data) * np.asarray(mask, dtype=bool)
        if np.all(np.isnan(z)):
            return np.nan, np.nan, -1
        k = int(np.nanargmax(z))
        ny, nx = z.shape
        yy, xx = divmod(k, nx)
        yy, xx = min(max(yy, 1), ny - 2), min(max(xx, 1), nx - 2)
        a, b, c, d, e, f = FIT @ z[yy - 1:yy + 2, xx - 1:xx + 2].astype(np.float64).flatten()
        det = 4 * d * f - e ** 2
        if abs(det) < 1e-6:
            return np.nan, np.nan, k
        xm = -(2 * f * b - c * e) / det
        ym = -(2 * d * c - b * e) / det
        return column + xx - 1 + xm, row + yy - 1 + ym, k


def centroids_quadratic(cube, mask=None, column=0, row=0):
    """Every cadence of one cutout (N, ny, nx) -> col[N], row[N], peak[N]."""
    out = [centroid_quadratic(im, mask, column, row) for im in cube]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.int32))


def centroid_moments(image, mask=None, column=0, row=0):
    """The moment centroid of one image -> (col, row): float64 nansums inside the mask, a zero or NaN total gives NaN."""
    image = np.asarray(image, dtype=np.float64)
    m = np.ones(image.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    yy, xx = np.indices(image.shape)
    with np.errstate(all="ignore"):
        f = np.where(m, image, np.nan)
        tot = np.nansum(f)
        if not tot == tot or tot == 0:
            return np.nan, np.nan
        return np.nansum((column + xx) * f) / tot, np.nansum((row + yy) * f) / tot


def classes(time, period, transit_time, duration, in_width=0.5, out_inner=1.0, out_outer=2.0):
    with np.errstate(all="ignore"):
        hp = period / 2
        x = np.abs(np.mod(np.asarray(time, dtype=np.float64) - transit_time + hp, period) - hp)
        cls = np.zeros(len(x), dtype=np.uint8)
        cls[x < in_width * duration] = 1
        cls[(x >= out_inner * duration) & (x < out_outer * duration)] = 2
    return cls


def difference_image(time, flux, flux_err, period, transit_time, duration, in_width=0.5, out_inner=1.0, out_outer=2.0, mask=None,
                     column=0, row=0):
    """One cutout -> the dict of DevicePixelCubeBatch.difference_images without the batch axis."""
    cls = classes(time, period, transit_time, duration, in_width, out_inner, out_outer)
    out = {"cadence_class": cls, "n_in": int((cls == 1).sum()), "n_out": int((cls == 2).sum())}
    flux, err = np.asarray(flux, dtype=np.float64), np.asarray(flux_err, dtype=np.float64)
    with np.errstate(all="ignore"):
        mean, var = {}, {}
        for name, c in (("in", 1), ("out", 2)):
            f, e = flux[cls == c], err[cls == c]
            ok = ~np.isnan(f)
            n = ok.sum(axis=0).astype(np.float64)
            mean[name] = np.where(ok, f, 0.0).sum(axis=0) / n
            var[name] = np.where(ok, e * e, 0.0).sum(axis=0) / n ** 2
        out.update(mean_in=mean["in"], mean_out=mean["out"], diff=mean["out"] - mean["in"], diff_err=np.sqrt(var["in"] + var["out"]))
    for key, im in (("diff", out["diff"]), ("out", out["mean_out"])):
        out["centroid_" + key] = np.array(centroid_quadratic(im, mask, column, row)[:2], dtype=np.float64)
        out["centroid_%s_moments" % key] = np.array(centroid_moments(im, mask, column, row), dtype=np.float64)
    out["offset"] = out["centroid_diff"] - out["centroid_out"]
    out["offset_pix"] = float(np.sqrt(np.sum(out["offset"] ** 2)))
    out["status"] = 1 if out["n_in"] == 0 else 2 if out["n_out"] == 0 else 3 if np.isnan(out["offset_pix"]) else 0
    return out


# ------------------------------------------------------------------------------------------------ frames
def psf(shape, cx, cy, amplitude=1000.0, sigma=0.9):
    yy, xx = np.indices(shape)
    return amplitude * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma * sigma))


# the special frames of cutout 0 (cadence numbers); the others are noisy PSF frames
TWO_MAXIMA, CORNER, EDGE, NAN_OUTSIDE, NAN_INSIDE, ALL_NAN, CONSTANT, NEGATIVE = 3, 5, 6, 8, 10, 12, 14, 16


@functools.lru_cache(maxsize=None)
def centroid_frames(shape):
    """float32 flux (3, N_CENTROID, ny, nx) of `shape`: a Gaussian PSF (amplitude 1000, sigma 0.9 px) whose sub-pixel centre
    varies per cadence, background 20, noise 3; cutout 0 carries the special frames.  Read-only."""
    ny, nx = shape
    rng = np.random.RandomState(100 * ny + nx)
    B, N = 3, N_CENTROID
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    for b in range(B):
        for i in range(N):
            cx, cy = (nx - 1) / 2 + rng.uniform(-0.5, 0.5), (ny - 1) / 2 + rng.uniform(-0.5, 0.5)
            flux[b, i] = psf(shape, cx, cy) + 20.0 + rng.normal(0.0, 3.0, shape)
    f = flux[0]
    f[TWO_MAXIMA, ny - 1, nx - 2] = f[TWO_MAXIMA, 0, 1] = 5000.0          # two equal maxima: the first index wins
    f[CORNER, ny - 1, nx - 1] = 6000.0                                  # the patch is clamped on both axes
    f[EDGE, 0, nx // 2] = 6000.0                                        # ... on one
    if ny > 4 and nx > 4:
        f[NAN_OUTSIDE, 0, 0] = np.nan                                   # outside the patch around the centre: ignored
    f[NAN_INSIDE, ny // 2, nx // 2] = np.nan                            # the brightest pixel's neighbour (or itself): NaN
    f[ALL_NAN] = np.nan
    f[CONSTANT] = 20.0                                                  # det = 0
    f[NEGATIVE] = -psf(shape, (nx - 1) / 2, (ny - 1) / 2) - 1.0        # under partial_mask() the argmax is a masked-out zero
    flux.setflags(write=False)
    return flux


def partial_mask(shape):
    """The lower right block: pixel 0 and the whole patch around (1, 1) are outside it (for the 7 x 9 and 9 x 8 cutouts)."""
    ny, nx = shape
    m = np.zeros(shape, dtype=bool)
    m[max(ny // 2 - 1, 2):, max(nx // 2 - 1, 2):] = True
    return m


def cutout_masks(shape):
    """One mask per cutout: the partial mask, the interior, a random one that keeps the 3 x 3 block at the centre (holes next to
    the brightest pixel make saddle-shaped patches whose extremum lies hundreds of pixels away: rounding grows by that factor,
    and a bound in pixels says nothing there)."""
    ny, nx = shape
    rng = np.random.RandomState(7)
    m = np.zeros((3,) + tuple(shape), dtype=bool)
    m[0] = partial_mask(shape)
    m[1, 1:ny - 1, 1:nx - 1] = True
    m[2] = rng.rand(ny, nx) < 0.7
    m[2, ny // 2 - 1:ny // 2 + 2, nx // 2 - 1:nx // 2 + 2] = True
    return m


def times(n, start=0.5):
    return start + np.arange(n) * CADENCE


@functools.lru_cache(maxsize=None)
def diff_case(shape, dip_on="neighbour"):
    """(time (3, N), flux, flux_err (3, N, ny, nx) float32) for BOXES: a target (amplitude 1000) at the centre pixel and a
    neighbour (amplitude 300) two pixels to its right, background 20, noise 0.5; a 1 % box dip on `dip_on` at each cutout's box.
    Cutout 0 has one NaN time (an in-transit cadence), pixel (0, 1) NaN at some and pixel (0, 0) at all of its in-transit
    cadences.  Read-only."""
    ny, nx = shape
    cy, cx = ny // 2, nx // 2
    rng = np.random.RandomState(1000 * ny + nx)
    B, N = len(BOXES), N_DIFF
    time = np.tile(times(N), (B, 1))
    target, neighbour = psf(shape, cx, cy), psf(shape, cx + 2, cy, amplitude=300.0)
    flux = np.empty((B, N, ny, nx), dtype=np.float32)
    for b, (P, t0, D) in enumerate(BOXES):
        dip = np.where(classes(time[b], P, t0, D) == 1, 0.99, 1.0)[:, None, None]
        scene = target * (dip if dip_on == "target" else 1.0) + neighbour * (dip if dip_on == "neighbour" else 1.0)
        flux[b] = scene + 20.0 + rng.normal(0.0, 0.5, (N, ny, nx))
    err = (0.5 + 0.1 * rng.rand(B, N, ny, nx)).astype(np.float32)
    inside = np.flatnonzero(classes(time[0], *BOXES[0]) == 1)
    flux[0, inside, 0, 0] = np.nan
    flux[0, inside[::3], 0, 1] = np.nan
    time[0, inside[4]] = np.nan
    for a in (time, flux, err):
        a.setflags(write=False)
    return time, flux, err


@functools.lru_cache(maxsize=None)
def diff_reference(shape, dip_on="neighbour"):
    """difference_image of every cutout of diff_case, stacked -> dict of arrays with the batch axis.  Read-only."""
    time, flux, err = diff_case(shape, dip_on)
    one = [difference_image(time[b], flux[b], err[b], *BOXES[b]) for b in range(len(BOXES))]
    return {k: np.stack([np.asarray(o[k]) for o in one]) for k in one[0]}
