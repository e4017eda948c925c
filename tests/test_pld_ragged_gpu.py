"""GPU: threshold masks computed on the device and PLD batches whose pixel masks differ in size (``ragged_masks=True``).

Yardsticks: ``threshold_mask_from_median_image`` (exact equality of the masks) and the EXISTING uniform PLD path run on each
cutout alone, ``pld_correct_batch([cube_b], ...)`` (identical outlier masks, max |delta corrected| / median(corrected) < 1e-6 —
the project's PLD parity, the bound of every test in tests/test_pld_gpu.py).  Each parity test prints the figure it measured."""
import numpy as np
import pytest

from lightkurve_amd import _capi, synth
from lightkurve_amd.correctors import PixelCube, pld_correct_batch
from lightkurve_amd.correctors.pldcorrector import threshold_mask_from_median_image as from_median
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch, _upload
from tests.test_pixcube_gpu import front_end_cubes, rolled_cubes

pytestmark = pytest.mark.gpu

PARITY = 1e-6
AMPS = (0, 30, 100, 300, 1000)
K2_SPECS = dict(aperture_mask=None, pld_aperture_mask="threshold", background_aperture_mask="background")


# ------------------------------------------------------------------------------------------------ helpers
def ragged_cubes(amps=AMPS, n=400):
    """Cutouts whose threshold masks differ in size: synth.pld_cutout(4, 20 + i) plus a static pattern of growing amplitude,
    which raises the MAD of the median image and so shrinks the mask (45, 38, 34, 25, 21 and, at amp 3000, 7 pixels)."""
    cubes = []
    for i, amp in enumerate(amps):
        t, flux, err, _ = synth.pld_cutout(4, 20 + i, n=n)
        pattern = (amp * np.abs(np.random.default_rng(100 + i).standard_normal((11, 11)))).astype(np.float32)
        cubes.append(PixelCube(t, (flux + pattern).astype(np.float32), err, mission="K2"))
    return cubes


def alone(cubes, masks=None, **kw):
    """The existing path on every cutout by itself; ``masks``: {argument: (B, ny, nx) array} given to cutout b as its own 2-D mask."""
    out = []
    for b, c in enumerate(cubes):
        own = {k: m[b] for k, m in (masks or {}).items()}
        corrected, outl = pld_correct_batch([c], **dict(kw, **own))
        out.append((corrected[0], outl[0]))
    return out


def assert_parity(got, ref, label):
    corrected, outl = got
    worst = 0.0
    for b, (rc, ro) in enumerate(ref):
        assert corrected[b].shape == rc.shape, (label, b)
        assert np.array_equal(outl[b], ro), "%s: outlier mask of cutout %d differs" % (label, b)
        worst = max(worst, float(np.max(np.abs(corrected[b] - rc)) / np.median(rc)))
    print("%s: max |delta corrected| / median = %.3e over %d cutouts" % (label, worst, len(ref)))
    assert worst < PARITY, (label, worst)
    return worst


def constant_cubes(images, n_cad=5):
    """One cutout per image, the same image in every cadence: the median image IS the image."""
    images = np.asarray(images, dtype=np.float32)
    flux = np.repeat(images[:, None], n_cad, axis=1)
    time = np.tile(np.arange(n_cad, dtype=np.float64), (len(images), 1))
    return DevicePixelCubeBatch.from_arrays(time, flux, np.ones_like(flux))


def mask_images(s):
    """(name, s x s image) cases; every special value the MAD cut has a rule for."""
    rng = np.random.default_rng(1000 + s)
    yy, xx = np.mgrid[:s, :s]

    def star(r, c, amp, width=1.3):
        return amp * np.exp(-((yy - r) ** 2 + (xx - c) ** 2) / (2 * width ** 2))

    noise = rng.normal(100.0, 3.0, (s, s))
    plain = noise + star(s / 2 - 0.3, s / 2 + 0.4, 4000.0)
    crowded = noise + star(s / 2, s / 2 - 0.5, 3000.0) + star(1.0, s - 2.0, 5000.0, 0.8) + star(s - 1.5, 0.5, 2500.0, 0.9)
    with_nan = plain.copy()
    with_nan[s // 2, s // 2] = np.nan                       # the brightest pixel has no value: nan_to_num -> 0, outside the mask
    with_nan[0, 1] = np.nan
    with_inf = plain.copy()
    with_inf[1, 1] = np.inf                                 # -> largest finite double: inside
    with_inf[s - 2, 2] = -np.inf                            # -> smallest: outside; both count for the nanmedian, not for the MAD
    no_finite = np.full((s, s), np.nan)
    no_finite[0, 0], no_finite[s - 1, s - 1] = np.inf, -np.inf
    empty = np.full((s, s), np.inf)                         # most pixels +inf: nanmedian = inf = the cut; DBL_MAX >= inf is false
    empty.ravel()[: (s * s) // 2 - 1] = noise.ravel()[: (s * s) // 2 - 1]
    twins = 1.0 + (yy * s + xx) / float(s * s)              # smooth floor in [1, 2): MAD ~ 0.25, only the two stars pass the cut
    twins[s // 2, 1] = 1000.0                               # two one-pixel regions, mirror images about the centre column
    twins[s // 2, s - 1] = 1000.0
    even_count = plain.copy()
    even_count[0, 0] = np.nan                               # flips the parity of the finite count: the other np.median branch
    flat = np.full((s, s), 7.0)                             # MAD 0: every pixel is >= the cut, one region
    return [("plain", plain), ("crowded", crowded), ("nan", with_nan), ("inf", with_inf), ("no_finite", no_finite),
            ("empty", empty), ("twins", twins), ("even_count", even_count), ("flat", flat)]


MASK_ARGS = [(3, "center", False), (0, None, True), (0, "center", False), (3, None, False), (3, (2.0, 3.0), False),
             (3, "center", True), (1.5, (0.0, 0.0), False)]


# ------------------------------------------------------------------------------------------------ 1. masks
@pytest.mark.filterwarnings("ignore:Mean of empty slice")     # np.median of no finite pixel, inside the yardstick
@pytest.mark.parametrize("s", [6, 9, 10, 11, 15])
def test_device_threshold_masks_equal_the_host_function(s):
    cases = mask_images(s)
    names = [c[0] for c in cases]
    images = np.array([c[1] for c in cases]).astype(np.float32).astype(np.float64)
    # the cases are what they are named for (on the yardstick), so the test cannot degenerate silently
    host = {nm: from_median(im, 3, "center") for nm, im in zip(names, images)}
    assert not host["no_finite"].any() and not host["empty"].any() and np.isfinite(images[names.index("empty")]).any()
    both = from_median(images[names.index("twins")], 3, None)
    assert both.sum() == 2 and both[s // 2, 1] and both[s // 2, s - 1]
    assert host["twins"].sum() == 1 and host["twins"][s // 2, 1]              # equal distances: the first in row-major order
    # several regions, of which the labelling keeps one (the 6 x 6 image is too crowded for any pixel to pass the cut)
    assert s == 6 or 0 < host["crowded"].sum() < from_median(images[names.index("crowded")], 3, None).sum()
    assert host["flat"].all()
    batch = constant_cubes(images)
    med = batch.median_images()
    assert np.array_equal(med, images, equal_nan=True)
    for threshold, ref, invert in MASK_ARGS:
        want = np.stack([from_median(im, threshold, ref) for im in med])
        want = ~want if invert else want
        got = batch.threshold_masks(threshold, ref, invert=invert)
        assert got.dtype == bool and got.shape == want.shape
        for b, nm in enumerate(names):
            assert np.array_equal(got[b], want[b]), (s, nm, threshold, ref, invert)
        d_mask, d_cnt, d_idx = batch.threshold_masks(threshold, ref, to_host=False, invert=invert)
        B, npix = len(names), s * s
        flat = want.reshape(B, npix)
        assert np.array_equal(d_mask.download(np.uint8, B * npix, stream=batch.stream).reshape(B, npix).astype(bool), flat)
        cnt = d_cnt.download(np.int32, B, stream=batch.stream)
        idx = d_idx.download(np.int32, B * npix, stream=batch.stream).reshape(B, npix)
        assert np.array_equal(cnt, flat.sum(axis=1))
        for b in range(B):
            assert np.array_equal(idx[b, :cnt[b]], np.flatnonzero(flat[b])) and np.all(idx[b, cnt[b]:] == -1), (s, names[b])


def serpentine(s):
    """One long 4-connected region winding through every other row, and a second region it does not touch: the worst case for
    label propagation (the smallest label has to travel the whole path)."""
    im = 1.0 + np.arange(s * s, dtype=np.float64).reshape(s, s) / (s * s)
    for r in range(0, s - 2, 2):
        im[r, :] = 1000.0
        im[r + 1, (s - 1) if (r // 2) % 2 == 0 else 0] = 1000.0
    im[s - 1, s - 3:] = 900.0
    return im


@pytest.mark.parametrize("s", [32, 64])
def test_device_threshold_masks_on_large_cutouts(s):
    images = np.array([serpentine(s), mask_images(s)[1][1], mask_images(s)[0][1]]).astype(np.float32).astype(np.float64)
    path = from_median(images[0], 3, (s - 1.0, s - 1.0))                # nearest to the bottom right corner: the small region
    assert path.sum() == 3 and from_median(images[0], 3, "center").sum() > s * (s // 2 - 1)
    batch = constant_cubes(images, n_cad=3)
    for threshold, ref, invert in MASK_ARGS + [(3, (s - 1.0, s - 1.0), False)]:
        want = np.stack([from_median(im, threshold, ref) for im in images])
        got = batch.threshold_masks(threshold, ref, invert=invert)
        assert np.array_equal(got, ~want if invert else want), (s, threshold, ref, invert)


def test_cutouts_beyond_the_device_limit_take_the_host_function():
    s = 65
    assert s * s > _capi.CUBE_MASK_MAX_NPIX == 4096
    images = np.array([mask_images(s)[0][1], mask_images(s)[1][1]]).astype(np.float32).astype(np.float64)
    batch = constant_cubes(images, n_cad=3)
    for threshold, ref, invert in ((3, "center", False), (0, None, True)):
        want = np.stack([from_median(im, threshold, ref) for im in images])
        assert np.array_equal(batch.threshold_masks(threshold, ref, invert=invert), ~want if invert else want)
    with pytest.raises(ValueError, match="at most 4096 pixels"):
        batch.threshold_masks(to_host=False)
    B, npix = 2, s * s
    d_med = batch._median_images_dev()
    from lightkurve_amd.device import DeviceBuffer, _vp
    d_mask, d_cnt, d_idx = DeviceBuffer(batch.handle, B * npix), DeviceBuffer(batch.handle, B * 4), DeviceBuffer(batch.handle, B * npix * 4)
    rc = _capi._lib.lk_cube_threshold_mask_batch_dev(batch.handle._h, B, s, s, _vp(d_med.ptr), 3.0, 1, s / 2, s / 2, 0, _vp(d_mask.ptr),
                                                     _vp(d_cnt.ptr), _vp(d_idx.ptr), _vp(None))
    assert rc == 1                                                     # LK_EINVAL


def test_device_threshold_masks_over_the_kept_cadences_only():
    cubes = front_end_cubes()                                # 4 all-NaN and 3 all-zero cadences per cutout, at different places
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    d_f, d_e, d_keep, n, _ = batch._aperture("all")
    assert n == 793
    for threshold, ref, invert in ((3, "center", False), (0, None, True)):
        got_kept = batch.threshold_masks(threshold, ref, d_keep=d_keep, invert=invert)
        got_all = batch.threshold_masks(threshold, ref, invert=invert)
        for b, c in enumerate(cubes):
            f32, e32 = c._aperture_sums(np.ones(c.shape[1:], bool))
            keep = ~(np.isnan(f32) | np.isnan(e32))
            with np.errstate(all="ignore"):
                kept = from_median(np.nanmedian(c.flux[keep].astype(np.float64), axis=0), threshold, ref)
                every = from_median(np.nanmedian(c.flux.astype(np.float64), axis=0), threshold, ref)
            assert np.array_equal(got_kept[b], ~kept if invert else kept), (b, threshold)
            assert np.array_equal(got_all[b], ~every if invert else every), (b, threshold)
    # a keep array of the caller's own: half of the cadences of a cutout whose star moves
    t, flux, err, _ = synth.pld_cutout(4, 77, n=200, npix=10)
    flux = flux.copy()
    flux[100:] = np.roll(flux[100:], 3, axis=2)
    one = DevicePixelCubeBatch.from_cubes([PixelCube(t, flux, err)] * 2)
    keep = np.zeros((2, 200), np.uint8)
    keep[0, :100], keep[1, 100:] = 1, 1
    d_keep, hold = _upload(one.handle, keep, one.stream, np.uint8)
    got = one.threshold_masks(3, "center", d_keep=d_keep)
    want = [from_median(np.median(flux[:100].astype(np.float64), axis=0)), from_median(np.median(flux[100:].astype(np.float64), axis=0))]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not np.array_equal(want[0], want[1])
    del hold


# ------------------------------------------------------------------------------------------------ 2. ragged parity, K2 defaults
def test_ragged_threshold_masks_order3_match_each_cutout_alone():
    cubes = ragged_cubes()
    counts = [int(c.create_threshold_mask(3).sum()) for c in cubes]
    assert len(set(counts)) >= 4 and min(counts) >= 16, counts
    kw = dict(K2_SPECS, pld_order=3, pca_components=16)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    got = batch.pld_correct(ragged_masks=True, **kw)
    assert got[0].shape == (5, 400)
    assert_parity(got, alone(cubes, **kw), "order 3, 16 components, threshold masks of %s pixels" % counts)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        batch.pld_correct(**kw)


# ------------------------------------------------------------------------------------------------ 3. counts below pca_components
def test_ragged_order2_and_a_cutout_with_too_few_pixels():
    cubes = ragged_cubes(AMPS + (3000,))
    assert int(cubes[5].create_threshold_mask(3).sum()) == 7
    kw = dict(K2_SPECS, pld_order=2, pca_components=8)
    with pytest.raises(ValueError, match=r"PLD masks of cutouts \[5\] select \[7\] pixels, fewer than pca_components = 8"):
        DevicePixelCubeBatch.from_cubes(cubes).pld_correct(ragged_masks=True, **kw)
    with pytest.raises(ValueError, match=r"PLD masks of cutouts \[5\] select \[7\] pixels, fewer than pca_components = 8"):
        pld_correct_batch(cubes, ragged_masks=True, **kw)
    got = DevicePixelCubeBatch.from_cubes(cubes[:5]).pld_correct(ragged_masks=True, **kw)
    assert_parity(got, alone(cubes[:5], **kw), "order 2, 8 components")
    # ... and with 7 components the 7-pixel cutout is as good as the others
    kw7 = dict(kw, pca_components=7)
    got = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(ragged_masks=True, **kw7)
    assert_parity(got, alone(cubes, **kw7), "order 2, 7 components, a 7-pixel mask among them")


def test_c_abi_refuses_counts_outside_the_block():
    rng = np.random.default_rng(5)
    B, N, P = 2, 120, 12
    pix = rng.uniform(50, 60, (B, N, P)).astype(np.float32)
    pix[1, :, 9:] = 0.0
    lcf = pix.sum(axis=2).astype(np.float32)
    t = np.tile(np.linspace(0.0, 3.0, N), (B, 1))
    knots = np.tile(np.array([0.0, 3.0]), (B, 1))
    args = (pix, pix, lcf, t, knots, lcf.astype(np.float64), np.ones((B, N)), 1, 4, 1)
    ok = _capi.pld_correct_batch(*args, p_count=[12, 9], pb_count=[12, 9])
    assert np.isfinite(ok["model"]).all()
    for counts in ([12, 3], [12, 0], [13, 12]):
        with pytest.raises(ValueError, match="ragged call needs"):
            _capi.pld_correct_batch(*args, p_count=counts, pb_count=[12, 12])
        with pytest.raises(ValueError, match="ragged call needs"):
            _capi.pld_correct_batch(*args, p_count=[12, 12], pb_count=counts)


# ------------------------------------------------------------------------------------------------ 4. ragged background masks
@pytest.mark.parametrize("normalize", [True, False])
def test_ragged_per_cutout_background_masks(normalize):
    cubes = ragged_cubes()
    rng = np.random.default_rng(17)
    pm = np.zeros((11, 11), bool)
    pm[2:9, 2:9] = True
    bm = np.zeros((5, 11, 11), bool)
    for b, size in enumerate((72, 40, 55, 16, 63)):
        outside = np.flatnonzero(~pm.ravel())
        bm[b].ravel()[rng.choice(outside, size, replace=False)] = True
    assert sorted(bm.reshape(5, -1).sum(axis=1).tolist()) == [16, 40, 55, 63, 72]
    kw = dict(aperture_mask=pm, pld_aperture_mask=pm, pld_order=2, pca_components=16, normalize_background_pixels=normalize)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        batch.pld_correct(background_aperture_mask=bm, **kw)
    got = batch.pld_correct(background_aperture_mask=bm, ragged_masks=True, **kw)
    assert_parity(got, alone(cubes, {"background_aperture_mask": bm}, **kw), "ragged background, normalize=%s" % normalize)
    # per-cutout masks of ONE size need no keyword, and give the bits of the call with it
    same_size = np.stack([np.roll(bm[3], b, axis=1) for b in range(5)])
    a = batch.pld_correct(background_aperture_mask=same_size, **kw)
    b_ = batch.pld_correct(background_aperture_mask=same_size, ragged_masks=True, **kw)
    assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1])
    assert_parity(a, alone(cubes, {"background_aperture_mask": same_size}, **kw), "per-cutout background masks of one size")


# ------------------------------------------------------------------------------------------------ 5. host front end
def test_host_front_end_ragged_equals_the_resident_call():
    """Both front ends end in the same design, regression and epilogue kernels on the same numbers (the zero-padded float32
    blocks, the counts, the SAP columns and the knots are equal bit for bit, as tests/test_pixcube_gpu.py shows for the
    uniform call), so the results must be EQUAL, not merely close."""
    cubes = ragged_cubes()
    kw = dict(K2_SPECS, pld_order=3, pca_components=16, ragged_masks=True)
    host = pld_correct_batch(cubes, **kw)
    dev = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(**kw)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    from lightkurve_amd import batch as lkbatch
    sharded = lkbatch.pld_correct_batch(cubes, **kw)                 # (one rank: the keyword reaches the shard)
    assert np.array_equal(sharded[0], host[0]) and np.array_equal(sharded[1], host[1])
    with pytest.raises(ValueError, match="different numbers of pixels"):
        lkbatch.pld_correct_batch(cubes, **dict(kw, ragged_masks=False))


# ------------------------------------------------------------------------------------------------ 6. the refused batch of before
def test_rolled_cubes_with_a_widened_star_are_accepted_with_the_keyword():
    cubes = rolled_cubes(widen_last=True)
    kw = dict(aperture_mask="all", pld_aperture_mask="threshold", background_aperture_mask="background", pld_order=2,
              pca_components=8)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        batch.pld_correct(**kw)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        pld_correct_batch(cubes, **kw)
    got = batch.pld_correct(ragged_masks=True, **kw)
    assert got[0].shape == (3, 696)
    assert_parity(got, alone(cubes, **kw), "rolled cubes, the last one widened")
    assert_parity(pld_correct_batch(cubes, ragged_masks=True, **kw), alone(cubes, **kw), "the same through the host front end")


# ------------------------------------------------------------------------------------------------ 7. bits
def test_equal_sizes_keep_their_bits_and_ragged_calls_repeat():
    cubes = rolled_cubes()
    kw = dict(K2_SPECS, pld_order=2, pca_components=8)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    plain = batch.pld_correct(**kw)
    keyword = batch.pld_correct(ragged_masks=True, **kw)
    assert np.array_equal(plain[0], keyword[0]) and np.array_equal(plain[1], keyword[1])
    h_plain, h_keyword = pld_correct_batch(cubes, **kw), pld_correct_batch(cubes, ragged_masks=True, **kw)
    assert np.array_equal(h_plain[0], h_keyword[0]) and np.array_equal(h_plain[1], h_keyword[1])
    assert np.array_equal(plain[0], h_plain[0])
    ragged = ragged_cubes()
    kw3 = dict(K2_SPECS, pld_order=3, pca_components=16, ragged_masks=True)
    rb = DevicePixelCubeBatch.from_cubes(ragged)
    a = rb.pld_correct(**kw3)
    t, y, e, off = synth.ls_batch(21, 3, 4000)                       # other work in between: different scratch contents
    _capi.ls_fast_batch(t - t[0], y, off, f0=0.01, df=0.01, M=20000, normalization="psd")
    b = rb.pld_correct(**kw3)
    c = DevicePixelCubeBatch.from_cubes(ragged).pld_correct(**kw3)
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])


# ------------------------------------------------------------------------------------------------ 8. chaining
def test_ragged_resident_result_chains_into_flatten():
    cubes = ragged_cubes()
    kw = dict(K2_SPECS, pld_order=2, pca_components=8, ragged_masks=True)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    corrected, outl = batch.pld_correct(**kw)
    dev, d_outl = batch.pld_correct(to_host=False, **kw)
    assert isinstance(dev, DeviceLightCurveBatch)
    host = dev.to_host()
    B, n = corrected.shape
    assert np.array_equal(host.n_off, np.arange(B + 1) * n)
    assert np.array_equal(host.flux.reshape(B, n), corrected)
    assert np.array_equal(d_outl.download(np.uint8, B * n).reshape(B, n).astype(bool), outl)
    flat = dev.flatten(window_length=101).to_host()
    ref = DeviceLightCurveBatch.from_arrays(host.time, host.flux, host.flux_err, host.n_off).flatten(window_length=101).to_host()
    assert np.array_equal(flat.flux, ref.flux, equal_nan=True) and np.array_equal(flat.flux_err, ref.flux_err, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 9. every eigen-solver route
def route_cubes(npix, B=4, n=300):
    return [PixelCube(*synth.pld_cutout(4, 40 + i, n=n, npix=npix)[:3], mission="K2") for i in range(B)]


def nested_masks(npix, sizes):
    """One mask per size: the pixels nearest to the centre first (so that every mask holds the star)."""
    yy, xx = np.mgrid[:npix, :npix]
    order = np.argsort(((yy - npix / 2 + 0.5) ** 2 + (xx - npix / 2 + 0.5) ** 2).ravel(), kind="stable")
    masks = np.zeros((len(sizes), npix * npix), bool)
    for b, size in enumerate(sizes):
        masks[b, order[:size]] = True
    return masks.reshape(len(sizes), npix, npix)


@pytest.mark.parametrize("npix,sizes,pca,order", [
    (15, (225, 180, 100, 20), 8, 2),     # pitch 225 > 138: subspace iteration; its 100-column matrix iterates on its own block,
                                         # the 20-column one (not wider than the 24-vector basis) takes the Jacobi inside that launch
    (15, (140, 139, 64, 3), 3, 1),       # the same launch with blocks on both sides of every route's limit
    (11, (121, 120, 64, 17), 16, 2),     # pitch 121: the tridiagonal direct solver, (P & 3) != 0 projection
    (11, (120, 63, 33, 16), 16, 1),      # pitch 120: its (P & 3) == 0 projection; a block of exactly pca_components columns
    (9, (3, 2, 1, 2), 1, 1),             # pitch 3: the direct solver on 1-, 2- and 3-column blocks (float64 ratio matrix, no f32 Gram)
    (9, (2, 1, 2, 1), 1, 2),             # pitch 2: the Jacobi on C itself
])
def test_every_eigen_solver_route_takes_the_padding(npix, sizes, pca, order):
    cubes = route_cubes(npix)
    pm = nested_masks(npix, sizes)
    kw = dict(aperture_mask="all", background_aperture_mask="all", pld_order=order, pca_components=pca)
    got = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(pld_aperture_mask=pm, ragged_masks=True, **kw)
    assert_parity(got, alone(cubes, {"pld_aperture_mask": pm}, **kw), "%d x %d, PLD masks of %s pixels" % (npix, npix, list(sizes)))
    # the same sizes as BACKGROUND masks (row sums with normalize_background_pixels run over the padded rows)
    if min(sizes) >= 2:
        kwb = dict(aperture_mask="all", pld_aperture_mask="empty", pld_order=order, pca_components=pca)
        got = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(background_aperture_mask=pm, ragged_masks=True, **kwb)
        assert_parity(got, alone(cubes, {"background_aperture_mask": pm}, **kwb), "background masks of %s pixels" % list(sizes))
