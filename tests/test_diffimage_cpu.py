"""CPU: the host mirrors of the quadratic centroid and of the transit difference image (correctors/pldcorrector.py:
centroid_quadratic, PixelCube.estimate_centroids, PixelCube.difference_image) against the numpy restatement of
tests/diffimage_cases.py, and the argument checks of the resident API that need no device."""
import numpy as np
import pytest

import diffimage_cases as C
from lightkurve_amd.correctors import PixelCube, centroid_quadratic


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def max_diff(a, b):
    ok = ~np.isnan(np.asarray(b, dtype=np.float64))
    return float(np.max(np.abs(np.asarray(a)[ok] - np.asarray(b)[ok]))) if ok.any() else 0.0


def test_fit_matrix_is_the_integer_table_over_36():
    """The table the kernel and the host mirror hard-code is (A^T A)^-1 A^T."""
    from lightkurve_amd.correctors.pldcorrector import _QUADRATIC_FIT_36
    assert np.max(np.abs(C.FIT * 36 - _QUADRATIC_FIT_36)) < 1e-12


def test_symmetric_source_returns_its_pixel_and_both_estimators_agree():
    for shape, (cy, cx) in (((7, 9), (3, 4)), ((9, 8), (5, 2)), ((3, 3), (1, 1))):
        im = C.psf(shape, cx, cy).astype(np.float32)
        yy, xx = np.indices(shape)
        sym = (np.abs(yy - cy) <= 1) & (np.abs(xx - cx) <= 1)            # an aperture that is symmetric about the source
        cube = PixelCube(np.arange(2.0), np.stack([im, im]), np.ones((2,) + shape, dtype=np.float32))
        qc, qr = cube.estimate_centroids(sym, method="quadratic", column=10, row=20)
        mc, mr = cube.estimate_centroids(sym, method="moments", column=10, row=20)
        col, row = centroid_quadratic(im, sym)
        err = max(abs(col - cx), abs(row - cy), np.max(np.abs(qc - 10 - cx)), np.max(np.abs(qr - 20 - cy)))
        agree = max(np.max(np.abs(qc - mc)), np.max(np.abs(qr - mr)))
        print("%s: |quadratic - pixel| = %.3g, |quadratic - moments| = %.3g" % (shape, err, agree))
        assert err < 1e-12 and agree < 1e-12
        assert C.centroid_quadratic(im, sym)[2] == cy * shape[1] + cx == centroid_quadratic(im, sym, return_peak=True)[2]


@pytest.mark.parametrize("shape", C.SHAPES)
def test_host_quadratic_centroids_equal_the_restatement(shape):
    flux = C.centroid_frames(shape)
    masks = C.cutout_masks(shape)
    for b in range(3):
        for mask in (None, masks[b]):
            cube = PixelCube(C.times(C.N_CENTROID), flux[b], np.ones_like(flux[b]))
            col, row = cube.estimate_centroids("all" if mask is None else mask, method="quadratic", column=3, row=-2)
            rc, rr, rp = C.centroids_quadratic(flux[b], mask, 3, -2)
            peak = np.array([centroid_quadratic(im, mask, return_peak=True)[2] for im in flux[b]])
            assert np.array_equal(peak, rp)
            assert same_nan(col, rc) and same_nan(row, rr)
            err = max(max_diff(col, rc), max_diff(row, rr))
            print("%s cutout %d mask %s: max |host - restatement| = %.3g px" % (shape, b, mask is not None, err))
            assert err < 1e-9
    # what the special frames are for
    col, row, peak = C.centroids_quadratic(flux[0])
    assert peak[C.TWO_MAXIMA] == 1 and peak[C.ALL_NAN] == -1 and peak[C.CORNER] == shape[0] * shape[1] - 1
    assert np.isnan(col[[C.NAN_INSIDE, C.ALL_NAN, C.CONSTANT]]).all()
    assert not np.isnan(col[[C.TWO_MAXIMA, C.CORNER, C.EDGE, C.NAN_OUTSIDE]]).any()
    col, row, peak = C.centroids_quadratic(flux[0], C.partial_mask(shape))
    assert peak[C.NEGATIVE] == 0                                        # a masked-out zero beats the all-negative aperture
    if shape != (3, 3):
        assert np.isnan(col[C.NEGATIVE]) and np.isnan(row[C.NEGATIVE])    # ... and its patch is flat


@pytest.mark.parametrize("shape", C.DIFF_SHAPES)
def test_host_difference_image_equals_the_restatement(shape):
    time, flux, err = C.diff_case(shape)
    ref = C.diff_reference(shape)
    assert 20 <= ref["n_in"][0] <= 60 and ref["n_out"][0] > 1.5 * ref["n_in"][0]
    assert list(ref["status"]) == [0, 0, 1] and ref["n_in"][2] == 0
    assert np.isnan(ref["mean_in"][0, 0, 0]) and not np.isnan(ref["mean_out"][0, 0, 0]) and not np.isnan(ref["mean_in"][0, 0, 1])
    for b, box in enumerate(C.BOXES):
        got = PixelCube(time[b], flux[b], err[b]).difference_image(*box)
        assert set(got) == set(ref)
        for key in ("cadence_class", "n_in", "n_out", "status"):
            assert np.array_equal(got[key], ref[key][b]), key
        for key in ("mean_in", "mean_out", "diff", "diff_err"):
            assert same_nan(got[key], ref[key][b]), key
            scale = np.nanmax(np.abs(ref[key][b])) if not np.isnan(ref[key][b]).all() else 1.0
            assert max_diff(got[key], ref[key][b]) / scale < 1e-12, key
        for key in ("centroid_diff", "centroid_out", "centroid_diff_moments", "centroid_out_moments", "offset", "offset_pix"):
            assert same_nan(got[key], ref[key][b]), key
            assert max_diff(got[key], ref[key][b]) < 1e-9, key


@pytest.mark.parametrize("shape", C.DIFF_SHAPES)
def test_difference_image_finds_the_dimming_pixel(shape):
    """The restatement itself: a dip on the neighbour two pixels away moves the difference image there, one on the target
    does not."""
    cy, cx = shape[0] // 2, shape[1] // 2
    ref = C.diff_reference(shape, "neighbour")
    print("neighbour dips: centroid_diff", ref["centroid_diff"][0], "offset_pix", ref["offset_pix"][0])
    assert np.hypot(ref["centroid_diff"][0, 0] - (cx + 2), ref["centroid_diff"][0, 1] - cy) < 0.2 and ref["offset_pix"][0] > 1.5
    ref = C.diff_reference(shape, "target")
    print("target dips: centroid_diff", ref["centroid_diff"][0], "offset_pix", ref["offset_pix"][0])
    assert ref["offset_pix"][0] < 0.2


def test_argument_validation():
    shape = (7, 9)
    time, flux, err = C.diff_case(shape)
    cube = PixelCube(time[1], flux[1], err[1])
    with pytest.raises(ValueError):
        cube.estimate_centroids(method="psf")
    with pytest.raises(ValueError):
        cube.difference_image(0.0, 1.0, 0.1)                                    # P = 0
    for widths in ((0.0, 1.0, 2.0), (1.5, 1.0, 2.0), (0.5, 2.0, 2.0), (-0.5, 1.0, 2.0)):
        with pytest.raises(ValueError):
            cube.difference_image(3.1, 1.234, 0.15, *widths)
    with pytest.raises(ValueError):
        centroid_quadratic(np.ones((2, 5)))                                     # no 3 x 3 patch
    with pytest.raises(ValueError):
        centroid_quadratic(np.ones((5, 5)), np.ones((4, 5), dtype=bool))
    with pytest.raises(ValueError):
        cube.estimate_centroids(np.ones((4, 5), dtype=bool), method="quadratic")
    assert np.isnan(centroid_quadratic(np.full((4, 4), np.nan))).all()          # the reference raises; the mirrors do not
    assert centroid_quadratic(np.full((4, 4), np.nan), return_peak=True)[2] == -1
