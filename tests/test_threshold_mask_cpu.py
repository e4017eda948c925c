"""No GPU: the host-side facts the device threshold mask and the ragged PLD call rest on.

``lk_cube_threshold_mask_batch_dev`` picks the masked pixel nearest to the reference pixel by SQUARED distance, (row - ref_row)^2
+ (col - ref_col)^2, where ``threshold_mask_from_median_image`` takes ``np.argmin`` over ``np.hypot``.  For the "center"
reference pixel (nx / 2, ny / 2) both are orderings of the same pixels; they must be the SAME ordering, ties included, or the
device could keep another region than the reference.  Squared distances there are multiples of 1/4 below 2^53, hence exact in
float64, so equal distances compare equal; what has to be shown is that np.hypot neither splits such a tie nor merges two
different distances."""
import numpy as np
import pytest

from lightkurve_amd.correctors.pldcorrector import _per_cutout_masks, _ragged_index_lists

SHAPES = [(ny, nx) for ny in range(4, 16) for nx in range(4, 16)]


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_squared_distance_orders_pixels_as_hypot_does(ny, nx):
    ref_col, ref_row = nx / 2, ny / 2
    rows, cols = np.divmod(np.arange(ny * nx), nx)                   # row-major, as np.argwhere lists the masked pixels
    d2 = (rows - ref_row) ** 2 + (cols - ref_col) ** 2
    hyp = np.array([np.hypot(r - ref_row, c - ref_col) for r, c in zip(rows, cols)])
    assert np.array_equal(np.argsort(d2, kind="stable"), np.argsort(hyp, kind="stable"))
    # ... and on every subset the first minimum is the same pixel: equal d2 <=> equal hypot, smaller d2 <=> smaller hypot
    assert np.array_equal(d2[:, None] < d2[None, :], hyp[:, None] < hyp[None, :])
    assert np.array_equal(d2[:, None] == d2[None, :], hyp[:, None] == hyp[None, :])


def test_ragged_index_lists_pad_with_minus_one_in_ascending_order():
    masks = np.zeros((3, 12), dtype=bool)
    masks[0, [1, 4, 7, 8, 11]] = True
    masks[1, [0, 2, 3]] = True
    masks[2, [5, 6, 9, 10]] = True
    idx, counts = _ragged_index_lists(masks, 3)
    assert idx.dtype == np.int32 and counts.dtype == np.int32 and idx.shape == (3, 5)
    assert counts.tolist() == [5, 3, 4]
    assert idx.tolist() == [[1, 4, 7, 8, 11], [0, 2, 3, -1, -1], [5, 6, 9, 10, -1]]
    # equal sizes: no padding at all
    idx, counts = _ragged_index_lists(masks[[1, 1]], 1)
    assert idx.tolist() == [[0, 2, 3], [0, 2, 3]] and counts.tolist() == [3, 3]


def test_ragged_index_lists_refuse_counts_below_pca_components():
    masks = np.zeros((4, 10), dtype=bool)
    masks[0, :6] = True
    masks[1, :3] = True
    masks[2, :4] = True
    masks[3, :2] = True
    with pytest.raises(ValueError, match=r"background masks of cutouts \[1, 3\] select \[3, 2\] pixels, fewer than pca_components = 4"):
        _ragged_index_lists(masks, 4, "background")
    idx, counts = _ragged_index_lists(masks, 2)                      # the smallest count itself is enough
    assert counts.tolist() == [6, 3, 4, 2] and idx.shape == (4, 6)
    with pytest.raises(ValueError, match=r"cutouts \[0\] select \[0\] pixels"):
        _ragged_index_lists(np.zeros((1, 5), dtype=bool), 1)
    with pytest.raises(ValueError, match="must be"):
        _ragged_index_lists(np.zeros(5, dtype=bool), 1)


def test_per_cutout_masks_are_told_from_shared_ones():
    assert _per_cutout_masks(None, 3, (4, 5)) is None
    assert _per_cutout_masks("threshold", 3, (4, 5)) is None
    assert _per_cutout_masks(np.ones((4, 5), bool), 3, (4, 5)) is None
    m = _per_cutout_masks(np.ones((3, 4, 5), np.uint8), 3, (4, 5))
    assert m.dtype == bool and m.shape == (3, 4, 5)
    with pytest.raises(ValueError, match="per-cutout masks"):
        _per_cutout_masks(np.ones((2, 4, 5), bool), 3, (4, 5))
