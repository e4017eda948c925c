"""GPU: the one offsets kernel behind ``lk_diffimage_offsets_batch_dev`` and ``lk_ampimage_offsets_batch_dev``
(csrc/pixcube.hip: centroid_offsets_kernel) against numpy, at B = 1, 256 and 257: both sides of its one 256-thread block edge.

Centroids are multiples of 1/8 below 64 in magnitude, so every difference, product and sum of the kernel is exact whatever the
compiler contracts: ``offset`` and ``status`` must equal numpy's, ``offset_pix`` may differ by the device square root's
rounding alone (2 units in the last place).  Rows cycle through five kinds, so every B but 1 holds them all:
    kind  difference entry                                       amplitude entry
    0     an ordinary row: status 0                              the same
    1     a NaN centroid: 3                                      the same
    2     n_in == 0: 1                                           fit_status 1 and a NaN centroid: 1, passed through
    3     n_out == 0: 2                                          fit_status 2 and a NaN centroid: 2
    4     n_in == n_out == 0 and a NaN centroid: 1 (first test)  an ordinary row
The buffers hold TAIL more rows than B, filled with a sentinel the kernel must leave alone.
"""
import numpy as np
import pytest

from lightkurve_amd import _capi
from lightkurve_amd.device import _upload, _vp

pytestmark = pytest.mark.gpu

TAIL = 64
SENTINEL = -7


def rows(B, seed):
    """-> the centroids (a_col, a_row, b_col, b_row) float64[4, B] of the amplitude entry and of the difference entry, then
    n_in, n_out, fit_status int32[B]."""
    rng = np.random.default_rng(seed)
    cen = rng.integers(-511, 512, size=(4, B)).astype(np.float64) / 8.0
    i = np.arange(B)
    kind = i % 5
    n_in = np.where((kind == 2) | (kind == 4), 0, rng.integers(1, 50, B)).astype(np.int32)
    n_out = np.where((kind == 3) | (kind == 4), 0, rng.integers(1, 50, B)).astype(np.int32)
    fit = np.where(kind == 2, 1, np.where(kind == 3, 2, 0)).astype(np.int32)
    cen_amp, cen_diff = cen.copy(), cen.copy()
    for c, kinds in ((cen_amp, (1, 2, 3)), (cen_diff, (1, 4))):
        at = i[np.isin(kind, kinds)]
        c[at % 4, at] = np.nan                                  # (each of the four centroid arrays takes its turn)
    return cen_amp, cen_diff, n_in, n_out, fit


def reference(cen, lead):
    dx, dy = cen[0] - cen[2], cen[1] - cen[3]
    pix = np.sqrt(dx * dx + dy * dy)
    return np.stack([dx, dy], axis=1), pix, np.where(lead != 0, lead, np.where(np.isnan(pix), 3, 0)).astype(np.int32)


def run(entry, B, lead_arrays, cen, null=None):
    """One call of ``entry`` on fresh buffers; ``null``: the position of a pointer argument passed as NULL instead."""
    h = _capi.Handle.get(0)
    held = []

    def up(a, dtype, fill):
        buf, k = _upload(h, np.concatenate([a, np.full((TAIL,) + a.shape[1:], fill, dtype=dtype)]), 0, dtype)
        held.append(k)
        return buf

    d_lead = [up(a, np.int32, 1) for a in lead_arrays]
    d_cen = [up(c, np.float64, 0.5) for c in cen]
    d_off = up(np.zeros((B, 2)), np.float64, SENTINEL)
    d_pix, d_status = up(np.zeros(B), np.float64, SENTINEL), up(np.zeros(B, np.int32), np.int32, SENTINEL)
    args = [_vp(d.ptr) for d in d_lead + d_cen + [d_off, d_pix, d_status]]
    if null is not None:
        args[null] = _vp(None)
    rc = getattr(_capi._lib, entry)(h._h, B, *args, _vp(None))
    return (rc, d_off.download(np.float64, 2 * (B + TAIL)).reshape(-1, 2), d_pix.download(np.float64, B + TAIL),
            d_status.download(np.int32, B + TAIL))


def check(got, want, B, what):
    rc, off, pix, status = got
    w_off, w_pix, w_status = want
    assert rc == _capi.LK_OK, what
    assert np.all(off[B:] == SENTINEL) and np.all(pix[B:] == SENTINEL) and np.all(status[B:] == SENTINEL), what
    assert np.array_equal(status[:B], w_status), (what, np.flatnonzero(status[:B] != w_status)[:5])
    assert np.array_equal(off[:B], w_off, equal_nan=True), what
    assert np.array_equal(np.isnan(pix[:B]), np.isnan(w_pix)), what
    ok = ~np.isnan(w_pix)
    ulps = np.abs(pix[:B][ok] - w_pix[ok]) / np.spacing(w_pix[ok])
    print("%s: offset_pix max |device - numpy| = %.1f ulp over %d rows" % (what, ulps.max() if ulps.size else 0.0, ok.sum()))
    assert np.all(ulps <= 2), what


@pytest.mark.parametrize("B", [1, 256, 257])
def test_both_entry_points_against_numpy(B):
    cen_amp, cen_diff, n_in, n_out, fit = rows(B, seed=B)
    lead = np.where(n_in == 0, 1, np.where(n_out == 0, 2, 0))
    want = reference(cen_diff, lead)
    if B > 1:
        assert set(want[2].tolist()) == {0, 1, 2, 3} and np.isnan(cen_diff[:, n_in == 0]).any()
    check(run("lk_diffimage_offsets_batch_dev", B, [n_in, n_out], cen_diff), want, B, "difference, B = %d" % B)
    want = reference(cen_amp, fit)
    if B > 1:
        assert set(want[2].tolist()) == {0, 1, 2, 3} and np.isnan(cen_amp[:, fit != 0]).any(axis=0).all()
    check(run("lk_ampimage_offsets_batch_dev", B, [fit], cen_amp), want, B, "amplitude, B = %d" % B)


def test_a_null_argument_is_refused_by_both_entry_points():
    B = 3
    cen_amp, cen_diff, n_in, n_out, fit = rows(B, seed=0)
    for entry, lead, cen in (("lk_diffimage_offsets_batch_dev", [n_in, n_out], cen_diff),
                             ("lk_ampimage_offsets_batch_dev", [fit], cen_amp)):
        for null in range(len(lead) + 7):
            rc, off, pix, status = run(entry, B, lead, cen, null=null)
            assert rc == _capi.LK_EINVAL, null
            assert np.all(off[:B] == 0) and np.all(pix[:B] == 0) and np.all(status[:B] == 0), null      # nothing was launched
        assert run(entry, 0, lead, cen)[0] == _capi.LK_EINVAL
