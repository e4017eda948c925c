"""GPU: the under-fitting goodness metric of RAGGED batches on a cadence grid (lk_underfit_grid_*, metrics.underfit_metric_ragged_batch,
DeviceLightCurveBatch.under_fitting_metric(cadenceno=)) against the repository's own ``underfit_metric_neighbors`` per target, fed
the neighbours on the target's cadences with NaN where a neighbour lacks one.  Tolerance: the house 1e-9 absolute on metric and
correlations (a correct kernel is within about n 2^-53)."""
import ctypes
import functools

import numpy as np
import pytest

import ragged_goodness_cases as R
import underfit_cases as U
from lightkurve_amd import _capi
from lightkurve_amd.correctors import metrics
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch, _off_ptr, _upload, _vp

pytestmark = pytest.mark.gpu
TOL = 1e-9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def same_result(a, b):
    return (same_bits(a["metric"], b["metric"]) and same_bits(a["correlations"], b["correlations"])
            and np.array_equal(a["n_common"], b["n_common"]))


def host(p, nb, masked=True):
    """The host-pointer entry point on a packed ragged batch (R.pack)."""
    return _capi.underfit_grid_neighbors_batch(p["flux"], p["n_off"], p["rows"], len(p["grid"]), nb,
                                               cadence_mask=p["mask"] if masked else None)


def resident(p, err=None):
    """A NaN-free resident batch of a packed ragged batch, with its cadence numbers."""
    dev = DeviceLightCurveBatch.from_arrays(p["time"], p["flux"], err, p["n_off"], cadenceno=p["cadenceno"])
    return dev.remove_nans()


def dev_call(p, nb, masked=True, block_from=None):
    """The _dev entry points on device buffers, rows given: the direct call, or (block_from = a packed batch) the prepared-rows
    route with the block made from that batch under its own mask."""
    h = _capi.Handle.get(0)
    nb = np.ascontiguousarray(nb, dtype=np.int32)
    B, M, Nx = len(p["n_off"]) - 1, nb.shape[1], len(p["grid"])

    def up(a, dtype):
        return (None, None) if a is None else _upload(h, a, 0, dtype)

    def ptr(buf):
        return _vp(buf.ptr if buf is not None else None)

    d_flux, k1 = up(p["flux"], np.float64)
    d_rows, k2 = up(p["rows"], np.int32)
    d_cm, k3 = up(p["mask"].astype(np.uint8) if (masked and p["mask"] is not None) else None, np.uint8)
    d_nb, k4 = up(nb if M else None, np.int32)
    d_corr, d_nc, d_metric = DeviceBuffer(h, max(B * M, 1) * 8), DeviceBuffer(h, B * 4), DeviceBuffer(h, B * 8)
    lib = _capi._lib
    if block_from is None:
        _capi._check(lib.lk_underfit_grid_neighbors_batch_dev(h._h, B, _off_ptr(p["n_off"]), ptr(d_rows), Nx, ptr(d_flux), ptr(d_cm), M,
                                                              ptr(d_nb), ptr(d_corr) if M else None, ptr(d_nc), ptr(d_metric), None))
    else:
        q = block_from
        Bn = len(q["n_off"]) - 1
        nbytes = ctypes.c_int64(0)
        _capi._check(lib.lk_underfit_grid_rows_bytes(Bn, Nx, ctypes.byref(nbytes)))
        pitch = (Nx + 127) // 128 * 128
        assert nbytes.value == Bn * pitch * 8 + Bn * (pitch // 64) * 8          # the z rows, then the presence words
        d_block = DeviceBuffer(h, nbytes.value)
        dq_flux, k5 = up(q["flux"], np.float64)
        dq_rows, k6 = up(q["rows"], np.int32)
        dq_cm, k7 = up(q["mask"].astype(np.uint8) if (masked and q["mask"] is not None) else None, np.uint8)
        _capi._check(lib.lk_underfit_grid_rows_prepare_dev(h._h, Bn, _off_ptr(q["n_off"]), ptr(dq_rows), Nx, ptr(dq_flux), ptr(dq_cm),
                                                           ptr(d_block), nbytes.value, None))
        _capi._check(lib.lk_underfit_grid_against_rows_batch_dev(h._h, B, _off_ptr(p["n_off"]), ptr(d_rows), Nx, ptr(d_flux), ptr(d_cm),
                                                                 Bn, ptr(d_block), M, ptr(d_nb), ptr(d_corr) if M else None, ptr(d_nc),
                                                                 ptr(d_metric), None))
    corr = d_corr.download(np.float64, B * M).reshape(B, M) if M else np.empty((B, 0))
    return dict(metric=d_metric.download(np.float64, B), correlations=corr, n_common=d_nc.download(np.int32, B))


def check(got, ref, nb):
    """got (dict) against the mirror's (metric, corr, n_common)."""
    ref_m, ref_c, ref_n = ref
    nb = np.asarray(nb)
    pad = nb < 0
    assert np.array_equal(got["n_common"], ref_n)
    assert got["correlations"].shape == nb.shape and np.array_equal(np.isnan(got["correlations"]), pad)
    err_m = np.max(np.abs(got["metric"] - ref_m))
    err_c = np.max(np.abs(got["correlations"][~pad] - ref_c[~pad])) if (~pad).any() else 0.0
    print("max |metric - mirror| %.3e   max |corr - mirror| %.3e   n_common %d..%d" % (err_m, err_c, ref_n.min(), ref_n.max()))
    assert err_m < TOL and err_c < TOL


@functools.lru_cache(maxsize=None)
def reference_run(cfg):
    """One run of the host-pointer entry point per configuration, shared by the tests that compare against it."""
    f = R.ragged_field(*cfg)
    r = host(f, f["neighbors"])
    for a in r.values():
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_parity_with_the_mirror_through_the_three_front_ends(cfg):
    f = R.ragged_field(*cfg)
    nb, Nx = f["neighbors"], cfg[2]
    ref = R.reference(cfg)
    assert ref[2].min() >= 0.6 * Nx                       # a collapsed intersection cannot hide a failure
    if cfg[0] in (21, 22, 23):
        assert np.median(ref[0]) < 0.5
    r = reference_run(cfg)
    check(r, ref, nb)
    assert same_result(dev_call(f, nb), r)
    m, c, n = resident(f).under_fitting_metric(nb, cadence_mask=f["mask"], return_correlations=True, cadenceno=f["grid"],
                                               return_common=True)
    assert same_result(dict(metric=m, correlations=c, n_common=n), r)
    cads, fl, ms = (np.split(f[k], f["n_off"][1:-1]) for k in ("cadenceno", "flux", "mask"))
    m2, c2, n2 = metrics.underfit_metric_ragged_batch(fl, cads, f["grid"], nb, cadence_mask_list=ms, return_correlations=True,
                                                      return_common=True)
    assert same_result(dict(metric=m2, correlations=c2, n_common=n2), r)
    assert same_bits(resident(f).under_fitting_metric(nb, cadence_mask=f["mask"], cadenceno=f["grid"]), r["metric"])


# ------------------------------------------------------------------------------------------------ 2. the uniform call's bits
@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 127, 128, 129, 2049])
def test_full_presence_without_a_mask_gives_the_bits_of_the_uniform_call(N):
    f = U.field(30 + N, 5, N, 4)
    p = R.pack(f["y"], np.ones(f["y"].shape, dtype=bool))
    uni = _capi.underfit_neighbors_batch(f["y"], f["neighbors"])
    for r in (host(p, f["neighbors"]), dev_call(p, f["neighbors"])):
        assert same_bits(r["metric"], uni["metric"]) and same_bits(r["correlations"], uni["correlations"])
        assert np.all(r["n_common"] == N)
    m, c = resident(p).under_fitting_metric(f["neighbors"], return_correlations=True, cadenceno=p["grid"])
    assert same_bits(m, uni["metric"]) and same_bits(c, uni["correlations"])


# ------------------------------------------------------------------------------------------------ 3. holes at the edges
def test_holes_that_straddle_the_word_step_and_chunk_edges():
    """Nx = 2050: words end at 63 | 64, steps at 127 | 128, the LDS chunk at 2047 | 2048, and the last row is alone in its step."""
    Nx = 2050
    f = U.field(55, 6, Nx, 5)
    has = np.ones((6, Nx), dtype=bool)
    has[0, [63, 64]] = False
    has[1, [127, 128]] = False
    has[2, [2047, 2048]] = False
    has[3, Nx - 1] = False
    p = R.pack(f["y"], has, f["cm"], f["t"])
    ref = R.mirror(f["y"], has & f["cm"][None, :], f["neighbors"], f["t"])
    r = host(p, f["neighbors"])
    check(r, ref, f["neighbors"])
    lost = (~has).any(axis=0) & f["cm"]
    assert r["n_common"].max() <= f["cm"].sum() and r["n_common"].min() == f["cm"].sum() - lost.sum()
    assert same_result(dev_call(p, f["neighbors"]), r)
    # without the mask every hole counts
    r2 = host(p, f["neighbors"], masked=False)
    check(r2, R.mirror(f["y"], has, f["neighbors"], f["t"]), f["neighbors"])
    assert r2["n_common"].min() == Nx - 7


# ------------------------------------------------------------------------------------------------ 4. neighbour lists
def test_more_neighbours_than_one_trip_of_the_wavefronts():
    """M = 70 on B = 80: three trips of 32 list positions, the last one partly filled; the first 33 are one position into the second."""
    cfg = R.CONFIGS[2]
    assert cfg[1] == 80 and cfg[3] == 70
    f = R.ragged_field(*cfg)
    check(reference_run(cfg), R.reference(cfg), f["neighbors"])
    nb = f["neighbors"][:, :33]
    r = host(f, nb)
    check(r, R.mirror(f["y"], f["has"] & f["cm"][None, :], nb, f["t"]), nb)
    assert (r["n_common"] > reference_run(cfg)["n_common"]).any()       # fewer neighbours, more common cadences


def test_padding_single_neighbour_and_no_neighbours():
    cfg = R.CONFIGS[3]
    f = R.ragged_field(*cfg)
    present = f["has"] & f["cm"][None, :]
    nb = f["neighbors"].copy()
    nb[0, 1:] = -1           # one neighbour
    nb[1, :] = -1            # none: metric exactly 1, correlations NaN, n_common the target's own count
    nb[2, ::2] = -1          # padding in between
    nb[3, :3] = -1           # padding in front
    r = host(f, nb)
    check(r, R.mirror(f["y"], present, nb, f["t"]), nb)
    assert r["metric"][1] == 1.0 and np.all(np.isnan(r["correlations"][1])) and r["n_common"][1] == present[1].sum()
    assert same_result(dev_call(f, nb), r)
    none = np.zeros((len(nb), 0), dtype=np.int32)
    r0 = host(f, none)
    assert r0["correlations"].shape == (len(nb), 0) and np.all(r0["metric"] == 1.0)
    assert np.array_equal(r0["n_common"], present.sum(axis=1))
    m0, c0, n0 = resident(f).under_fitting_metric(none, cadence_mask=f["mask"], return_correlations=True, cadenceno=f["grid"],
                                                  return_common=True)
    assert c0.shape == (len(nb), 0) and np.all(m0 == 1.0) and np.array_equal(n0, r0["n_common"])
    r1 = host(f, f["neighbors"][:, :1])
    check(r1, R.mirror(f["y"], present, f["neighbors"][:, :1], f["t"]), f["neighbors"][:, :1])


def test_duplicated_neighbour_equals_the_mirror_with_the_column_repeated():
    cfg = R.CONFIGS[1]
    f = R.ragged_field(*cfg)
    nb = f["neighbors"].copy()
    nb[:, 2] = nb[:, 0]
    r = host(f, nb)
    check(r, R.mirror(f["y"], f["has"] & f["cm"][None, :], nb, f["t"]), nb)
    assert same_bits(r["correlations"][:, 2], r["correlations"][:, 0])


def test_disjoint_light_curves_give_nan_and_no_error():
    y = 1000.0 + np.random.default_rng(5).normal(0, 1, (3, 300))
    has = np.ones((3, 300), dtype=bool)
    has[0, 150:] = False
    has[1, :150] = False
    has[2, 151:] = False              # shares exactly one cadence (row 150) with 1
    nb = np.array([[1, -1], [0, -1], [1, -1], ], dtype=np.int32)
    p = R.pack(y, has)
    for r in (host(p, nb), dev_call(p, nb)):
        assert r["n_common"].tolist() == [0, 0, 1]
        assert np.all(np.isnan(r["metric"])) and np.all(np.isnan(r["correlations"]))
    nb2 = np.array([[2, -1], [-1, -1], [0, -1]], dtype=np.int32)      # 0 and 2 share 150 cadences
    r = host(p, nb2)
    check(r, R.mirror(y, has, nb2), nb2)
    assert r["n_common"].tolist() == [150, 150, 150]


def test_constant_flux_neighbour_and_target():
    cfg = R.CONFIGS[3]
    f = R.ragged_field(*cfg)
    y = f["y"].copy()
    y[4, :] = 1234.5                   # z == 0 exactly: the mirror's rms = inf rule
    p = R.pack(y, f["has"], f["cm"], f["t"])
    nb = f["neighbors"]
    r = host(p, nb)
    check(r, R.mirror(y, f["has"] & f["cm"][None, :], nb, f["t"]), nb)
    assert np.all(bits(r["correlations"][4]) == 0) and r["metric"][4] == 1.0
    assert np.all(bits(r["correlations"][nb == 4]) == 0)


# ------------------------------------------------------------------------------------------------ 5. order independence
def test_a_sub_batch_gives_the_same_bits():
    cfg = R.CONFIGS[0]
    f = R.ragged_field(*cfg)
    full = reference_run(cfg)
    for t in (0, 17, 36):
        idx = np.concatenate([[t], f["neighbors"][t]])
        sub_nb = np.full((len(idx), len(idx) - 1), -1, dtype=np.int32)
        sub_nb[0] = np.arange(1, len(idx))
        r = host(R.pack(f["y"][idx], f["has"][idx], f["cm"], f["t"]), sub_nb)
        assert same_bits(r["correlations"][0], full["correlations"][t]) and bits(r["metric"][0]) == bits(full["metric"][t])
        assert r["n_common"][0] == full["n_common"][t]


def test_permuting_a_row_permutes_the_correlations_bit_for_bit():
    cfg = R.CONFIGS[2]
    f = R.ragged_field(*cfg)
    base = reference_run(cfg)
    nb = f["neighbors"].copy()
    perm = np.random.default_rng(1).permutation(nb.shape[1])
    nb[3] = nb[3][perm]
    nb[7] = nb[7][::-1]
    r = host(f, nb)
    assert same_bits(r["correlations"][3], base["correlations"][3][perm])
    assert same_bits(r["correlations"][7], base["correlations"][7][::-1])
    untouched = np.delete(np.arange(len(nb)), [3, 7])
    assert same_bits(r["correlations"][untouched], base["correlations"][untouched])
    assert same_bits(r["metric"][untouched], base["metric"][untouched]) and np.array_equal(r["n_common"], base["n_common"])


def test_two_runs_are_equal():
    cfg = R.CONFIGS[2]
    f = R.ragged_field(*cfg)
    assert same_result(host(f, f["neighbors"]), reference_run(cfg))


# ------------------------------------------------------------------------------------------------ 6. prepared rows
def test_the_prepared_rows_route_equals_the_direct_route():
    for cfg in (R.CONFIGS[0], R.CONFIGS[3]):
        f = R.ragged_field(*cfg)
        assert same_result(dev_call(f, f["neighbors"], block_from=f), reference_run(cfg))


def test_neighbor_batch_equal_to_the_batch_gives_the_bits_of_the_call_without_it():
    cfg = R.CONFIGS[1]
    f = R.ragged_field(*cfg)
    nb = f["neighbors"]
    dev = resident(f)
    a = dev.under_fitting_metric(nb, return_correlations=True, cadenceno=f["grid"], return_common=True)
    b = dev.under_fitting_metric(nb, return_correlations=True, cadenceno=f["grid"], return_common=True, neighbor_batch=dev)
    c = dev.under_fitting_metric(nb, return_correlations=True, cadenceno=f["grid"], return_common=True, neighbor_batch=resident(f))
    for x in (b, c):
        assert same_bits(a[0], x[0]) and same_bits(a[1], x[1]) and np.array_equal(a[2], x[2])
    check(dict(metric=a[0], correlations=a[1], n_common=a[2]), R.mirror(f["y"], f["has"], nb, f["t"]), nb)
    # a masked target against unmasked neighbour rows: the neighbours' medians are over all of their cadences
    present = f["has"] & f["cm"][None, :]
    m, cc, n = dev.under_fitting_metric(nb, cadence_mask=f["mask"], return_correlations=True, cadenceno=f["grid"], return_common=True,
                                        neighbor_batch=dev)
    ref = R.mirror(f["y"], present, nb, f["t"], zn=R.z_rows(f["y"], f["has"]))
    check(dict(metric=m, correlations=cc, n_common=n), ref, nb)


def test_cadences_off_the_grid_are_dropped_first():
    cfg = R.CONFIGS[3]
    f = R.ragged_field(*cfg)
    keep = np.ones(cfg[2], dtype=bool)
    keep[[0, 7, 64]] = False                                  # the grid loses three cadences that the targets still have
    grid = f["grid"][keep]
    has = f["has"][:, keep]
    y, cm, t = f["y"][:, keep], f["cm"][keep], f["t"][keep]
    m, c, n = resident(f).under_fitting_metric(f["neighbors"], cadence_mask=f["mask"], return_correlations=True, cadenceno=grid,
                                               return_common=True)
    check(dict(metric=m, correlations=c, n_common=n), R.mirror(y, has & cm[None, :], f["neighbors"], t), f["neighbors"])


# ------------------------------------------------------------------------------------------------ 7. chain
def test_cbv_correct_then_under_fitting_metric_stays_resident():
    cfg = R.CONFIGS[0]
    f = R.ragged_field(*cfg)
    nb, grid, B = f["neighbors"], f["grid"], cfg[1]
    dev = resident(f, err=1e-3 * f["flux"])
    corrected, _d_outl, _d_w = dev.cbv_correct(f["S"], cbv_indices=[1, 2], cadence_mask=f["mask"], to_host=False, cadenceno=grid)
    d_metric, d_corr, d_nc = corrected.under_fitting_metric(nb, cadence_mask=f["mask"], return_correlations=True, to_host=False,
                                                            cadenceno=grid, return_common=True)
    metric = d_metric.download(np.float64, B, stream=corrected.stream)          # one download at the end
    corr = d_corr.download(np.float64, nb.size, stream=corrected.stream).reshape(nb.shape)
    n_common = d_nc.download(np.int32, B, stream=corrected.stream)
    flux = np.full(f["y"].shape, np.nan)
    flux[f["has"]] = corrected.flux_host()
    check(dict(metric=metric, correlations=corr, n_common=n_common),
          R.mirror(np.nan_to_num(flux), f["has"] & f["cm"][None, :], nb, f["t"]), nb)
    print("min metric after cbv_correct %.4f, median before %.4f" % (metric.min(), np.median(reference_run(cfg)["metric"])))
    assert metric.min() > 0.99 and np.median(reference_run(cfg)["metric"]) < 0.5


# ------------------------------------------------------------------------------------------------ 8. errors
def test_bad_rows_and_shapes_are_refused():
    f = R.ragged_field(*R.CONFIGS[3])
    nb = f["neighbors"]
    bad = dict(f)
    rows = f["rows"].copy()
    n1 = int(f["n_off"][1])
    rows[n1 + 3] = rows[n1 + 2]                               # target 1: not strictly increasing
    bad["rows"] = rows
    with pytest.raises(ValueError, match="target 1: rows must be strictly increasing"):
        host(bad, nb)
    with pytest.raises(ValueError, match="light curve 1: rows must be strictly increasing"):
        dev_call(bad, nb)
    rows = f["rows"].copy()
    rows[-1] = len(f["grid"])
    bad["rows"] = rows
    with pytest.raises(ValueError, match="rows must be strictly increasing indices"):
        dev_call(bad, nb)
    h = _capi.Handle.get(0)
    out = ctypes.c_int64(0)
    assert _capi._lib.lk_underfit_grid_rows_bytes(0, 10, ctypes.byref(out)) == _capi.LK_EINVAL
    assert _capi._lib.lk_underfit_grid_rows_bytes(1, _capi.UNDERFIT_GRID_MAX_NX + 1, ctypes.byref(out)) == _capi.LK_EINVAL
    assert _capi._lib.lk_underfit_grid_rows_bytes(1, _capi.UNDERFIT_GRID_MAX_NX, ctypes.byref(out)) == 0
    z = np.zeros(4)
    off = np.array([0, 2, 4], dtype=np.int64)
    r = np.array([0, 1, 0, 1], dtype=np.int32)
    ip = _capi._c_i32p
    for B, Nx, M, nbc in ((0, 2, 0, None), (2, 0, 0, None), (2, 2, -1, None), (2, 2, 1, np.array([[0], [0]], dtype=np.int32)),
                          (2, 2, 1, np.array([[1], [2]], dtype=np.int32))):
        rc = _capi._lib.lk_underfit_grid_neighbors_batch(h._h, B, _capi._ptr(off, _capi._c_ip), _capi._ptr(r, ip), Nx, _capi._ptr(z),
                                                         None, M, _capi._ptr(nbc, ip), None, None, _capi._ptr(z))
        assert rc == _capi.LK_EINVAL, (B, Nx, M)
