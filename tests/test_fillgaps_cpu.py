"""CPU: the numpy restatement of fill_gaps (tests/fillgaps_cases.py) against numpy itself, the indexing of the noise stream, and
the argument checks of the Python front ends, which must raise before any device call."""
import numpy as np
import pytest

import fillgaps_cases as C
import overfit_cases as OC
from lightkurve_amd import _capi, fillgaps
from lightkurve_amd.device import DeviceLightCurveBatch
from lightkurve_amd.ingest import LightCurveBatch


def _ulps(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def test_cadence_path_times_are_np_interp():
    """d = t - m c interpolated with np.interp over the full cadence range, plus m c: what the reference computes.  2 ulp cover a
    numpy build whose interp loop contracts slope * (x - x0) + y0 into a fused multiply-add."""
    worst = 0.0
    for lc in C.batch("cadenceno"):
        keep = ~np.isnan(lc["flux"])
        t, c = lc["time"][keep], lc["cadenceno"][keep]
        if t.size < 2:
            continue
        nt, nc, ins = C.cadence_path_times(t, c)
        m = np.median(np.diff(t))
        ncf = np.arange(c[0], c[-1] + 1).astype(np.float64)
        ref = np.interp(ncf, c.astype(np.float64), t - m * c.astype(np.float64)) + m * ncf
        assert nc[0] == c[0] and nc[-1] == c[-1] and np.all(np.diff(nc) == 1)
        assert np.array_equal(nc[~ins], c)
        worst = max(worst, _ulps(nt, ref))
        assert np.all(np.abs(nt[~ins] - t) <= np.spacing(t))       # recomputed originals: within 1 ulp
    print("cadence path against np.interp: %.2f ulp" % worst)
    assert worst <= 2.0


def test_time_path_threshold_gaps():
    """1.1875 m inserts nothing, 1.25 m exactly one cadence; cut cadences of the binary grid come back bit for bit."""
    for gap, want in ((C.SHIFT_NONE, 0), (C.SHIFT_ONE, 1)):
        t = 2.0 + np.arange(40) / 64.0
        t[20:] += gap * C.M0
        nt, ins = C.time_path_times(t)
        assert int(ins.sum()) == want
        if want:
            assert nt[20] == t[19] + C.M0 and ins[20]
    lc = C.batch("time")[6]
    r = C.expected("time")[6]
    k599 = np.flatnonzero(lc["time"] == 2.0 + 599 / 64.0)[0]
    assert lc["time"][k599 + 1] - lc["time"][k599] == (1 + C.SHIFT_NONE) * C.M0
    o = np.flatnonzero(r["time"] == lc["time"][k599])[0]
    assert not r["inserted"][o + 1] and r["time"][o + 1] == lc["time"][k599 + 1]
    k899 = np.flatnonzero(lc["time"] == lc["time"][k599 + 1] + 299 / 64.0)[0]
    o = np.flatnonzero(r["time"] == lc["time"][k899])[0]
    assert r["inserted"][o + 1] and not r["inserted"][o + 2] and r["time"][o + 1] == lc["time"][k899] + C.M0
    for b in (3, 5, 7):                        # unshifted grids: the refill is the full grid
        K = C._cuts(b)[0]
        r = C.expected("time")[b]
        assert np.array_equal(r["time"], 2.0 + np.arange(K) / 64.0)
        assert r["n_inserted"] == K - C.LENGTHS[b] and r["m"] == C.M0
    assert C.expected("time")[4]["n_inserted"] == 0
    assert np.isnan(C.expected("time")[5]["flux_err"][20:23]).all()        # the NaN error next to the gap spreads into it
    assert [r["n_inserted"] for r in C.expected("time")] == [0, 0, 0, 1, 0, 3, 8, 3040]
    assert [r["n_inserted"] for r in C.expected("cadenceno")] == [0, 0, 0, 1, 0, 3, 7, 3040]


def test_normals_indexing_of_inserted_cadences():
    """Inserted cadence j of target b is normal j of (sample 0, target b): pair j // 2, cosine for even j, sine for odd j."""
    seed, target, sid = 0x1234567890, 7, 3
    g = OC.normals(11, 0, target, seed, sid)
    for j in (0, 1, 4, 9, 10):
        x0, x1, x2, x3 = OC.philox4x32_10(np.array([j // 2]), 0, target, sid, seed & 0xFFFFFFFF, seed >> 32)
        u1 = float(((int(x0[0]) >> 5) << 26) + (int(x1[0]) >> 6) + 1) * 2.0 ** -53
        u2 = float(((int(x2[0]) >> 5) << 26) + (int(x3[0]) >> 6)) * 2.0 ** -53
        r, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        assert g[j] == (r * np.sin(ang) if j & 1 else r * np.cos(ang))
        assert OC.normals(j + 1, 0, target, seed, sid)[j] == g[j]      # a prefix: the count of inserted cadences does not matter


class _NoDevice(object):
    def __getattr__(self, name):
        raise AssertionError("device call %s before the argument checks were done" % name)


def _host_batch(n_off, cadenceno=True):
    n_off = np.asarray(n_off, dtype=np.int64)
    b = DeviceLightCurveBatch.__new__(DeviceLightCurveBatch)
    b.n_off, b.nan_free, b.is_sorted, b.stream, b.meta, b._keep = n_off, True, True, 0, [dict() for _ in n_off[1:]], []
    b.d_time = b.d_flux = b.d_flux_err = object()
    b.d_quality = None
    b.d_cadenceno = object() if cadenceno else None
    b.handle = _NoDevice()
    return b


def test_front_ends_validate_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", _NoDevice())
    b = _host_batch([0, 30, 55])
    with pytest.raises(NotImplementedError, match="linear"):
        b.fill_gaps(method="linear")
    with pytest.raises(ValueError, match="carries cadence numbers"):
        _host_batch([0, 30, 55], cadenceno=False).fill_gaps(by="cadenceno")
    with pytest.raises(ValueError, match="by must be"):
        b.fill_gaps(by="index")
    with pytest.raises(ValueError, match=r"noise_std must hold one value per light curve: shape \(2,\)"):
        b.fill_gaps(noise_std=np.ones(3))
    with pytest.raises(ValueError, match="noise_std must be one of"):
        b.fill_gaps(noise_std="mad")
    with pytest.raises(ValueError, match=r"group must be an integer array .* shape \(2,\)"):
        b.stitch(group=[0, 1, 1])
    with pytest.raises(ValueError, match="group must be an integer array"):
        b.stitch(group=[0.5, 1.0])
    with pytest.raises(ValueError, match="corrector"):
        b.stitch(corrector="flatten")
    with pytest.raises(ValueError, match="order"):
        b.stitch(order="sorted")
    hb = LightCurveBatch(np.arange(5.0), np.ones(5), np.ones(5), [0, 2, 5])
    with pytest.raises(NotImplementedError):
        hb.fill_gaps(method="spline")
    with pytest.raises(ValueError, match="carries cadence numbers"):
        hb.fill_gaps(by="cadenceno")
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        hb.stitch(group=[0])


def test_noise_modes_and_stitch_plan():
    meta_n = [{"NORMALIZED": True}, {"NORMALIZED": True}]
    assert fillgaps.check_fill_gaps("gaussian_noise", "auto", True, "auto", None, meta_n)[:2] == (True, "cdpp")
    assert fillgaps.check_fill_gaps("gaussian_noise", "auto", False, "auto", None, [{"NORMALIZED": True}, {}])[:2] == (False, "std")
    assert fillgaps.check_fill_gaps("gaussian_noise", "time", True, "std", None, meta_n)[:2] == (False, "std")
    stats = np.array([[0.02, 1.0, 0.5, 3.0], [0.02, 2.0, 0.25, 0.0]])
    nm, ns = fillgaps.noise_arrays(stats, "cdpp", None, None, lambda: np.array([100.0, np.nan]))
    assert np.array_equal(nm, [1.0, 2.0]) and np.array_equal(ns, [100.0 * 1e-6, 0.25])      # a NaN CDPP falls back to sd
    labels = fillgaps.check_stitch([7, 3, 7, 9, 3], 5, None, "given")
    assert labels.tolist() == [0, 1, 0, 2, 1]                                             # numbered by first appearance
    perm, seg_off, n_off = fillgaps.stitch_plan(labels, [2, 3, 0, 5, 7])
    assert perm.tolist() == [0, 2, 1, 4, 3] and seg_off.tolist() == [0, 2, 4, 5] and n_off.tolist() == [0, 2, 12, 17]
    perm, _s, _n = fillgaps.stitch_plan(labels, [2, 3, 1, 5, 7], start_time=[9.0, 5.0, 1.0, 0.0, 4.0])
    assert perm.tolist() == [2, 0, 4, 1, 3]
    assert fillgaps.stitch_plan(fillgaps.check_stitch(None, 3, "normalize", "given"), [1, 2, 3])[2].tolist() == [0, 6]
