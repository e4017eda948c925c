"""The lean closed form of the fast Lomb-Scargle kernels (gls_power_sums_lean in csrc/ls_epilogue.hpp): the angle from two
reciprocal square roots — on every kernel of lsfast.hip that calls it.

Routes (oversampling 5 unless said; df = 0.01, f0 = df; three ragged targets of 1777 / 300 / 901 cadences, unequal errors):
  rows512   M = 27000: Nfft = 2^18 = 512 x 512, at most 256 sample-bearing rows -> pruned column kernel, 16-column tiles,
            fft_rows512_power_kernel
  generic   M = 2000: Nfft = 2^14 = 128 x 128 -> fft_rows_power_kernel<4, 3, 4>
  ov2       M = 2000, oversampling 2: Nfft = 2^12 = 64 x 64.  Every thread of the fused kernel needs 4 <= 8 outputs, so this
            shape runs fft_rows_power_kernel<3, 3, 4> with ALL of its four outputs per thread in use (generic uses one),
            not lsf_power_kernel
  reg_unfused  M = 40000, oversampling 1: Nfft = 2^16 = 256 x 256, 10 outputs per thread > 8 -> the register transforms
            write the spectra, lsf_power_kernel
  lds       M = 20: Nfft = 2^7 = 16 x 8, no register path -> fft_cols_kernel / fft_rows_kernel in LDS, lsf_power_kernel
Each runs the four normalisations x fit_mean on / off x dy given / None.

Reference: oracle.np_oracle.ls_power_fast (the numpy port of astropy's fast_impl), never another path of the library.
Tolerance (the parity tests'): 1e-9 of the target's largest reference power on the frequencies >= 1 / span, identical NaN
pattern there (below one cycle per baseline the closed form cancels and 1e-9 is not the reference's own precision).
Peaks: max_power / argmax of a call equal nanmax / nanargmax of the same call's power, bit for bit."""
import numpy as np
import pytest

from lightkurve_amd import _capi
from oracle import np_oracle as O

TOL = 1e-9
DF = 0.01
NS = (1777, 300, 901)
SPAN_DF = (0.24, 0.19, 0.12)            # span * df per target: 2 span df < 1/2, at most 256 of 512 rows of the 2 df grid
SCALE = np.array([1.5, 0.7, 2.0])       # 'lk_psd' per-target factors
NORMS = ("standard", "psd", "lk_amplitude", "lk_psd")
# name: (M, oversampling)
ROUTES = {"rows512": (27000, 5), "generic": (2000, 5), "ov2": (2000, 2), "reg_unfused": (40000, 1), "lds": (20, 5)}


def ceil_log2(v):
    m = 0
    while (1 << m) < v:
        m += 1
    return m


def geometry(M, oversampling):
    """lsfast_launch: log2 of Nfft, of N1 (column length) and of N2 (row length); outputs per thread of the fused row kernel."""
    m = max(3, ceil_log2(M * oversampling))
    m1, m2 = (m + 1) // 2, m // 2
    a = 1 << ((m2 + 1) // 2)
    k2need = (M + (1 << m1) - 1) >> m1
    return m, m1, m2, (k2need + a - 1) // a, k2need


def make_target(seed, n, span, f_sig):
    """n irregular sorted cadences on [0, span] (both ends sampled), a sinusoid well above the noise, unequal errors."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, span, n))
    t[0], t[-1] = 0.0, span
    y = 1.0 + 5e-3 * np.sin(2 * np.pi * f_sig * t + rng.uniform(0, 6.0)) + rng.normal(0, 5e-4, n)
    dy = 5e-4 * rng.uniform(0.5, 2.0, n)
    return t, y, dy


def targets(M):
    """The batch of a route: signals at 0.25, 0.33 and 0.41 of the grid's largest frequency."""
    return [make_target(4100 + i, n, s / DF, (0.25 + 0.08 * i) * M * DF) for i, (n, s) in enumerate(zip(NS, SPAN_DF))]


def pack(arrs):
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return np.concatenate(arrs), off


def run(tv, f0, M, oversampling, use_dy, fit_mean, norm, scale=None):
    t, off = pack([a for a, _, _ in tv])
    y, _ = pack([b for _, b, _ in tv])
    dy = pack([c for _, _, c in tv])[0] if use_dy else None
    return _capi.ls_fast_peaks_batch(t, y, off, dy=dy, f0=f0, df=DF, M=M, fit_mean=fit_mean, normalization=norm,
                                     scale=scale if norm == "lk_psd" else None, oversampling=oversampling)


def reference(tgt, f0, M, oversampling, use_dy, fit_mean, norm, lk_scale=1.0):
    t, y, dy = tgt
    with np.errstate(all="ignore"):
        return O.ls_power_fast(t, y, dy if use_dy else None, f0, DF, M, normalization=norm, lk_scale=lk_scale,
                               fit_mean=fit_mean, oversampling=oversampling)


def check_peaks(pw, mx, am):
    for b in range(pw.shape[0]):
        if np.all(np.isnan(pw[b])):
            assert np.isnan(mx[b]) and am[b] == -1, b
        else:
            assert mx[b] == np.nanmax(pw[b]) and am[b] == np.nanargmax(pw[b]), b


def check_parity(pw, ref, t, f0, M, label, min_frac=0.5):
    fr = f0 + DF * np.arange(M)
    cond = fr * (t.max() - t.min()) >= 1.0
    assert cond.sum() > min_frac * M, label
    assert np.array_equal(np.isfinite(ref[cond]), np.isfinite(pw[cond])), label
    ok = cond & np.isfinite(ref)
    err = np.max(np.abs(pw[ok] - ref[ok])) / np.max(np.abs(ref[ok]))
    print("%s: rel err %.3e over %d frequencies" % (label, err, ok.sum()))
    assert err <= TOL, (label, err)


def test_routes_are_what_they_claim():
    for name, (M, ov) in ROUTES.items():
        m, m1, m2, kb, k2need = geometry(M, ov)
        reg = 4 <= m1 <= 10 and 4 <= m2 <= 10
        rows2 = [min(1 << m1, int((2.0 * s * (1 << m) + 4.0) / (1 << m2)) + 1) for s in SPAN_DF]
        if name == "rows512":
            want = max(5, ceil_log2(max(rows2)))
            assert (m, m1, m2) == (18, 9, 9) and kb <= 8 and k2need <= 128 and max(rows2) <= 256 and want == 8 < m1
        elif name == "generic":
            assert (m, m2, kb) == (14, 7, 1) and reg
        elif name == "ov2":
            assert (m, m2, kb) == (12, 6, 4) and reg
        elif name == "reg_unfused":
            assert (m, m1, m2, kb) == (16, 8, 8, 10) and reg
        else:
            assert (m, m1, m2) == (7, 4, 3) and not reg
        assert all(2.0 * s * (1 << m) < (1 << m) - 8.0 for s in SPAN_DF)         # the 2 df grid does not wrap
    assert [len(t) for t, _, _ in targets(2000)] == list(NS)


@pytest.mark.gpu
@pytest.mark.parametrize("use_dy", [False, True], ids=["nody", "dy"])
@pytest.mark.parametrize("fit_mean", [True, False], ids=["fit_mean", "no_fit_mean"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_every_normalisation(route, fit_mean, use_dy):
    M, ov = ROUTES[route]
    tv = targets(M)
    for norm in NORMS:
        pw, mx, am = run(tv, DF, M, ov, use_dy, fit_mean, norm, SCALE)
        assert pw.shape == (3, M)
        check_peaks(pw, mx, am)
        for b, tgt in enumerate(tv):
            ref = reference(tgt, DF, M, ov, use_dy, fit_mean, norm, SCALE[b])
            check_parity(pw[b], ref, tgt[0], DF, M, "%s %s fit_mean %d dy %d target %d" % (route, norm, fit_mean, use_dy, b))


def degenerate_batch(M):
    """ordinary | one cadence at t = 0 | two cadences | constant flux (256 equal weights: the mean is exact) | ordinary"""
    o = targets(M)
    rng = np.random.default_rng(4200)
    tc = np.sort(rng.uniform(0.0, 17.0, 256))
    one = (np.array([0.0]), np.array([1.3]), np.array([5e-4]))
    two = (np.array([0.0, 7.3]), np.array([1.001, 0.998]), np.array([5e-4, 7e-4]))
    const = (tc - tc[0], np.ones(256), np.full(256, 5e-4))
    return [o[0], one, two, const, o[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("f0", [DF, 0.0], ids=["f0_df", "f0_zero"])
@pytest.mark.parametrize("route", ["rows512", "generic", "lds"])
def test_degenerate_targets_beside_ordinary_ones(route, f0):
    M, ov = ROUTES[route]
    tv = degenerate_batch(M)
    pw, mx, am = run(tv, f0, M, ov, False, True, "psd")
    check_peaks(pw, mx, am)
    refs = [reference(tgt, f0, M, ov, False, True, "psd") for tgt in tv]
    # one cadence: tan 2w = 0 / 0 at every frequency — the reference is NaN throughout, and so is the kernel
    assert np.all(np.isnan(refs[1]))
    assert np.all(np.isnan(pw[1])) and np.isnan(mx[1]) and am[1] == -1
    # constant flux: every y sum is an exact zero, so the power is 0 (not NaN) wherever the reference's is
    fr = f0 + DF * np.arange(M)
    cond = fr * tv[3][0].max() >= 1.0
    assert np.array_equal(np.isfinite(refs[3][cond]), np.isfinite(pw[3][cond]))
    assert np.all(refs[3][cond] == 0.0) and np.all(pw[3][cond] == 0.0)
    # two cadences (a floating-mean sinusoid through two points is under-determined: CC SS - ... cancels to rounding
    # noise, so only the call, the peaks and the neighbours are checked) and the ordinary targets beside them
    print("%s f0 %g two cadences: %d finite of %d, reference %d" % (route, f0, np.isfinite(pw[2]).sum(), M, np.isfinite(refs[2]).sum()))
    for b in (0, 4):
        check_parity(pw[b], refs[b], tv[b][0], f0, M, "%s f0 %g degenerate batch target %d" % (route, f0, b))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["rows512", "generic", "lds"])
def test_two_cadences_without_fit_mean(route):
    """Two cadences dt apart, no floating mean: two parameters through two points.  The normal equations' determinant
    CC SS - CS^2 is w1 w2 sin^2(2 pi f dt): where |sin(2 pi f dt)| >= 0.1 the fit is conditioned no worse than 100 and the
    parity bound holds with room; nearer the zeros the power is rounding noise over rounding noise in the reference too, and
    only the NaN pattern is compared."""
    M, ov = ROUTES[route]
    tv = degenerate_batch(M)
    pw, mx, am = run(tv, DF, M, ov, False, False, "psd")
    check_peaks(pw, mx, am)
    for b in (0, 4):
        ref = reference(tv[b], DF, M, ov, False, False, "psd")
        check_parity(pw[b], ref, tv[b][0], DF, M, "%s no fit_mean degenerate batch target %d" % (route, b))
    t = tv[2][0]
    ref = reference(tv[2], DF, M, ov, False, False, "psd")
    fr = DF + DF * np.arange(M)
    cond = fr * t[1] >= 1.0
    assert np.array_equal(np.isfinite(ref[cond]), np.isfinite(pw[2][cond]))
    ok = cond & np.isfinite(ref) & (np.abs(np.sin(2 * np.pi * fr * t[1])) >= 0.1)
    assert ok.sum() >= 5
    err = np.max(np.abs(pw[2][ok] - ref[ok])) / np.max(np.abs(ref[ok]))
    print("%s no fit_mean two cadences: rel err %.3e over %d frequencies" % (route, err, ok.sum()))
    assert err <= TOL, (route, err)


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_same_call_twice_is_bit_identical(route):
    M, ov = ROUTES[route]
    tv = targets(M)
    first = run(tv, DF, M, ov, True, True, "lk_amplitude")
    second = run(tv, DF, M, ov, True, True, "lk_amplitude")
    assert np.array_equal(first[0].view(np.int64), second[0].view(np.int64))
    assert np.array_equal(first[1].view(np.int64), second[1].view(np.int64))
    assert np.array_equal(first[2], second[2])
