"""The routes of lsfast_launch / lsfastchi2_launch beside the hot one (2^16 .. 2^20 grids, oversampling >= 4, pruned column
kernel, fused row kernel), each through the batch API:

R1  Nfft = bitceil(M * oversampling) = 2^21 .. 2^24: m1 > 10, no register path.  hipMemsetAsync, lsf_scatter_kernel for every
    target (time-ordered ones too), lsf_unquantize_kernel, the LDS transforms fft_cols_kernel / fft_rows_kernel at N1 = 2048 or
    4096 (CT = 2 or 1 columns, RT = 4, 2 or 1 rows per workgroup, ~98 KB of dynamic LDS), lsf_power_kernel, peaks by
    argmax_launch; for nterms = 2 the same transforms on six grids and lsf_chi2_power_kernel.
R2  Nfft = 2^3 .. 2^7: m2 < 4, the same generic kernels at N1 = 4 .. 16.  Grids with bitceil(M * oversampling) < 8 stay out:
    lsfast_launch pads them to 8 cells where astropy transforms 4 or fewer, so the two extirpolate onto different grids; that
    is the launcher's documented floor, not something these tests pin either way.
R3  register path without the fused row kernel: rows_power_available is false when ceil(ceil(M / N1) / 2^ceil(m2 / 2)) > 8
    (oversampling 1 .. 3): spreading of ordered and unordered targets, launch_cols_reg with rows_used, launch_rows_reg,
    lsf_power_kernel, argmax_launch.

Reference: oracle.np_oracle.ls_power_fast / ls_power_fastchi2 (numpy ports of astropy's fast_impl / fastchi2_impl), never
another path of the library.  Tolerance (the file family's): max |gpu - ref| <= 1e-9 max |ref| per target over the
frequencies with f (t.max() - t.min()) >= 1, identical finite / NaN pattern there; returned peaks equal nanmax / nanargmax of
the returned powers bit for bit.  The worst relative error of each case is printed."""
import numpy as np
import pytest

from lightkurve_amd import _capi
from oracle import np_oracle as O

TOL = 1e-9


# ------------------------------------------------------------------------------------ the launchers' geometry, restated
def ceil_log2(v):
    m = 0
    while (1 << m) < v:
        m += 1
    return m


def geometry(M, oversampling):
    """lsfast_launch: m = log2 Nfft, m1 = log2 N1 (column length), m2 = log2 N2 (row length)."""
    m = max(3, ceil_log2(M * oversampling))
    return m, (m + 1) // 2, m // 2


def reg_path(m1, m2):
    return 4 <= m1 <= 10 and 4 <= m2 <= 10


def fused_kb(m1, m2, M):
    """Outputs per thread the fused row kernel would need; it is instantiated for <= 8."""
    a = 1 << ((m2 + 1) // 2)
    k2need = (M + (1 << m1) - 1) >> m1
    return (k2need + a - 1) // a


def rows_power_available(m1, m2, M):
    return 4 <= m2 <= 10 and fused_kb(m1, m2, M) <= 8


def generic_tiles(m1, m2):
    """(CT, RT) of fft_cols_kernel / fft_rows_kernel: columns / rows of 4096 points per workgroup."""
    n1, n2 = 1 << m1, 1 << m2
    return max(1, min(n2, 4096 // n1)), max(1, min(n1, 4096 // n2))


def nowrap(t, nfft, df):
    """lsf_prep_kernel: the 2 df grid of a target does not wrap (with sorted times: an 'ordered' target)."""
    return 2.0 * (t.max() - t.min()) * nfft * df < nfft - 8.0


# ------------------------------------------------------------------------------------ targets
def make_target(seed, n, span, f_sig):
    """n irregular sorted cadences on [0, span] (both ends sampled): 1 + 5e-3 sin + 5e-4 noise, unequal errors."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, span, n))
    t[0], t[-1] = 0.0, span
    y = 1.0 + 5e-3 * np.sin(2 * np.pi * f_sig * t + rng.uniform(0, 6.0)) + rng.normal(0, 5e-4, n)
    dy = 5e-4 * rng.uniform(0.5, 2.0, n)
    return t, y, dy


def shuffled(tv, seed=7):
    perm = np.random.default_rng(seed).permutation(len(tv[0]))
    return tuple(a[perm] for a in tv)


def pack(arrs):
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return np.concatenate(arrs), off


R1_SPAN = 400.0
R1_SIG = (137.3, 41.7)
# name: (M, log2 Nfft, N1, N2, CT, RT, targets, shuffle the second, dy)
R1_CASES = {
    "2^21": (300000, 21, 2048, 1024, 2, 4, 2, False, False),
    "2^21_shuffled_dy": (300000, 21, 2048, 1024, 2, 4, 2, True, True),
    "2^22": (700000, 22, 2048, 2048, 2, 2, 2, False, False),
    "2^23": (1400000, 23, 4096, 2048, 1, 2, 2, False, False),
    "2^24": (3000000, 24, 4096, 4096, 1, 1, 1, False, False),
}


def r1_df(M):
    return 1e-4 * (3e6 / M)


def r1_targets(name):
    _, _, _, _, _, _, nt, shuf, _ = R1_CASES[name]
    tv = [make_target(2100 + i, n, R1_SPAN, f) for i, (n, f) in enumerate(zip((3000, 700), R1_SIG))][:nt]
    if shuf:
        tv[1] = shuffled(tv[1])
    return tv


R2_SHAPES = [(1, 5), (2, 5), (3, 5), (6, 5), (12, 5), (25, 5), (8, 1), (5, 1)]      # (M, oversampling): Nfft = 8 .. 128
R2_DY_SHAPE = (12, 5)                    # the shape that also runs with the target's unequal errors
R2_DF = 0.5


def r2_target():
    return make_target(2200, 50, 10.0, 1.3)


R3_FMAX = 200.0
R3_SPAN_DF = 0.45                       # span * df: 2 span df < 1, the 2 df grid does not wrap
# name: (M, oversampling, log2 Nfft, kb, shuffle the second)
R3_CASES = {
    "2^16_kb10": (40000, 1, 16, 10, False),
    "2^16_kb10_shuffled": (40000, 1, 16, 10, True),
    "2^18_kb13": (200000, 1, 18, 13, False),
    "2^20_kb10": (300000, 2, 20, 10, False),
}


def r3_targets(name):
    M, _, _, _, shuf = R3_CASES[name]
    df = R3_FMAX / M
    tv = [make_target(2300 + i, n, R3_SPAN_DF / df, f) for i, (n, f) in enumerate(zip((3000, 700), (137.3, 41.7)))]
    if shuf:
        tv[1] = shuffled(tv[1])
    return tv, df


# ------------------------------------------------------------------------------------ comparison
def rel_err(got, ref, fr, t, label):
    cond = fr * (t.max() - t.min()) >= 1.0
    assert cond.any()
    assert np.array_equal(np.isfinite(ref[cond]), np.isfinite(got[cond])), label
    ok = cond & np.isfinite(ref)
    err = np.max(np.abs(got[ok] - ref[ok])) / np.max(np.abs(ref[ok]))
    print("%s: rel err %.3e over %d frequencies" % (label, err, ok.sum()))
    return err


def run_peaks_and_compare(tv, f0, df, M, oversampling, use_dy, label, fit_mean=True):
    t, off = pack([a for a, _, _ in tv])
    y, _ = pack([b for _, b, _ in tv])
    dy = pack([c for _, _, c in tv])[0] if use_dy else None
    pw, mx, am = _capi.ls_fast_peaks_batch(t, y, off, dy=dy, f0=f0, df=df, M=M, fit_mean=fit_mean, normalization="psd",
                                           oversampling=oversampling)
    assert pw.shape == (len(tv), M)
    assert np.array_equal(mx, np.nanmax(pw, axis=1))
    assert np.array_equal(am, np.nanargmax(pw, axis=1))
    fr = f0 + df * np.arange(M)
    worst = 0.0
    for b, (tb, yb, eb) in enumerate(tv):
        ref = O.ls_power_fast(tb, yb, eb if use_dy else None, f0, df, M, normalization="psd", fit_mean=fit_mean,
                              oversampling=oversampling)
        worst = max(worst, rel_err(pw[b], ref, fr, tb, "%s target %d" % (label, b)))
    assert worst <= TOL, (label, worst)


def test_cases_are_what_they_claim():
    for name, (M, lg, n1, n2, ct, rt, nt, shuf, _) in R1_CASES.items():
        m, m1, m2 = geometry(M, 5)
        assert (m, 1 << m1, 1 << m2) == (lg, n1, n2) and not reg_path(m1, m2) and m1 > 10, name
        assert generic_tiles(m1, m2) == (ct, rt), name
        assert ((ct << m1) + (1 << m1) // 2 + 1) * 16 > 64 * 1024          # more than the default dynamic LDS: want_lds
        tv = r1_targets(name)
        assert [len(a[0]) for a in tv] == [3000, 700][:nt]
        assert [bool(np.all(np.diff(a[0]) >= 0)) for a in tv] == [True, not shuf][:nt]
        assert all(nowrap(a[0], 1 << m, r1_df(M)) for a in tv)              # "ordered" where sorted, scattered all the same
        assert M * r1_df(M) == pytest.approx(300.0) and max(R1_SIG) < 300.0
    assert {(c[4], c[5]) for c in R1_CASES.values()} == {(2, 4), (2, 2), (1, 2), (1, 1)}
    assert geometry(3355444, 5)[0] == 25
    seen = set()
    for M, ov in R2_SHAPES:
        m, m1, m2 = geometry(M, ov)
        assert 3 <= m <= 7 and m2 < 4 and not reg_path(m1, m2) and (1 << m) >= 8 and (1 << m) == O._bitceil(M * ov)
        seen.add(m)
    assert seen == {3, 4, 5, 6, 7} and R2_DY_SHAPE in R2_SHAPES
    t = r2_target()[0]
    assert R2_DF * (t.max() - t.min()) >= 1.0                               # every frequency is in the compared band
    for name, (M, ov, lg, kb, shuf) in R3_CASES.items():
        m, m1, m2 = geometry(M, ov)
        assert m == lg and reg_path(m1, m2) and m2 >= 8 and 1 <= ov <= 3, name
        assert fused_kb(m1, m2, M) == kb and not rows_power_available(m1, m2, M), name
        tv, df = r3_targets(name)
        assert all(nowrap(a[0], 1 << m, df) and 2.0 * (a[0].max() - a[0].min()) * df < 1.0 for a in tv), name
        assert [bool(np.all(np.diff(a[0]) >= 0)) for a in tv] == [True, not shuf], name
    # the hot route these cases stay off: the bench grid is fused
    m, m1, m2 = geometry(100000, 5)
    assert reg_path(m1, m2) and rows_power_available(m1, m2, 100000)


# ------------------------------------------------------------------------------------ R1
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R1_CASES))
def test_r1_lds_transforms(name):
    M, use_dy = R1_CASES[name][0], R1_CASES[name][8]
    df = r1_df(M)
    run_peaks_and_compare(r1_targets(name), df, df, M, 5, use_dy, "R1 " + name)


@pytest.mark.gpu
def test_r1_two_terms_at_2000_frequencies():
    """fastchi2 at 2^21 (six grids per target): both ends of the spectrum, a stride through it and the injected peak."""
    M = 300000
    df = r1_df(M)
    tv = r1_targets("2^21")
    t, off = pack([a for a, _, _ in tv])
    y, _ = pack([b for _, b, _ in tv])
    pw = _capi.ls_fast_batch(t, y, off, f0=df, df=df, M=M, normalization="psd", nterms=2)
    assert pw.shape == (2, M)
    worst = 0.0
    for b, (tb, yb, _) in enumerate(tv):
        jp = int(round(R1_SIG[b] / df)) - 1
        idx = np.unique(np.concatenate([np.arange(700), np.arange(M - 700, M), np.arange(0, M, M // 590),
                                        np.arange(jp - 5, jp + 6)]))
        assert 1990 <= len(idx) <= 2010 and abs(int(np.nanargmax(pw[b])) - jp) <= 5
        ref = O.ls_power_fastchi2(tb, yb, None, df, df, M, nterms=2, normalization="psd", idx=idx)
        worst = max(worst, rel_err(pw[b][idx], ref, df + df * idx, tb, "R1 2^21 nterms 2 target %d" % b))
    assert worst <= TOL, worst


@pytest.mark.gpu
def test_r1_grid_beyond_2_24_is_refused():
    t, y, _ = r2_target()
    with pytest.raises(ValueError):
        _capi.ls_fast_peaks_batch(t, y, [0, len(t)], f0=1e-4, df=1e-4, M=3355444, oversampling=5)


# ------------------------------------------------------------------------------------ R2
@pytest.mark.gpu
@pytest.mark.parametrize("fit_mean", (True, False))
@pytest.mark.parametrize("M,oversampling,use_dy", [s + (False,) for s in R2_SHAPES] + [R2_DY_SHAPE + (True,)])
def test_r2_tiny_grids(M, oversampling, use_dy, fit_mean):
    tv = r2_target()
    label = "R2 M %d oversampling %d dy %d fit_mean %d" % (M, oversampling, use_dy, fit_mean)
    run_peaks_and_compare([tv], R2_DF, R2_DF, M, oversampling, use_dy, label + " fast", fit_mean=fit_mean)
    t, y, e = tv
    dy = e if use_dy else None
    pw = _capi.ls_fast_batch(t, y, [0, len(t)], dy=dy, f0=R2_DF, df=R2_DF, M=M, fit_mean=fit_mean, normalization="psd",
                             oversampling=oversampling, nterms=2)
    assert pw.shape == (1, M)
    ref = O.ls_power_fastchi2(t, y, dy, R2_DF, R2_DF, M, nterms=2, fit_mean=fit_mean, normalization="psd",
                              oversampling=oversampling)
    err = rel_err(pw[0], ref, R2_DF + R2_DF * np.arange(M), t, label + " nterms 2")
    assert err <= TOL, (label, err)


# ------------------------------------------------------------------------------------ R3
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R3_CASES))
def test_r3_register_path_without_the_fused_row_kernel(name):
    M, ov = R3_CASES[name][:2]
    tv, df = r3_targets(name)
    run_peaks_and_compare(tv, df, df, M, ov, name == "2^18_kb13", "R3 " + name)
