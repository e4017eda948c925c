"""The arithmetic the fast Lomb-Scargle kernels leave out because its result is known in advance: the row kernel
(fft_rows512_power_kernel) forms only the outputs kb = 2 q + e that M reaches, the column kernel (fft_cols_pruned_kernel)
skips the upper half of its input when rows_used <= P / 2.  Every edge of both decisions, against a reference built HERE
from oracle.np_oracle._trig_sum_fft(..., oversampling=o) and the closed form of astropy's fast_impl (restated below), never
against another path of the library.  Tolerance (the parity tests'): 1e-9 of the target's maximum power, identical NaN
pattern, equal argmax; the returned peaks are np.nanmax / the first np.nanargmax of the returned powers, bit for bit.
All frequencies are >= 1 / span (below it the closed form cancels and 1e-9 is not the reference's own precision)."""
import numpy as np
import pytest

from lightkurve_amd import _capi
from oracle import np_oracle as O

TOL = 1e-9
NFFT18 = 1 << 18


def bitceil(n):
    return 1 << int(np.ceil(np.log2(n)))


def make_target(seed, n, span, f_sig):
    """n irregular sorted cadences on [0, span] (both ends sampled), a sinusoid well above the noise."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, span, n))
    t[0], t[-1] = 0.0, span
    y = 1.0 + 5e-3 * np.sin(2 * np.pi * f_sig * t + rng.uniform(0, 6.0)) + rng.normal(0, 5e-4, n)
    return t, y


def ref_power(t, y, f0, df, M, oversampling):
    """astropy fast_impl.py:74-135 (fit_mean, center_data, no dy, psd normalisation) on f0 + df arange(M)."""
    w = np.full(len(t), 1.0 / len(t))
    y = y - np.dot(w, y)
    kw = dict(oversampling=oversampling)
    Sh, Ch = O._trig_sum_fft(t, w * y, df, M, f0, **kw)
    S2, C2 = O._trig_sum_fft(t, w, df, M, f0, freq_factor=2, **kw)
    S, C = O._trig_sum_fft(t, w, df, M, f0, **kw)
    tan2 = (S2 - 2 * S * C) / (C2 - (C * C - S * S))
    S2w = tan2 / np.sqrt(1 + tan2 * tan2)
    C2w = 1 / np.sqrt(1 + tan2 * tan2)
    Cw = np.sqrt(0.5) * np.sqrt(1 + C2w)
    Sw = np.sqrt(0.5) * np.sign(S2w) * np.sqrt(1 - C2w)
    YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
    CC = 0.5 * (1 + C2 * C2w + S2 * S2w) - (C * Cw + S * Sw) ** 2
    SS = 0.5 * (1 - C2 * C2w - S2 * S2w) - (S * Cw - C * Sw) ** 2
    return (YC * YC / CC + YS * YS / SS) * 0.5 * len(t)


def rows_used(t, nfft, df, n2=512):
    """lsf_prep_kernel's count of sample-bearing rows of the grids (df, df, 2 df)."""
    span = (t.max() - t.min()) * nfft * df
    return [int((span * k + 4.0) / n2) + 1 for k in (1.0, 1.0, 2.0)]


def pack(ts, ys):
    off = np.zeros(len(ts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in ts])
    return np.concatenate(ts), np.concatenate(ys), off


def check(ts, ys, f0, df, M, oversampling, t_call=None, t_ref=None, **kw):
    """One library call on the batch; every target against the reference, the peaks against the returned powers."""
    t, y, off = pack(ts if t_call is None else t_call, ys)
    pw, mx, am = _capi.ls_fast_peaks_batch(t, y, off, f0=f0, df=df, M=M, normalization="psd", oversampling=oversampling, **kw)
    assert pw.shape == (len(ts), M)
    assert np.array_equal(mx, np.nanmax(pw, axis=1))
    assert np.array_equal(am, np.nanargmax(pw, axis=1))
    for b, (tt, yy) in enumerate(zip(ts if t_ref is None else t_ref, ys)):
        ref = ref_power(tt, yy, f0, df, M, oversampling)
        ok = np.isfinite(ref)
        assert np.array_equal(ok, np.isfinite(pw[b])), b
        err = np.max(np.abs(pw[b][ok] - ref[ok])) / np.max(np.abs(ref[ok]))
        print("M %d oversampling %d target %d: rel err %.3e" % (M, oversampling, b, err))
        assert err < TOL, (M, oversampling, b, err)
        assert am[b] == np.nanargmax(ref), (M, oversampling, b)


# ------------------------------------------------------------------------------------------------------ row kernel
# Nfft = 2^18 = 512 x 512: the 16 x 32 row kernel, N1 = 512.  Thread (ka, e) keeps kb = 2 q + e; kb_need = ceil(ceil(M / N1) / 16)
ROW_SPAN, ROW_DF, ROW_F0 = 20.0, 0.01, 0.1          # span x df = 0.2: 205 rows on the 2 df grid -> P = 256
ROW_CASES = ([(2100, 64, 1), (65536, 4, 8)]         # (M, oversampling, kb_need): one kb ... all eight
             + [(512 * 16 * j + d, 6, j + (d > 0)) for j in (3, 4, 5) for d in (-1, 0, 1)]      # the 16-row edges
             + [(30000, 6, 4)])                     # the last wanted row of k2 is partial (30000 % 512 = 304)


def row_batch():
    if not hasattr(row_batch, "v"):
        row_batch.v = [make_target(100 + i, n, ROW_SPAN, 7.3 + 11.1 * i) for i, n in enumerate((300, 1103, 2000))]
    return [a for a, _ in row_batch.v], [b for _, b in row_batch.v]


def test_row_cases_are_what_they_claim():
    for M, o, kb_need in ROW_CASES:
        assert bitceil(M * o) == NFFT18, (M, o)
        assert -(-(-(-M // 512)) // 16) == kb_need, (M, o)
    assert any(M % 512 for M, _, _ in ROW_CASES)
    assert bitceil(100000 * 5) == 1 << 19 and -(-(-(-100000 // 1024)) // 16) == 7
    ts, _ = row_batch()
    assert all(rows_used(t, NFFT18, ROW_DF) == [103, 103, 205] for t in ts)


@pytest.mark.gpu
@pytest.mark.parametrize("M,oversampling,kb_need", ROW_CASES)
def test_row_kernel_kept_outputs(M, oversampling, kb_need):
    ts, ys = row_batch()
    check(ts, ys, ROW_F0, ROW_DF, M, oversampling)


@pytest.mark.gpu
def test_row_kernel_bench_shape_two_targets():
    """Nfft = 2^19 = 1024 x 512, M = 1e5: kb_need = 7 — three q in every wave and a fourth in the waves of ka < 4 only."""
    df = 0.005
    tv = [make_target(200 + i, n, 20.0, 3.3 + 40.0 * i) for i, n in enumerate((1500, 1999))]
    ts, ys = [a for a, _ in tv], [b for _, b in tv]
    assert [rows_used(t, 1 << 19, df) for t in ts] == [[103, 103, 205]] * 2
    check(ts, ys, 0.1, df, 100000, 5)


@pytest.mark.gpu
def test_row_kernel_phase_recurrence_when_times_do_not_start_at_zero():
    """t[0] != 0.  Through the rebasing entry (absolute times in, t - t[0] on the device: the reference sees t - t[0]); and
    through the plain entry, where the kernel's own e^{2 pi i t0 f} recurrence (first index ka + 16 e, stride 32 N1) runs
    and the reference applies the same phase in numpy."""
    ts, ys = row_batch()
    M, o = 40000, 6
    t_abs = [t + 1325.25 for t in ts]
    check(ts, ys, ROW_F0, ROW_DF, M, o, t_call=t_abs, t_ref=[t - t[0] for t in t_abs], absolute_time=True)
    t_sh = [t + 3.7 for t in ts]
    check(t_sh, ys, ROW_F0, ROW_DF, M, o)


# --------------------------------------------------------------------------------------------------- column kernel
# rows_used = floor((span + 4) / 512) + 1, span = (t_max - t_min) Nfft df, twice that on the 2 df grid.  P = 2^lp is the batch's
# largest rows_used rounded up; a grid takes the short path when rows_used <= P / 2.  Per lp: a target whose 2 df grid fills
# P rows (its df grids: P / 2, the last short value), one with P / 2 + 1 rows (the first full value), one with P / 2.
COL_DF = 0.01


def col_span(rows2):
    """A time span whose 2 df grid has rows2 sample-bearing rows (the middle of that row count's range)."""
    return (256.0 * (rows2 - 1) + 126.0) / (NFFT18 * COL_DF)


def col_batch(lp):
    P = 1 << lp
    spans = [col_span(P), col_span(P // 2 + 1), col_span(P // 2)]
    f0 = COL_DF * np.ceil(1.05 / min(spans) / COL_DF)
    tv = [make_target(300 + 10 * lp + i, n, s, f0 + 5.03 + 7.7 * i) for i, (n, s) in enumerate(zip((1777, 300, 901), spans))]
    return [a for a, _ in tv], [b for _, b in tv], f0


@pytest.mark.parametrize("lp", [5, 6, 7, 8])
def test_column_batches_sit_on_the_edges(lp):
    P = 1 << lp
    ts, _, f0 = col_batch(lp)
    ru = [rows_used(t, NFFT18, COL_DF) for t in ts]
    assert ru[0] == [P // 2, P // 2, P]
    assert ru[1][2] == P // 2 + 1 and ru[2][2] == P // 2
    assert max(5, int(np.ceil(np.log2(max(max(r) for r in ru))))) == lp      # the launcher's choice of P
    assert all(2.0 * (t[-1] - t[0]) * NFFT18 * COL_DF < NFFT18 - 8.0 for t in ts)     # no wrap: the fused extirpolation
    assert all(f0 * (t[-1] - t[0]) >= 1.0 for t in ts)


@pytest.mark.gpu
@pytest.mark.parametrize("lp", [5, 6, 7, 8])
def test_column_kernel_short_and_full_inputs(lp):
    ts, ys, f0 = col_batch(lp)
    check(ts, ys, f0, COL_DF, 40000, 6)
