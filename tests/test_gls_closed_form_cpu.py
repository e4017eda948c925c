"""The arithmetic of gls_power_sums_lean (csrc/ls_epilogue.hpp), restated in numpy operation by operation, against the
literal reference expression (astropy fast_impl.py:93-131) evaluated in longdouble — both on the same fp64 trig sums of
seeded random ragged light curves.

On f >= 1 / span (the parity tests' domain) the lean form's error is at most 1e-11 of the target's largest power — two
orders above the 8.6e-14 it measures, two below the parity tests' 1e-9 — and at most 10 x the error of the reference
expression's own fp64 evaluation (1.2e-13).  NaN comes out where the reference's does: tan 2w = 0 / 0 (one cadence with
fit_mean), den = 0 with num != 0 (inf * 0 in the reference), SS = 0 with YS = 0 (f = 0)."""
import numpy as np

LD = np.longdouble


def reference(Sh, Ch, S, C, S2, C2, fit_mean):
    """fast_impl.py:93-131 as written, in the dtype of its inputs (psd normalisation without the constant factor)."""
    one, half, two = Sh.dtype.type(1), Sh.dtype.type(0.5), Sh.dtype.type(2)
    with np.errstate(all="ignore"):
        if fit_mean:
            tan2 = (S2 - two * S * C) / (C2 - (C * C - S * S))
        else:
            tan2 = S2 / C2
        S2w = tan2 / np.sqrt(one + tan2 * tan2)
        C2w = one / np.sqrt(one + tan2 * tan2)
        Cw = np.sqrt(half) * np.sqrt(one + C2w)
        Sw = np.sqrt(half) * np.sign(S2w) * np.sqrt(one - C2w)
        YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
        CC = half * (one + C2 * C2w + S2 * S2w)
        SS = half * (one - C2 * C2w - S2 * S2w)
        if fit_mean:
            CC = CC - (C * Cw + S * Sw) ** 2
            SS = SS - (S * Cw - C * Sw) ** 2
        return YC * YC / CC + YS * YS / SS


def rsqrt(x):
    return 1.0 / np.sqrt(x)             # the host side of rsqrt_refined; the device's is within 2 ulp of it


def lean(Sh, Ch, S, C, S2, C2, fit_mean):
    """gls_power_sums_lean, fp64, the same operations in the same order (a fused multiply-add aside)."""
    with np.errstate(all="ignore"):
        num, den = S2, C2
        if fit_mean:
            num = S2 - 2.0 * S * C
            den = C2 - (C * C - S * S)
        lean_angle = np.fmax(np.abs(num), np.abs(den)) >= 1e-150
        r = rsqrt(num * num + den * den)
        C2w = np.abs(den) * r
        S2w = np.where(den == 0.0, np.nan, np.where(den < 0.0, -num, num) * r)
        tan2 = num / den                                        # where num^2 + den^2 would underflow
        C2w_ref = 1.0 / np.sqrt(1.0 + tan2 * tan2)
        C2w = np.where(lean_angle, C2w, C2w_ref)
        S2w = np.where(lean_angle, S2w, tan2 * C2w_ref)
        u = 0.5 + 0.5 * C2w
        rc = rsqrt(u)
        Cw = u * rc
        Sw = 0.5 * S2w * rc
        YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
        CC = 0.5 * (1.0 + C2 * C2w + S2 * S2w)
        SS = 0.5 * (1.0 - C2 * C2w - S2 * S2w)
        if fit_mean:
            a, b = C * Cw + S * Sw, S * Cw - C * Sw
            CC = CC - a * a
            SS = SS - b * b
        return YC * YC / CC + YS * YS / SS


def trig_sums(seed, nf=200):
    """The six sums of one random ragged light curve at nf frequencies >= 1 / span, as the kernels get them (fp64)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 400))
    span = rng.uniform(5.0, 90.0)
    t = np.sort(rng.uniform(0.0, span, n))
    t -= t[0]
    y = 1.0 + rng.uniform(1e-4, 1e-2) * np.sin(2 * np.pi * rng.uniform(0.1, 5.0) * t) + rng.normal(0, 1e-3, n)
    w = rng.uniform(0.5, 2.0, n) ** -2.0
    w /= w.sum()
    y = y - np.dot(w, y)
    f = np.sort(rng.uniform(1.0 / t[-1], 0.5 * n / t[-1] + 1.0, nf))
    ph = 2 * np.pi * np.outer(f, t)
    s1, c1, s2, c2 = np.sin(ph), np.cos(ph), np.sin(2 * ph), np.cos(2 * ph)
    return s1 @ (w * y), c1 @ (w * y), s1 @ w, c1 @ w, s2 @ w, c2 @ w


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-18


def test_lean_form_against_the_longdouble_reference():
    worst_lean = worst_ref = 0.0
    for fit_mean in (True, False):
        for seed in range(60):
            sums = trig_sums(seed)
            truth = reference(*[a.astype(LD) for a in sums], fit_mean)
            top = float(np.max(np.abs(truth)))
            got = lean(*sums, fit_mean)
            ref64 = reference(*sums, fit_mean)
            assert np.all(np.isfinite(truth)) and np.all(np.isfinite(got))
            e_lean = float(np.max(np.abs(got.astype(LD) - truth))) / top
            e_ref = float(np.max(np.abs(ref64.astype(LD) - truth))) / top
            assert e_lean <= 1e-11, (fit_mean, seed, e_lean)
            worst_lean, worst_ref = max(worst_lean, e_lean), max(worst_ref, e_ref)
    print("largest error / largest power: lean %.2e, reference in fp64 %.2e" % (worst_lean, worst_ref))
    assert worst_lean <= 10.0 * worst_ref


def one(*v):
    return [np.array([x], dtype=np.float64) for x in v]


def test_nan_one_cadence_with_fit_mean():
    # one cadence at t = 0, weight 1, centred flux 0: S = S2 = 0, C = C2 = 1 at every frequency -> tan 2w = 0 / 0
    sums = one(0.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    assert np.isnan(reference(*[a.astype(LD) for a in sums], True)[0])
    assert np.isnan(reference(*sums, True)[0]) and np.isnan(lean(*sums, True)[0])


def test_nan_den_zero_num_nonzero():
    for num in (0.3, -0.3):
        sums = one(0.01, 0.02, 0.0, 0.0, num, 0.0)
        assert np.isnan(reference(*sums, False)[0]) and np.isnan(lean(*sums, False)[0])


def test_nan_ss_zero_at_f_zero():
    # f = 0 without fit_mean: S2 = 0, C2 = 1 -> w = 0, SS = 0 and YS = 0: 0 / 0
    sums = one(0.0, 0.01, 0.0, 1.0, 0.0, 1.0)
    assert np.isnan(reference(*sums, False)[0]) and np.isnan(lean(*sums, False)[0])


def test_underflowing_angle_takes_the_reference_expression():
    for num, den in ((3e-160, 4e-160), (-3e-170, 4e-155), (2e-151, -1e-200)):
        sums = one(0.01, 0.02, 0.0, 0.0, num, den)
        got, ref = lean(*sums, False)[0], reference(*sums, False)[0]
        assert np.isfinite(ref) and abs(got - ref) <= 1e-14 * abs(ref)
    # just above the threshold the lean angle is used and agrees
    sums = one(0.01, 0.02, 0.0, 0.0, 3e-150, -4e-150)
    got, ref = lean(*sums, False)[0], reference(*sums, False)[0]
    assert np.isfinite(ref) and abs(got - ref) <= 1e-13 * abs(ref)
