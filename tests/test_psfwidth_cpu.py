"""CPU: the numpy mirror PixelCube.psf_width (the definition of the fit of the PSF width per cutout) on the scenes of
tests/psfwidth_cases.py — against an independent joint least-squares fit, its derivative tables against finite differences,
its pulls against the truth — and the preconditions under which test_psfwidth_gpu.py may compare statuses and iteration counts
exactly: no decision of a compared cutout hangs on rounding."""
import numpy as np
import pytest

import psfwidth_cases as C
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.correctors.pldcorrector import _psf_width_tables

IDS = lambda c: "%dx%d-S%d-N%d-%s%s%s%s" % (c[0] + c[1:4] + ("" if c[4] else "-unshifted", "-masks" if c[5] else "", "" if c[6] else "-unweighted"))


def parameters(setting):
    p = dict(C.DEFAULTS)
    p.update(C.SETTINGS[setting])
    return p


def test_against_a_joint_least_squares_fit():
    """The variable projection against scipy.optimize.least_squares over all theta_n and the two widths at once (tolerances
    1e-14), on a small clean cutout: (5, 7), S = 2, N = 8, the mirror with tol = 1e-10.  The two minimise the same sum, so they
    agree to where scipy stops.  Measured here: max |sigma_mirror - sigma_joint| = 9.2e-10 px; the bound is ten times that
    rounded up to one digit, 1e-8 px (never more than 1e-6 px, three orders below the statistical error of 9e-3 px)."""
    sc = C.scene((5, 7), 2, 8)
    kw = C.cutout_arguments(sc, 0, False)
    r = PixelCube(sc["time"][0], sc["flux"][0], sc["err"][0]).psf_width(tol=1e-10, **kw)
    assert r["status"] == 0 and r["n_cadences"] == 8
    theta0 = np.concatenate([sc["true_flux"][0].T, np.full((8, 1), sc["true_bkg"][0])], axis=1)
    sg, _ = C.reference_fit(sc["flux"][0], sc["err"][0], sc["star_col"][0], sc["star_row"][0], kw["shifts"], sc["sigma"][0], theta0)
    d = np.max(np.abs(r["sigma"] - sg))
    print("max |sigma_mirror - sigma_joint| = %.3g px (sigma %s, sigma_err %s)" % (d, r["sigma"], r["sigma_err"]))
    assert d < BOUND_JOINT <= 1e-6


BOUND_JOINT = 1e-8


def test_derivative_tables_equal_finite_differences():
    """d(factor)/d(sigma) of the tables against central differences of the factor table (h = 1e-5 px: truncation ~ h^2 f''' / 6
    ~ 1e-10, rounding ~ 1e-16 / h = 1e-11) within 1e-7 of the largest derivative, at the widths and centres the scenes use."""
    rng = np.random.default_rng(5)
    h, worst = 1e-5, 0.0
    for sg in (0.2, 0.8, 1.1, 1.3, 5.0):
        for n in (3, 7, 17, 33):
            c = rng.uniform(-1.0, n, (3, 4))
            val, der = _psf_width_tables(c, sg, n)
            fd = (_psf_width_tables(c, sg + h, n)[0] - _psf_width_tables(c, sg - h, n)[0]) / (2 * h)
            assert val.shape == der.shape == (3, 4, n)
            worst = max(worst, np.max(np.abs(der - fd)) / np.max(np.abs(der)))
    print("largest |table - finite difference| / max |table| = %.3g" % worst)
    assert worst < 1e-7


def test_pulls_of_the_fitted_widths():
    """40 clean cutouts of (11, 11), S = 4, N = 33 with different seeds: all have status 0 and the 80 pulls (sigma - truth) /
    sigma_err have an rms in [0.7, 1.3] (+-3.8 of the rms's own standard error 1 / sqrt(160))."""
    pulls = []
    for seed in range(40):
        c = C.clean_cutout(seed)
        r = PixelCube(c["time"], c["flux"], c["err"]).psf_width(**c["kw"])
        assert r["status"] == 0, seed
        pulls.append((r["sigma"] - c["sigma"]) / r["sigma_err"])
    pulls = np.concatenate(pulls)
    rms = np.sqrt(np.mean(pulls ** 2))
    print("%d pulls: rms %.4f, largest |pull| %.2f" % (len(pulls), rms, np.max(np.abs(pulls))))
    assert len(pulls) == 80 and np.all(np.isfinite(pulls)) and 0.7 <= rms <= 1.3


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_no_decision_of_a_compared_cutout_hangs_on_rounding(case):
    """The preconditions of the exact comparisons on the device, on every compared case: no step within 0.1 % of tol, no
    unclamped step component within 0.1 % of max_step, no visited width within 0.1 % of a bound, no pivot ratio between 1e-14
    and 1e-9 (the singular cadences of cutout 3 sit at rounding level, below), and a contractive iteration: each step after
    the first is below half the one before it while that is above 1e-10 (steps that were clamped, and the one after a clamped
    step, are exempt: the clamp holds them at max_step on purpose)."""
    p = parameters(case[3])
    for b, r in enumerate(C.mirror(*case)):
        steps, raw, vis = r["steps"][:r["n_iter"]], np.abs(r["raw_steps"][:r["n_iter"]]), r["visited"][:r["n_iter"]]
        assert np.all(np.isfinite(steps)) and np.all(np.isfinite(raw)) and np.all(np.isfinite(vis)), (case, b)
        if p["tol"] > 0:
            assert not np.any(np.abs(steps / p["tol"] - 1.0) < 1e-3), (case, b)
        assert not np.any(np.abs(raw / p["max_step"] - 1.0) < 1e-3), (case, b)
        for bound in (p["min_sigma"], p["max_sigma"]):
            assert not np.any(np.abs(vis / bound - 1.0) < 1e-3), (case, b)
        ratio = r["min_pivot_ratio"]
        assert not 1e-14 < ratio < 1e-9, (case, b, ratio)
        clamped = np.any(raw > p["max_step"], axis=1)
        for i in range(1, len(steps)):
            if steps[i - 1] > 1e-10 and not clamped[i] and not clamped[i - 1]:
                assert steps[i] < 0.5 * steps[i - 1], (case, b, steps)


def test_every_status_arises_where_it_is_meant_to():
    N = C.N_MAIN
    DROPPED = len(range(1, N, 3))                             # cadence_mask[1, 1::3] = False
    sc = C.scene((5, 7), 2, N)
    assert np.isnan(sc["flux"][1]).any() and np.isnan(sc["flux"][1, N // 2]).all() and np.isnan(sc["time"][1]).sum() == 1
    e = sc["err"][1]
    assert (e == 0).any() and np.isnan(e).any() and np.isinf(e).any() and not sc["mask"][1].all()
    assert np.isnan(sc["shifts"][0][1]).sum() == 1 and np.isnan(sc["star_col"][2, 0]) and np.isnan(sc["star_col"][2]).sum() == 1
    assert sc["star_col"][3, 0] == sc["star_col"][3, 1] and (~sc["cadence_mask"][1]).sum() == DROPPED and sc["cadence_mask"][[0, 2, 3]].all()
    assert np.all((sc["sigma"] >= 0.8) & (sc["sigma"] <= 1.3)) and np.all(np.abs(sc["sigma0"] / sc["sigma"] - 1.0) <= 0.15 + 1e-12)
    for shape, S in C.SHAPES:
        refs = C.mirror(shape, S, N)
        r = refs[0]
        assert r["status"] == 0 and (r["cadence_status"] == 0).all() and r["n_cadences"] == N and r["n_pixels"] == N * shape[0] * shape[1]
        assert np.isfinite(r["trace"][:r["n_iter"] + 1]).all() and np.isnan(r["trace"][r["n_iter"] + 1:]).all()
        assert np.array_equal(r["trace"][0], sc["sigma0"][0]) and np.array_equal(r["trace"][r["n_iter"]], r["sigma"])
        assert np.max(np.abs(r["sigma"] - sc["sigma"][0]) / r["sigma_err"]) < 5, (shape, S)
        st = refs[1]["cadence_status"]
        assert refs[1]["status"] == 0 and (st == 6).sum() == DROPPED and (st == 1).sum() == 1 and (st == 2).sum() == 1, (shape, S, st)
        assert set(st.tolist()) == {0, 1, 2, 6} and refs[1]["n_cadences"] == (st == 0).sum()
        assert refs[1]["n_pixels"] == refs[1]["n_used"][st == 0].sum()
        if S >= 2:
            assert refs[2]["status"] == 0 and refs[2]["star_index"].tolist() == list(range(1, S))
            r = refs[3]
            assert r["status"] == 1 and (r["cadence_status"] == 3).all() and r["n_iter"] == 0 and np.isnan(r["last_step"])
            assert np.isnan(r["sigma"]).all() and np.isnan(r["chi2"]) and r["n_cadences"] == 0 and r["n_pixels"] == 0
            assert np.array_equal(r["trace"][0], C.scene(shape, S, N)["sigma0"][3]) and np.isnan(r["trace"][1:]).all()
    for shape, S in (((5, 7), 2), ((11, 11), 4)):
        full = C.mirror(shape, S, N)
        fixed, short, bounded, clamped = (C.mirror(shape, S, N, k, True, k != "fixed") for k in ("fixed", "short", "bounded", "clamped"))
        for b in range(3):
            assert fixed[b]["status"] == 0 and fixed[b]["n_iter"] == 6 and np.isfinite(fixed[b]["trace"]).all()
            r = short[b]
            assert r["status"] == 4 and r["n_iter"] == 2 and np.isnan(r["sigma"]).all() and np.isnan(r["sigma_err"]).all()
            assert np.isnan(r["sigma_cov"]) and np.isnan(r["chi2"]) and np.isfinite(r["last_step"])
            assert np.isfinite(r["trace"][:2]).all() and np.isnan(r["trace"][2:]).all()
            r = clamped[b]
            assert r["status"] == 0 and np.all(r["steps"][np.any(np.abs(r["raw_steps"]) > 0.02, axis=1)] == 0.02)
            assert (np.abs(r["raw_steps"][0]) > 0.02).any() and r["n_iter"] > full[b]["n_iter"]
            assert np.max(np.abs(r["sigma"] - full[b]["sigma"])) < 1e-6
        r = bounded[1]
        assert r["status"] == 5 and r["n_iter"] == 1 and np.isnan(r["sigma"]).all() and r["visited"][0].max() > 1.24
        assert np.isfinite(r["trace"][0]).all() and np.isnan(r["trace"][1:]).all() and r["n_cadences"] > 0
        assert bounded[0]["status"] == 0 and bounded[2]["status"] == 0


def test_a_subset_of_cadences_gives_a_consistent_width():
    """cadence_mask: every tenth cadence of the clean cutout gives a width within 5 sigma_err of the one from all cadences, a
    sqrt(10) larger error within 30 %, and the cadences left out have status 6."""
    sc = C.scene((5, 7), 2, C.N_LONG[1])
    cube, kw = PixelCube(sc["time"][0], sc["flux"][0], sc["err"][0]), C.cutout_arguments(sc, 0, False)
    sel = np.arange(C.N_LONG[1]) % 10 == 0
    full, tenth = cube.psf_width(**kw), cube.psf_width(**dict(kw, cadence_mask=sel))
    assert full["status"] == 0 and tenth["status"] == 0 and tenth["n_cadences"] == sel.sum()
    assert np.array_equal(tenth["cadence_status"], np.where(sel, 0, 6))
    assert np.all(np.abs(tenth["sigma"] - full["sigma"]) < 5 * tenth["sigma_err"])
    assert np.all(np.abs(tenth["sigma_err"] / full["sigma_err"] / np.sqrt(len(sel) / sel.sum()) - 1.0) < 0.3)


def test_arguments_are_checked():
    sc = C.scene((5, 7), 2, 1)
    cube = PixelCube(sc["time"][0], sc["flux"][0], sc["err"][0])
    good = dict(C.cutout_arguments(sc, 0, False), sigma0=1.0)
    assert cube.psf_width(**good)["status"] == 0
    for kw in (dict(max_iter=0), dict(max_iter=65), dict(max_iter=2.5), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf), dict(max_step=0.0),
               dict(max_step=-0.1), dict(max_step=np.nan), dict(min_sigma=0.0), dict(min_sigma=-1.0), dict(min_sigma=np.nan),
               dict(max_sigma=np.inf), dict(max_sigma=np.nan), dict(min_sigma=1.01), dict(max_sigma=0.99), dict(sigma0=(1.0, 5.5)),
               dict(sigma0=0.0), dict(sigma0=np.nan), dict(star_col=[np.nan, np.nan]), dict(shifts=(np.zeros(2), np.zeros(2))),
               dict(shifts=(np.zeros(1),)), dict(cadence_mask=np.ones(2, dtype=bool)), dict(cadence_mask=np.ones(1)),
               dict(star_col=np.full(9, 101.0), star_row=np.full(9, 201.0))):
        with pytest.raises(ValueError):
            cube.psf_width(**dict(good, **kw))
