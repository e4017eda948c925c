"""No GPU: the preconditions of tests/test_pld_blocks_gpu.py.  The numpy restatement of the PLD design blocks
(tests/pld_block_cases.py) with numpy's SVD in place of the kernels' eigen-solvers meets the bars the kernels are held to; every
block of every case is conditioned well enough for those bars to speak about the kernel (s[ko-1] / s[0] >= 0.05: below that,
A V / sqrt(lambda) amplifies the rounding of the Gram matrix past the 1e-10 asked of Q^T Q); the first-order and background
blocks have the gap at the cut that the subspace assertion needs; and every case takes the kernel route it was chosen for,
predicted from constants that are read back from pld.hip — a change that moves one of them fails here and says which cases
have to move with it."""
import os
import re

import numpy as np
import pytest

import pld_block_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "lightkurve_amd", "csrc", "pld.hip")) as _f:
    SRC = _f.read()


def _has(pattern):
    return re.search(pattern, SRC) is not None


def test_route_constants_are_those_of_pld_hip():
    """The decisions `pld_block_cases.route` restates, as pld.hip writes them.  If one of these fails, the launcher has changed:
    update the constants in tests/pld_block_cases.py AND move the cases to the new boundaries."""
    assert _has(r"constexpr int kMomentMinCols = %d;" % C.MOMENT_MIN_COLS)
    assert _has(r"const bool moment = Pc >= kMomentMinCols && k1 <= 48;")
    assert _has(r"constexpr int PLD_DIRECT_MAX = %d;" % C.DIRECT_MAX)
    assert _has(r"if \(P >= 3 && P <= PLD_DIRECT_MAX\) \{") and _has(r"if \(P < 3\) \{  // Jacobi")
    assert _has(r"if \(k1 <= %d\) \{\s*if \(o == 2\) LK_MG\(2, 4, 0\); else if \(o == 3\) LK_MG\(3, 4, 0\); else LK_MG\(4, 4, 0\);\s*"
                r"\} else \{\s*if \(o == 2\) LK_MG\(2, 12, 0\); else if \(o == 3\) LK_MG\(3, 12, 0\); else LK_MG\(4, 12, 0\);" % C.PRE_SPLIT)
    assert _has(r"if \(pl\.nfull > 0\)\s*\\\s*hipLaunchKernelGGL\(\(pld_moment_gram_kernel<O, true, PRE, KS>\)")
    assert _has(r"if \(pl\.nwt > pl\.nfull\)\s*\\\s*hipLaunchKernelGGL\(\(pld_moment_gram_kernel<O, false, PRE, KS>\)")
    assert _has(r"if \(\(Pc & 3\) == 0 && Pc >= %d\) \{\s*const int T = \(Pc \+ 63\) / 64;\s*hipLaunchKernelGGL\(pld_moment_expand_sym_kernel"
                % C.SYM_MIN_COLS)
    assert _has(r"float \*G32 = \(Pc > PLD_DIRECT_MAX && \(Pc & 3\) == 0\) \?")
    assert _has(r"static bool pca_f32_ok\(int P, int k\) \{ return P >= %d && \(P \+ 15\) / 16 <= %d && k <= 48; \}"
                % (C.F32_MIN_P, C.F32_MAX_TILES))
    assert _has(r"const bool v4 = \(P & 3\) == 0 && P >= 4;")
    assert _has(r"const int wr = kt <= 1 \? \(o >= 3 \? 4 : 2\) : 1;")
    assert _has(r"#define LK_PPO\(O\) do \{ if \(kt <= 1\) LK_PP\(O, 1, \(O >= 3 \? 4 : 2\)\); else if \(kt == 2\) LK_PP\(O, 2, 1\); "
                r"else LK_PP\(O, 3, 1\); \} while \(0\)")
    assert _has(r"LK_REQUIRE\(pmax <= %d," % C.MAX_COLS)
    # the largest pixel block of the float32-source route, and the first beyond it
    assert C.pixel_route(144, 8)["gram"] == "f32src" and C.pixel_route(145, 8)["gram"] == "ratio"


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.name)
def test_case_takes_the_route_it_was_chosen_for(case):
    bl = C.blocks(case)
    assert all(b.Pc <= C.MAX_COLS for b in bl)
    for i, want in case.expect.items():
        got = C.route(case, bl[i])
        assert {k: got.get(k) for k in want} == want, (case.name, i, got)


def test_cases_sit_on_both_sides_of_every_boundary():
    prod = {c.name: [C.route(c, b) for b in C.blocks(c) if b.kind == "product"] for c in C.ROUTE_CASES}
    allr = [r for rs in prod.values() for r in rs]
    widths = sorted(b.Pc for c in C.ROUTE_CASES for b in C.blocks(c) if b.kind == "product")
    assert max(w for w in widths if w < C.MOMENT_MIN_COLS) == 91 and min(w for w in widths if w >= C.MOMENT_MIN_COLS) == 105
    assert 136 in widths and 153 in widths and 4060 in widths           # direct / iteration; the widest block admitted
    moment = [r for r in allr if r["gram"] == "moment"]
    assert {r["O"] for r in moment} == {2, 3, 4}
    assert {r["PRE"] for r in moment} == {4, 12} and {r["expand"] for r in moment} == {"plain", "sym"}
    assert {(r["KT"], r["WR"]) for r in moment} == {(1, 2), (1, 4), (2, 1), (3, 1)}
    assert {r["G32"] for r in moment if r["solver"] == "subspace"} == {True, False}
    assert any(r["FULL"] for r in moment) and any(not r["FULL"] for r in moment) and all(r["MASKED"] for r in moment)
    assert {r["solver"] for r in allr} == {"jacobi", "direct", "subspace"}
    assert {r["VEC4"] for r in allr if r["gram"] == "products"} == {True, False}
    assert C.ncombos(C.REFUSED.c, C.REFUSED.order) > C.MAX_COLS >= C.ncombos(C.REFUSED.c - 1, C.REFUSED.order)
    pix = {(c.P, C.route(c, C.blocks(c)[0])["gram"], C.route(c, C.blocks(c)[0])["solver"]) for c in C.PIXEL_CASES}
    assert pix == {(3, "ratio", "direct"), (4, "f32src", "direct"), (144, "f32src", "subspace"), (145, "ratio", "subspace"),
                   (148, "ratio", "subspace")}
    assert {c.normalize for c in C.PIXEL_CASES} == {True, False}
    # cadence tails around the 64-cadence stage of each WR
    assert {C.route(c, C.blocks(c)[-2])["WR"] for c in C.TAIL_BASES} == {1, 2, 4}
    assert {c.N for c in C.TAIL_CASES} == {50, 64, 65, 127, 129, 255, 257}


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.name)
def test_restatement_meets_its_own_bars(case):
    """Bars 1-4 (and 5 where there is a gap) with the SVD's basis; the conditioning floor and, for the first-order and
    background blocks, the gap at the cut, in both cutouts of the batch."""
    for b in range(2):
        cut = C.cutout(case, b)
        X = C.reference_design(case, cut)
        assert X.shape[1] + C.N_INNER + C.DEGREE + 2 == C.design_width(case)
        for blk, S, unc in C.sources(case, cut, X):
            fig = C.check_block(case, blk, X[:, blk.col0:blk.col0 + blk.ko], S, unc, tol=1e-10, label="%s[%d]" % (case.name, b))
            assert fig["floor"] >= C.FLOOR, (case.name, b, blk, fig["floor"])
            if blk.kind != "product":
                assert fig["gap"] > C.GAP and fig["subspace"] is not None, (case.name, b, blk, fig["gap"])
        ps = C.prior_reference(case, cut["flux"])
        assert ps.shape == (C.design_width(case),) and ps[0] * case.c == pytest.approx(ps[-1], rel=1e-15)


def test_normalised_background_rows_are_exact_in_float32():
    """Integer pixels with row sums below 2^24: any summation order gives the same float32 divisor."""
    cut = C.cutout(C.PIXEL_CASES[-2], 0)
    bkg = cut["bkg"]
    assert np.array_equal(bkg, np.rint(bkg)) and bkg.sum(axis=1, dtype=np.float64).max() < 2 ** 24
    fwd = np.add.reduce(bkg, axis=1, dtype=np.float32)
    rev = np.add.reduce(bkg[:, ::-1], axis=1, dtype=np.float32)
    assert np.array_equal(fwd, rev) and np.array_equal(fwd.astype(np.float64), bkg.astype(np.float64).sum(axis=1))
