"""Shapes, inputs and the numpy restatement behind tests/test_pld_blocks_cpu.py and tests/test_pld_blocks_gpu.py: every PCA
block of lk_pld_design_batch (pld.hip) against numpy, on each side of every boundary between the kernel routes.

Inputs are built so that numpy repeats exactly what the kernels consume:
  * PLD pixels: float32(flux[:, None] * (1 + 0.01 A)), A = Qn diag(sv) Qp^T (the construction of _prescribed_spectrum in
    tests/test_designmatrix_gpu.py): the leading c singular values fall from 1 to 0.2, the others start a decade below.  The
    first column of Qn is the (centred, normalised) shape of the light curve, so the light curve adds no direction of its own.
    The first-order source is float64(pix32 / flux32) - column means: one float32 division, as numpy's float32 / float32.
  * background pixels: the same construction rounded to integers, row sums below 2^24: the float32 row sum is exact in any
    order and pix32 / rowsum32 is one correctly rounded float32 division.  Without normalisation the source is the pixels.
  * order-o product block: products of the first-order columns of the design matrix UNDER TEST (the very doubles the product
    kernels read) in itertools.combinations_with_replacement order, float64, minus their column means.

`route(...)` restates the launcher's decisions (pld_design_launch, pca_block, pca_products_moment, eig_topk, moment_plan);
tests/test_pld_blocks_cpu.py checks it against the constants in pld.hip, and every case against the route it was chosen for.
`check_block` holds the assertions that both test files make of a block."""
import itertools
import math
from collections import namedtuple

import numpy as np

EPS = 2.2e-16
# the constants of pld.hip the cases are aimed at (tests/test_pld_blocks_cpu.py reads them back from the source)
MOMENT_MIN_COLS = 100     # kMomentMinCols
DIRECT_MAX = 138          # PLD_DIRECT_MAX
PRE_SPLIT = 16            # pld_moment_gram_kernel: PRE = 4 for k1 <= 16, 12 above
SYM_MIN_COLS = 128        # pld_moment_expand_sym_kernel: (Pc & 3) == 0 && Pc >= 128
F32_MIN_P, F32_MAX_TILES = 4, 9   # pca_f32_ok: P >= 4 && (P + 15) / 16 <= 9
MAX_COLS = 4096
N_INNER, DEGREE = 6, 3    # spline block: 6 interior knots of degree 3

Case = namedtuple("Case", "name c order N P Pb normalize seed expect")
Block = namedtuple("Block", "kind order Pc ko col0")   # kind: 'first' | 'product' | 'bkg'


def ncombos(k, o):
    return math.comb(k + o - 1, o)


# ------------------------------------------------------------------------------------------------------------- routes
def moment_tiles(k, o):
    """moment_plan of pld.hip: (nwt, nfull) — the wave tiles of the staircase and how many of them the FULL body takes (all 16
    tiles needed, no column-mean duty)."""
    cols = list(itertools.combinations_with_replacement(range(k), o))
    pc = len(cols)
    rperm = sorted(range(pc), key=lambda i: (cols[i][-1], i))
    colstart = [sum(1 for c in cols if c[0] < m) for m in range(k + 2)]
    wt = []
    for r0 in range(0, pc, 64):
        rt = [min((cols[x][-1] for x in rperm[r0 + 16 * i:r0 + 16 * i + 16]), default=None) for i in range(4)]
        mn = min(x for x in rt if x is not None)
        for cg in range((colstart[mn] // 16) * 16, pc, 64):
            mask = 0
            for i in range(4):
                for j in range(4):
                    if rt[i] is not None and cg + 16 * j < pc and cg + 16 * j + 16 > colstart[rt[i]]:
                        mask |= 1 << (4 * i + j)
            if mask:
                wt.append([r0, cg, mask, 0])
    wt.sort(key=lambda w: -bin(w[2]).count("1"))                          # stable, as std::stable_sort
    done = [False] * ((pc + 15) // 16)
    for last_pass in (False, True):                                       # column means: a masked wave tile where there is a choice
        for w in wt:
            for i in range(4):
                r = w[0] // 16 + i
                if (last_pass or w[2] != 0xffff) and (w[2] & (0xf << (4 * i))) and r < len(done) and not done[r]:
                    done[r] = True
                    w[3] |= 1 << i
    return len(wt), sum(1 for w in wt if w[2] == 0xffff and w[3] == 0)


def _solver(P):
    return "jacobi" if P < 3 else ("direct" if P <= DIRECT_MAX else "subspace")


def pixel_route(P, k):
    """pca_block for a first-order or background block of P pixels."""
    f32 = P >= F32_MIN_P and (P + 15) // 16 <= F32_MAX_TILES and k <= 48
    r = dict(gram="f32src" if f32 else "ratio", solver=_solver(P), KT=(k + 15) // 16)
    if not f32:
        r["VEC4"] = P % 4 == 0 and P >= 4
    return r


def product_route(k1, o, c):
    Pc = ncombos(k1, o)
    ko = min(c, Pc)
    if Pc < MOMENT_MIN_COLS:
        return dict(gram="products", solver=_solver(Pc), KT=(ko + 15) // 16, VEC4=Pc % 4 == 0 and Pc >= 4)
    nwt, nfull = moment_tiles(k1, o)
    kt = (ko + 15) // 16
    return dict(gram="moment", O=o, PRE=4 if k1 <= PRE_SPLIT else 12, FULL=nfull > 0, MASKED=nwt > nfull,
                expand="sym" if Pc % 4 == 0 and Pc >= SYM_MIN_COLS else "plain", G32=Pc > DIRECT_MAX and Pc % 4 == 0,
                solver=_solver(Pc), KT=kt, WR=(4 if o >= 3 else 2) if kt <= 1 else 1)


def blocks(case):
    """The PCA blocks of a case's design matrix, in column order."""
    out, col = [], 0
    k1 = min(case.c, case.P) if case.order > 0 else 0
    if k1:
        out.append(Block("first", 1, case.P, k1, 0))
        col = k1
        for o in range(2, case.order + 1):
            Pc = ncombos(k1, o)
            out.append(Block("product", o, Pc, min(case.c, Pc), col))
            col += min(case.c, Pc)
    out.append(Block("bkg", 0, case.Pb, min(case.c, case.Pb), col))
    return out


def route(case, blk):
    if blk.kind == "product":
        return product_route(min(case.c, case.P), blk.order, case.c)
    return pixel_route(blk.Pc, blk.ko)


def design_width(case):
    return sum(b.ko for b in blocks(case)) + N_INNER + DEGREE + 1 + 1


# -------------------------------------------------------------------------------------------------------------- cases
def _case(name, c, order, N=300, P=None, Pb=None, normalize=True, seed=0, expect=None):
    P = c + 4 if P is None else P
    return Case(name, c, order, N, P, 2 * c + 8 if Pb is None else Pb, normalize, seed, expect or {})


# expect: {block index: the route entries the case exists for}
ROUTE_CASES = [
    _case("c1_o3", 1, 3, expect={0: dict(gram="f32src", solver="direct"), 1: dict(gram="products", solver="jacobi"),
                                 2: dict(gram="products", solver="jacobi")}),
    _case("c2_o3", 2, 3, expect={1: dict(gram="products", solver="direct", VEC4=False),
                                 2: dict(gram="products", solver="direct", VEC4=True)}),
    _case("c13_o2", 13, 2, expect={1: dict(gram="products", solver="direct", VEC4=False, KT=1)}),
    _case("c14_o2", 14, 2, expect={1: dict(gram="moment", O=2, expand="plain", solver="direct", PRE=4, G32=False, KT=1, WR=2)}),
    _case("c16_o2", 16, 2, expect={1: dict(gram="moment", O=2, expand="sym", solver="direct", PRE=4, G32=False, KT=1, WR=2)}),
    _case("c17_o2", 17, 2, expect={1: dict(gram="moment", O=2, expand="plain", solver="subspace", PRE=12, G32=False, KT=2, WR=1)}),
    _case("c33_o2", 33, 2, expect={1: dict(gram="moment", O=2, expand="plain", solver="subspace", PRE=12, G32=False, KT=3, WR=1)}),
    _case("c48_o2", 48, 2, expect={1: dict(gram="moment", O=2, expand="sym", solver="subspace", PRE=12, G32=True, KT=3, WR=1,
                                           FULL=True, MASKED=True)}),
    _case("c7_o3", 7, 3, expect={1: dict(gram="products", solver="direct"), 2: dict(gram="products", solver="direct")}),
    _case("c8_o3", 8, 3, expect={1: dict(gram="products", solver="direct"),
                                 2: dict(gram="moment", O=3, expand="plain", solver="direct", PRE=4, KT=1, WR=4)}),
    _case("c5_o4", 5, 4, expect={1: dict(gram="products"), 2: dict(gram="products"), 3: dict(gram="products", solver="direct")}),
    _case("c6_o4", 6, 4, expect={1: dict(gram="products"), 2: dict(gram="products"),
                                 3: dict(gram="moment", O=4, expand="plain", solver="direct", PRE=4, KT=1, WR=4)}),
    _case("c28_o3_widest", 28, 3, N=200, expect={1: dict(gram="moment", O=2, expand="plain", solver="subspace", G32=False, KT=2),
                                                 2: dict(gram="moment", O=3, expand="sym", solver="subspace", PRE=12, G32=True, KT=2,
                                                         WR=1, FULL=True, MASKED=True)}),
    _case("c16_P5_o2", 16, 2, P=5, expect={0: dict(gram="f32src", solver="direct"), 1: dict(gram="products", solver="direct", KT=1)}),
]
assert [ncombos(28, 3), ncombos(29, 3)] == [4060, 4495]

REFUSED = _case("c29_o3_refused", 29, 3, N=64)            # 4495 product columns > 4096

# first-order and background blocks on the same integer-valued pixels, order 1, c = 8, with and without normalisation
PIXEL_CASES = []
for _P, _exp in ((3, dict(gram="ratio", solver="direct", VEC4=False)), (4, dict(gram="f32src", solver="direct")),
                 (144, dict(gram="f32src", solver="subspace")), (145, dict(gram="ratio", solver="subspace", VEC4=False)),
                 (148, dict(gram="ratio", solver="subspace", VEC4=True))):
    for _norm in (True, False):
        PIXEL_CASES.append(_case("pix_P%d_%s" % (_P, "norm" if _norm else "raw"), 8, 1, P=_P, Pb=_P, normalize=_norm,
                                 expect={0: _exp, 1: _exp}))

TAIL_N = (50, 64, 65, 127, 129, 255, 257)
TAIL_BASES = [c for c in ROUTE_CASES if c.name in ("c14_o2", "c8_o3", "c17_o2")]     # WR = 2, 4, 1
TAIL_CASES = [b._replace(name="%s_N%d" % (b.name, n), N=n) for b in TAIL_BASES for n in TAIL_N]

INDEPENDENCE = _case("c16_o3_N257", 16, 3, N=257)

ALL_CASES = ROUTE_CASES + PIXEL_CASES + TAIL_CASES + [INDEPENDENCE]


# ------------------------------------------------------------------------------------------------------------- inputs
def _smooth(N):
    return np.sin(np.linspace(0.0, 20.0, N))


def _spectrum_matrix(N, P, c, rng):
    """A = Qn diag(sv) Qp^T; the first column of Qn is the centred light-curve shape."""
    r = min(N, P)
    k = min(c, r)
    sv = np.concatenate([np.geomspace(1.0, 0.2, k), np.geomspace(0.02, 1e-4, r - k)])
    shape = _smooth(N) - _smooth(N).mean()
    Qn = np.linalg.qr(np.column_stack([shape, rng.normal(size=(N, r - 1))]) if r > 1 else shape[:, None])[0]
    Qp = np.linalg.qr(rng.normal(size=(P, r)))[0]
    return (Qn * sv) @ Qp.T


def _integer_pixels(N, P, c, rng):
    """Integer-valued float32 pixels about 1e5 with row sums below 2^24 (P <= 148), on a light curve that varies by 1e-4."""
    flux = 1.0e5 * (1.0 + 1.0e-4 * _smooth(N))
    pix = np.rint(flux[:, None] * (1.0 + 0.01 * _spectrum_matrix(N, P, c, rng)))
    assert pix.sum(axis=1).max() < 2 ** 24 and pix.min() > 0
    return pix.astype(np.float32), flux.astype(np.float32)


def cutout(case, b):
    """Cutout b of a case: dict(pix, bkg, flux (float32), time, knots).  Pixel-route cases share one integer-valued pixel
    array between the two blocks; the others have float pixels on a light curve of 2 % amplitude and their own background."""
    rng = np.random.default_rng(1000 * case.seed + 7919 * b + 31 * case.c + case.P + 17 * case.N)
    N = case.N
    if case.name.startswith("pix_"):
        pix, flux = _integer_pixels(N, case.P, case.c, rng)
        bkg = pix
    else:
        f64 = 1000.0 * (1.0 + 0.02 * _smooth(N))
        flux = f64.astype(np.float32)
        pix = (f64[:, None] * (1.0 + 0.01 * _spectrum_matrix(N, case.P, case.c, rng))).astype(np.float32)
        bkg, _ = _integer_pixels(N, case.Pb, case.c, rng)
    t = np.linspace(0.0, 30.0, N)
    knots = np.concatenate([[t.min()], np.percentile(t, np.linspace(0, 100, N_INNER + 2)[1:-1]), [t.max()]])
    return dict(pix=pix, bkg=bkg, flux=flux, time=t, knots=knots)


def batch(case, B=2):
    cs = [cutout(case, b) for b in range(B)]
    return {k: np.stack([c[k] for c in cs]) for k in cs[0]}


# -------------------------------------------------------------------------------------------------------- restatement
def first_source(pix32, flux32):
    unc = (pix32 / flux32[:, None]).astype(np.float64)                    # float32 division
    return unc - unc.mean(axis=0), unc


def bkg_source(bkg32, normalize):
    if normalize:
        rs = bkg32.sum(axis=1, dtype=np.float32)                         # exact: integers, sums below 2^24
        assert np.array_equal(rs.astype(np.float64), bkg32.astype(np.float64).sum(axis=1))
        unc = (bkg32 / rs[:, None]).astype(np.float64)
    else:
        unc = bkg32.astype(np.float64)
    return unc - unc.mean(axis=0), unc


def product_source(U1, o):
    idx = list(itertools.combinations_with_replacement(range(U1.shape[1]), o))
    unc = np.stack([np.prod(U1[:, list(t)], axis=1) for t in idx], axis=1)
    return unc - unc.mean(axis=0), unc


def sources(case, cut, X):
    """(block, S, S_unc) for every PCA block; the product blocks are formed from the first-order columns of X."""
    out = []
    for blk in blocks(case):
        if blk.kind == "first":
            S, unc = first_source(cut["pix"], cut["flux"])
        elif blk.kind == "product":
            S, unc = product_source(X[:, :min(case.c, case.P)], blk.order)
        else:
            S, unc = bkg_source(cut["bkg"], case.normalize)
        out.append((blk, S, unc))
    return out


def reference_design(case, cut):
    """The PCA blocks with numpy's SVD in place of the kernels' eigen-solvers (N x sum(ko)); the products are formed from the
    SVD's own first-order block."""
    X = np.zeros((case.N, sum(b.ko for b in blocks(case))))
    for blk in blocks(case):
        if blk.kind == "first":
            S = first_source(cut["pix"], cut["flux"])[0]
        elif blk.kind == "product":
            S = product_source(X[:, :min(case.c, case.P)], blk.order)[0]
        else:
            S = bkg_source(cut["bkg"], case.normalize)[0]
        X[:, blk.col0:blk.col0 + blk.ko] = np.linalg.svd(S, full_matrices=False)[0][:, :blk.ko]
    return X


def prior_reference(case, flux32):
    sd = 10.0 * float(np.float32(np.nanstd(flux32.astype(np.float64))))
    ps = np.full(design_width(case), sd)
    bl = blocks(case)
    ps[:bl[-1].col0] = sd / case.c                                       # the PLD columns; background, spline and constant keep sd
    return ps


def defined_columns(case, blk):
    """Columns of a block that the data determine.  A NORMALISED background block of Pb <= pca_components pixels has rows
    that sum to 1: the centred source has rank Pb - 1 and its last requested component is the quotient of two rounding
    errors — in the reference (fbpca) as here (include/lkhip.h, lk_pld_design_batch).  It is left out of the assertions."""
    if blk.kind == "bkg" and case.normalize and blk.ko == blk.Pc:
        return blk.ko - 1
    return blk.ko


# --------------------------------------------------------------------------------------------------------- assertions
ORTHO_BAR, RANGE_BAR, VAR_BAR, SUBSPACE_BAR, GAP, FLOOR, PROJECT_BAR = 1e-10, 1e-9, 1e-5, 1e-6, 0.05, 0.05, 1e-8


def backward_bar(blk, rt, N, s0, unc_norm, tol):
    """Relative bar of ||G Q - Q (Q^T G Q)||_F / (s0^2 sqrt(ko)) and the derived figure behind it (None for the iteration).
    Subspace iteration: the project's bars, 1e-6 at the default stop criterion and 1e-8 at 1e-10.  Direct solvers have no
    tolerance; what is left is the formation of the Gram matrix in float64:
      * product blocks: 10 (N + Pc) eps ||S_unc||_2^2 — the uncentred norm, because the moment form subtracts N mu mu^T;
      * pixel blocks are centred BEFORE the Gram matrix: (N + Pc) eps s0^2 for the products, and a column mean off by at most
        N eps |mu_j| moves S by 1 dmu^T, ||.||_2 <= N eps ||S_unc||_2 (1 mu^T is a projection of S_unc), hence G by at most
        2 s0 N eps ||S_unc||_2: 10 (N + Pc) eps s0 (s0 + ||S_unc||_2), capped at the project's 1e-8."""
    if rt["solver"] == "subspace":
        return (1e-6 if tol == 0.0 else 1e-8), None
    if blk.kind == "product":
        derived = 10.0 * (N + blk.Pc) * EPS * unc_norm ** 2 / s0 ** 2
        assert derived <= PROJECT_BAR, ("derived bar above the project's 1e-8", derived)
        return derived, derived
    derived = 10.0 * (N + blk.Pc) * EPS * (s0 + unc_norm) / s0
    return min(derived, PROJECT_BAR), derived


def check_block(case, blk, Q, S, unc, tol=0.0, label=""):
    """Assertions 1-5 on the ko columns Q of one block.  Every figure is measured and printed before anything is asserted, and a
    failure names all the assertions the block misses; returns the figures."""
    N = case.N
    rt = route(case, blk)
    ko = defined_columns(case, blk)
    Q = Q[:, :ko]
    Us, s, _ = np.linalg.svd(S, full_matrices=False)
    s0 = s[0]
    fig = dict(label=label, kind=blk.kind, order=blk.order, Pc=blk.Pc, ko=ko, solver=rt["solver"], gram=rt["gram"], tol=tol)
    fig["floor"] = s[ko - 1] / s0
    failed = []
    # 1 orthonormal columns
    fig["ortho"] = np.max(np.abs(Q.T @ Q - np.eye(ko)))
    if not fig["ortho"] < ORTHO_BAR:
        failed.append(("orthonormality", fig["ortho"], ORTHO_BAR))
    # 2 range
    Ur = Us[:, s > 1e-12 * s0]
    fig["range"] = np.linalg.norm(Q - Ur @ (Ur.T @ Q)) / np.sqrt(ko)
    if not fig["range"] <= RANGE_BAR:
        failed.append(("range", fig["range"], RANGE_BAR))
    # 3 backward error
    G = S @ S.T
    GQ = G @ Q
    H = Q.T @ GQ
    fig["backward"] = np.linalg.norm(GQ - Q @ H) / (s0 ** 2 * np.sqrt(ko))
    fig["bar"], fig["derived"] = backward_bar(blk, rt, N, s0, np.linalg.norm(unc, 2), tol)
    if not fig["backward"] <= fig["bar"]:
        failed.append(("backward error", fig["backward"], fig["bar"]))
    # 4 captured variance
    fig["variance"] = 1.0 - np.trace(H) / np.sum(s[:ko] ** 2)
    if not fig["variance"] <= VAR_BAR:
        failed.append(("captured variance", fig["variance"], VAR_BAR))
    # 5 subspace, where the reference has a gap at the cut
    s_next = s[ko] if ko < len(s) else 0.0
    fig["gap"] = (s[ko - 1] - s_next) / s[ko - 1]
    fig["subspace"] = None
    if fig["gap"] > GAP:
        U = Us[:, :ko]
        fig["subspace"] = np.linalg.norm(Q - U @ (U.T @ Q), 2)             # = ||P_svd - P_Q||_2 for two ko-dimensional subspaces
        if not fig["subspace"] <= SUBSPACE_BAR:
            failed.append(("subspace", fig["subspace"], SUBSPACE_BAR))
    print(format_figures(fig))
    assert not failed, (label, blk, failed)
    return fig


def format_figures(f):
    return ("%-26s %-7s o%d Pc=%4d ko=%2d %-8s %-8s tol=%-5g ortho %.1e range %.1e backward %.1e (bar %.1e) var %+.1e "
            "gap %.3f floor %.3f subspace %s" % (f["label"], f["kind"], f["order"], f["Pc"], f["ko"], f["gram"], f["solver"], f["tol"],
                                                 f["ortho"], f["range"], f["backward"], f["bar"], f["variance"], f["gap"], f["floor"],
                                                 "-" if f["subspace"] is None else "%.1e" % f["subspace"]))
