// spline_basis.hpp — one row of the clamped B-spline basis (patsy bs(x, ..., include_intercept=True)), shared by every kernel
// that builds a spline block (pld.hip: pld_spline_kernel; sff.hip: sff_design_kernel) so that they give the same bits for the
// same x and knots.  Include it only in translation units compiled with the default floating-point contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace lk {

// de Boor: the degree + 1 non-zero basis values Nv[0..degree] of x on the knot vector [lo x (degree + 1), inner(0) ..
// inner(n_inner - 1), hi x (degree + 1)]; returns the column of Nv[0].  degree <= 7.
template <class Inner>
__device__ __forceinline__ int bspline_row(double x, double lo, double hi, Inner inner, int n_inner, int degree, double *Nv) {
    const int order = degree + 1;
    auto T = [&](int i) -> double {  // full knot vector: order copies of lo, inner, order copies of hi
        if (i < order) return lo;
        if (i >= order + n_inner) return hi;
        return inner(i - order);
    };
    // knot span: largest mu with T(mu) <= x < T(mu+1), the right end belongs to the last non-empty span
    int mu = order - 1;
    const int last = order + n_inner - 1;
    while (mu < last && !(x < T(mu + 1))) ++mu;
    while (mu > order - 1 && T(mu) == T(mu + 1)) --mu;  // skip empty spans at repeated interior knots
    double left[8], right[8];
    Nv[0] = 1.0;
#pragma unroll
    for (int j = 1; j < 8; ++j) Nv[j] = 0.0;
    for (int j = 1; j <= degree; ++j) {
        left[j] = x - T(mu + 1 - j);
        right[j] = T(mu + j) - x;
        double saved = 0.0;
        for (int r = 0; r < j; ++r) {
            const double den = right[r + 1] + left[j - r];
            const double tmp = den != 0.0 ? Nv[r] / den : 0.0;
            // the fused form is spelled out: left to the compiler, saved + right * tmp (saved itself a product) may fuse either
            // product, and a caller whose degree is a constant gets the other choice than the loop does
            Nv[r] = fma(right[r + 1], tmp, saved);
            saved = left[j - r] * tmp;
        }
        Nv[j] = saved;
    }
    return mu - degree;
}

}  // namespace lk
