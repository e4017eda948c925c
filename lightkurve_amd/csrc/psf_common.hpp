// psf_common.hpp — what psfphot.hip (fluxes at given positions), prfphot.hip (the same with a tabulated PRF), psffit.hip (fluxes and a common shift per cadence), prffit.hip (the same with a tabulated PRF), psfwidth.hip
// (the width of a cutout) and psfpos.hip (the positions of a cutout's stars) share: the cadence-per-four-lanes mapping, the
// Gaussian's edge integral, the table of factors and their derivatives by the centre (psffit.hip and psfpos.hip), the sums over
// a cadence's lanes, a tile's cadences and a wavefront, the Cholesky without pivoting with its singularity test, and the
// host-side grouping of a batch's cutouts by their star count.
#pragma once
#include <cmath>
#include <vector>

#include "lk_common.hpp"

namespace lk {

constexpr int PSF_LPC = 4;          // lanes per cadence: lane sub of a cadence takes the pixel rows sub, sub + 4, ...
constexpr int PSF_T = 64 / PSF_LPC; // cadences per workgroup of one wavefront
constexpr int PSF_MAX_STARS = 8;
constexpr int PSF_MAX_LDS = 160 * 1024;
constexpr double PSF_PIVOT_CUT = 1e-12;  // singular: a pivot d_k <= PSF_PIVOT_CUT * G_kk

// E(k) of the header: the Gaussian's integral up to the lower edge of pixel k (upper edge of pixel k - 1), as erf
__device__ __forceinline__ double psf_edge(int k, double c, double den) { return erf(((double)k - 0.5 - c) / den); }

// the sum of v over the PSF_LPC lanes of a cadence (adjacent lanes), the same bits in each of them: a + b is commutative, so
// the two lanes of a pair — and then the two pairs — hold the same sum
template <class T> __device__ __forceinline__ T psf_cadence_sum(T v) {
#pragma unroll
    for (int o = 1; o < PSF_LPC; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum over the PSF_T cadences of a tile of a value that the PSF_LPC lanes of each cadence already share (psf_cadence_sum):
// the butterfly across the cadences, the same bits in every lane and an order that depends on nothing
template <class T> __device__ __forceinline__ T psf_tile_sum(T v) {
#pragma unroll
    for (int o = PSF_LPC; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum of v over the 64 lanes of a wavefront by the same butterfly
template <class T> __device__ __forceinline__ T psf_wave_sum(T v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// One run of tables (a star's len column or row factors at centre c, width sg) for cadence slot cl: val[k][cl] = (E(k + 1) -
// E(k)) / 2 and der[k][cl] = its derivative by c, -(P(k + 1) - P(k)); every edge's erf and exp serve the two pixels it
// separates, len + 1 evaluations for len factors.
__device__ __forceinline__ void fit_table_run(double *__restrict__ val, double *__restrict__ der, int len, double c, double sg) {
    constexpr double INV_SQRT_2PI = 0.3989422804014327;
    const double den = M_SQRT2 * sg, pn = INV_SQRT_2PI / sg;
    double z = (-0.5 - c) / den;
    double lo = psf_edge(0, c, den), plo = exp(-z * z) * pn;
    for (int k = 0; k < len; ++k) {
        z = ((double)(k + 1) - 0.5 - c) / den;
        const double hi = psf_edge(k + 1, c, den), phi = exp(-z * z) * pn;
        val[k * PSF_T] = 0.5 * (hi - lo);
        der[k * PSF_T] = plo - phi;
        lo = hi, plo = phi;
    }
}

// G = L L^T in index order, no pivoting (G: upper triangle read); true when a pivot is not finite or <= PSF_PIVOT_CUT * G_kk
template <int K> __device__ __forceinline__ bool psf_cholesky(const double (&G)[K][K], double (&L)[K][K]) {
    bool singular = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double d = G[k][k];
#pragma unroll
        for (int j = 0; j < k; ++j) d -= L[k][j] * L[k][j];
        singular = singular || !(isfinite(d) && d > PSF_PIVOT_CUT * G[k][k]);
        L[k][k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            double s = G[k][i];
#pragma unroll
            for (int j = 0; j < k; ++j) s -= L[i][j] * L[k][j];
            L[i][k] = s / L[k][k];
        }
    }
    return singular;
}

// theta = G^-1 rhs from the factor: L z = rhs, L^T theta = z
template <int K> __device__ __forceinline__ void psf_solve(const double (&L)[K][K], const double (&rhs)[K], double (&theta)[K]) {
    double z[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double s = rhs[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s -= L[i][j] * z[j];
        z[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int j = i + 1; j < K; ++j) s -= L[j][i] * theta[j];
        theta[i] = s / L[i][i];
    }
}

// var[k] = (G^-1)_kk: M = L^-1 column by column, (G^-1)_kk = sum_i M_ik^2, i >= k
template <int K> __device__ __forceinline__ void psf_variances(const double (&L)[K][K], double (&var)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double M[K];
        M[k] = 1.0 / L[k][k];
        double v = M[k] * M[k];
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = k; j < i; ++j) s -= L[i][j] * M[j];
            M[i] = s / L[i][i];
            v += M[i] * M[i];
        }
        var[k] = v;
    }
}

// The stars of a batch as the kernels read them.  par [B][2 S_max + 2]: star columns, star rows (the cutout's stars — no NaN
// coordinate — first and in order), sigma_col, sigma_row (NaN for a NULL sigma_host: prfphot.hip's model has no width).  ints = order | n_stars | star_off, B each: order lists the cutouts
// grouped by their star count, those of S stars at order[first[S] .. first[S + 1]); star_off the first output row of a cutout.
struct PsfStars {
    std::vector<double> par;
    std::vector<int> ints;
    int first[PSF_MAX_STARS + 2] = {0};
    int total = 0;
};

inline int psf_group_stars(int B, int S_max, const double *star_col_host, const double *star_row_host, const double *sigma_host,
                           int32_t *star_off_host, PsfStars &st) {
    const int PAR = 2 * S_max + 2;
    st.par.assign((size_t)B * PAR, NAN);
    st.ints.assign((size_t)3 * B, 0);
    int *order = st.ints.data(), *n_stars = order + B, *star_off = n_stars + B;
    for (int b = 0; b < B; ++b) {
        double *p = st.par.data() + (size_t)b * PAR;
        int S = 0;
        for (int s = 0; s < S_max; ++s) {
            const double c = star_col_host[(size_t)b * S_max + s], r = star_row_host[(size_t)b * S_max + s];
            if (std::isnan(c) || std::isnan(r)) continue;
            LK_REQUIRE(std::isfinite(c) && std::isfinite(r), "cutout %d: star %d has an infinite coordinate", b, s);
            p[S] = c;
            p[S_max + S] = r;
            ++S;
        }
        LK_REQUIRE(S >= 1, "cutout %d has no star", b);
        for (int k = 0; sigma_host && k < 2; ++k) {
            const double sg = sigma_host[2 * (size_t)b + k];
            LK_REQUIRE(std::isfinite(sg) && sg > 0.0, "cutout %d: sigma must be finite and > 0 (got %g)", b, sg);
            p[2 * S_max + k] = sg;
        }
        n_stars[b] = S;
        star_off[b] = st.total;
        st.total += S;
        ++st.first[S + 1];
    }
    for (int S = 1; S <= PSF_MAX_STARS + 1; ++S) st.first[S] += st.first[S - 1];  // first[S]: where the cutouts of S stars begin
    int at[PSF_MAX_STARS + 1];
    for (int S = 0; S <= PSF_MAX_STARS; ++S) at[S] = st.first[S];
    for (int b = 0; b < B; ++b) order[at[n_stars[b]]++] = b;
    if (star_off_host) {
        for (int b = 0; b < B; ++b) star_off_host[b] = star_off[b];
        star_off_host[B] = st.total;
    }
    return LK_OK;
}

// psfphot.hip: status[b] = 0 when a cadence of cutout b has cadence_status 0, else 1 (cube_psfphot_status_kernel)
int psf_status_launch(int B, int N, const int8_t *cadence_status, int32_t *status, hipStream_t stream);

}  // namespace lk
