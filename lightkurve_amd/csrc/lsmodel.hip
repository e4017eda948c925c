// lsmodel.hip — LombScarglePeriodogram.model for a ragged batch on gfx950: the best-fit truncated Fourier series of every
// target at the target's own frequency, evaluated and subtracted on the device.
//
// Reference: lightkurve_amd/periodogram.py ls_model_host (astropy 4.3.1 LombScargle.model -> mle.periodic_fit,
// implementations/mle.py:58-114, reached from the reference's periodogram.py:991-1018).  One frequency per target; one
// workgroup of 512 threads per target, two streaming passes over its cadences:
//
//   weights  dy given: one pass over the target's dy decides whether they are all finite (w = dy^-2) or not (w = 1, the rule
//            of the other stages: packed.bls_ivar); dy NULL: w = 1 and nothing is read.
//   pass 1   t = time - time[first], x = 2 pi f t; one sincos and the angle-addition recurrence give cos(kx), sin(kx) for
//            k <= 2 nterms.  Per thread 6 nterms + 2 running sums, the product-to-sum form of the fastchi2 kernels:
//            C_k = sum w cos(kx) (k = 0 .. 2 nterms; C_0 = sum w), S_k = sum w sin(kx) (k = 1 .. 2 nterms),
//            YC_m = sum w (y - y[first]) cos(mx) (m = 0 .. nterms), YS_m = sum w (y - y[first]) sin(mx) (m = 1 .. nterms).
//            The kernel is templated on nterms and the loops over k are fully unrolled: every sum lives in a register.
//   scalar   thread 0: y_mean = y[first] + YC_0 / C_0 (center_data; else 0).  The moments of the normal equations follow
//            from the sums — sin a sin b = (C_{a-b} - C_{a+b}) / 2, cos a cos b = (C_{a-b} + C_{a+b}) / 2,
//            sin a cos b = (S_{a+b} + S_{a-b}) / 2 — and the right-hand side from sum w x (y - y_mean) =
//            Y*_a - (y_mean - y[first]) *_a, which is why ONE pass suffices although y_mean is only known at its end
//            (subtracting y[first] first keeps that difference free of cancellation for a normalised light curve).
//            K x K solve (K = 2 nterms + fit_mean <= 17) in LDS, LU with partial pivoting.
//   pass 2   (rows from L2) the model, the residual, chi2_ref = sum w (y - y_mean)^2, chi2_model = sum w (y - model)^2.
//
// STATUS per target — 1: fitted.  0: frequency NaN or <= 0, the target is skipped (nothing is fitted).  -1: fewer than K
// cadences, or a pivot / coefficient that is zero or not finite (astropy raises; a batch reports it per target).  Where the
// status is not 1: theta and the statistics are NaN, the model is NaN, the residual is the flux, bit for bit.
//
// ORDER OF THE SUMS — the rule of blsstats.hip: thread-strided (thread i takes cadences i, i + 512, ...), then a 64-lane xor
// butterfly, then the eight waves added in wave order by one thread.  No floating-point atomics: a target's outputs are a
// function of its own data alone (not of B, the neighbours or the grid).
#include <algorithm>
#include <cmath>
#include <vector>

#include "lk_common.hpp"

namespace lk {

namespace {

constexpr int LM_NT = 512;                        // threads per workgroup (one workgroup per target)
constexpr int LM_NW = LM_NT / 64;                 // its waves
constexpr int LM_MAX_TERMS = 8;
constexpr int LM_MAX_K = 2 * LM_MAX_TERMS + 1;    // columns of the widest design matrix
constexpr int LM_EVAL_NT = 256;                   // threads per workgroup of the evaluation kernel

__device__ __forceinline__ double wave_sum_lm(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// sum over m <= nterms of th[2m - 1] sin(mx) + th[2m] cos(mx): the periodic part of the model (th[0] is the bias)
__device__ __forceinline__ double ls_series(double x, int nterms, const double *th) {
    double s1, c1;
    sincos(x, &s1, &c1);
    double sk = s1, ck = c1, acc = th[1] * s1 + th[2] * c1;
    for (int m = 2; m <= nterms; ++m) {
        const double cn = ck * c1 - sk * s1;
        sk = sk * c1 + ck * s1;
        ck = cn;
        acc += th[2 * m - 1] * sk + th[2 * m] * ck;
    }
    return acc;
}

// A[K][K + 1] (augmented, in LDS) -> x[K]; false when a pivot or a solution entry is zero / not finite
__device__ bool solve_lm(double (*A)[LM_MAX_K + 1], int K, double *x) {
    for (int c = 0; c < K; ++c) {
        int p = c;
        for (int r = c + 1; r < K; ++r)
            if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
        if (!(fabs(A[p][c]) > 0.0) || !isfinite(A[p][c])) return false;
        if (p != c)
            for (int k = c; k <= K; ++k) {
                const double s = A[c][k];
                A[c][k] = A[p][k];
                A[p][k] = s;
            }
        for (int r = c + 1; r < K; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int k = c; k <= K; ++k) A[r][k] -= f * A[c][k];
        }
    }
    bool ok = true;
    for (int r = K - 1; r >= 0; --r) {
        double s = A[r][K];
        for (int k = r + 1; k < K; ++k) s -= A[r][k] * x[k];
        x[r] = s / A[r][r];
        ok = ok && isfinite(x[r]);
    }
    return ok;
}

}  // namespace

template <int NTERMS>
__global__ __launch_bounds__(LM_NT) void ls_model_kernel(const double *__restrict__ time, const double *__restrict__ flux,
                                                         const double *__restrict__ dy, const int64_t *__restrict__ n_off,
                                                         const double *__restrict__ frequency, int fit_mean, int center_data,
                                                         int keep_mean, double *__restrict__ theta, double *__restrict__ stats,
                                                         double *__restrict__ model, double *__restrict__ residual) {
    constexpr int NK = 2 * NTERMS;                // highest harmonic of the sums
    constexpr int NSUM = 6 * NTERMS + 2;          // C_0..C_NK | S_1..S_NK | YC_0..YC_NTERMS | YS_1..YS_NTERMS
    constexpr int OFF_S = NK, OFF_YC = 2 * NK + 1, OFF_YS = 2 * NK + 1 + NTERMS;
    __shared__ double sh_part[LM_NW][NSUM + 1];
    __shared__ double sh_sum[NSUM];
    __shared__ double sh_A[LM_MAX_K][LM_MAX_K + 1];
    __shared__ double sh_theta[LM_MAX_K], sh_x[LM_MAX_K];
    __shared__ double sh_ymean;
    __shared__ int sh_status, sh_bad_dy;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lo = n_off[b], n = n_off[b + 1] - lo;
    const double *tb = time + lo, *yb = flux + lo;
    const int K = NK + (fit_mean ? 1 : 0);
    const double f = frequency[b];
    const double omega = 2 * M_PI * f;
    int status = !(f > 0.0) ? 0 : (n < K ? -1 : 1);   // NaN fails f > 0
    const double t0 = n > 0 ? tb[0] : 0.0, y0 = n > 0 ? yb[0] : 0.0;

    // ---------------------------------------------------------------------------------------------------- weights
    const double *eb = nullptr;
    if (dy && status == 1) {
        if (tid == 0) sh_bad_dy = 0;
        __syncthreads();
        bool bad = false;
        for (int64_t i = tid; i < n; i += LM_NT) bad = bad || !isfinite(dy[lo + i]);
        if (bad) sh_bad_dy = 1;
        __syncthreads();
        if (!sh_bad_dy) eb = dy + lo;
    }

    if (status == 1) {
        // ------------------------------------------------------------------------------------------------ pass 1
        double aC[NK + 1], aS[NK + 1], aYC[NTERMS + 1], aYS[NTERMS + 1];
#pragma unroll
        for (int k = 0; k <= NK; ++k) aC[k] = aS[k] = 0.0;
#pragma unroll
        for (int k = 0; k <= NTERMS; ++k) aYC[k] = aYS[k] = 0.0;
        for (int64_t i = tid; i < n; i += LM_NT) {
            const double tv = tb[i] - t0, yv = yb[i] - y0;
            double w = 1.0;
            if (eb) {
                const double e = eb[i];
                w = 1.0 / (e * e);
            }
            const double yw = yv * w;
            double s1, c1;
            sincos(omega * tv, &s1, &c1);
            double sk = 0.0, ck = 1.0;
            aC[0] += w;
            aYC[0] += yw;
#pragma unroll
            for (int k = 1; k <= NK; ++k) {
                const double cn = ck * c1 - sk * s1;
                sk = sk * c1 + ck * s1;
                ck = cn;
                aC[k] += w * ck;
                aS[k] += w * sk;
                if (k <= NTERMS) {
                    aYC[k] += yw * ck;
                    aYS[k] += yw * sk;
                }
            }
        }
#pragma unroll
        for (int k = 0; k <= NK; ++k) {
            const double r = wave_sum_lm(aC[k]);
            if (lane == 0) sh_part[wave][k] = r;
        }
#pragma unroll
        for (int k = 1; k <= NK; ++k) {
            const double r = wave_sum_lm(aS[k]);
            if (lane == 0) sh_part[wave][OFF_S + k] = r;
        }
#pragma unroll
        for (int k = 0; k <= NTERMS; ++k) {
            const double r = wave_sum_lm(aYC[k]);
            if (lane == 0) sh_part[wave][OFF_YC + k] = r;
        }
#pragma unroll
        for (int k = 1; k <= NTERMS; ++k) {
            const double r = wave_sum_lm(aYS[k]);
            if (lane == 0) sh_part[wave][OFF_YS + k] = r;
        }
        __syncthreads();
        if (tid < NSUM) {
            double r = sh_part[0][tid];
            for (int w = 1; w < LM_NW; ++w) r += sh_part[w][tid];
            sh_sum[tid] = r;
        }
        __syncthreads();

        // ------------------------------------------------------------------------------------------------ scalar part
        if (tid == 0) {
            const double *S = sh_sum;
            auto Cs = [&](int k) { return S[k < 0 ? -k : k]; };
            auto Ss = [&](int k) { return k > 0 ? S[OFF_S + k] : (k < 0 ? -S[OFF_S - k] : 0.0); };
            const double y_mean = center_data ? y0 + S[OFF_YC] / S[0] : 0.0;
            const double d = y_mean - y0;
            const int first = fit_mean ? 1 : 0;      // column of sin(x); column j >= first: harmonic (j - first) / 2 + 1,
                                                     // a sine when j - first is even
            for (int r = 0; r < K; ++r) {
                const bool r_bias = r < first, r_sin = ((r - first) & 1) == 0;
                const int a = r_bias ? 0 : (r - first) / 2 + 1;
                for (int c = 0; c < K; ++c) {
                    const bool c_bias = c < first, c_sin = ((c - first) & 1) == 0;
                    const int e = c_bias ? 0 : (c - first) / 2 + 1;
                    double v;
                    if (r_bias || c_bias) {          // a bias column is cos(0 x)
                        const int h = a + e;
                        const bool is_sin = (!r_bias && r_sin) || (!c_bias && c_sin);
                        v = is_sin ? Ss(h) : Cs(h);
                    } else if (r_sin && c_sin) {
                        v = 0.5 * (Cs(a - e) - Cs(a + e));
                    } else if (!r_sin && !c_sin) {
                        v = 0.5 * (Cs(a - e) + Cs(a + e));
                    } else if (r_sin) {
                        v = 0.5 * (Ss(a + e) + Ss(a - e));
                    } else {
                        v = 0.5 * (Ss(a + e) + Ss(e - a));
                    }
                    sh_A[r][c] = v;
                }
                sh_A[r][K] = r_bias ? S[OFF_YC] - d * S[0] : (r_sin ? S[OFF_YS + a] - d * Ss(a) : S[OFF_YC + a] - d * Cs(a));
            }
            const bool ok = isfinite(y_mean) && solve_lm(sh_A, K, sh_x);
            sh_status = ok ? 1 : -1;
            sh_ymean = y_mean;
            sh_theta[0] = fit_mean ? sh_x[0] : 0.0;
            for (int j = first; j < K; ++j) sh_theta[j - first + 1] = sh_x[j];
        }
        __syncthreads();
        status = sh_status;
    }

    double *th_out = theta + (int64_t)b * (NK + 1), *st = stats + (int64_t)b * LK_LS_MODEL_NSTATS;
    if (status != 1) {
        // ------------------------------------------------------------------------------------- skipped or not fitted
        if (tid <= NK) th_out[tid] = NAN;
        if (tid == 0) {
            st[0] = st[1] = st[2] = NAN;
            st[3] = (double)status;
        }
        for (int64_t i = tid; i < n; i += LM_NT) {
            if (model) model[lo + i] = NAN;
            if (residual) residual[lo + i] = yb[i];
        }
        return;
    }

    // ---------------------------------------------------------------------------------------------------- pass 2
    const double y_mean = sh_ymean, bias = sh_theta[0];
    if (tid <= NK) th_out[tid] = sh_theta[tid];
    double c_ref = 0.0, c_mod = 0.0;
    for (int64_t i = tid; i < n; i += LM_NT) {
        const double tv = tb[i] - t0, yv = yb[i];
        double w = 1.0;
        if (eb) {
            const double e = eb[i];
            w = 1.0 / (e * e);
        }
        const double per = ls_series(omega * tv, NTERMS, sh_theta);
        const double mdl = y_mean + (bias + per);
        const double r_ref = yv - y_mean, r_mod = yv - mdl;
        c_ref += w * (r_ref * r_ref);
        c_mod += w * (r_mod * r_mod);
        if (model) model[lo + i] = mdl;
        if (residual) residual[lo + i] = keep_mean ? yv - per : r_mod;
    }
    c_ref = wave_sum_lm(c_ref);
    c_mod = wave_sum_lm(c_mod);
    if (lane == 0) {
        sh_part[wave][0] = c_ref;
        sh_part[wave][1] = c_mod;
    }
    __syncthreads();
    if (tid == 0) {
        double r_ref = sh_part[0][0], r_mod = sh_part[0][1];
        for (int w = 1; w < LM_NW; ++w) {
            r_ref += sh_part[w][0];
            r_mod += sh_part[w][1];
        }
        st[0] = y_mean;
        st[1] = r_ref;
        st[2] = r_mod;
        st[3] = 1.0;
    }
}

// out = y_mean + bias + series(t_fit - t_ref[b]) over target b's slice [m_off[b], m_off[b + 1]) of t_fit; NaN where the target
// was not fitted.  par: t_ref[B] | frequency[B].  Workgroup (b, j) of gridDim.y takes the slice's chunks j, j + gridDim.y, ...
__global__ __launch_bounds__(LM_EVAL_NT) void ls_model_eval_kernel(const double *__restrict__ t_fit, const int64_t *__restrict__ m_off,
                                                                   const double *__restrict__ par, int B, int nterms,
                                                                   const double *__restrict__ theta, const double *__restrict__ stats,
                                                                   double *__restrict__ out) {
    __shared__ double sh_theta[LM_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = m_off[b], m = m_off[b + 1] - lo;
    if (tid <= 2 * nterms) sh_theta[tid] = theta[(int64_t)b * (2 * nterms + 1) + tid];
    __syncthreads();
    const double *st = stats + (int64_t)b * LK_LS_MODEL_NSTATS;
    const bool fitted = st[3] == 1.0;
    const double t_ref = par[b], omega = 2 * M_PI * par[B + b], offset = st[0] + sh_theta[0];
    for (int64_t i = (int64_t)blockIdx.y * LM_EVAL_NT + tid; i < m; i += (int64_t)gridDim.y * LM_EVAL_NT)
        out[lo + i] = fitted ? offset + ls_series(omega * (t_fit[lo + i] - t_ref), nterms, sh_theta) : NAN;
}

namespace {

template <int NTERMS>
void launch_fit(int B, hipStream_t stream, const double *time, const double *flux, const double *dy, const int64_t *d_off,
                const double *d_freq, int fit_mean, int center_data, int keep_mean, double *theta, double *stats, double *model,
                double *residual) {
    hipLaunchKernelGGL(ls_model_kernel<NTERMS>, dim3((unsigned)B), dim3(LM_NT), 0, stream, time, flux, dy, d_off, d_freq, fit_mean,
                       center_data, keep_mean, theta, stats, model, residual);
}

int check_offsets(int B, const int64_t *off, const char *name) {
    LK_REQUIRE(off[0] == 0, "%s must be prefix offsets starting at 0", name);
    for (int b = 0; b < B; ++b) LK_REQUIRE(off[b + 1] >= off[b], "%s must be non-decreasing", name);
    return LK_OK;
}

}  // namespace

int ls_model_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *dy,
                    const double *frequency_host, int nterms, int fit_mean, int center_data, int keep_mean, double *theta,
                    double *stats, double *model, double *residual, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host, "bad batch description");
    LK_REQUIRE(nterms >= 1 && nterms <= LM_MAX_TERMS, "nterms must be 1 .. %d (got %d)", LM_MAX_TERMS, nterms);
    if (B == 0) return LK_OK;
    LK_REQUIRE(frequency_host, "NULL frequency");
    LK_REQUIRE(theta && stats, "NULL output buffer");
    if (const int rc = check_offsets(B, n_off_host, "n_off")) return rc;
    LK_REQUIRE(n_off_host[B] == 0 || (time && flux), "NULL time or flux");
    int64_t *d_off;
    double *d_freq;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, (size_t)B + 1).upload(d_freq, frequency_host, (size_t)B).carve(stream))
        return rc;
    fit_mean = fit_mean != 0, center_data = center_data != 0, keep_mean = keep_mean != 0;
#define LM_CASE(NTERMS)                                                                                                          \
    case NTERMS:                                                                                                                 \
        launch_fit<NTERMS>(B, stream, time, flux, dy, d_off, d_freq, fit_mean, center_data, keep_mean, theta, stats, model,      \
                           residual);                                                                                            \
        break;
    switch (nterms) {
        LM_CASE(1) LM_CASE(2) LM_CASE(3) LM_CASE(4) LM_CASE(5) LM_CASE(6) LM_CASE(7) LM_CASE(8)
    }
#undef LM_CASE
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int ls_model_eval_launch(lk_handle *h, int B, const int64_t *m_off_host, const double *t_fit, const double *t_ref_host,
                         const double *frequency_host, int nterms, const double *theta, const double *stats, double *out,
                         hipStream_t stream) {
    LK_REQUIRE(B >= 0 && m_off_host, "bad batch description");
    LK_REQUIRE(nterms >= 1 && nterms <= LM_MAX_TERMS, "nterms must be 1 .. %d (got %d)", LM_MAX_TERMS, nterms);
    if (B == 0) return LK_OK;
    LK_REQUIRE(t_ref_host && frequency_host, "NULL t_ref or frequency");
    LK_REQUIRE(theta && stats, "NULL fit parameters");
    if (const int rc = check_offsets(B, m_off_host, "m_off")) return rc;
    if (m_off_host[B] == 0) return LK_OK;
    LK_REQUIRE(t_fit && out, "NULL t_fit or out");
    int64_t longest = 0;
    for (int b = 0; b < B; ++b) longest = std::max(longest, m_off_host[b + 1] - m_off_host[b]);
    std::vector<double> par((size_t)B * 2);
    for (int b = 0; b < B; ++b) {
        par[b] = t_ref_host[b];
        par[(size_t)B + b] = frequency_host[b];
    }
    int64_t *d_off;
    double *d_par;
    if (const int rc =
            Scratch(h, h->ws).upload(d_off, m_off_host, (size_t)B + 1).upload(d_par, (const double *)par.data(), par.size()).carve(stream))
        return rc;
    const unsigned chunks = (unsigned)std::min<int64_t>((longest + LM_EVAL_NT - 1) / LM_EVAL_NT, 64);
    hipLaunchKernelGGL(ls_model_eval_kernel, dim3((unsigned)B, chunks), dim3(LM_EVAL_NT), 0, stream, t_fit, d_off, d_par, B, nterms,
                       theta, stats, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
