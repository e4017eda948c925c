// ampimage.hip — the per-pixel sinusoid fit of resident pixel cubes on gfx950: amplitude images, the periodic twin of the
// transit difference image of pixcube.hip (is a pulsation, a rotation signal or a contact binary on the target's pixels or on a
// neighbour's?).
//
// Reference: PixelCube.amplitude_image (correctors/pldcorrector.py), plain float64 numpy: pixel p of cutout b is fitted, on the
// cadences where the time is finite and its own flux is not NaN, by the design of lk_ls_model_batch with fit_mean, center_data
// and unit weights — x = [1, sin(2 pi m f (t - t_ref)), cos(2 pi m f (t - t_ref))], m = 1 .. nterms, K = 2 nterms + 1 columns,
// y centred on the pixel's own mean.  Everything float64 after the float32 load.
//
//   trig     one thread per (cutout, cadence): the 2 nterms sines and cosines and a validity byte (finite time, usable
//            frequency), once per cutout; n_valid[b] counts the valid cadences (integer atomics, one per wavefront).
//   pivot    one thread per pixel: its first finite value at a valid cadence.  The sums below run over y' = y - pivot, exact in
//            float64, so that they do not carry the pedestal; the pivot goes back into `level` at the end.
//   accum    workgroup (chunk of AI_CHUNK cadences, cutout), lanes = adjacent pixels (cutouts of more than AI_T pixels take
//            them in groups).  The chunk's trig rows are staged once in LDS.  A lane walks its pixel down the chunk in cadence
//            order and keeps n, sum y', sum x_k y'.  A pixel's normal matrix differs from the cutout's only where the pixel has
//            NaNs: the chunk's shared entries sum x_i x_j (i <= j) are formed once per workgroup, and a lane adds x_i x_j of
//            the cadences IT misses on the rare NaN branch (written only where there are any).
//   finish   one thread per pixel adds the chunks in index order, takes the missed entries off the shared matrix, centres the
//            right-hand side, solves the K x K system and its inverse by Gaussian elimination with partial pivoting (fully
//            unrolled: the augmented matrix lives in registers) and writes theta, level and the inverse entries that
//            amplitude_err needs.
//   resid    the same chunking re-reads the cube and reduces chi2 = sum (y - model)^2 from the residuals, chunk partials.
//   images   one thread per pixel: chi2 in index order, then amplitude, phase, amplitude_err, snr.
//
// No floating-point atomics; the order of every sum depends on N alone, so a cutout's images have the same bits alone, in any
// batch position and from run to run.  Rows of cadences with an invalid time are not loaded; flux_err is not read.
#include <cmath>
#include <vector>

#include "lk_common.hpp"

namespace lk {

namespace {

constexpr int AI_CHUNK = 128;  // cadences per workgroup: the order of every sum depends on N alone
constexpr int AI_T = 128;      // lanes: adjacent pixels of one cadence row per load
constexpr int AI_ROWS = 8;     // cadence rows whose loads a lane issues before it uses them
constexpr int AI_MAX_TERMS = 3;

constexpr int ai_tri(int K) { return K * (K + 1) / 2; }          // entries i <= j of a K x K symmetric matrix
__host__ __device__ constexpr int ai_idx(int K, int i, int j) {  // their row-major index, i <= j
    return i * K - i * (i - 1) / 2 + (j - i);
}

// [A | I] -> [U | L^-1 P] -> A^-1 in the right half; A: K x 2K in registers (every index is a compile-time constant once the
// loops are unrolled).  false for a pivot that is zero or not finite.
template <int K> __device__ __forceinline__ bool ai_invert(double (&A)[K][2 * K]) {
    constexpr int W = 2 * K;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        int p = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < K; ++r) {
            const double a = fabs(A[r][c]);
            if (a > best) {
                best = a;
                p = r;
            }
        }
        ok = ok && best > 0.0 && isfinite(best);
#pragma unroll
        for (int r = c + 1; r < K; ++r)
            if (r == p) {
#pragma unroll
                for (int k = c; k < W; ++k) {
                    const double s = A[c][k];
                    A[c][k] = A[r][k];
                    A[r][k] = s;
                }
            }
#pragma unroll
        for (int r = c + 1; r < K; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int k = c; k < W; ++k) A[r][k] -= f * A[c][k];
        }
    }
#pragma unroll
    for (int col = K; col < W; ++col) {
#pragma unroll
        for (int r = K - 1; r >= 0; --r) {
            double s = A[r][col];
#pragma unroll
            for (int k = r + 1; k < K; ++k) s -= A[r][k] * A[k][col];
            A[r][col] = s / A[r][r];
        }
    }
    return ok;
}

// the chunk's trig rows and validity bytes -> LDS; rows past the end of the cutout are invalid
template <int NT>
__device__ __forceinline__ void ai_stage(const double *__restrict__ trig, const uint8_t *__restrict__ valid, size_t row0, int rows,
                                         double *sh_x, uint8_t *sh_valid) {
    for (int k = threadIdx.x; k < AI_CHUNK * 2 * NT; k += AI_T) sh_x[k] = k < rows * 2 * NT ? trig[row0 * 2 * NT + k] : 0.0;
    for (int j = threadIdx.x; j < AI_CHUNK; j += AI_T) sh_valid[j] = j < rows ? valid[row0 + j] : 0;
    __syncthreads();
}

}  // namespace

// par = [frequency[B] | t_ref[B]].  trig[b][i] = sin(x), cos(x), sin(2x), cos(2x), ... with m x = ((2 pi m) f) (t - t_ref), the
// expression of the mirror; zeros where the cadence is not valid.  n_valid is zeroed by the launcher.
__global__ __launch_bounds__(256) void cube_ampimage_trig_kernel(const double *__restrict__ time, const double *__restrict__ par,
                                                                 int B, int N, int nterms, double *__restrict__ trig,
                                                                 uint8_t *__restrict__ valid, int *__restrict__ n_valid) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (i < N) {
        const double f = par[b], t = time[(size_t)b * N + i];
        ok = f > 0.0 && isfinite(f) && isfinite(t);
        const double dt = t - par[B + b];
        double *out = trig + ((size_t)b * N + i) * 2 * nterms;
        for (int m = 1; m <= nterms; ++m) {
            double s = 0.0, c = 0.0;
            if (ok) sincos(((2.0 * M_PI * m) * f) * dt, &s, &c);
            out[2 * m - 2] = s;
            out[2 * m - 1] = c;
        }
        valid[(size_t)b * N + i] = ok ? 1 : 0;
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&n_valid[b], __popcll(bal));
}

// pivot[b][p]: the first finite value of pixel p at a valid cadence, 0 for a pixel without one
__global__ __launch_bounds__(AI_T) void cube_ampimage_pivot_kernel(const float *__restrict__ flux, const uint8_t *__restrict__ valid,
                                                                   int N, int npix, double *__restrict__ pivot) {
    const int b = blockIdx.y, p = blockIdx.x * AI_T + threadIdx.x;
    if (p >= npix) return;
    const uint8_t *va = valid + (size_t)b * N;
    const float *f = flux + (size_t)b * N * npix + p;
    double pv = 0.0;
    for (int i = 0; i < N; ++i) {
        if (!va[i]) continue;
        const float v = f[(size_t)i * npix];
        if (isfinite(v)) {
            pv = (double)v;
            break;
        }
    }
    pivot[(size_t)b * npix + p] = pv;
}

// Workgroup (chunk, b).  Outputs per chunk: cshared[b][chunk][tri(K)] = sum over the valid cadences of x_i x_j (x_0 = 1, so
// entry (0, 0) counts them); pcnt[b][chunk][p] = the pixel's values; psum[b][chunk][K][p] = sum y' | sum x_k y';
// pmiss[b][chunk][tri(K)][p] = sum x_i x_j over the valid cadences where the pixel is NaN — written only for a pixel that
// misses any (the finish kernel knows from the counts).
template <int NT>
__global__ __launch_bounds__(AI_T) void cube_ampimage_accum_kernel(const float *__restrict__ flux, const double *__restrict__ trig,
                                                                   const uint8_t *__restrict__ valid,
                                                                   const double *__restrict__ pivot, int N, int npix, int chunks,
                                                                   double *__restrict__ cshared, int *__restrict__ pcnt,
                                                                   double *__restrict__ psum, double *__restrict__ pmiss) {
    constexpr int K = 2 * NT + 1, TRI = ai_tri(K);
    __shared__ double sh_x[AI_CHUNK * 2 * NT];
    __shared__ uint8_t sh_valid[AI_CHUNK];
    const int b = blockIdx.y, ch = blockIdx.x, c0 = ch * AI_CHUNK, rows = min(AI_CHUNK, N - c0);
    const size_t row0 = (size_t)b * N + c0, slot = (size_t)b * chunks + ch;
    ai_stage<NT>(trig, valid, row0, rows, sh_x, sh_valid);
    if (threadIdx.x < TRI) {                                   // the shared entries: thread (i, j) walks the chunk in order
        int i = 0, j = threadIdx.x;
        while (j >= K - i) {
            j -= K - i;
            ++i;
        }
        j += i;
        double s = 0.0;
        for (int r = 0; r < rows; ++r) {
            if (!sh_valid[r]) continue;
            const double xi = i == 0 ? 1.0 : sh_x[r * 2 * NT + i - 1], xj = j == 0 ? 1.0 : sh_x[r * 2 * NT + j - 1];
            s += xi * xj;
        }
        cshared[slot * TRI + threadIdx.x] = s;
    }
    const float *fl = flux + row0 * npix;
    for (int p = threadIdx.x; p < npix; p += AI_T) {
        const double pv = pivot[(size_t)b * npix + p];
        int n = 0, n_miss = 0;
        double sy = 0.0, r[2 * NT], miss[TRI];
#pragma unroll
        for (int k = 0; k < 2 * NT; ++k) r[k] = 0.0;
#pragma unroll
        for (int k = 0; k < TRI; ++k) miss[k] = 0.0;
        for (int j0 = 0; j0 < rows; j0 += AI_ROWS) {
            float v[AI_ROWS];
#pragma unroll
            for (int u = 0; u < AI_ROWS; ++u) v[u] = sh_valid[j0 + u] ? fl[(size_t)(j0 + u) * npix + p] : 0.0f;
#pragma unroll
            for (int u = 0; u < AI_ROWS; ++u) {
                if (!sh_valid[j0 + u]) continue;
                const double *x = sh_x + (j0 + u) * 2 * NT;
                if (isnan(v[u])) {
                    ++n_miss;
                    double xr[K];
                    xr[0] = 1.0;
#pragma unroll
                    for (int k = 0; k < 2 * NT; ++k) xr[k + 1] = x[k];
#pragma unroll
                    for (int i = 0; i < K; ++i)
#pragma unroll
                        for (int j = i; j < K; ++j) miss[ai_idx(K, i, j)] += xr[i] * xr[j];
                    continue;
                }
                const double yd = (double)v[u] - pv;
                ++n;
                sy += yd;
#pragma unroll
                for (int k = 0; k < 2 * NT; ++k) r[k] += x[k] * yd;
            }
        }
        pcnt[slot * npix + p] = n;
        double *ps = psum + slot * K * npix + p;
        ps[0] = sy;
#pragma unroll
        for (int k = 0; k < 2 * NT; ++k) ps[(size_t)(k + 1) * npix] = r[k];
        if (n_miss) {
            double *pm = pmiss + slot * TRI * npix + p;
#pragma unroll
            for (int k = 0; k < TRI; ++k) pm[(size_t)k * npix] = miss[k];
        }
    }
}

// One thread per pixel.  theta: [K][B][npix] (coefficient-major: every coefficient image of the batch is one block); level,
// pivot: [B][npix]; cinv: [3 nterms][B][npix] = (C_ss, C_sc, C_cc) of every harmonic, C the inverse of the pixel's normal matrix;
// n_used: [B][npix]; fit_status[b]: 1 frequency NaN or <= 0, 2 fewer than K + 1 valid cadences, else 0 (written by pixel 0).
// A cutout whose status is not 0, a pixel with fewer than K values and one with a zero or non-finite pivot or coefficient are
// NaN in theta, level and cinv; n_used is 0 for a cutout that was not fitted.
template <int NT>
__global__ __launch_bounds__(AI_T) void cube_ampimage_finish_kernel(const double *__restrict__ par, const int *__restrict__ n_valid,
                                                                    const double *__restrict__ pivot,
                                                                    const double *__restrict__ cshared,
                                                                    const int *__restrict__ pcnt, const double *__restrict__ psum,
                                                                    const double *__restrict__ pmiss, int B, int npix, int chunks,
                                                                    double *__restrict__ theta, double *__restrict__ level,
                                                                    double *__restrict__ cinv, int *__restrict__ n_used,
                                                                    int *__restrict__ fit_status) {
    constexpr int K = 2 * NT + 1, TRI = ai_tri(K);
    const int b = blockIdx.y, p = blockIdx.x * AI_T + threadIdx.x;
    if (p >= npix) return;
    const double f = par[b];
    const int status = !(f > 0.0 && isfinite(f)) ? 1 : (n_valid[b] < K + 1 ? 2 : 0);
    if (p == 0) fit_status[b] = status;
    const size_t o = (size_t)b * npix + p, img = (size_t)B * npix;
    long long n = 0;
    double rhs[K], sh[TRI], ms[TRI];
#pragma unroll
    for (int k = 0; k < K; ++k) rhs[k] = 0.0;
#pragma unroll
    for (int k = 0; k < TRI; ++k) sh[k] = ms[k] = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        const size_t slot = (size_t)b * chunks + ch;
        const double *cs = cshared + slot * TRI;
        const int nc = pcnt[slot * npix + p];
        n += nc;
#pragma unroll
        for (int k = 0; k < K; ++k) rhs[k] += psum[(slot * K + k) * npix + p];
#pragma unroll
        for (int k = 0; k < TRI; ++k) sh[k] += cs[k];
        if ((double)nc != cs[0]) {                             // the pixel misses cadences of this chunk (entry (0, 0) counts them)
#pragma unroll
            for (int k = 0; k < TRI; ++k) ms[k] += pmiss[(slot * TRI + k) * npix + p];
        }
    }
    double A[K][2 * K];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int k = i <= j ? ai_idx(K, i, j) : ai_idx(K, j, i);
            A[i][j] = sh[k] - ms[k];
            A[i][K + j] = i == j ? 1.0 : 0.0;
        }
    // y - y_mean = y' - d, d = sum y' / n: the centred right-hand side is sum x_k y' - d sum x_k
    const double d = rhs[0] / (double)n;
    double th[K];
    double yc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) yc[k] = rhs[k] - d * A[0][k];
    bool ok = status == 0 && n >= K && ai_invert<K>(A);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) s += A[i][K + j] * yc[j];
        th[i] = s;
        ok = ok && isfinite(s);
    }
    const double lv = pivot[o] + d + th[0];
    ok = ok && isfinite(lv);
#pragma unroll
    for (int k = 0; k < K; ++k) theta[k * img + o] = ok ? th[k] : NAN;
    level[o] = ok ? lv : NAN;
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        cinv[(3 * m) * img + o] = ok ? A[2 * m + 1][K + 2 * m + 1] : NAN;
        cinv[(3 * m + 1) * img + o] = ok ? A[2 * m + 1][K + 2 * m + 2] : NAN;
        cinv[(3 * m + 2) * img + o] = ok ? A[2 * m + 2][K + 2 * m + 2] : NAN;
    }
    n_used[o] = status == 0 ? (int)n : 0;
}

// Workgroup (chunk, b), the chunking of the accumulation: pchi[b][chunk][p] = sum over the pixel's values of (y - model)^2,
// model = level + sum_m theta_s,m sin(m x) + theta_c,m cos(m x).  A cutout that was not fitted is not read.
template <int NT>
__global__ __launch_bounds__(AI_T) void cube_ampimage_resid_kernel(const float *__restrict__ flux, const double *__restrict__ trig,
                                                                   const uint8_t *__restrict__ valid,
                                                                   const double *__restrict__ theta,
                                                                   const double *__restrict__ level,
                                                                   const int *__restrict__ fit_status, int B, int N, int npix,
                                                                   int chunks, double *__restrict__ pchi) {
    __shared__ double sh_x[AI_CHUNK * 2 * NT];
    __shared__ uint8_t sh_valid[AI_CHUNK];
    const int b = blockIdx.y, ch = blockIdx.x, c0 = ch * AI_CHUNK, rows = min(AI_CHUNK, N - c0);
    const size_t row0 = (size_t)b * N + c0, slot = (size_t)b * chunks + ch, img = (size_t)B * npix;
    const bool fitted = fit_status[b] == 0;
    if (fitted) ai_stage<NT>(trig, valid, row0, rows, sh_x, sh_valid);
    const float *fl = flux + row0 * npix;
    for (int p = threadIdx.x; p < npix; p += AI_T) {
        double chi = 0.0;
        if (fitted) {
            const size_t o = (size_t)b * npix + p;
            const double lv = level[o];
            double th[2 * NT];
#pragma unroll
            for (int k = 0; k < 2 * NT; ++k) th[k] = theta[(k + 1) * img + o];
            for (int j0 = 0; j0 < rows; j0 += AI_ROWS) {
                float v[AI_ROWS];
#pragma unroll
                for (int u = 0; u < AI_ROWS; ++u) v[u] = sh_valid[j0 + u] ? fl[(size_t)(j0 + u) * npix + p] : 0.0f;
#pragma unroll
                for (int u = 0; u < AI_ROWS; ++u) {
                    if (!sh_valid[j0 + u] || isnan(v[u])) continue;
                    const double *x = sh_x + (j0 + u) * 2 * NT;
                    double per = 0.0;
#pragma unroll
                    for (int k = 0; k < 2 * NT; ++k) per += th[k] * x[k];
                    const double res = (double)v[u] - (lv + per);
                    chi += res * res;
                }
            }
        }
        pchi[slot * npix + p] = chi;
    }
}

// One thread per pixel: chi2 = the chunks' partials in index order (NaN for a pixel without a fit), then per harmonic
// amplitude = hypot(s, c), phase = atan2(c, s), amplitude_err = sqrt(sigma2 (s^2 C_ss + 2 s c C_sc + c^2 C_cc)) / amplitude with
// sigma2 = chi2 / (n_used - K) (NaN for n_used == K), snr = amplitude / amplitude_err.  Harmonic-major images [nterms][B][npix].
template <int NT>
__global__ __launch_bounds__(AI_T) void cube_ampimage_images_kernel(const double *__restrict__ pchi, const double *__restrict__ theta,
                                                                    const double *__restrict__ level,
                                                                    const double *__restrict__ cinv, const int *__restrict__ n_used,
                                                                    int B, int npix, int chunks, double *__restrict__ chi2,
                                                                    double *__restrict__ amplitude, double *__restrict__ phase,
                                                                    double *__restrict__ amplitude_err, double *__restrict__ snr) {
    constexpr int K = 2 * NT + 1;
    const int b = blockIdx.y, p = blockIdx.x * AI_T + threadIdx.x;
    if (p >= npix) return;
    const size_t o = (size_t)b * npix + p, img = (size_t)B * npix;
    double chi = 0.0;
    for (int ch = 0; ch < chunks; ++ch) chi += pchi[((size_t)b * chunks + ch) * npix + p];
    if (level[o] != level[o]) chi = NAN;
    chi2[o] = chi;
    const int n = n_used[o];
    const double sigma2 = n > K ? chi / (double)(n - K) : NAN;
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        const double s = theta[(2 * m + 1) * img + o], c = theta[(2 * m + 2) * img + o];
        const double a = hypot(s, c);
        const double var = sigma2 * (s * s * cinv[(3 * m) * img + o] + 2.0 * s * c * cinv[(3 * m + 1) * img + o] +
                                     c * c * cinv[(3 * m + 2) * img + o]);
        const double e = sqrt(var) / a;
        amplitude[m * img + o] = a;
        phase[m * img + o] = atan2(c, s);
        amplitude_err[m * img + o] = e;
        snr[m * img + o] = a / e;
    }
}

namespace {

struct AiBuffers {
    const double *par, *pivot;
    double *trig, *cshared, *psum, *pmiss, *pchi, *cinv;
    uint8_t *valid;
    int *n_valid, *pcnt;
};

template <int NT>
void ai_launch(int B, int N, int npix, int chunks, const float *flux, const AiBuffers &s, double *theta, double *level,
               double *amplitude, double *phase, double *amplitude_err, double *snr, double *chi2, int *n_used, int *fit_status,
               hipStream_t stream) {
    const dim3 by_chunk(chunks, B), by_pixel((npix + AI_T - 1) / AI_T, B);
    hipLaunchKernelGGL(cube_ampimage_accum_kernel<NT>, by_chunk, dim3(AI_T), 0, stream, flux, (const double *)s.trig,
                       (const uint8_t *)s.valid, s.pivot, N, npix, chunks, s.cshared, s.pcnt, s.psum, s.pmiss);
    hipLaunchKernelGGL(cube_ampimage_finish_kernel<NT>, by_pixel, dim3(AI_T), 0, stream, s.par, (const int *)s.n_valid, s.pivot,
                       (const double *)s.cshared, (const int *)s.pcnt, (const double *)s.psum, (const double *)s.pmiss, B, npix,
                       chunks, theta, level, s.cinv, n_used, fit_status);
    hipLaunchKernelGGL(cube_ampimage_resid_kernel<NT>, by_chunk, dim3(AI_T), 0, stream, flux, (const double *)s.trig,
                       (const uint8_t *)s.valid, (const double *)theta, (const double *)level, (const int *)fit_status, B, N, npix,
                       chunks, s.pchi);
    hipLaunchKernelGGL(cube_ampimage_images_kernel<NT>, by_pixel, dim3(AI_T), 0, stream, (const double *)s.pchi,
                       (const double *)theta, (const double *)level, (const double *)s.cinv, (const int *)n_used, B, npix, chunks,
                       chi2, amplitude, phase, amplitude_err, snr);
}

}  // namespace

int cube_ampimage_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency_host,
                         int nterms, const double *t_ref_host, double *theta, double *level, double *amplitude, double *phase,
                         double *amplitude_err, double *snr, double *chi2, int32_t *n_used, int32_t *fit_status,
                         hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(nterms >= 1 && nterms <= AI_MAX_TERMS, "nterms must be 1 .. %d (got %d)", AI_MAX_TERMS, nterms);
    LK_REQUIRE(time && flux && frequency_host && t_ref_host, "NULL input");
    LK_REQUIRE(theta && level && amplitude && phase && amplitude_err && snr && chi2 && n_used && fit_status, "NULL output buffer");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    const int chunks = (N + AI_CHUNK - 1) / AI_CHUNK, K = 2 * nterms + 1, tri = ai_tri(K);
    const size_t slots = (size_t)B * chunks;
    std::vector<double> par((size_t)2 * B);
    for (int b = 0; b < B; ++b) {
        par[b] = frequency_host[b];
        par[(size_t)B + b] = t_ref_host[b];
    }
    double *d_par, *d_pivot;
    AiBuffers s;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)par.data(), par.size())
                           .buf(s.trig, (size_t)B * N * 2 * nterms)
                           .buf(d_pivot, (size_t)B * npix)
                           .buf(s.cshared, slots * tri)
                           .buf(s.psum, slots * K * npix)
                           .buf(s.pmiss, slots * tri * npix)
                           .buf(s.pchi, slots * npix)
                           .buf(s.cinv, (size_t)3 * nterms * B * npix)
                           .buf(s.pcnt, slots * npix)
                           .buf(s.n_valid, (size_t)B)
                           .buf(s.valid, (size_t)B * N)
                           .carve(stream))
        return rc;
    s.par = d_par;
    s.pivot = d_pivot;
    LK_HIP_CHECK(hipMemsetAsync(s.n_valid, 0, (size_t)B * 4, stream));
    hipLaunchKernelGGL(cube_ampimage_trig_kernel, dim3((N + 255) / 256, B), dim3(256), 0, stream, time, (const double *)d_par, B, N,
                       nterms, s.trig, s.valid, s.n_valid);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cube_ampimage_pivot_kernel, dim3((npix + AI_T - 1) / AI_T, B), dim3(AI_T), 0, stream, flux,
                       (const uint8_t *)s.valid, N, npix, d_pivot);
    LK_HIP_CHECK(hipGetLastError());
    switch (nterms) {
    case 1:
        ai_launch<1>(B, N, npix, chunks, flux, s, theta, level, amplitude, phase, amplitude_err, snr, chi2, (int *)n_used,
                     (int *)fit_status, stream);
        break;
    case 2:
        ai_launch<2>(B, N, npix, chunks, flux, s, theta, level, amplitude, phase, amplitude_err, snr, chi2, (int *)n_used,
                     (int *)fit_status, stream);
        break;
    default:
        ai_launch<3>(B, N, npix, chunks, flux, s, theta, level, amplitude, phase, amplitude_err, snr, chi2, (int *)n_used,
                     (int *)fit_status, stream);
        break;
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
