// pgsmooth.hip — Periodogram.smooth / Periodogram.flatten on gfx950.
//
// Reference: src/lightkurve/periodogram.py:182-284 (smooth: 'boxkernel' = astropy.convolution.convolve with a
// Box1DKernel, 'logmedian' = moving nanmedian in log10(frequency) windows) and :381-429 (flatten = power / smooth).
// The reference's logmedian is a Python while-loop with one np.nanmedian per window; here every (window, target) pair
// is one workgroup running the radix select of block_select.hpp, and a second kernel averages, for every frequency,
// the medians of the windows that contain it — in window order, like the reference's `bkg[m] += ...`.
// The window bookkeeping (which frequencies fall in window k, which windows contain frequency j) depends only on the
// frequency grid and is prepared by the caller exactly as the reference does it (numpy log10, the same running sum
// for the window centres): see lightkurve_amd/periodogram.py::_logmedian_windows.
// Compiled with -ffp-contract=off: products and sums round separately, as in astropy's C convolution loop.
#include "block_select.hpp"
#include "lk_common.hpp"

namespace lk {

// one workgroup per (window k, target b): med[b][k] = nanmedian(power[b][lo_k : hi_k]) / corr
__global__ __launch_bounds__(256) void pg_window_median_kernel(const double *__restrict__ power, int64_t M,
                                                                const int *__restrict__ win_lo,
                                                                const int *__restrict__ win_hi, int K, double corr,
                                                                double *__restrict__ med) {
    __shared__ unsigned long long sh[264];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lo = win_lo[k], n = win_hi[k] - lo;
    const double *row = power + (size_t)b * (size_t)M + lo;
    auto val = [&](int i) { return row[i]; };
    auto keep = [&](int i) { return !isnan(row[i]); };
    long long c = 0;
    for (int i = tid; i < n; i += 256) c += keep(i) ? 1 : 0;
    const long long cnt = block_count_dyn(c, reinterpret_cast<long long *>(sh));
    const double m = block_median(n, cnt, val, keep, sh);  // NaN if nothing is kept (np.nanmedian of all-NaN)
    if (tid == 0) med[(size_t)b * K + k] = m / corr;
}

// out[b][j] = (sum over the windows klo_j..khi_j that contain j, in window order) / (number of those windows)
__global__ __launch_bounds__(256) void pg_window_average_kernel(const double *__restrict__ med, int K,
                                                                 const int *__restrict__ klo,
                                                                 const int *__restrict__ khi, int64_t M,
                                                                 double *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int a = klo[j], z = khi[j];
    double s = 0.0;
    for (int k = a; k <= z; ++k) s += med[(size_t)b * K + k];
    out[(size_t)b * (size_t)M + j] = s / (double)(z - a + 1);  // no window: 0/0 = NaN like the reference
}

// per target: does the row hold a NaN?  (astropy: nan_interpolate = isnan(array.sum()))
__global__ __launch_bounds__(256) void pg_has_nan_kernel(const double *__restrict__ power, int64_t M,
                                                          int *__restrict__ flag) {
    const int b = blockIdx.x;
    const double *row = power + (size_t)b * (size_t)M;
    int f = 0;
    for (int64_t j = threadIdx.x; j < M; j += 256) f |= isnan(row[j]) ? 1 : 0;
    f = __syncthreads_or(f);
    if (threadIdx.x == 0) flag[b] = f;
}

// astropy.convolution.convolve(power, kernel): boundary='fill' (zeros), normalize_kernel=True,
// nan_treatment='interpolate'.  taps = the (already flipped) kernel, ksum = its sum.
__global__ __launch_bounds__(256) void pg_boxsmooth_kernel(const double *__restrict__ power, int64_t M,
                                                            const double *__restrict__ taps, int nk, double ksum,
                                                            const int *__restrict__ has_nan,
                                                            double *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double *row = power + (size_t)b * (size_t)M;
    const int half = nk / 2;
    double top = 0.0;
    if (!has_nan[b]) {
        for (int ii = 0; ii < nk; ++ii) {
            const int64_t idx = j + ii - half;
            const double v = (idx >= 0 && idx < M) ? row[idx] : 0.0;
            top += v * taps[ii];
        }
        out[(size_t)b * (size_t)M + j] = top / ksum;
    } else {
        double bot = 0.0;
        for (int ii = 0; ii < nk; ++ii) {
            const int64_t idx = j + ii - half;
            const double v = (idx >= 0 && idx < M) ? row[idx] : 0.0;
            if (!isnan(v)) {
                top += v * taps[ii];
                bot += taps[ii];
            }
        }
        out[(size_t)b * (size_t)M + j] = bot != 0.0 ? top / bot : __longlong_as_double(0x7ff8000000000000ll);
    }
}

int pg_logmedian_launch(lk_handle *h, int B, int64_t M, const double *power, int K, const int *win_lo_host,
                        const int *win_hi_host, const int *klo_host, const int *khi_host, double corr, double *out,
                        hipStream_t stream) {
    LK_REQUIRE(B >= 0 && M >= 1 && K >= 0, "need B >= 0, M >= 1, K >= 0");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && out && klo_host && khi_host, "NULL buffer");
    LK_REQUIRE(K == 0 || (win_lo_host && win_hi_host), "NULL window table");
    LK_REQUIRE(M < ((int64_t)1 << 31), "M too large");
    LK_REQUIRE(B <= 65535, "at most 65535 periodograms per call (got %d)", B);
    for (int k = 0; k < K; ++k)
        LK_REQUIRE(win_lo_host[k] >= 0 && win_lo_host[k] <= win_hi_host[k] && win_hi_host[k] <= M,
                   "window %d = [%d, %d) outside [0, M]", k, win_lo_host[k], win_hi_host[k]);
    for (int64_t j = 0; j < M; ++j)
        LK_REQUIRE(klo_host[j] >= 0 && khi_host[j] < K + (K == 0) && klo_host[j] <= khi_host[j] + 1,
                   "frequency %lld lists windows [%d, %d] outside [0, K)", (long long)j, klo_host[j], khi_host[j]);
    int *d_lo, *d_hi, *d_klo, *d_khi;
    double *d_med;
    if (const int rc = Scratch(h, h->ws).buf(d_lo, K + 1).buf(d_hi, K + 1).buf(d_klo, M).buf(d_khi, M)
            .buf(d_med, (size_t)B * (size_t)(K + 1)).carve(stream))
        return rc;
    if (K) {
        LK_HIP_CHECK(hipMemcpyAsync(d_lo, win_lo_host, (size_t)K * 4, hipMemcpyHostToDevice, stream));
        LK_HIP_CHECK(hipMemcpyAsync(d_hi, win_hi_host, (size_t)K * 4, hipMemcpyHostToDevice, stream));
    }
    LK_HIP_CHECK(hipMemcpyAsync(d_klo, klo_host, (size_t)M * 4, hipMemcpyHostToDevice, stream));
    LK_HIP_CHECK(hipMemcpyAsync(d_khi, khi_host, (size_t)M * 4, hipMemcpyHostToDevice, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));  // the host tables belong to the caller
    if (K)
        hipLaunchKernelGGL(pg_window_median_kernel, dim3((unsigned)K, (unsigned)B), dim3(256), 0, stream, power, M, d_lo,
                           d_hi, K, corr, d_med);
    hipLaunchKernelGGL(pg_window_average_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                       d_med, K, d_klo, d_khi, M, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int pg_boxsmooth_launch(lk_handle *h, int B, int64_t M, const double *power, const double *taps_host, int nk,
                        double *out, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && M >= 1, "need B >= 0 and M >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && out && taps_host, "NULL buffer");
    LK_REQUIRE(nk >= 1 && nk % 2 == 1, "the kernel must have an odd number of taps");
    LK_REQUIRE(B <= 65535, "at most 65535 periodograms per call (got %d)", B);
    double ksum = 0.0;
    for (int i = 0; i < nk; ++i) ksum += taps_host[i];
    LK_REQUIRE(ksum > 1e-8, "The kernel can't be normalized, because its sum is close to zero.");
    double *d_taps;
    int *d_flag;
    if (const int rc = Scratch(h, h->ws).buf(d_taps, nk).buf(d_flag, B).carve(stream)) return rc;
    LK_HIP_CHECK(hipMemcpyAsync(d_taps, taps_host, (size_t)nk * 8, hipMemcpyHostToDevice, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    hipLaunchKernelGGL(pg_has_nan_kernel, dim3(B), dim3(256), 0, stream, power, M, d_flag);
    hipLaunchKernelGGL(pg_boxsmooth_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream, power,
                       M, d_taps, nk, ksum, d_flag, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ seismology 2-D ACF
// estimate_numax_acf2d (reference src/lightkurve/seismology/numax_estimators.py:15-205) slides a window of W = 2 spread
// samples over the spectrum and, for every central frequency, takes the full autocorrelation of the mean-subtracted
// window (seismology/utils.py:106-158: p_sel -= nanmean(p_sel); C = np.correlate(p_sel, p_sel, "full")[W - 1:]) and the
// "mean collapsed correlation" (sum |C| - 1) / W.  One workgroup per (window, periodogram): the window lives in LDS, a
// thread owns four consecutive lags and slides a four-value register window over the samples (one broadcast read and one
// new sample per four FMAs).  W^2 / 2 MACs per window, everything on chip; HBM traffic is W in and W out per window.
// The numax estimator reads `metric` alone: the STORE = false instantiation (lk_pg_acf_metric_batch_dev) is the same
// arithmetic without the W doubles of `acf2d` per window.  The deltanu kernel further down shares the two helpers, so
// every lag it forms has the bits the 2-D kernel gives the same window.

// p[0 .. W) = the window minus its nanmean, p[W .. W + 8) = 0; red = 8 doubles of scratch.  Ends behind a barrier.
__device__ __forceinline__ void acf_load_window(const double *__restrict__ src, int W, double *p, double *red) {
    const int tid = threadIdx.x;
    double s = 0.0;
    long long c = 0;
    for (int i = tid; i < W; i += 256) {
        const double v = src[i];
        p[i] = v;
        if (!isnan(v)) {
            s += v;
            ++c;
        }
    }
    if (tid < 8) p[W + tid] = 0.0;  // the register window runs up to three samples past the end
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        c += __shfl_xor(c, o);
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        red[tid >> 6] = s;
        red[4 + (tid >> 6)] = (double)c;
    }
    __syncthreads();
    const double mean = (red[0] + red[1] + red[2] + red[3]) / (red[4] + red[5] + red[6] + red[7]);
    __syncthreads();
    for (int i = tid; i < W; i += 256) p[i] -= mean;  // NaN samples stay NaN (and poison every lag, as in numpy)
    __syncthreads();
}

// a[r] = C[l0 + r] = sum_{i < W - l0 - r} p[i] p[i + l0 + r], r < 4 and 0 <= l0 < W: every lag is one fma chain over
// ascending i, whatever group it is computed in; terms past the window's end multiply the zero pad
__device__ __forceinline__ void acf_four_lags(const double *p, int W, int l0, double &a0, double &a1, double &a2,
                                              double &a3) {
    a0 = a1 = a2 = a3 = 0.0;
    double q0 = p[l0], q1 = p[l0 + 1], q2 = p[l0 + 2], q3 = p[l0 + 3];
    const int n_i = W - l0;
    int i = 0;
    for (; i < n_i - 3; ++i) {  // all four lags have a partner inside the window
        const double x = p[i];
        a0 = fma(x, q0, a0);
        a1 = fma(x, q1, a1);
        a2 = fma(x, q2, a2);
        a3 = fma(x, q3, a3);
        q0 = q1;
        q1 = q2;
        q2 = q3;
        q3 = p[i + l0 + 4];
    }
    for (; i < n_i; ++i) {  // last three samples: lag l0 + r only pairs samples i < W - l0 - r (no 0 * NaN terms)
        const double x = p[i];
        a0 = fma(x, q0, a0);
        if (i < n_i - 1) a1 = fma(x, q1, a1);
        if (i < n_i - 2) a2 = fma(x, q2, a2);
        q0 = q1;
        q1 = q2;
        q2 = q3;
        q3 = 0.0;
    }
}

template <bool STORE>
__global__ __launch_bounds__(256) void pg_acf2d_kernel(const double *__restrict__ power, int64_t M,
                                                        const int *__restrict__ win_start, int n_win, int W,
                                                        double *__restrict__ acf2d, double *__restrict__ metric) {
    extern __shared__ __attribute__((aligned(16))) double acf_lds[];  // W + 8 samples | 8 doubles of reduction scratch
    double *p = acf_lds, *red = acf_lds + W + 8;
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    acf_load_window(power + (size_t)b * (size_t)M + win_start[w], W, p, red);
    double *out = STORE ? acf2d + ((size_t)b * n_win + w) * (size_t)W : nullptr;
    double msum = 0.0;
    // lags l0 .. l0 + 3; groups are dealt from both ends (short and long lags alternate) to balance the triangle
    const int ngrp = (W + 3) / 4;
    for (int g = tid; g < ngrp; g += 256) {
        const int gg = (g & 1) ? (ngrp - 1 - (g >> 1)) : (g >> 1);
        const int l0 = 4 * gg;
        double a0, a1, a2, a3;
        acf_four_lags(p, W, l0, a0, a1, a2, a3);
        if (STORE) {
            if (l0 < W) out[l0] = a0;
            if (l0 + 1 < W) out[l0 + 1] = a1;
            if (l0 + 2 < W) out[l0 + 2] = a2;
            if (l0 + 3 < W) out[l0 + 3] = a3;
        }
        if (l0 < W) msum += fabs(a0);
        if (l0 + 1 < W) msum += fabs(a1);
        if (l0 + 2 < W) msum += fabs(a2);
        if (l0 + 3 < W) msum += fabs(a3);
    }
    for (int o = 32; o > 0; o >>= 1) msum += __shfl_xor(msum, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = msum;
    __syncthreads();
    if (tid == 0) metric[(size_t)b * n_win + w] = ((red[0] + red[1] + red[2] + red[3]) - 1.0) / (double)W;
}

// acf2d == nullptr: the metric alone
static int acf2d_launch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int *win_start_host, int W,
                        double *acf2d, double *metric, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && M >= 1 && n_win >= 0, "need B >= 0, M >= 1, n_win >= 0");
    if (B == 0 || n_win == 0) return LK_OK;
    LK_REQUIRE(power && win_start_host && metric, "NULL buffer");
    LK_REQUIRE(W >= 1 && W <= 16384, "window of %d samples outside 1..16384", W);
    LK_REQUIRE(B <= 65535, "at most 65535 periodograms per call");
    for (int k = 0; k < n_win; ++k)
        LK_REQUIRE(win_start_host[k] >= 0 && (int64_t)win_start_host[k] + W <= M, "window %d = [%d, %d) outside [0, M)", k,
                   win_start_host[k], win_start_host[k] + W);
    int *d_start;
    if (const int rc = Scratch(h, h->ws).buf(d_start, n_win).carve(stream)) return rc;
    LK_HIP_CHECK(hipMemcpyAsync(d_start, win_start_host, (size_t)n_win * 4, hipMemcpyHostToDevice, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    auto *kernel = acf2d ? pg_acf2d_kernel<true> : pg_acf2d_kernel<false>;
    {
        const int rc_ = want_lds(h, reinterpret_cast<const void *>(kernel), 160 * 1024);
        if (rc_) return rc_;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_win, (unsigned)B), dim3(256), (size_t)(W + 16) * 8, stream, power, M,
                       d_start, n_win, W, acf2d, metric);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int pg_acf2d_launch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int *win_start_host, int W,
                    double *acf2d, double *metric, hipStream_t stream) {
    LK_REQUIRE(B == 0 || n_win == 0 || acf2d, "NULL buffer");
    return acf2d_launch(h, B, M, power, n_win, win_start_host, W, acf2d, metric, stream);
}

int pg_acf_metric_launch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int *win_start_host, int W,
                         double *metric, hipStream_t stream) {
    return acf2d_launch(h, B, M, power, n_win, win_start_host, W, nullptr, metric, stream);
}

// ------------------------------------------------------------------------------------------------ SNR = power / background
// Periodogram.flatten's one division (reference periodogram.py:381-429), IEEE double like numpy's.  V2: two doubles per
// lane through 16-byte accesses (every pointer 16-byte aligned), the odd last element alone.
template <bool V2>
__global__ __launch_bounds__(256) void pg_divide_kernel(const double *__restrict__ num, const double *__restrict__ den,
                                                         int64_t n, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (V2) {
        const int64_t i = 2 * t;
        if (i + 1 < n) {
            const double2 a = *reinterpret_cast<const double2 *>(num + i), d = *reinterpret_cast<const double2 *>(den + i);
            *reinterpret_cast<double2 *>(out + i) = make_double2(a.x / d.x, a.y / d.y);
        } else if (i < n) {
            out[i] = num[i] / den[i];
        }
    } else if (t < n) {
        out[t] = num[t] / den[t];
    }
}

int pg_snr_launch(lk_handle *h, int B, int64_t M, const double *power, const double *bkg, double *out,
                  hipStream_t stream) {
    LK_REQUIRE(B >= 0 && M >= 1, "need B >= 0 and M >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && bkg && out, "NULL buffer");
    const int64_t n = (int64_t)B * M;
    const bool v2 = ((reinterpret_cast<uintptr_t>(power) | reinterpret_cast<uintptr_t>(bkg) |
                      reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t blocks = ((v2 ? (n + 1) / 2 : n) + 255) / 256;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "B * M too large");
    if (v2)
        hipLaunchKernelGGL(pg_divide_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, power, bkg, n, out);
    else
        hipLaunchKernelGGL(pg_divide_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, power, bkg, n, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ numax: smooth + argmax
// is `a` ahead of `b`?  (value, index) pairs, index < 0 = none.  np.argmax order: a NaN is the maximum, then the larger
// value; the lower index wins among equals.  A strict total order, so a butterfly leaves every lane with the same pair.
struct ArgmaxFirst {
    __device__ bool operator()(double av, int ak, double bv, int bk) const {
        if (ak < 0) return false;
        if (bk < 0) return true;
        const bool an = isnan(av), bn = isnan(bv);
        if (an || bn) return an && (!bn || ak < bk);
        return av > bv || (av == bv && ak < bk);
    }
};

// the pair every thread holds -> the best of the workgroup in every thread; sv / sk: 4 doubles / 4 ints of LDS
template <class Ahead>
__device__ __forceinline__ void block_best(double &v, int &k, Ahead ahead, double *sv, int *sk) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int ok = __shfl_xor(k, o);
        if (ahead(ov, ok, v, k)) {
            v = ov;
            k = ok;
        }
    }
    const int tid = threadIdx.x;
    __syncthreads();  // the scratch may still be read from the previous call
    if ((tid & 63) == 0) {
        sv[tid >> 6] = v;
        sk[tid >> 6] = k;
    }
    __syncthreads();
    v = sv[0];
    k = sk[0];
    for (int w = 1; w < 4; ++w)
        if (ahead(sv[w], sk[w], v, k)) {
            v = sv[w];
            k = sk[w];
        }
}

// The tail of estimate_numax_acf2d (numax_estimators.py:181-186) for one target per workgroup: with nk > 0,
// metric_smooth = astropy.convolution.convolve(metric, Gaussian1DKernel(sqrt(n_win)), boundary='extend') — taps = the
// normalised kernel, seismology._gaussian_taps, edges replicated, summed in tap order — else metric_smooth = metric;
// arg = np.argmax(metric_smooth).  metric_smooth may be metric itself when nk == 0.
__global__ __launch_bounds__(256) void pg_numax_pick_kernel(const double *metric, int n_win,
                                                             const double *__restrict__ taps, int nk,
                                                             double *metric_smooth, int64_t *__restrict__ arg) {
    __shared__ double sv[4];
    __shared__ int sk[4];
    const int b = blockIdx.x, tid = threadIdx.x, half = nk / 2;
    const double *row = metric + (size_t)b * n_win;
    double *out = metric_smooth + (size_t)b * n_win;
    double bv = 0.0;
    int bk = -1;
    for (int i = tid; i < n_win; i += 256) {
        double s = row[i];
        if (nk) {
            s = 0.0;
            for (int k = 0; k < nk; ++k) s += row[min(max(i + k - half, 0), n_win - 1)] * taps[k];
        }
        out[i] = s;
        if (ArgmaxFirst()(s, i, bv, bk)) {
            bv = s;
            bk = i;
        }
    }
    block_best(bv, bk, ArgmaxFirst(), sv, sk);
    if (tid == 0) arg[b] = bk;
}

int pg_numax_pick_launch(lk_handle *h, int B, int n_win, const double *metric, const double *taps_host, int nk,
                         double *metric_smooth, int64_t *argmax_out, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_win >= 1, "need B >= 0 and n_win >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(metric && metric_smooth && argmax_out, "NULL buffer");
    LK_REQUIRE(nk == 0 || (taps_host && nk % 2 == 1), "the kernel must have an odd number of taps (or none)");
    LK_REQUIRE(nk == 0 || metric_smooth != metric, "metric_smooth may alias metric only without taps");
    double *d_taps;
    if (const int rc = Scratch(h, h->ws).upload(d_taps, taps_host, (size_t)nk, nk > 0).carve(stream)) return rc;
    hipLaunchKernelGGL(pg_numax_pick_kernel, dim3((unsigned)B), dim3(256), 0, stream, metric, n_win, d_taps, nk,
                       metric_smooth, argmax_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ deltanu, ragged
// estimate_deltanu_acf2d (reference src/lightkurve/seismology/deltanu_estimators.py:18-153) for one target per
// workgroup, each with its OWN window: start / W samples around its numax (one envelope FWHM either side), the lags
// np.linspace(0, W fs, W) = i * step with the last one set to stop, and the empirical deltanu.  The caller derives these
// from numax with the reference's scalar arithmetic (seismology._deltanu_plan); the kernel does what depends on the
// spectrum.  The reference takes all W lags of the window and reads lag 0 and the lags within 25 % of the empirical
// deltanu; only those are formed here, by the helpers of the 2-D kernel (the same bits as its lags of this window):
//   sel  = lag > emp - 0.25 emp and lag < emp + 0.25 emp          (the reference's expression; no contraction here)
//   acf  = (|C^2| / |C[0]^2|) / (3 / (2 W))                        on sel
//   peaks = scipy.signal.find_peaks(acf[sel], distance=distance): _local_maxima_1d (midpoint of a plateau, neither end of
//           the slice), then _select_by_peak_distance with ceil(distance): the highest peak first, its neighbours
//           closer than that dropped
//   deltanu = the lag of the surviving peak closest to emp, the first of equally close ones.
// scipy orders peaks of EXACTLY equal height by an unstable argsort; here the later one goes first, which is what a
// stable argsort gives and what scipy itself does on short peak lists (tests/test_seismology_exact_gpu.py, the
// equal-heights cases of tests/seismology_cases.py: two and three equal maxima closer than the distance).
// status: 0 ok; 1 skipped (emp is NaN: the caller's mark for a numax that is NaN or <= 0); 2 the window is not inside
// [0, M), is shorter than 2 or longer than 16384 samples, or does not fit the workgroup's LDS together with its
// selection; 3 nothing to pick: no local maximum inside the selection (fewer than 3 lags, a constant window or a NaN in
// it among the causes), or distance < 1 or NaN (where scipy raises).
// LDS (doubles): W + 8 window | 8 scratch | the selected slice.  The window's space holds the peak list afterwards.
__device__ __forceinline__ void block_min_sum(int &mn, int &sum, int *scratch) {
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o));
        sum += __shfl_xor(sum, o);
    }
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) {
        scratch[tid >> 6] = mn;
        scratch[4 + (tid >> 6)] = sum;
    }
    __syncthreads();
    mn = min(min(scratch[0], scratch[1]), min(scratch[2], scratch[3]));
    sum = scratch[4] + scratch[5] + scratch[6] + scratch[7];
}

// higher peak first, the later of equal ones
struct PeakHigher {
    __device__ bool operator()(double av, int ak, double bv, int bk) const {
        if (ak < 0) return false;
        if (bk < 0) return true;
        return av > bv || (av == bv && ak > bk);
    }
};
// np.argmin of a distance: smaller first, the earlier of equal ones
struct Closer {
    __device__ bool operator()(double av, int ak, double bv, int bk) const {
        if (ak < 0) return false;
        if (bk < 0) return true;
        return av < bv || (av == bv && ak < bk);
    }
};

__global__ __launch_bounds__(256) void pg_deltanu_kernel(const double *__restrict__ power, int64_t M,
                                                          const int *__restrict__ start, const int *__restrict__ width,
                                                          const double *__restrict__ emp_v,
                                                          const double *__restrict__ distance_v,
                                                          const double *__restrict__ step_v,
                                                          const double *__restrict__ stop_v, int lds_doubles, int max_sel,
                                                          double *__restrict__ deltanu, int *__restrict__ n_peaks,
                                                          int *__restrict__ status, int *__restrict__ sel_lo_out,
                                                          int *__restrict__ sel_len_out, double *__restrict__ acf_out) {
    extern __shared__ __attribute__((aligned(16))) double acf_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double emp = emp_v[b], step = step_v[b], stop = stop_v[b], distance = distance_v[b];
    const int W = width[b], st = start[b];
    if (acf_out)
        for (int j = tid; j < max_sel; j += 256) acf_out[(size_t)b * max_sel + j] = qnan;
    int sel_lo = 0, n = 0, n_kept = 0;
    double best = qnan;
    // every exit below is taken by the whole workgroup: its conditions are uniform
    int stat = isnan(emp) ? 1 : (st < 0 || W < 2 || W > 16384 || (int64_t)st + W > M || W + 16 > lds_doubles) ? 2 : 0;
    double *p = acf_lds, *red = acf_lds + W + 8, *x = red + 8;
    auto lag = [&](int i) { return i == W - 1 ? stop : (double)i * step; };
    if (stat == 0) {
        const double lo_t = emp - 0.25 * emp, hi_t = emp + 0.25 * emp;
        sel_lo = W;
        for (int i = tid; i < W; i += 256) {
            const double l = lag(i);
            if (l > lo_t && l < hi_t) {
                sel_lo = min(sel_lo, i);
                ++n;
            }
        }
        block_min_sum(sel_lo, n, reinterpret_cast<int *>(red));
        if (n == 0) sel_lo = 0;
        if (W + 16 + n > lds_doubles) stat = 2;
        else if (n < 3 || !(distance >= 1.0)) stat = 3;
    }
    if (stat == 0) {
        acf_load_window(power + (size_t)b * (size_t)M + st, W, p, red);
        const int ngrp = (n + 3) / 4;
        for (int g = tid; g <= ngrp; g += 256) {  // group ngrp: lag 0
            const int l0 = g == ngrp ? 0 : sel_lo + 4 * g;
            double a0, a1, a2, a3;
            acf_four_lags(p, W, l0, a0, a1, a2, a3);
            if (g == ngrp) {
                red[0] = a0;
            } else {
                const int j = 4 * g;
                x[j] = a0;
                if (j + 1 < n) x[j + 1] = a1;
                if (j + 2 < n) x[j + 2] = a2;
                if (j + 3 < n) x[j + 3] = a3;
            }
        }
        __syncthreads();  // the window is dead from here on
        const double c0 = red[0], den = fabs(c0 * c0), noise = 3.0 / (2.0 * (double)W);
        for (int j = tid; j < n; j += 256) {
            const double c = x[j], v = (fabs(c * c) / den) / noise;
            x[j] = v;
            if (acf_out && j < max_sel) acf_out[(size_t)b * max_sel + j] = v;
        }
        __syncthreads();
        // local maxima, in slice order: pk[0 .. n_pk)
        int *pk = reinterpret_cast<int *>(p), *state = pk + n, *wcnt = reinterpret_cast<int *>(red + 1);
        int n_pk = 0;
        for (int c = 0; c < n; c += 256) {
            const int i = c + tid;
            int mid = -1;
            if (i >= 1 && i < n - 1 && x[i - 1] < x[i]) {
                int ahead = i + 1;
                while (ahead < n - 1 && x[ahead] == x[i]) ++ahead;
                if (x[ahead] < x[i]) mid = (i + ahead - 1) / 2;
            }
            const unsigned long long m = __ballot(mid >= 0);
            const int wave = tid >> 6, lane = tid & 63;
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = n_pk;
            for (int w = 0; w < wave; ++w) off += wcnt[w];
            if (mid >= 0) pk[off + __popcll(m & ((1ull << lane) - 1ull))] = mid;
            n_pk += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            __syncthreads();
        }
        for (int k = tid; k < n_pk; k += 256) state[k] = 0;  // 0 undecided, 1 kept, 2 dropped
        __syncthreads();
        const double dist_up = ceil(distance);
        const int dist = dist_up < 2147483647.0 ? (int)dist_up : 2147483647;
        double *sv = red;
        int *sk = reinterpret_cast<int *>(red + 4);
        for (;;) {  // one round per kept peak: the selection is about one `distance` wide, so two or three rounds
            double hv = 0.0;
            int hk = -1;
            for (int k = tid; k < n_pk; k += 256)
                if (state[k] == 0 && PeakHigher()(x[pk[k]], k, hv, hk)) {
                    hv = x[pk[k]];
                    hk = k;
                }
            block_best(hv, hk, PeakHigher(), sv, sk);
            if (hk < 0) break;
            const int at = pk[hk];  // (every thread read this round's states before block_best's barriers)
            for (int k = tid; k < n_pk; k += 256)
                if (k == hk) state[k] = 1;
                else if (state[k] == 0 && abs(pk[k] - at) < dist) state[k] = 2;
            __syncthreads();
        }
        double dv = 0.0;
        int dk = -1, cnt = 0, unused = 0;
        for (int k = tid; k < n_pk; k += 256)
            if (state[k] == 1) {
                ++cnt;
                const double d = fabs(lag(sel_lo + pk[k]) - emp);
                if (Closer()(d, k, dv, dk)) {
                    dv = d;
                    dk = k;
                }
            }
        block_best(dv, dk, Closer(), sv, sk);
        block_min_sum(unused, cnt, reinterpret_cast<int *>(red));
        n_kept = cnt;
        if (dk < 0) stat = 3;
        else best = lag(sel_lo + pk[dk]);
    }
    if (tid == 0) {
        deltanu[b] = best;
        n_peaks[b] = n_kept;
        status[b] = stat;
        sel_lo_out[b] = sel_lo;
        sel_len_out[b] = n;
    }
}

int pg_deltanu_launch(lk_handle *h, int B, int64_t M, const double *power, const int *start_host, const int *width_host,
                      const double *emp_host, const double *distance_host, const double *step_host,
                      const double *stop_host, int max_sel, double *deltanu, int *n_peaks, int *status, int *sel_lo,
                      int *sel_len, double *acf, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && M >= 1 && max_sel >= 0, "need B >= 0, M >= 1, max_sel >= 0");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && start_host && width_host && emp_host && distance_host && step_host && stop_host,
               "NULL per-target table");
    LK_REQUIRE(deltanu && n_peaks && status && sel_lo && sel_len, "NULL output");
    // one LDS size for the launch: the widest valid window plus max_sel, inside 160 KB; a target that needs more is status 2
    int w_max = 2;
    for (int b = 0; b < B; ++b)
        if (width_host[b] <= 16384) w_max = std::max(w_max, width_host[b]);
    const int lds_doubles = (int)std::min<int64_t>((int64_t)w_max + 16 + max_sel, 160 * 1024 / 8);
    int *d_start, *d_width;
    double *d_emp, *d_dist, *d_step, *d_stop;
    if (const int rc = Scratch(h, h->ws).upload(d_start, start_host, B).upload(d_width, width_host, B)
            .upload(d_emp, emp_host, B).upload(d_dist, distance_host, B).upload(d_step, step_host, B)
            .upload(d_stop, stop_host, B).carve(stream))
        return rc;
    {
        const int rc_ = want_lds(h, reinterpret_cast<const void *>(pg_deltanu_kernel), 160 * 1024);
        if (rc_) return rc_;
    }
    hipLaunchKernelGGL(pg_deltanu_kernel, dim3((unsigned)B), dim3(256), (size_t)lds_doubles * 8, stream, power, M, d_start,
                       d_width, d_emp, d_dist, d_step, d_stop, lds_doubles, max_sel, deltanu, n_peaks, status, sel_lo,
                       sel_len, acf);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
