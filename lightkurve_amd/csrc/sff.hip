// sff.hip — SFFCorrector.correct (reference src/lightkurve/correctors/sffcorrector.py, lightkurve 2.x: self-flat-fielding, the K2
// roll-motion correction) for B ragged light curves resident in HBM:
//   sff_arclength   _estimate_arclength: centroids -> arclength along the roll, the flip decided by the sign of the slope;
//   sff_knots       normalise (flux / median), raw mean, std and chunk means for the priors, the long-term spline's percentile
//                   knots of time and every window's percentile knots of arclength (exact order statistics, numpy's _lerp);
//   sff_design      the block-structured design matrix [ spline(time) | window 1 | ... | window W ] and its priors, one row per
//                   cadence, written straight into HBM (no host round trip): the hot kernel;
//   (regress_launch, regress.hip, unchanged: the fit)
//   sff_parts / sff_epilogue   the component models 'spline' and 'sff' with exact medians, restore_trend, the final scaling.
// K must be uniform per regression call, so targets are grouped by (n_knots, W) on the host and every group runs in chunks of
// targets that fit the caller's scratch block; nothing is padded and every kernel works on one target per workgroup (or one
// row per thread), so a target's result has the same bits in any batch and for any chunk size.
// "Outside the window" is decided BY INDEX (cadence not in [lo_j, up_j)); the reference decides it by value
// (~np.in1d(ar, ar[a:b])): the two differ only when an arclength outside the window is bit-equal to one inside it.
#include "lk_common.hpp"

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "block_select.hpp"
#include "spline_basis.hpp"

namespace lk {

constexpr int SFF_NT = 256;
constexpr int SFF_TAB = 6;        // int64 words per target of a chunk's table: offset in the batch, N, offset in the chunk,
                                  // offset of its window points, index in the batch, spare
constexpr int SFF_TDEG = 3;       // degree of the long-term spline (create_spline_matrix's default)
constexpr int SFF_KMAX = 4095;    // widest matrix lk_regress_batch_dev takes

__device__ __forceinline__ double sff_block_min(double x, double *shd) {
    const int tid = threadIdx.x, nt = blockDim.x;
    shd[tid] = x;
    __syncthreads();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        if (tid < s) shd[tid] = fmin(shd[tid], shd[tid + s]);
        __syncthreads();
    }
    const double r = shd[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double sff_block_max(double x, double *shd) { return -sff_block_min(-x, shd); }

// numpy's _lerp(a, b, t) (function_base.py): a + (b - a) t, replaced by b - (b - a)(1 - t) where t >= 0.5
__device__ __forceinline__ double sff_lerp(double a, double b, double t) {
    const double d = __dsub_rn(b, a);
    return t >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t))) : __dadd_rn(a, __dmul_rn(d, t));
}

// np.percentile(a, q_k) for q_k = np.linspace(0, 100, m + 1)[k], 0 < k < m, of the n values val(0..n): numpy's 'linear' method
// (virtual index (n - 1) q, its floor and the next index clipped into the array, _lerp between the two order statistics;
// q_k = k (100 / m) / 100 as linspace and percentile round it).  sorted: val is non-decreasing, the order statistics are plain
// reads.  Called by the whole workgroup.
template <class Val>
__device__ double sff_percentile(int n, int k, int m, Val val, bool sorted, unsigned long long *sh) {
    const double q = __ddiv_rn(__dmul_rn((double)k, __ddiv_rn(100.0, (double)m)), 100.0);
    const double vi = __dmul_rn((double)(n - 1), q);
    const double fl = floor(vi);
    const double g = __dsub_rn(vi, fl);
    const int lo = min(max((int)fl, 0), n - 1), hi = min(max((int)fl + 1, 0), n - 1);
    double a, b;
    if (sorted) {
        a = val(lo);
        b = val(hi);
    } else {
        auto all = [](int) { return true; };
        a = block_select_kth(n, lo, val, all, sh);
        b = hi == lo ? a : block_select_kth(n, hi, val, all, sh);
    }
    return sff_lerp(a, b, g);
}

// ------------------------------------------------------------------------------------------------ (a) arclength
// One workgroup per target.  c = col - min(col), r = row - min(row); the degree-1 least-squares slope of r on c has the sign of
// sum (c - mean c)(r - mean r) (centred sums, added in an order that depends on N alone); negative: c = max(c) - c.
// arc = sqrt(c c + r r), every operation rounded on its own.  info (nullable) b -> {time[0], time[N - 1], count of non-finite
// values among time / flux / flux_err / col / row, flipped}; flipped (nullable) int32[B].
__global__ __launch_bounds__(SFF_NT) void sff_arclength_kernel(const int64_t *__restrict__ off, const double *__restrict__ col,
                                                               const double *__restrict__ row, const double *__restrict__ time,
                                                               const double *__restrict__ flux, const double *__restrict__ err,
                                                               double *__restrict__ arc, double *__restrict__ info,
                                                               int *__restrict__ flipped) {
    __shared__ unsigned long long sh[264];
    double *shd = reinterpret_cast<double *>(sh);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t o = off[b];
    const int N = (int)(off[b + 1] - o);
    if (N <= 0) return;
    const double *cc = col + o, *rr = row + o;
    double mnc = INFINITY, mxc = -INFINITY, mnr = INFINITY;
    long long bad = 0;
    for (int i = tid; i < N; i += SFF_NT) {
        const double c = cc[i], r = rr[i];
        mnc = fmin(mnc, c);
        mxc = fmax(mxc, c);
        mnr = fmin(mnr, r);
        bad += (isfinite(c) ? 0 : 1) + (isfinite(r) ? 0 : 1);
        if (time) bad += isfinite(time[o + i]) ? 0 : 1;
        if (flux) bad += isfinite(flux[o + i]) ? 0 : 1;
        if (err) bad += isfinite(err[o + i]) ? 0 : 1;
    }
    mnc = sff_block_min(mnc, shd);
    mxc = sff_block_max(mxc, shd);
    mnr = sff_block_min(mnr, shd);
    bad = block_count_dyn(bad, reinterpret_cast<long long *>(sh));
    double sc = 0.0, sr = 0.0;
    for (int i = tid; i < N; i += SFF_NT) {
        sc += cc[i] - mnc;
        sr += rr[i] - mnr;
    }
    const double mc = block_sum_dyn(sc, shd) / (double)N, mr = block_sum_dyn(sr, shd) / (double)N;
    double sxy = 0.0;
    for (int i = tid; i < N; i += SFF_NT) sxy += ((cc[i] - mnc) - mc) * ((rr[i] - mnr) - mr);
    sxy = block_sum_dyn(sxy, shd);
    const bool flip = sxy < 0.0;
    const double cmax = mxc - mnc;
    for (int i = tid; i < N; i += SFF_NT) {
        double c = cc[i] - mnc;
        const double r = rr[i] - mnr;
        if (flip) c = cmax - c;
        arc[o + i] = __dsqrt_rn(__dadd_rn(__dmul_rn(c, c), __dmul_rn(r, r)));
    }
    if (tid == 0) {
        if (info) {
            info[4 * b + 0] = time ? time[o] : 0.0;
            info[4 * b + 1] = time ? time[o + N - 1] : 0.0;
            info[4 * b + 2] = (double)bad;
            info[4 * b + 3] = flip ? 1.0 : 0.0;
        }
        if (flipped) flipped[b] = flip ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ (b) knots and prior terms
// grid (W + 1, G).  Workgroup 0 of a target: f = flux / median(flux), e = flux_err / median(flux) (LightCurve.normalize), the
// cadence mask's bytes, stats = {median, mean(flux), np.std(f), 0}, the means of the n_knots chunks of np.array_split(f,
// n_knots) (the long-term block's prior_mu) and the long-term spline's knots [min(time), percentiles of time, max(time)].
// Workgroup j + 1: window j's knots [min(x), percentiles of arc[lo_j : up_j], max(x)] for x = arc inside the window and -1
// outside (so min(x) is -1 as soon as there is an outside, i.e. W > 1), and wout[g][j] = the window's basis at its lower
// boundary knot, column 0: what every cadence OUTSIDE the window gets there.  It is 1 up to the rounding of de Boor's
// recursion (the other degree columns are exactly 0: every left term is x - lo = 0), and taking it from bspline_row keeps
// the block the bits of lk_spline_basis_batch_dev for the outside cadences too.
__global__ __launch_bounds__(SFF_NT) void sff_knots_kernel(const int64_t *__restrict__ tab, const int32_t *__restrict__ wp, int W,
                                                           int bins, int degree, int n_knots, const double *__restrict__ time,
                                                           const double *__restrict__ flux, const double *__restrict__ err,
                                                           const uint8_t *__restrict__ cmask, const double *__restrict__ arc,
                                                           double *__restrict__ f, double *__restrict__ e,
                                                           uint8_t *__restrict__ cm, double *__restrict__ stats,
                                                           double *__restrict__ cmean, double *__restrict__ kt,
                                                           double *__restrict__ kw, double *__restrict__ wout) {
    __shared__ unsigned long long sh[264];
    double *shd = reinterpret_cast<double *>(sh);
    const int g = blockIdx.y, tid = threadIdx.x;
    const int64_t src = tab[SFF_TAB * g], loc = tab[SFF_TAB * g + 2], wpo = tab[SFF_TAB * g + 3];
    const int N = (int)tab[SFF_TAB * g + 1];
    auto all = [](int) { return true; };
    if (blockIdx.x > 0) {
        const int j = blockIdx.x - 1;
        const int lo = j == 0 ? 0 : wp[wpo + j - 1], up = j == W - 1 ? N : wp[wpo + j];
        const int n = up - lo;
        const double *a = arc + src + lo;
        double *out = kw + ((size_t)g * W + j) * (bins + 1);
        auto val = [&](int i) { return a[i]; };
        double mn = INFINITY, mx = -INFINITY;
        for (int i = tid; i < n; i += SFF_NT) {
            mn = fmin(mn, a[i]);
            mx = fmax(mx, a[i]);
        }
        mn = sff_block_min(mn, shd);
        mx = sff_block_max(mx, shd);
        if (tid == 0) {
            out[0] = W > 1 ? fmin(-1.0, mn) : mn;
            out[bins] = W > 1 ? fmax(-1.0, mx) : mx;
        }
        for (int k = 1; k < bins; ++k) {
            const double v = sff_percentile(n, k, bins, val, false, sh);
            if (tid == 0) out[k] = v;
        }
        if (tid == 0) {  // (its own stores above, read back in program order)
            double Nv[8];
            bspline_row(out[0], out[0], out[bins], [&](int i) { return out[1 + i]; }, bins - 1, degree, Nv);
            wout[(size_t)g * W + j] = Nv[0];
        }
        return;
    }
    const double *y = flux + src, *t = time + src;
    auto yv = [&](int i) { return y[i]; };
    const double med = block_median(N, (long long)N, yv, all, sh);
    double s = 0.0;
    for (int i = tid; i < N; i += SFF_NT) {
        s += y[i];
        f[loc + i] = y[i] / med;
        e[loc + i] = err[src + i] / med;
        if (cm) cm[loc + i] = cmask[src + i] ? 1 : 0;
    }
    const double raw_mean = block_sum_dyn(s, shd) / (double)N;
    s = 0.0;
    for (int i = tid; i < N; i += SFF_NT) s += y[i] / med;
    const double fmean = block_sum_dyn(s, shd) / (double)N;
    s = 0.0;
    for (int i = tid; i < N; i += SFF_NT) {
        const double d = y[i] / med - fmean;
        s += d * d;
    }
    const double sd = sqrt(block_sum_dyn(s, shd) / (double)N);
    if (tid == 0) {
        stats[4 * g + 0] = med;
        stats[4 * g + 1] = raw_mean;
        stats[4 * g + 2] = sd;
        stats[4 * g + 3] = 0.0;
    }
    // np.array_split(f, n_knots): the first N % n_knots chunks hold N / n_knots + 1 values, the others N / n_knots
    const int q = N / n_knots, rem = N % n_knots;
    for (int k = tid; k < n_knots; k += SFF_NT) {
        const int i0 = k * q + min(k, rem), len = q + (k < rem ? 1 : 0);
        double acc = 0.0;
        for (int i = i0; i < i0 + len; ++i) acc += y[i] / med;
        cmean[(size_t)g * n_knots + k] = acc / (double)len;
    }
    // the long-term spline's knots: percentiles of time (plain reads where the times are non-decreasing)
    const int n_inner = n_knots - SFF_TDEG - 1;
    long long desc = 0;
    double mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < N; i += SFF_NT) {
        desc += (i > 0 && t[i] < t[i - 1]) ? 1 : 0;
        mn = fmin(mn, t[i]);
        mx = fmax(mx, t[i]);
    }
    const bool sorted = block_count_dyn(desc, reinterpret_cast<long long *>(sh)) == 0;
    mn = sff_block_min(mn, shd);
    mx = sff_block_max(mx, shd);
    double *out = kt + (size_t)g * (n_inner + 2);
    auto tv = [&](int i) { return t[i]; };
    if (tid == 0) {
        out[0] = mn;
        out[n_inner + 1] = mx;
    }
    if (sorted) {
        for (int k = 1 + tid; k <= n_inner; k += SFF_NT) out[k] = sff_percentile(N, k, n_inner + 1, tv, true, sh);
    } else {
        for (int k = 1; k <= n_inner; ++k) {
            const double v = sff_percentile(N, k, n_inner + 1, tv, false, sh);
            if (tid == 0) out[k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ (c) design matrix
// grid (ceil(max N / 256), G).  A thread owns one cadence: its window (binary search in the target's window points), the
// SFF_TDEG + 1 non-zero values of the long-term basis at time and the degree + 1 non-zero values of its own window's basis at
// arclength (bspline_row, the function lk_spline_basis_batch_dev evaluates), parked in LDS.  Then the workgroup writes its
// 256 rows — one contiguous run of 256 K doubles — with the lanes along the run, 16 bytes per lane: the basis values where a
// column belongs to the cadence's spans, [wout, 0, ..., 0] in the blocks of the other windows (x = -1 = the lower boundary
// knot there: wout is that window's basis value, 1 up to rounding, from sff_knots_kernel), 0 elsewhere.  Workgroup 0 of a target also writes its priors: the long-term block mu = chunk means, sigma = 1000 std
// + 1e-6; the window blocks mu = 0, sigma = 10000 std + 1e-6.
__global__ __launch_bounds__(SFF_NT) void sff_design_kernel(const int64_t *__restrict__ tab, const int32_t *__restrict__ wp, int W,
                                                            int bins, int degree, int n_knots, int K,
                                                            const double *__restrict__ time, const double *__restrict__ arc,
                                                            const double *__restrict__ kt, const double *__restrict__ kw,
                                                            const double *__restrict__ wout, const double *__restrict__ stats,
                                                            const double *__restrict__ cmean, double *__restrict__ X, double *__restrict__ mu,
                                                            double *__restrict__ sg) {
    __shared__ double s_t[SFF_NT][SFF_TDEG + 1];
    __shared__ double s_w[SFF_NT][8];
    __shared__ int s_mut[SFF_NT], s_muw[SFF_NT], s_win[SFF_NT];
    const int g = blockIdx.y, tid = threadIdx.x;
    const int64_t src = tab[SFF_TAB * g], loc = tab[SFF_TAB * g + 2], wpo = tab[SFF_TAB * g + 3];
    const int N = (int)tab[SFF_TAB * g + 1];
    const int r0 = blockIdx.x * SFF_NT;
    if (r0 >= N) return;
    const int n_inner_t = n_knots - SFF_TDEG - 1, nbw = bins + degree;
    if (blockIdx.x == 0) {
        const double sd = stats[4 * g + 2];
        const double s_long = __dadd_rn(__dmul_rn(1000.0, sd), 1e-6), s_win_sigma = __dadd_rn(__dmul_rn(10000.0, sd), 1e-6);
        for (int c = tid; c < K; c += SFF_NT) {
            mu[(size_t)g * K + c] = c < n_knots ? cmean[(size_t)g * n_knots + c] : 0.0;
            sg[(size_t)g * K + c] = c < n_knots ? s_long : s_win_sigma;
        }
    }
    const int n = r0 + tid;
    if (n < N) {
        int lo = 0, hi = W - 1;  // the number of window points <= n
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (wp[wpo + mid] <= n)
                lo = mid + 1;
            else
                hi = mid;
        }
        s_win[tid] = lo;
        double Nv[8];
        const double *k1 = kt + (size_t)g * (n_inner_t + 2);
        s_mut[tid] = bspline_row(time[src + n], k1[0], k1[n_inner_t + 1], [&](int i) { return k1[1 + i]; }, n_inner_t, SFF_TDEG, Nv);
#pragma unroll
        for (int j = 0; j <= SFF_TDEG; ++j) s_t[tid][j] = Nv[j];
        const double *k2 = kw + ((size_t)g * W + lo) * (bins + 1);
        s_muw[tid] = bspline_row(arc[src + n], k2[0], k2[bins], [&](int i) { return k2[1 + i]; }, bins - 1, degree, Nv);
#pragma unroll
        for (int j = 0; j < 8; ++j) s_w[tid][j] = Nv[j];
    }
    __syncthreads();
    const int nrow = min(SFF_NT, N - r0), total = nrow * K;
    double *base = X + ((size_t)loc + r0) * K;
    auto val = [&](int el) -> double {
        const int r = el / K, c = el - r * K;
        if (c < n_knots) {
            const int j = c - s_mut[r];
            return (j >= 0 && j <= SFF_TDEG) ? s_t[r][j] : 0.0;
        }
        const int cw = c - n_knots, blk = cw / nbw, jj = cw - blk * nbw;
        if (blk != s_win[r]) return jj == 0 ? wout[(size_t)g * W + blk] : 0.0;
        const int j = jj - s_muw[r];
        return (j >= 0 && j <= degree) ? s_w[r][j] : 0.0;
    };
    const int head = (int)((reinterpret_cast<uintptr_t>(base) >> 3) & 1);  // one double up to 16-byte alignment
    if (head && tid == 0) base[0] = val(0);
    const int npair = (total - head) >> 1;
    for (int p = tid; p < npair; p += SFF_NT) {
        const int el = head + 2 * p;
        *reinterpret_cast<double2 *>(base + el) = make_double2(val(el), val(el + 1));
    }
    if (((total - head) & 1) && tid == 0) base[total - 1] = val(total - 1);
}

// ------------------------------------------------------------------------------------------------ (e) components and epilogue
// ps[i] = X[i][:n_knots] w[:n_knots], pf[i] = X[i][n_knots:] w[n_knots:] per cadence of a chunk: one wavefront per row, lanes
// over the columns, the lane sums added in a fixed tree.
__global__ __launch_bounds__(SFF_NT) void sff_parts_kernel(const int64_t *__restrict__ tab, int K, int n_knots,
                                                           const double *__restrict__ X, const double *__restrict__ w,
                                                           double *__restrict__ ps, double *__restrict__ pf) {
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t loc = tab[SFF_TAB * g + 2];
    const int N = (int)tab[SFF_TAB * g + 1];
    const double *wt = w + (size_t)g * K;
    for (int r = blockIdx.x * 4 + wave; r < N; r += gridDim.x * 4) {
        const double *row = X + ((size_t)loc + r) * K;
        double as = 0.0, af = 0.0;
        for (int k = lane; k < K; k += 64) {
            const double p = row[k] * wt[k];
            if (k < n_knots)
                as += p;
            else
                af += p;
        }
        for (int o = 32; o > 0; o >>= 1) {
            as += __shfl_down(as, o);
            af += __shfl_down(af, o);
        }
        if (lane == 0) {
            ps[loc + r] = as;
            pf[loc + r] = af;
        }
    }
}

// One workgroup per target: spline = ps - median(ps), sff = pf - median(pf) (np.median), corrected = f - model (the
// regression's model has its median removed already), + spline - nanmedian(spline) with restore_trend, then corrected and the
// errors times mean(raw flux); everything goes to the target's place in the batch, with the regression's outlier bytes and
// coefficients.
__global__ __launch_bounds__(1024) void sff_epilogue_kernel(const int64_t *__restrict__ tab, int K, int restore_trend,
                                                            const double *__restrict__ f, const double *__restrict__ e,
                                                            const double *__restrict__ model, const uint8_t *__restrict__ outl,
                                                            const double *__restrict__ ps, const double *__restrict__ pf,
                                                            const double *__restrict__ stats, const double *__restrict__ w,
                                                            double *__restrict__ flux_out, double *__restrict__ err_out,
                                                            uint8_t *__restrict__ outl_out, double *__restrict__ spline_out,
                                                            double *__restrict__ sff_out, double *__restrict__ w_out,
                                                            int w_pitch) {
    __shared__ unsigned long long sh[1024];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t src = tab[SFF_TAB * g], loc = tab[SFF_TAB * g + 2], b = tab[SFF_TAB * g + 4];
    const int N = (int)tab[SFF_TAB * g + 1];
    auto all = [](int) { return true; };
    const double *s = ps + loc, *q = pf + loc;
    const double med_s = block_median(N, (long long)N, [&](int i) { return s[i]; }, all, sh);
    const double med_f = block_median(N, (long long)N, [&](int i) { return q[i]; }, all, sh);
    double med2 = 0.0;
    if (restore_trend) med2 = block_median(N, (long long)N, [&](int i) { return s[i] - med_s; }, all, sh);
    const double raw_mean = stats[4 * g + 1];
    for (int i = tid; i < N; i += 1024) {
        const double sp = s[i] - med_s;
        double c = f[loc + i] - model[loc + i];
        if (restore_trend) c = c + (sp - med2);
        flux_out[src + i] = c * raw_mean;
        err_out[src + i] = e[loc + i] * raw_mean;
        outl_out[src + i] = outl[loc + i];
        if (spline_out) spline_out[src + i] = sp;
        if (sff_out) sff_out[src + i] = q[i] - med_f;
    }
    if (w_out)
        for (int c = tid; c < K; c += 1024) w_out[(size_t)b * w_pitch + c] = w[(size_t)g * K + c];
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
inline size_t sff_carve(size_t &used, size_t bytes) {
    const size_t at = used;
    used = (used + bytes + 255) & ~size_t(255);
    return at;
}

// the part of the scratch block that lives for the whole call: batch offsets, arclength, per-target info, window points
struct SffFixed {
    size_t off, arc, info, wp, total;
};
SffFixed sff_fixed_layout(int B, size_t ntot, size_t nwp) {
    SffFixed p;
    size_t used = 0;
    p.off = sff_carve(used, (size_t)(B + 1) * 8);
    p.arc = sff_carve(used, ntot * 8);
    p.info = sff_carve(used, (size_t)B * 4 * 8);
    p.wp = sff_carve(used, std::max<size_t>(nwp, 1) * 4);
    p.total = used;
    return p;
}

// one chunk: G targets of one (n_knots, W) with n cadences in all
struct SffChunkLayout {
    size_t tab, f, e, cm, model, outl, ps, pf, stats, cmean, kt, kw, wout, mu, sg, w, X, total;
};
SffChunkLayout sff_chunk_layout(size_t G, size_t n, int K, int W, int bins, int n_knots) {
    SffChunkLayout p;
    size_t used = 0;
    p.tab = sff_carve(used, G * SFF_TAB * 8);
    p.f = sff_carve(used, n * 8);
    p.e = sff_carve(used, n * 8);
    p.cm = sff_carve(used, n);
    p.model = sff_carve(used, n * 8);
    p.outl = sff_carve(used, n);
    p.ps = sff_carve(used, n * 8);
    p.pf = sff_carve(used, n * 8);
    p.stats = sff_carve(used, G * 4 * 8);
    p.cmean = sff_carve(used, G * n_knots * 8);
    p.kt = sff_carve(used, G * (size_t)(n_knots - SFF_TDEG + 1) * 8);
    p.kw = sff_carve(used, G * W * (size_t)(bins + 1) * 8);
    p.wout = sff_carve(used, G * W * 8);
    p.mu = sff_carve(used, G * K * 8);
    p.sg = sff_carve(used, G * K * 8);
    p.w = sff_carve(used, G * K * 8);
    p.X = sff_carve(used, n * (size_t)K * 8);
    p.total = used;
    return p;
}

struct SffChunk {
    int n_knots, W, K;
    std::vector<int> targets;  // indices into the batch, ascending
    size_t n;                  // their cadences
};

inline int sff_width(int n_knots, int W, int bins, int degree) { return n_knots + W * (bins + degree); }

// Targets with status 0 grouped by (n_knots, W) in key order, each group cut into chunks that fit `budget` bytes (greedy, in
// batch order).  A target whose own chunk does not fit is an error.
int sff_plan(int B, const int64_t *n_off, const int32_t *n_knots, const int32_t *win_off, const int32_t *status, int bins,
             int degree, size_t budget, std::vector<SffChunk> &chunks, size_t *largest) {
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (int b = 0; b < B; ++b)
        if (!status || status[b] == 0) groups[{n_knots[b], win_off[b + 1] - win_off[b] + 1}].push_back(b);
    *largest = 0;
    for (const auto &kv : groups) {
        const int nk = kv.first.first, W = kv.first.second, K = sff_width(nk, W, bins, degree);
        SffChunk cur{nk, W, K, {}, 0};
        for (const int b : kv.second) {
            const size_t N = (size_t)(n_off[b + 1] - n_off[b]);
            LK_REQUIRE(sff_chunk_layout(1, N, K, W, bins, nk).total <= budget,
                       "scratch too small: target %d alone (%zu cadences x %d columns) needs %zu bytes of %zu (lk_sff_scratch_bytes)",
                       b, N, K, sff_chunk_layout(1, N, K, W, bins, nk).total, budget);
            if (!cur.targets.empty() &&
                (sff_chunk_layout(cur.targets.size() + 1, cur.n + N, K, W, bins, nk).total > budget || cur.targets.size() >= 65535)) {
                chunks.push_back(cur);
                cur.targets.clear();
                cur.n = 0;
            }
            cur.targets.push_back(b);
            cur.n += N;
            *largest = std::max(*largest, sff_chunk_layout(cur.targets.size(), cur.n, K, W, bins, nk).total);
        }
        if (!cur.targets.empty()) chunks.push_back(cur);
    }
    return LK_OK;
}

int sff_shape_ok(int B, const int64_t *n_off, const int32_t *win_off, const int32_t *wp, int bins, int degree) {
    LK_REQUIRE(B >= 1 && n_off && win_off, "need B >= 1 targets, their offsets and their window offsets");
    LK_REQUIRE(bins >= 1 && bins <= 1024, "bins must be in 1..1024 (got %d)", bins);
    LK_REQUIRE(degree >= 0 && degree <= 7, "spline degree outside 0..7");
    LK_REQUIRE(n_off[0] == 0 && win_off[0] == 0, "n_off[0] and win_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t N = n_off[b + 1] - n_off[b];
        LK_REQUIRE(N >= 2 && N < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)N);
        LK_REQUIRE(win_off[b + 1] >= win_off[b], "win_off must be non-decreasing");
        if (!wp) continue;
        for (int k = win_off[b]; k < win_off[b + 1]; ++k)
            LK_REQUIRE(wp[k] > 0 && wp[k] < N && (k == win_off[b] || wp[k] > wp[k - 1]),
                       "target %d: window_points must be ascending cut indices inside (0, %lld)", b, (long long)N);
    }
    return LK_OK;
}
}  // namespace

int sff_scratch_bytes(int B, const int64_t *n_off, const int32_t *n_knots, const int32_t *win_off, int bins, int degree,
                      int64_t max_scratch_bytes, int64_t *bytes, int *n_chunks) {
    int rc = sff_shape_ok(B, n_off, win_off, nullptr, bins, degree);
    if (rc) return rc;
    LK_REQUIRE(n_knots && bytes, "NULL buffer");
    LK_REQUIRE(max_scratch_bytes >= 0, "max_scratch_bytes must be >= 0 (0: the default of %lld)", (long long)LK_SFF_SCRATCH_DEFAULT);
    std::vector<int32_t> status((size_t)B);
    for (int b = 0; b < B; ++b)
        status[b] = n_knots[b] < SFF_TDEG + 1 ? 1 : sff_width(n_knots[b], win_off[b + 1] - win_off[b] + 1, bins, degree) > SFF_KMAX ? 3 : 0;
    const SffFixed fx = sff_fixed_layout(B, (size_t)n_off[B], (size_t)win_off[B]);
    const size_t cap = (size_t)(max_scratch_bytes ? max_scratch_bytes : LK_SFF_SCRATCH_DEFAULT);
    LK_REQUIRE(cap > fx.total, "scratch too small: %zu bytes do not hold the batch's arclength (%zu bytes)", cap, fx.total);
    std::vector<SffChunk> chunks;
    size_t largest = 0;
    rc = sff_plan(B, n_off, n_knots, win_off, status.data(), bins, degree, cap - fx.total, chunks, &largest);
    if (rc) return rc;
    *bytes = (int64_t)(fx.total + largest);
    if (n_chunks) *n_chunks = (int)chunks.size();
    return LK_OK;
}

int sff_arclength_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *col, const double *row, double *arc,
                         int32_t *flipped, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0 || n_off_host[B] == 0) return LK_OK;
    LK_REQUIRE(col && row && arc, "NULL buffer");
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b)
        LK_REQUIRE(n_off_host[b + 1] - n_off_host[b] >= 0 && n_off_host[b + 1] - n_off_host[b] < ((int64_t)1 << 30),
                   "target %d has %lld cadences", b, (long long)(n_off_host[b + 1] - n_off_host[b]));
    int64_t *d_off;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).carve(stream)) return rc;
    hipLaunchKernelGGL(sff_arclength_kernel, dim3(B), dim3(SFF_NT), 0, stream, (const int64_t *)d_off, col, row,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, arc, (double *)nullptr,
                       (int *)flipped);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

namespace {
// kernels (b) and (c) of one chunk whose table is on the device
void sff_front(const SffChunk &c, const int64_t *tab, const int32_t *wp, int maxN, int bins, int degree, const double *time,
               const double *flux, const double *err, const uint8_t *cmask, const double *arc, double *f, double *e, uint8_t *cm,
               double *stats, double *cmean, double *kt, double *kw, double *wout, double *X, double *mu, double *sg,
               hipStream_t stream) {
    const int G = (int)c.targets.size();
    hipLaunchKernelGGL(sff_knots_kernel, dim3(c.W + 1, G), dim3(SFF_NT), 0, stream, tab, wp, c.W, bins, degree, c.n_knots, time, flux,
                       err, cmask, arc, f, e, cmask ? cm : (uint8_t *)nullptr, stats, cmean, kt, kw, wout);
    hipLaunchKernelGGL(sff_design_kernel, dim3((maxN + SFF_NT - 1) / SFF_NT, G), dim3(SFF_NT), 0, stream, tab, wp, c.W, bins, degree,
                       c.n_knots, c.K, time, arc, (const double *)kt, (const double *)kw, (const double *)wout, (const double *)stats,
                       (const double *)cmean, X, mu, sg);
}

// the table of a chunk and its offsets inside the chunk
int sff_table(const SffChunk &c, const int64_t *n_off, const int32_t *win_off, std::vector<int64_t> &tab, std::vector<int64_t> &loff) {
    const size_t G = c.targets.size();
    tab.assign(G * SFF_TAB, 0);
    loff.assign(G + 1, 0);
    int maxN = 0;
    for (size_t g = 0; g < G; ++g) {
        const int b = c.targets[g];
        const int64_t N = n_off[b + 1] - n_off[b];
        tab[SFF_TAB * g + 0] = n_off[b];
        tab[SFF_TAB * g + 1] = N;
        tab[SFF_TAB * g + 2] = loff[g];
        tab[SFF_TAB * g + 3] = win_off[b];
        tab[SFF_TAB * g + 4] = b;
        loff[g + 1] = loff[g] + N;
        maxN = std::max<int>(maxN, (int)N);
    }
    return maxN;
}
}  // namespace

// Stops after (c): the design matrix, priors and knots of B targets that all have n_knots long-term columns and the same
// number of windows (one regression group), for callers that run their own fit and for the tests of the design kernel.
int sff_design_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *err,
                      const double *arc, const int32_t *win_off_host, const int32_t *wp_host, int bins, int degree, int n_knots,
                      double *X, double *prior_mu, double *prior_sigma, double *knots_time, double *knots_win, double *f_out,
                      double *e_out, hipStream_t stream) {
    int rc = sff_shape_ok(B, n_off_host, win_off_host, wp_host, bins, degree);
    if (rc) return rc;
    LK_REQUIRE(time && flux && err && arc && X && prior_mu && prior_sigma && knots_time && knots_win && f_out && e_out, "NULL buffer");
    LK_REQUIRE(win_off_host[B] == 0 || wp_host, "window_points is NULL");
    LK_REQUIRE(B <= 65535, "at most 65535 targets per call (got %d)", B);
    LK_REQUIRE(n_knots >= SFF_TDEG + 1, "the long-term spline needs n_knots >= %d (got %d)", SFF_TDEG + 1, n_knots);
    const int W = win_off_host[1] - win_off_host[0] + 1;
    for (int b = 0; b < B; ++b)
        LK_REQUIRE(win_off_host[b + 1] - win_off_host[b] + 1 == W, "every target of a design call needs the same number of windows");
    SffChunk c{n_knots, W, sff_width(n_knots, W, bins, degree), {}, (size_t)n_off_host[B]};
    LK_REQUIRE(c.K <= SFF_KMAX, "K=%d is wider than the regression takes (%d)", c.K, SFF_KMAX);
    for (int b = 0; b < B; ++b) c.targets.push_back(b);
    std::vector<int64_t> tab, loff;
    const int maxN = sff_table(c, n_off_host, win_off_host, tab, loff);
    int64_t *d_tab;
    int32_t *d_wp;
    double *d_stats, *d_cmean, *d_wout;
    Scratch ws(h, h->ws);
    ws.upload(d_tab, (const int64_t *)tab.data(), tab.size())
        .upload(d_wp, wp_host, (size_t)win_off_host[B], win_off_host[B] != 0)
        .buf(d_stats, (size_t)B * 4)
        .buf(d_cmean, (size_t)B * n_knots)
        .buf(d_wout, (size_t)B * W);
    if ((rc = ws.carve(stream))) return rc;
    sff_front(c, d_tab, d_wp, maxN, bins, degree, time, flux, err, nullptr, arc, f_out, e_out, nullptr, d_stats, d_cmean, knots_time,
              knots_win, d_wout, X, prior_mu, prior_sigma, stream);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int sff_correct_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *err,
                       const double *col, const double *row, const uint8_t *cmask, const int32_t *win_off_host,
                       const int32_t *wp_host, int bins, int degree, double timescale, int restore_trend, double clip_sigma,
                       int niters, void *scratch, int64_t scratch_bytes, double *flux_out, double *err_out, uint8_t *outl_out,
                       int32_t *status_host, double *arclength, double *spline, double *sff, double *w, int w_pitch,
                       hipStream_t stream) {
    int rc = sff_shape_ok(B, n_off_host, win_off_host, wp_host, bins, degree);
    if (rc) return rc;
    LK_REQUIRE(time && flux && err && col && row && flux_out && err_out && outl_out && status_host, "NULL buffer");
    LK_REQUIRE(win_off_host[B] == 0 || wp_host, "window_points is NULL");
    LK_REQUIRE(timescale > 0.0 && timescale == timescale, "timescale must be positive");
    LK_REQUIRE(niters >= 1, "niters must be >= 1");
    LK_REQUIRE(scratch != nullptr && ((uintptr_t)scratch & 255) == 0 && scratch_bytes >= 0, "scratch must be a 256-byte aligned device buffer");
    LK_REQUIRE(!w || w_pitch >= 1, "w needs its row pitch");
    const size_t ntot = (size_t)n_off_host[B], nwp = (size_t)win_off_host[B];
    const SffFixed fx = sff_fixed_layout(B, ntot, nwp);
    LK_REQUIRE(fx.total < (size_t)scratch_bytes, "scratch too small: %lld bytes do not hold the batch's arclength (%zu bytes)",
               (long long)scratch_bytes, fx.total);
    char *blk = static_cast<char *>(scratch);
    int64_t *d_off = reinterpret_cast<int64_t *>(blk + fx.off);
    double *d_arc = arclength ? arclength : reinterpret_cast<double *>(blk + fx.arc);
    double *d_info = reinterpret_cast<double *>(blk + fx.info);
    int32_t *d_wp = reinterpret_cast<int32_t *>(blk + fx.wp);
    if ((rc = h->stage.copy(d_off, n_off_host, (size_t)(B + 1) * 8, stream))) return rc;
    if (nwp && (rc = h->stage.copy(d_wp, wp_host, nwp * 4, stream))) return rc;
    hipLaunchKernelGGL(sff_arclength_kernel, dim3(B), dim3(SFF_NT), 0, stream, (const int64_t *)d_off, col, row, time, flux, err,
                       d_arc, d_info, (int *)nullptr);
    LK_HIP_CHECK(hipGetLastError());
    std::vector<double> info((size_t)B * 4);
    LK_HIP_CHECK(hipMemcpyAsync(info.data(), d_info, info.size() * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    // statuses and the long-term spline's width, with the reference's scalar arithmetic: int((time[-1] - time[0]) / timescale)
    std::vector<int32_t> nk((size_t)B, 0);
    bool any_bad = false;
    for (int b = 0; b < B; ++b) {
        const double span = (info[4 * b + 1] - info[4 * b]) / timescale;
        int st = 0;
        if (info[4 * b + 2] != 0.0 || !(span == span))
            st = 2;
        else if (span < (double)(SFF_TDEG + 1))
            st = 1;
        else if (!(span < 1e6) || sff_width((int)span, win_off_host[b + 1] - win_off_host[b] + 1, bins, degree) > SFF_KMAX)
            st = 3;
        nk[b] = st == 0 ? (int)span : 0;
        status_host[b] = st;
        any_bad = any_bad || st != 0;
    }
    if (w) LK_HIP_CHECK(hipMemsetAsync(w, 0xFF, (size_t)B * w_pitch * 8, stream));  // (all bits set: a NaN)
    if (any_bad)
        for (int b = 0; b < B; ++b) {
            if (status_host[b] == 0) continue;
            const size_t o = (size_t)n_off_host[b], n = (size_t)(n_off_host[b + 1] - n_off_host[b]);
            LK_HIP_CHECK(hipMemsetAsync(flux_out + o, 0xFF, n * 8, stream));
            LK_HIP_CHECK(hipMemsetAsync(err_out + o, 0xFF, n * 8, stream));
            LK_HIP_CHECK(hipMemsetAsync(outl_out + o, 0, n, stream));
            if (spline) LK_HIP_CHECK(hipMemsetAsync(spline + o, 0xFF, n * 8, stream));
            if (sff) LK_HIP_CHECK(hipMemsetAsync(sff + o, 0xFF, n * 8, stream));
        }
    std::vector<SffChunk> chunks;
    size_t largest = 0;
    rc = sff_plan(B, n_off_host, nk.data(), win_off_host, status_host, bins, degree, (size_t)scratch_bytes - fx.total, chunks, &largest);
    if (rc) return rc;
    char *cb = blk + fx.total;
    std::vector<int64_t> tab, loff;
    for (const SffChunk &c : chunks) {
        LK_REQUIRE(!w || w_pitch >= c.K, "w_pitch=%d is narrower than a target's %d coefficients", w_pitch, c.K);
        const int G = (int)c.targets.size();
        const SffChunkLayout L = sff_chunk_layout((size_t)G, c.n, c.K, c.W, bins, c.n_knots);
        const int maxN = sff_table(c, n_off_host, win_off_host, tab, loff);
        int64_t *d_tab = reinterpret_cast<int64_t *>(cb + L.tab);
        double *d_f = reinterpret_cast<double *>(cb + L.f), *d_e = reinterpret_cast<double *>(cb + L.e);
        uint8_t *d_cm = reinterpret_cast<uint8_t *>(cb + L.cm), *d_outl = reinterpret_cast<uint8_t *>(cb + L.outl);
        double *d_model = reinterpret_cast<double *>(cb + L.model), *d_ps = reinterpret_cast<double *>(cb + L.ps);
        double *d_pf = reinterpret_cast<double *>(cb + L.pf), *d_stats = reinterpret_cast<double *>(cb + L.stats);
        double *d_cmean = reinterpret_cast<double *>(cb + L.cmean), *d_kt = reinterpret_cast<double *>(cb + L.kt);
        double *d_wout = reinterpret_cast<double *>(cb + L.wout);
        double *d_kw = reinterpret_cast<double *>(cb + L.kw), *d_mu = reinterpret_cast<double *>(cb + L.mu);
        double *d_sg = reinterpret_cast<double *>(cb + L.sg), *d_w = reinterpret_cast<double *>(cb + L.w);
        double *d_X = reinterpret_cast<double *>(cb + L.X);
        if ((rc = h->stage.copy(d_tab, tab.data(), tab.size() * 8, stream))) return rc;
        sff_front(c, d_tab, d_wp, maxN, bins, degree, time, flux, err, cmask, d_arc, d_f, d_e, d_cm, d_stats, d_cmean, d_kt, d_kw,
                  d_wout, d_X, d_mu, d_sg, stream);
        LK_HIP_CHECK(hipGetLastError());
        rc = regress_launch(h, G, loff.data(), c.K, d_X, d_f, d_e, cmask ? d_cm : nullptr, d_mu, d_sg, clip_sigma, niters, d_w,
                            d_model, d_outl, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(sff_parts_kernel, dim3(64, G), dim3(SFF_NT), 0, stream, (const int64_t *)d_tab, c.K, c.n_knots,
                           (const double *)d_X, (const double *)d_w, d_ps, d_pf);
        hipLaunchKernelGGL(sff_epilogue_kernel, dim3(G), dim3(1024), 0, stream, (const int64_t *)d_tab, c.K, restore_trend,
                           (const double *)d_f, (const double *)d_e, (const double *)d_model, (const uint8_t *)d_outl,
                           (const double *)d_ps, (const double *)d_pf, (const double *)d_stats, (const double *)d_w, flux_out,
                           err_out, outl_out, spline, sff, w, w_pitch);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

}  // namespace lk
