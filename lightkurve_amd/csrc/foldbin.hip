// foldbin.hip — phase-binned folded light curves for a ragged batch on gfx950.
//
// Reference: lc.fold(period, epoch_time).bin(...) (src/lightkurve/lightcurve.py:1089-1214, 1558-1763, FoldedLightCurve.cycle /
// odd_mask / even_mask :3213-3250) over astropy@4.3.1 aggregate_downsample (timeseries/downsample.py:60-130) applied to the
// phase column: relative time r = (phase - start) * 86400, edges = numpy's running sum of the bin size (formed by the caller,
// PER TARGET), slot in bin k when edges[k] < r <= edges[k+1] (r == 0 -> bin 0) and r < edges[n_bins].
//
// Four kernels:
//   fold_bin_plan_kernel   one workgroup per target, one stream over time / flux / flux_err: smallest and largest phase, the
//                          number of phases >= a threshold, the smallest cycle, max |flux|, max |err|, max - min flux, "has a finite error".
//                          64 B per target go to the host, which forms start, bin size, n_bins and the edges from them.
//   fold_cycle_kernel      cycle / odd / even per slot of a folded (sorted) batch.
//   phase_bin_kernel       one thread per (target, bin) of a folded batch: the bin is a contiguous slot range (two binary
//                          searches, as ingest.hip's bin_kernel); phase_bin_median_kernel: one workgroup per bin, nanmedian
//                          through block_select.hpp.
//   fold_bin_kernel        the fused form: one workgroup per target, no sort and no n-sized intermediate.  Every cadence's
//                          phase is recomputed (fold_phase.hpp: fold_kernel's bits), its bin found by an arithmetic guess
//                          corrected against the actual edges, and it is accumulated per bin in LDS.
//
// Reproducibility of the fused sums: no floating-point atomics.  Every addend is rounded to a multiple of a per-target quantum
// q = 2^e and accumulated as a 64-bit integer (lsfast.hip's fallback scatter does the same), so the adds are exact and commute:
// the result does not depend on arrival order, on B or on the neighbouring targets.  e is chosen from the target's own largest
// addend and its cadence count so that the sum of all of them stays below 2^62: the rounding of one addend is at most
// 2^-63 n max|x|, i.e. the bin's mean is within n * 2^-63 of max|flux| of the exact mean (2e-15 at 20 000 cadences).
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_select.hpp"
#include "fold_phase.hpp"
#include "lk_common.hpp"

namespace lk {

constexpr int FB_THREADS = 1024;
constexpr int FB_LDS_BINS = LK_FOLD_BIN_LDS_BINS;  // bins per target accumulated in LDS (32 B each); more: a global slab

__device__ __forceinline__ double fb_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double fb_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// relative time of a phase [s] and the centre of bin k (downsample.py:85-97, ingest.hip's bin_kernel)
__device__ __forceinline__ double fb_rel(double ph, double start) { return (ph - start) * 86400.0; }
__device__ __forceinline__ double fb_centre(double start, double edge, double size_sec) {
    return start + (edge + size_sec / 2.0) / 86400.0;
}

// workgroup reduction with an order-independent op (min / max / integer-valued sums below 2^53): 64-lane butterfly, one LDS
// word per wave.  Called by every thread; sh: blockDim.x / 64 doubles.
template <class Op> __device__ __forceinline__ double fb_reduce(double x, Op op, double *sh) {
    for (int o = 32; o >= 1; o >>= 1) x = op(x, __shfl_xor(x, o));
    const int nw = (int)(blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = sh[0];
    for (int i = 1; i < nw; ++i) r = op(r, sh[i]);
    return r;
}

// ------------------------------------------------------------------------------------------------ plan (pass 1)
// par: period | epoch_time | wrap_phase | count_from, B each.  plan[b][LK_FOLD_BIN_NPLAN] as include/lkhip.h lists it.
__global__ __launch_bounds__(FB_THREADS) void fold_bin_plan_kernel(const double *__restrict__ t, const double *__restrict__ flux,
                                                                    const double *__restrict__ err,
                                                                    const int64_t *__restrict__ n_off, int B,
                                                                    const double *__restrict__ par, double epoch_phase,
                                                                    int normalize_phase, int epoch_given,
                                                                    double *__restrict__ plan) {
    __shared__ double sh[FB_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    const double P = par[b];
    const FoldPar fp = fold_par(P, par[B + b], epoch_phase, par[2 * B + b], normalize_phase);
    const double from = par[3 * B + b];
    const double inf = fb_inf();
    double pmin = inf, pmax = -inf, tmin = inf, tmax = -inf, fmx = 0.0, emx = 0.0, cnt = 0.0, fin = 0.0;
    double flo = inf, fhi = -inf;
    for (int i = tid; i < n; i += nt) {
        const double ti = t[lo + i];
        const double ph = fold_phase(fp, ti);
        if (!isnan(ph)) {
            pmin = fmin(pmin, ph);
            pmax = fmax(pmax, ph);
            tmin = fmin(tmin, ti);
            tmax = fmax(tmax, ti);
            if (ph >= from) cnt += 1.0;
        }
        const double f = flux[lo + i];
        if (isfinite(f)) {
            fmx = fmax(fmx, fabs(f));
            flo = fmin(flo, f);
            fhi = fmax(fhi, f);
        }
        if (err) {
            const double e = err[lo + i];
            if (isfinite(e)) {
                fin = 1.0;
                emx = fmax(emx, fabs(e));
            }
        }
    }
    auto mn = [](double a, double c) { return fmin(a, c); };
    auto mx = [](double a, double c) { return fmax(a, c); };
    auto ad = [](double a, double c) { return a + c; };
    pmin = fb_reduce(pmin, mn, sh);
    pmax = fb_reduce(pmax, mx, sh);
    tmin = fb_reduce(tmin, mn, sh);
    tmax = fb_reduce(tmax, mx, sh);
    fmx = fb_reduce(fmx, mx, sh);
    flo = fb_reduce(flo, mn, sh);
    fhi = fb_reduce(fhi, mx, sh);
    emx = fb_reduce(emx, mx, sh);
    cnt = fb_reduce(cnt, ad, sh);
    fin = fb_reduce(fin, mx, sh);
    if (tid == 0) {
        // the cycle is monotone in t (one subtraction, one division, floor): its minimum sits at the first or the last time
        const double e = epoch_given ? par[B + b] : pmin;
        const double cmin = n > 0 && tmin <= tmax ? fmin(fb_cycle(tmin, e, P), fb_cycle(tmax, e, P)) : 0.0;
        double *p = plan + (size_t)b * LK_FOLD_BIN_NPLAN;
        p[0] = pmin;
        p[1] = pmax;
        p[2] = cnt;
        p[3] = fin;
        p[4] = cmin;
        p[5] = fmx;
        p[6] = emx;
        p[7] = flo <= fhi ? fhi - flo : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ cycle / odd / even
// par: period | cycle_epoch | cycle_min, B each.  Slot i of target b holds cadence order[lo + i].
__global__ __launch_bounds__(256) void fold_cycle_kernel(const double *__restrict__ t, const int64_t *__restrict__ order,
                                                          const int64_t *__restrict__ n_off, int B,
                                                          const double *__restrict__ par, int64_t *__restrict__ cycle,
                                                          uint8_t *__restrict__ odd, uint8_t *__restrict__ even) {
    const int b = blockIdx.y;
    const int64_t lo = n_off[b], n = n_off[b + 1] - lo;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long c = (long long)(fb_cycle(t[lo + order[lo + i]], par[B + b], par[b]) - par[2 * B + b]);
    if (cycle) cycle[lo + i] = c;
    if (odd) odd[lo + i] = (uint8_t)(c & 1);
    if (even) even[lo + i] = (uint8_t)((c & 1) ^ 1);
}

// ------------------------------------------------------------------------------------------------ bins of a folded batch
// The slot range [i0, i1) of bin k: phases are sorted, so r is non-decreasing (ingest.hip's bin_kernel, edges per target).
__device__ __forceinline__ void phase_bin_range(const double *__restrict__ ph, int n, double start,
                                                const double *__restrict__ edges, int k, int nb, int *i0_out, int *i1_out) {
    auto first_gt = [&](double x) {
        int a = 0, c = n;
        while (a < c) {
            const int mid = (a + c) >> 1;
            if (fb_rel(ph[mid], start) > x)
                c = mid;
            else
                a = mid + 1;
        }
        return a;
    };
    auto first_ge = [&](double x) {
        int a = 0, c = n;
        while (a < c) {
            const int mid = (a + c) >> 1;
            if (fb_rel(ph[mid], start) >= x)
                c = mid;
            else
                a = mid + 1;
        }
        return a;
    };
    const int i0 = k == 0 ? first_ge(edges[0]) : first_gt(edges[k]);
    int i1 = first_gt(edges[k + 1]);
    i1 = min(i1, first_ge(edges[nb]));  // keep: rel < last edge
    *i0_out = i0;
    *i1_out = max(i1, i0);
}

// the target that owns global bin g: last b with bin_off[b] <= g
__device__ __forceinline__ int phase_bin_owner(const int64_t *__restrict__ bin_off, int B, int64_t g) {
    int b_lo = 0, b_hi = B;
    while (b_hi - b_lo > 1) {
        const int mid = (b_lo + b_hi) >> 1;
        if (bin_off[mid] <= g)
            b_lo = mid;
        else
            b_hi = mid;
    }
    return b_lo;
}

// par: start | size_sec, B each; edges: target b's n_bins_b + 1 edges at bin_off[b] + b; sel (nullable): only the slots with
// sel[i] == sel_value count.  Outputs per bin: centre, nanmean, rmse of the errors (nanstd of the flux where !has_err[b]),
// number of selected slots; a bin without a selected slot holds NaN.
__global__ __launch_bounds__(256) void phase_bin_kernel(const double *__restrict__ phase, const double *__restrict__ flux,
                                                         const double *__restrict__ err, const uint8_t *__restrict__ sel,
                                                         int sel_value, const int64_t *__restrict__ n_off,
                                                         const int64_t *__restrict__ bin_off, int B,
                                                         const double *__restrict__ par, const double *__restrict__ edges_all,
                                                         const uint8_t *__restrict__ has_err, double *__restrict__ p_out,
                                                         double *__restrict__ f_out, double *__restrict__ e_out,
                                                         int32_t *__restrict__ c_out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= bin_off[B]) return;
    const int b = phase_bin_owner(bin_off, B, g);
    const int k = (int)(g - bin_off[b]), nb = (int)(bin_off[b + 1] - bin_off[b]);
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    const double start = par[b], size_sec = par[B + b];
    const double *edges = edges_all + bin_off[b] + b;
    int i0, i1;
    phase_bin_range(phase + lo, n, start, edges, k, nb, &i0, &i1);
    const bool he = err && has_err[b];
    double s = 0.0, s2 = 0.0;
    int cs = 0, cf = 0, ce = 0;
    for (int i = i0; i < i1; ++i) {
        if (sel && sel[lo + i] != sel_value) continue;
        ++cs;
        const double f = flux[lo + i];
        if (!isnan(f)) {
            s += f;
            ++cf;
        }
        if (he) {
            const double e = err[lo + i];
            if (isfinite(e)) ++ce;  // rmse: sqrt(nansum(x^2) / count(isfinite(x)))
            if (!isnan(e)) s2 = fma(e, e, s2);
        }
    }
    const double qnan = fb_qnan();
    const double mean = cf ? s / (double)cf : qnan;
    double eo;
    if (he) {
        eo = ce ? sqrt(s2 / (double)ce) : qnan;
    } else {  // no usable errors anywhere in this light curve: nanstd of the flux in the bin
        double v = 0.0;
        for (int i = i0; i < i1; ++i) {
            if (sel && sel[lo + i] != sel_value) continue;
            const double f = flux[lo + i];
            if (!isnan(f)) {
                const double d = f - mean;
                v = fma(d, d, v);
            }
        }
        eo = cf ? sqrt(v / (double)cf) : qnan;
    }
    p_out[g] = fb_centre(start, edges[k], size_sec);
    f_out[g] = cs ? mean : qnan;
    e_out[g] = cs ? eo : qnan;
    c_out[g] = cs;
}

// np.nanmedian of the selected non-NaN flux of each bin, one workgroup per bin (overwrites phase_bin_kernel's mean)
__global__ __launch_bounds__(256) void phase_bin_median_kernel(const double *__restrict__ phase, const double *__restrict__ flux,
                                                                const uint8_t *__restrict__ sel, int sel_value,
                                                                const int64_t *__restrict__ n_off,
                                                                const int64_t *__restrict__ bin_off, int B,
                                                                const double *__restrict__ par,
                                                                const double *__restrict__ edges_all,
                                                                double *__restrict__ f_out) {
    __shared__ unsigned long long sh[264];
    const int64_t g = blockIdx.x;
    const int b = phase_bin_owner(bin_off, B, g);
    const int k = (int)(g - bin_off[b]), nb = (int)(bin_off[b + 1] - bin_off[b]);
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    int i0, i1;
    phase_bin_range(phase + lo, n, par[b], edges_all + bin_off[b] + b, k, nb, &i0, &i1);
    const double *f = flux + lo + i0;
    const uint8_t *m = sel ? sel + lo + i0 : nullptr;
    auto val = [&](int i) { return f[i]; };
    auto keep = [&](int i) { return !isnan(f[i]) && (!m || m[i] == sel_value); };
    long long c = 0;
    for (int i = threadIdx.x; i < i1 - i0; i += 256) c += keep(i) ? 1 : 0;
    const long long count = block_count_dyn(c, reinterpret_cast<long long *>(sh));
    const double med = block_median(i1 - i0, count, val, keep, sh);
    if (threadIdx.x == 0) f_out[g] = med;
}

// ------------------------------------------------------------------------------------------------ fused fold + bin
// The bin of relative time r, or -1: an arithmetic guess corrected against the edge values, so membership is the reference's
// comparison (edges[k] < r <= edges[k+1], r == 0 -> bin 0, r < edges[nb]) and not a division.
__device__ __forceinline__ int fb_locate(double r, const double *__restrict__ edges, int nb, double size_sec) {
    if (!(r >= edges[0] && r < edges[nb])) return -1;  // (NaN fails both)
    int k = (int)fmin(r / size_sec, (double)(nb - 1));
    k = max(k, 0);
    while (k > 0 && r <= edges[k]) --k;
    while (k + 1 < nb && r > edges[k + 1]) ++k;
    return k;
}

// accumulators of one target: LDS arrays, or (GLOBAL) its slab in device memory, touched by this workgroup only; there the
// plain zero stores, the L2 atomics and the final loads are ordered by the barriers and the loads bypass L1
template <bool GLOBAL> struct FbAcc {
    long long *sf, *se;
    int *cnt, *cf, *ce, *fl;
    template <class T> __device__ __forceinline__ static T ld(const T *p) {
        if (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return *p;
    }
    template <class T> __device__ __forceinline__ static void zero(T *p) {
        if (GLOBAL)
            __hip_atomic_store(p, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            *p = (T)0;
    }
    __device__ __forceinline__ static void add64(long long *p, long long v) {
        atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
};

struct FbTarget {
    const double *t, *flux, *err;  // the target's cadences (err null: none)
    const double *edges;
    int n, nb, which, has_err, qf, qe, qv;
    double start, size_sec, cyc_epoch, cyc_min;
    FoldPar fp;
};

// flags per bin: 1 / 2: a +inf / -inf flux, 4: an infinite err^2, 8: an infinite squared deviation
template <bool GLOBAL>
__device__ __forceinline__ void fb_sweep(const FbTarget &T, FbAcc<GLOBAL> A, double *__restrict__ p_out, double *__restrict__ f_out,
                                         double *__restrict__ e_out, int32_t *__restrict__ c_out) {
    const int tid = threadIdx.x, nt = blockDim.x;
    auto barrier = [] {
        if (GLOBAL) __threadfence();
        __syncthreads();
    };
    for (int k = tid; k < T.nb; k += nt) {
        A.zero(A.sf + k), A.zero(A.se + k), A.zero(A.cnt + k), A.zero(A.cf + k), A.zero(A.ce + k), A.zero(A.fl + k);
    }
    barrier();
    // the selected cadence's bin, or -1
    auto bin_of = [&](int i) {
        const double ti = T.t[i];
        if (T.which) {
            const long long c = (long long)(fb_cycle(ti, T.cyc_epoch, T.fp.P) - T.cyc_min);
            if ((int)(c & 1) != (T.which == 1 ? 1 : 0)) return -1;
        }
        return fb_locate(fb_rel(fold_phase(T.fp, ti), T.start), T.edges, T.nb, T.size_sec);
    };
    // pass 2: counts, flux sums, err^2 sums
    for (int i = tid; i < T.n; i += nt) {
        const int k = bin_of(i);
        if (k < 0) continue;
        atomicAdd(A.cnt + k, 1);
        const double f = T.flux[i];
        if (!isnan(f)) {
            atomicAdd(A.cf + k, 1);
            if (isinf(f))
                atomicOr(A.fl + k, f > 0.0 ? 1 : 2);
            else
                A.add64(A.sf + k, llrint(ldexp(f, -T.qf)));
        }
        if (T.has_err) {
            const double e = T.err[i];
            if (isfinite(e)) atomicAdd(A.ce + k, 1);
            if (!isnan(e)) {
                const double x = e * e;
                if (isinf(x))
                    atomicOr(A.fl + k, 4);
                else
                    A.add64(A.se + k, llrint(ldexp(x, -T.qe)));
            }
        }
    }
    barrier();
    auto mean_of = [&](int k, int cf, int fl) {
        double s = ldexp((double)A.ld(A.sf + k), T.qf);
        if (fl & 1) s += fb_inf();
        if (fl & 2) s -= fb_inf();
        return cf ? s / (double)cf : fb_qnan();
    };
    // pass 3, targets without a finite error only: nanstd needs the bins' means first
    if (!T.has_err) {
        for (int i = tid; i < T.n; i += nt) {
            const int k = bin_of(i);
            if (k < 0) continue;
            const double f = T.flux[i];
            const int fl = A.ld(A.fl + k);
            if (isnan(f) || (fl & 3)) continue;  // (an infinite flux in the bin: its nanstd is NaN, set below)
            const double d = f - mean_of(k, A.ld(A.cf + k), fl);
            const double v = d * d;
            if (isinf(v))
                atomicOr(A.fl + k, 8);
            else
                A.add64(A.se + k, llrint(ldexp(v, -T.qv)));
        }
        barrier();
    }
    const double qnan = fb_qnan();
    for (int k = tid; k < T.nb; k += nt) {
        const int cs = A.ld(A.cnt + k), cf = A.ld(A.cf + k), ce = A.ld(A.ce + k), fl = A.ld(A.fl + k);
        const double mean = mean_of(k, cf, fl);
        double eo;
        if (T.has_err) {
            double s2 = ldexp((double)A.ld(A.se + k), T.qe);
            if (fl & 4) s2 = fb_inf();
            eo = ce ? sqrt(s2 / (double)ce) : qnan;
        } else {
            double v = ldexp((double)A.ld(A.se + k), T.qv);
            if (fl & 8) v = fb_inf();
            if (fl & 3) v = qnan;
            eo = cf ? sqrt(v / (double)cf) : qnan;
        }
        p_out[k] = fb_centre(T.start, T.edges[k], T.size_sec);
        f_out[k] = cs ? mean : qnan;
        e_out[k] = cs ? eo : qnan;
        c_out[k] = cs;
    }
}

// par: period | epoch_time | wrap_phase | start | size_sec | cycle_epoch | cycle_min, B each.  ipar: has_err | qf | qe | qv.
// tab: n_off (B + 1) | bin_off (B + 1) | slab_off (B + 1, in bins).
__global__ __launch_bounds__(FB_THREADS) void fold_bin_kernel(const double *__restrict__ t, const double *__restrict__ flux,
                                                               const double *__restrict__ err, const int64_t *__restrict__ tab,
                                                               int B, const double *__restrict__ par,
                                                               const int *__restrict__ ipar, double epoch_phase,
                                                               int normalize_phase, int which,
                                                               const double *__restrict__ edges_all, char *__restrict__ slab,
                                                               double *__restrict__ p_out, double *__restrict__ f_out,
                                                               double *__restrict__ e_out, int32_t *__restrict__ c_out) {
    __shared__ long long s_sf[FB_LDS_BINS], s_se[FB_LDS_BINS];
    __shared__ int s_cnt[FB_LDS_BINS], s_cf[FB_LDS_BINS], s_ce[FB_LDS_BINS], s_fl[FB_LDS_BINS];
    const int b = blockIdx.x;
    const int64_t *n_off = tab, *bin_off = tab + (B + 1), *slab_off = tab + 2 * (B + 1);
    const int64_t lo = n_off[b], bo = bin_off[b];
    FbTarget T;
    T.n = (int)(n_off[b + 1] - lo);
    T.nb = (int)(bin_off[b + 1] - bo);
    if (T.nb <= 0) return;
    T.t = t + lo;
    T.flux = flux + lo;
    T.err = err ? err + lo : nullptr;
    T.edges = edges_all + bo + b;
    T.which = which;
    T.has_err = err ? ipar[b] : 0;
    T.qf = ipar[B + b];
    T.qe = ipar[2 * B + b];
    T.qv = ipar[3 * B + b];
    T.fp = fold_par(par[b], par[B + b], epoch_phase, par[2 * B + b], normalize_phase);
    T.start = par[3 * B + b];
    T.size_sec = par[4 * B + b];
    T.cyc_epoch = par[5 * B + b];
    T.cyc_min = par[6 * B + b];
    if (T.nb <= FB_LDS_BINS) {
        FbAcc<false> A{s_sf, s_se, s_cnt, s_cf, s_ce, s_fl};
        fb_sweep(T, A, p_out + bo, f_out + bo, e_out + bo, c_out + bo);
    } else {
        char *base = slab + slab_off[b] * 32;
        const size_t nb = (size_t)T.nb;
        FbAcc<true> A{reinterpret_cast<long long *>(base),
                      reinterpret_cast<long long *>(base + 8 * nb),
                      reinterpret_cast<int *>(base + 16 * nb),
                      reinterpret_cast<int *>(base + 20 * nb),
                      reinterpret_cast<int *>(base + 24 * nb),
                      reinterpret_cast<int *>(base + 28 * nb)};
        fb_sweep(T, A, p_out + bo, f_out + bo, e_out + bo, c_out + bo);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
namespace {
int fb_check_batch(int B, const int64_t *n_off_host, int64_t *nmax) {
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    *nmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)n);
        *nmax = std::max(*nmax, n);
    }
    return LK_OK;
}

// bins [bin_off[b], bin_off[b+1]) with their edges at bin_off[b] + b: increasing from 0, as the running sum forms them
int fb_check_bins(int B, const int64_t *bin_off, const double *start, const double *size_sec, const double *edges) {
    LK_REQUIRE(bin_off[0] == 0, "bin_off must be prefix offsets starting at 0");
    for (int b = 0; b < B; ++b) {
        const int64_t nb = bin_off[b + 1] - bin_off[b];
        LK_REQUIRE(nb >= 0 && nb < ((int64_t)1 << 30), "target %d has %lld bins", b, (long long)nb);
        if (nb == 0) continue;
        LK_REQUIRE(std::isfinite(start[b]) && std::isfinite(size_sec[b]) && size_sec[b] > 0.0,
                   "target %d: the bin start must be finite and the bin size positive", b);
        const double *e = edges + bin_off[b] + b;
        LK_REQUIRE(e[0] == 0.0, "target %d: edges must start at 0", b);
        for (int64_t k = 0; k < nb; ++k)
            LK_REQUIRE(e[k + 1] > e[k], "target %d: bin edges must be strictly increasing (edge %lld)", b, (long long)(k + 1));
    }
    return LK_OK;
}

// exponent e of the quantum 2^e: n addends of at most vmax sum to less than 2^62 quanta
int fb_quantum_exp(double vmax, int64_t n) {
    if (!(vmax > 0.0)) return 0;
    if (!std::isfinite(vmax)) vmax = 1.7976931348623157e308;
    int L = 0;
    while (((int64_t)1 << L) < n) ++L;
    return std::ilogb(vmax) + 1 + L - 62;
}
}  // namespace

int fold_bin_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                         const double *period_host, const double *epoch_time_host, int epoch_given, double epoch_phase,
                         const double *wrap_phase_host, int normalize_phase, const double *count_from_host, double *plan_host,
                         hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && period_host && epoch_time_host && wrap_phase_host && plan_host, "NULL buffer");
    int64_t nmax;
    if (const int rc = fb_check_batch(B, n_off_host, &nmax)) return rc;
    std::vector<double> par((size_t)4 * B);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(std::isfinite(period_host[b]) && period_host[b] != 0.0, "target %d: period must be finite and non-zero", b);
        par[b] = period_host[b];
        par[(size_t)B + b] = epoch_time_host[b];
        par[(size_t)2 * B + b] = wrap_phase_host[b];
        par[(size_t)3 * B + b] = count_from_host ? count_from_host[b] : -HUGE_VAL;
    }
    int64_t *d_off;
    double *d_par, *d_plan;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, (size_t)B + 1).upload(d_par, par.data(), par.size())
            .buf(d_plan, (size_t)B * LK_FOLD_BIN_NPLAN).carve(stream))
        return rc;
    hipLaunchKernelGGL(fold_bin_plan_kernel, dim3(B), dim3(FB_THREADS), 0, stream, t, flux, err, d_off, B, d_par, epoch_phase,
                       normalize_phase, epoch_given, d_plan);
    LK_HIP_CHECK(hipGetLastError());
    LK_HIP_CHECK(hipMemcpyAsync(plan_host, d_plan, (size_t)B * LK_FOLD_BIN_NPLAN * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    return LK_OK;
}

int fold_cycle_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int64_t *order,
                      const double *period_host, const double *cycle_epoch_host, const double *cycle_min_host, int64_t *cycle,
                      uint8_t *odd, uint8_t *even, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(B <= 65535, "at most 65535 targets per call on this path (got %d): split the batch", B);
    LK_REQUIRE(t && order && period_host && cycle_epoch_host && cycle_min_host, "NULL buffer");
    int64_t nmax;
    if (const int rc = fb_check_batch(B, n_off_host, &nmax)) return rc;
    if (nmax == 0) return LK_OK;
    std::vector<double> par((size_t)3 * B);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(std::isfinite(period_host[b]) && period_host[b] != 0.0, "target %d: period must be finite and non-zero", b);
        par[b] = period_host[b];
        par[(size_t)B + b] = cycle_epoch_host[b];
        par[(size_t)2 * B + b] = cycle_min_host[b];
    }
    int64_t *d_off;
    double *d_par;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, (size_t)B + 1).upload(d_par, par.data(), par.size()).carve(stream))
        return rc;
    hipLaunchKernelGGL(fold_cycle_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)B), dim3(256), 0, stream, t, order, d_off,
                       B, d_par, cycle, odd, even);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int phase_bin_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *phase, const double *flux, const double *err,
                     const uint8_t *sel, int sel_value, const int64_t *bin_off_host, const double *start_host,
                     const double *size_sec_host, const double *edges_host, const uint8_t *has_err_host, int median,
                     double *phase_out, double *flux_out, double *err_out, int32_t *count_out, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host && bin_off_host, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(phase && flux && start_host && size_sec_host && edges_host && has_err_host && phase_out && flux_out && err_out &&
                   count_out,
               "NULL buffer");
    int64_t nmax;
    if (const int rc = fb_check_batch(B, n_off_host, &nmax)) return rc;
    if (const int rc = fb_check_bins(B, bin_off_host, start_host, size_sec_host, edges_host)) return rc;
    const int64_t nbins = bin_off_host[B];
    if (nbins == 0) return LK_OK;
    LK_REQUIRE(!median || nbins < ((int64_t)1 << 31), "too many bins for one call (%lld): split the batch", (long long)nbins);
    std::vector<double> par((size_t)2 * B);
    for (int b = 0; b < B; ++b) {
        par[b] = start_host[b];
        par[(size_t)B + b] = size_sec_host[b];
    }
    int64_t *d_off, *d_boff;
    double *d_par, *d_edges;
    uint8_t *d_he;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, (size_t)B + 1).upload(d_boff, bin_off_host, (size_t)B + 1)
            .upload(d_par, par.data(), par.size()).upload(d_edges, edges_host, (size_t)(nbins + B))
            .upload(d_he, has_err_host, (size_t)B).carve(stream))
        return rc;
    hipLaunchKernelGGL(phase_bin_kernel, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, stream, phase, flux, err, sel,
                       sel_value, d_off, d_boff, B, d_par, d_edges, d_he, phase_out, flux_out, err_out, count_out);
    if (median)
        hipLaunchKernelGGL(phase_bin_median_kernel, dim3((unsigned)nbins), dim3(256), 0, stream, phase, flux, sel, sel_value, d_off,
                           d_boff, B, d_par, d_edges, flux_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int fold_bin_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                    const double *period_host, const double *epoch_time_host, double epoch_phase, const double *wrap_phase_host,
                    int normalize_phase, const double *cycle_epoch_host, const double *plan_host, int which,
                    const int64_t *bin_off_host, const double *start_host, const double *size_sec_host, const double *edges_host,
                    double *phase_out, double *flux_out, double *err_out, int32_t *count_out, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host && bin_off_host, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && period_host && epoch_time_host && wrap_phase_host && cycle_epoch_host && plan_host && start_host &&
                   size_sec_host && edges_host && phase_out && flux_out && err_out && count_out,
               "NULL buffer");
    LK_REQUIRE(which >= 0 && which <= 2, "which must be 0 (all), 1 (odd) or 2 (even)");
    int64_t nmax;
    if (const int rc = fb_check_batch(B, n_off_host, &nmax)) return rc;
    if (const int rc = fb_check_bins(B, bin_off_host, start_host, size_sec_host, edges_host)) return rc;
    const int64_t nbins = bin_off_host[B];
    if (nbins == 0) return LK_OK;
    std::vector<int64_t> tab((size_t)3 * (B + 1), 0);
    std::vector<double> par((size_t)7 * B);
    std::vector<int> ipar((size_t)4 * B);
    int64_t *slab_off = tab.data() + 2 * (size_t)(B + 1);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(std::isfinite(period_host[b]) && period_host[b] != 0.0, "target %d: period must be finite and non-zero", b);
        const int64_t n = n_off_host[b + 1] - n_off_host[b], nb = bin_off_host[b + 1] - bin_off_host[b];
        const double *pl = plan_host + (size_t)b * LK_FOLD_BIN_NPLAN;
        tab[b + 1] = n_off_host[b + 1];
        tab[(size_t)(B + 1) + b + 1] = bin_off_host[b + 1];
        slab_off[b + 1] = slab_off[b] + (nb > FB_LDS_BINS ? nb : 0);
        par[b] = period_host[b];
        par[(size_t)B + b] = epoch_time_host[b];
        par[(size_t)2 * B + b] = wrap_phase_host[b];
        par[(size_t)3 * B + b] = start_host[b];
        par[(size_t)4 * B + b] = size_sec_host[b];
        par[(size_t)5 * B + b] = cycle_epoch_host[b];
        par[(size_t)6 * B + b] = pl[4];
        ipar[b] = pl[3] > 0.0 ? 1 : 0;
        ipar[(size_t)B + b] = fb_quantum_exp(pl[5], n);
        ipar[(size_t)2 * B + b] = fb_quantum_exp(pl[6] * pl[6], n);
        ipar[(size_t)3 * B + b] = fb_quantum_exp(pl[7] * pl[7], n);  // |flux - bin mean| <= max - min of the flux
    }
    int64_t *d_tab;
    double *d_par, *d_edges;
    int *d_ipar;
    char *d_slab;
    if (const int rc = Scratch(h, h->ws).upload(d_tab, tab.data(), tab.size()).upload(d_par, par.data(), par.size())
            .upload(d_ipar, ipar.data(), ipar.size()).upload(d_edges, edges_host, (size_t)(nbins + B))
            .buf(d_slab, (size_t)slab_off[B] * 32).carve(stream))
        return rc;
    hipLaunchKernelGGL(fold_bin_kernel, dim3(B), dim3(FB_THREADS), 0, stream, t, flux, err, d_tab, B, d_par, d_ipar, epoch_phase,
                       normalize_phase, which, d_edges, d_slab, phase_out, flux_out, err_out, count_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
