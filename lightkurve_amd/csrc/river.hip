// river.hip — river diagrams (cycle x phase images) of a ragged batch on gfx950: the data behind LightCurve.plot_river.
//
// The definition is include/lkhip.h's: y = flux / nanmedian(flux), phase = fold_phase (fold_kernel's bits,
// epoch_phase 0, wrap_phase 0.5, normalised), row = FoldedLightCurve.cycle (fb_cycle of the same header), column j when edges[j] < phase <= edges[j+1].
//
// Two kernels:
//   river_plan_kernel   one workgroup per target, one stream over time / flux / flux_err: the two medians that scale the image
//                       (exact order statistics, block_select.hpp; the time differences formed on the fly), smallest and
//                       largest cycle, the sorted / finite-time flag, the first time and the maxima the quanta are sized by.
//                       72 B per target go to the host, which forms statuses, n_bins, n_cycles, cell_off and the edges.
//   river_kernel        one workgroup per tile.  A tile is a block of whole rows of one target (or, where one row has more
//                       cells than LDS holds, a column chunk of one row) of at most LK_RIVER_LDS_CELLS cells.  The cycle is
//                       non-decreasing in t, so a block of rows is one contiguous cadence range (two binary searches); inside
//                       it membership is decided per cadence: fold_phase, an arithmetic guess of the column corrected against
//                       the uploaded edges, the cycle for the row.
//
// mean / sigma: foldbin.hip's scheme.  No floating-point atomics: every addend is rounded to a multiple of a per-target quantum
// 2^e and accumulated as a 64-bit integer in LDS, so the adds are exact and commute; e comes from the target's own largest addend
// and cadence count (sum below 2^62), never from the batch or the tile.  median: the tile's values are counted per cell, the counts
// scanned, the values scattered into per-cell segments (LDS, or the tile's slab of device scratch when more than
// LK_RIVER_LDS_VALS take part); the order inside a segment is free, the result is an order statistic.  A segment of up to
// LK_RIVER_CELL_THREAD values is ranked by one thread, a longer one by the workgroup's radix select.
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_select.hpp"
#include "fold_phase.hpp"
#include "lk_common.hpp"

namespace lk {

constexpr int RV_PLAN_THREADS = 1024;
constexpr int RV_THREADS = 512;
constexpr int RV_CELLS = LK_RIVER_LDS_CELLS;
constexpr int RV_VALS = LK_RIVER_LDS_VALS;
constexpr int RV_LDS_WORDS = RV_CELLS * 5 / 2;  // 64-bit words of LDS per workgroup (60 KiB: two workgroups per CU)
constexpr int RV_INF_FLAG = 1 << 30;            // sigma: an infinite err^2 in the cell (kept in the count word)
static_assert(RV_CELLS + RV_VALS + RV_THREADS <= RV_LDS_WORDS, "median: counts | cursors | values | select scratch");
static_assert(RV_CELLS % 2 == 0, "the count array ends on a 64-bit word");

enum { RV_MEAN = 0, RV_MEDIAN = 1, RV_SIGMA = 2 };

__device__ __forceinline__ double rv_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double rv_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

template <class Op> __device__ __forceinline__ double rv_reduce(double x, Op op, double *sh) {
    for (int o = 32; o >= 1; o >>= 1) x = op(x, __shfl_xor(x, o));
    const int nw = (int)(blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = sh[0];
    for (int i = 1; i < nw; ++i) r = op(r, sh[i]);
    return r;
}

// ------------------------------------------------------------------------------------------------ plan
// par: period | epoch_time, B each.  plan[b][LK_RIVER_NPLAN] as include/lkhip.h lists it.
__global__ __launch_bounds__(RV_PLAN_THREADS) void river_plan_kernel(const double *__restrict__ t, const double *__restrict__ flux,
                                                                      const double *__restrict__ err,
                                                                      const int64_t *__restrict__ n_off, int B,
                                                                      const double *__restrict__ par, int epoch_given,
                                                                      double *__restrict__ plan) {
    __shared__ unsigned long long sh[RV_PLAN_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    const double *tt = t + lo, *ff = flux + lo;
    const double P = par[b];
    const double t0 = n > 0 ? tt[0] : rv_qnan();
    const double e = epoch_given ? par[B + b] : t0;
    const double inf = rv_inf();
    double tmin = inf, tmax = -inf, fmx = 0.0, emx = 0.0, nfin = 0.0, bad = 0.0;
    long long c_f = 0, c_d = 0;
    for (int i = tid; i < n; i += nt) {
        const double ti = tt[i];
        if (isfinite(ti)) {
            tmin = fmin(tmin, ti);
            tmax = fmax(tmax, ti);
        } else {
            bad = 1.0;
        }
        if (i + 1 < n) {
            const double d = tt[i + 1] - ti;
            if (!(d >= 0.0)) bad = 1.0;  // (a NaN difference comes from a non-finite time)
            if (!isnan(d)) ++c_d;
        }
        const double f = ff[i];
        if (!isnan(f)) ++c_f;
        if (isfinite(f)) {
            nfin += 1.0;
            fmx = fmax(fmx, fabs(f));
        }
        if (err) {
            const double s = err[lo + i];
            if (isfinite(s)) emx = fmax(emx, fabs(s));
        }
    }
    auto mn = [](double a, double c) { return fmin(a, c); };
    auto mx = [](double a, double c) { return fmax(a, c); };
    auto ad = [](double a, double c) { return a + c; };
    double *shd = reinterpret_cast<double *>(sh);
    tmin = rv_reduce(tmin, mn, shd);
    tmax = rv_reduce(tmax, mx, shd);
    fmx = rv_reduce(fmx, mx, shd);
    emx = rv_reduce(emx, mx, shd);
    nfin = rv_reduce(nfin, ad, shd);  // (integer-valued, below 2^53: exact in any order)
    bad = rv_reduce(bad, mx, shd);
    __syncthreads();
    const long long n_f = block_count_dyn(c_f, reinterpret_cast<long long *>(sh));
    const long long n_d = block_count_dyn(c_d, reinterpret_cast<long long *>(sh));
    // np.nanmedian(flux) and np.nanmedian(np.diff(t)), the difference formed on the fly
    const double med = block_median(n, n_f, [&](int i) { return ff[i]; }, [&](int i) { return !isnan(ff[i]); }, sh);
    const double dt = block_median(
        n > 0 ? n - 1 : 0, n_d, [&](int i) { return tt[i + 1] - tt[i]; }, [&](int i) { return !isnan(tt[i + 1] - tt[i]); }, sh);
    if (tid == 0) {
        // the cycle is monotone in t (one subtraction, one division, floor): its extremes sit at the extreme finite times
        const bool any = tmin <= tmax;
        double *p = plan + (size_t)b * LK_RIVER_NPLAN;
        p[0] = med;
        p[1] = dt;
        p[2] = any ? fmin(fb_cycle(tmin, e, P), fb_cycle(tmax, e, P)) : 0.0;
        p[3] = any ? fmax(fb_cycle(tmin, e, P), fb_cycle(tmax, e, P)) : -1.0;
        p[4] = nfin;
        p[5] = bad > 0.0 ? 0.0 : 1.0;
        p[6] = t0;
        p[7] = fmx;
        p[8] = emx;
    }
}

// ------------------------------------------------------------------------------------------------ the image
// The column of a phase, or -1: an arithmetic guess corrected against the edge values, so membership is the comparison
// edges[j] < ph <= edges[j+1] and not a division (a phase equal to edges[0] is in no column; NaN fails the first test).
__device__ __forceinline__ int rv_locate(double ph, const double *__restrict__ edges, int nb, double inv_width) {
    if (!(ph > edges[0] && ph <= edges[nb])) return -1;
    int k = (int)fmin((ph - edges[0]) * inv_width, (double)(nb - 1));
    k = max(k, 0);
    while (k > 0 && ph <= edges[k]) --k;
    while (k + 1 < nb && ph > edges[k + 1]) ++k;
    return k;
}

// np.median of v[0..k), 1 <= k <= LK_RIVER_CELL_THREAD, by one thread: every value is ranked by counting (ties by position)
__device__ __forceinline__ double rv_thread_median(const double *v, int k) {
    const int ka = (k - 1) >> 1, kb = k >> 1;
    double a = 0.0, c = 0.0;
    for (int j = 0; j < k; ++j) {
        const double vj = v[j];
        const unsigned long long kj = f64_sortable(vj);
        int r = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned long long ki = f64_sortable(v[i]);
            r += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
        }
        if (r == ka) a = vj;
        if (r == kb) c = vj;
    }
    return ka == kb ? a : (a + c) * 0.5;
}

// tab: n_off (B + 1) | cell_off (B + 1) | edge_off (B + 1) | slab_off (B + 1, in doubles).  par: period | epoch | smallest cycle |
// median flux, B each.  ipar: n_bins | qf | qe, B each.  tiles: target, first row, end row, first column, end column per workgroup.
template <int METHOD>
__global__ __launch_bounds__(RV_THREADS) void river_kernel(const double *__restrict__ t, const double *__restrict__ flux,
                                                            const double *__restrict__ err, const int64_t *__restrict__ tab, int B,
                                                            const double *__restrict__ par, const int *__restrict__ ipar,
                                                            const int *__restrict__ tiles, const double *__restrict__ edges_all,
                                                            double *__restrict__ slab, double *__restrict__ river,
                                                            int32_t *__restrict__ count, int32_t *__restrict__ route) {
    __shared__ unsigned long long lds[RV_LDS_WORDS];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int *tile = tiles + (size_t)5 * blockIdx.x;
    const int b = tile[0], r0 = tile[1], r1 = tile[2], c0 = tile[3], c1 = tile[4];
    const int64_t lo = tab[b];
    const int n = (int)(tab[b + 1] - lo);
    const int nb = ipar[b];
    const int W = c1 - c0, C = (r1 - r0) * W;  // (the launcher made C <= LK_RIVER_LDS_CELLS)
    const double *tt = t + lo, *ff = flux + lo;
    const double *edges = edges_all + tab[2 * (size_t)(B + 1) + b];
    const double P = par[b], e = par[B + b], cmin = par[2 * B + b], med = par[3 * B + b];
    const FoldPar fp = fold_par(P, e, 0.0, 0.5, 1);
    const double inv_width = (double)nb / (edges[nb] - edges[0]);
    double *r_out = river + tab[(size_t)(B + 1) + b];
    int32_t *c_out = count + tab[(size_t)(B + 1) + b];
    auto out_index = [&](int c) { return (size_t)(r0 + c / W) * nb + c0 + c % W; };
    // the cadences of rows [r0, r1): the cycle is non-decreasing in t
    auto first_row_ge = [&](double r) {
        int a = 0, c = n;
        while (a < c) {
            const int mid = (a + c) >> 1;
            if (fb_cycle(tt[mid], e, P) - cmin >= r)
                c = mid;
            else
                a = mid + 1;
        }
        return a;
    };
    const int i0 = first_row_ge((double)r0), i1 = first_row_ge((double)r1);
    // the cell of cadence i inside this tile and its y, or -1 (membership per cadence; the range only bounds the stream)
    auto cell_of = [&](int i, double *y) {
        const double ti = tt[i];
        const double rr = fb_cycle(ti, e, P) - cmin;
        if (!(rr >= (double)r0 && rr < (double)r1)) return -1;
        const int col = rv_locate(fold_phase(fp, ti), edges, nb, inv_width);
        if (col < c0 || col >= c1) return -1;
        *y = ff[i] / med;
        if (!isfinite(*y)) return -1;
        return ((int)rr - r0) * W + (col - c0);
    };
    int bits = c1 - c0 == nb ? LK_RIVER_ROUTE_ROWS : LK_RIVER_ROUTE_COLUMNS;

    if (METHOD != RV_MEDIAN) {
        long long *sf = reinterpret_cast<long long *>(lds), *se = sf + RV_CELLS;
        int *cnt = reinterpret_cast<int *>(se + RV_CELLS);
        const int qf = ipar[B + b], qe = ipar[2 * B + b];
        for (int c = tid; c < C; c += nt) sf[c] = 0, se[c] = 0, cnt[c] = 0;
        __syncthreads();
        for (int i = i0 + tid; i < i1; i += nt) {
            double y;
            const int c = cell_of(i, &y);
            if (c < 0) continue;
            atomicAdd(cnt + c, 1);
            atomicAdd(reinterpret_cast<unsigned long long *>(sf + c), (unsigned long long)llrint(ldexp(y, -qf)));
            if (METHOD == RV_SIGMA) {
                const double u = err[lo + i] / med;
                if (!isnan(u)) {
                    const double x = u * u;
                    if (isinf(x))
                        atomicOr(cnt + c, RV_INF_FLAG);
                    else
                        atomicAdd(reinterpret_cast<unsigned long long *>(se + c), (unsigned long long)llrint(ldexp(x, -qe)));
                }
            }
        }
        __syncthreads();
        for (int c = tid; c < C; c += nt) {
            const int k = cnt[c] & (RV_INF_FLAG - 1);
            double v = rv_qnan();
            if (k) {
                v = ldexp((double)sf[c], qf) / (double)k;
                if (METHOD == RV_SIGMA) {
                    const double s2 = (cnt[c] & RV_INF_FLAG) ? rv_inf() : ldexp((double)se[c], qe);
                    v = (v - 1.0) / sqrt(s2);
                }
            }
            const size_t o = out_index(c);
            r_out[o] = v;
            c_out[o] = k;
        }
    } else {
        int *cnt = reinterpret_cast<int *>(lds), *cur = cnt + RV_CELLS;
        double *vals_lds = reinterpret_cast<double *>(lds + RV_CELLS);
        unsigned long long *sh = lds + RV_CELLS + RV_VALS;
        for (int c = tid; c < C; c += nt) cnt[c] = 0;
        __syncthreads();
        for (int i = i0 + tid; i < i1; i += nt) {
            double y;
            const int c = cell_of(i, &y);
            if (c >= 0) atomicAdd(cnt + c, 1);
        }
        __syncthreads();
        // cur[c] = first slot of cell c: thread-contiguous chunks of cells, one workgroup scan of the chunk totals
        const int per = (C + nt - 1) / nt, cb = tid * per;
        int local = 0;
        for (int u = 0; u < per; ++u)
            if (cb + u < C) local += cnt[cb + u];
        int total;
        int run = block_exscan_int(local, reinterpret_cast<int *>(sh), &total);
        for (int u = 0; u < per; ++u)
            if (cb + u < C) {
                cur[cb + u] = run;
                run += cnt[cb + u];
            }
        // more values than LDS holds (duplicate times, hundreds of cadences per cell): the tile's slab of device scratch, touched
        // by this workgroup only.  Whole-row tiles of a target have disjoint cadence ranges and total <= i1 - i0; column chunk q
        // of a row has its own copy of the target's range
        const bool in_lds = total <= RV_VALS;
        double *vals = in_lds ? vals_lds : slab + tab[3 * (size_t)(B + 1) + b] + (size_t)(c0 / RV_CELLS) * n + i0;
        bits |= in_lds ? LK_RIVER_ROUTE_VALS_LDS : LK_RIVER_ROUTE_VALS_SCRATCH;
        __syncthreads();
        for (int i = i0 + tid; i < i1; i += nt) {
            double y;
            const int c = cell_of(i, &y);
            if (c >= 0) vals[atomicAdd(cur + c, 1)] = y;
        }
        if (!in_lds) __threadfence();
        __syncthreads();
        // cur[c] is now the END of cell c's segment
        int small = 0, big = 0;
        for (int c = tid; c < C; c += nt) {
            const int k = cnt[c];
            if (k > LK_RIVER_CELL_THREAD) {
                big = 1;
                continue;
            }
            small |= k > 0 ? 1 : 0;
            const size_t o = out_index(c);
            r_out[o] = k ? rv_thread_median(vals + (cur[c] - k), k) : rv_qnan();
            c_out[o] = k;
        }
        small = __syncthreads_or(small);
        big = __syncthreads_or(big);
        if (small) bits |= LK_RIVER_ROUTE_CELL_THREAD;
        if (big) {
            bits |= LK_RIVER_ROUTE_CELL_GROUP;
            for (int c = 0; c < C; ++c) {
                const int k = cnt[c];  // (the same in every thread: the branch is workgroup-uniform)
                if (k <= LK_RIVER_CELL_THREAD) continue;
                const double *v = vals + (cur[c] - k);
                const double m = block_median(k, (long long)k, [&](int i) { return v[i]; }, [](int) { return true; }, sh);
                if (tid == 0) {
                    const size_t o = out_index(c);
                    r_out[o] = m;
                    c_out[o] = k;
                }
            }
        }
    }
    if (route && tid == 0) atomicOr(route + b, bits);
}

// ------------------------------------------------------------------------------------------------ launchers
namespace {
int rv_check_batch(int B, const int64_t *n_off_host) {
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)n);
    }
    return LK_OK;
}

// exponent e of the quantum 2^e: n addends of at most vmax sum to less than 2^62 quanta (foldbin.hip's rule)
int rv_quantum_exp(double vmax, int64_t n) {
    if (!(vmax > 0.0)) return 0;
    if (!std::isfinite(vmax)) vmax = 1.7976931348623157e308;
    int L = 0;
    while (((int64_t)1 << L) < n) ++L;
    return std::ilogb(vmax) + 1 + L - 62;
}
}  // namespace

int river_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                      const double *period_host, const double *epoch_time_host, int epoch_given, double *plan_host,
                      hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && period_host && plan_host && (epoch_time_host || !epoch_given), "NULL buffer");
    if (const int rc = rv_check_batch(B, n_off_host)) return rc;
    std::vector<double> par((size_t)2 * B, 0.0);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(std::isfinite(period_host[b]) && period_host[b] > 0.0, "target %d: period must be finite and positive", b);
        par[b] = period_host[b];
        if (epoch_given) par[(size_t)B + b] = epoch_time_host[b];
    }
    int64_t *d_off;
    double *d_par, *d_plan;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, (size_t)B + 1).upload(d_par, par.data(), par.size())
            .buf(d_plan, (size_t)B * LK_RIVER_NPLAN).carve(stream))
        return rc;
    hipLaunchKernelGGL(river_plan_kernel, dim3(B), dim3(RV_PLAN_THREADS), 0, stream, t, flux, err, d_off, B, d_par, epoch_given,
                       d_plan);
    LK_HIP_CHECK(hipGetLastError());
    LK_HIP_CHECK(hipMemcpyAsync(plan_host, d_plan, (size_t)B * LK_RIVER_NPLAN * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    return LK_OK;
}

int river_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                 const double *period_host, const double *epoch_time_host, const double *plan_host, int method,
                 const int32_t *n_bins_host, const int32_t *n_cycles_host, const int64_t *cell_off_host, const double *edges_host,
                 double *river, int32_t *count, int32_t *route, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && period_host && epoch_time_host && plan_host && n_bins_host && n_cycles_host && cell_off_host &&
                   edges_host && river && count,
               "NULL buffer");
    LK_REQUIRE(method == RV_MEAN || method == RV_MEDIAN || method == RV_SIGMA, "method must be 0 (mean), 1 (median) or 2 (sigma)");
    LK_REQUIRE(method != RV_SIGMA || err != nullptr, "method sigma needs flux_err");
    if (const int rc = rv_check_batch(B, n_off_host)) return rc;
    LK_REQUIRE(cell_off_host[0] == 0, "cell_off must be prefix offsets starting at 0");
    std::vector<int64_t> tab((size_t)4 * (B + 1), 0);
    std::vector<double> par((size_t)4 * B, 0.0);
    std::vector<int> ipar((size_t)3 * B, 0), tiles;
    int64_t *cell_off = tab.data() + (size_t)(B + 1), *edge_off = tab.data() + 2 * (size_t)(B + 1),
            *slab_off = tab.data() + 3 * (size_t)(B + 1);
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        const int64_t nb = n_bins_host[b], nc = n_cycles_host[b];
        const double *pl = plan_host + (size_t)b * LK_RIVER_NPLAN;
        LK_REQUIRE(nb >= 0 && nc >= 0, "target %d: negative n_bins or n_cycles", b);
        const int64_t cells = nb * nc;
        LK_REQUIRE(cell_off_host[b + 1] - cell_off_host[b] == cells, "target %d: cell_off does not match n_cycles x n_bins", b);
        tab[b + 1] = n_off_host[b + 1];
        cell_off[b + 1] = cell_off_host[b + 1];
        edge_off[b + 1] = edge_off[b] + nb + 1;
        slab_off[b + 1] = slab_off[b];
        if (cells == 0) continue;
        LK_REQUIRE(nb < ((int64_t)1 << 30) && nc < ((int64_t)1 << 30), "target %d: too many bins or cycles", b);
        const double P = period_host[b], med = pl[0];
        LK_REQUIRE(std::isfinite(P) && P > 0.0, "target %d: period must be finite and positive", b);
        LK_REQUIRE(std::isfinite(epoch_time_host[b]), "target %d: epoch_time must be finite", b);
        LK_REQUIRE(std::isfinite(med) && med != 0.0, "target %d: the median flux must be finite and non-zero", b);
        LK_REQUIRE(std::isfinite(pl[2]) && pl[3] - pl[2] + 1.0 == (double)nc, "target %d: n_cycles does not match the plan", b);
        const double *ed = edges_host + edge_off[b];
        for (int64_t k = 0; k < nb; ++k)
            LK_REQUIRE(ed[k + 1] > ed[k], "target %d: bin edges must be strictly increasing (edge %lld)", b, (long long)(k + 1));
        LK_REQUIRE(std::isfinite(ed[0]) && std::isfinite(ed[nb]), "target %d: bin edges must be finite", b);
        par[b] = P;
        par[(size_t)B + b] = epoch_time_host[b];
        par[(size_t)2 * B + b] = pl[2];
        par[(size_t)3 * B + b] = med;
        ipar[b] = (int)nb;
        const double ymax = pl[7] / std::fabs(med), umax = pl[8] / std::fabs(med);
        ipar[(size_t)B + b] = rv_quantum_exp(ymax, n);
        ipar[(size_t)2 * B + b] = rv_quantum_exp(umax * umax, n);
        if (nb <= RV_CELLS) {
            // whole rows: as many as LDS has cells for; median: not more than the LDS value list is expected to hold (a cycle
            // has about P / dt cadences) — a property of the target alone, a fuller tile goes through its slab
            int64_t R = RV_CELLS / nb;
            if (method == RV_MEDIAN && pl[1] > 0.0) {
                const double per_cycle = P / pl[1];
                if (per_cycle * (double)R > (double)RV_VALS) R = std::max<int64_t>(1, (int64_t)((double)RV_VALS / per_cycle));
            }
            for (int64_t r = 0; r < nc; r += R) {
                const int row[5] = {b, (int)r, (int)std::min(r + R, nc), 0, (int)nb};
                tiles.insert(tiles.end(), row, row + 5);
            }
            if (method == RV_MEDIAN) slab_off[b + 1] += n;
        } else {
            const int64_t chunks = (nb + RV_CELLS - 1) / RV_CELLS;
            LK_REQUIRE(nc * chunks < ((int64_t)1 << 28), "target %d: too many tiles (%lld rows x %lld column chunks)", b,
                       (long long)nc, (long long)chunks);
            for (int64_t r = 0; r < nc; ++r)
                for (int64_t c = 0; c < nb; c += RV_CELLS) {
                    const int row[5] = {b, (int)r, (int)r + 1, (int)c, (int)std::min(c + RV_CELLS, nb)};
                    tiles.insert(tiles.end(), row, row + 5);
                }
            if (method == RV_MEDIAN) slab_off[b + 1] += n * chunks;
        }
        LK_REQUIRE(tiles.size() / 5 < ((size_t)1 << 30), "too many tiles for one call: split the batch");
    }
    if (route) LK_HIP_CHECK(hipMemsetAsync(route, 0, (size_t)B * sizeof(int32_t), stream));
    const size_t n_tiles = tiles.size() / 5;
    if (n_tiles == 0) return LK_OK;
    int64_t *d_tab;
    double *d_par, *d_edges, *d_slab;
    int *d_ipar, *d_tiles;
    if (const int rc = Scratch(h, h->ws).upload(d_tab, tab.data(), tab.size()).upload(d_par, par.data(), par.size())
            .upload(d_ipar, ipar.data(), ipar.size()).upload(d_tiles, tiles.data(), tiles.size())
            .upload(d_edges, edges_host, (size_t)edge_off[B]).buf(d_slab, (size_t)slab_off[B]).carve(stream))
        return rc;
    const dim3 grid((unsigned)n_tiles), block(RV_THREADS);
    if (method == RV_MEAN)
        hipLaunchKernelGGL(river_kernel<RV_MEAN>, grid, block, 0, stream, t, flux, err, d_tab, B, d_par, d_ipar, d_tiles, d_edges,
                           d_slab, river, count, route);
    else if (method == RV_MEDIAN)
        hipLaunchKernelGGL(river_kernel<RV_MEDIAN>, grid, block, 0, stream, t, flux, err, d_tab, B, d_par, d_ipar, d_tiles, d_edges,
                           d_slab, river, count, route);
    else
        hipLaunchKernelGGL(river_kernel<RV_SIGMA>, grid, block, 0, stream, t, flux, err, d_tab, B, d_par, d_ipar, d_tiles, d_edges,
                           d_slab, river, count, route);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
