// interp.hip — CotrendingBasisVectors.interpolate for a ragged resident batch on gfx950: K shared columns (the basis vectors of
// one channel) given on Nx knots are interpolated to every target's own times and written as the targets' design matrices.
//
// Reference: src/lightkurve/correctors/cbvcorrector.py CotrendingBasisVectors.interpolate — every vector through
// scipy.interpolate.PchipInterpolator(cbv_time[~gap], vector[~gap], extrapolate=...) evaluated at lc.time.  scipy
// (interpolate/_cubic.py): the derivatives at the knots come from _find_derivatives / _edge_case, the piecewise cubic from
// CubicHermiteSpline's coefficients.  correctors/cbvcorrector.py interpolate_cbvs is the same arithmetic in numpy, operation for
// operation (this file is built with -ffp-contract=off for that).
//
//   knot_compact_kernel   the indices of the knots that are kept (knot_keep != 0), in order, and their number
//   knot_check_kernel     kept knot times finite and strictly increasing, kept values finite
//   knot_gather_kernel    the kept rows of (knot_time, Y) packed
//   pchip_slopes_kernel   D[j][k], one thread per (knot, column)
//   pchip_eval_kernel     one workgroup per tile of PI_TILE cadences of one target -> X_out rows, inside bytes
//   pchip_inside_kernel   the inside bytes alone (X_out == NULL)
//
// Every output element depends on its own time, the knots and the column alone: nothing is reduced across cadences, so a
// target's rows have the same bits whatever the batch, the tile or the lookup route.
#include <algorithm>
#include <cmath>

#include "lk_common.hpp"

namespace lk {

constexpr int PI_TILE = 256;          // cadences per workgroup of pchip_eval_kernel (tests/test_cbv_interp_gpu.py names it)
constexpr int PI_LDS_KNOTS = 2048;    // knot times a workgroup keeps in LDS (16 KB); a tile that spans more searches global memory

__global__ __launch_bounds__(1024) void knot_compact_kernel(const uint8_t *__restrict__ keep, int Nx, int *__restrict__ kidx,
                                                             int *__restrict__ st) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int j0 = 0; j0 < Nx; j0 += 1024) {
        const int j = j0 + tid;
        const bool on = j < Nx && keep[j] != 0;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0;
            total += s_w[w];
        }
        if (on) kidx[base + before + __popcll(bal & ((1ull << lane) - 1ull))] = j;
        base += total;
        __syncthreads();
    }
    if (tid == 0) st[0] = base;
}

// st[0]: the number of kept knots; st[1] |= 1: a kept time is not finite or not above the kept time before it, |= 2: a kept
// value is not finite.  kidx nullable: every knot is kept.
__global__ __launch_bounds__(256) void knot_check_kernel(const double *__restrict__ x, const double *__restrict__ Y, int K,
                                                          const int *__restrict__ kidx, int *__restrict__ st) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= st[0]) return;
    const int r = kidx ? kidx[j] : j;
    const double xv = x[r];
    int bad = 0;
    if (!isfinite(xv)) bad |= 1;
    if (j > 0 && !(x[kidx ? kidx[j - 1] : j - 1] < xv)) bad |= 1;
    for (int k = 0; k < K; ++k)
        if (!isfinite(Y[(size_t)r * K + k])) bad |= 2;
    if (bad) atomicOr(st + 1, bad);
}

__global__ __launch_bounds__(256) void knot_gather_kernel(const double *__restrict__ x, const double *__restrict__ Y, int K,
                                                           const int *__restrict__ kidx, int Nk, double *__restrict__ xk,
                                                           double *__restrict__ Yk) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Nk * K) return;
    const int j = e / K, k = e - j * K, r = kidx[j];
    Yk[e] = Y[(size_t)r * K + k];
    if (k == 0) xk[j] = x[r];
}

__device__ __forceinline__ int pchip_sign(double v) { return (v > 0.0) - (v < 0.0); }

// scipy's PchipInterpolator._edge_case: the three-point end derivative, kept shape-preserving
__device__ __forceinline__ double pchip_edge(double h0, double h1, double m0, double m1) {
    const double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
    if (pchip_sign(d) != pchip_sign(m0)) return 0.0;
    if (pchip_sign(m0) != pchip_sign(m1) && fabs(d) > 3.0 * fabs(m0)) return 3.0 * m0;
    return d;
}

// D[j][k]: scipy's PchipInterpolator._find_derivatives on Nx >= 2 knots, x strictly increasing, Y finite (Nx x K row-major)
__global__ __launch_bounds__(256) void pchip_slopes_kernel(const double *__restrict__ x, const double *__restrict__ Y, int Nx, int K,
                                                            double *__restrict__ D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Nx * K) return;
    const int j = e / K, k = e - j * K;
    auto secant = [&](int a) { return (Y[(size_t)(a + 1) * K + k] - Y[(size_t)a * K + k]) / (x[a + 1] - x[a]); };
    double d;
    if (Nx == 2) {
        d = secant(0);
    } else if (j == 0) {
        d = pchip_edge(x[1] - x[0], x[2] - x[1], secant(0), secant(1));
    } else if (j == Nx - 1) {
        d = pchip_edge(x[Nx - 1] - x[Nx - 2], x[Nx - 2] - x[Nx - 3], secant(Nx - 2), secant(Nx - 3));
    } else {
        const double hm = x[j] - x[j - 1], hp = x[j + 1] - x[j], mm = secant(j - 1), mp = secant(j);
        if (pchip_sign(mm) != pchip_sign(mp) || mm == 0.0 || mp == 0.0) {
            d = 0.0;
        } else {
            const double w1 = 2.0 * hp + hm, w2 = hp + 2.0 * hm;
            const double whmean = (w1 / mm + w2 / mp) / (w1 + w2);
            d = 1.0 / whmean;
        }
    }
    D[e] = d;
}

// numpy.searchsorted(a[0..n), v, 'right'): the number of entries <= v (v is not NaN)
__device__ __forceinline__ int upper_bound_f64(const double *a, int n, double v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One workgroup = the cadences [blockIdx.x PI_TILE, + PI_TILE) of target blockIdx.y.
//  1. the smallest and largest time of the tile (NaN left out) give the knot intervals [glo, ghi] the tile can touch: two
//     searches of the whole knot vector by one thread.  Up to PI_LDS_KNOTS knot times of that range go to LDS and every lane
//     searches there (a sorted light curve: a few knots, or a few hundred); a wider range — many knots per query, or a target
//     whose times are not sorted — searches global memory.  Both give numpy's interval, so the route changes no bit.
//  2. per cadence: interval i, s = t - x[i], dx = x[i + 1] - x[i] and two flag bits, in LDS.
//  3. the lanes walk the flattened (cadence, column) index of the tile's Kout-wide output rows, so a wave stores 512
//     contiguous bytes; the per-cadence values come from LDS, Y and D from the cache.
__global__ __launch_bounds__(PI_TILE) void pchip_eval_kernel(const double *__restrict__ t, const int64_t *__restrict__ n_off,
                                                              const double *__restrict__ x, const double *__restrict__ Y,
                                                              const double *__restrict__ D, int Nx, int K, int extrapolate,
                                                              int append_constant, double *__restrict__ X_out,
                                                              uint8_t *__restrict__ inside) {
    __shared__ double s_x[PI_LDS_KNOTS];
    __shared__ double s_s[PI_TILE], s_dx[PI_TILE];
    __shared__ int s_i[PI_TILE];
    __shared__ unsigned char s_f[PI_TILE];
    __shared__ double s_min[PI_TILE / 64], s_max[PI_TILE / 64];
    __shared__ int s_rng[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo), c0 = blockIdx.x * PI_TILE;
    if (c0 >= n) return;
    const int nc = min(PI_TILE, n - c0);
    const bool live = tid < nc;
    const double tv = live ? t[lo + c0 + tid] : nan("");
    const bool num = tv == tv;
    double tmin = num ? tv : INFINITY, tmax = num ? tv : -INFINITY;
    for (int sh = 32; sh >= 1; sh >>= 1) {
        tmin = fmin(tmin, __shfl_xor(tmin, sh));
        tmax = fmax(tmax, __shfl_xor(tmax, sh));
    }
    if ((tid & 63) == 0) s_min[tid >> 6] = tmin, s_max[tid >> 6] = tmax;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PI_TILE / 64; ++w) tmin = fmin(tmin, s_min[w]), tmax = fmax(tmax, s_max[w]);
        const int glo = min(max(upper_bound_f64(x, Nx, tmin) - 1, 0), Nx - 2);
        const int ghi = max(min(max(upper_bound_f64(x, Nx, tmax) - 1, 0), Nx - 2), glo);
        s_rng[0] = glo, s_rng[1] = ghi;
    }
    __syncthreads();
    const int glo = s_rng[0], ghi = s_rng[1], cnt = ghi - glo + 2;  // knots glo .. ghi + 1 <= Nx - 1
    const bool in_lds = cnt <= PI_LDS_KNOTS;
    if (in_lds) {
        for (int j = tid; j < cnt; j += PI_TILE) s_x[j] = x[glo + j];
        __syncthreads();
    }
    const double x_first = x[0], x_last = x[Nx - 1];
    const bool is_in = tv >= x_first && tv <= x_last;  // false for NaN
    if (live) {
        int iv = glo;
        double xa = 0.0, xb = 1.0;
        if (num) {
            if (in_lds) {
                iv = min(max(glo + upper_bound_f64(s_x, cnt, tv) - 1, glo), ghi);
                xa = s_x[iv - glo], xb = s_x[iv - glo + 1];
            } else {
                iv = min(max(upper_bound_f64(x, Nx, tv) - 1, 0), Nx - 2);
                xa = x[iv], xb = x[iv + 1];
            }
        }
        s_i[tid] = iv;
        s_s[tid] = tv - xa;
        s_dx[tid] = xb - xa;
        s_f[tid] = (unsigned char)(((!num || (!is_in && !extrapolate)) ? 1 : 0) | (tv == x_last ? 2 : 0));
        if (inside) inside[lo + c0 + tid] = is_in ? 1 : 0;
    }
    __syncthreads();
    const int Kout = K + (append_constant ? 1 : 0), total = nc * Kout;
    const int qK = PI_TILE / Kout, rK = PI_TILE - qK * Kout;
    double *__restrict__ out = X_out + (size_t)(lo + c0) * Kout;
    int c = tid / Kout, k = tid - c * Kout;
    for (int e = tid; e < total; e += PI_TILE) {
        double v;
        if (k == K) {
            v = 1.0;
        } else {
            const int f = s_f[c];
            if (f & 1) {
                v = nan("");
            } else {
                const size_t a = (size_t)s_i[c] * K + k;
                const double y0 = Y[a], y1 = Y[a + K];
                if (f & 2) {
                    v = y1;  // the last knot itself: s = dx there, and the cubic's value is y1 only up to rounding
                } else {
                    const double d0 = D[a], d1 = D[a + K], dx = s_dx[c], s = s_s[c];
                    const double sl = (y1 - y0) / dx, tt = (d0 + d1 - 2.0 * sl) / dx;
                    const double q0 = tt / dx, q1 = (sl - d0) / dx - tt;
                    v = y0 + s * (d0 + s * (q1 + s * q0));
                }
            }
        }
        out[e] = v;
        k += rK, c += qK;
        if (k >= Kout) k -= Kout, ++c;
    }
}

__global__ __launch_bounds__(256) void pchip_inside_kernel(const double *__restrict__ t, int64_t ntot, const double *__restrict__ x,
                                                            int Nx, uint8_t *__restrict__ inside) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ntot) return;
    const double tv = t[i];
    inside[i] = (tv >= x[0] && tv <= x[Nx - 1]) ? 1 : 0;
}

int pchip_interp_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, int Nx, int K, const double *knot_time,
                        const double *Y, const uint8_t *knot_keep, int extrapolate, int append_constant, double *X_out,
                        uint8_t *inside, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    LK_REQUIRE(K >= 1, "K must be >= 1 (got %d)", K);
    LK_REQUIRE(Nx >= 2, "interpolation needs at least 2 knots (got %d)", Nx);
    LK_REQUIRE((int64_t)Nx * K < ((int64_t)1 << 31) && K < (1 << 20), "Nx=%d knots x K=%d columns: too many values", Nx, K);
    LK_REQUIRE(knot_time && Y, "NULL buffer");
    LK_REQUIRE(B <= 65535, "at most 65535 targets per call on this path (got %d): split the batch", B);
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    int64_t nmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t nb = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(nb >= 0 && nb < ((int64_t)1 << 30), "target %d: %lld cadences outside 0..2^30", b, (long long)nb);
        nmax = std::max(nmax, nb);
    }
    const int64_t ntot = n_off_host[B];
    LK_REQUIRE(ntot == 0 || (t && (X_out || inside)), "NULL buffer");
    const size_t nk = (size_t)Nx * K;
    const bool masked = knot_keep != nullptr;
    const int init[2] = {masked ? 0 : Nx, 0};
    int64_t *d_off;
    int *d_st, *d_kidx;
    double *d_xk, *d_Yk, *d_D;
    Scratch ws(h, h->ws);
    ws.upload(d_off, n_off_host, (size_t)B + 1)
        .upload(d_st, init, 2)
        .buf(d_kidx, (size_t)Nx, masked)
        .buf(d_xk, (size_t)Nx, masked)
        .buf(d_Yk, nk, masked)
        .buf(d_D, nk, X_out != nullptr);
    if (const int rc = ws.carve(stream)) return rc;
    if (masked) hipLaunchKernelGGL(knot_compact_kernel, dim3(1), dim3(1024), 0, stream, knot_keep, Nx, d_kidx, d_st);
    hipLaunchKernelGGL(knot_check_kernel, dim3((Nx + 255) / 256), dim3(256), 0, stream, knot_time, Y, K, (const int *)d_kidx, d_st);
    LK_HIP_CHECK(hipGetLastError());
    int st[2] = {0, 0};
    LK_HIP_CHECK(hipMemcpyAsync(st, d_st, 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    const int Nk = st[0];
    LK_REQUIRE(Nk >= 2 && Nk <= Nx, "interpolation needs at least 2 kept knots (knot_keep leaves %d of %d)", Nk, Nx);
    LK_REQUIRE(!(st[1] & 1), "the kept knot times must be finite and strictly increasing");
    LK_REQUIRE(!(st[1] & 2), "the columns must be finite at every kept knot");
    if (B == 0 || ntot == 0) return LK_OK;
    const double *xs = knot_time, *Ys = Y;
    if (masked) {
        hipLaunchKernelGGL(knot_gather_kernel, dim3((unsigned)(((size_t)Nk * K + 255) / 256)), dim3(256), 0, stream, knot_time, Y, K,
                           (const int *)d_kidx, Nk, d_xk, d_Yk);
        xs = d_xk, Ys = d_Yk;
    }
    if (X_out) {
        hipLaunchKernelGGL(pchip_slopes_kernel, dim3((unsigned)(((size_t)Nk * K + 255) / 256)), dim3(256), 0, stream, xs, Ys, Nk, K,
                           d_D);
        hipLaunchKernelGGL(pchip_eval_kernel, dim3((unsigned)((nmax + PI_TILE - 1) / PI_TILE), B), dim3(PI_TILE), 0, stream, t,
                           (const int64_t *)d_off, xs, Ys, (const double *)d_D, Nk, K, extrapolate ? 1 : 0, append_constant ? 1 : 0,
                           X_out, inside);
    } else {
        hipLaunchKernelGGL(pchip_inside_kernel, dim3((unsigned)((ntot + 255) / 256)), dim3(256), 0, stream, t, ntot, xs, Nk, inside);
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
