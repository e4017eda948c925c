// pixelpg.hip — per-pixel Lomb-Scargle periodograms of resident pixel cubes on gfx950: which pixels of a cutout vary, and at
// which frequency (what TargetPixelFile.plot_pixels(periodogram=True) loops for).  The frequency-grid generalisation of
// ampimage.hip's accumulation with the closed form of ls.hip (ls_epilogue.hpp) as its epilogue.
//
// Reference: PixelCube.pixel_periodogram (correctors/pldcorrector.py), plain float64 numpy: pixel p of cutout b is taken on the
// cadences where the time is finite and its own flux is not NaN, n_used[p] of them, unit weights; its spectrum on the shared grid
// of F frequencies is astropy's floating-mean GLS with the exact sums and lightkurve's scaling.  All pixels of a cutout share
// the cadences and the weights, so of the six sums of the closed form S, C, S2, C2 belong to the (cutout, frequency) and only
// Sh = sum y sin, Ch = sum y cos to the pixel: 2 fp64 FMAs per (cadence, frequency, pixel).
//
//   stats    one thread per pixel walks its cadences in order: the pivot (its first value), n_used, sum y' (y' = y - pivot,
//            exact in float64: the sums below do not carry the pedestal), its first and last used cadence (the 'psd' scale);
//            n_valid[b] and status[b]; whether any pixel of a group of PP_T pixels lacks cadences that the cutout has.
//   spectra  workgroup (cutout, tile of PP_FT frequencies, group of PP_T adjacent pixels), lanes = pixels.  It walks all N
//            cadences in chunks of PP_CH.  For a chunk every lane generates the sine and cosine of a different (cadence,
//            frequency) — (t - t_ref) and the exactly reduced product of sincos2pi_prod (ls_epilogue.hpp), no recurrence — into LDS and
//            keeps, for the cadences IT generated, the shared sums of its frequency; then every lane walks its pixel down the
//            chunk (coalesced float32 row loads, PP_ROWS in flight) and folds y' into its 2 PP_FT register accumulators, the
//            trig values read as LDS broadcasts.  At the end the shared sums are added across the generating lanes in lane
//            order, and the lane applies the closed form per frequency: the mean goes back through S, C (sum (y' - d) sin =
//            sum y' sin - d S with d = sum y' / n), the power is stored [b][f][p] (pixel fastest: coalesced) where asked for,
//            and the tile's peak (first index of the largest non-NaN power) goes to scratch.
//            Two instantiations of the one body: MISS = false for pixel groups where no fitted pixel lacks a cadence (a NaN
//            is a select to zero, nothing else), MISS = true for the others: on the NaN branch a lane adds what the cadence
//            contributes to the shared sums of every frequency, and the epilogue takes that off.  Both are launched; a
//            workgroup whose group is the other kind returns at once, so groups without NaNs do not carry the 4 PP_FT extra
//            accumulators.  The data sums are the same expressions in the same order in both.
//   peaks    one thread per pixel: the tiles' peaks in tile order -> peak_power, peak_index.
//
// No floating-point atomics; the order of every sum depends on N (and the tile constants) alone, so a cutout's outputs have the
// same bits alone, at any batch position, with or without the power cube and from run to run.  Rows of cadences with an invalid
// time are not loaded; flux_err is not read.
#include <cmath>
#include <vector>

#include "lk_common.hpp"
#include "ls_epilogue.hpp"

namespace lk {

namespace {

constexpr int PP_T = 128;    // pixels per group: adjacent pixels of one cadence row
constexpr int PP_W = 64;     // lanes of a spectra workgroup: one wavefront
constexpr int PP_FT = 16;    // frequencies per workgroup: 2 PP_FT float64 accumulators per lane
constexpr int PP_CH = 32;    // cadences per staged chunk: PP_CH x PP_FT (sin, cos) pairs = 8 KB of LDS
constexpr int PP_ROWS = 8;   // cadence rows whose loads a lane issues before it uses them
constexpr int PP_GJ = PP_W / PP_FT;  // lanes that generate one frequency's values of a chunk (cadences r = gj, gj + PP_GJ, ...)
static_assert(PP_CH % PP_GJ == 0 && PP_CH % PP_ROWS == 0 && PP_W >= 4 * PP_FT, "tile constants");

}  // namespace

// One thread per pixel, workgroup (pixel group, cutout).  pivot, sy: [B][npix]; n_used (the output image): the pixel's values at
// the cadences with a finite time, 0 for a cutout with fewer than 4 of those (status 2); first / last: its first and last used
// cadence; n_valid[b], status[b] (pixel 0); gmiss[b][group] = 1 where a pixel with 4 or more values lacks a valid cadence.
__global__ __launch_bounds__(PP_T) void cube_pixelpg_stats_kernel(const double *__restrict__ time, const float *__restrict__ flux,
                                                                  int N, int npix, double *__restrict__ pivot,
                                                                  double *__restrict__ sy, int *__restrict__ n_used,
                                                                  int *__restrict__ first, int *__restrict__ last,
                                                                  int *__restrict__ n_valid, int *__restrict__ status,
                                                                  int *__restrict__ gmiss) {
    const int b = blockIdx.y, p = blockIdx.x * PP_T + threadIdx.x;
    const bool act = p < npix;
    const double *tm = time + (size_t)b * N;
    const float *f = flux + (size_t)b * N * npix + (act ? p : 0);
    int n = 0, nv = 0, i_first = 0, i_last = 0;
    double pv = 0.0, s = 0.0;
    for (int i0 = 0; i0 < N; i0 += PP_ROWS) {
        float v[PP_ROWS];
        bool ok[PP_ROWS];
#pragma unroll
        for (int u = 0; u < PP_ROWS; ++u) {
            ok[u] = i0 + u < N && isfinite(tm[min(i0 + u, N - 1)]);
            v[u] = ok[u] && act ? f[(size_t)(i0 + u) * npix] : NAN;
        }
#pragma unroll
        for (int u = 0; u < PP_ROWS; ++u) {
            if (!ok[u]) continue;
            ++nv;
            if (isnan(v[u])) continue;
            if (n == 0) {
                pv = isfinite(v[u]) ? (double)v[u] : 0.0;
                i_first = i0 + u;
            }
            ++n;
            s += (double)v[u] - pv;
            i_last = i0 + u;
        }
    }
    const bool fitted = nv >= 4;
    if (act) {
        const size_t o = (size_t)b * npix + p;
        pivot[o] = pv;
        sy[o] = s;
        n_used[o] = fitted ? n : 0;
        first[o] = i_first;
        last[o] = i_last;
    }
    if (p == 0) {
        n_valid[b] = nv;
        status[b] = fitted ? 0 : 2;
    }
    const int any = __syncthreads_or(act && fitted && n >= 4 && n != nv);
    if (threadIdx.x == 0) gmiss[(size_t)b * gridDim.x + blockIdx.x] = any ? 1 : 0;
}

// Workgroup = one wavefront for (cutout, frequency tile, pixel group[, half]); blocks are dealt so that all workgroups of a cutout
// run on one XCD (block i runs on XCD i % 8, as in ls.hip): the cutout's rows are then served by that XCD's L2 for all of its
// frequency tiles.  PPL pixels per lane (p, p + 64, ...): one LDS broadcast of (sin, cos) feeds 2 PPL FMAs.  MISS = false runs
// with PPL = 2 (a group of PP_T pixels per wavefront), MISS = true with PPL = 1 and two wavefronts per group: its lanes carry the 4
// PP_FT sums of the cadences they miss as well.  The generating lanes and the order of every sum are the same in both.
// power (nullable): [B][F][npix].  tile_peak / tile_idx: [B][ftiles][npix], NaN / -1 for a pixel without a finite power in the tile.
template <bool MISS, int PPL>
__global__ __launch_bounds__(PP_W) void cube_pixelpg_spectra_kernel(
    const double *__restrict__ time, const float *__restrict__ flux, const double *__restrict__ freq, const double *__restrict__ t_ref,
    const double *__restrict__ pivot, const double *__restrict__ sy, const int *__restrict__ n_used, const int *__restrict__ first,
    const int *__restrict__ last, const int *__restrict__ n_valid, const int *__restrict__ gmiss, int B, int N, int npix, int F,
    int ftiles, int pgroups, int norm, double oversample, double *__restrict__ power, double *__restrict__ tile_peak,
    int *__restrict__ tile_idx) {
    constexpr int SUBS = PP_T / (PP_W * PPL);                  // wavefronts per pixel group
    static_assert(SUBS >= 1 && SUBS * PP_W * PPL == PP_T, "a pixel group is a whole number of wavefronts");
    __shared__ double2 sh_tr[PP_CH][PP_FT];
    __shared__ uint8_t sh_valid[PP_CH];
    __shared__ double sh_part[PP_GJ][PP_FT][4];
    __shared__ double sh_tot[PP_FT][4];

    const unsigned bid = blockIdx.x, per = (unsigned)ftiles * (unsigned)pgroups * SUBS;
    const unsigned xcd = bid & 7u, slot = bid >> 3;
    const int b = (int)((slot / per) * 8u + xcd);
    if (b >= B) return;
    const unsigned rem = slot % per;
    const int tile = (int)(rem / ((unsigned)pgroups * SUBS)), pg = (int)((rem / SUBS) % (unsigned)pgroups), sub = (int)(rem % SUBS);
    if ((gmiss[(size_t)b * pgroups + pg] != 0) != MISS) return;

    const int tid = threadIdx.x, f0 = tile * PP_FT, nf = min(PP_FT, F - f0);
    int px[PPL];
    bool act[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        px[q] = pg * PP_T + (sub * PPL + q) * PP_W + tid;
        act[q] = px[q] < npix;
    }
    const int nv = n_valid[b];
    if (nv < 4) {                                              // status 2: nothing is read, every spectrum is NaN
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            if (!act[q]) continue;
            if (power)
                for (int k = 0; k < nf; ++k) power[((size_t)b * F + f0 + k) * npix + px[q]] = NAN;
            tile_peak[((size_t)b * ftiles + tile) * npix + px[q]] = NAN;
            tile_idx[((size_t)b * ftiles + tile) * npix + px[q]] = -1;
        }
        return;
    }

    const int gk = tid % PP_FT, gj = tid / PP_FT;
    const double fg = gk < nf ? freq[f0 + gk] : 0.0, tr = t_ref[b];
    const double *tm = time + (size_t)b * N;
    const float *fl = flux + (size_t)b * N * npix;
    double pv[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) pv[q] = act[q] ? pivot[(size_t)b * npix + px[q]] : 0.0;
    double gS = 0.0, gC = 0.0, gS2 = 0.0, gC2 = 0.0;
    double aS[PPL][PP_FT], aC[PPL][PP_FT];
    double mS[MISS ? PP_FT : 1], mC[MISS ? PP_FT : 1], mS2[MISS ? PP_FT : 1], mC2[MISS ? PP_FT : 1];
    static_assert(!MISS || PPL == 1, "the missed sums are kept for one pixel per lane");
#pragma unroll
    for (int q = 0; q < PPL; ++q)
#pragma unroll
        for (int k = 0; k < PP_FT; ++k) aS[q][k] = aC[q][k] = 0.0;
#pragma unroll
    for (int k = 0; k < (MISS ? PP_FT : 1); ++k) mS[k] = mC[k] = mS2[k] = mC2[k] = 0.0;

    for (int c0 = 0; c0 < N; c0 += PP_CH) {
        const int rows = min(PP_CH, N - c0);
        __syncthreads();                                       // the previous chunk has been consumed
#pragma unroll
        for (int m = 0; m < PP_CH / PP_GJ; ++m) {
            const int r = gj + PP_GJ * m;
            double s = 0.0, c = 0.0;
            bool ok = false;
            if (r < rows) {
                const double t = tm[c0 + r];
                ok = isfinite(t);
                if (ok) sincos2pi_prod(fg, t - tr, &s, &c);
            }
            sh_tr[r][gk] = make_double2(s, c);
            if (gk == 0) sh_valid[r] = ok ? 1 : 0;
            gS += s;
            gC += c;
            gS2 = fma(2.0 * s, c, gS2);
            gC2 += fma(c, c, -(s * s));
        }
        __syncthreads();
        for (int j0 = 0; j0 < PP_CH; j0 += PP_ROWS) {
            float v[PPL][PP_ROWS];
#pragma unroll
            for (int u = 0; u < PP_ROWS; ++u)
#pragma unroll
                for (int q = 0; q < PPL; ++q)
                    v[q][u] = act[q] && sh_valid[j0 + u] ? fl[(size_t)(c0 + j0 + u) * npix + px[q]] : 0.0f;
#pragma unroll
            for (int u = 0; u < PP_ROWS; ++u) {
                if (!sh_valid[j0 + u]) continue;
                const double2 *x = sh_tr[j0 + u];
                if constexpr (MISS) {
                    if (isnan(v[0][u])) {
#pragma unroll
                        for (int k = 0; k < PP_FT; ++k) {
                            const double2 sc = x[k];
                            mS[k] += sc.x;
                            mC[k] += sc.y;
                            mS2[k] = fma(2.0 * sc.x, sc.y, mS2[k]);
                            mC2[k] += fma(sc.y, sc.y, -(sc.x * sc.x));
                        }
                    }
                }
                double yd[PPL];
#pragma unroll
                for (int q = 0; q < PPL; ++q) yd[q] = isnan(v[q][u]) ? 0.0 : (double)v[q][u] - pv[q];
#pragma unroll
                for (int k = 0; k < PP_FT; ++k) {
                    const double2 sc = x[k];
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        aS[q][k] = fma(yd[q], sc.x, aS[q][k]);
                        aC[q][k] = fma(yd[q], sc.y, aC[q][k]);
                    }
                }
            }
        }
    }
    // the shared sums of the tile: the generating lanes' partials in lane order
    sh_part[gj][gk][0] = gS;
    sh_part[gj][gk][1] = gC;
    sh_part[gj][gk][2] = gS2;
    sh_part[gj][gk][3] = gC2;
    __syncthreads();
    if (tid < 4 * PP_FT) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < PP_GJ; ++j) s += sh_part[j][tid >> 2][tid & 3];
        sh_tot[tid >> 2][tid & 3] = s;
    }
    __syncthreads();

#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (!act[q]) continue;
        const int p = px[q];
        const size_t o = (size_t)b * npix + p;
        const int n = n_used[o];
        const bool ok = n >= 4;
        const double dn = (double)n, inv = 1.0 / dn, d = sy[o] * inv;
        double scale = 1.0;
        if (norm == LK_NORM_LK_PSD) {                          // lightkurve's 2 / (n oversample fs), fs from the pixel's own span [uHz]
            const double fs = (1.0 / (tm[last[o]] - tm[first[o]])) / oversample * (1e6 / 86400.0);
            scale = 2.0 / (dn * oversample * fs);
        }
        double best = NAN;
        int bi = -1;
#pragma unroll
        for (int k = 0; k < PP_FT; ++k) {
            if (k >= nf) continue;
            double S = sh_tot[k][0], C = sh_tot[k][1], S2 = sh_tot[k][2], C2 = sh_tot[k][3];
            if constexpr (MISS) {
                S -= mS[k];
                C -= mC[k];
                S2 -= mS2[k];
                C2 -= mC2[k];
            }
            const double Sh = (aS[q][k] - d * S) * inv, Ch = (aC[q][k] - d * C) * inv;
            const double pw = ok ? gls_power_sums(Sh, Ch, S * inv, C * inv, S2 * inv, C2 * inv, 1, norm, 1.0, 0.5 * dn, dn, scale) : NAN;
            if (power) power[((size_t)b * F + f0 + k) * npix + p] = pw;
            if (pw == pw && (bi < 0 || pw > best)) {
                best = pw;
                bi = f0 + k;
            }
        }
        tile_peak[((size_t)b * ftiles + tile) * npix + p] = best;
        tile_idx[((size_t)b * ftiles + tile) * npix + p] = bi;
    }
}

// One thread per pixel: the first index of the largest non-NaN power over the tiles in tile order (NaN / -1 without one)
__global__ __launch_bounds__(PP_T) void cube_pixelpg_peaks_kernel(const double *__restrict__ tile_peak,
                                                                  const int *__restrict__ tile_idx, int npix, int ftiles,
                                                                  double *__restrict__ peak_power, int *__restrict__ peak_index) {
    const int b = blockIdx.y, p = blockIdx.x * PP_T + threadIdx.x;
    if (p >= npix) return;
    double best = NAN;
    int bi = -1;
    for (int t = 0; t < ftiles; ++t) {
        const size_t s = ((size_t)b * ftiles + t) * npix + p;
        const int i = tile_idx[s];
        const double v = tile_peak[s];
        if (i >= 0 && (bi < 0 || v > best)) {
            best = v;
            bi = i;
        }
    }
    peak_power[(size_t)b * npix + p] = best;
    peak_index[(size_t)b * npix + p] = bi;
}

int cube_pixelpg_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency_host,
                        int F, int normalization, double oversample_factor, const double *t_ref_host, double *power,
                        double *peak_power, int32_t *peak_index, int32_t *n_used, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1 && F >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1, F >= 1");
    LK_REQUIRE(time && flux && frequency_host && t_ref_host, "NULL input");
    LK_REQUIRE(peak_power && peak_index && n_used && status, "NULL output buffer");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    LK_REQUIRE((int64_t)F * npix < (int64_t)1 << 31, "a power cube of %d x %d values per cutout is too large", F, npix);
    LK_REQUIRE(normalization == LK_NORM_LK_AMPLITUDE || normalization == LK_NORM_LK_PSD,
               "normalization must be LK_NORM_LK_AMPLITUDE or LK_NORM_LK_PSD (got %d)", normalization);
    LK_REQUIRE(oversample_factor > 0.0 && std::isfinite(oversample_factor), "oversample_factor must be finite and > 0");
    for (int k = 0; k < F; ++k)
        LK_REQUIRE(frequency_host[k] > 0.0 && std::isfinite(frequency_host[k]), "frequency %d is not finite and > 0", k);
    const int ftiles = (F + PP_FT - 1) / PP_FT, pgroups = (npix + PP_T - 1) / PP_T;
    const size_t nblocks = (size_t)((B + 7) / 8) * 8 * (size_t)ftiles * (size_t)pgroups;   // x 2 for the groups that miss cadences
    LK_REQUIRE(2 * nblocks < ((size_t)1 << 31), "grid too large (B=%d, F=%d, npix=%d)", B, F, npix);
    const size_t px = (size_t)B * npix;
    double *d_freq, *d_tref, *d_pivot, *d_sy, *d_tile_peak;
    int *d_first, *d_last, *d_nvalid, *d_gmiss, *d_tile_idx;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_freq, frequency_host, (size_t)F)
                           .upload(d_tref, t_ref_host, (size_t)B)
                           .buf(d_pivot, px)
                           .buf(d_sy, px)
                           .buf(d_tile_peak, px * ftiles)
                           .buf(d_first, px)
                           .buf(d_last, px)
                           .buf(d_tile_idx, px * ftiles)
                           .buf(d_nvalid, (size_t)B)
                           .buf(d_gmiss, (size_t)B * pgroups)
                           .carve(stream))
        return rc;
    const dim3 by_pixel(pgroups, B);
    hipLaunchKernelGGL(cube_pixelpg_stats_kernel, by_pixel, dim3(PP_T), 0, stream, time, flux, N, npix, d_pivot, d_sy, (int *)n_used,
                       d_first, d_last, d_nvalid, (int *)status, d_gmiss);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((cube_pixelpg_spectra_kernel<false, 2>), dim3((unsigned)nblocks), dim3(PP_W), 0, stream, time, flux,
                       (const double *)d_freq, (const double *)d_tref, (const double *)d_pivot, (const double *)d_sy,
                       (const int *)n_used, (const int *)d_first, (const int *)d_last, (const int *)d_nvalid, (const int *)d_gmiss, B, N,
                       npix, F, ftiles, pgroups, normalization, oversample_factor, power, d_tile_peak, d_tile_idx);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((cube_pixelpg_spectra_kernel<true, 1>), dim3((unsigned)(2 * nblocks)), dim3(PP_W), 0, stream, time, flux,
                       (const double *)d_freq, (const double *)d_tref, (const double *)d_pivot, (const double *)d_sy,
                       (const int *)n_used, (const int *)d_first, (const int *)d_last, (const int *)d_nvalid, (const int *)d_gmiss, B, N,
                       npix, F, ftiles, pgroups, normalization, oversample_factor, power, d_tile_peak, d_tile_idx);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cube_pixelpg_peaks_kernel, by_pixel, dim3(PP_T), 0, stream, (const double *)d_tile_peak,
                       (const int *)d_tile_idx, npix, ftiles, peak_power, (int *)peak_index);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
