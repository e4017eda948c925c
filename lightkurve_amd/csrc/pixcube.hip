// pixcube.hip — what PLDCorrector does to a target-pixel cutout BEFORE the design matrix, for B same-shaped float32 cubes
// [B][N][npix] resident in HBM (lightkurve_amd/cubes.py: DevicePixelCubeBatch):
//   cube_aperture   simple aperture photometry (TargetPixelFile.to_lightcurve, flux_method='sum',
//                   src/lightkurve/targetpixelfile.py:868-923) + the NaN-cadence flags of PLDCorrector.__init__
//                   (correctors/pldcorrector.py:109-120);
//   cube_centroids  the moment centroids of TargetPixelFile.estimate_centroids (what SFFCorrector's arclength is made from);
//   cube_centroids_quadratic   the same method's 'quadratic' estimator (lightkurve.utils.centroid_quadratic) per cadence;
//   cube_diffimage  the transit difference image of every cutout (mean out-of-transit minus mean in-transit image, with its
//                   error image) and image_centroids, both estimators on such float64 images;
//   cube_median     the per-pixel nanmedian image behind create_threshold_mask (targetpixelfile.py:680-742);
//   cube_compact / cube_gather   the compaction tpf[~nan_mask], the pixel series of the PLD / background apertures
//                   (pldcorrector.py:203-227) and the spline's percentile knots;
//   pld_corrected   corrected = (y - model) + (spline - median(spline))   (pldcorrector.py:418-420).
// This file is compiled with -ffp-contract=off: the float32 aperture sums must round every product and every sum on its
// own, in pixel order, to equal numpy's (see cube_aperture_kernel), and the knot lerp numpy's _lerp.
#include "lk_common.hpp"

#include <algorithm>

#include "block_select.hpp"
#include "stage_tile.hpp"  // stage_contiguous, shared with psfphot.hip
#include "fold_phase.hpp"  // np_mod: the difference image classes its cadences by create_transit_mask's phase

namespace lk {

constexpr int AP_T = 64;       // cadences per workgroup: one lane of wave 0 (flux) and of wave 1 (flux_err) each
constexpr int AP_WMAX = 127;   // pixel columns per LDS chunk: 2 tiles x 64 rows x 127 dwords + the mask < 64 KB
constexpr int MED_G = 16;      // adjacent pixels per workgroup of the median image: one 64-byte segment of every cadence row

// columns [p0, p0 + w) of rows x npix floats -> tile[row * pitch + column - p0] (cutouts wider than one chunk)
__device__ __forceinline__ void stage_columns(const float *__restrict__ g, float *__restrict__ tile, int rows, int npix, int p0,
                                              int w, int pitch) {
    for (int i = threadIdx.x; i < rows * w; i += blockDim.x) {
        const int r = i / w, c = i - r * w;
        tile[r * pitch + c] = g[(size_t)r * npix + p0 + c];
    }
}

// Aperture sums of AP_T consecutive cadences of one cutout.  numpy adds the aperture's pixels of a cadence ONE AFTER THE
// OTHER in row-major pixel order, in float32 (PixelCube._aperture_sums: `cube[:, ap]` is laid out pixel-major, so the
// reduction over the pixels walks whole cadence vectors); flux_err = sqrt_f32(sum_f32(e * e rounded to float32)).  NaN
// pixels (and NaN e * e) count as 0; the flux is NaN when no aperture pixel is finite, or when EVERY pixel of the cadence
// image is 0.  So: no tree over the pixels — a lane owns a cadence and walks its row.  Walking rows in global memory would
// put 4 * npix bytes between the lanes of a load; instead the tile (contiguous in memory: cadences x pixels) is staged
// through LDS with coalesced 16-byte loads and every lane walks its own LDS row.  ds_read_b32 conflicts are per 32-lane
// half on bank (address / 4) mod 32: the row pitch is odd, so the 32 rows of a half sit on 32 different banks.
// Wave 0 sums the flux tile and wave 1 the flux_err tile; waves 2-3 only help staging.  keep = !(isnan(flux) |
// isnan(flux_err)); counts[b] += kept cadences, counts[B + b] += kept cadences with a non-finite pixel anywhere in the image.
__global__ __launch_bounds__(256) void cube_aperture_kernel(const float *__restrict__ flux, const float *__restrict__ ferr,
                                                            const uint8_t *__restrict__ mask, int mask_stride, int B, int N,
                                                            int npix, int W, int pitch, float *__restrict__ flux_out,
                                                            float *__restrict__ err_out, uint8_t *__restrict__ keep_out,
                                                            unsigned long long *__restrict__ counts) {
    extern __shared__ __align__(16) float ap_tile[];
    __shared__ float s_err[AP_T];
    float *tf = ap_tile, *te = ap_tile + AP_T * pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(ap_tile + 2 * AP_T * pitch);
    const int b = blockIdx.y, c0 = blockIdx.x * AP_T, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int rows = min(AP_T, N - c0);
    const float *gf = flux + ((size_t)b * N + c0) * npix, *ge = ferr + ((size_t)b * N + c0) * npix;
    const uint8_t *m = mask + (size_t)b * mask_stride;
    float acc = 0.0f;
    bool allzero = true, anyfinite = false, bad = false;
    for (int p0 = 0; p0 < npix; p0 += W) {
        const int w = min(W, npix - p0);
        if (p0) __syncthreads();  // the previous chunk has been walked
        if (w == npix) {
            stage_contiguous(gf, tf, rows * npix, npix, pitch);
            stage_contiguous(ge, te, rows * npix, npix, pitch);
        } else {
            stage_columns(gf, tf, rows, npix, p0, w, pitch);
            stage_columns(ge, te, rows, npix, p0, w, pitch);
        }
        for (int i = tid; i < w; i += 256) sm[i] = m[p0 + i];
        __syncthreads();
        if (wave == 0 && lane < rows) {
            const float *row = tf + lane * pitch;
            for (int p = 0; p < w; ++p) {
                const float v = row[p];
                allzero = allzero && v == 0.0f;
                bad = bad || !isfinite(v);
                if (sm[p]) {
                    if (!isnan(v)) acc = acc + v;
                    anyfinite = anyfinite || isfinite(v);
                }
            }
        } else if (wave == 1 && lane < rows) {
            const float *row = te + lane * pitch;
            for (int p = 0; p < w; ++p)
                if (sm[p]) {
                    const float e2 = row[p] * row[p];
                    if (!isnan(e2)) acc = acc + e2;
                }
        }
    }
    if (wave == 1 && lane < rows) s_err[lane] = __fsqrt_rn(acc);
    __syncthreads();
    if (wave == 0) {
        bool keep = false;
        if (lane < rows) {
            const float f = (anyfinite && !allzero) ? acc : __int_as_float(0x7fc00000);
            const float e = s_err[lane];
            keep = !(isnan(f) || isnan(e));
            const size_t o = (size_t)b * N + c0 + lane;
            flux_out[o] = f;
            err_out[o] = e;
            keep_out[o] = keep ? 1 : 0;
        }
        const unsigned long long kept = __ballot(keep), dirty = __ballot(keep && bad);
        if (lane == 0) {
            if (kept) atomicAdd(&counts[b], (unsigned long long)__popcll(kept));
            if (dirty) atomicAdd(&counts[B + b], (unsigned long long)__popcll(dirty));
        }
    }
}

// TargetPixelFile.estimate_centroids(aperture_mask, method='moments') (src/lightkurve/targetpixelfile.py): per cadence the flux-
// weighted mean pixel position inside the aperture, col = sum_p (column0 + x_p) m_p flux_p / sum_p m_p flux_p and likewise
// for row, summed in float64 with NaN pixels counting as 0 (nansum); a total that is zero or NaN gives NaN.  One wavefront
// per cadence: lane l adds the pixels l, l + 64, ... in that order and the 64 lane sums are added in a butterfly, so the
// order of every sum depends on npix alone.  Pixel p sits at x_p = p % nx, y_p = p / nx.  T: float (a cadence of a cube) or
// double (a difference image); every lane of the wavefront returns the result.
template <class T>
__device__ __forceinline__ void wave_centroid_moments(const T *__restrict__ img, const uint8_t *__restrict__ m, int npix, int nx,
                                                      double column0, double row0, int lane, double &col, double &row) {
    double tot = 0.0, sx = 0.0, sy = 0.0;
    for (int p = lane; p < npix; p += 64) {
        const T v = img[p];
        if (m[p] && !isnan(v)) {
            const int y = p / nx, x = p - y * nx;
            const double d = (double)v;
            tot = tot + d;
            sx = sx + (column0 + (double)x) * d;
            sy = sy + (row0 + (double)y) * d;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        tot = tot + __shfl_xor(tot, o);
        sx = sx + __shfl_xor(sx, o);
        sy = sy + __shfl_xor(sy, o);
    }
    const bool ok = tot == tot && tot != 0.0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    col = ok ? sx / tot : nan;
    row = ok ? sy / tot : nan;
}

__global__ __launch_bounds__(256) void cube_centroids_kernel(const float *__restrict__ flux, const uint8_t *__restrict__ mask,
                                                             int mask_stride, int N, int npix, int nx, double column0,
                                                             double row0, double *__restrict__ col_out,
                                                             double *__restrict__ row_out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    double col, row;
    wave_centroid_moments(flux + ((size_t)b * N + i) * npix, mask + (size_t)b * mask_stride, npix, nx, column0, row0, lane, col,
                          row);
    if (lane == 0) {
        col_out[(size_t)b * N + i] = col;
        row_out[(size_t)b * N + i] = row;
    }
}

// lightkurve.utils.centroid_quadratic(data, mask) (TargetPixelFile.estimate_centroids(method='quadratic')) of one (ny, nx) image
// by one wavefront.  z = data * mask (a masked-out finite pixel is 0, a masked-out NaN / inf pixel NaN); k = nanargmax(z), the
// FIRST flat index of the largest value that is not NaN: lane l scans the pixels l, l + 64, ... and keeps (value, first index),
// and the 64 pairs meet in a butterfly whose order is (larger value, then smaller index), so k does not depend on how the pixels
// fell on the lanes.  (yy, xx) = divmod(k, nx) clamped into [1, ny - 2] x [1, nx - 2]; nine lanes fetch the 3 x 3 patch of z
// around it (row-major, x fastest) and every lane fits P = a + b x + c y + d x^2 + e x y + f y^2 through (A^T A)^-1 A^T, which
// for x, y in {0, 1, 2} is exactly the integer table below over 36; det = 4 d f - e^2, |det| < 1e-6 -> NaN, else the extremum
// xm = -(2 f b - c e) / det, ym = -(2 d c - b e) / det and col = column0 + xx - 1 + xm, row = row0 + yy - 1 + ym (the pixel-index
// convention of the moments: a symmetric source centred on pixel (i, j) gives (i, j)).  A NaN in the patch gives NaN through
// the arithmetic; no pixel that is not NaN gives NaN and peak = -1.  peak = k, before the clamp.  All float64, no contraction.
template <class T>
__device__ __forceinline__ void wave_centroid_quadratic(const T *__restrict__ img, const uint8_t *__restrict__ m, int npix, int nx,
                                                        double column0, double row0, int lane, double &col, double &row,
                                                        int &peak) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double best = 0.0;
    int bi = -1;
    for (int p = lane; p < npix; p += 64) {
        const double z = (double)img[p] * (m[p] ? 1.0 : 0.0);
        if (z == z && (bi < 0 || z > best)) {
            best = z;
            bi = p;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) {
            best = ob;
            bi = oi;
        }
    }
    peak = bi;
    col = row = nan;
    if (bi < 0) return;  // (the whole wavefront)
    const int ny = npix / nx;
    const int yy = min(max(bi / nx, 1), ny - 2), xx = min(max(bi % nx, 1), nx - 2);
    double zl = 0.0;
    if (lane < 9) {
        const int q = (yy - 1 + lane / 3) * nx + xx - 1 + lane % 3;
        zl = (double)img[q] * (m[q] ? 1.0 : 0.0);
    }
    const double w[6][9] = {{29, 8, -1, 8, -4, -4, -1, -4, 5},      {-27, 24, 3, -18, 24, -6, -9, 24, -15},
                            {-27, -18, -9, 24, 24, 24, 3, -6, -15}, {6, -12, 6, 6, -12, 6, 6, -12, 6},
                            {9, 0, -9, 0, 0, 0, -9, 0, 9},          {6, 6, 6, -12, -12, -12, 6, 6, 6}};
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double z = __shfl(zl, j);
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = c[k] + w[k][j] * z;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = c[k] / 36.0;
    const double b1 = c[1], c1 = c[2], d = c[3], e = c[4], f = c[5];
    const double det = 4.0 * d * f - e * e;
    if (fabs(det) < 1e-6) return;
    const double xm = -(2.0 * f * b1 - c1 * e) / det, ym = -(2.0 * d * c1 - b1 * e) / det;
    col = ((column0 + (double)xx) - 1.0) + xm;
    row = ((row0 + (double)yy) - 1.0) + ym;
}

// One wavefront per cadence, the mapping of cube_centroids_kernel: the cube is read once, coalesced; peak_out is nullable.
__global__ __launch_bounds__(256) void cube_centroids_quadratic_kernel(const float *__restrict__ flux,
                                                                       const uint8_t *__restrict__ mask, int mask_stride, int N,
                                                                       int npix, int nx, double column0, double row0,
                                                                       double *__restrict__ col_out, double *__restrict__ row_out,
                                                                       int *__restrict__ peak_out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    double col, row;
    int peak;
    wave_centroid_quadratic(flux + ((size_t)b * N + i) * npix, mask + (size_t)b * mask_stride, npix, nx, column0, row0, lane, col,
                            row, peak);
    if (lane == 0) {
        col_out[(size_t)b * N + i] = col;
        row_out[(size_t)b * N + i] = row;
        if (peak_out) peak_out[(size_t)b * N + i] = peak;
    }
}

// Either estimator on B float64 images [B][npix] (the difference images below), one wavefront per image
__global__ __launch_bounds__(256) void image_centroids_kernel(const double *__restrict__ image, const uint8_t *__restrict__ mask,
                                                              int mask_stride, int B, int npix, int nx, double column0,
                                                              double row0, int quadratic, double *__restrict__ col_out,
                                                              double *__restrict__ row_out, int *__restrict__ peak_out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const double *img = image + (size_t)b * npix;
    const uint8_t *m = mask + (size_t)b * mask_stride;
    double col, row;
    int peak = -1;
    if (quadratic) wave_centroid_quadratic(img, m, npix, nx, column0, row0, lane, col, row, peak);
    else wave_centroid_moments(img, m, npix, nx, column0, row0, lane, col, row);
    if (lane == 0) {
        col_out[b] = col;
        row_out[b] = row;
        if (peak_out) peak_out[b] = peak;
    }
}

// ------------------------------------------------------------------------------------------------ difference images
// Per cutout b one box (P, t0, D); par = [P[B] | t0[B] | D[B]].  Cadence i with time t has the phase
// x = np_mod(t - t0 + P/2, P) - P/2 (create_transit_mask's expression) and the class
//   1 (in)   |x| < in_width D,      2 (out)  out_inner D <= |x| < out_outer D,      0 (none) otherwise and for a NaN time.
// n_in[b] / n_out[b] (zeroed by the launcher) count the cadences of the two classes: integer atomics, one per wavefront.
constexpr int DI_CHUNK = 128;  // cadences per workgroup of the accumulation: the order of every sum depends on N alone
constexpr int DI_T = 128;      // its lanes: adjacent pixels of one cadence row per load

__global__ __launch_bounds__(256) void cube_diffimage_class_kernel(const double *__restrict__ time, const double *__restrict__ par,
                                                                   int B, int N, double in_width, double out_inner,
                                                                   double out_outer, uint8_t *__restrict__ cls,
                                                                   int *__restrict__ n_in, int *__restrict__ n_out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    if (i < N) {
        const double P = par[b], t0 = par[B + b], D = par[2 * B + b], hp = P / 2.0;
        const double x = fabs(np_mod(time[(size_t)b * N + i] - t0 + hp, P) - hp);
        c = x < in_width * D ? 1 : (x >= out_inner * D && x < out_outer * D ? 2 : 0);
        cls[(size_t)b * N + i] = (uint8_t)c;
    }
    const unsigned long long bal_in = __ballot(c == 1), bal_out = __ballot(c == 2);
    if ((threadIdx.x & 63) == 0) {
        if (bal_in) atomicAdd(&n_in[b], __popcll(bal_in));
        if (bal_out) atomicAdd(&n_out[b], __popcll(bal_out));
    }
}

// Workgroup (chunk, b): the cadences [chunk DI_CHUNK, +DI_CHUNK) of cutout b, lane = pixel (cutouts of more than DI_T pixels
// take them in groups).  A lane walks its pixel down the chunk's cadences in order and keeps, for the in and the out class,
// the float64 sum of the float32 flux values that are not NaN, the sum of flux_err^2 over the same cadences and their number:
// psum[b][chunk][s_in | s_out | e_in | e_out][npix], pcnt[b][chunk][n_in | n_out][npix].  The class is uniform over the
// workgroup, so the rows of a cadence without a class are not loaded at all; every other row of both cubes is loaded once, as
// runs of adjacent floats.  No atomics: cube_diffimage_finish_kernel adds the chunks in index order.
__global__ __launch_bounds__(DI_T) void cube_diffimage_accum_kernel(const float *__restrict__ flux, const float *__restrict__ ferr,
                                                                    const uint8_t *__restrict__ cls, int N, int npix, int chunks,
                                                                    double *__restrict__ psum, int *__restrict__ pcnt) {
    const int b = blockIdx.y, ch = blockIdx.x, c0 = ch * DI_CHUNK, rows = min(DI_CHUNK, N - c0);
    const uint8_t *cl = cls + (size_t)b * N + c0;
    const size_t base = ((size_t)b * N + c0) * npix;
    double *ps = psum + ((size_t)b * chunks + ch) * 4 * npix;
    int *pc = pcnt + ((size_t)b * chunks + ch) * 2 * npix;
    for (int p = threadIdx.x; p < npix; p += DI_T) {
        double s_in = 0.0, s_out = 0.0, e_in = 0.0, e_out = 0.0;
        int k_in = 0, k_out = 0;
        for (int j = 0; j < rows; ++j) {
            const int c = cl[j];
            if (c == 0) continue;
            const float v = flux[base + (size_t)j * npix + p], e = ferr[base + (size_t)j * npix + p];
            if (isnan(v)) continue;
            const double d = (double)v, q = (double)e * (double)e;
            if (c == 1) {
                s_in = s_in + d;
                e_in = e_in + q;
                ++k_in;
            } else {
                s_out = s_out + d;
                e_out = e_out + q;
                ++k_out;
            }
        }
        ps[p] = s_in;
        ps[npix + p] = s_out;
        ps[2 * npix + p] = e_in;
        ps[3 * npix + p] = e_out;
        pc[p] = k_in;
        pc[npix + p] = k_out;
    }
}

// One thread per pixel: the chunks' partials added in index order, then mean_in = s_in / n_in, mean_out = s_out / n_out,
// diff = mean_out - mean_in (positive where the dimming is) and diff_err = sqrt(e_in / n_in^2 + e_out / n_out^2).  A pixel
// without a value in a class has 0 / 0 = NaN in every image that needs that class.
__global__ __launch_bounds__(256) void cube_diffimage_finish_kernel(const double *__restrict__ psum, const int *__restrict__ pcnt,
                                                                    int npix, int chunks, double *__restrict__ mean_in,
                                                                    double *__restrict__ mean_out, double *__restrict__ diff,
                                                                    double *__restrict__ diff_err) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    double s_in = 0.0, s_out = 0.0, e_in = 0.0, e_out = 0.0;
    long long k_in = 0, k_out = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const double *ps = psum + ((size_t)b * chunks + ch) * 4 * npix;
        const int *pc = pcnt + ((size_t)b * chunks + ch) * 2 * npix;
        s_in = s_in + ps[p];
        s_out = s_out + ps[npix + p];
        e_in = e_in + ps[2 * npix + p];
        e_out = e_out + ps[3 * npix + p];
        k_in += pc[p];
        k_out += pc[npix + p];
    }
    const double ni = (double)k_in, no = (double)k_out;
    const double mi = s_in / ni, mo = s_out / no;
    const size_t o = (size_t)b * npix + p;
    mean_in[o] = mi;
    mean_out[o] = mo;
    diff[o] = mo - mi;
    diff_err[o] = sqrt(e_in / (ni * ni) + e_out / (no * no));
}

// offset[b] = centroid_a - centroid_b as (col, row), offset_pix[b] its norm, and the status of cutout b.  The leading status is
// fit_status[b] where fit_status is given (amplitude images), else 1 for no in-transit cadence, 2 for no out-of-transit cadence
// (difference images); where that is 0: 3 for a centroid that is not defined (NaN), else 0.  The norm is numpy's
// sqrt(dx * dx + dy * dy), every product and the sum rounded on its own: this file is built with -ffp-contract=off, and in a
// file built with contraction the sum fuses and offset_pix moves in the last place
__global__ __launch_bounds__(256) void centroid_offsets_kernel(int B, const int *__restrict__ fit_status,
                                                               const int *__restrict__ n_in, const int *__restrict__ n_out,
                                                               const double *__restrict__ a_col, const double *__restrict__ a_row,
                                                               const double *__restrict__ b_col, const double *__restrict__ b_row,
                                                               double *__restrict__ offset, double *__restrict__ offset_pix,
                                                               int *__restrict__ status) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double dx = a_col[b] - b_col[b], dy = a_row[b] - b_row[b];
    const double r = sqrt(dx * dx + dy * dy);
    offset[2 * (size_t)b] = dx;
    offset[2 * (size_t)b + 1] = dy;
    offset_pix[b] = r;
    const int lead = fit_status ? fit_status[b] : n_in[b] == 0 ? 1 : n_out[b] == 0 ? 2 : 0;
    status[b] = lead != 0 ? lead : r != r ? 3 : 0;
}

// np.nanmedian(cube.astype(float64), axis=0) of the cadences with keep != 0 (all of them when keep is NULL): exact order
// statistics (block_select.hpp), the mean of the two middle values for an even count, NaN for a pixel that has no value.
// The column of one pixel is strided by npix floats, so a workgroup owns MED_G = 16 ADJACENT pixels of one cutout and
// selects them one after the other straight from global memory: the 16 columns share the same 64-byte segment of every
// cadence row, so only the first pixel's passes go to HBM and the other fifteen's hit the L2 (N x 64 B per workgroup).
// Chosen over an LDS-staged tile because this kernel only runs for data-dependent mask specs and a staged column set
// would cap N at what fits 160 KB; the select itself makes 9 passes over a column either way.
__global__ __launch_bounds__(256) void cube_median_image_kernel(const float *__restrict__ cube, const uint8_t *__restrict__ keep,
                                                                int N, int npix, double *__restrict__ med) {
    __shared__ unsigned long long sh[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint8_t *kp = keep ? keep + (size_t)b * N : nullptr;
    const int p1 = min(npix, (int)(blockIdx.x + 1) * MED_G);
    for (int p = blockIdx.x * MED_G; p < p1; ++p) {
        const float *col = cube + (size_t)b * N * npix + p;
        auto val = [&](int i) { return (double)col[(size_t)i * npix]; };
        auto kf = [&](int i) { return (!kp || kp[i]) && !isnan(col[(size_t)i * npix]); };
        long long cnt = 0;
        for (int i = tid; i < N; i += 256) cnt += kf(i) ? 1 : 0;
        cnt = block_count_dyn(cnt, reinterpret_cast<long long *>(sh));
        const double r = block_median(N, cnt, val, kf, sh);
        if (tid == 0) med[(size_t)b * npix + p] = r;
    }
}

// ------------------------------------------------------------------------------------------------ background
// TargetPixelFile.estimate_background per cadence: bkg[b][i] = np.nanmedian(cube[b][i][mask_b]) in float32 (the mirror is
// PixelCube.estimate_background), n_pixels = the selected pixels that are not NaN, scatter = nanmedian(|sel - bkg|) in
// float32, and cube_out = cube - bkg over ALL pixels of the cadence.  NaN is the only excluded value, +-inf are values; an
// even count gives (a + b) * 0.5f of the two middle values, rounded once in float32 (this file has no contraction); no value
// gives NaN.  Selection is exact, so every output has the same bits wherever the cutout sits in a batch.
//
// float32 -> a key whose unsigned order is the order of the values (-0.0 below +0.0); every NaN becomes the largest key,
// which no other value has, so the NaNs of a row sort behind its n values.
constexpr int BG_T = 64;                 // cadences per workgroup of the small route (16 per wavefront)
constexpr int BG_SMALL_MAX_NPIX = 224;   // the route cut: 64 rows x 225 dwords + the key lists stay below 64 KB of LDS
constexpr unsigned BG_NAN_KEY = 0xffffffffu;

__device__ __forceinline__ unsigned f32_sortable(float x) {
    if (isnan(x)) return BG_NAN_KEY;
    const unsigned u = (unsigned)__float_as_int(x);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_sortable(unsigned u) {
    u = (u >> 31) ? (u & 0x7fffffffu) : ~u;
    return __int_as_float((int)u);  // (BG_NAN_KEY -> 0x7fffffff, a NaN)
}

// LDS written by some lanes of a wavefront and read by others of the same one
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Median of the n keys of keys[0 .. S) that are not BG_NAN_KEY, by one wavefront: every entry is ranked by counting the
// entries below it, (key, index) in lexicographic order, so the ranks are a permutation of 0 .. S - 1 whatever the ties and
// the entries of rank (n - 1) / 2 and n / 2 are the middle ones.  Lane l ranks the entries l, l + 64, ...; the list is read
// four keys per ds_read_b128 (every lane the same address: a broadcast) and is padded with BG_NAN_KEY up to a multiple of
// four — a padding entry sits behind every real one in that order and adds to no rank.  S^2 / 64 comparisons per lane.
__device__ __forceinline__ float wave_median_keys(const unsigned *__restrict__ keys, int S, int n, int lane) {
    if (n <= 0) return __int_as_float(0x7fc00000);  // (n is the same in every lane)
    const int k1 = (n - 1) >> 1, k2 = n >> 1, S4 = (S + 3) >> 2;
    const uint4 *kv = reinterpret_cast<const uint4 *>(keys);
    float a = 0.0f, b = 0.0f;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < S;
        const unsigned k = valid ? keys[j] : BG_NAN_KEY;
        int rank = 0;
        for (int q = 0; q < S4; ++q) {
            const uint4 w = kv[q];
            const int i = 4 * q;
            rank += (w.x < k || (w.x == k && i < j)) ? 1 : 0;
            rank += (w.y < k || (w.y == k && i + 1 < j)) ? 1 : 0;
            rank += (w.z < k || (w.z == k && i + 2 < j)) ? 1 : 0;
            rank += (w.w < k || (w.w == k && i + 3 < j)) ? 1 : 0;
        }
        const float v = f32_from_sortable(k);
        const unsigned long long ha = __ballot(valid && rank == k1), hb = __ballot(valid && rank == k2);
        if (ha) a = __shfl(v, __ffsll((long long)ha) - 1);
        if (hb) b = __shfl(v, __ffsll((long long)hb) - 1);
    }
    return k1 == k2 ? a : (a + b) * 0.5f;
}

// tile[row * pitch + column] - sub[row] -> rows x npix floats that are CONTIGUOUS in global memory: stage_contiguous backwards
__device__ __forceinline__ void unstage_contiguous_minus(const float *__restrict__ tile, const float *__restrict__ sub,
                                                         float *__restrict__ g, int total, int npix, int pitch) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
    const int head = min(total, (4 - mis) & 3);
    if (tid < head) g[tid] = tile[(tid / npix) * pitch + tid % npix] - sub[tid / npix];
    const int nvec = (total - head) >> 2;
    float4 *gv = reinterpret_cast<float4 *>(g + head);
#pragma unroll 4
    for (int v = tid; v < nvec; v += nt) {
        const int i = head + 4 * v;
        int r = i / npix, c = i - r * npix;
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = tile[r * pitch + c] - sub[r];
            if (++c == npix) {
                c = 0;
                ++r;
            }
        }
        gv[v] = make_float4(e[0], e[1], e[2], e[3]);
    }
    const int i = head + 4 * nvec + tid;
    if (i < total) g[i] = tile[(i / npix) * pitch + i % npix] - sub[i / npix];
}

// Small route (npix <= BG_SMALL_MAX_NPIX): a workgroup stages BG_T consecutive cadences of one cutout (contiguous in memory)
// in LDS with 16-byte loads, lists the selected pixel numbers of the cutout's mask in ascending order once, and every
// wavefront takes the cadences wave, wave + 4, ... of the tile: the keys of its selected pixels go to the wavefront's own
// list, wave_median_keys finds the median, the keys of |v - bkg| replace them for the scatter.  The subtracted tile leaves
// with 16-byte stores.  The cube is read once and written once.
__global__ __launch_bounds__(256) void cube_background_kernel(const float *__restrict__ cube, const uint8_t *__restrict__ mask,
                                                              int mask_stride, int N, int npix, int pitch, int want_scatter,
                                                              float *__restrict__ bkg_out, int *__restrict__ npix_out,
                                                              float *__restrict__ scatter_out, float *__restrict__ cube_out) {
    extern __shared__ __align__(16) float bg_tile[];
    __shared__ __align__(16) unsigned s_keys[4][BG_SMALL_MAX_NPIX];
    __shared__ int s_sel[BG_SMALL_MAX_NPIX];
    __shared__ float s_bkg[BG_T];
    __shared__ int s_wcnt[4];
    const int b = blockIdx.y, c0 = blockIdx.x * BG_T, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int rows = min(BG_T, N - c0);
    const size_t off = ((size_t)b * N + c0) * npix;
    stage_contiguous(cube + off, bg_tile, rows * npix, npix, pitch);
    // the selected pixels in ascending order (npix <= 256 threads: one ballot per wavefront, offsets from the four counts)
    const bool on = tid < npix && mask[(size_t)b * mask_stride + tid] != 0;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, S = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += s_wcnt[w];
        S += s_wcnt[w];
    }
    if (on) s_sel[before + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    unsigned *keys = s_keys[wave];
    const int S4 = (S + 3) & ~3;
    for (int r = wave; r < rows; r += 4) {
        const float *row = bg_tile + r * pitch;
        int n = 0;
        for (int j = lane; j < S4; j += 64) {
            const unsigned k = j < S ? f32_sortable(row[s_sel[j]]) : BG_NAN_KEY;
            keys[j] = k;
            n += k != BG_NAN_KEY ? 1 : 0;
        }
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        wave_lds_sync();
        const float med = wave_median_keys(keys, S, n, lane);
        float sc = 0.0f;
        if (want_scatter) {
            wave_lds_sync();  // every lane has read the keys
            int n2 = 0;
            for (int j = lane; j < S; j += 64) {
                const unsigned k = f32_sortable(fabsf(f32_from_sortable(keys[j]) - med));
                keys[j] = k;
                n2 += k != BG_NAN_KEY ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o);
            wave_lds_sync();
            sc = wave_median_keys(keys, S, n2, lane);
        }
        wave_lds_sync();  // ... before the next cadence's keys overwrite them
        if (lane == 0) {
            const size_t o = (size_t)b * N + c0 + r;
            bkg_out[o] = med;
            npix_out[o] = n;
            if (want_scatter) scatter_out[o] = sc;
            s_bkg[r] = med;
        }
    }
    if (!cube_out) return;  // (the whole workgroup)
    __syncthreads();
    unstage_contiguous_minus(bg_tile, s_bkg, cube_out + off, rows * npix, npix, pitch);
}

// Large route: one workgroup per cadence over global memory (the row stays in the caches between the passes), the radix
// select of block_select.hpp on the values widened to float64 — exact and order-preserving; the two middle values come back
// as they are and meet in float32.
__global__ __launch_bounds__(256) void cube_background_wide_kernel(const float *__restrict__ cube, const uint8_t *__restrict__ mask,
                                                                   int mask_stride, int N, int npix, int want_scatter,
                                                                   float *__restrict__ bkg_out, int *__restrict__ npix_out,
                                                                   float *__restrict__ scatter_out, float *__restrict__ cube_out) {
    __shared__ unsigned long long sh[264];
    const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const size_t off = ((size_t)b * N + i) * npix;
    const float *row = cube + off;
    const uint8_t *m = mask + (size_t)b * mask_stride;
    const float nan = __int_as_float(0x7fc00000);
    auto median = [&](auto val, auto keep, long long &cnt) -> float {
        long long c = 0;
        for (int p = tid; p < npix; p += 256) c += keep(p) ? 1 : 0;
        cnt = block_count_dyn(c, reinterpret_cast<long long *>(sh));
        if (cnt <= 0) return nan;  // (the whole workgroup)
        const float a = (float)block_select_kth(npix, (cnt - 1) / 2, val, keep, sh);
        if (cnt & 1) return a;
        const float hi = (float)block_select_kth(npix, cnt / 2, val, keep, sh);
        return (a + hi) * 0.5f;
    };
    long long n = 0, n2 = 0;
    const float med = median([&](int p) { return (double)row[p]; }, [&](int p) { return m[p] != 0 && !isnan(row[p]); }, n);
    float sc = 0.0f;
    if (want_scatter)
        sc = median([&](int p) { return (double)fabsf(row[p] - med); },
                    [&](int p) { return m[p] != 0 && !isnan(row[p] - med); }, n2);
    if (tid == 0) {
        const size_t o = (size_t)b * N + i;
        bkg_out[o] = med;
        npix_out[o] = (int)n;
        if (want_scatter) scatter_out[o] = sc;
    }
    if (cube_out)
        for (int p = tid; p < npix; p += 256) cube_out[off + p] = row[p] - med;
}

// cube_out = cube - rows[b][i] for rows given by the caller.  A workgroup walks a share of one cutout (N * npix < 2^31
// values): 16-byte loads and stores where source and destination are misaligned alike, else value by value.
__global__ __launch_bounds__(256) void cube_subtract_rows_kernel(const float *__restrict__ cube, const float *__restrict__ rows,
                                                                 int N, int npix, float *__restrict__ cube_out) {
    const int b = blockIdx.y, total = N * npix;
    const int t = blockIdx.x * 256 + threadIdx.x, nt = gridDim.x * 256;
    const float *g = cube + (size_t)b * total;
    const float *sub = rows + (size_t)b * N;
    float *o = cube_out + (size_t)b * total;
    if (((reinterpret_cast<uintptr_t>(g) ^ reinterpret_cast<uintptr_t>(o)) & 15) != 0) {
        for (long long i = t; i < total; i += nt) o[i] = g[i] - sub[(int)i / npix];
        return;
    }
    const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
    const int head = min(total, (4 - mis) & 3);
    if (t < head) o[t] = g[t] - sub[t / npix];
    const int nvec = (total - head) >> 2;
    const float4 *gv = reinterpret_cast<const float4 *>(g + head);
    float4 *ov = reinterpret_cast<float4 *>(o + head);
    for (int v = t; v < nvec; v += nt) {
        const float4 x = gv[v];
        const int i = head + 4 * v;
        int r = i / npix, c = i - r * npix;
        float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = e[k] - sub[r];
            if (++c == npix) {
                c = 0;
                ++r;
            }
        }
        ov[v] = make_float4(e[0], e[1], e[2], e[3]);
    }
    const int tail = head + 4 * nvec;
    if (t < total - tail) o[tail + t] = g[tail + t] - sub[(tail + t) / npix];
}

// One workgroup per cutout: exclusive scan of keep -> src[j] = cadence of the j-th kept one, the compacted time / SAP flux
// / error columns (float64 = the float32 sums widened; lcf = the float32 flux itself) and the spline knots
// [t[0], lerp(t[lo], t[lo + 1], g) per interior knot, t[n - 1]] (np.percentile of non-decreasing times: numpy's _lerp,
// a + (b - a) g, replaced by b - (b - a)(1 - g) where g >= 0.5).  Nothing is written past n kept cadences; a count
// other than n raises bit 1 of *flags.
__global__ __launch_bounds__(256) void cube_compact_kernel(const uint8_t *__restrict__ keep, const double *__restrict__ time,
                                                           const float *__restrict__ f32, const float *__restrict__ e32, int N,
                                                           int n, int *__restrict__ src, double *__restrict__ t_out,
                                                           double *__restrict__ y_out, double *__restrict__ e_out,
                                                           float *__restrict__ lcf_out, int n_inner,
                                                           const int *__restrict__ knot_lo, const double *__restrict__ knot_g,
                                                           double *__restrict__ knots, int *__restrict__ flags) {
    __shared__ int s_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t in0 = (size_t)b * N, out0 = (size_t)b * n;
    int base = 0;
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int i = c0 + tid;
        const bool k = i < N && keep[in0 + i] != 0;
        const unsigned long long bal = __ballot(k);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_cnt[w];
            all += s_cnt[w];
        }
        const int pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (k && pos < n) {
            src[out0 + pos] = i;
            if (t_out) t_out[out0 + pos] = time[in0 + i];
            if (y_out) y_out[out0 + pos] = (double)f32[in0 + i];
            if (e_out) e_out[out0 + pos] = (double)e32[in0 + i];
            if (lcf_out) lcf_out[out0 + pos] = f32[in0 + i];
        }
        base += all;
        __syncthreads();
    }
    if (base != n) {
        if (tid == 0) atomicOr(flags, 2);
        return;
    }
    if (!knots) return;
    __syncthreads();  // this workgroup's own t_out is read back below
    const double *t = t_out + out0;
    for (int k = tid; k < n_inner + 2; k += 256) {
        double r;
        if (k == 0) {
            r = t[0];
        } else if (k == n_inner + 1) {
            r = t[n - 1];
        } else {
            const int lo = knot_lo[k - 1];
            const double g = knot_g[k - 1], a = t[lo], bb = t[min(lo + 1, n - 1)], d = bb - a;
            r = g >= 0.5 ? bb - d * (1.0 - g) : a + d * g;
        }
        knots[(size_t)b * (n_inner + 2) + k] = r;
    }
}

// out[b][j][q] = cube[b][src[b][j]][idx[b][q]] (idx NULL: every pixel in place); a value that is not finite raises bit 0 of
// *flags.  A negative idx entry is padding (lk_pld_gather_ragged_batch_dev: cutouts whose masks differ in size share one row
// pitch): that column is +0.0f in every row and does not count as a pixel; an entry >= npix raises bit 2 and reads nothing.
__global__ __launch_bounds__(256) void cube_gather_kernel(const float *__restrict__ cube, const int *__restrict__ src,
                                                          const int *__restrict__ idx, int idx_stride, int N, int npix, int n,
                                                          int P, float *__restrict__ out, int *__restrict__ flags) {
    const int b = blockIdx.y;
    const long long total = (long long)n * P;
    const float *cb = cube + (size_t)b * N * npix;
    const int *sb = src + (size_t)b * n;
    const int *ib = idx ? idx + (size_t)b * idx_stride : nullptr;
    if (*reinterpret_cast<volatile int *>(flags) & 2) return;  // cube_compact_kernel did not fill src (keep does not hold n)
    bool bad = false, oob = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / P), q = (int)(i - (long long)j * P);
        const int row = sb[j];
        if ((unsigned)row >= (unsigned)N) continue;
        const int px = ib ? ib[q] : q;
        oob = oob || px >= npix;
        const float v = (unsigned)px < (unsigned)npix ? cb[(size_t)row * npix + px] : 0.0f;
        out[(size_t)b * total + i] = v;
        bad = bad || !isfinite(v);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, 1);
    if (__any(oob) && (threadIdx.x & 63) == 0) atomicOr(flags, 4);
}

// threshold_mask_from_median_image (correctors/pldcorrector.py; reference targetpixelfile.py:700-742) of one cutout per
// workgroup, on the float64 median image cube_median_image_kernel wrote:
//   vals = the finite pixels; mad = median(|vals - median(vals)|); cut = (1.4826 * mad * threshold) + nanmedian(image), every
//   product and the sum rounded on its own in that order; mask = nan_to_num(image) >= cut (NaN -> 0, +-inf -> +-DBL_MAX).
//   No finite pixel: the medians are NaN, so is the cut, and the mask is empty.
// With a reference pixel (use_ref) and a mask that is not empty: 4-connected labelling by minimum-label propagation in LDS
// (label = smallest pixel number of the region; every sweep also jumps to the label's own label) until a sweep changes
// nothing, then the region of the masked pixel nearest to (ref_col, ref_row) is kept — squared distances in double, the first
// minimum in row-major order (np.argmin over np.argwhere; tests/test_threshold_mask_cpu.py: same order as np.hypot).
// invert flips the result ('background' = ~threshold_mask(0, None)).  Outputs: mask bytes, the count, and the selected pixel
// numbers in ascending order padded with -1.  lab[] holds -1 for a pixel outside the mask.
constexpr int TM_MAX_NPIX = LK_CUBE_MASK_MAX_NPIX;
__global__ __launch_bounds__(256) void cube_threshold_mask_kernel(const double *__restrict__ median, int ny, int nx,
                                                                  double threshold, int use_ref, double ref_col, double ref_row,
                                                                  int invert, uint8_t *__restrict__ mask_out,
                                                                  int *__restrict__ count_out, int *__restrict__ idx_out) {
    __shared__ unsigned long long sh[264];
    __shared__ int lab[TM_MAX_NPIX];
    __shared__ int s_flag, s_cnt[4], s_bi[256];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, npix = ny * nx;
    const double *im = median + (size_t)b * npix;
    auto finite = [&](int i) { return isfinite(im[i]); };
    auto notnan = [&](int i) { return !isnan(im[i]); };
    auto raw = [&](int i) { return im[i]; };
    long long nf = 0, nn = 0;
    for (int i = tid; i < npix; i += 256) {
        nf += finite(i) ? 1 : 0;
        nn += notnan(i) ? 1 : 0;
    }
    nf = block_count_dyn(nf, reinterpret_cast<long long *>(sh));
    nn = block_count_dyn(nn, reinterpret_cast<long long *>(sh));
    const double m1 = block_median(npix, nf, raw, finite, sh);
    auto dev = [&](int i) { return fabs(im[i] - m1); };
    const double mad = block_median(npix, nf, dev, finite, sh);
    const double nanmed = block_median(npix, nn, raw, notnan, sh);
    const double cut = __dadd_rn(__dmul_rn(__dmul_rn(1.4826, mad), threshold), nanmed);
    int any = 0;
    for (int i = tid; i < npix; i += 256) {
        double v = im[i];
        if (isnan(v)) v = 0.0;
        else if (isinf(v)) v = v > 0.0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
        const bool in = v >= cut;
        lab[i] = in ? i : -1;
        any |= in ? 1 : 0;
    }
    if (tid == 0) s_flag = 0;
    __syncthreads();
    if (any) s_flag = 1;
    __syncthreads();
    const bool nonempty = s_flag != 0;
    if (use_ref && nonempty) {
        volatile int *vl = lab;
        for (;;) {
            __syncthreads();   // every thread has read the previous sweep's flag
            if (tid == 0) s_flag = 0;
            __syncthreads();
            bool ch = false;
            for (int i = tid; i < npix; i += 256) {
                const int own = vl[i];
                if (own < 0) continue;
                const int r = i / nx, c = i - r * nx;
                int m = own;
                if (r > 0 && vl[i - nx] >= 0) m = min(m, vl[i - nx]);
                if (r + 1 < ny && vl[i + nx] >= 0) m = min(m, vl[i + nx]);
                if (c > 0 && vl[i - 1] >= 0) m = min(m, vl[i - 1]);
                if (c + 1 < nx && vl[i + 1] >= 0) m = min(m, vl[i + 1]);
                m = min(m, vl[m]);   // (m is a masked pixel of this region: its label is one too, and never larger)
                if (m < own) {
                    vl[i] = m;
                    ch = true;
                }
            }
            if (ch) s_flag = 1;
            __syncthreads();
            if (!s_flag) break;
        }
        // the masked pixel nearest to the reference pixel: (squared distance, pixel number) smallest first
        double bd = __longlong_as_double(0x7ff0000000000000ll);
        int bi = 0x7fffffff;
        for (int i = tid; i < npix; i += 256) {
            if (lab[i] < 0) continue;
            const int r = i / nx, c = i - r * nx;
            const double dr = (double)r - ref_row, dc = (double)c - ref_col;
            const double d2 = __dadd_rn(__dmul_rn(dr, dr), __dmul_rn(dc, dc));
            if (d2 < bd || (d2 == bd && i < bi)) {
                bd = d2;
                bi = i;
            }
        }
        double *shd = reinterpret_cast<double *>(sh);
        shd[tid] = bd;
        s_bi[tid] = bi;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const double od = shd[tid + s];
                const int oi = s_bi[tid + s];
                if (od < shd[tid] || (od == shd[tid] && oi < s_bi[tid])) {
                    shd[tid] = od;
                    s_bi[tid] = oi;
                }
            }
            __syncthreads();
        }
        const int keep_label = lab[s_bi[0]];
        __syncthreads();
        for (int i = tid; i < npix; i += 256)
            if (lab[i] != keep_label) lab[i] = -1;
        __syncthreads();
    }
    // mask, count and the ascending index list (ballot scan over chunks of 256 pixels)
    int base = 0;
    for (int c0 = 0; c0 < npix; c0 += 256) {
        const int i = c0 + tid;
        const bool sel = i < npix && ((lab[i] >= 0) != (invert != 0));
        const unsigned long long bal = __ballot(sel);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_cnt[w];
            all += s_cnt[w];
        }
        if (i < npix) mask_out[(size_t)b * npix + i] = sel ? 1 : 0;
        if (sel) idx_out[(size_t)b * npix + base + before + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        base += all;
        __syncthreads();
    }
    for (int i = base + tid; i < npix; i += 256) idx_out[(size_t)b * npix + i] = -1;
    if (tid == 0) count_out[b] = base;
}

// out = (y - model) + (spline - np.median(spline)) per cutout, or y - model without a spline part
__global__ __launch_bounds__(1024) void pld_corrected_kernel(const double *__restrict__ y, const double *__restrict__ model,
                                                             const double *__restrict__ spline, int N, double *__restrict__ out) {
    __shared__ unsigned long long sh[1024];
    const size_t o = (size_t)blockIdx.x * N;
    const int tid = threadIdx.x;
    double med = 0.0;
    if (spline) {
        auto val = [&](int i) { return spline[o + i]; };
        auto keep = [&](int) { return true; };
        med = block_median(N, (long long)N, val, keep, sh);
    }
    for (int i = tid; i < N; i += 1024) {
        const double d = y[o + i] - model[o + i];
        out[o + i] = spline ? d + (spline[o + i] - med) : d;
    }
}

int cube_aperture_launch(lk_handle *h, int B, int N, int npix, const float *flux, const float *flux_err, const uint8_t *mask,
                         int mask_stride, float *flux_out, float *err_out, uint8_t *keep_out, int64_t *kept_host,
                         int64_t *nonfinite_host, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 2 && npix >= 1, "need 1 <= B <= 65535, N >= 2, npix >= 1");
    LK_REQUIRE(flux && flux_err && mask && flux_out && err_out && keep_out && kept_host, "NULL buffer");
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    unsigned long long *d_cnt;
    if (const int rc = Scratch(h, h->ws).buf(d_cnt, (size_t)2 * B).carve(stream)) return rc;
    LK_HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)2 * B * 8, stream));
    const int W = std::min(npix, AP_WMAX), pitch = W | 1;
    const size_t lds = (size_t)2 * AP_T * pitch * 4 + (size_t)((W + 15) & ~15);
    hipLaunchKernelGGL(cube_aperture_kernel, dim3((N + AP_T - 1) / AP_T, B), dim3(256), lds, stream, flux, flux_err, mask,
                       mask_stride, B, N, npix, W, pitch, flux_out, err_out, keep_out, d_cnt);
    LK_HIP_CHECK(hipGetLastError());
    std::vector<int64_t> cnt((size_t)2 * B);
    LK_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)2 * B * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    for (int b = 0; b < B; ++b) {
        kept_host[b] = cnt[b];
        if (nonfinite_host) nonfinite_host[b] = cnt[(size_t)B + b];
    }
    return LK_OK;
}

int cube_centroids_launch(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask, int mask_stride,
                          double column0, double row0, double *col_out, double *row_out, hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(nx >= 1 && npix % nx == 0, "npix = %d is not a whole number of rows of nx = %d pixels", npix, nx);
    LK_REQUIRE(flux && mask && col_out && row_out, "NULL buffer");
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    hipLaunchKernelGGL(cube_centroids_kernel, dim3((N + 3) / 4, B), dim3(256), 0, stream, flux, mask, mask_stride, N, npix, nx,
                       column0, row0, col_out, row_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_centroids_quadratic_launch(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                    int mask_stride, double column0, double row0, double *col_out, double *row_out,
                                    int32_t *peak_out, hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(nx >= 1 && npix % nx == 0, "npix = %d is not a whole number of rows of nx = %d pixels", npix, nx);
    LK_REQUIRE(nx >= 3 && npix / nx >= 3, "the quadratic centroid fits a 3 x 3 patch: a %d x %d cutout is too small", npix / nx, nx);
    LK_REQUIRE(flux && mask && col_out && row_out, "NULL buffer");
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    hipLaunchKernelGGL(cube_centroids_quadratic_kernel, dim3((N + 3) / 4, B), dim3(256), 0, stream, flux, mask, mask_stride, N,
                       npix, nx, column0, row0, col_out, row_out, (int *)peak_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int image_centroids_launch(lk_handle *h, int B, int npix, int nx, const double *image, const uint8_t *mask, int mask_stride,
                           double column0, double row0, int method, double *col_out, double *row_out, int32_t *peak_out,
                           hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && npix >= 1, "need B >= 1 images of at least one pixel");
    LK_REQUIRE(nx >= 1 && npix % nx == 0, "npix = %d is not a whole number of rows of nx = %d pixels", npix, nx);
    LK_REQUIRE(method == LK_CENTROID_MOMENTS || method == LK_CENTROID_QUADRATIC, "method must be LK_CENTROID_MOMENTS or LK_CENTROID_QUADRATIC");
    LK_REQUIRE(method == LK_CENTROID_MOMENTS || (nx >= 3 && npix / nx >= 3),
               "the quadratic centroid fits a 3 x 3 patch: a %d x %d image is too small", npix / nx, nx);
    LK_REQUIRE(image && mask && col_out && row_out, "NULL buffer");
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    hipLaunchKernelGGL(image_centroids_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, image, mask, mask_stride, B, npix, nx,
                       column0, row0, method == LK_CENTROID_QUADRATIC ? 1 : 0, col_out, row_out, (int *)peak_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_diffimage_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const float *flux_err,
                          const double *period_host, const double *transit_time_host, const double *duration_host, double in_width,
                          double out_inner, double out_outer, uint8_t *cls, double *mean_in, double *mean_out, double *diff,
                          double *diff_err, int32_t *n_in, int32_t *n_out, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(time && flux && flux_err && cls && mean_in && mean_out && diff && diff_err && n_in && n_out, "NULL buffer");
    LK_REQUIRE(period_host && transit_time_host && duration_host, "NULL box parameters");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    LK_REQUIRE(in_width > 0.0 && in_width <= out_inner && out_inner < out_outer,
               "need 0 < in_width <= out_inner < out_outer (got %g, %g, %g)", in_width, out_inner, out_outer);
    for (int b = 0; b < B; ++b)
        LK_REQUIRE(period_host[b] != 0.0 && period_host[b] == period_host[b], "cutout %d: the period must be a non-zero number", b);
    const int chunks = (N + DI_CHUNK - 1) / DI_CHUNK;
    std::vector<double> par((size_t)3 * B);
    for (int b = 0; b < B; ++b) {
        par[b] = period_host[b];
        par[(size_t)B + b] = transit_time_host[b];
        par[2 * (size_t)B + b] = duration_host[b];
    }
    double *d_par, *d_psum;
    int *d_pcnt;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)par.data(), par.size())
                           .buf(d_psum, (size_t)B * chunks * 4 * npix)
                           .buf(d_pcnt, (size_t)B * chunks * 2 * npix)
                           .carve(stream))
        return rc;
    LK_HIP_CHECK(hipMemsetAsync(n_in, 0, (size_t)B * 4, stream));
    LK_HIP_CHECK(hipMemsetAsync(n_out, 0, (size_t)B * 4, stream));
    hipLaunchKernelGGL(cube_diffimage_class_kernel, dim3((N + 255) / 256, B), dim3(256), 0, stream, time, (const double *)d_par, B, N,
                       in_width, out_inner, out_outer, cls, (int *)n_in, (int *)n_out);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cube_diffimage_accum_kernel, dim3(chunks, B), dim3(DI_T), 0, stream, flux, flux_err, (const uint8_t *)cls, N,
                       npix, chunks, d_psum, d_pcnt);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cube_diffimage_finish_kernel, dim3((npix + 255) / 256, B), dim3(256), 0, stream, (const double *)d_psum,
                       (const int *)d_pcnt, npix, chunks, mean_in, mean_out, diff, diff_err);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int centroid_offsets_launch(lk_handle *h, int B, const int32_t *fit_status, const int32_t *n_in, const int32_t *n_out,
                            const double *a_col, const double *a_row, const double *b_col, const double *b_row, double *offset,
                            double *offset_pix, int32_t *status, hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1, "need B >= 1 cutouts");
    LK_REQUIRE((fit_status || (n_in && n_out)) && a_col && a_row && b_col && b_row && offset && offset_pix && status, "NULL buffer");
    hipLaunchKernelGGL(centroid_offsets_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, (const int *)fit_status,
                       (const int *)n_in, (const int *)n_out, a_col, a_row, b_col, b_row, offset, offset_pix, (int *)status);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_median_image_launch(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *keep, double *median,
                             hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(cube && median, "NULL buffer");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    hipLaunchKernelGGL(cube_median_image_kernel, dim3((npix + MED_G - 1) / MED_G, B), dim3(256), 0, stream, cube, keep, N, npix,
                       median);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_background_launch(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *mask, int mask_stride,
                           int want_scatter, float *bkg, int32_t *n_pixels, float *scatter, float *cube_out, hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(cube && mask && bkg && n_pixels, "NULL buffer");
    LK_REQUIRE(!want_scatter || scatter, "want_scatter needs the scatter buffer");
    LK_REQUIRE(cube_out != cube, "cube_out must not be the cube itself");
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    // the route depends on npix alone: a cutout's bits are the same in any batch
    if (npix <= BG_SMALL_MAX_NPIX) {
        const int pitch = npix | 1;
        hipLaunchKernelGGL(cube_background_kernel, dim3((N + BG_T - 1) / BG_T, B), dim3(256), (size_t)BG_T * pitch * 4, stream, cube,
                           mask, mask_stride, N, npix, pitch, want_scatter ? 1 : 0, bkg, (int *)n_pixels, scatter, cube_out);
    } else {
        hipLaunchKernelGGL(cube_background_wide_kernel, dim3(N, B), dim3(256), 0, stream, cube, mask, mask_stride, N, npix,
                           want_scatter ? 1 : 0, bkg, (int *)n_pixels, scatter, cube_out);
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_subtract_rows_launch(lk_handle *h, int B, int N, int npix, const float *cube, const float *rows, float *cube_out,
                              hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && npix >= 1, "need 1 <= B <= 65535, N >= 1, npix >= 1");
    LK_REQUIRE(cube && rows && cube_out, "NULL buffer");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    // 4 values per thread and 4 trips: enough workgroups in flight per cutout to stream, few enough to amortise their start
    const int gx = (int)std::min<int64_t>(((int64_t)N * npix + 4095) / 4096, 1024);
    hipLaunchKernelGGL(cube_subtract_rows_kernel, dim3(gx, B), dim3(256), 0, stream, cube, rows, N, npix, cube_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int cube_threshold_mask_launch(lk_handle *h, int B, int ny, int nx, const double *median, double threshold, int use_ref,
                               double ref_col, double ref_row, int invert, uint8_t *mask, int32_t *count, int32_t *idx,
                               hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && ny >= 1 && nx >= 1, "need B >= 1 cutouts of at least one pixel");
    LK_REQUIRE((int64_t)ny * nx <= LK_CUBE_MASK_MAX_NPIX, "a %d x %d cutout has more than the %d pixels the device labelling holds in LDS",
               ny, nx, LK_CUBE_MASK_MAX_NPIX);
    LK_REQUIRE(median && mask && count && idx, "NULL buffer");
    LK_REQUIRE(!use_ref || (ref_col == ref_col && ref_row == ref_row), "the reference pixel is NaN");
    hipLaunchKernelGGL(cube_threshold_mask_kernel, dim3(B), dim3(256), 0, stream, median, ny, nx, threshold, use_ref, ref_col,
                       ref_row, invert, mask, (int *)count, (int *)idx);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int pld_gather_launch(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time, const float *flux32,
                      const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx_host, int pld_idx_stride, int Pb,
                      const int32_t *bkg_idx_host, int bkg_idx_stride, int n_inner, const int32_t *knot_lo_host,
                      const double *knot_g_host, double *t_out, double *y_out, double *err_out, float *lcf_out, float *pld_out,
                      float *bkg_out, double *knots_out, int *nonfinite_host, hipStream_t stream, const int32_t *pld_idx_dev,
                      const int32_t *bkg_idx_dev) {
    // pld_idx_dev / bkg_idx_dev (lk_pld_gather_ragged_batch_dev): per-cutout index lists already on the device, -1 = padding,
    // any stride >= P / Pb; the kernel checks their entries, the host lists are NULL then
    const bool ragged = pld_idx_dev || bkg_idx_dev;
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 2 && npix >= 1 && n >= 1 && n <= N, "need 1 <= B <= 65535, N >= 2, npix >= 1, 1 <= n <= N");
    LK_REQUIRE(cube && keep && nonfinite_host, "NULL buffer");
    LK_REQUIRE((!y_out && !lcf_out) || flux32, "the SAP flux columns need flux32");
    LK_REQUIRE(!err_out || err32, "the SAP error column needs err32");
    LK_REQUIRE(!t_out || time, "the compacted times need time");
    LK_REQUIRE((int64_t)N * npix < (int64_t)1 << 31, "a cutout of %d x %d values is too large", N, npix);
    LK_REQUIRE(P >= 0 && P <= npix && Pb >= 0 && Pb <= npix, "P and Pb must be between 0 and npix");
    LK_REQUIRE(pld_idx_host || pld_idx_dev || P == 0 || P == npix, "pld_idx may only be NULL for all pixels or none");
    LK_REQUIRE(bkg_idx_host || bkg_idx_dev || Pb == 0 || Pb == npix, "bkg_idx may only be NULL for all pixels or none");
    if (ragged) {
        LK_REQUIRE(!pld_idx_host && !bkg_idx_host, "index lists are either all on the host or all on the device");
        LK_REQUIRE(!pld_idx_dev || pld_idx_stride >= P, "pld_idx_stride must be >= P");
        LK_REQUIRE(!bkg_idx_dev || bkg_idx_stride >= Pb, "bkg_idx_stride must be >= Pb");
    } else {
        LK_REQUIRE(pld_idx_stride == 0 || pld_idx_stride == P, "pld_idx_stride must be 0 (shared) or P");
        LK_REQUIRE(bkg_idx_stride == 0 || bkg_idx_stride == Pb, "bkg_idx_stride must be 0 (shared) or Pb");
    }
    LK_REQUIRE(n_inner >= 0, "n_inner must be >= 0");
    if (knots_out) {
        LK_REQUIRE(t_out, "the knots are taken from the compacted times: t_out is NULL");
        LK_REQUIRE(n_inner == 0 || (knot_lo_host && knot_g_host), "NULL knot plan");
        for (int k = 0; k < n_inner; ++k)
            LK_REQUIRE(knot_lo_host[k] >= 0 && knot_lo_host[k] < n && knot_g_host[k] >= 0.0 && knot_g_host[k] <= 1.0,
                       "knot %d: index %d / weight %g outside the %d kept cadences", k, knot_lo_host[k], knot_g_host[k], n);
    }
    const size_t n_pi = pld_idx_host ? (size_t)(pld_idx_stride ? B : 1) * P : 0;
    const size_t n_bi = bkg_idx_host ? (size_t)(bkg_idx_stride ? B : 1) * Pb : 0;
    for (size_t i = 0; i < n_pi; ++i)
        LK_REQUIRE(pld_idx_host[i] >= 0 && pld_idx_host[i] < npix, "pld_idx[%zu] = %d is not a pixel of the cutout", i, pld_idx_host[i]);
    for (size_t i = 0; i < n_bi; ++i)
        LK_REQUIRE(bkg_idx_host[i] >= 0 && bkg_idx_host[i] < npix, "bkg_idx[%zu] = %d is not a pixel of the cutout", i, bkg_idx_host[i]);
    const size_t nk = knots_out ? (size_t)n_inner : 0;
    int *d_src, *d_pi, *d_bi, *d_klo, *d_flags;
    double *d_kg;
    Scratch ws(h, h->ws);
    ws.buf(d_src, (size_t)B * n)
        .upload(d_pi, pld_idx_host, n_pi, n_pi != 0)
        .upload(d_bi, bkg_idx_host, n_bi, n_bi != 0)
        .upload(d_klo, knot_lo_host, nk, nk != 0).upload(d_kg, knot_g_host, nk, nk != 0)
        .buf(d_flags, 1);
    if (const int rc = ws.carve(stream)) return rc;
    LK_HIP_CHECK(hipMemsetAsync(d_flags, 0, 4, stream));
    hipLaunchKernelGGL(cube_compact_kernel, dim3(B), dim3(256), 0, stream, keep, time, flux32, err32, N, n, d_src, t_out, y_out,
                       err_out, lcf_out, n_inner, d_klo, d_kg, knots_out, d_flags);
    LK_HIP_CHECK(hipGetLastError());
    // (no output: the caller uses the resident cube itself as that block — all pixels, no cadence dropped — and has the
    // finite-pixel count of cube_aperture instead)
    const int gx = (int)std::min<int64_t>(((int64_t)n * std::max(P, Pb) + 1023) / 1024 + 1, 4096);
    if (P > 0 && pld_out) {
        hipLaunchKernelGGL(cube_gather_kernel, dim3(gx, B), dim3(256), 0, stream, cube, (const int *)d_src,
                           pld_idx_dev ? (const int *)pld_idx_dev : (const int *)d_pi, pld_idx_stride, N, npix, n, P, pld_out, d_flags);
        LK_HIP_CHECK(hipGetLastError());
    }
    if (Pb > 0 && bkg_out) {
        hipLaunchKernelGGL(cube_gather_kernel, dim3(gx, B), dim3(256), 0, stream, cube, (const int *)d_src,
                           bkg_idx_dev ? (const int *)bkg_idx_dev : (const int *)d_bi, bkg_idx_stride, N, npix, n, Pb, bkg_out, d_flags);
        LK_HIP_CHECK(hipGetLastError());
    }
    int flags = 0;
    LK_HIP_CHECK(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    LK_REQUIRE(!(flags & 2), "keep does not flag exactly n = %d cadences in every cutout", n);
    LK_REQUIRE(!(flags & 4), "an index list names a pixel outside the cutout's %d", npix);
    *nonfinite_host = flags & 1;
    return LK_OK;
}

int pld_corrected_launch(lk_handle *h, int B, int N, const double *y, const double *model, const double *spline, double *out,
                         hipStream_t stream) {
    (void)h;
    LK_REQUIRE(B >= 1 && N >= 1 && y && model && out, "bad arguments");
    hipLaunchKernelGGL(pld_corrected_kernel, dim3(B), dim3(1024), 0, stream, y, model, spline, N, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
