// prffit.hip — PSF photometry with a TABULATED PRF that fits each cadence's pointing shift, on resident pixel cubes on gfx950:
// psffit.hip's iteration (per cadence the fluxes of up to 8 stars, a constant background and one common (column, row) shift of
// all stars, by variable projection) with prfphot.hip's model (Keys' cubic convolution on a super-sampled table) and the
// model's derivative by the centre from the same 16 taps.
//
// Reference: TabulatedPRF.evaluate_with_gradient and PixelCube.psf_fit(prf=) (correctors/pldcorrector.py), plain float64 numpy;
// include/lkhip.h has the definition.
//
//   polyphase  prfphot.hip's copy of the table (prf_polyphase_launch), once per call, before the fit launches.
//   fit        workgroup (tile of cadences, cutout) of PRF_FORM_THREADS = 512 threads (256 at S = 7 and 8: prf_fit_threads),
//              instantiated on the star count S.  The tile
//              is PSF_T = 16 cadences, or 8 where 16 do not fit the LDS (a launch argument; lanes of cadences beyond the tile are
//              inactive, as at a cutout's last tile).  The tile of flux and flux_err and the mask are staged in LDS once and the
//              used pixels counted once.  Wavefront 0 is psffit.hip's wavefront — PSF_LPC = 4 adjacent lanes per cadence, with
//              the cadence's status, phase, shift u, n_iter and last_step in registers — and the others only form images.
//              One pass (an evaluation at every cadence's current u), at most max_iter + 1 of them:
//                taps    wavefront 0 has left every cadence's u in LDS; all threads share out the tile's (cadence, star) pairs:
//                        prfphot.hip's taps plus the eight derivative weights w'(f) x -os (192 bytes a pair);
//                images  every wavefront takes pairs in turn, lane = pixel, and parks the S model images of every cadence in
//                        LDS (prf_value, [cadence][star][pixel] with prfphot.hip's pitch rule);
//                walk 1  wavefront 0: G = A^T W A and A^T W y over each lane's pixel rows in index order, the fixed butterfly,
//                        the Cholesky and the solve (psffit.hip's, with av[s] read from LDS); theta[cadence][0 .. S] to LDS;
//                deriv.  every wavefront takes cadences in turn, lane = pixel: D0 = sum_s theta_s dP_s/dc and D1 = sum_s theta_s
//                        dP_s/dr, s in index order, from the same 16 taps and the same branch-free loads, parked in LDS: 2 npix
//                        doubles per cadence (per-star derivative images would be 2 S npix: 186 KB at 11 x 11 with 4 stars);
//                walk 2  wavefront 0: C = A^T W D, E = D^T W D, g = D^T W r and chi2, the Schur complement, and then the step
//                        or the outputs exactly as cube_psffit_kernel; the new u and "a cadence is not done" to LDS.
//              The loop condition is workgroup-uniform: every thread reads the flag that wavefront 0 wrote before the pass's last
//              barrier, no wavefront leaves before the loop ends, and all five barriers of a pass are outside every condition.
//   status     psfphot.hip's status kernel: 1 when no cadence is ok.
//
// LDS per workgroup = tile x (8 (mpitch + dpitch + S + 3) + 192 S + 4 pitch (8 with flux_err)) + 8 + npix bytes, mpitch, dpitch
// and pitch the padded S npix, 2 npix and npix: at 11 x 11 with flux_err and 16 cadences 122 369 bytes at S = 4 and 160 513 at S =
// 6; S = 7 would need 179 073, above PSF_MAX_LDS, so S = 7 and 8 run tiles of 8 cadences there (89 601 and 98 881 bytes).  The
// launcher refuses a call (LK_EINVAL with the byte count, before every launch) only when 8 cadences do not fit either.
//
// No atomics; a cadence's sums meet only across its own four lanes and their order depends on the cutout's own data alone, so a
// cutout's outputs have the same bits alone, at any batch position, at either tile length, with a shared or a per-cutout table
// index and from run to run.
#include "prf_common.hpp"  // the polyphase table, the taps and the value, shared with prfphot.hip
#include "psf_common.hpp"  // the lane mapping, the cadence sum, the Cholesky and the star grouping, shared with the Gaussian files
#include "stage_tile.hpp"

namespace lk {

namespace {

constexpr int PRF_FIT_SHORT_TILE = 8;  // the tile where PSF_T cadences do not fit the LDS

// The workgroup of S stars: PRF_FORM_THREADS (eight wavefronts, 256 registers a lane) up to 6 stars.  At 7 and 8 stars L, theta
// and C of walk 2 do not fit 256 registers (60 and 224 bytes of scratch a lane), so these run four wavefronts with 512 registers
// a lane and no scratch; prfphot.hip measured four forming wavefronts within 5 % of eight.
constexpr int prf_fit_threads(int S) { return S <= 6 ? PRF_FORM_THREADS : PRF_FORM_THREADS / 2; }

// prfphot.hip's taps of one (star, cadence) and the derivatives of its eight weights by the star's centre.  192 bytes.
struct PrfGradTaps {
    PrfTaps t;
    double dw[8];
};

__device__ __forceinline__ void prf_grad_taps(PrfGradTaps &t, double c, double r, const PrfTable &g) {
    const int sub = g.TYp * g.TXp;
    prf_axis(c, g.hx, g.os, sub, t.t.w, t.t.x0, t.t.xph, t.dw);
    prf_axis(r, g.hy, g.os, sub * g.os, t.t.w + 4, t.t.y0, t.t.yph, t.dw + 4);
}

// dP/dc and dP/dr at pixel (iy, ix): prf_value's taps and order with w' on one axis and w on the other
__device__ __forceinline__ void prf_gradient(const PrfGradTaps &t, const float *__restrict__ tp, int TYp, int TXp, int iy, int ix,
                                             double &dc, double &dr) {
    double ac = 0.0, ar = 0.0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const unsigned Y = (unsigned)(t.t.y0[jj] + iy);
        const bool oky = Y < (unsigned)TYp;
        const unsigned rb = (unsigned)t.t.yph[jj] + Y * (unsigned)TXp;
        double r = 0.0, rc = 0.0;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const unsigned X = (unsigned)(t.t.x0[ii] + ix);
            const bool ok = oky && X < (unsigned)TXp;
            const float v = tp[ok ? rb + (unsigned)t.t.xph[ii] + X : 0u];  // no branch: a tap off the table reads sample 0 and counts 0
            const double x = ok ? (double)v : 0.0;
            r += t.t.w[ii] * x;
            rc += t.dw[ii] * x;
        }
        ac += t.t.w[4 + jj] * rc;
        ar += t.dw[4 + jj] * r;
    }
    dc = ac, dr = ar;
}

}  // namespace

struct PrfFitArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask;
    const int *order, *star_off;  // order: the cutouts of this launch (one star count)
    const double *par;            // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first); the two widths are not used
    const double *u0_col, *u0_row;  // nullable: the initial shifts
    PrfTable tab;
    double column0, row0, tol, max_step, max_shift;
    unsigned long long inv_nx;  // ceil(2^32 / nx): p / nx = (p inv_nx) >> 32 for p nx < 2^32
    int mask_stride, S_max, N, ny, nx, pitch, mpitch, dpitch, tile, use_err, max_iter;
    double *time_out, *flux_out, *err_out, *bkg, *chi2;  // time_out nullable
    double *shift_col, *shift_row, *shift_col_err, *shift_row_err, *last_step;
    int *n_used, *n_iter;
    int8_t *cstat;
};

template <int S> __global__ __launch_bounds__(prf_fit_threads(S)) void cube_prffit_kernel(const PrfFitArgs a) {
    constexpr int K = S + 1, THREADS = prf_fit_threads(S), WAVES = THREADS / 64;
    extern __shared__ __align__(16) double prffit_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cl = lane / PSF_LPC, sub = lane % PSF_LPC;
    const int T = a.tile, b = a.order[blockIdx.y], c0 = blockIdx.x * T;
    const int rows = min(T, a.N - c0), npix = a.ny * a.nx;
    const bool fitter = wave == 0, active = fitter && cl < rows;
    const int cs = cl < rows ? cl : 0;  // the LDS slot this lane reads: a lane without a cadence reads slot 0 and writes nothing
    double *mod = prffit_lds;                 // the model images [cadence][star][pixel], cadence pitch mpitch
    double *der = mod + T * a.mpitch;         // D0 | D1 [cadence][2][pixel], cadence pitch dpitch
    double *th = der + T * a.dpitch;          // theta [cadence][K]
    double *uu = th + T * K;                  // the current shift [cadence][2]
    int *flag = reinterpret_cast<int *>(uu + 2 * T);  // a cadence of the tile is not done (one double's room)
    PrfGradTaps *taps = reinterpret_cast<PrfGradTaps *>(uu + 2 * T + 1);  // [cadence][star]
    float *tf = reinterpret_cast<float *>(taps + T * S);
    float *te = tf + T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + T * a.pitch : te);

    const size_t cad = (size_t)b * a.N + c0 + cs, off = ((size_t)b * a.N + c0) * npix;
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = tid; i < npix; i += THREADS) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    const double u0c = a.u0_col ? a.u0_col[cad] : 0.0, u0r = a.u0_row ? a.u0_row[cad] : 0.0;
    const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
    const float *tp = a.tab.tp + (size_t)a.tab.index[b] * a.tab.os * a.tab.os * a.tab.TYp * a.tab.TXp;
    __syncthreads();

    // wavefront 0: the used pixels do not depend on the shift, counted once; the cadence's state
    const float *yrow = tf + cs * a.pitch, *erow = te + cs * a.pitch;
    const double *mrow = mod + cs * a.mpitch, *drow = der + cs * a.dpitch;
    int n = 0, st = 0, phase = 2, nit = 0;  // phase: 0 iterating; 1 stopped and ok: the next evaluation writes the outputs; 2 done
    double uc = u0c, ur = u0r, last = NAN;
    if (fitter) {
        for (int iy = sub; iy < a.ny; iy += PSF_LPC)
            for (int ix = 0, q = iy * a.nx; ix < a.nx; ++ix, ++q) {
                const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                n += active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f ? 1 : 0;
            }
        n = psf_cadence_sum(n);
        st = !(isfinite(t) && isfinite(u0c) && isfinite(u0r)) ? 1 : n < S + 4 ? 2 : 0;
        phase = !active || st ? 2 : 0;
        if (active && sub == 0) uu[2 * cl] = uc, uu[2 * cl + 1] = ur;
        const int go = __any(phase != 2);
        if (lane == 0) *flag = go;
    }
    __syncthreads();

    // pass = the iteration number of every cadence that still iterates (they all start at pass 1); at most max_iter + 1 passes.
    // Every thread of the workgroup reads the same flag, so all of them take the same number of passes and meet at every barrier
    for (int pass = 1; pass <= a.max_iter + 1; ++pass) {
        if (!*flag) break;

        // taps at u: the threads share out the tile's (cadence, star) pairs
        for (int q = tid; q < rows * S; q += THREADS) {
            const int c = q / S, s = q - c * S;
            PrfGradTaps tq;
            prf_grad_taps(tq, p[s] + uu[2 * c] - a.column0, p[a.S_max + s] + uu[2 * c + 1] - a.row0, a.tab);
            taps[q] = tq;
        }
        __syncthreads();

        // the model images: every wavefront one pair after the other, lane = pixel
#pragma unroll 1
        for (int q = wave; q < rows * S; q += WAVES) {
            const int c = q / S, s = q - c * S;
            const PrfTaps tq = taps[q].t;
            double *dst = mod + c * a.mpitch + s * npix;
#pragma unroll 1
            for (int i = lane; i < npix; i += 64) {
                const int iy = (int)(((unsigned long long)i * a.inv_nx) >> 32);
                dst[i] = prf_value(tq, tp, a.tab.TYp, a.tab.TXp, iy, i - iy * a.nx);
            }
        }
        __syncthreads();

        // walk 1 (wavefront 0): G[i][j], i <= j, and rhs over this lane's pixel rows, in index order; column S is the constant
        double L[K][K], theta[K];
        bool singular = false;
        if (fitter) {
            double G[K][K], rhs[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                rhs[i] = 0.0;
#pragma unroll
                for (int j = 0; j < K; ++j) G[i][j] = 0.0;
            }
            for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
                int q = iy * a.nx;
                // no branch on the pixel: one that is not used enters with w = 0 and y = 0
#pragma unroll 2
                for (int ix = 0; ix < a.nx; ++ix, ++q) {
                    const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                    const bool used = active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                    const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                    double av[K];
#pragma unroll
                    for (int s = 0; s < S; ++s) av[s] = mrow[s * npix + q];
                    av[S] = 1.0;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const double wa = w * av[i];
                        rhs[i] += wa * y;
#pragma unroll
                        for (int j = i; j < K; ++j) G[i][j] += wa * av[j];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < K; ++i) {
                rhs[i] = psf_cadence_sum(rhs[i]);
#pragma unroll
                for (int j = i; j < K; ++j) G[i][j] = psf_cadence_sum(G[i][j]);
            }
            singular = psf_cholesky<K>(G, L);
            psf_solve<K>(L, rhs, theta);
            if (active && sub == 0) {
#pragma unroll
                for (int i = 0; i < K; ++i) th[cl * K + i] = theta[i];
            }
        }
        __syncthreads();

        // the theta-weighted derivative images: every wavefront one cadence after the other, lane = pixel
#pragma unroll 1
        for (int c = wave; c < rows; c += WAVES) {
            double *dst = der + c * a.dpitch;
#pragma unroll 1
            for (int i = lane; i < npix; i += 64) {
                const int iy = (int)(((unsigned long long)i * a.inv_nx) >> 32), ix = i - iy * a.nx;
                double d0 = 0.0, d1 = 0.0;
#pragma unroll 1
                for (int s = 0; s < S; ++s) {
                    double gc, gr;
                    prf_gradient(taps[c * S + s], tp, a.tab.TYp, a.tab.TXp, iy, ix, gc, gr);
                    const double ths = th[c * K + s];
                    d0 += ths * gc;
                    d1 += ths * gr;
                }
                dst[i] = d0;
                dst[npix + i] = d1;
            }
        }
        __syncthreads();

        // walk 2 (wavefront 0): r = y - A theta, D from LDS; C = A^T W D, E = D^T W D, g = D^T W r, chi2
        if (fitter) {
            double C0[K], C1[K], e00 = 0.0, e01 = 0.0, e11 = 0.0, g0 = 0.0, g1 = 0.0, chi = 0.0;
#pragma unroll
            for (int i = 0; i < K; ++i) C0[i] = C1[i] = 0.0;
            for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
                int q = iy * a.nx;
#pragma unroll 2
                for (int ix = 0; ix < a.nx; ++ix, ++q) {
                    const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                    const bool used = active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                    const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                    double av[K], m = theta[S];
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        av[s] = mrow[s * npix + q];
                        m += theta[s] * av[s];
                    }
                    av[S] = 1.0;
                    const double d0 = drow[q], d1 = drow[npix + q];
                    const double res = y - m, wd0 = w * d0, wd1 = w * d1;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        C0[i] += wd0 * av[i];
                        C1[i] += wd1 * av[i];
                    }
                    e00 += wd0 * d0, e01 += wd0 * d1, e11 += wd1 * d1;
                    g0 += wd0 * res, g1 += wd1 * res;
                    chi += w * (res * res);
                }
            }
#pragma unroll
            for (int i = 0; i < K; ++i) C0[i] = psf_cadence_sum(C0[i]), C1[i] = psf_cadence_sum(C1[i]);
            e00 = psf_cadence_sum(e00), e01 = psf_cadence_sum(e01), e11 = psf_cadence_sum(e11);
            g0 = psf_cadence_sum(g0), g1 = psf_cadence_sum(g1), chi = psf_cadence_sum(chi);

            // S2 = E - (L^-1 C)^T (L^-1 C), its Cholesky with the pivot cut on E_kk, du = S2^-1 g
            double s00 = e00, s01 = e01, s11 = e11;
            {
                double Y0[K], Y1[K];
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    double v0 = C0[i], v1 = C1[i];
#pragma unroll
                    for (int j = 0; j < i; ++j) v0 -= L[i][j] * Y0[j], v1 -= L[i][j] * Y1[j];
                    Y0[i] = v0 / L[i][i], Y1[i] = v1 / L[i][i];
                    s00 -= Y0[i] * Y0[i], s01 -= Y0[i] * Y1[i], s11 -= Y1[i] * Y1[i];
                }
            }
            singular = singular || !(isfinite(s00) && s00 > PSF_PIVOT_CUT * e00);
            const double l00 = sqrt(s00), l10 = s01 / l00, d11 = s11 - l10 * l10;
            singular = singular || !(isfinite(d11) && d11 > PSF_PIVOT_CUT * e11);
            const double l11 = sqrt(d11);

            if (phase == 1) {
                // the evaluation at the final u: psf_photometry's outputs at shifts = u, and the shift errors sqrt((S2^-1)_kk)
                if (singular) st = 3;
                else if (sub == 0) {
                    double var[K];
                    psf_variances<K>(L, var);
                    const size_t row0 = (size_t)a.star_off[b];
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const size_t o = (row0 + s) * a.N + c0 + cl;
                        a.flux_out[o] = theta[s];
                        a.err_out[o] = sqrt(var[s]);
                    }
                    a.bkg[cad] = theta[S];
                    a.chi2[cad] = chi;
                    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m10 = -l10 * m00 * m11;
                    a.shift_col_err[cad] = sqrt(m00 * m00 + m10 * m10);
                    a.shift_row_err[cad] = m11;
                }
                phase = 2;
            } else if (phase == 0) {
                if (singular) {
                    st = 3, phase = 2;
                } else {
                    const double z0 = g0 / l00, z1 = (g1 - l10 * z0) / l11;
                    double du1 = z1 / l11, du0 = (z0 - l10 * du1) / l00;
                    du0 = du0 > a.max_step ? a.max_step : du0 < -a.max_step ? -a.max_step : du0;
                    du1 = du1 > a.max_step ? a.max_step : du1 < -a.max_step ? -a.max_step : du1;
                    uc += du0, ur += du1, nit = pass;
                    last = fabs(du0) > fabs(du1) ? fabs(du0) : fabs(du1);
                    const double ec = fabs(uc - u0c), er = fabs(ur - u0r);
                    if ((ec > er ? ec : er) > a.max_shift) st = 5, phase = 2;
                    else if (a.tol > 0.0 && last < a.tol) phase = 1;
                    else if (pass == a.max_iter) {
                        if (a.tol > 0.0) st = 4, phase = 2;
                        else phase = 1;
                    }
                }
            }
            if (active && sub == 0) uu[2 * cl] = uc, uu[2 * cl + 1] = ur;
            const int go = __any(phase != 2);
            if (lane == 0) *flag = go;
        }
        __syncthreads();
    }

    if (!active || sub != 0) return;
    const bool ok = st == 0;
    const size_t row0 = (size_t)a.star_off[b];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const size_t o = (row0 + s) * a.N + c0 + cl;
        if (a.time_out) a.time_out[o] = t;
        if (!ok) a.flux_out[o] = a.err_out[o] = NAN;
    }
    if (!ok) a.bkg[cad] = a.chi2[cad] = a.shift_col_err[cad] = a.shift_row_err[cad] = NAN;
    a.shift_col[cad] = ok ? uc : NAN;
    a.shift_row[cad] = ok ? ur : NAN;
    a.last_step[cad] = last;
    a.n_iter[cad] = nit;
    a.n_used[cad] = n;
    a.cstat[cad] = (int8_t)st;
}

namespace {

template <int S> int prffit_launch(lk_handle *h, const PrfFitArgs &a, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_prffit_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_prffit_kernel<S>, dim3((a.N + a.tile - 1) / a.tile, count), dim3(prf_fit_threads(S)), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_prffit_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const float *prf_table, int n_prf, int Ty, int Tx, int oversample, const int32_t *prf_index_host,
                       const double *shift0_col, const double *shift0_row, int max_iter, double tol, double max_step,
                       double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off_host, double *time_out,
                       double *flux_out, double *flux_err_out, double *background, double *chi2, double *shift_col,
                       double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step, int32_t *n_iter,
                       int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && prf_table, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(flux_out && flux_err_out && background && chi2 && n_used && cadence_status && status, "NULL output buffer");
    LK_REQUIRE(shift_col && shift_row && shift_col_err && shift_row_err && last_step && n_iter, "NULL output buffer");
    LK_REQUIRE((shift0_col == nullptr) == (shift0_row == nullptr), "shift0_col and shift0_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
    LK_REQUIRE(max_iter >= 1 && max_iter <= 64, "max_iter must be 1 .. 64 (got %d)", max_iter);
    LK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "tol must be finite and >= 0 (got %g)", tol);
    LK_REQUIRE(max_step > 0.0 && max_shift > 0.0, "max_step and max_shift must be > 0 (got %g, %g)", max_step, max_shift);
    LK_REQUIRE(n_prf >= 1 && Ty >= 1 && Tx >= 1 && oversample >= 1, "need n_prf >= 1, Ty >= 1, Tx >= 1, oversample >= 1 (got %d, %d, %d, %d)",
               n_prf, Ty, Tx, oversample);
    const int64_t npix64 = (int64_t)ny * nx;
    LK_REQUIRE((int64_t)N * npix64 < (int64_t)1 << 31, "a cutout of %d x %d x %d values is too large", N, ny, nx);
    const int os = oversample, TYp = (Ty + os - 1) / os, TXp = (Tx + os - 1) / os;
    const int64_t table64 = (int64_t)os * os * TYp * TXp;
    LK_REQUIRE((int64_t)n_prf * table64 < (int64_t)1 << 30, "%d tables of %d x %d samples at oversample %d are too large", n_prf, Ty, Tx, os);
    LK_REQUIRE((int64_t)std::max(ny, nx) * os < (int64_t)1 << 30, "a %d x %d cutout at oversample %d is too large", ny, nx, os);
    for (int b = 0; prf_index_host && b < B; ++b)
        LK_REQUIRE(prf_index_host[b] >= 0 && prf_index_host[b] < n_prf, "cutout %d: prf_index %d outside 0 .. %d", b, prf_index_host[b], n_prf - 1);
    // the tile's row pitch as in psfphot.hip: 4 x an odd number; the images' and the derivatives' cadence pitch likewise, in doubles
    const int npix = (int)npix64, pitch = 4 * (((npix + 3) / 4) | 1), dpitch = 4 * (((2 * npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const auto mpitch = [&](int S) { return 4 * (((S * npix + 3) / 4) | 1); };
    const auto lds_bytes = [&](int S, int tile) {
        return (size_t)tile * ((size_t)(mpitch(S) + dpitch + S + 3) * 8 + (size_t)S * sizeof(PrfGradTaps)
                               + (size_t)pitch * 4 * (use_flux_err ? 2 : 1)) + 8 + npix;
    };
    LK_REQUIRE(lds_bytes(S_max, PRF_FIT_SHORT_TILE) <= (size_t)PSF_MAX_LDS,
               "a %d x %d cutout with %d stars needs %zu bytes of LDS for the shift fit with a table at %d cadences a tile, more than %d",
               ny, nx, S_max, lds_bytes(S_max, PRF_FIT_SHORT_TILE), PRF_FIT_SHORT_TILE, PSF_MAX_LDS);

    // the cutout's stars (no NaN coordinate) first and in order; the cutouts grouped by their star count
    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, nullptr, star_off_host, stars)) return rc;
    std::vector<int> pidx(B, 0);
    if (prf_index_host) pidx.assign(prf_index_host, prf_index_host + B);
    double *d_par;
    int *d_ints, *d_pidx;
    float *d_tp;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)stars.par.data(), stars.par.size())
                           .upload(d_ints, (const int *)stars.ints.data(), stars.ints.size())
                           .upload(d_pidx, (const int *)pidx.data(), pidx.size())
                           .buf(d_tp, (size_t)n_prf * table64)
                           .carve(stream))
        return rc;
    if (const int rc = prf_polyphase_launch(prf_table, n_prf, Ty, Tx, os, TYp, TXp, d_tp, stream)) return rc;
    PrfFitArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask;
    a.star_off = d_ints + 2 * B;
    a.par = d_par, a.u0_col = shift0_col, a.u0_row = shift0_row;
    a.tab.tp = d_tp, a.tab.index = d_pidx, a.tab.os = os, a.tab.TYp = TYp, a.tab.TXp = TXp;
    a.tab.hx = 0.5 * (Tx - 1), a.tab.hy = 0.5 * (Ty - 1);
    a.column0 = column0, a.row0 = row0, a.tol = tol, a.max_step = max_step, a.max_shift = max_shift;
    a.inv_nx = (((unsigned long long)1 << 32) + nx - 1) / nx;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.dpitch = dpitch;
    a.use_err = use_flux_err ? 1 : 0, a.max_iter = max_iter;
    a.time_out = time_out, a.flux_out = flux_out, a.err_out = flux_err_out, a.bkg = background, a.chi2 = chi2;
    a.shift_col = shift_col, a.shift_row = shift_row, a.shift_col_err = shift_col_err, a.shift_row_err = shift_row_err;
    a.last_step = last_step, a.n_iter = (int *)n_iter, a.n_used = (int *)n_used, a.cstat = cadence_status;
    for (int S = 1; S <= S_max; ++S) {
        const int count = stars.first[S + 1] - stars.first[S];
        if (!count) continue;
        a.order = d_ints + stars.first[S];
        a.mpitch = mpitch(S);
        a.tile = lds_bytes(S, PSF_T) <= (size_t)PSF_MAX_LDS ? PSF_T : PRF_FIT_SHORT_TILE;
        const size_t lds = lds_bytes(S, a.tile);
        int rc = LK_OK;
        switch (S) {
        case 1: rc = prffit_launch<1>(h, a, count, lds, stream); break;
        case 2: rc = prffit_launch<2>(h, a, count, lds, stream); break;
        case 3: rc = prffit_launch<3>(h, a, count, lds, stream); break;
        case 4: rc = prffit_launch<4>(h, a, count, lds, stream); break;
        case 5: rc = prffit_launch<5>(h, a, count, lds, stream); break;
        case 6: rc = prffit_launch<6>(h, a, count, lds, stream); break;
        case 7: rc = prffit_launch<7>(h, a, count, lds, stream); break;
        default: rc = prffit_launch<8>(h, a, count, lds, stream); break;
        }
        if (rc) return rc;
    }
    return psf_status_launch(B, N, cadence_status, status, stream);
}

}  // namespace lk
