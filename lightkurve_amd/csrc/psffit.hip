// psffit.hip — PSF photometry that fits each cadence's pointing shift, on resident pixel cubes on gfx950: per cadence the fluxes
// of up to 8 stars, a constant background AND one common (column, row) shift of all stars, by variable projection — the
// non-linear piece that psfphot.hip (fluxes at given shifts) leaves to its caller.
//
// Reference: PixelCube.psf_fit (correctors/pldcorrector.py), plain float64 numpy; include/lkhip.h has the definition.
//
//   fit      workgroup (tile of PSF_T = 16 cadences, cutout) of ONE wavefront, PSF_LPC = 4 adjacent lanes per cadence: the mapping
//            of cube_psfphot_kernel<S>, instantiated on the star count S.  The tile of flux and flux_err and the mask are staged
//            in LDS once; every evaluation after that reads LDS alone, so the cube is read from HBM once however many
//            iterations run.  One evaluation at the cadence's current shift u:
//              tables  the four lanes of a cadence share out its 2 S runs (star, axis) and rebuild the factor table AND the
//                      derivative table in LDS ([factor][cadence]); every edge's erf and exp serve the two pixels it separates;
//              walk 1  lane k takes the pixel rows k, k + 4, ... in index order: G = A^T W A (upper triangle) and A^T W y in
//                      registers; the four partial sums meet in the fixed butterfly; every lane factors G (Cholesky without
//                      pivoting) and solves for theta;
//              walk 2  the same rows again with theta and L live: C = A^T W D (K x 2), E = D^T W D, g = D^T W r and chi2, D the
//                      derivative of the model by the shift; butterfly; Y = L^-1 C, S2 = E - Y^T Y (the Schur complement, not a
//                      (K + 2)^2 matrix), its 2 x 2 Cholesky and du = S2^-1 g.
//            The loop over evaluations is wave-uniform and ends when every cadence of the tile is done.  A cadence that has
//            stopped with status 0 takes one more evaluation at its final u, which writes its outputs (the values of
//            psf_photometry at shifts = u, and the shift errors from S2); after that, and for a cadence that stopped with another
//            status, the evaluations of the tile go on without touching its u, n_iter or last_step.
//   status   psfphot.hip's status kernel: 1 when no cadence is ok.
//
// Tile and lanes.  LDS per workgroup = 16 cadences x (8 pitch bytes of flux and flux_err + 16 S (nx + ny) bytes of tables, twice
// the shifted psf_photometry kernel's): 38.5 KB at 11 x 11 with 4 stars, so four wavefronts fit a CU, one per SIMD, where the
// shifted psf_photometry kernel has five.  Eight lanes per cadence would halve the tile (19.3 KB, eight wavefronts) at the price
// of every lane repeating the solve (the Cholesky, three substitutions and the Schur complement: about a sixth of an
// evaluation's instructions at S = 4, so 1.16 x the instructions for 2 x the wavefronts to hide the LDS and the division latency
// behind).  Measured at 500 x 4000 x 11 x 11, S = 4, true shifts of +-0.3 px (wall of the whole call, the library built with
// PSF_LPC = 8 aside): 4 lanes 19.55 ms, 8 lanes 26.44 ms — here the repeated solves cost more than the occupancy gains, unlike
// the shifted psf_photometry kernel (3.49 / 3.07 ms in the same two runs).  Four lanes are kept.  Of the 19.55 ms, 18.5 ms are
// this kernel, 5.00 evaluations per tile (a tile waits for its slowest cadence; 3.88 steps per cadence on
// average) — 3.7 ms per evaluation of the batch against 3.25 ms for the whole shifted psf_photometry kernel
// (profiles/psffit_walls.txt, profiles/psffit_kernel_stats.txt).
//
// Registers: L, theta and C are live in walk 2 next to the constants of erf and exp, which the compiler hoists out of the
// iteration loop.  No instantiation uses scratch; S >= 4 lives partly in AGPRs, and at S = 5 .. 8 the compiler reports 6 VGPR
// spills into AGPRs (profiles/kernel_resources.md).  A table builder that is not inlined keeps the constants out of the loop but
// its call frame costs 8 bytes of scratch per lane, so it is inlined.
//
// No atomics; the order of every sum depends on the cutout's own data alone, so a cutout's outputs have the same bits alone,
// at any batch position and from run to run.
#include "psf_common.hpp"
#include "stage_tile.hpp"

namespace lk {

struct FitArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask;
    const int *order, *star_off;  // order: the cutouts of this launch (one star count)
    const double *par;            // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first), sigma_col, sigma_row
    const double *u0_col, *u0_row;  // nullable: the initial shifts
    double column0, row0, tol, max_step, max_shift;
    int mask_stride, S_max, N, ny, nx, pitch, use_err, max_iter;
    double *time_out, *flux_out, *err_out, *bkg, *chi2;  // time_out nullable
    double *shift_col, *shift_row, *shift_col_err, *shift_row_err, *last_step;
    int *n_used, *n_iter;
    int8_t *cstat;
};

template <int S> __global__ __launch_bounds__(64) void cube_psffit_kernel(const FitArgs a) {
    constexpr int K = S + 1;
    extern __shared__ __align__(16) double fit_lds[];
    const int b = a.order[blockIdx.y], c0 = blockIdx.x * PSF_T, lane = threadIdx.x, cl = lane / PSF_LPC, sub = lane % PSF_LPC;
    const int rows = min(PSF_T, a.N - c0), npix = a.ny * a.nx, nt = a.nx + a.ny;
    const bool active = cl < rows;
    double *sh_val = fit_lds;                     // S x nt factors per cadence, [factor][cadence]
    double *sh_der = sh_val + S * nt * PSF_T;     // their derivatives by the star's centre
    float *tf = reinterpret_cast<float *>(sh_der + S * nt * PSF_T);
    float *te = tf + PSF_T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + PSF_T * a.pitch : te);

    const size_t cad = (size_t)b * a.N + c0 + (active ? cl : 0), off = ((size_t)b * a.N + c0) * npix;
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = lane; i < npix; i += 64) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    const double u0c = a.u0_col ? a.u0_col[cad] : 0.0, u0r = a.u0_row ? a.u0_row[cad] : 0.0;
    const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
    __syncthreads();

    // the used pixels do not depend on the shift: counted once
    const float *yrow = tf + cl * a.pitch, *erow = te + cl * a.pitch;
    int n = 0;
    for (int iy = sub; iy < a.ny; iy += PSF_LPC)
        for (int ix = 0, q = iy * a.nx; ix < a.nx; ++ix, ++q) {
            const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
            n += active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f ? 1 : 0;
        }
    n = psf_cadence_sum(n);

    int st = !(isfinite(t) && isfinite(u0c) && isfinite(u0r)) ? 1 : n < S + 4 ? 2 : 0;
    int phase = !active || st ? 2 : 0;  // 0 iterating; 1 stopped and ok: the next evaluation writes the outputs; 2 done
    int nit = 0;
    double uc = u0c, ur = u0r, last = NAN;

    // pass = the iteration number of every cadence that still iterates (they all start at pass 1); at most max_iter + 1 passes
    for (int pass = 1; pass <= a.max_iter + 1 && __any(phase != 2); ++pass) {
        __syncthreads();  // the walks of the pass before have read the tables
        // tables at u: the lanes of a cadence share out its 2 S runs (star, axis)
#pragma unroll 1
        for (int q = sub; q < 2 * S; q += PSF_LPC) {
            const int s = q >> 1, ax = q & 1, base = (s * nt + (ax ? a.nx : 0)) * PSF_T + cl;
            fit_table_run(sh_val + base, sh_der + base, ax ? a.ny : a.nx, ax ? p[a.S_max + s] + ur - a.row0 : p[s] + uc - a.column0,
                          p[2 * a.S_max + ax]);
        }
        __syncthreads();

        // walk 1: G[i][j], i <= j, and rhs over this lane's pixel rows, in index order; column S of the design is the constant
        double G[K][K], rhs[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            rhs[i] = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) G[i][j] = 0.0;
        }
        for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
            int q = iy * a.nx;
            double gr[S];
#pragma unroll
            for (int s = 0; s < S; ++s) gr[s] = sh_val[(s * nt + a.nx + iy) * PSF_T + cl];
            // no branch on the pixel: one that is not used enters with w = 0 and y = 0
#pragma unroll 2
            for (int ix = 0; ix < a.nx; ++ix, ++q) {
                const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                const bool used = active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                double av[K];
#pragma unroll
                for (int s = 0; s < S; ++s) av[s] = sh_val[(s * nt + ix) * PSF_T + cl] * gr[s];
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
        double L[K][K], theta[K];
        bool singular = psf_cholesky<K>(G, L);
        psf_solve<K>(L, rhs, theta);

        // walk 2: r = y - A theta, D = the model's derivative by (dc, dr); C = A^T W D, E = D^T W D, g = D^T W r, chi2
        double C0[K], C1[K], e00 = 0.0, e01 = 0.0, e11 = 0.0, g0 = 0.0, g1 = 0.0, chi = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) C0[i] = C1[i] = 0.0;
        for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
            int q = iy * a.nx;
            double gr[S], tg[S], td[S];  // the row factor; theta_s x the row factor; theta_s x the row derivative
#pragma unroll
            for (int s = 0; s < S; ++s) {
                gr[s] = sh_val[(s * nt + a.nx + iy) * PSF_T + cl];
                tg[s] = theta[s] * gr[s];
                td[s] = theta[s] * sh_der[(s * nt + a.nx + iy) * PSF_T + cl];
            }
#pragma unroll 2
            for (int ix = 0; ix < a.nx; ++ix, ++q) {
                const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                const bool used = active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                double av[K], m = theta[S], d0 = 0.0, d1 = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const double gc = sh_val[(s * nt + ix) * PSF_T + cl];
                    av[s] = gc * gr[s];
                    m += theta[s] * av[s];
                    d0 += tg[s] * sh_der[(s * nt + ix) * PSF_T + cl];
                    d1 += td[s] * gc;
                }
                av[S] = 1.0;
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

template <int S> int fit_launch(lk_handle *h, const FitArgs &a, int chunks, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_psffit_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_psffit_kernel<S>, dim3(chunks, count), dim3(64), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_psffit_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const double *sigma_host, const double *shift0_col, const double *shift0_row, int max_iter, double tol,
                       double max_step, double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off_host,
                       double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2, double *shift_col,
                       double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step, int32_t *n_iter,
                       int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && sigma_host, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(flux_out && flux_err_out && background && chi2 && n_used && cadence_status && status, "NULL output buffer");
    LK_REQUIRE(shift_col && shift_row && shift_col_err && shift_row_err && last_step && n_iter, "NULL output buffer");
    LK_REQUIRE((shift0_col == nullptr) == (shift0_row == nullptr), "shift0_col and shift0_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
    LK_REQUIRE(max_iter >= 1 && max_iter <= 64, "max_iter must be 1 .. 64 (got %d)", max_iter);
    LK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "tol must be finite and >= 0 (got %g)", tol);
    LK_REQUIRE(max_step > 0.0 && max_shift > 0.0, "max_step and max_shift must be > 0 (got %g, %g)", max_step, max_shift);
    const int64_t npix64 = (int64_t)ny * nx;
    LK_REQUIRE((int64_t)N * npix64 < (int64_t)1 << 31, "a cutout of %d x %d x %d values is too large", N, ny, nx);
    // the tile's row pitch as in psfphot.hip: 4 x an odd number
    const int npix = (int)npix64, nt = nx + ny, pitch = 4 * (((npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const size_t tile_bytes = (size_t)PSF_T * pitch * 4 * (use_flux_err ? 2 : 1) + npix;
    const auto lds_bytes = [&](int S) { return (size_t)2 * S * nt * 8 * PSF_T + tile_bytes; };  // factors and derivatives
    LK_REQUIRE(lds_bytes(S_max) <= (size_t)PSF_MAX_LDS, "a %d x %d cutout with %d stars needs %zu bytes of LDS for the shift fit, more than %d",
               ny, nx, S_max, lds_bytes(S_max), PSF_MAX_LDS);

    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, sigma_host, star_off_host, stars)) return rc;
    double *d_par;
    int *d_ints;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)stars.par.data(), stars.par.size())
                           .upload(d_ints, (const int *)stars.ints.data(), stars.ints.size())
                           .carve(stream))
        return rc;
    FitArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask;
    a.star_off = d_ints + 2 * B;
    a.par = d_par, a.u0_col = shift0_col, a.u0_row = shift0_row;
    a.column0 = column0, a.row0 = row0, a.tol = tol, a.max_step = max_step, a.max_shift = max_shift;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.use_err = use_flux_err ? 1 : 0;
    a.max_iter = max_iter;
    a.time_out = time_out, a.flux_out = flux_out, a.err_out = flux_err_out, a.bkg = background, a.chi2 = chi2;
    a.shift_col = shift_col, a.shift_row = shift_row, a.shift_col_err = shift_col_err, a.shift_row_err = shift_row_err;
    a.last_step = last_step, a.n_iter = (int *)n_iter, a.n_used = (int *)n_used, a.cstat = cadence_status;
    const int chunks = (N + PSF_T - 1) / PSF_T;
    for (int S = 1; S <= S_max; ++S) {
        const int count = stars.first[S + 1] - stars.first[S];
        if (!count) continue;
        a.order = d_ints + stars.first[S];
        int rc = LK_OK;
        switch (S) {
        case 1: rc = fit_launch<1>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 2: rc = fit_launch<2>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 3: rc = fit_launch<3>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 4: rc = fit_launch<4>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 5: rc = fit_launch<5>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 6: rc = fit_launch<6>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 7: rc = fit_launch<7>(h, a, chunks, count, lds_bytes(S), stream); break;
        default: rc = fit_launch<8>(h, a, chunks, count, lds_bytes(S), stream); break;
        }
        if (rc) return rc;
    }
    return psf_status_launch(B, N, cadence_status, status, stream);
}

}  // namespace lk
