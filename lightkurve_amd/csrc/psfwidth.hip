// psfwidth.hip — the PSF width of a cutout, fitted on resident pixel cubes on gfx950: ONE pair (sigma_col, sigma_row) per cutout,
// shared by all its cadences, by variable projection — the input that psfphot.hip and psffit.hip take as given.  The first
// kernel of the family whose non-linear unknowns are shared across cadences: the linear unknowns (S fluxes and a background per
// cadence) are projected out per cadence and the cadences' 2 x 2 Schur complements are summed over the cutout.
//
// Reference: PixelCube.psf_width (correctors/pldcorrector.py), plain float64 numpy; include/lkhip.h has the definition.
//
// One evaluation at the cutout's current v = (sigma_col, sigma_row) is two kernels; the host enqueues the pair max_iter + 1
// times with no synchronisation and no host read in between.
//   evaluate  workgroup (tile of PSF_T = 16 cadences, cutout) of ONE wavefront, PSF_LPC = 4 adjacent lanes per cadence: the
//             mapping, the staging, the LDS layout and the two walks of cube_psffit_kernel<S>, instantiated on the star count S,
//             with the derivatives by the width in the place of the derivatives by the shift.  It reads v and the phase from the
//             cutout's state record and returns at once when the cutout has stopped: a finished cutout costs one load per
//             tile.  A tile that cadence_mask leaves out entirely writes a record of +0 without reading the cube.  Per
//             cadence: g_n = D^T W r, S2_n = E - (L^-1 C)^T (L^-1 C), chi2_n; a cadence that does not contribute enters the
//             tile's sums as +0; the 16 cadences are added by a fixed __shfl_xor butterfly (psf_tile_sum) and lane 0 writes the
//             tile's record (g, H, chi2, the two counts: 64 bytes) to scratch; the cadence_status of the tile's cadences is
//             written as well.
//   step      one wavefront per cutout: adds the cutout's tile records lane-strided in index order and then by the butterfly
//             (psf_wave_sum) — an order fixed by the number of tiles alone —, factors H, applies the update rules of the
//             header, writes the trace row, advances the state (0 iterating -> 1 final evaluation pending -> 2 done) and, on
//             the final evaluation, the outputs.
//
// LDS per workgroup: cube_psffit_kernel's own count (a factor and a derivative table per cadence next to the tile).  No
// instantiation uses scratch memory (profiles/kernel_resources.md).
//
// No atomics; the order of every sum depends on N alone, so a cutout's outputs have the same bits alone, at any batch position,
// with any other cutouts in the batch and from run to run.
#include "psf_common.hpp"
#include "stage_tile.hpp"

namespace lk {

// the state of a cutout's iteration, in device memory between the kernels
struct WidthState {
    double v[2], last;     // the current (sigma_col, sigma_row); the last step taken
    int phase, n_iter, status, pad;  // phase: 0 iterating; 1 stopped and ok: the next evaluation is the final one; 2 done
};

// the sums of one tile of cadences (or, added up, of a cutout) at one evaluation
struct WidthSums {
    double g0, g1, h00, h01, h11, chi2;
    long long n_cad, n_pix;
};
static_assert(sizeof(WidthSums) == 64, "a tile record is 64 bytes");

struct WidthArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask, *cmask;  // cmask nullable: the cadences to fit on
    const int *order;             // the cutouts of this launch (one star count)
    const double *par;            // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first), then sigma0 (not read)
    const double *sh_col, *sh_row;  // nullable: the shifts
    const WidthState *state;
    double column0, row0;
    int mask_stride, S_max, N, ny, nx, pitch, use_err, chunks;
    WidthSums *tiles;  // [B][chunks]
    int8_t *cstat;
};

struct StepArgs {
    WidthState *state;
    const WidthSums *tiles;
    double tol, max_step, min_sigma, max_sigma;
    int chunks, max_iter, pass;
    double *sigma, *sigma_err, *sigma_cov, *chi2, *last_step, *trace;
    int *n_iter, *n_cad, *status;
    long long *n_pix;
};

// One run of tables (a star's len column or row factors at centre c, width sg) for cadence slot cl: val[k][cl] = (E(k + 1) -
// E(k)) / 2 and der[k][cl] = its derivative by sg, -(Q(k + 1) - Q(k)), Q(k) = (k - 1/2 - c) exp(-z_k^2) / (sqrt(2 pi) sg^2);
// every edge's erf and exp serve the two pixels it separates, as in psffit.hip's fit_table_run.
__device__ __forceinline__ void width_table_run(double *__restrict__ val, double *__restrict__ der, int len, double c, double sg) {
    constexpr double INV_SQRT_2PI = 0.3989422804014327;
    const double den = M_SQRT2 * sg, qn = INV_SQRT_2PI / (sg * sg);
    double x = -0.5 - c, z = x / den;
    double lo = psf_edge(0, c, den), qlo = x * exp(-z * z) * qn;
    for (int k = 0; k < len; ++k) {
        x = (double)(k + 1) - 0.5 - c, z = x / den;
        const double hi = psf_edge(k + 1, c, den), qhi = x * exp(-z * z) * qn;
        val[k * PSF_T] = 0.5 * (hi - lo);
        der[k * PSF_T] = qlo - qhi;
        lo = hi, qlo = qhi;
    }
}

__global__ __launch_bounds__(256) void cube_psfwidth_init_kernel(int B, int rows, const double *__restrict__ par, int PAR,
                                                                 WidthState *__restrict__ state, double *__restrict__ trace) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B * rows * 2) trace[i] = NAN;
    if (i < B) {
        WidthState s;
        s.v[0] = par[(size_t)i * PAR + PAR - 2], s.v[1] = par[(size_t)i * PAR + PAR - 1], s.last = NAN;
        s.phase = s.n_iter = s.status = s.pad = 0;
        state[i] = s;
    }
}

template <int S> __global__ __launch_bounds__(64) void cube_psfwidth_eval_kernel(const WidthArgs a) {
    constexpr int K = S + 1;
    extern __shared__ __align__(16) double width_lds[];
    const int b = a.order[blockIdx.y];
    if (a.state[b].phase == 2) return;  // the cutout has stopped: nothing of it is read or written any more
    const int c0 = blockIdx.x * PSF_T, lane = threadIdx.x, cl = lane / PSF_LPC, sub = lane % PSF_LPC;
    const int rows = min(PSF_T, a.N - c0), npix = a.ny * a.nx, nt = a.nx + a.ny;
    const bool active = cl < rows;
    double *sh_val = width_lds;                   // S x nt factors per cadence, [factor][cadence]
    double *sh_der = sh_val + S * nt * PSF_T;     // their derivatives by the width of their axis
    float *tf = reinterpret_cast<float *>(sh_der + S * nt * PSF_T);
    float *te = tf + PSF_T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + PSF_T * a.pitch : te);

    const size_t cad = (size_t)b * a.N + c0 + (active ? cl : 0), off = ((size_t)b * a.N + c0) * npix;
    const bool selected = a.cmask ? a.cmask[cad] != 0 : true;
    if (!__any(active && selected)) {  // cadence_mask leaves the whole tile out: its record is +0 and the cube is not read
        if (lane == 0) a.tiles[(size_t)b * a.chunks + blockIdx.x] = WidthSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
        if (active && sub == 0) a.cstat[cad] = 6;
        return;
    }
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = lane; i < npix; i += 64) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    const double uc = a.sh_col ? a.sh_col[cad] : 0.0, ur = a.sh_row ? a.sh_row[cad] : 0.0;
    const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
    const double v0 = a.state[b].v[0], v1 = a.state[b].v[1];

    // tables at v: the lanes of a cadence share out its 2 S runs (star, axis); they touch LDS that the staging does not
#pragma unroll 1
    for (int q = sub; q < 2 * S; q += PSF_LPC) {
        const int s = q >> 1, ax = q & 1, base = (s * nt + (ax ? a.nx : 0)) * PSF_T + cl;
        width_table_run(sh_val + base, sh_der + base, ax ? a.ny : a.nx, ax ? p[a.S_max + s] + ur - a.row0 : p[s] + uc - a.column0,
                        ax ? v1 : v0);
    }
    __syncthreads();

    const float *yrow = tf + cl * a.pitch, *erow = te + cl * a.pitch;
    int n = 0;
    for (int iy = sub; iy < a.ny; iy += PSF_LPC)
        for (int ix = 0, q = iy * a.nx; ix < a.nx; ++ix, ++q) {
            const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
            n += active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f ? 1 : 0;
        }
    n = psf_cadence_sum(n);
    int st = !selected ? 6 : !(isfinite(t) && isfinite(uc) && isfinite(ur)) ? 1 : n < S + 2 ? 2 : 0;

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
    const bool singular = psf_cholesky<K>(G, L);
    psf_solve<K>(L, rhs, theta);

    // walk 2: r = y - A theta, D = the model's derivative by (sigma_col, sigma_row); C = A^T W D, E = D^T W D, g = D^T W r, chi2
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

    // S2 = E - (L^-1 C)^T (L^-1 C)
    double s00 = e00, s01 = e01, s11 = e11;
    {
        double Y0[K], Y1[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double y0 = C0[i], y1 = C1[i];
#pragma unroll
            for (int j = 0; j < i; ++j) y0 -= L[i][j] * Y0[j], y1 -= L[i][j] * Y1[j];
            Y0[i] = y0 / L[i][i], Y1[i] = y1 / L[i][i];
            s00 -= Y0[i] * Y0[i], s01 -= Y0[i] * Y1[i], s11 -= Y1[i] * Y1[i];
        }
    }
    if (st == 0 && singular) st = 3;

    // the tile's sums: the four lanes of a cadence hold the same values, a cadence that does not contribute enters as +0
    const bool in = active && st == 0;
    WidthSums r;
    r.g0 = psf_tile_sum(in ? g0 : 0.0), r.g1 = psf_tile_sum(in ? g1 : 0.0);
    r.h00 = psf_tile_sum(in ? s00 : 0.0), r.h01 = psf_tile_sum(in ? s01 : 0.0), r.h11 = psf_tile_sum(in ? s11 : 0.0);
    r.chi2 = psf_tile_sum(in ? chi : 0.0);
    r.n_cad = psf_tile_sum(in ? 1 : 0), r.n_pix = psf_tile_sum(in ? n : 0);
    if (lane == 0) a.tiles[(size_t)b * a.chunks + blockIdx.x] = r;
    if (active && sub == 0) a.cstat[cad] = (int8_t)st;
}

__global__ __launch_bounds__(64) void cube_psfwidth_step_kernel(const StepArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    WidthState s = a.state[b];
    if (s.phase == 2) return;
    // the cutout's sums: lane-strided over its tile records in index order, then the butterfly
    const WidthSums *tile = a.tiles + (size_t)b * a.chunks;
    double g0 = 0.0, g1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0, chi = 0.0;
    long long nc = 0, np = 0;
    for (int i = lane; i < a.chunks; i += 64) {
        const WidthSums r = tile[i];
        g0 += r.g0, g1 += r.g1, h00 += r.h00, h01 += r.h01, h11 += r.h11, chi += r.chi2, nc += r.n_cad, np += r.n_pix;
    }
    g0 = psf_wave_sum(g0), g1 = psf_wave_sum(g1), h00 = psf_wave_sum(h00), h01 = psf_wave_sum(h01), h11 = psf_wave_sum(h11);
    chi = psf_wave_sum(chi), nc = psf_wave_sum(nc), np = psf_wave_sum(np);
    if (lane != 0) return;

    const int rows = a.max_iter + 1;
    double *trace = a.trace + (size_t)b * rows * 2;
    trace[2 * s.n_iter] = s.v[0], trace[2 * s.n_iter + 1] = s.v[1];  // evaluation pass is made at row n_iter = pass - 1 or less

    // H = L2 L2^T, the 2 x 2 Cholesky without pivoting
    bool singular = !(isfinite(h00) && h00 > 0.0);
    const double l00 = sqrt(h00), l10 = h01 / l00, d11 = h11 - l10 * l10;
    singular = singular || !(isfinite(d11) && d11 > PSF_PIVOT_CUT * h11);
    const double l11 = sqrt(d11);

    const bool final_eval = s.phase == 1;
    bool ok = false;
    if (nc == 0) s.status = 1, s.phase = 2;
    else if (singular) s.status = 3, s.phase = 2;
    else if (final_eval) ok = true, s.phase = 2;
    else {
        const double z0 = g0 / l00, z1 = (g1 - l10 * z0) / l11;
        double dv1 = z1 / l11, dv0 = (z0 - l10 * dv1) / l00;
        dv0 = dv0 > a.max_step ? a.max_step : dv0 < -a.max_step ? -a.max_step : dv0;
        dv1 = dv1 > a.max_step ? a.max_step : dv1 < -a.max_step ? -a.max_step : dv1;
        s.v[0] += dv0, s.v[1] += dv1, s.n_iter = a.pass;
        s.last = fabs(dv0) > fabs(dv1) ? fabs(dv0) : fabs(dv1);
        if (!(s.v[0] >= a.min_sigma && s.v[0] <= a.max_sigma && s.v[1] >= a.min_sigma && s.v[1] <= a.max_sigma)) s.status = 5, s.phase = 2;
        else if (a.tol > 0.0 && s.last < a.tol) s.phase = 1;
        else if (a.pass == a.max_iter) {
            if (a.tol > 0.0) s.status = 4, s.phase = 2;
            else s.phase = 1;
        }
    }
    a.state[b] = s;
    if (s.phase != 2) return;
    // the cutout has stopped: its outputs, NaN in the four float outputs unless this was the final evaluation of an ok cutout
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m10 = -l10 * m00 * m11;
    a.sigma[2 * b] = ok ? s.v[0] : NAN, a.sigma[2 * b + 1] = ok ? s.v[1] : NAN;
    a.sigma_err[2 * b] = ok ? sqrt(m00 * m00 + m10 * m10) : NAN, a.sigma_err[2 * b + 1] = ok ? m11 : NAN;
    a.sigma_cov[b] = ok ? m10 * m11 : NAN;
    a.chi2[b] = ok ? chi : NAN;
    a.last_step[b] = s.last;
    a.n_iter[b] = s.n_iter, a.n_cad[b] = (int)nc, a.n_pix[b] = np, a.status[b] = s.status;
}

namespace {

template <int S> int width_launch(lk_handle *h, const WidthArgs &a, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_psfwidth_eval_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_psfwidth_eval_kernel<S>, dim3(a.chunks, count), dim3(64), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_psfwidth_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                         const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                         const double *sigma0_host, const double *shift_col, const double *shift_row, const uint8_t *cadence_mask,
                         int max_iter, double tol, double max_step, double min_sigma, double max_sigma, double column0, double row0,
                         int use_flux_err, double *sigma, double *sigma_err, double *sigma_cov, double *chi2, double *last_step,
                         double *trace, int32_t *n_iter, int32_t *n_cadences, int64_t *n_pixels, int8_t *cadence_status,
                         int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && sigma0_host, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(sigma && sigma_err && sigma_cov && chi2 && last_step && trace, "NULL output buffer");
    LK_REQUIRE(n_iter && n_cadences && n_pixels && cadence_status && status, "NULL output buffer");
    LK_REQUIRE((shift_col == nullptr) == (shift_row == nullptr), "shift_col and shift_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
    LK_REQUIRE(max_iter >= 1 && max_iter <= 64, "max_iter must be 1 .. 64 (got %d)", max_iter);
    LK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "tol must be finite and >= 0 (got %g)", tol);
    LK_REQUIRE(max_step > 0.0, "max_step must be > 0 (got %g)", max_step);
    LK_REQUIRE(std::isfinite(min_sigma) && std::isfinite(max_sigma) && min_sigma > 0.0,
               "min_sigma and max_sigma must be finite, min_sigma > 0 (got %g, %g)", min_sigma, max_sigma);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 2; ++k) {
            const double s0 = sigma0_host[2 * (size_t)b + k];
            LK_REQUIRE(s0 >= min_sigma && s0 <= max_sigma, "cutout %d: need min_sigma <= sigma0 <= max_sigma (got %g, %g, %g)", b,
                       min_sigma, s0, max_sigma);
        }
    const int64_t npix64 = (int64_t)ny * nx;
    LK_REQUIRE((int64_t)N * npix64 < (int64_t)1 << 31, "a cutout of %d x %d x %d values is too large", N, ny, nx);
    // the tile's row pitch as in psfphot.hip: 4 x an odd number
    const int npix = (int)npix64, nt = nx + ny, pitch = 4 * (((npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const size_t tile_bytes = (size_t)PSF_T * pitch * 4 * (use_flux_err ? 2 : 1) + npix;
    const auto lds_bytes = [&](int S) { return (size_t)2 * S * nt * 8 * PSF_T + tile_bytes; };  // factors and derivatives
    LK_REQUIRE(lds_bytes(S_max) <= (size_t)PSF_MAX_LDS, "a %d x %d cutout with %d stars needs %zu bytes of LDS for the width fit, more than %d",
               ny, nx, S_max, lds_bytes(S_max), PSF_MAX_LDS);

    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, sigma0_host, nullptr, stars)) return rc;
    const int chunks = (N + PSF_T - 1) / PSF_T;
    double *d_par;
    int *d_ints;
    WidthState *d_state;
    WidthSums *d_tiles;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)stars.par.data(), stars.par.size())
                           .upload(d_ints, (const int *)stars.ints.data(), stars.ints.size())
                           .buf(d_state, (size_t)B)
                           .buf(d_tiles, (size_t)B * chunks)
                           .carve(stream))
        return rc;
    const int PAR = 2 * S_max + 2, cells = B * (max_iter + 1) * 2;  // cells >= B
    hipLaunchKernelGGL(cube_psfwidth_init_kernel, dim3((cells + 255) / 256), dim3(256), 0, stream, B, max_iter + 1, (const double *)d_par,
                       PAR, d_state, trace);
    LK_HIP_CHECK(hipGetLastError());

    WidthArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask, a.cmask = cadence_mask;
    a.par = d_par, a.sh_col = shift_col, a.sh_row = shift_row, a.state = d_state;
    a.column0 = column0, a.row0 = row0;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.use_err = use_flux_err ? 1 : 0;
    a.chunks = chunks, a.tiles = d_tiles, a.cstat = cadence_status;
    StepArgs s;
    s.state = d_state, s.tiles = d_tiles;
    s.tol = tol, s.max_step = max_step, s.min_sigma = min_sigma, s.max_sigma = max_sigma;
    s.chunks = chunks, s.max_iter = max_iter;
    s.sigma = sigma, s.sigma_err = sigma_err, s.sigma_cov = sigma_cov, s.chi2 = chi2, s.last_step = last_step, s.trace = trace;
    s.n_iter = (int *)n_iter, s.n_cad = (int *)n_cadences, s.status = (int *)status, s.n_pix = (long long *)n_pixels;
    // pass = the iteration number of every cutout that still iterates; pass max_iter + 1 can only be a final evaluation
    for (int pass = 1; pass <= max_iter + 1; ++pass) {
        for (int S = 1; S <= S_max; ++S) {
            const int count = stars.first[S + 1] - stars.first[S];
            if (!count) continue;
            a.order = d_ints + stars.first[S];
            int rc = LK_OK;
            switch (S) {
            case 1: rc = width_launch<1>(h, a, count, lds_bytes(S), stream); break;
            case 2: rc = width_launch<2>(h, a, count, lds_bytes(S), stream); break;
            case 3: rc = width_launch<3>(h, a, count, lds_bytes(S), stream); break;
            case 4: rc = width_launch<4>(h, a, count, lds_bytes(S), stream); break;
            case 5: rc = width_launch<5>(h, a, count, lds_bytes(S), stream); break;
            case 6: rc = width_launch<6>(h, a, count, lds_bytes(S), stream); break;
            case 7: rc = width_launch<7>(h, a, count, lds_bytes(S), stream); break;
            default: rc = width_launch<8>(h, a, count, lds_bytes(S), stream); break;
            }
            if (rc) return rc;
        }
        s.pass = pass;
        hipLaunchKernelGGL(cube_psfwidth_step_kernel, dim3(B), dim3(64), 0, stream, s);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

}  // namespace lk
