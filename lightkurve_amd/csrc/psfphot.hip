// psfphot.hip — deblended PSF photometry per cadence of resident pixel cubes on gfx950: the fluxes of up to 8 stars at known
// positions and a constant background, by weighted linear least squares on every cadence's image (which of the blended stars
// has the transit?).
//
// Reference: PixelCube.psf_photometry (correctors/pldcorrector.py), plain float64 numpy; include/lkhip.h has the definition.
//
//   tables   (calls without shifts) one workgroup per cutout: the nx column and ny row factors of every star, the
//            pixel-integrated Gaussian being separable — 2 erf per factor, once per cutout.
//   fit      workgroup (tile of PSF_T = 16 cadences, cutout) of ONE wavefront, PSF_LPC = 4 adjacent lanes per cadence.  The tile
//            of flux and flux_err (contiguous in memory) is staged in LDS with 16-byte loads; its row pitch is 4 x an odd
//            number, so the 8 cadences x 4 pixel rows of a ds_read_b32 half fall on different banks for an odd nx.  With shifts
//            the four lanes of a cadence form its factor tables in LDS ([factor][cadence]), (star, axis) runs each; without, the
//            cutout's tables are read from the tables kernel's scratch.  Lane k of a cadence walks the pixel rows k, k + 4, ...
//            in index order and keeps G = A^T W A (upper triangle), A^T W y and the count in registers (the kernel is
//            instantiated on the star count S); the four partial sums meet in a fixed two-step butterfly that leaves the same
//            bits in all four lanes, every lane factors G by Cholesky without pivoting, solves, inverts the factor for the
//            variances, and the lanes walk the SAME tile again for chi2: the cube is read from HBM once.
//   status   one workgroup per cutout: 1 when no cadence is ok.
//
// Why four lanes per cadence: the tile a wavefront must hold is what bounds the occupancy.  With one lane per cadence (64
// cadences, 62 KB at 11 x 11) two wavefronts fit a CU and half its SIMDs idle; with four, a wavefront holds 16.3 KB and nine fit.
// Measured at 500 x 4000 x 11 x 11, S = 4 (wall of the whole call, without / with shifts): 1 lane 5.55 / 11.9 ms, 2 lanes 3.83 /
// 8.69 ms, 4 lanes 2.61 / 4.89 ms, 8 lanes 2.69 / 4.21 ms (every lane of a cadence repeats the solve).  The other mapping of
// the pixels — one wavefront per cadence — needs a 6-step tree for each of the (S + 1)(S + 2) / 2 + S + 1 sums of every cadence
// (about 360 cross-lane operations for S = 4 against the 50 multiply-adds of two pixels per lane); it was not built.
//
// No atomics; the order of every sum depends on the cutout's own data alone, so a cutout's outputs have the same bits alone,
// at any batch position and from run to run.
#include "psf_common.hpp"  // the lane mapping, psf_edge, the cadence sum, the Cholesky and the star grouping, shared with psffit.hip
#include "stage_tile.hpp"

namespace lk {

namespace {

// factor k of star s of a cutout (p: its row of par): k < nx the column factor of pixel column k, else the row factor of pixel
// row k - nx, with the star moved by (dc, dr)
__device__ __forceinline__ double psf_factor(const double *__restrict__ p, int S_max, int s, int k, int nx, double dc, double dr,
                                             double column0, double row0) {
    const bool col = k < nx;
    const double c = col ? p[s] + dc - column0 : p[S_max + s] + dr - row0, den = M_SQRT2 * p[2 * S_max + (col ? 0 : 1)];
    const int e = col ? k : k - nx;
    return 0.5 * (psf_edge(e + 1, c, den) - psf_edge(e, c, den));
}

}  // namespace

struct PsfArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask;
    const int *order, *star_off;  // order: the cutouts of this launch (one star count)
    const double *par;        // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first), sigma_col, sigma_row
    const double *tab;        // [B][S_max][nx + ny]: the factor tables of the cutouts (no shifts)
    const double *shift_col, *shift_row;
    double column0, row0;
    int mask_stride, S_max, N, ny, nx, pitch, use_err;
    double *time_out, *flux_out, *err_out, *bkg, *chi2;  // time_out nullable
    int *n_used;
    int8_t *cstat;
};

// tab[b][s][0 .. nx) = the column factors of star s, [nx .. nx + ny) its row factors; thread = one factor
__global__ __launch_bounds__(64) void cube_psfphot_tables_kernel(const double *__restrict__ par, const int *__restrict__ n_stars,
                                                                    int S_max, int ny, int nx, double column0, double row0,
                                                                    double *__restrict__ tab) {
    const int b = blockIdx.x, nt = nx + ny;
    const double *p = par + (size_t)b * (2 * S_max + 2);
    for (int i = threadIdx.x; i < n_stars[b] * nt; i += 64)
        tab[(size_t)b * S_max * nt + i] = psf_factor(p, S_max, i / nt, i % nt, nx, 0.0, 0.0, column0, row0);
}

template <int S> __global__ __launch_bounds__(64) void cube_psfphot_kernel(const PsfArgs a) {
    constexpr int K = S + 1;
    extern __shared__ __align__(16) double psf_lds[];
    const int b = a.order[blockIdx.y], c0 = blockIdx.x * PSF_T, lane = threadIdx.x, cl = lane / PSF_LPC, sub = lane % PSF_LPC;
    const int rows = min(PSF_T, a.N - c0), npix = a.ny * a.nx, nt = a.nx + a.ny;
    const bool shifted = a.shift_col != nullptr, active = cl < rows;
    const int tstride = shifted ? PSF_T : 1, toff = shifted ? cl : 0;
    double *sh_tab = psf_lds;                                               // S x nt factors, per cadence with shifts
    float *tf = reinterpret_cast<float *>(sh_tab + S * nt * tstride);
    float *te = tf + PSF_T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + PSF_T * a.pitch : te);

    const size_t cad = (size_t)b * a.N + c0 + (active ? cl : 0), off = ((size_t)b * a.N + c0) * npix;
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = lane; i < npix; i += 64) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    bool fin = isfinite(t);
    if (shifted) {
        const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
        const double dc = a.shift_col[cad], dr = a.shift_row[cad];
        fin = fin && isfinite(dc) && isfinite(dr);
        // the lanes of a cadence share out its 2 S runs of factors (star, axis); along a run every edge's erf serves the two
        // pixels it separates: n + 1 evaluations for n factors, the values of psf_factor
#pragma unroll 1
        for (int q = sub; q < 2 * S; q += PSF_LPC) {
            const int s = q >> 1, n = (q & 1) ? a.ny : a.nx, base = s * nt + ((q & 1) ? a.nx : 0);
            const double c = (q & 1) ? p[a.S_max + s] + dr - a.row0 : p[s] + dc - a.column0, den = M_SQRT2 * p[2 * a.S_max + (q & 1)];
            double lo = psf_edge(0, c, den);
            for (int k = 0; k < n; ++k) {
                const double hi = psf_edge(k + 1, c, den);
                sh_tab[(base + k) * PSF_T + cl] = 0.5 * (hi - lo);
                lo = hi;
            }
        }
    } else {
        for (int i = lane; i < S * nt; i += 64) sh_tab[i] = a.tab[(size_t)b * a.S_max * nt + i];
    }
    __syncthreads();

    // the sums over this lane's pixel rows, in index order: G[i][j], i <= j, and rhs; column S of the design is the constant
    const float *yrow = tf + cl * a.pitch, *erow = te + cl * a.pitch;
    int n = 0;
    double G[K][K], rhs[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        rhs[i] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) G[i][j] = 0.0;
    }
    for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
        int p = iy * a.nx;
        double gr[S];
#pragma unroll
        for (int s = 0; s < S; ++s) gr[s] = sh_tab[(s * nt + a.nx + iy) * tstride + toff];
        // no branch on the pixel: one that is not used enters with w = 0 and y = 0, which leaves every sum's bits as they are
        // (the factors are >= 0, so the products are +0), and the loads of the next pixels need not wait for this one's test
#pragma unroll 2
        for (int ix = 0; ix < a.nx; ++ix, ++p) {
            const float yf = yrow[p], ef = a.use_err ? erow[p] : 1.0f;
            const bool used = active && sm[p] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
            const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
            double av[K];
#pragma unroll
            for (int s = 0; s < S; ++s) av[s] = sh_tab[(s * nt + ix) * tstride + toff] * gr[s];
            av[S] = 1.0;
            n += used ? 1 : 0;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const double wa = w * av[i];
                rhs[i] += wa * y;
#pragma unroll
                for (int j = i; j < K; ++j) G[i][j] += wa * av[j];
            }
        }
    }

    n = psf_cadence_sum(n);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        rhs[i] = psf_cadence_sum(rhs[i]);
#pragma unroll
        for (int j = i; j < K; ++j) G[i][j] = psf_cadence_sum(G[i][j]);
    }

    // every lane of the cadence: G = L L^T in index order, no pivoting; solve; (G^-1)_kk for the variances
    double L[K][K], theta[K], var[K];
    const bool singular = psf_cholesky<K>(G, L);
    psf_solve<K>(L, rhs, theta);
    psf_variances<K>(L, var);
    const int st = !fin ? 1 : n < S + 2 ? 2 : singular ? 3 : 0;

    // chi2 from the residuals, over the tile the lanes have just walked (st is the same in the lanes of a cadence)
    double chi = 0.0;
    if (st == 0) {
        for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
            int p = iy * a.nx;
            double gr[S];
#pragma unroll
            for (int s = 0; s < S; ++s) gr[s] = sh_tab[(s * nt + a.nx + iy) * tstride + toff];
#pragma unroll 2
            for (int ix = 0; ix < a.nx; ++ix, ++p) {
                const float yf = yrow[p], ef = a.use_err ? erow[p] : 1.0f;
                const bool used = sm[p] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                const double w = a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                double m = theta[S];
#pragma unroll
                for (int s = 0; s < S; ++s) m += theta[s] * (sh_tab[(s * nt + ix) * tstride + toff] * gr[s]);
                const double res = (double)yf - m;
                chi += used ? w * (res * res) : 0.0;
            }
        }
    }
    chi = psf_cadence_sum(chi);
    if (!active || sub != 0) return;
    const bool ok = st == 0;
    const size_t row0 = (size_t)a.star_off[b];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const size_t o = (row0 + s) * a.N + c0 + cl;
        if (a.time_out) a.time_out[o] = t;
        a.flux_out[o] = ok ? theta[s] : NAN;
        a.err_out[o] = ok ? sqrt(var[s]) : NAN;
    }
    a.bkg[cad] = ok ? theta[S] : NAN;
    a.chi2[cad] = ok ? chi : NAN;
    a.n_used[cad] = n;
    a.cstat[cad] = (int8_t)st;
}

// status[b] = 0 when a cadence of the cutout is ok, else 1
__global__ __launch_bounds__(256) void cube_psfphot_status_kernel(const int8_t *__restrict__ cstat, int N, int *__restrict__ status) {
    const int b = blockIdx.x;
    int any = 0;
    for (int i = threadIdx.x; i < N; i += 256) any |= cstat[(size_t)b * N + i] == 0 ? 1 : 0;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) status[b] = any ? 0 : 1;
}

int psf_status_launch(int B, int N, const int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    hipLaunchKernelGGL(cube_psfphot_status_kernel, dim3(B), dim3(256), 0, stream, cadence_status, N, (int *)status);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

namespace {

template <int S> int psf_launch(lk_handle *h, const PsfArgs &a, int chunks, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_psfphot_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_psfphot_kernel<S>, dim3(chunks, count), dim3(64), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_psfphot_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                        const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                        const double *sigma_host, const double *shift_col, const double *shift_row, double column0, double row0,
                        int use_flux_err, int32_t *star_off_host, double *time_out, double *flux_out, double *flux_err_out, double *background,
                        double *chi2, int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && sigma_host, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(flux_out && flux_err_out && background && chi2 && n_used && cadence_status && status, "NULL output buffer");
    LK_REQUIRE((shift_col == nullptr) == (shift_row == nullptr), "shift_col and shift_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
    const int64_t npix64 = (int64_t)ny * nx;
    LK_REQUIRE((int64_t)N * npix64 < (int64_t)1 << 31, "a cutout of %d x %d x %d values is too large", N, ny, nx);
    // row pitch of the tile: 4 x an odd number, so the 8 cadences x 4 pixel rows of a ds_read_b32 half spread over the banks
    const int npix = (int)npix64, nt = nx + ny, pitch = 4 * (((npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const bool shifted = shift_col != nullptr;
    const size_t tile_bytes = (size_t)PSF_T * pitch * 4 * (use_flux_err ? 2 : 1) + npix;
    const auto lds_bytes = [&](int S) { return (size_t)S * nt * 8 * (shifted ? PSF_T : 1) + tile_bytes; };
    LK_REQUIRE(lds_bytes(S_max) <= (size_t)PSF_MAX_LDS, "a %d x %d cutout with %d stars%s needs %zu bytes of LDS, more than %d", ny, nx,
               S_max, shifted ? " and shifts" : "", lds_bytes(S_max), PSF_MAX_LDS);

    // the cutout's stars (no NaN coordinate) first and in order; the cutouts grouped by their star count
    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, sigma_host, star_off_host, stars)) return rc;
    const std::vector<double> &par = stars.par;
    const std::vector<int> &ints = stars.ints;
    const int *first = stars.first;

    double *d_par, *d_tab;
    int *d_ints;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)par.data(), par.size())
                           .upload(d_ints, (const int *)ints.data(), ints.size())
                           .buf(d_tab, (size_t)B * S_max * nt, !shifted)
                           .carve(stream))
        return rc;
    if (!shifted) {
        hipLaunchKernelGGL(cube_psfphot_tables_kernel, dim3(B), dim3(64), 0, stream, (const double *)d_par,
                           (const int *)(d_ints + B), S_max, ny, nx, column0, row0, d_tab);
        LK_HIP_CHECK(hipGetLastError());
    }
    PsfArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask;
    a.star_off = d_ints + 2 * B;
    a.par = d_par, a.tab = d_tab, a.shift_col = shift_col, a.shift_row = shift_row;
    a.column0 = column0, a.row0 = row0;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.use_err = use_flux_err ? 1 : 0;
    a.time_out = time_out, a.flux_out = flux_out, a.err_out = flux_err_out, a.bkg = background, a.chi2 = chi2;
    a.n_used = (int *)n_used, a.cstat = cadence_status;
    const int chunks = (N + PSF_T - 1) / PSF_T;
    for (int S = 1; S <= S_max; ++S) {
        const int count = first[S + 1] - first[S];
        if (!count) continue;
        a.order = d_ints + first[S];
        int rc = LK_OK;
        switch (S) {
        case 1: rc = psf_launch<1>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 2: rc = psf_launch<2>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 3: rc = psf_launch<3>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 4: rc = psf_launch<4>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 5: rc = psf_launch<5>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 6: rc = psf_launch<6>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 7: rc = psf_launch<7>(h, a, chunks, count, lds_bytes(S), stream); break;
        default: rc = psf_launch<8>(h, a, chunks, count, lds_bytes(S), stream); break;
        }
        if (rc) return rc;
    }
    return psf_status_launch(B, N, cadence_status, status, stream);
}

}  // namespace lk
