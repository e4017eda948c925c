// prfphot.hip — deblended PSF photometry per cadence of resident pixel cubes on gfx950 with a TABULATED PRF: psfphot.hip's linear
// fit (the fluxes of up to 8 stars at known positions and a constant background, weighted least squares on every cadence's image)
// with the model taken from a super-sampled table by Keys' cubic convolution instead of a Gaussian's erf.
//
// Reference: TabulatedPRF.evaluate and PixelCube.psf_photometry(prf=) (correctors/pldcorrector.py), plain float64 numpy;
// include/lkhip.h has the definition.
//
//   polyphase  once per call: Tp[table][py][px][Y][X] = T[table][Y os + py][X os + px], zero where the source is outside the
//              table.  The oversampling is an integer, so all pixels of a cutout share the fractional parts (f, g) of a (star,
//              cadence) and pixel (iy, ix) reads the taps (j0 - 1 + jj + iy os, i0 - 1 + ii + ix os): in the natural layout 16
//              gathers at a stride of os samples, in this one each of the 16 taps of a cutout's pixels is one contiguous
//              sub-image of at most TYp x TXp floats (576 bytes for a 551 x 551 table at os = 50) that neighbouring lanes read
//              together.
//   images     (calls without shifts) one workgroup per cutout: the model image of every star, the same at all cadences, as
//              [B][S_max][npix] doubles.
//   fit        psfphot.hip's workgroup — a tile of PSF_T = 16 cadences of one cutout, ONE wavefront, PSF_LPC = 4 adjacent lanes per
//              cadence, the tile of flux and flux_err staged in LDS with 16-byte loads — and its walk, solve and second walk, with
//              av[s] = the model image of star s read from LDS.  Without shifts the cutout's S images are copied from the images
//              kernel's scratch.  With shifts they differ per cadence (500 x 4000 x 4 x 121 doubles are 7.7 GB: not through HBM)
//              and are formed here: the threads first share out the tile's 16 S (cadence, star) pairs and leave each pair's taps —
//              8 weights, and per tap the phase's offset and the first sub-image index — in LDS; then every wavefront of the
//              workgroup (PRF_FORM_THREADS = 512: eight) takes pairs in turn, lane = pixel, 16 loads without a branch and 20
//              multiply-adds per value, and parks the images in LDS ([cadence][star][pixel], the cadence pitch 4 x an odd number
//              of doubles so that the 8 cadences x 4 pixel rows of a ds_read_b64 half fall on different banks for an odd nx) for
//              both walks; after the barrier wavefront 0 fits and the others leave.
//   status     psfphot.hip's status kernel: 1 when no cadence is ok.
//
// Measured at 500 x 4000 x 11 x 11, S = 4, a 551 x 551 table at os = 50 (wall of the whole call with shifts; without them 2.4 to
// 2.7 ms in every form): one wavefront forming pair after pair, each tap's load under its own branch, 131.2 ms — bound by latency,
// 86 KB of LDS admit one workgroup per CU; there the table's natural layout gave 123.3 ms, and forming every value in the first walk
// and again in the second (nothing parked, 24 KB of LDS) 59.5 ms.  With the loads free of branches and batched, images parked: 4
// forming wavefronts 17.97 ms, 8 wavefronts 17.11 ms (kept), 16 wavefronts 16.72 ms (spills from 6 stars on); 8 wavefronts on the
// natural layout 21.55 ms, so the polyphase copy pays 1.26 x.  The walk's arithmetic is psfphot.hip's, written again here: that file
// is not touched and its outputs keep their bits.
//
// No atomics; the order of every sum depends on the cutout's own data alone, so a cutout's outputs have the same bits alone,
// at any batch position, with a shared or a per-cutout table index and from run to run.
#include "prf_common.hpp"  // the polyphase table, the taps and the value, shared with prffit.hip
#include "psf_common.hpp"  // the lane mapping, the cadence sum, the Cholesky and the star grouping, shared with the Gaussian files
#include "stage_tile.hpp"

namespace lk {

struct PrfArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask;
    const int *order, *star_off;  // order: the cutouts of this launch (one star count)
    const double *par;        // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first); the two widths are not used
    const double *img;        // [B][S_max][npix]: the model images of the cutouts (no shifts)
    const double *shift_col, *shift_row;
    PrfTable tab;
    double column0, row0;
    unsigned long long inv_nx;  // ceil(2^32 / nx): p / nx = (p inv_nx) >> 32 for p nx < 2^32
    int mask_stride, S_max, N, ny, nx, pitch, mpitch, use_err;
    double *time_out, *flux_out, *err_out, *bkg, *chi2;  // time_out nullable
    int *n_used;
    int8_t *cstat;
};

// tp[k][py][px][Y][X] = T[k][Y os + py][X os + px], 0 outside; thread = one value of tp
__global__ __launch_bounds__(256) void cube_prfphot_polyphase_kernel(const float *__restrict__ T, int n_prf, int Ty, int Tx, int os,
                                                                       int TYp, int TXp, float *__restrict__ tp) {
    const int total = n_prf * os * os * TYp * TXp;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int X = i % TXp, Y = (i / TXp) % TYp, px = (i / (TXp * TYp)) % os, py = (i / (TXp * TYp * os)) % os;
        const int k = i / (TXp * TYp * os * os), y = Y * os + py, x = X * os + px;
        tp[i] = y < Ty && x < Tx ? T[((size_t)k * Ty + y) * Tx + x] : 0.0f;
    }
}

int prf_polyphase_launch(const float *prf_table, int n_prf, int Ty, int Tx, int os, int TYp, int TXp, float *tp, hipStream_t stream) {
    const int total = n_prf * os * os * TYp * TXp;
    hipLaunchKernelGGL(cube_prfphot_polyphase_kernel, dim3(std::min((total + 255) / 256, 4096)), dim3(256), 0, stream, prf_table, n_prf,
                       Ty, Tx, os, TYp, TXp, tp);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// img[b][s][p] = the model of star s of cutout b at pixel p, no shift; workgroup = cutout, thread = pixel
__global__ __launch_bounds__(64) void cube_prfphot_images_kernel(const double *__restrict__ par, const int *__restrict__ n_stars,
                                                                    int S_max, int ny, int nx, double column0, double row0,
                                                                    const PrfTable g, double *__restrict__ img) {
    const int b = blockIdx.x, npix = ny * nx;
    const double *p = par + (size_t)b * (2 * S_max + 2);
    const float *tp = g.tp + (size_t)g.index[b] * g.os * g.os * g.TYp * g.TXp;
    for (int s = 0; s < n_stars[b]; ++s) {
        PrfTaps t;
        prf_taps(t, p[s] + 0.0 - column0, p[S_max + s] + 0.0 - row0, g);
        for (int i = threadIdx.x; i < npix; i += 64)
            img[((size_t)b * S_max + s) * npix + i] = prf_value(t, tp, g.TYp, g.TXp, i / nx, i % nx);
    }
}

template <int S> __global__ __launch_bounds__(PRF_FORM_THREADS) void cube_prfphot_kernel(const PrfArgs a) {
    constexpr int K = S + 1;
    extern __shared__ __align__(16) double prf_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;  // 64, or PRF_FORM_THREADS with shifts: wavefront 0 fits, all of them form the images
    const int b = a.order[blockIdx.y], c0 = blockIdx.x * PSF_T, lane = tid & 63, cl = tid / PSF_LPC, sub = tid % PSF_LPC;
    const int rows = min(PSF_T, a.N - c0), npix = a.ny * a.nx;
    const bool shifted = a.shift_col != nullptr, active = cl < rows;
    double *mod = prf_lds;                                                  // the model images: S x npix, per cadence with shifts
    PrfTaps *taps = reinterpret_cast<PrfTaps *>(mod + (shifted ? PSF_T * a.mpitch : S * npix));  // [cadence][star], with shifts
    float *tf = reinterpret_cast<float *>(taps + (shifted ? PSF_T * S : 0));
    float *te = tf + PSF_T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + PSF_T * a.pitch : te);

    const size_t cad = (size_t)b * a.N + c0 + (active ? cl : 0), off = ((size_t)b * a.N + c0) * npix;
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = tid; i < npix; i += nthr) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    bool fin = isfinite(t);
    if (shifted) {
        const double dcl = a.shift_col[cad], drl = a.shift_row[cad];
        fin = fin && isfinite(dcl) && isfinite(drl);
        const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
        // the taps of the tile's (cadence, star) pairs, shared out over the threads
        for (int q = tid; q < rows * S; q += nthr) {
            const int c = q / S, s = q - c * S;
            const size_t at = (size_t)b * a.N + c0 + c;
            PrfTaps tq;
            prf_taps(tq, p[s] + a.shift_col[at] - a.column0, p[a.S_max + s] + a.shift_row[at] - a.row0, a.tab);
            taps[q] = tq;
        }
        __syncthreads();
        // every wavefront one pair after the other, lane = pixel: the 16 taps of its pixels are 16 contiguous sub-images
        const float *tp = a.tab.tp + (size_t)a.tab.index[b] * a.tab.os * a.tab.os * a.tab.TYp * a.tab.TXp;
#pragma unroll 1
        for (int q = tid >> 6; q < rows * S; q += nthr >> 6) {
            const int c = q / S, s = q - c * S;
            const PrfTaps tq = taps[q];
            double *dst = mod + c * a.mpitch + s * npix;
#pragma unroll 1
            for (int i = lane; i < npix; i += 64) {
                const int iy = (int)(((unsigned long long)i * a.inv_nx) >> 32);
                dst[i] = prf_value(tq, tp, a.tab.TYp, a.tab.TXp, iy, i - iy * a.nx);
            }
        }
    } else {
        for (int i = tid; i < S * npix; i += nthr) mod[i] = a.img[(size_t)b * a.S_max * npix + i];
    }
    __syncthreads();
    if (tid >= 64) return;

    // the sums over this lane's pixel rows, in index order: G[i][j], i <= j, and rhs; column S of the design is the constant
    const float *yrow = tf + cl * a.pitch, *erow = te + cl * a.pitch;
    const double *mrow = mod + (shifted ? cl * a.mpitch : 0);
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
        // no branch on the pixel: one that is not used enters with w = 0 and y = 0 (psfphot.hip)
#pragma unroll 2
        for (int ix = 0; ix < a.nx; ++ix, ++p) {
            const float yf = yrow[p], ef = a.use_err ? erow[p] : 1.0f;
            const bool used = active && sm[p] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
            const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
            double av[K];
#pragma unroll
            for (int s = 0; s < S; ++s) av[s] = mrow[s * npix + p];
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

    // chi2 from the residuals, over the tile and the images the lanes have just walked (st is the same in the lanes of a cadence)
    double chi = 0.0;
    if (st == 0 && active) {
        for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
            int p = iy * a.nx;
#pragma unroll 2
            for (int ix = 0; ix < a.nx; ++ix, ++p) {
                const float yf = yrow[p], ef = a.use_err ? erow[p] : 1.0f;
                const bool used = sm[p] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                const double w = a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                double m = theta[S];
#pragma unroll
                for (int s = 0; s < S; ++s) m += theta[s] * mrow[s * npix + p];
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

namespace {

template <int S> int prf_launch(lk_handle *h, const PrfArgs &a, int chunks, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_prfphot_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_prfphot_kernel<S>, dim3(chunks, count), dim3(a.shift_col ? PRF_FORM_THREADS : 64), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_prfphot_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                        const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                        const float *prf_table, int n_prf, int Ty, int Tx, int oversample, const int32_t *prf_index_host,
                        const double *shift_col, const double *shift_row, double column0, double row0, int use_flux_err,
                        int32_t *star_off_host, double *time_out, double *flux_out, double *flux_err_out, double *background,
                        double *chi2, int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && prf_table, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(flux_out && flux_err_out && background && chi2 && n_used && cadence_status && status, "NULL output buffer");
    LK_REQUIRE((shift_col == nullptr) == (shift_row == nullptr), "shift_col and shift_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
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
    // row pitch of the tile: 4 x an odd number, as psfphot.hip; the images' cadence pitch likewise, in doubles
    const int npix = (int)npix64, pitch = 4 * (((npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const bool shifted = shift_col != nullptr;
    const size_t tile_bytes = (size_t)PSF_T * pitch * 4 * (use_flux_err ? 2 : 1) + npix;
    const auto mpitch = [&](int S) { return 4 * (((S * npix + 3) / 4) | 1); };
    const auto lds_bytes = [&](int S) {
        return (shifted ? (size_t)PSF_T * mpitch(S) * 8 + (size_t)PSF_T * S * sizeof(PrfTaps) : (size_t)S * npix * 8) + tile_bytes;
    };
    LK_REQUIRE(lds_bytes(S_max) <= (size_t)PSF_MAX_LDS, "a %d x %d cutout with %d stars%s needs %zu bytes of LDS, more than %d", ny, nx,
               S_max, shifted ? " and shifts" : "", lds_bytes(S_max), PSF_MAX_LDS);

    // the cutout's stars (no NaN coordinate) first and in order; the cutouts grouped by their star count
    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, nullptr, star_off_host, stars)) return rc;
    const std::vector<int> &ints = stars.ints;
    const int *first = stars.first;
    std::vector<int> pidx(B, 0);
    if (prf_index_host) pidx.assign(prf_index_host, prf_index_host + B);

    double *d_par, *d_img;
    int *d_ints, *d_pidx;
    float *d_tp;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)stars.par.data(), stars.par.size())
                           .upload(d_ints, (const int *)ints.data(), ints.size())
                           .upload(d_pidx, (const int *)pidx.data(), pidx.size())
                           .buf(d_tp, (size_t)n_prf * table64)
                           .buf(d_img, (size_t)B * S_max * npix, !shifted)
                           .carve(stream))
        return rc;
    if (const int rc = prf_polyphase_launch(prf_table, n_prf, Ty, Tx, os, TYp, TXp, d_tp, stream)) return rc;
    PrfTable tab;
    tab.tp = d_tp, tab.index = d_pidx, tab.os = os, tab.TYp = TYp, tab.TXp = TXp, tab.hx = 0.5 * (Tx - 1), tab.hy = 0.5 * (Ty - 1);
    if (!shifted) {
        hipLaunchKernelGGL(cube_prfphot_images_kernel, dim3(B), dim3(64), 0, stream, (const double *)d_par, (const int *)(d_ints + B),
                           S_max, ny, nx, column0, row0, tab, d_img);
        LK_HIP_CHECK(hipGetLastError());
    }
    PrfArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask;
    a.star_off = d_ints + 2 * B;
    a.par = d_par, a.img = d_img, a.shift_col = shift_col, a.shift_row = shift_row;
    a.tab = tab;
    a.column0 = column0, a.row0 = row0;
    a.inv_nx = (((unsigned long long)1 << 32) + nx - 1) / nx;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.use_err = use_flux_err ? 1 : 0;
    a.time_out = time_out, a.flux_out = flux_out, a.err_out = flux_err_out, a.bkg = background, a.chi2 = chi2;
    a.n_used = (int *)n_used, a.cstat = cadence_status;
    const int chunks = (N + PSF_T - 1) / PSF_T;
    for (int S = 1; S <= S_max; ++S) {
        const int count = first[S + 1] - first[S];
        if (!count) continue;
        a.order = d_ints + first[S];
        a.mpitch = mpitch(S);
        int rc = LK_OK;
        switch (S) {
        case 1: rc = prf_launch<1>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 2: rc = prf_launch<2>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 3: rc = prf_launch<3>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 4: rc = prf_launch<4>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 5: rc = prf_launch<5>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 6: rc = prf_launch<6>(h, a, chunks, count, lds_bytes(S), stream); break;
        case 7: rc = prf_launch<7>(h, a, chunks, count, lds_bytes(S), stream); break;
        default: rc = prf_launch<8>(h, a, chunks, count, lds_bytes(S), stream); break;
        }
        if (rc) return rc;
    }
    return psf_status_launch(B, N, cadence_status, status, stream);
}

}  // namespace lk
