// psfpos.hip — the positions of a cutout's stars, fitted on resident pixel cubes on gfx950: ONE (column, row) per fitted star,
// shared by all the cutout's cadences, by variable projection — the last input that psfphot.hip, psffit.hip and psfwidth.hip
// take as given.  psfwidth.hip's structure with 2 S shared non-linear unknowns in the place of 2: the linear unknowns (S fluxes
// and a background per cadence) are projected out per cadence and the cadences' 2 S x 2 S Schur complements are summed over the
// cutout.
//
// Reference: PixelCube.psf_positions (correctors/pldcorrector.py), plain float64 numpy; include/lkhip.h has the definition.
//
// One evaluation at the cutout's current positions is two kernels; the host enqueues the pair max_iter + 1 times with no
// synchronisation and no host read in between.
//   evaluate  workgroup (tile of PSF_T = 16 cadences, cutout) of ONE wavefront, PSF_LPC = 4 adjacent lanes per cadence: the
//             mapping, the staging, the LDS layout, the tables (fit_table_run: a factor and its derivative by the centre) and
//             walk 1 of cube_psffit_kernel<S>.  It reads the positions and the phase from the cutout's state record and returns
//             at once when the cutout has stopped.  A tile that cadence_mask leaves out entirely writes a record of +0 without
//             reading the cube.  All 2 S columns of D are always formed: fit_star is applied in the step kernel, because the
//             Schur complement over the fitted subset is exactly the submatrix of S2.
//             Walk 2 runs once per STAR PANEL, s = S - 1 down to 0 in a loop that is not unrolled: a panel holds the two rows
//             of E = D^T W D of star s (2 x 2 S), C_s = A^T W D_s (K x 2), g_s and chi2 in registers — 6 S + 5 accumulators where
//             the whole of E and C would be S (2 S + 1) + 2 S K, 280 doubles at S = 8.  After the butterfly over the cadence's
//             lanes Y_s = L^-1 C_s is parked in LDS (K x 2 S doubles per cadence); the panels run downwards so that Y_t, t > s,
//             is already there and the blocks S2[2 s + a][2 t + b] = E - Y_s^T Y_t, t >= s, are finished at once, added over
//             the tile's 16 cadences by psf_tile_sum (a cadence that does not contribute enters as +0) and written by lane 0.
//             Star s's own theta is picked by a chain of selects and its tables are read from LDS at a run-time index, so no
//             register array is indexed dynamically.
//   step      one wavefront per cutout: every entry of the record is summed lane-strided over the cutout's tile records in
//             index order and then by the butterfly (psf_wave_sum) — an order fixed by the number of tiles alone —; lane 0
//             selects the fitted rows and columns, runs the P x P Cholesky, the solve, the clamp and the update rules of the
//             header in LDS, writes the trace row and advances the state (0 iterating -> 1 final evaluation pending -> 2 done);
//             when the cutout stops all lanes write its outputs, H^-1 from L^-1 on the final evaluation.
//
// Tile records: entry-major, rec[cutout][entry][tile], so that the step kernel's lane-strided sum over the tiles of one entry
// reads consecutive doubles.  For a cutout of S stars, P = 2 S: entries 0 .. P - 1 are g, then the upper triangle of H by rows
// (entry P + r P - r (r - 1) / 2 + c - r for c >= r), then chi2: P + P (P + 1) / 2 + 1 doubles; the two 64-bit counts sit in an
// array of their own, cnt[cutout][2][tile].  A cutout's slice has the stride of the batch's S_max.
//
// LDS per workgroup: cube_psffit_kernel's own count plus 16 x 8 K 2 S bytes of parked Y.  No instantiation uses scratch memory
// (profiles/kernel_resources.md).
//
// No atomics; the order of every sum depends on N alone, so a cutout's outputs have the same bits alone, at any batch position,
// with any other cutouts in the batch and from run to run.
#include "psf_common.hpp"
#include "stage_tile.hpp"

namespace lk {

constexpr int POS_PMAX = 2 * PSF_MAX_STARS;  // the most unknowns of a cutout

// the number of doubles of a tile record at S stars
constexpr int pos_record_len(int S) { return 2 * S + S * (2 * S + 1) + 1; }

// the state of a cutout's iteration, in device memory between the kernels
struct PosState {
    double v[POS_PMAX];    // (column, row) of every star of the cutout, index 2 star + axis; the fitted ones move
    double last;           // the last step taken
    int phase, n_iter, status, pad;  // phase: 0 iterating; 1 stopped and ok: the next evaluation is the final one; 2 done
};

struct PosArgs {
    const double *time;
    const float *flux, *ferr;
    const uint8_t *mask, *cmask;  // cmask nullable: the cadences to fit on
    const int *order;             // the cutouts of this launch (one star count)
    const double *par;            // [B][2 S_max + 2]: star columns, star rows (the cutout's stars first), sigma_col, sigma_row
    const double *sh_col, *sh_row;  // nullable: the shifts
    const PosState *state;
    double column0, row0;
    int mask_stride, S_max, N, ny, nx, pitch, use_err, chunks, rec_max;
    double *rec;     // [B][rec_max][chunks]
    long long *cnt;  // [B][2][chunks]: contributing cadences, their used pixels
    int8_t *cstat;
};

struct PosStepArgs {
    PosState *state;
    const double *rec;
    const long long *cnt;
    const double *par;
    const int *n_stars;  // [B]
    const int *sel;      // [B][S_max]: star s of the cutout sits in the caller's slot sel & 255 and is fitted when sel & 256
    double tol, max_step, max_offset;
    int chunks, max_iter, pass, S_max, rec_max;
    double *col, *row, *col_err, *row_err, *cov, *chi2, *last_step, *trace;
    int *n_iter, *n_cad, *status;
    long long *n_pix;
};

__global__ __launch_bounds__(256) void cube_psfpos_init_kernel(int B, int cells, const double *__restrict__ par, int S_max,
                                                               const int *__restrict__ n_stars, PosState *__restrict__ state,
                                                               double *__restrict__ trace) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < cells) trace[i] = NAN;
    if (i < B) {
        const double *p = par + (size_t)i * (2 * S_max + 2);
        PosState s;
        const int S = n_stars[i];
#pragma unroll
        for (int k = 0; k < PSF_MAX_STARS; ++k) {
            s.v[2 * k] = k < S ? p[k] : NAN;
            s.v[2 * k + 1] = k < S ? p[S_max + k] : NAN;
        }
        s.last = NAN;
        s.phase = s.n_iter = s.status = s.pad = 0;
        state[i] = s;
    }
}

template <int S> __global__ __launch_bounds__(64) void cube_psfpos_eval_kernel(const PosArgs a) {
    constexpr int K = S + 1, P = 2 * S, NH = P * (P + 1) / 2;
    extern __shared__ __align__(16) double pos_lds[];
    const int b = a.order[blockIdx.y];
    if (a.state[b].phase == 2) return;  // the cutout has stopped: nothing of it is read or written any more
    const int c0 = blockIdx.x * PSF_T, lane = threadIdx.x, cl = lane / PSF_LPC, sub = lane % PSF_LPC;
    const int rows = min(PSF_T, a.N - c0), npix = a.ny * a.nx, nt = a.nx + a.ny;
    const bool active = cl < rows;
    double *sh_val = pos_lds;                     // S x nt factors per cadence, [factor][cadence]
    double *sh_der = sh_val + S * nt * PSF_T;     // their derivatives by the star's centre
    double *sh_y = sh_der + S * nt * PSF_T;       // Y = L^-1 C, K x P per cadence, [i P + p][cadence]
    float *tf = reinterpret_cast<float *>(sh_y + K * P * PSF_T);
    float *te = tf + PSF_T * a.pitch;
    uint8_t *sm = reinterpret_cast<uint8_t *>(a.use_err ? te + PSF_T * a.pitch : te);
    double *rec = a.rec + (size_t)b * a.rec_max * a.chunks + blockIdx.x;  // entry e of this tile: rec[e * chunks]
    long long *cnt = a.cnt + (size_t)b * 2 * a.chunks + blockIdx.x;

    const size_t cad = (size_t)b * a.N + c0 + (active ? cl : 0), off = ((size_t)b * a.N + c0) * npix;
    const bool selected = a.cmask ? a.cmask[cad] != 0 : true;
    if (!__any(active && selected)) {  // cadence_mask leaves the whole tile out: its record is +0 and the cube is not read
        for (int e = lane; e < P + NH + 1; e += 64) rec[(size_t)e * a.chunks] = 0.0;
        if (lane == 0) cnt[0] = 0, cnt[a.chunks] = 0;
        if (active && sub == 0) a.cstat[cad] = 6;
        return;
    }
    stage_contiguous(a.flux + off, tf, rows * npix, npix, a.pitch);
    if (a.use_err) stage_contiguous(a.ferr + off, te, rows * npix, npix, a.pitch);
    for (int i = lane; i < npix; i += 64) sm[i] = a.mask[(size_t)b * a.mask_stride + i];
    const double t = a.time[cad];
    const double uc = a.sh_col ? a.sh_col[cad] : 0.0, ur = a.sh_row ? a.sh_row[cad] : 0.0;
    const double *p = a.par + (size_t)b * (2 * a.S_max + 2);
    const double *v = a.state[b].v;

    // tables at v: the lanes of a cadence share out its 2 S runs (star, axis); they touch LDS that the staging does not
#pragma unroll 1
    for (int q = sub; q < 2 * S; q += PSF_LPC) {
        const int s = q >> 1, ax = q & 1, base = (s * nt + (ax ? a.nx : 0)) * PSF_T + cl;
        fit_table_run(sh_val + base, sh_der + base, ax ? a.ny : a.nx, ax ? v[q] + ur - a.row0 : v[q] + uc - a.column0,
                      p[2 * a.S_max + ax]);
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
    if (st == 0 && singular) st = 3;
    const bool in = active && st == 0;  // a cadence that does not contribute enters the tile's sums as +0

    // walk 2, once per star panel s: r = y - A theta; D_s = theta_s x (the derivative of star s's image by its column, by its
    // row); the rows 2 s and 2 s + 1 of E = D^T W D, C_s = A^T W D_s, g_s = D_s^T W r, chi2
    double chi = 0.0;
#pragma unroll 1
    for (int s = S - 1; s >= 0; --s) {
        double ths = 0.0;
#pragma unroll
        for (int u = 0; u < S; ++u) ths = u == s ? theta[u] : ths;
        double Ec[P], Er[P], Cc[K], Cr[K], g0 = 0.0, g1 = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) Ec[i] = Er[i] = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) Cc[i] = Cr[i] = 0.0;
        chi = 0.0;
        const double *sval = sh_val + s * nt * PSF_T + cl, *sder = sh_der + s * nt * PSF_T + cl;
        for (int iy = sub; iy < a.ny; iy += PSF_LPC) {
            int q = iy * a.nx;
            double gr[S], tg[S], td[S];  // the row factor; theta_u x the row factor; theta_u x the row derivative
#pragma unroll
            for (int u = 0; u < S; ++u) {
                gr[u] = sh_val[(u * nt + a.nx + iy) * PSF_T + cl];
                tg[u] = theta[u] * gr[u];
                td[u] = theta[u] * sh_der[(u * nt + a.nx + iy) * PSF_T + cl];
            }
            const double stg = ths * sval[(a.nx + iy) * PSF_T], std_ = ths * sder[(a.nx + iy) * PSF_T];
#pragma unroll 2
            for (int ix = 0; ix < a.nx; ++ix, ++q) {
                const float yf = yrow[q], ef = a.use_err ? erow[q] : 1.0f;
                const bool used = active && sm[q] && isfinite(yf) && isfinite(ef) && ef > 0.0f;
                const double y = used ? (double)yf : 0.0, w = !used ? 0.0 : a.use_err ? 1.0 / ((double)ef * (double)ef) : 1.0;
                double av[K], dc[S], dr[S], m = theta[S];
#pragma unroll
                for (int u = 0; u < S; ++u) {
                    const double gc = sh_val[(u * nt + ix) * PSF_T + cl];
                    av[u] = gc * gr[u];
                    m += theta[u] * av[u];
                    dc[u] = tg[u] * sh_der[(u * nt + ix) * PSF_T + cl];
                    dr[u] = td[u] * gc;
                }
                av[S] = 1.0;
                const double res = y - m, wd0 = w * (stg * sder[ix * PSF_T]), wd1 = w * (std_ * sval[ix * PSF_T]);
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    Cc[i] += wd0 * av[i];
                    Cr[i] += wd1 * av[i];
                }
#pragma unroll
                for (int u = 0; u < S; ++u) {
                    Ec[2 * u] += wd0 * dc[u], Ec[2 * u + 1] += wd0 * dr[u];
                    Er[2 * u] += wd1 * dc[u], Er[2 * u + 1] += wd1 * dr[u];
                }
                g0 += wd0 * res, g1 += wd1 * res;
                chi += w * (res * res);
            }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) Cc[i] = psf_cadence_sum(Cc[i]), Cr[i] = psf_cadence_sum(Cr[i]);
#pragma unroll
        for (int i = 0; i < P; ++i) Ec[i] = psf_cadence_sum(Ec[i]), Er[i] = psf_cadence_sum(Er[i]);
        g0 = psf_cadence_sum(g0), g1 = psf_cadence_sum(g1), chi = psf_cadence_sum(chi);

        // Y_s = L^-1 C_s, parked for the panels below this one
        double Y0[K], Y1[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double y0 = Cc[i], y1 = Cr[i];
#pragma unroll
            for (int j = 0; j < i; ++j) y0 -= L[i][j] * Y0[j], y1 -= L[i][j] * Y1[j];
            Y0[i] = y0 / L[i][i], Y1[i] = y1 / L[i][i];
            if (sub == 0) sh_y[(i * P + 2 * s) * PSF_T + cl] = Y0[i], sh_y[(i * P + 2 * s + 1) * PSF_T + cl] = Y1[i];
        }
        __syncthreads();

        // the blocks S2[2 s + a][2 u + b] = E - Y_s^T Y_u, u >= s, added over the tile's cadences
        g0 = psf_tile_sum(in ? g0 : 0.0), g1 = psf_tile_sum(in ? g1 : 0.0);
        if (lane == 0) rec[(size_t)(2 * s) * a.chunks] = g0, rec[(size_t)(2 * s + 1) * a.chunks] = g1;
        const int r0 = 2 * s, h0 = P + r0 * P - r0 * (r0 - 1) / 2 - r0, h1 = P + (r0 + 1) * P - (r0 + 1) * r0 / 2 - (r0 + 1);
#pragma unroll
        for (int c = 0; c < P; ++c) {
            if (c >= r0) {  // uniform: s is
                double e0 = Ec[c], e1 = Er[c];
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const double yu = sh_y[(i * P + c) * PSF_T + cl];
                    e0 -= Y0[i] * yu, e1 -= Y1[i] * yu;
                }
                e0 = psf_tile_sum(in ? e0 : 0.0), e1 = psf_tile_sum(in ? e1 : 0.0);
                if (lane == 0) {
                    rec[(size_t)(h0 + c) * a.chunks] = e0;
                    if (c > r0) rec[(size_t)(h1 + c) * a.chunks] = e1;
                }
            }
        }
    }
    chi = psf_tile_sum(in ? chi : 0.0);
    const long long nc = psf_tile_sum(in ? 1LL : 0LL), np = psf_tile_sum(in ? (long long)n : 0LL);
    if (lane == 0) rec[(size_t)(P + NH) * a.chunks] = chi, cnt[0] = nc, cnt[a.chunks] = np;
    if (active && sub == 0) a.cstat[cad] = (int8_t)st;
}

__global__ __launch_bounds__(64) void cube_psfpos_step_kernel(const PosStepArgs a) {
    __shared__ double sums[pos_record_len(PSF_MAX_STARS)], Hf[POS_PMAX][POS_PMAX], Lm[POS_PMAX][POS_PMAX], Mi[POS_PMAX][POS_PMAX];
    __shared__ double gf[POS_PMAX], zv[POS_PMAX];
    __shared__ int full[POS_PMAX], fitted_of[POS_PMAX];  // full[p]: the column among 2 S of unknown p; fitted_of: its inverse or -1
    __shared__ int col_of[POS_PMAX], flag, n_fit;         // col_of: index 2 slot + axis of the caller -> the unknown, or -1
    __shared__ long long counts[2];
    const int b = blockIdx.x, lane = threadIdx.x;
    PosState *state = a.state + b;
    if (state->phase == 2) return;
    const int S = a.n_stars[b], P2 = 2 * S, R = pos_record_len(S);
    // the cutout's sums: every entry lane-strided over its tile records in index order, then the butterfly
    const double *rec = a.rec + (size_t)b * a.rec_max * a.chunks;
    for (int e = 0; e < R; ++e) {
        double v = 0.0;
        for (int i = lane; i < a.chunks; i += 64) v += rec[(size_t)e * a.chunks + i];
        v = psf_wave_sum(v);
        if (lane == 0) sums[e] = v;
    }
    for (int e = 0; e < 2; ++e) {
        long long v = 0;
        for (int i = lane; i < a.chunks; i += 64) v += a.cnt[((size_t)b * 2 + e) * a.chunks + i];
        v = psf_wave_sum(v);
        if (lane == 0) counts[e] = v;
    }
    const int *sel = a.sel + (size_t)b * a.S_max;
    const double *par = a.par + (size_t)b * (2 * a.S_max + 2);
    const int W = 2 * a.S_max, rows = a.max_iter + 1;
    if (lane == 0) {
        const long long nc = counts[0];
        int P = 0;
        for (int s = 0; s < S; ++s) {
            const bool f = (sel[s] & 256) != 0;
            fitted_of[2 * s] = f ? P : -1, fitted_of[2 * s + 1] = f ? P + 1 : -1;
            if (f) full[P] = 2 * s, full[P + 1] = 2 * s + 1, P += 2;
        }
        int phase = state->phase, n_iter = state->n_iter, status = state->status;
        double last = state->last;
        double *trace = a.trace + ((size_t)b * rows + n_iter) * W;  // evaluation pass is made at row n_iter = pass - 1 or less
        for (int s = 0; s < S; ++s) trace[2 * (sel[s] & 255)] = state->v[2 * s], trace[2 * (sel[s] & 255) + 1] = state->v[2 * s + 1];

        bool singular = false;
        if (nc != 0) {
            // the fitted rows and columns of H, and H = Lm Lm^T without pivoting
            for (int p = 0; p < P; ++p) {
                gf[p] = sums[full[p]];
                for (int q = p; q < P; ++q) {
                    const int r = full[p], c = full[q];
                    Hf[p][q] = Hf[q][p] = sums[P2 + r * P2 - r * (r - 1) / 2 + c - r];
                }
            }
            for (int k = 0; k < P; ++k) {
                double d = Hf[k][k];
                for (int j = 0; j < k; ++j) d -= Lm[k][j] * Lm[k][j];
                singular = singular || !(isfinite(d) && d > PSF_PIVOT_CUT * Hf[k][k]);
                Lm[k][k] = sqrt(d);
                for (int i = k + 1; i < P; ++i) {
                    double t = Hf[k][i];
                    for (int j = 0; j < k; ++j) t -= Lm[i][j] * Lm[k][j];
                    Lm[i][k] = t / Lm[k][k];
                }
            }
        }
        const bool final_eval = phase == 1;
        bool ok = false;
        if (nc == 0) status = 1, phase = 2;
        else if (singular) status = 3, phase = 2;
        else if (final_eval) ok = true, phase = 2;
        else {
            for (int i = 0; i < P; ++i) {
                double t = gf[i];
                for (int j = 0; j < i; ++j) t -= Lm[i][j] * zv[j];
                zv[i] = t / Lm[i][i];
            }
            for (int i = P - 1; i >= 0; --i) {
                double t = zv[i];
                for (int j = i + 1; j < P; ++j) t -= Lm[j][i] * gf[j];
                gf[i] = t / Lm[i][i];  // dv
            }
            bool left = false;
            last = 0.0;
            for (int p = 0; p < P; ++p) {
                double dv = gf[p];
                dv = dv > a.max_step ? a.max_step : dv < -a.max_step ? -a.max_step : dv;
                const int k = full[p];
                const double nv = state->v[k] + dv, start = k & 1 ? par[a.S_max + (k >> 1)] : par[k >> 1];
                state->v[k] = nv;
                last = fabs(dv) > last ? fabs(dv) : last;
                left = left || fabs(nv - start) > a.max_offset;
            }
            n_iter = a.pass;
            if (left) status = 5, phase = 2;
            else if (a.tol > 0.0 && last < a.tol) phase = 1;
            else if (a.pass == a.max_iter) {
                if (a.tol > 0.0) status = 4, phase = 2;
                else phase = 1;
            }
        }
        state->phase = phase, state->n_iter = n_iter, state->status = status, state->last = last;
        if (ok)  // Mi = Lm^-1 column by column; H^-1 = Mi^T Mi
            for (int k = 0; k < P; ++k) {
                Mi[k][k] = 1.0 / Lm[k][k];
                for (int i = k + 1; i < P; ++i) {
                    double t = 0.0;
                    for (int j = k; j < i; ++j) t -= Lm[i][j] * Mi[j][k];
                    Mi[i][k] = t / Lm[i][i];
                }
            }
        flag = phase != 2 ? 0 : ok ? 2 : 1;
        n_fit = P;
        if (phase == 2) {
            a.chi2[b] = ok ? sums[R - 1] : NAN;
            a.last_step[b] = last;
            a.n_iter[b] = n_iter, a.n_cad[b] = (int)nc, a.n_pix[b] = counts[1], a.status[b] = status;
        }
    }
    __syncthreads();
    if (flag == 0) return;
    // the cutout has stopped: its outputs in the caller's slot layout, one lane per slot.  NaN in the fitted stars' positions and
    // errors and in position_cov unless this was the final evaluation of an ok cutout; a star that is not fitted keeps its given
    // bits; an empty slot is NaN
    const bool ok = flag == 2;
    const int P = n_fit;
    if (lane < a.S_max) {
        int star = -1;
        for (int s = 0; s < S; ++s) star = (sel[s] & 255) == lane ? s : star;
        const bool f = star >= 0 && (sel[star] & 256) != 0;
        const int pc = f ? fitted_of[2 * star] : -1, pr = f ? fitted_of[2 * star + 1] : -1;
        double vc = 0.0, vr = 0.0;
        if (ok && f)
            for (int i = pc; i < P; ++i) vc += Mi[i][pc] * Mi[i][pc], vr += i >= pr ? Mi[i][pr] * Mi[i][pr] : 0.0;
        const size_t o = (size_t)b * a.S_max + lane;
        a.col[o] = star < 0 ? NAN : f ? (ok ? state->v[2 * star] : NAN) : par[star];
        a.row[o] = star < 0 ? NAN : f ? (ok ? state->v[2 * star + 1] : NAN) : par[a.S_max + star];
        a.col_err[o] = ok && f ? sqrt(vc) : NAN;
        a.row_err[o] = ok && f ? sqrt(vr) : NAN;
        col_of[2 * lane] = pc, col_of[2 * lane + 1] = pr;
    }
    __syncthreads();
    for (int e = lane; e < W * W; e += 64) {
        const int r = e / W, c = e % W, pr = col_of[r], pc = col_of[c];
        double v = NAN;
        if (ok && pr >= 0 && pc >= 0) {
            v = 0.0;
            for (int i = pr > pc ? pr : pc; i < P; ++i) v += Mi[i][pr] * Mi[i][pc];
        }
        a.cov[(size_t)b * W * W + e] = v;
    }
}

namespace {

template <int S> int pos_launch(lk_handle *h, const PosArgs &a, int count, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024)
        if (const int rc = want_lds(h, reinterpret_cast<const void *>(&cube_psfpos_eval_kernel<S>), PSF_MAX_LDS)) return rc;
    hipLaunchKernelGGL(cube_psfpos_eval_kernel<S>, dim3(a.chunks, count), dim3(64), lds, stream, a);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace

int cube_psfpos_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const double *sigma_host, const uint8_t *fit_star_host, const double *shift_col, const double *shift_row,
                       const uint8_t *cadence_mask, int max_iter, double tol, double max_step, double max_offset, double column0,
                       double row0, int use_flux_err, double *star_col, double *star_row, double *star_col_err, double *star_row_err,
                       double *position_cov, double *chi2, double *last_step, double *trace, int32_t *n_iter, int32_t *n_cadences,
                       int64_t *n_pixels, int8_t *cadence_status, int32_t *status, hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ny >= 1 && nx >= 1, "need 1 <= B <= 65535, N >= 1, ny >= 1, nx >= 1");
    LK_REQUIRE(S_max >= 1 && S_max <= PSF_MAX_STARS, "S_max must be 1 .. %d (got %d)", PSF_MAX_STARS, S_max);
    LK_REQUIRE(time && flux && mask && star_col_host && star_row_host && sigma_host, "NULL input");
    LK_REQUIRE(!use_flux_err || flux_err, "use_flux_err needs flux_err");
    LK_REQUIRE(star_col && star_row && star_col_err && star_row_err && position_cov && chi2 && last_step && trace, "NULL output buffer");
    LK_REQUIRE(n_iter && n_cadences && n_pixels && cadence_status && status, "NULL output buffer");
    LK_REQUIRE((shift_col == nullptr) == (shift_row == nullptr), "shift_col and shift_row go together");
    LK_REQUIRE(std::isfinite(column0) && std::isfinite(row0), "column0 / row0 must be finite");
    LK_REQUIRE(max_iter >= 1 && max_iter <= 64, "max_iter must be 1 .. 64 (got %d)", max_iter);
    LK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "tol must be finite and >= 0 (got %g)", tol);
    LK_REQUIRE(max_step > 0.0 && max_offset > 0.0, "max_step and max_offset must be > 0 (got %g, %g)", max_step, max_offset);
    const int64_t npix64 = (int64_t)ny * nx;
    LK_REQUIRE((int64_t)N * npix64 < (int64_t)1 << 31, "a cutout of %d x %d x %d values is too large", N, ny, nx);
    // the tile's row pitch as in psfphot.hip: 4 x an odd number
    const int npix = (int)npix64, nt = nx + ny, pitch = 4 * (((npix + 3) / 4) | 1);
    LK_REQUIRE(mask_stride == 0 || mask_stride == npix, "mask_stride must be 0 (one mask for the batch) or npix");
    const size_t tile_bytes = (size_t)PSF_T * pitch * 4 * (use_flux_err ? 2 : 1) + npix;
    // factors and derivatives as in psffit.hip, and the parked Y = L^-1 C, (S + 1) x 2 S doubles per cadence
    const auto lds_bytes = [&](int S) { return (size_t)2 * S * nt * 8 * PSF_T + (size_t)(S + 1) * 2 * S * 8 * PSF_T + tile_bytes; };
    LK_REQUIRE(lds_bytes(S_max) <= (size_t)PSF_MAX_LDS,
               "a %d x %d cutout with %d stars needs %zu bytes of LDS for the position fit, more than %d", ny, nx, S_max,
               lds_bytes(S_max), PSF_MAX_LDS);

    PsfStars stars;
    if (const int rc = psf_group_stars(B, S_max, star_col_host, star_row_host, sigma_host, nullptr, stars)) return rc;
    // star s of a cutout (psf_group_stars' order: the slots without a NaN coordinate) -> its slot, and whether it is fitted
    std::vector<int> sel((size_t)B * S_max, 0);
    for (int b = 0; b < B; ++b) {
        int S = 0, fitted = 0;
        for (int s = 0; s < S_max; ++s) {
            const size_t o = (size_t)b * S_max + s;
            if (std::isnan(star_col_host[o]) || std::isnan(star_row_host[o])) continue;
            const bool f = !fit_star_host || fit_star_host[o] != 0;
            sel[(size_t)b * S_max + S++] = s | (f ? 256 : 0);
            fitted += f ? 1 : 0;
        }
        LK_REQUIRE(fitted >= 1, "cutout %d has no fitted star", b);
    }
    const int chunks = (N + PSF_T - 1) / PSF_T, rec_max = pos_record_len(S_max);
    double *d_par, *d_rec;
    int *d_ints, *d_sel;
    long long *d_cnt;
    PosState *d_state;
    if (const int rc = Scratch(h, h->ws)
                           .upload(d_par, (const double *)stars.par.data(), stars.par.size())
                           .upload(d_ints, (const int *)stars.ints.data(), stars.ints.size())
                           .upload(d_sel, (const int *)sel.data(), sel.size())
                           .buf(d_state, (size_t)B)
                           .buf(d_rec, (size_t)B * rec_max * chunks)
                           .buf(d_cnt, (size_t)B * 2 * chunks)
                           .carve(stream))
        return rc;
    const int cells = B * (max_iter + 1) * 2 * S_max;  // cells >= B
    hipLaunchKernelGGL(cube_psfpos_init_kernel, dim3((cells + 255) / 256), dim3(256), 0, stream, B, cells, (const double *)d_par, S_max,
                       (const int *)(d_ints + B), d_state, trace);
    LK_HIP_CHECK(hipGetLastError());

    PosArgs a;
    a.time = time, a.flux = flux, a.ferr = flux_err, a.mask = mask, a.cmask = cadence_mask;
    a.par = d_par, a.sh_col = shift_col, a.sh_row = shift_row, a.state = d_state;
    a.column0 = column0, a.row0 = row0;
    a.mask_stride = mask_stride, a.S_max = S_max, a.N = N, a.ny = ny, a.nx = nx, a.pitch = pitch, a.use_err = use_flux_err ? 1 : 0;
    a.chunks = chunks, a.rec_max = rec_max, a.rec = d_rec, a.cnt = d_cnt, a.cstat = cadence_status;
    PosStepArgs s;
    s.state = d_state, s.rec = d_rec, s.cnt = d_cnt, s.par = d_par, s.n_stars = d_ints + B, s.sel = d_sel;
    s.tol = tol, s.max_step = max_step, s.max_offset = max_offset;
    s.chunks = chunks, s.max_iter = max_iter, s.S_max = S_max, s.rec_max = rec_max;
    s.col = star_col, s.row = star_row, s.col_err = star_col_err, s.row_err = star_row_err, s.cov = position_cov, s.chi2 = chi2;
    s.last_step = last_step, s.trace = trace;
    s.n_iter = (int *)n_iter, s.n_cad = (int *)n_cadences, s.status = (int *)status, s.n_pix = (long long *)n_pixels;
    // pass = the iteration number of every cutout that still iterates; pass max_iter + 1 can only be a final evaluation
    for (int pass = 1; pass <= max_iter + 1; ++pass) {
        for (int S = 1; S <= S_max; ++S) {
            const int count = stars.first[S + 1] - stars.first[S];
            if (!count) continue;
            a.order = d_ints + stars.first[S];
            int rc = LK_OK;
            switch (S) {
            case 1: rc = pos_launch<1>(h, a, count, lds_bytes(S), stream); break;
            case 2: rc = pos_launch<2>(h, a, count, lds_bytes(S), stream); break;
            case 3: rc = pos_launch<3>(h, a, count, lds_bytes(S), stream); break;
            case 4: rc = pos_launch<4>(h, a, count, lds_bytes(S), stream); break;
            case 5: rc = pos_launch<5>(h, a, count, lds_bytes(S), stream); break;
            case 6: rc = pos_launch<6>(h, a, count, lds_bytes(S), stream); break;
            case 7: rc = pos_launch<7>(h, a, count, lds_bytes(S), stream); break;
            default: rc = pos_launch<8>(h, a, count, lds_bytes(S), stream); break;
            }
            if (rc) return rc;
        }
        s.pass = pass;
        hipLaunchKernelGGL(cube_psfpos_step_kernel, dim3(B), dim3(64), 0, stream, s);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

}  // namespace lk
