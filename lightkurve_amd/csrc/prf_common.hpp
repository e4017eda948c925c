// prf_common.hpp — what prfphot.hip (fluxes at given shifts with a tabulated PRF) and prffit.hip (the same with each cadence's
// shift fitted) share: the polyphase copy of the table (made by prfphot.hip's kernel for both), the taps of one (star, cadence) pair,
// and the value of Keys' cubic convolution at a pixel.  Reference: TabulatedPRF (correctors/pldcorrector.py).
#pragma once
#include "psf_common.hpp"

namespace lk {

namespace {

constexpr int PRF_FORM_THREADS = 512;  // the workgroup of a call with shifts: eight wavefronts form the images, the first one fits
constexpr double PRF_FAR = 1e9;  // a star whose table coordinate is not inside +-PRF_FAR samples has no tap on the table

// the polyphase table and its geometry
struct PrfTable {
    const float *tp;     // [n_prf][os][os][TYp][TXp]
    const int *index;    // [B]: the table of every cutout
    int os, TYp, TXp;    // TYp = ceil(Ty / os), TXp = ceil(Tx / os)
    double hx, hy;       // (Tx - 1) / 2, (Ty - 1) / 2: the table coordinate of the star's centre
};

// The taps of one (star, cadence): w[0 .. 3] the column weights w_-1 .. w_2 at f, w[4 .. 7] the row weights at g; tap ii of pixel
// column ix is Tp[..][px][..][x0[ii] + ix] with xph[ii] = px TYp TXp the offset of its phase, likewise y0 / yph (yph = py os TYp
// TXp).  128 bytes.
struct PrfTaps {
    double w[8];
    int x0[4], xph[4], y0[4], yph[4];
};

// one axis: c = the star's centre in pixels from the centre of pixel 0; u = (0 - c) os + half, i0 = floor(u), f = u - i0.  dw
// (nullable): the four weights' derivatives by c, w'(f) du/dc with du/dc = -os (TabulatedPRF.evaluate_with_gradient)
__device__ __forceinline__ void prf_axis(double c, double half, int os, int phase_stride, double *__restrict__ w,
                                         int *__restrict__ first, int *__restrict__ phase, double *__restrict__ dw = nullptr) {
    const double u = (0.0 - c) * (double)os + half;
    const bool far = !(fabs(u) < PRF_FAR);  // also a NaN
    const double fl = floor(u), f = far ? 0.0 : u - fl;
    w[0] = ((-f + 2.0) * f - 1.0) * f * 0.5;
    w[1] = ((3.0 * f - 5.0) * f * f + 2.0) * 0.5;
    w[2] = ((-3.0 * f + 4.0) * f + 1.0) * f * 0.5;
    w[3] = (f - 1.0) * f * f * 0.5;
    if (dw) {
        const double m = -(double)os;
        dw[0] = ((-3.0 * f + 4.0) * f - 1.0) * 0.5 * m;
        dw[1] = (9.0 * f - 10.0) * f * 0.5 * m;
        dw[2] = ((-9.0 * f + 8.0) * f + 1.0) * 0.5 * m;
        dw[3] = (3.0 * f - 2.0) * f * 0.5 * m;
    }
    const int a = far ? 0 : (int)fl - 1;  // the table index of tap -1 of pixel 0
    int q = a / os, r = a % os;
    if (r < 0) r += os, --q;  // floored: a = q os + r, 0 <= r < os
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        first[k] = far ? -(1 << 30) : q;  // far: below every sub-image for every pixel (nx os < 2^30 is required)
        phase[k] = r * phase_stride;
        if (++r == os) r = 0, ++q;
    }
}

__device__ __forceinline__ void prf_taps(PrfTaps &t, double c, double r, const PrfTable &g) {
    const int sub = g.TYp * g.TXp;
    prf_axis(c, g.hx, g.os, sub, t.w, t.x0, t.xph);
    prf_axis(r, g.hy, g.os, sub * g.os, t.w + 4, t.y0, t.yph);
}

// P at pixel (iy, ix): sum_jj w_jj (sum_ii w_ii T), both in the order -1 .. 2, T = 0 outside the table
__device__ __forceinline__ double prf_value(const PrfTaps &t, const float *__restrict__ tp, int TYp, int TXp, int iy, int ix) {
    double acc = 0.0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const unsigned Y = (unsigned)(t.y0[jj] + iy);
        const bool oky = Y < (unsigned)TYp;
        const unsigned rb = (unsigned)t.yph[jj] + Y * (unsigned)TXp;
        double r = 0.0;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const unsigned X = (unsigned)(t.x0[ii] + ix);
            const bool ok = oky && X < (unsigned)TXp;
            const float v = tp[ok ? rb + (unsigned)t.xph[ii] + X : 0u];  // no branch: a tap off the table reads sample 0 and counts 0
            r += t.w[ii] * (ok ? (double)v : 0.0);
        }
        acc += t.w[4 + jj] * r;
    }
    return acc;
}

}  // namespace

// prfphot.hip: the polyphase copy tp[k][py][px][Y][X] = T[k][Y os + py][X os + px], 0 outside the table, TYp = ceil(Ty / os), TXp =
// ceil(Tx / os); tp holds n_prf os os TYp TXp floats.  Enqueued (cube_prfphot_polyphase_kernel)
int prf_polyphase_launch(const float *prf_table, int n_prf, int Ty, int Tx, int os, int TYp, int TXp, float *tp, hipStream_t stream);

}  // namespace lk
