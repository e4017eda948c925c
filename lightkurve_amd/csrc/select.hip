// select.hip — the cadence-selection steps of a transit search for a ragged batch on gfx950: which cadences are outliers,
// the batch without the cadences a byte mask names, and the CDPP noise metric of what is left.
//
//   outlier_mask_launch    LightCurve.remove_outliers (src/lightkurve/lightcurve.py:1430-1556) with sigma_lower / sigma_upper:
//                          astropy.stats.sigma_clip(y, sigma_lower, sigma_upper, maxiters, cenfunc=median, stdfunc=std).mask
//                          (astropy@4.3.1 stats/sigma_clipping.py, _sigmaclip_noaxis) per ragged row
//   select_columns_launch  lc[mask] / lc[~mask] (LightCurve.__getitem__ with a boolean array) for every column of the batch:
//                          order-preserving compaction by a byte mask over all cadences
//   cdpp_launch            the tail of LightCurve.estimate_cdpp (:1764-1833; running_mean: utils.py:374-386) per row:
//                          normalize("ppm") of the kept values, running mean over transit_duration cadences, np.std
//
// Built with -ffp-contract=off: lo = cen - std * sigma_lower must round as numpy rounds it (a fused multiply-add moves the
// bound by an ulp and with it a cadence that sits on it), and np.std squares and sums in two roundings.
#include <cmath>

#include "block_select.hpp"
#include "lk_common.hpp"

namespace lk {

constexpr int SEL_NT = 1024;  // threads per row of the clip and CDPP kernels (block_sum_dyn needs a power of two)

// ------------------------------------------------------------------------------------------------ asymmetric sigma clip
// One workgroup per row.  outlier[] itself is the state (0 = still kept), so the launcher carves nothing of the batch's
// size.  Each round: cen = median, std = sqrt(mean((x - mean)^2)) of the kept values, keep lo <= x <= hi (equality keeps: a
// constant row loses nothing); stop when a round removes nothing or after maxiters rounds (maxiters < 0: no cap).  The mask
// that comes back is astropy's: not finite, or outside the LAST round's bounds.
__global__ __launch_bounds__(SEL_NT) void outlier_mask_kernel(const double *__restrict__ y, const int64_t *__restrict__ n_off,
                                                              double sigma_lower, double sigma_upper, int maxiters,
                                                              uint8_t *__restrict__ outlier) {
    __shared__ unsigned long long sh[SEL_NT];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = n_off[row];
    const int n = (int)(n_off[row + 1] - lo);
    y += lo;
    outlier += lo;
    auto val = [&](int i) { return y[i]; };
    auto keep = [&](int i) { return outlier[i] == 0; };
    long long cnt = 0;
    for (int i = tid; i < n; i += SEL_NT) {
        const bool fin = isfinite(y[i]);
        outlier[i] = fin ? 0 : 1;
        cnt += fin;
    }
    __syncthreads();
    long long count = block_count_dyn(cnt, reinterpret_cast<long long *>(sh));
    double lo_b = -INFINITY, hi_b = INFINITY;
    for (int it = 0; (maxiters < 0 || it < maxiters) && count > 0; ++it) {
        const double cen = block_median(n, count, val, keep, sh);
        double part = 0.0;
        for (int i = tid; i < n; i += SEL_NT)
            if (outlier[i] == 0) part += y[i];
        const double mean = block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)count;
        part = 0.0;
        for (int i = tid; i < n; i += SEL_NT)
            if (outlier[i] == 0) {
                const double d = y[i] - mean;
                part += d * d;
            }
        const double sd = sqrt(block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)count);
        lo_b = cen - sd * sigma_lower;
        hi_b = cen + sd * sigma_upper;
        cnt = 0;
        for (int i = tid; i < n; i += SEL_NT)
            if (outlier[i] == 0) {
                const double v = y[i];
                const bool in = (v >= lo_b) && (v <= hi_b);
                outlier[i] = in ? 0 : 1;
                cnt += in;
            }
        __syncthreads();
        const long long newcount = block_count_dyn(cnt, reinterpret_cast<long long *>(sh));
        const bool changed = newcount != count;
        count = newcount;
        if (!changed) break;
    }
    for (int i = tid; i < n; i += SEL_NT) {
        const double v = y[i];
        outlier[i] = (!isfinite(v) || v < lo_b || v > hi_b) ? 1 : 0;
    }
}

int outlier_mask_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma_lower, double sigma_upper,
                        int maxiters, uint8_t *outlier, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)n);
    }
    // (NaN bounds would clip nothing, negative ones everything on one side: astropy takes both, so do we; only NaN is refused)
    LK_REQUIRE(!std::isnan(sigma_lower) && !std::isnan(sigma_upper), "sigma_lower / sigma_upper must not be NaN");
    if (n_off_host[B] == 0) return LK_OK;
    LK_REQUIRE(y && outlier, "NULL buffer");
    int64_t *d_off;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).carve(stream)) return rc;
    hipLaunchKernelGGL(outlier_mask_kernel, dim3(B), dim3(SEL_NT), 0, stream, y, d_off, sigma_lower, sigma_upper, maxiters,
                       outlier);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ select by a byte mask
struct SelCols {
    const void *in[8];
    void *out[8];
    int elem[8];  // 4 or 8 bytes
};

__global__ __launch_bounds__(256) void select_count_kernel(const uint8_t *__restrict__ mask, int invert,
                                                            const int64_t *__restrict__ n_off, int64_t *__restrict__ kept) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = n_off[b], n = n_off[b + 1] - lo;
    long long c = 0;
    for (int64_t i = tid; i < n; i += 256) c += ((mask[lo + i] != 0) != (invert != 0)) ? 1 : 0;
    __shared__ long long sh[8];
    const long long tot = block_count_fast(c, sh);
    if (tid == 0) kept[b] = tot;
}

// every wave owns a contiguous strip of the row, positions from ballot prefixes (as ingest_pack_kernel): the output order is
// the input order whatever the scheduling
__global__ __launch_bounds__(512) void select_pack_kernel(const uint8_t *__restrict__ mask, int invert,
                                                           const int64_t *__restrict__ n_off, const int64_t *__restrict__ new_off,
                                                           int ncols, SelCols cp) {
    __shared__ int shi[8];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t lo = n_off[b], olo = new_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    mask += lo;
    const bool inv = invert != 0;
    const int nw = nt >> 6, wv = tid >> 6, lane = tid & 63;
    const int strip = ((n + nw - 1) / nw + 63) & ~63;
    const int k_lo = min(wv * strip, n), k_hi = min(k_lo + strip, n);
    int c = 0;
    for (int k = k_lo + lane; k < k_hi; k += 64) c += ((mask[k] != 0) != inv) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) shi[wv] = c;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += shi[w];
    for (int k0 = k_lo; k0 < k_hi; k0 += 64) {
        const int k = k0 + lane;
        const bool m = k < k_hi && ((mask[k] != 0) != inv);
        const unsigned long long bal = __ballot(m);
        if (m) {
            const int64_t pos = olo + base + __popcll(bal & ((1ull << lane) - 1ull));
            for (int cidx = 0; cidx < ncols; ++cidx) {
                if (cp.elem[cidx] == 8)
                    static_cast<uint64_t *>(cp.out[cidx])[pos] = static_cast<const uint64_t *>(cp.in[cidx])[lo + k];
                else
                    static_cast<uint32_t *>(cp.out[cidx])[pos] = static_cast<const uint32_t *>(cp.in[cidx])[lo + k];
            }
        }
        base += __popcll(bal);
    }
}

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

int select_columns_launch(lk_handle *h, int B, const int64_t *n_off_host, const uint8_t *mask, int invert, int ncols,
                          const int *elem_bytes, const void *const *cols_in, void *const *cols_out, int64_t *new_off_host,
                          hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr && new_off_host != nullptr, "bad batch description");
    LK_REQUIRE(ncols >= 0 && ncols <= 8, "at most 8 columns per call (got %d)", ncols);
    if (B == 0) {
        new_off_host[0] = 0;
        return LK_OK;
    }
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)n);
    }
    const size_t ntot = (size_t)n_off_host[B];
    LK_REQUIRE(mask != nullptr || ntot == 0, "mask is NULL");
    LK_REQUIRE(ncols == 0 || (elem_bytes && cols_in && cols_out), "NULL column table");
    SelCols cp;
    for (int c = 0; c < 8; ++c) cp.in[c] = nullptr, cp.out[c] = nullptr, cp.elem[c] = 8;
    for (int c = 0; c < ncols; ++c) {
        LK_REQUIRE(elem_bytes[c] == 4 || elem_bytes[c] == 8, "column %d: elements of 4 or 8 bytes (got %d)", c, elem_bytes[c]);
        LK_REQUIRE(cols_in[c] && cols_out[c], "column %d is NULL", c);
        cp.in[c] = cols_in[c], cp.out[c] = cols_out[c], cp.elem[c] = elem_bytes[c];
    }
    // the pack reads column c at lo + k while another wave writes it at pos <= lo + k: no output may touch an input, the mask
    // or another output
    for (int c = 0; c < ncols; ++c) {
        const size_t nb = ntot * (size_t)cp.elem[c];
        LK_REQUIRE(!ranges_overlap(cp.out[c], nb, mask, ntot), "cols_out[%d] overlaps the mask", c);
        for (int d = 0; d < ncols; ++d) {
            const size_t nd = ntot * (size_t)cp.elem[d];
            LK_REQUIRE(!ranges_overlap(cp.out[c], nb, cp.in[d], nd), "cols_out[%d] overlaps cols_in[%d]: select is out of place", c, d);
            LK_REQUIRE(d == c || !ranges_overlap(cp.out[c], nb, cp.out[d], nd), "cols_out[%d] overlaps cols_out[%d]", c, d);
        }
    }
    int64_t *d_off, *d_kept, *d_new;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).buf(d_kept, B + 1).buf(d_new, B + 1).carve(stream)) return rc;
    hipLaunchKernelGGL(select_count_kernel, dim3(B), dim3(256), 0, stream, mask, invert, d_off, d_kept);
    exscan_i64_launch(d_kept, B, d_new, stream);
    if (ncols > 0 && ntot > 0)
        hipLaunchKernelGGL(select_pack_kernel, dim3(B), dim3(512), 0, stream, mask, invert, d_off, d_new, ncols, cp);
    LK_HIP_CHECK(hipMemcpyAsync(new_off_host, d_new, (size_t)(B + 1) * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));  // the caller needs the new offsets to address the selected batch
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ CDPP
// One workgroup per row; cum is the row's slice (n + 1 doubles at n_off[row] + row) of a scratch array.
//   med  = median of the kept values                                   (normalize: lightcurve.py:1216-1292)
//   ppm  = kept / med * 1e6, in the original order
//   cum[j] = ppm[0] + ... + ppm[j - 1]: the row is swept in tiles of SEL_NT cadences; inside a tile a wave scan and the wave
//            totals in wave order, between tiles one running carry.  A dropped cadence adds +0.0.  The order of every
//            addition follows from the row's own values and flags alone: the same bits for any B, position or run.
//   mean_j = (cum[j + w] - cum[j]) / w, j < n_kept - w + 1, w = min(transit_duration, n_kept)     (utils.py:374-386)
//   cdpp = sqrt(mean((mean_j - mean(mean_j))^2))                                                  (np.std, two passes)
__global__ __launch_bounds__(SEL_NT) void cdpp_kernel(const double *__restrict__ flat, const uint8_t *__restrict__ outlier,
                                                      const int64_t *__restrict__ n_off, int transit_duration,
                                                      double *__restrict__ cum_all, double *__restrict__ cdpp) {
    __shared__ unsigned long long sh[SEL_NT];
    __shared__ double wsum[SEL_NT / 64];
    __shared__ int wcnt[SEL_NT / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t lo = n_off[row];
    const int n = (int)(n_off[row + 1] - lo);
    flat += lo;
    if (outlier) outlier += lo;
    double *cum = cum_all + lo + row;
    auto val = [&](int i) { return flat[i]; };
    auto keep = [&](int i) { return outlier == nullptr || outlier[i] == 0; };
    long long cnt = 0;
    for (int i = tid; i < n; i += SEL_NT) cnt += keep(i) ? 1 : 0;
    const long long nk = block_count_dyn(cnt, reinterpret_cast<long long *>(sh));
    if (nk == 0) {  // (uniform)
        if (tid == 0) cdpp[row] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double med = block_median(n, nk, val, keep, sh);
    // ---- cum[]: ordered compaction (ballot prefixes) and prefix sums in one sweep
    if (tid == 0) cum[0] = 0.0;
    double carry = 0.0;
    int placed = 0;
    for (int i0 = 0; i0 < n; i0 += SEL_NT) {
        const int i = i0 + tid;
        const bool m = i < n && keep(i);
        const double v = m ? flat[i] / med * 1e6 : 0.0;
        double inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        const unsigned long long bal = __ballot(m);
        __syncthreads();  // wsum / wcnt may still be read by the previous tile
        if (lane == 63) wsum[wv] = inc;
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        double before = 0.0, all = 0.0;
        int cbefore = 0, call = 0;
        for (int w = 0; w < SEL_NT / 64; ++w) {
            if (w == wv) {
                before = all;
                cbefore = call;
            }
            all += wsum[w];
            call += wcnt[w];
        }
        if (m) cum[placed + cbefore + __popcll(bal & ((1ull << lane) - 1ull)) + 1] = carry + (before + inc);
        carry += all;
        placed += call;
    }
    __syncthreads();  // cum[] is read across threads from here on (global memory, written by this workgroup)
    const int w = (int)min((long long)transit_duration, nk);
    const int m_cnt = (int)nk - w + 1;
    const double dw = (double)w;
    double part = 0.0;
    for (int j = tid; j < m_cnt; j += SEL_NT) part += (cum[j + w] - cum[j]) / dw;
    const double mean = block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)m_cnt;
    part = 0.0;
    for (int j = tid; j < m_cnt; j += SEL_NT) {
        const double d = (cum[j + w] - cum[j]) / dw - mean;
        part += d * d;
    }
    const double var = block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)m_cnt;
    if (tid == 0) cdpp[row] = sqrt(var);
}

int cdpp_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *flat_flux, const uint8_t *outlier,
                int transit_duration, double *cdpp_out, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr, "bad batch description");
    LK_REQUIRE(transit_duration >= 1, "transit_duration must be >= 1 cadence (got %d)", transit_duration);
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "target %d has %lld cadences", b, (long long)n);
    }
    LK_REQUIRE(cdpp_out != nullptr && (flat_flux != nullptr || n_off_host[B] == 0), "NULL buffer");
    const size_t ntot = (size_t)n_off_host[B];
    int64_t *d_off;
    double *d_cum;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).buf(d_cum, ntot + (size_t)B).carve(stream)) return rc;
    hipLaunchKernelGGL(cdpp_kernel, dim3(B), dim3(SEL_NT), 0, stream, flat_flux, outlier, d_off, transit_duration, d_cum,
                       cdpp_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
