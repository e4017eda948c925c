// overfit.hip — the over-fitting goodness metric of a resident batch, its white noise made on the device.
// Reference: src/lightkurve/correctors/metrics.py:24-138 (overfit_metric_lombscargle).  Per target, on the n kept cadences:
//
//     z0 = y_orig / median(y_orig) - 1.0,  z1 = y_corr / median(y_corr) - 1.0        (these two IEEE operations, in this order)
//     mean_unc = nanmean(err_corr / median(y_corr))
//     P0, P1 = the default Lomb-Scargle ('fast', amplitude normalisation, fit_mean = center_data = 1, oversampling 5) of z0, z1
//     Pn_k   = the same of g_k[i] = normal(i) * mean_unc,  k < n_samples;   mnp_k = nanmean(Pn_k)
//     change = P1 - P0 (NaN dropped);  n_up = #(change > 0);  S = sum of change[change > 0]
//     per_k  = 0 if n_up == 0, inf if n_up * mnp_k == 0, else S / (n_up * mnp_k)
//     metric = 2 / (1 + exp(max(mean_k per_k, 0)))                                   (NaN propagates: max(NaN, 0) is NaN)
//
// The 2 + n_samples periodograms go through lsfast_launch as it is.  It resets (and may regrow) the handle's scratch arena,
// so nothing of this file lives there: rows, noise and spectra are carved from ONE caller-owned block (overfit_plan), and the
// samples are taken in rounds of R so that the block stays under the caller's byte budget.  A target's numbers do not depend
// on R: a row's periodogram does not depend on the other rows of its launch, and every sum below has an order that is a
// function of its length alone.
//
// Noise: Philox4x32-10 (Salmon et al. 2011), key = (seed & 0xffffffff, seed >> 32), counter = (i, k, first_target + b,
// stream_id) for the pair of kept cadences (2i, 2i + 1) of sample k of row b; Box-Muller on 53-bit uniforms built from the
// four output words.  Any (target, sample, cadence) gets the same number whatever B, R or the launch shape.
//
// Summation orders.  nanmean of the errors (prepare): thread j of 1024 adds elements j, j + 1024, ... in ascending order, then
// a halving tree over the 1024 partial sums.  Spectra (change and noise mean): the same with 256 threads.  The sample terms
// enter their mean in order of k, added by one thread.  No atomics.
#include "block_select.hpp"
#include "lk_common.hpp"

#include <algorithm>
#include <cmath>

namespace lk {

constexpr int OF_PREP_NT = 1024;   // prepare: block_median wants a wide workgroup (two selects over n gathered values)
constexpr int OF_NT = 256;         // noise and spectra passes

// ------------------------------------------------------------------------------------------------ Philox4x32-10
struct Philox4 {
    uint32_t x[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// two standard normals from one Philox call: u1 in (0, 1], u2 in [0, 1), both exact multiples of 2^-53
__device__ __forceinline__ void philox_normal_pair(const Philox4 &p, double &a, double &b) {
    const uint64_t w1 = (((uint64_t)(p.x[0] >> 5)) << 26) + (p.x[1] >> 6) + 1u;
    const uint64_t w2 = (((uint64_t)(p.x[2] >> 5)) << 26) + (p.x[3] >> 6);
    const double u1 = (double)w1 * 0x1p-53, u2 = (double)w2 * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    double s, c;
    sincos(ang, &s, &c);
    a = r * c;
    b = r * s;
}

// ------------------------------------------------------------------------------------------------ prepare
// One workgroup per target: exact medians of the kept cadences of both fluxes, the packed rows z0[b], z1[b], the rebased
// times t - t[first kept] (written R times: rows (r, b) of the time block serve the R x B noise rows of a round, rows (0, b)
// the two flux launches), and mean_unc[b].
__global__ __launch_bounds__(OF_PREP_NT) void overfit_prepare_kernel(const double *__restrict__ time, const double *__restrict__ y0,
                                                                    const double *__restrict__ y1, const double *__restrict__ e1,
                                                                    int N, int n, const int32_t *__restrict__ keep_idx, int B,
                                                                    int R, double *__restrict__ z0, double *__restrict__ z1,
                                                                    double *__restrict__ trel, double *__restrict__ mean_unc) {
    __shared__ unsigned long long sh[OF_PREP_NT];
    __shared__ int sh_cnt[OF_PREP_NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t in = (size_t)b * N, out = (size_t)b * n;
    auto idx = [&](int i) { return keep_idx ? keep_idx[i] : i; };
    auto all = [&](int) { return true; };
    const double med0 = block_median(n, (long long)n, [&](int i) { return y0[in + idx(i)]; }, all, sh);
    __syncthreads();
    const double med1 = block_median(n, (long long)n, [&](int i) { return y1[in + idx(i)]; }, all, sh);
    __syncthreads();
    const double t0 = time[in + idx(0)];
    double s = 0.0;
    int cnt = 0;
    for (int i = tid; i < n; i += OF_PREP_NT) {
        const int j = idx(i);
        // y / med - 1.0 as two separately rounded operations (a zero median gives non-finite rows, as in the reference)
        z0[out + i] = __dsub_rn(__ddiv_rn(y0[in + j], med0), 1.0);
        z1[out + i] = __dsub_rn(__ddiv_rn(y1[in + j], med1), 1.0);
        const double tr = __dsub_rn(time[in + j], t0);
        for (int r = 0; r < R; ++r) trel[((size_t)r * B + b) * n + i] = tr;
        const double u = __ddiv_rn(e1[in + j], med1);
        if (u == u) {
            s += u;
            ++cnt;
        }
    }
    double *shd = reinterpret_cast<double *>(sh);
    shd[tid] = s;
    sh_cnt[tid] = cnt;
    __syncthreads();
    for (int h = OF_PREP_NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            shd[tid] += shd[tid + h];
            sh_cnt[tid] += sh_cnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) mean_unc[b] = sh_cnt[0] ? shd[0] / (double)sh_cnt[0] : __longlong_as_double(0x7ff8000000000000ll);
}

// ------------------------------------------------------------------------------------------------ noise
// Rows (kk, b), kk < nk: g[(kk B + b) n + c] = normal(target first_target + b, sample k0 + kk, cadence c) * mean_unc[b]
// (mean_unc == NULL: the normals themselves).  One thread = one Philox call = cadences 2i and 2i + 1; bpr workgroups per row.
// A row starts 16-byte aligned when its first element index is even: then the pair goes out as one 16-byte store.
__global__ __launch_bounds__(OF_NT) void overfit_noise_kernel(int B, int n, int bpr, int k0, uint32_t key0, uint32_t key1,
                                                             uint32_t first_target, uint32_t stream_id,
                                                             const double *__restrict__ mean_unc, double *__restrict__ g) {
    const int row = blockIdx.x / bpr, i = (blockIdx.x - row * bpr) * OF_NT + threadIdx.x;
    const int c = 2 * i;
    if (c >= n) return;
    const int kk = row / B, b = row - kk * B;
    double a, s;
    philox_normal_pair(philox4x32_10((uint32_t)i, (uint32_t)(k0 + kk), first_target + (uint32_t)b, stream_id, key0, key1), a, s);
    const double mu = mean_unc ? mean_unc[b] : 1.0;
    a *= mu;
    s *= mu;
    const size_t base = (size_t)row * n;
    if (c + 1 < n) {
        if ((base & 1) == 0) {
            *reinterpret_cast<double2 *>(g + base + c) = make_double2(a, s);
        } else {
            g[base + c] = a;
            g[base + c + 1] = s;
        }
    } else {
        g[base + c] = a;   // the last pair of an odd count: its second normal is discarded
    }
}

// ------------------------------------------------------------------------------------------------ spectra
// The workgroup's fixed-order sum: thread j holds the partial sum of elements j, j + 256, ...; a halving tree finishes it.
__device__ __forceinline__ void of_tree(double *sd, int *sc, int tid) {
    __syncthreads();
    for (int h = OF_NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sd[tid] += sd[tid + h];
            sc[tid] += sc[tid + h];
        }
        __syncthreads();
    }
}

// change = P1 - P0 of target b: n_up = #(change > 0) (a NaN is not > 0: dropped), S = their sum.
__global__ __launch_bounds__(OF_NT) void overfit_change_kernel(const double *__restrict__ P0, const double *__restrict__ P1, int M,
                                                              int *__restrict__ n_up, double *__restrict__ S) {
    __shared__ double sd[OF_NT];
    __shared__ int sc[OF_NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *p0 = P0 + (size_t)b * M, *p1 = P1 + (size_t)b * M;
    double s = 0.0;
    int c = 0;
#pragma unroll 4
    for (int j = tid; j < M; j += OF_NT) {
        const double d = __dsub_rn(p1[j], p0[j]);
        if (d > 0.0) {
            s += d;
            ++c;
        }
    }
    sd[tid] = s;
    sc[tid] = c;
    of_tree(sd, sc, tid);
    if (tid == 0) {
        n_up[b] = sc[0];
        S[b] = sd[0];
    }
}

// nanmean of each noise spectrum of a round: row (kk, b) -> mnp[(k0 + kk) B + b]
__global__ __launch_bounds__(OF_NT) void overfit_noise_mean_kernel(const double *__restrict__ Pn, int M, double *__restrict__ mnp) {
    __shared__ double sd[OF_NT];
    __shared__ int sc[OF_NT];
    const int row = blockIdx.x, tid = threadIdx.x;
    const double *p = Pn + (size_t)row * M;
    double s = 0.0;
    int c = 0;
#pragma unroll 4
    for (int j = tid; j < M; j += OF_NT) {
        const double v = p[j];
        if (v == v) {
            s += v;
            ++c;
        }
    }
    sd[tid] = s;
    sc[tid] = c;
    of_tree(sd, sc, tid);
    if (tid == 0) mnp[row] = sc[0] ? sd[0] / (double)sc[0] : __longlong_as_double(0x7ff8000000000000ll);
}

// the closed form, one thread per target; the sample terms are added in order of k
__global__ __launch_bounds__(OF_NT) void overfit_metric_kernel(int B, int n_samples, const int *__restrict__ n_up,
                                                              const double *__restrict__ S, const double *__restrict__ mnp,
                                                              double *__restrict__ metric) {
    const int b = blockIdx.x * OF_NT + threadIdx.x;
    if (b >= B) return;
    const int nu = n_up[b];
    const double s = S[b];
    double acc = 0.0;
    for (int k = 0; k < n_samples; ++k) {
        double per = 0.0;
        if (nu != 0) {
            const double den = (double)nu * mnp[(size_t)k * B + b];
            per = den == 0.0 ? __longlong_as_double(0x7ff0000000000000ll) : s / den;
        }
        acc += per;
    }
    const double mean = acc / (double)n_samples;
    const double m = mean != mean ? mean : (mean > 0.0 ? mean : 0.0);   // numpy.max([mean, 0]): NaN stays NaN
    metric[b] = 2.0 / (1.0 + exp(m));
}

// ------------------------------------------------------------------------------------------------ scratch plan
namespace {
inline int of_blocks_per_row(int n) { return ((n + 1) / 2 + OF_NT - 1) / OF_NT; }

struct OverfitPlan {
    int R;   // samples per round
    size_t z0, z1, trel, g, p0, p1, pn, mean_unc, mnp, n_up, S, total;
};

inline size_t of_carve(size_t &used, size_t bytes) {
    const size_t at = used;
    used = (used + bytes + 255) & ~size_t(255);
    return at;
}

OverfitPlan of_layout(int B, int n, int64_t M, int n_samples, int R) {
    OverfitPlan p;
    const size_t rows = (size_t)B * n * 8, spec = (size_t)B * M * 8;
    size_t used = 0;
    p.R = R;
    p.z0 = of_carve(used, rows);
    p.z1 = of_carve(used, rows);
    p.trel = of_carve(used, rows * R);
    p.g = of_carve(used, rows * R);
    p.p0 = of_carve(used, spec);
    p.p1 = of_carve(used, spec);
    p.pn = of_carve(used, spec * R);
    p.mean_unc = of_carve(used, (size_t)B * 8);
    p.mnp = of_carve(used, (size_t)B * n_samples * 8);
    p.n_up = of_carve(used, (size_t)B * 4);
    p.S = of_carve(used, (size_t)B * 8);
    p.total = used;
    return p;
}

// the largest round that fits `budget` (and one launch: R B rows as an int); one sample per round when none fits
OverfitPlan of_plan(int B, int n, int64_t M, int n_samples, size_t budget) {
    const int64_t wg_per_sample = (int64_t)B * of_blocks_per_row(n);   // (the noise pass: one launch per round, 1-D grid)
    const int rmax = (int)std::min<int64_t>(n_samples, std::min<int64_t>(((int64_t)1 << 30) / B, (((int64_t)1 << 31) - 1) / wg_per_sample));
    int R = 1;
    for (int r = std::max(1, rmax); r > 1; --r)
        if (of_layout(B, n, M, n_samples, r).total <= budget) {
            R = r;
            break;
        }
    return of_layout(B, n, M, n_samples, R);
}
}  // namespace

static int overfit_shape_ok(int B, int n, int64_t M, int n_samples) {
    LK_REQUIRE(B >= 1 && B < (1 << 24), "B must be in [1, 2^24) (got %d)", B);
    LK_REQUIRE(n >= 3 && n < (1 << 30), "the over-fitting metric needs 3 <= n < 2^30 kept cadences (got %d)", n);
    LK_REQUIRE(M >= 2 && M < ((int64_t)1 << 24), "the frequency grid needs 2 <= M < 2^24 points (got %lld)", (long long)M);
    LK_REQUIRE(n_samples >= 1 && n_samples <= (1 << 20), "n_samples must be in [1, 2^20] (got %d)", n_samples);
    LK_REQUIRE((int64_t)B * of_blocks_per_row(n) < ((int64_t)1 << 31), "B x n = %d x %d is more than one noise launch covers", B, n);
    return LK_OK;
}

int overfit_scratch_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes, int *samples_per_round) {
    int rc = overfit_shape_ok(B, n, M, n_samples);
    if (rc) return rc;
    LK_REQUIRE(bytes != nullptr, "bytes is NULL");
    LK_REQUIRE(max_scratch_bytes >= 0, "max_scratch_bytes must be >= 0 (0: the default of %lld)", (long long)LK_OVERFIT_SCRATCH_DEFAULT);
    const OverfitPlan p = of_plan(B, n, M, n_samples, (size_t)(max_scratch_bytes ? max_scratch_bytes : LK_OVERFIT_SCRATCH_DEFAULT));
    *bytes = (int64_t)p.total;
    if (samples_per_round) *samples_per_round = p.R;
    return LK_OK;
}

static int overfit_rng_ok(int B, int64_t first_target, int64_t stream_id) {
    LK_REQUIRE(first_target >= 0 && first_target + B <= ((int64_t)1 << 32), "first_target + B must stay within 32 bits (got %lld + %d)",
               (long long)first_target, B);
    LK_REQUIRE(stream_id >= 0 && stream_id < ((int64_t)1 << 32), "stream_id must be in [0, 2^32) (got %lld)", (long long)stream_id);
    return LK_OK;
}

static void overfit_noise_rows(int B, int n, int nk, int k0, uint64_t seed, int64_t first_target, int64_t stream_id,
                               const double *mean_unc, double *g, hipStream_t stream) {
    const int bpr = of_blocks_per_row(n);
    hipLaunchKernelGGL(overfit_noise_kernel, dim3((unsigned)((size_t)nk * B * bpr)), dim3(OF_NT), 0, stream, B, n, bpr, k0,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)first_target, (uint32_t)stream_id, mean_unc, g);
}

int overfit_noise_launch(lk_handle *h, int B, int n, int k, uint64_t seed, int64_t first_target, int64_t stream_id, double *out,
                         hipStream_t stream) {
    LK_REQUIRE(B >= 1 && B < (1 << 24), "B must be in [1, 2^24) (got %d)", B);
    LK_REQUIRE(n >= 1 && n < (1 << 30), "n must be in [1, 2^30) (got %d)", n);
    LK_REQUIRE(k >= 0, "the sample index must be >= 0 (got %d)", k);
    LK_REQUIRE(out != nullptr && ((uintptr_t)out & 15) == 0, "out must be a 16-byte aligned device buffer");
    LK_REQUIRE((int64_t)B * of_blocks_per_row(n) < ((int64_t)1 << 31), "B x n = %d x %d is more than one noise launch covers", B, n);
    int rc = overfit_rng_ok(B, first_target, stream_id);
    if (rc) return rc;
    overfit_noise_rows(B, n, 1, k, seed, first_target, stream_id, nullptr, out, stream);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int overfit_metric_launch(lk_handle *h, int B, int N, const double *time, const double *flux_orig, const double *flux_corr,
                          const double *err_corr, int n, const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples,
                          uint64_t seed, int64_t first_target, int64_t stream_id, void *scratch, int64_t scratch_bytes,
                          double *metric, hipStream_t stream) {
    int rc = overfit_shape_ok(B, n, M, n_samples);
    if (rc) return rc;
    LK_REQUIRE(N >= n && N < (1 << 30), "need n <= N < 2^30 (got n=%d, N=%d)", n, N);
    LK_REQUIRE(keep_idx != nullptr || n == N, "keep_idx is NULL (all cadences) but n=%d != N=%d", n, N);
    LK_REQUIRE(time && flux_orig && flux_corr && err_corr && metric, "NULL buffer");
    LK_REQUIRE(f0 >= 0.0 && df > 0.0, "the grid needs f0 >= 0 and df > 0 (got f0=%g, df=%g)", f0, df);
    if ((rc = overfit_rng_ok(B, first_target, stream_id))) return rc;
    LK_REQUIRE(scratch != nullptr && ((uintptr_t)scratch & 255) == 0, "scratch must be a 256-byte aligned device buffer");
    LK_REQUIRE(scratch_bytes >= 0, "scratch_bytes must be >= 0");
    const OverfitPlan p = of_plan(B, n, M, n_samples, (size_t)scratch_bytes);
    LK_REQUIRE(p.total <= (size_t)scratch_bytes, "scratch too small: %lld bytes given, one sample per round needs %lld "
               "(lk_overfit_scratch_bytes)", (long long)scratch_bytes, (long long)p.total);
    char *base = static_cast<char *>(scratch);
    auto at = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    double *d_z0 = at(p.z0), *d_z1 = at(p.z1), *d_t = at(p.trel), *d_g = at(p.g), *d_p0 = at(p.p0), *d_p1 = at(p.p1), *d_pn = at(p.pn);
    double *d_mu = at(p.mean_unc), *d_mnp = at(p.mnp), *d_S = at(p.S);
    int *d_nup = reinterpret_cast<int *>(base + p.n_up);
    const int R = p.R;
    std::vector<int64_t> off((size_t)R * B + 1);
    for (size_t r = 0; r < off.size(); ++r) off[r] = (int64_t)r * n;

    hipLaunchKernelGGL(overfit_prepare_kernel, dim3(B), dim3(OF_PREP_NT), 0, stream, time, flux_orig, flux_corr, err_corr, N, n,
                       keep_idx, B, R, d_z0, d_z1, d_t, d_mu);
    LK_HIP_CHECK(hipGetLastError());
    auto ls = [&](int rows, const double *y, double *power) {
        return lsfast_launch(h, rows, off.data(), d_t, y, nullptr, f0, df, M, 1, 1, LK_NORM_LK_AMPLITUDE, nullptr, 5, power, stream);
    };
    if ((rc = ls(B, d_z0, d_p0))) return rc;
    if ((rc = ls(B, d_z1, d_p1))) return rc;
    hipLaunchKernelGGL(overfit_change_kernel, dim3(B), dim3(OF_NT), 0, stream, (const double *)d_p0, (const double *)d_p1, (int)M,
                       d_nup, d_S);
    for (int k0 = 0; k0 < n_samples; k0 += R) {
        const int nk = std::min(R, n_samples - k0);
        overfit_noise_rows(B, n, nk, k0, seed, first_target, stream_id, d_mu, d_g, stream);
        LK_HIP_CHECK(hipGetLastError());
        if ((rc = ls(nk * B, d_g, d_pn))) return rc;
        hipLaunchKernelGGL(overfit_noise_mean_kernel, dim3((unsigned)(nk * B)), dim3(OF_NT), 0, stream, (const double *)d_pn, (int)M,
                           d_mnp + (size_t)k0 * B);
    }
    hipLaunchKernelGGL(overfit_metric_kernel, dim3((B + OF_NT - 1) / OF_NT), dim3(OF_NT), 0, stream, B, n_samples,
                       (const int *)d_nup, (const double *)d_S, (const double *)d_mnp, metric);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
