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
#include "philox.hpp"

#include <algorithm>
#include <cmath>

namespace lk {

constexpr int OF_PREP_NT = 1024;   // prepare: block_median wants a wide workgroup (two selects over n gathered values)
constexpr int OF_NT = 256;         // noise and spectra passes

// ------------------------------------------------------------------------------------------------ prepare
// One workgroup per target: exact medians of the kept cadences of both fluxes, the packed rows z0[b], z1[b], the rebased
// times t - t[first kept] (written R times: rows (r, b) of the time block serve the R x B noise rows of a round, rows (0, b)
// the two flux launches), and mean_unc[b].  A session does it in two halves: y1 == NULL writes z0 and the times alone (begin),
// y0 == NULL writes z1 and mean_unc alone (every evaluation); each half does what the whole does to its own outputs.
//
// Where a target's rows start is the one thing a batch's layout decides.  Target b's cadences are [n_off[b], n_off[b + 1]) of the
// inputs, its kept ones keep_idx[k_off[b] .. k_off[b + 1]) (target-relative, ascending; keep_idx == NULL: all), and its packed row
// starts at element k_off[b] of a block of cad = k_off[B] elements (round r of the times and of the noise: r cad + k_off[b]).
// n_off == NULL is the uniform batch: n_off[b] = b N, k_off[b] = b n, cad = B n and ONE keep_idx serves every target; it reads no
// table.  b is uniform over the workgroup, so the choice is a scalar branch.
__global__ __launch_bounds__(OF_PREP_NT) void overfit_prepare_kernel(const double *__restrict__ time, const double *__restrict__ y0,
                                                                    const double *__restrict__ y1, const double *__restrict__ e1,
                                                                    int N, int n, const int64_t *__restrict__ n_off,
                                                                    const int32_t *__restrict__ keep_idx,
                                                                    const int64_t *__restrict__ k_off, int64_t cad, int R,
                                                                    double *__restrict__ z0, double *__restrict__ z1,
                                                                    double *__restrict__ trel, double *__restrict__ mean_unc) {
    __shared__ unsigned long long sh[OF_PREP_NT];
    __shared__ int sh_cnt[OF_PREP_NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ragged = n_off != nullptr;
    const size_t in = ragged ? (size_t)n_off[b] : (size_t)b * N, out = ragged ? (size_t)k_off[b] : (size_t)b * n;
    if (ragged) n = (int)(k_off[b + 1] - k_off[b]);
    const int32_t *kb = keep_idx ? keep_idx + (ragged ? out : 0) : nullptr;
    auto idx = [&](int i) { return kb ? kb[i] : i; };
    auto all = [&](int) { return true; };
    double med0 = 0.0, med1 = 0.0, t0 = 0.0;   // (y0, y1: uniform over the grid)
    if (y0) {
        med0 = block_median(n, (long long)n, [&](int i) { return y0[in + idx(i)]; }, all, sh);
        __syncthreads();
        t0 = time[in + idx(0)];
    }
    if (y1) {
        med1 = block_median(n, (long long)n, [&](int i) { return y1[in + idx(i)]; }, all, sh);
        __syncthreads();
    }
    double s = 0.0;
    int cnt = 0;
    for (int i = tid; i < n; i += OF_PREP_NT) {
        const int j = idx(i);
        // y / med - 1.0 as two separately rounded operations (a zero median gives non-finite rows, as in the reference)
        if (y0) {
            z0[out + i] = __dsub_rn(__ddiv_rn(y0[in + j], med0), 1.0);
            const double tr = __dsub_rn(time[in + j], t0);
            for (int r = 0; r < R; ++r) trel[(size_t)r * (size_t)cad + out + i] = tr;
        }
        if (y1) {
            z1[out + i] = __dsub_rn(__ddiv_rn(y1[in + j], med1), 1.0);
            const double u = __ddiv_rn(e1[in + j], med1);
            if (u == u) {
                s += u;
                ++cnt;
            }
        }
    }
    if (!y1) return;
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
// Rows (kk, b), kk < nk: g[kk cad + k_off[b] + c] = normal(target first_target + b, sample k0 + kk, kept cadence c of that target)
// * mean_unc[b] (mean_unc == NULL: the normals themselves); k_off == NULL: the uniform batch, k_off[b] = b n.  One thread = one
// Philox call = cadences 2i and 2i + 1, so any (target, sample, cadence) gets the same number on either layout; bpr workgroups
// per row, sized by the longest row: the ones past a shorter row's end leave at once.
// A row starts 16-byte aligned when its first element index is even: then the pair goes out as one 16-byte store.
__global__ __launch_bounds__(OF_NT) void overfit_noise_kernel(int B, int n, const int64_t *__restrict__ k_off, int64_t cad, int bpr,
                                                             int k0, uint32_t key0, uint32_t key1, uint32_t first_target,
                                                             uint32_t stream_id, const double *__restrict__ mean_unc,
                                                             double *__restrict__ g) {
    const int row = blockIdx.x / bpr, i = (blockIdx.x - row * bpr) * OF_NT + threadIdx.x;
    const int kk = row / B, b = row - kk * B;
    if (k_off) n = (int)(k_off[b + 1] - k_off[b]);
    const int c = 2 * i;
    if (c >= n) return;
    double a, s;
    philox_normal_pair(philox4x32_10((uint32_t)i, (uint32_t)(k0 + kk), first_target + (uint32_t)b, stream_id, key0, key1), a, s);
    const double mu = mean_unc ? mean_unc[b] : 1.0;
    a *= mu;
    s *= mu;
    const size_t base = (size_t)kk * (size_t)cad + (k_off ? (size_t)k_off[b] : (size_t)b * n);
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

// the closed form, one thread per target; the sample terms are added in order of k.  mean_unc == NULL: mnp holds the noise
// spectra's means themselves; else mnp holds those of the UNIT normals (a session's u_k) and the mean is |mean_unc[b]| * u_k:
// the amplitude-normalised periodogram is homogeneous of degree one in its input.
__global__ __launch_bounds__(OF_NT) void overfit_metric_kernel(int B, int n_samples, const int *__restrict__ n_up,
                                                              const double *__restrict__ S, const double *__restrict__ mnp,
                                                              const double *__restrict__ mean_unc, double *__restrict__ metric) {
    const int b = blockIdx.x * OF_NT + threadIdx.x;
    if (b >= B) return;
    const int nu = n_up[b];
    const double s = S[b];
    const double amp = mean_unc ? fabs(mean_unc[b]) : 1.0;
    double acc = 0.0;
    for (int k = 0; k < n_samples; ++k) {
        double per = 0.0;
        if (nu != 0) {
            const double mk = mnp[(size_t)k * B + b];
            const double den = (double)nu * (mean_unc ? amp * mk : mk);
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
    size_t z0, z1, trel, g, p0, p1, pn, mean_unc, mnp, n_up, S, offs, total;
};

inline size_t of_carve(size_t &used, size_t bytes) {
    const size_t at = used;
    used = (used + bytes + 255) & ~size_t(255);
    return at;
}

// cad: the kept cadences of all B targets together (B n for a uniform batch); offs: the ragged flavours also keep the batch's
// two offset tables (2 (B + 1) int64) in the block, after everything else
OverfitPlan of_layout(int B, size_t cad, int64_t M, int n_samples, int R, bool offs) {
    OverfitPlan p;
    const size_t rows = cad * 8, spec = (size_t)B * M * 8;
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
    p.offs = offs ? of_carve(used, 2 * ((size_t)B + 1) * 8) : used;
    p.total = used;
    return p;
}

// the largest round that fits `budget` (and one launch: R B rows as an int); one sample per round when none fits
// nmax: the longest row (n for a uniform batch)
OverfitPlan of_plan(int B, size_t cad, int nmax, int64_t M, int n_samples, size_t budget, bool offs) {
    const int64_t wg_per_sample = (int64_t)B * of_blocks_per_row(nmax);   // (the noise pass: one launch per round, 1-D grid)
    const int rmax = (int)std::min<int64_t>(n_samples, std::min<int64_t>(((int64_t)1 << 30) / B, (((int64_t)1 << 31) - 1) / wg_per_sample));
    int R = 1;
    for (int r = std::max(1, rmax); r > 1; --r)
        if (of_layout(B, cad, M, n_samples, r, offs).total <= budget) {
            R = r;
            break;
        }
    return of_layout(B, cad, M, n_samples, R, offs);
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
    const OverfitPlan p = of_plan(B, (size_t)B * n, n, M, n_samples,
                                  (size_t)(max_scratch_bytes ? max_scratch_bytes : LK_OVERFIT_SCRATCH_DEFAULT), false);
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

// nk samples from k0 on, one launch.  n: the longest row; d_koff: the kept offsets on the device, NULL for a uniform batch
static void overfit_noise_rows(int B, int n, const int64_t *d_koff, size_t cad, int nk, int k0, uint64_t seed, int64_t first_target,
                               int64_t stream_id, const double *mean_unc, double *g, hipStream_t stream) {
    const int bpr = of_blocks_per_row(n);
    hipLaunchKernelGGL(overfit_noise_kernel, dim3((unsigned)((size_t)nk * B * bpr)), dim3(OF_NT), 0, stream, B, n, d_koff, (int64_t)cad,
                       bpr, k0, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)first_target, (uint32_t)stream_id,
                       mean_unc, g);
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
    overfit_noise_rows(B, n, nullptr, (size_t)B * n, 1, k, seed, first_target, stream_id, nullptr, out, stream);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ the batch's own offsets
// k_off_host: the B + 1 offsets of the kept cadences; keep_idx == NULL keeps all and k_off_host may be NULL or n_off_host.
static int overfit_rows_ok(int B, const int64_t *n_off_host, const int32_t *keep_idx, const int64_t *&k_off_host, int64_t M,
                           int n_samples, int *nmax) {
    LK_REQUIRE(B >= 1 && B < (1 << 24), "B must be in [1, 2^24) (got %d)", B);
    LK_REQUIRE(n_off_host != nullptr && n_off_host[0] == 0, "n_off must be given and start at 0");
    if (k_off_host == nullptr) {
        LK_REQUIRE(keep_idx == nullptr, "keep_idx is given without k_off");
        k_off_host = n_off_host;
    }
    LK_REQUIRE(k_off_host[0] == 0, "k_off must start at 0");
    *nmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t N = n_off_host[b + 1] - n_off_host[b], n = k_off_host[b + 1] - k_off_host[b];
        LK_REQUIRE(N >= 0 && N < (1 << 30), "target %d: %lld cadences outside 0..2^30", b, (long long)N);
        LK_REQUIRE(n >= 3, "target %d: the over-fitting metric needs at least 3 kept cadences (got %lld)", b, (long long)n);
        LK_REQUIRE(n <= N && (keep_idx != nullptr || n == N), "target %d keeps %lld of %lld cadences%s", b, (long long)n, (long long)N,
                   keep_idx ? "" : " but keep_idx is NULL (all cadences)");
        *nmax = std::max(*nmax, (int)n);
    }
    LK_REQUIRE(M >= 2 && M < ((int64_t)1 << 24), "the frequency grid needs 2 <= M < 2^24 points (got %lld)", (long long)M);
    LK_REQUIRE(n_samples >= 1 && n_samples <= (1 << 20), "n_samples must be in [1, 2^20] (got %d)", n_samples);
    LK_REQUIRE((int64_t)B * of_blocks_per_row(*nmax) < ((int64_t)1 << 31), "B x n = %d x %d is more than one noise launch covers", B,
               *nmax);
    return LK_OK;
}

int overfit_scratch_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                               int *samples_per_round) {
    int nmax = 0;
    LK_REQUIRE(k_off_host != nullptr, "k_off is NULL (the offsets of the kept cadences; the batch's own when all are kept)");
    const int64_t *k = k_off_host;
    int rc = overfit_rows_ok(B, k_off_host, nullptr, k, M, n_samples, &nmax);
    if (rc) return rc;
    LK_REQUIRE(bytes != nullptr, "bytes is NULL");
    LK_REQUIRE(max_scratch_bytes >= 0, "max_scratch_bytes must be >= 0 (0: the default of %lld)", (long long)LK_OVERFIT_SCRATCH_DEFAULT);
    const OverfitPlan p = of_plan(B, (size_t)k_off_host[B], nmax, M, n_samples,
                                  (size_t)(max_scratch_bytes ? max_scratch_bytes : LK_OVERFIT_SCRATCH_DEFAULT), true);
    *bytes = (int64_t)p.total;
    if (samples_per_round) *samples_per_round = p.R;
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ one call
// The checks every launcher below starts with, each flavour's own first and in its own order.  A ragged batch comes out with
// k_off_host set (n_off_host when all cadences are kept) and n = its longest row.
static int overfit_batch_ok(OverfitBatch &bt, double f0, double df, int64_t M, int n_samples, const void *block, int64_t bytes) {
    if (bt.ragged) {
        if (const int rc = overfit_rows_ok(bt.B, bt.n_off_host, bt.keep_idx, bt.k_off_host, M, n_samples, &bt.n)) return rc;
    } else {
        if (const int rc = overfit_shape_ok(bt.B, bt.n, M, n_samples)) return rc;
        LK_REQUIRE(bt.N >= bt.n && bt.N < (1 << 30), "need n <= N < 2^30 (got n=%d, N=%d)", bt.n, bt.N);
        LK_REQUIRE(bt.keep_idx != nullptr || bt.n == bt.N, "keep_idx is NULL (all cadences) but n=%d != N=%d", bt.n, bt.N);
    }
    LK_REQUIRE(f0 >= 0.0 && df > 0.0, "the grid needs f0 >= 0 and df > 0 (got f0=%g, df=%g)", f0, df);
    LK_REQUIRE(block != nullptr && ((uintptr_t)block & 255) == 0, "scratch must be a 256-byte aligned device buffer");
    LK_REQUIRE(bytes >= 0, "scratch_bytes must be >= 0");
    const OverfitPlan p = of_plan(bt.B, bt.cad(), bt.n, M, n_samples, (size_t)bytes, bt.ragged);
    LK_REQUIRE(p.total <= (size_t)bytes, "scratch too small: %lld bytes given, one sample per round needs %lld (%s)", (long long)bytes,
               (long long)p.total, bt.ragged ? "lk_overfit_scratch_rows_bytes" : "lk_overfit_scratch_bytes");
    return LK_OK;
}

namespace {
// one call's view of the caller-owned block and the steps the unsplit metric and a session share
struct OverfitRun {
    lk_handle *h;
    OverfitBatch bt;       // as overfit_batch_ok left it
    int B, n, n_samples;   // n: the kept cadences of every target; of the longest one when the batch is ragged
    double f0, df;
    int64_t M;
    hipStream_t stream;
    size_t cad;            // the kept cadences of all targets together
    OverfitPlan p;
    char *base;
    std::vector<int64_t> off;   // row offsets of the largest launch (R B rows: row (r, b) starts at r cad + the kept offset of b)

    OverfitRun(lk_handle *h_, const OverfitBatch &bt_, double f0_, double df_, int64_t M_, int n_samples_, void *block, size_t bytes,
               hipStream_t st)
        : h(h_), bt(bt_), B(bt_.B), n(bt_.n), n_samples(n_samples_), f0(f0_), df(df_), M(M_), stream(st), cad(bt_.cad()),
          p(of_plan(B, cad, n, M_, n_samples_, bytes, bt_.ragged)), base(static_cast<char *>(block)), off((size_t)p.R * B + 1) {
        for (int r = 0; r < p.R; ++r)
            for (int b = 0; b < B; ++b)
                off[(size_t)r * B + b] = (int64_t)r * (int64_t)cad + (bt.ragged ? bt.k_off_host[b] : (int64_t)b * n);
        off.back() = (int64_t)p.R * (int64_t)cad;
    }
    double *at(size_t o) const { return reinterpret_cast<double *>(base + o); }
    int *n_up() const { return reinterpret_cast<int *>(base + p.n_up); }
    // ragged: the batch's offsets on the device, then the kept cadences' offsets; a uniform block has neither (NULL: the kernels
    // compute them)
    const int64_t *d_noff() const { return bt.ragged ? reinterpret_cast<const int64_t *>(base + p.offs) : nullptr; }
    const int64_t *d_koff() const { return bt.ragged ? d_noff() + B + 1 : nullptr; }

    // ragged: both offset tables into the block (captured before the call returns), once per block
    int upload_offsets() const {
        if (!bt.ragged) return LK_OK;
        int64_t *d = reinterpret_cast<int64_t *>(base + p.offs);
        if (const int rc = h->stage.copy(d, bt.n_off_host, ((size_t)B + 1) * 8, stream)) return rc;
        return h->stage.copy(d + B + 1, bt.k_off_host, ((size_t)B + 1) * 8, stream);
    }
    int prepare(const double *time, const double *y0, const double *y1, const double *e1) const {
        hipLaunchKernelGGL(overfit_prepare_kernel, dim3(B), dim3(OF_PREP_NT), 0, stream, time, y0, y1, e1, bt.N, n, d_noff(), bt.keep_idx,
                           d_koff(), (int64_t)cad, p.R, at(p.z0), at(p.z1), at(p.trel), at(p.mean_unc));
        LK_HIP_CHECK(hipGetLastError());
        return LK_OK;
    }
    int ls(int rows, const double *y, double *power) const {
        return lsfast_launch(h, rows, off.data(), at(p.trel), y, nullptr, f0, df, M, 1, 1, LK_NORM_LK_AMPLITUDE, nullptr, 5, power, stream);
    }
    // P1, then n_up and S against P0
    int change() const {
        if (const int rc = ls(B, at(p.z1), at(p.p1))) return rc;
        hipLaunchKernelGGL(overfit_change_kernel, dim3(B), dim3(OF_NT), 0, stream, (const double *)at(p.p0), (const double *)at(p.p1),
                           (int)M, n_up(), at(p.S));
        return LK_OK;
    }
    // mnp[k][b] = nanmean(LS of sample k's normals times scale[b]) (scale == NULL: the unit normals), in rounds of R samples
    int noise_means(uint64_t seed, int64_t first_target, int64_t stream_id, const double *scale) const {
        for (int k0 = 0; k0 < n_samples; k0 += p.R) {
            const int nk = std::min(p.R, n_samples - k0);
            overfit_noise_rows(B, n, d_koff(), cad, nk, k0, seed, first_target, stream_id, scale, at(p.g), stream);
            LK_HIP_CHECK(hipGetLastError());
            if (const int rc = ls(nk * B, at(p.g), at(p.pn))) return rc;
            hipLaunchKernelGGL(overfit_noise_mean_kernel, dim3((unsigned)(nk * B)), dim3(OF_NT), 0, stream, (const double *)at(p.pn),
                               (int)M, at(p.mnp) + (size_t)k0 * B);
        }
        return LK_OK;
    }
    int metric(const double *amp, double *out) const {
        hipLaunchKernelGGL(overfit_metric_kernel, dim3((B + OF_NT - 1) / OF_NT), dim3(OF_NT), 0, stream, B, n_samples,
                           (const int *)n_up(), (const double *)at(p.S), (const double *)at(p.mnp), amp, out);
        LK_HIP_CHECK(hipGetLastError());
        return LK_OK;
    }
};
}  // namespace

int overfit_metric_launch(lk_handle *h, OverfitBatch bt, const double *time, const double *flux_orig, const double *flux_corr,
                          const double *err_corr, double f0, double df, int64_t M, int n_samples, uint64_t seed, int64_t first_target,
                          int64_t stream_id, void *scratch, int64_t scratch_bytes, double *metric, hipStream_t stream) {
    int rc = overfit_batch_ok(bt, f0, df, M, n_samples, scratch, scratch_bytes);
    if (rc) return rc;
    LK_REQUIRE(time && flux_orig && flux_corr && err_corr && metric, "NULL buffer");
    if ((rc = overfit_rng_ok(bt.B, first_target, stream_id))) return rc;
    const OverfitRun run(h, bt, f0, df, M, n_samples, scratch, (size_t)scratch_bytes, stream);
    if ((rc = run.upload_offsets())) return rc;
    if ((rc = run.prepare(time, flux_orig, flux_corr, err_corr))) return rc;
    if ((rc = run.ls(bt.B, run.at(run.p.z0), run.at(run.p.p0)))) return rc;
    if ((rc = run.change())) return rc;
    if ((rc = run.noise_means(seed, first_target, stream_id, run.at(run.p.mean_unc)))) return rc;
    return run.metric(nullptr, metric);
}

// ------------------------------------------------------------------------------------------------ session
// The metric in two halves for a caller that scores MANY corrections of one original batch with one noise stream (the ridge
// search): begin takes everything that does not depend on the correction (z0, the times, P0 and u_k = nanmean(LS of the unit
// normals of sample k)); an evaluation packs z1 and mean_unc, takes P1 in ONE launch of B rows and closes the form with
// mnp_k = |mean_unc| * u_k.  P0 and P1 are the bits of the unsplit call, so n_up and S are too; only mnp_k differs, by the
// rounding of nanmean(LS(normal * mean_unc)) against |mean_unc| * nanmean(LS(normal)).  Edge rules: a NaN mean_unc gives a NaN
// noise mean (a NaN metric) and a zero one a zero noise mean (per_k = inf, metric 0) when n_up > 0; n_up == 0 gives 0.  The
// block has the layout of the unsplit call's scratch (same size, same rounds); an evaluation writes z1, P1, mean_unc, n_up and
// S and nothing that begin wrote.  Ragged: begin also puts the two offset tables into the block, and an evaluation reads them
// there (its own n_off_host / k_off_host must be begin's: they size the plan and the periodogram launch).
int overfit_session_begin_launch(lk_handle *h, OverfitBatch bt, const double *time, const double *flux_orig, double f0, double df,
                                 int64_t M, int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *session,
                                 int64_t session_bytes, hipStream_t stream) {
    int rc = overfit_batch_ok(bt, f0, df, M, n_samples, session, session_bytes);
    if (rc) return rc;
    LK_REQUIRE(time && flux_orig, "NULL buffer");
    if ((rc = overfit_rng_ok(bt.B, first_target, stream_id))) return rc;
    const OverfitRun run(h, bt, f0, df, M, n_samples, session, (size_t)session_bytes, stream);
    if ((rc = run.upload_offsets())) return rc;
    if ((rc = run.prepare(time, flux_orig, nullptr, nullptr))) return rc;
    if ((rc = run.ls(bt.B, run.at(run.p.z0), run.at(run.p.p0)))) return rc;
    return run.noise_means(seed, first_target, stream_id, nullptr);
}

int overfit_session_eval_launch(lk_handle *h, OverfitBatch bt, const double *flux_corr, const double *err_corr, double f0, double df,
                                int64_t M, int n_samples, void *session, int64_t session_bytes, double *metric, hipStream_t stream) {
    int rc = overfit_batch_ok(bt, f0, df, M, n_samples, session, session_bytes);
    if (rc) return rc;
    LK_REQUIRE(flux_corr && err_corr && metric, "NULL buffer");
    const OverfitRun run(h, bt, f0, df, M, n_samples, session, (size_t)session_bytes, stream);
    if ((rc = run.prepare(nullptr, nullptr, flux_corr, err_corr))) return rc;
    if ((rc = run.change())) return rc;
    return run.metric(run.at(run.p.mean_unc), metric);
}

}  // namespace lk
