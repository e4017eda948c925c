// fillgaps.hip — LightCurve.fill_gaps (lightkurve 2.x lightcurve.py, method="gaussian_noise") for a ragged batch on gfx950, and
// the segment gather behind DeviceLightCurveBatch.stitch (LightCurveCollection.stitch: a vstack of the corrected segments).
//
//   fill_gaps_plan_launch    per light curve: m = median(diff(time)) (exact), mu = nanmean(flux), sd = nanstd(flux), where every
//                            original cadence lands in the filled light curve (pos) and how long that one is (new_off)
//   fill_gaps_launch         the filled columns and the byte mask of the inserted cadences
//   gather_segments_launch   S segments of up to 8 columns from one packed layout into another, one launch
//
// Two paths, chosen by the cadence numbers being there or not (include/lkhip.h has the reference's arithmetic in full):
//   time       prev = t[0]; for every next original t: while (t - prev) > 1.2 m: insert prev + m, prev = that; then t.  The chain
//              of additions of one gap is serial and belongs to ONE lane, in the plan pass (its length) and in the fill pass (its
//              times); everything else is parallel over cadences.
//   cadenceno  every cadence number of [c_first, c_last]; times from d = t - m c, linear in c between the gap's two originals
//              (np.interp's expression), plus m c.  Originals are recomputed the same way, as the reference does.
// Inserted cadences: flux_err linear in time between the gap's originals (np.interp's expression on the ORIGINAL times), quality
// 65536, flux = noise_mean + noise_std * normal, normal = philox.hpp's with counter (pair of inserted cadences of that light
// curve, 0, first_target + b, stream_id): inserted cadence 2i takes the cosine normal, 2i + 1 the sine normal.
//
// Built with -ffp-contract=off: every product and sum above rounds on its own, as numpy's.  Summation orders (mu, sd): thread j
// of 512 adds elements j, j + 512, ... ascending, then a halving tree: a function of the light curve's length alone.  No
// floating-point atomics; every cadence is computed from its own light curve's values alone, so a target's output does not depend
// on B, its neighbours or the launch shape.
#include <algorithm>
#include <climits>
#include <cmath>

#include "block_select.hpp"
#include "lk_common.hpp"
#include "philox.hpp"

namespace lk {

constexpr int FG_NT = 512;                      // plan: a power of two (block_sum_dyn); block_median_sampled as bls_prepare_kernel
constexpr int FG_CAND = 4096;                   // plan: LDS candidates of the sampled median (doubles)
constexpr int FG_TILE = 1024;                   // fill: output cadences a workgroup sweeps at a time
constexpr int FG_FILL_NT = 256;                 // fill: threads per chunk of a light curve
constexpr int64_t FG_MAX_N = (int64_t)1 << 30;  // cadences per light curve, before and after
constexpr int FG_MAX_GAP = 1 << 20;             // inserted cadences of ONE gap (one lane walks them)
constexpr int FG_QUALITY_INSERTED = 65536;

enum { FG_BAD_TIME = 1, FG_BAD_CADENCENO = 2, FG_BAD_LENGTH = 3 };

// ------------------------------------------------------------------------------------------------ plan
// stats[4 b ..] = m, mu, sd, n_inserted.  pos[n_off[b] + i] = index of original i inside the filled light curve.  bad[0]
// (all ones before) = min over the refused light curves of 4 b + reason; a refused one plans no insertion.
__global__ __launch_bounds__(FG_NT) void fill_gaps_plan_kernel(const double *__restrict__ time, const double *__restrict__ flux,
                                                               const int32_t *__restrict__ cad, const int64_t *__restrict__ n_off,
                                                               double *__restrict__ stats, int32_t *__restrict__ pos,
                                                               int64_t *__restrict__ count, unsigned long long *__restrict__ bad) {
    __shared__ __attribute__((aligned(16))) unsigned long long sh[FG_NT];
    __shared__ __attribute__((aligned(16))) double cand[FG_CAND];
    __shared__ int shi[FG_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    time += lo, flux += lo, pos += lo;
    if (cad) cad += lo;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // ---- mu, sd over the finite-or-infinite (not NaN) fluxes
    double part = 0.0;
    long long cnt = 0;
    for (int i = tid; i < n; i += FG_NT) {
        const double v = flux[i];
        if (v == v) part += v, ++cnt;
    }
    const long long nf = block_count_dyn(cnt, reinterpret_cast<long long *>(sh));
    const double mu = nf ? block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)nf : nan;
    part = 0.0;
    for (int i = tid; i < n; i += FG_NT) {
        const double v = flux[i];
        if (v == v) {
            const double d = v - mu;
            part += d * d;
        }
    }
    const double sd = nf ? sqrt(block_sum_dyn(part, reinterpret_cast<double *>(sh)) / (double)nf) : nan;
    auto finish = [&](double m, long long inserted) {
        if (tid == 0) {
            stats[4 * b] = m, stats[4 * b + 1] = mu, stats[4 * b + 2] = sd, stats[4 * b + 3] = (double)inserted;
            count[b] = n + inserted;
        }
    };
    auto refuse = [&](double m, int why) {  // (uniform)
        for (int i = tid; i < n; i += FG_NT) pos[i] = i;
        if (tid == 0) atomicMin(bad, (unsigned long long)b * 4ull + (unsigned long long)why);
        finish(m, 0);
    };
    if (n < 2) {  // comes back unchanged
        if (tid == 0 && n == 1) pos[0] = 0;
        finish(nan, 0);
        return;
    }
    auto all = [&](int) { return true; };
    // (about one pass over the steps; block_median's radix select took eight and 0.5 ms at 1000 x 20 000)
    const double m = block_median_sampled(n - 1, (long long)(n - 1), [&](int i) { return time[i + 1] - time[i]; }, all, sh, cand, FG_CAND);
    __syncthreads();
    // ---- the order the path needs
    cnt = 0;
    for (int i = tid; i < n - 1; i += FG_NT) cnt += cad ? (cad[i + 1] <= cad[i] ? 1 : 0) : (time[i + 1] < time[i] ? 1 : 0);
    if (block_count_dyn(cnt, reinterpret_cast<long long *>(sh)) > 0) {
        refuse(m, cad ? FG_BAD_CADENCENO : FG_BAD_TIME);
        return;
    }
    if (cad) {
        const int64_t c0 = cad[0], span = (int64_t)cad[n - 1] - c0 + 1;
        if (span >= FG_MAX_N) {
            refuse(m, FG_BAD_LENGTH);
            return;
        }
        for (int i = tid; i < n; i += FG_NT) pos[i] = (int32_t)((int64_t)cad[i] - c0);
        finish(m, span - n);
        return;
    }
    // ---- time path: the length of every gap's chain (one lane per gap), scanned in tiles of FG_NT gaps
    const double thr = 1.2 * m;
    long long carry = 0, toolong = 0;
    if (tid == 0) pos[0] = 0;
    for (int i0 = 0; i0 < n - 1; i0 += FG_NT) {
        const int i = i0 + tid;
        int g = 0;
        if (i < n - 1) {
            const double t0 = time[i], t1 = time[i + 1];
            if ((t1 - t0) > thr) {
                if (!(m > 0.0) || !((t1 - t0) / m < (double)FG_MAX_GAP)) {
                    toolong = 1;
                } else {
                    double prev = t0;
                    while ((t1 - prev) > thr) {
                        const double nx = prev + m;
                        if (nx == prev || g >= FG_MAX_GAP) {  // the chain does not advance / runs away
                            toolong = 1;
                            break;
                        }
                        prev = nx;
                        ++g;
                    }
                }
            }
        }
        int tot;
        const int ex = block_exscan_int(g, shi, &tot);
        if (i < n - 1) pos[i + 1] = (int32_t)((long long)(i + 1) + carry + ex + g);
        carry += tot;
        if (carry + n >= FG_MAX_N) toolong = 1;
    }
    __syncthreads();
    if (block_count_dyn(toolong, reinterpret_cast<long long *>(sh)) > 0) {
        __syncthreads();
        refuse(m, FG_BAD_LENGTH);
        return;
    }
    finish(m, carry);
}

int fill_gaps_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                          const int32_t *cadenceno, double *stats, int32_t *pos, int64_t *new_off_host, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr && new_off_host != nullptr, "bad batch description");
    if (B == 0) {
        new_off_host[0] = 0;
        return LK_OK;
    }
    LK_REQUIRE(n_off_host[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(n >= 0 && n < FG_MAX_N, "target %d has %lld cadences", b, (long long)n);
    }
    LK_REQUIRE(stats != nullptr, "stats is NULL");
    LK_REQUIRE((time && flux && pos) || n_off_host[B] == 0, "NULL buffer");
    int64_t *d_off, *d_cnt, *d_new;
    unsigned long long *d_bad;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).buf(d_cnt, B + 1).buf(d_new, B + 1).buf(d_bad, 1).carve(stream))
        return rc;
    LK_HIP_CHECK(hipMemsetAsync(d_bad, 0xff, 8, stream));
    hipLaunchKernelGGL(fill_gaps_plan_kernel, dim3(B), dim3(FG_NT), 0, stream, time, flux, cadenceno, d_off, stats, pos, d_cnt, d_bad);
    exscan_i64_launch(d_cnt, B, d_new, stream);
    unsigned long long bad = 0;
    LK_HIP_CHECK(hipMemcpyAsync(new_off_host, d_new, (size_t)(B + 1) * 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));  // the caller sizes the filled batch from the new offsets
    LK_HIP_CHECK(hipGetLastError());
    if (bad != ~0ull) {
        const long long b = (long long)(bad >> 2);
        const int why = (int)(bad & 3);
        LK_REQUIRE(why != FG_BAD_TIME, "fill_gaps needs the light curve sorted by time: light curve %lld is not", b);
        LK_REQUIRE(why != FG_BAD_CADENCENO, "fill_gaps by cadence number: the cadence numbers of light curve %lld are not strictly increasing", b);
        LK_REQUIRE(false, "fill_gaps: light curve %lld would get a gap of more than %d or a length of more than %lld cadences "
                   "(median time step not positive, or tiny against a gap)", b, FG_MAX_GAP, (long long)FG_MAX_N - 1);
    }
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ fill
struct FillCols {
    const double *t, *f, *e;
    const int32_t *q, *c;
    double *to, *fo, *eo;
    int32_t *qo, *co;
    uint8_t *mo;
};

// Two kernels over a grid of (light curve, chunk of it) after the launcher has marked every output cadence inserted:
// fill_originals_kernel, one thread per ORIGINAL: its row goes to pos[i], unmarked, and on the time path the same lane walks
// the gap behind it, parking its own index in the flux of every inserted cadence and, on the time path, writing the chain's
// times (the plan's additions again: the same bits); fill_inserted_kernel, one thread per output cadence still marked: its gap
// from the parked index (a bisection of pos per inserted cadence cost 0.5 ms at 1000 x 20 000: 15 dependent loads), then its
// columns.  All indices are checked against the light
// curve's new length: a plan that does not belong to the batch leaves cadences unwritten, never writes outside.
struct FillRow {
    const double *t, *f, *e;
    const int32_t *q, *c, *pos;
    double *to, *fo, *eo;
    int32_t *qo, *co;
    uint8_t *mo;
    int n, nn;
};

__device__ __forceinline__ FillRow fill_row(const FillCols &cp, const int64_t *n_off, const int64_t *new_off, const int32_t *pos, int b) {
    const int64_t lo = n_off[b], olo = new_off[b];
    FillRow r;
    r.n = (int)(n_off[b + 1] - lo), r.nn = (int)(new_off[b + 1] - olo);
    r.t = cp.t + lo, r.f = cp.f + lo, r.e = cp.e ? cp.e + lo : nullptr;
    r.q = cp.q ? cp.q + lo : nullptr, r.c = cp.c ? cp.c + lo : nullptr, r.pos = pos + lo;
    r.to = cp.to + olo, r.fo = cp.fo + olo, r.eo = cp.eo ? cp.eo + olo : nullptr;
    r.qo = cp.qo ? cp.qo + olo : nullptr, r.co = cp.co ? cp.co + olo : nullptr, r.mo = cp.mo + olo;
    return r;
}

__global__ __launch_bounds__(FG_FILL_NT) void fill_originals_kernel(FillCols cp, const int64_t *__restrict__ n_off,
                                                                   const int64_t *__restrict__ new_off, const double *__restrict__ stats,
                                                                   const int32_t *__restrict__ pos) {
    const int b = blockIdx.x;
    const FillRow r = fill_row(cp, n_off, new_off, pos, b);
    const int n = r.n, nn = r.nn;
    const double m = stats[4 * b];
    const bool recompute = r.c != nullptr && n >= 2;  // (fewer than 2 cadences: unchanged)
    for (int i = blockIdx.y * FG_FILL_NT + threadIdx.x; i < n; i += gridDim.y * FG_FILL_NT) {
        const int o = r.pos[i];
        if (o < 0 || o >= nn) continue;
        const double ti = r.t[i];
        double tn = ti;
        if (recompute) {
            const double cf = (double)r.c[i];
            const double d = ti - m * cf;
            tn = d + m * cf;
        }
        r.to[o] = tn;
        r.fo[o] = r.f[i];
        if (r.eo) r.eo[o] = r.e[i];
        if (r.qo) r.qo[o] = r.q[i];
        if (r.co) r.co[o] = r.c[i];
        r.mo[o] = 0;
        if (i + 1 < n) {  // the gap behind it: every inserted cadence learns its gap (parked in its flux), the time path its time
            const int g = min(r.pos[i + 1], nn) - o - 1;
            double prev = ti;
            for (int k = 1; k <= g; ++k) {
                r.fo[o + k] = (double)i;
                if (r.c == nullptr) {
                    prev = prev + m;
                    r.to[o + k] = prev;
                }
            }
        }
    }
}

__global__ __launch_bounds__(FG_FILL_NT) void fill_inserted_kernel(FillCols cp, const int64_t *__restrict__ n_off,
                                                                  const int64_t *__restrict__ new_off, const double *__restrict__ stats,
                                                                  const int32_t *__restrict__ pos, const double *__restrict__ noise_mean,
                                                                  const double *__restrict__ noise_std, uint32_t key0, uint32_t key1,
                                                                  uint32_t first_target, uint32_t stream_id) {
    const int b = blockIdx.x;
    const FillRow r = fill_row(cp, n_off, new_off, pos, b);
    const int n = r.n, nn = r.nn;
    if (nn == n) return;  // nothing inserted (uniform)
    __shared__ int list[FG_TILE];
    __shared__ int count;
    const double m = stats[4 * b], nm = noise_mean[b], ns = noise_std[b];
    // per tile of FG_TILE output cadences: the marked ones are collected in LDS (an integer counter; their order does not matter,
    // each writes its own cadence), then served by dense lanes: at 4 % inserted a lane per cadence left the waves 2 - 3 lanes wide
    // in the generator's log / sincos
    for (int base = blockIdx.y * FG_TILE; base < nn; base += gridDim.y * FG_TILE) {
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
        const int end = min(base + FG_TILE, nn);
        for (int o = base + threadIdx.x; o < end; o += FG_FILL_NT)
            if (r.mo[o] != 0) list[atomicAdd(&count, 1)] = o;
        __syncthreads();
        const int found = count;
        for (int s = threadIdx.x; s < found; s += FG_FILL_NT) {
            const int o = list[s];
            const double parked = r.fo[o];  // the original in front of its gap, left there by fill_originals_kernel
            if (!(parked >= 0.0 && parked < (double)(n - 1))) continue;
            const int j = (int)parked;
            if (!(r.pos[j] < o && o < r.pos[j + 1])) continue;
            const int g = o - r.pos[j], k = o - (j + 1);
            double x;
            if (r.c) {
                const double cfj = (double)r.c[j], cfj1 = (double)r.c[j + 1], cf = (double)(r.c[j] + g);
                const double dj = r.t[j] - m * cfj, dj1 = r.t[j + 1] - m * cfj1;
                const double slope = (dj1 - dj) / (cfj1 - cfj);
                const double nd = slope * (cf - cfj) + dj;
                x = nd + m * cf;
                r.to[o] = x;
                if (r.co) r.co[o] = r.c[j] + g;
            } else {
                x = r.to[o];  // (the chain's link, written by fill_originals_kernel)
            }
            if (r.eo) {
                const double slope = (r.e[j + 1] - r.e[j]) / (r.t[j + 1] - r.t[j]);
                r.eo[o] = slope * (x - r.t[j]) + r.e[j];
            }
            if (r.qo) r.qo[o] = FG_QUALITY_INSERTED;
            double ga, gs;
            philox_normal_pair(philox4x32_10((uint32_t)(k >> 1), 0u, first_target + (uint32_t)b, stream_id, key0, key1), ga, gs);
            r.fo[o] = nm + ns * ((k & 1) ? gs : ga);
        }
        __syncthreads();
    }
}

int fill_gaps_launch(lk_handle *h, int B, const int64_t *n_off_host, const int64_t *new_off_host, const double *time,
                     const double *flux, const double *flux_err, const int32_t *quality, const int32_t *cadenceno, const double *stats,
                     const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed, int64_t first_target,
                     int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out, int32_t *quality_out,
                     int32_t *cadenceno_out, uint8_t *inserted, hipStream_t stream) {
    LK_REQUIRE(B >= 0 && n_off_host != nullptr && new_off_host != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off_host[0] == 0 && new_off_host[0] == 0, "n_off[0] and new_off[0] must be 0");
    int64_t longest = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_off_host[b + 1] - n_off_host[b], nn = new_off_host[b + 1] - new_off_host[b];
        LK_REQUIRE(n >= 0 && n < FG_MAX_N, "target %d has %lld cadences", b, (long long)n);
        LK_REQUIRE(nn >= n && nn < FG_MAX_N, "target %d: %lld cadences cannot be filled to %lld", b, (long long)n, (long long)nn);
        longest = std::max(longest, nn);
    }
    LK_REQUIRE(first_target >= 0 && first_target <= 0xffffffffll && stream_id >= 0 && stream_id <= 0xffffffffll,
               "first_target and stream_id must fit 32 bits");
    LK_REQUIRE(first_target + (int64_t)B - 1 <= 0xffffffffll, "first_target + B must fit 32 bits");
    if (new_off_host[B] == 0) return LK_OK;
    LK_REQUIRE(stats && noise_mean && noise_std, "stats, noise_mean, noise_std must be non-NULL");
    LK_REQUIRE(time_out && flux_out && inserted, "time_out, flux_out, inserted must be non-NULL");
    LK_REQUIRE((time && flux && pos) || n_off_host[B] == 0, "NULL buffer");
    LK_REQUIRE((flux_err == nullptr) == (flux_err_out == nullptr), "flux_err and flux_err_out go together");
    LK_REQUIRE((quality == nullptr) == (quality_out == nullptr), "quality and quality_out go together");
    LK_REQUIRE((cadenceno == nullptr) == (cadenceno_out == nullptr), "cadenceno and cadenceno_out go together");
    int64_t *d_off, *d_new;
    if (const int rc = Scratch(h, h->ws).upload(d_off, n_off_host, B + 1).upload(d_new, new_off_host, B + 1).carve(stream)) return rc;
    FillCols cp{time, flux, flux_err, quality, cadenceno, time_out, flux_out, flux_err_out, quality_out, cadenceno_out, inserted};
    LK_HIP_CHECK(hipMemsetAsync(inserted, 1, (size_t)new_off_host[B], stream));
    const unsigned gy = (unsigned)std::min<int64_t>(std::max<int64_t>((longest + FG_TILE - 1) / FG_TILE, 1), 64);
    hipLaunchKernelGGL(fill_originals_kernel, dim3(B, gy), dim3(FG_FILL_NT), 0, stream, cp, d_off, d_new, stats, pos);
    hipLaunchKernelGGL(fill_inserted_kernel, dim3(B, gy), dim3(FG_FILL_NT), 0, stream, cp, d_off, d_new, stats, pos, noise_mean,
                       noise_std, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)first_target,
                       (uint32_t)stream_id);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ stitch: segment gather
struct SegCols {
    const void *in[8];
    void *out[8];
    int elem[8];  // 4 or 8 bytes
};

// segment s: dst_off[s + 1] - dst_off[s] elements of every column from src_start[s] to dst_off[s]; blockIdx.y strides inside it
__global__ __launch_bounds__(256) void gather_segments_kernel(const int64_t *__restrict__ src_start, const int64_t *__restrict__ dst_off,
                                                              int ncols, SegCols cp) {
    const int s = blockIdx.x;
    const int64_t src = src_start[s], dst = dst_off[s], len = dst_off[s + 1] - dst;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.y * 256)
        for (int cidx = 0; cidx < ncols; ++cidx) {
            if (cp.elem[cidx] == 8)
                static_cast<uint64_t *>(cp.out[cidx])[dst + i] = static_cast<const uint64_t *>(cp.in[cidx])[src + i];
            else
                static_cast<uint32_t *>(cp.out[cidx])[dst + i] = static_cast<const uint32_t *>(cp.in[cidx])[src + i];
        }
}

int gather_segments_launch(lk_handle *h, int S, const int64_t *src_start_host, const int64_t *dst_off_host, int64_t n_src, int ncols,
                           const int *elem_bytes, const void *const *cols_in, void *const *cols_out, hipStream_t stream) {
    LK_REQUIRE(S >= 0 && n_src >= 0, "bad segment description");
    LK_REQUIRE(ncols >= 0 && ncols <= 8, "at most 8 columns per call (got %d)", ncols);
    if (S == 0 || ncols == 0) return LK_OK;
    LK_REQUIRE(src_start_host && dst_off_host, "NULL segment table");
    LK_REQUIRE(dst_off_host[0] == 0, "dst_off[0] must be 0");
    int64_t longest = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t len = dst_off_host[s + 1] - dst_off_host[s];
        LK_REQUIRE(len >= 0, "segment %d has a negative length", s);
        LK_REQUIRE(src_start_host[s] >= 0 && src_start_host[s] <= n_src - len, "segment %d reads outside the %lld source cadences", s,
                   (long long)n_src);
        longest = len > longest ? len : longest;
    }
    if (dst_off_host[S] == 0) return LK_OK;
    LK_REQUIRE(elem_bytes && cols_in && cols_out, "NULL column table");
    SegCols cp;
    for (int c = 0; c < 8; ++c) cp.in[c] = nullptr, cp.out[c] = nullptr, cp.elem[c] = 8;
    for (int c = 0; c < ncols; ++c) {
        LK_REQUIRE(elem_bytes[c] == 4 || elem_bytes[c] == 8, "column %d: elements of 4 or 8 bytes (got %d)", c, elem_bytes[c]);
        LK_REQUIRE(cols_in[c] && cols_out[c] && cols_in[c] != cols_out[c], "column %d is NULL or gathered in place", c);
        cp.in[c] = cols_in[c], cp.out[c] = cols_out[c], cp.elem[c] = elem_bytes[c];
    }
    int64_t *d_src, *d_dst;
    if (const int rc = Scratch(h, h->ws).upload(d_src, src_start_host, S).upload(d_dst, dst_off_host, S + 1).carve(stream)) return rc;
    const int64_t per = (longest + 1023) / 1024;  // ~4 elements per thread
    const unsigned gy = (unsigned)(per < 1 ? 1 : (per > 64 ? 64 : per));
    hipLaunchKernelGGL(gather_segments_kernel, dim3(S, gy), dim3(256), 0, stream, d_src, d_dst, ncols, cp);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
