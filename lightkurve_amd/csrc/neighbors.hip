// neighbors.hip — the under-fitting goodness metric of a resident batch, neighbours given by index.
// Reference: src/lightkurve/correctors/metrics.py:141-257 (underfit_metric_neighbors) over _compute_correlation
// (:451-475).  Only the target's column of its (m + 1)^2 correlation matrix enters the metric, so for target t with valid
// neighbours S_t (m = |S_t|) on the n kept cadences:
//
//     med_b  = numpy.median(y_b[kept]);   z_b[i] = y_b[kept[i]] / med_b - 1.0       (these two IEEE operations, in this order)
//     G(a,b) = sum_i z_a[i] z_b[i];       c(t,j) = G(t,j) / sqrt(G(t,t) G(j,j))     (0 when either self-product is 0)
//     metric_t = 2 / (1 + exp(scale * sum_j |c(t,j)|^3 / (m + 1))),  scale = ln(2 / 0.95 - 1) / (0.0007 + 0.8083 n^-0.5023)
//
// Two passes on the caller's stream.  PREPARE (one workgroup per target): exact median (block_median), the compacted z row
// written to scratch as float64 at a pitch of 128-element steps (the tail of the last step is zero: a zero adds nothing to a
// sum, so no pass has tail code and every row starts 16-byte aligned whatever the parity of n), and G(b,b).  PAIR (one
// workgroup per target, the hot path): the m dot products against the neighbours' z rows, then c and the metric.
//
// Summation order of G(a,b) — a function of n alone: element i belongs to step i / 128, lane (i / 2) % 64, component i % 2;
// a lane keeps one running sum per component, visits its steps in ascending order and adds with fma(z_a, z_b, sum) (the
// same bits whichever row is called a); at the end the lane adds its two components, then six xor-butterfly levels
// (distance 32 ... 1) finish the dot in every lane alike.  One wavefront computes one dot from start to end, so nothing
// depends on B, M, the neighbour's position in the list or the workgroup: G(t,j) and G(j,t) are the same bits, and so is a
// run on a sub-batch.  No atomics.
//
// The neighbours may also be the rows of ANOTHER array, prepared once into a caller-owned block (underfit_rows_*: Bn rows at the
// same pitch, then their Bn self-products) and used by any number of pair passes: the pair kernel takes the target rows and the
// neighbour rows as two arrays, which are one and the same in the call above.
#include "block_select.hpp"
#include "lk_common.hpp"

#include <algorithm>
#include <cmath>

namespace lk {

constexpr int UF_STEP = 128;          // elements per step of a dot: 64 lanes x one 16-byte load
constexpr int UF_NT = 512;            // threads of a pair workgroup: 8 wavefronts, one or more neighbours each
constexpr int UF_NW = UF_NT / 64;
constexpr int UF_A = 4;               // neighbours a wavefront carries at once (each an independent stream of 16-byte loads)
constexpr int UF_CHUNK = 2048;        // elements of the target's row per LDS buffer (16 KiB; two buffers)
constexpr int UF_CSTEPS = UF_CHUNK / UF_STEP;

// The dots of ONE target row against NA other rows over steps [k0, k1): tgt(k) returns the target's two elements of step k
// for this lane, row(a, k) those of row a.  ax / ay: the lane's running sums per component.
template <int NA, class Tgt, class Row>
__device__ __forceinline__ void uf_dot_steps(int k0, int k1, Tgt tgt, Row row, double (&ax)[UF_A], double (&ay)[UF_A]) {
#pragma unroll 2
    for (int k = k0; k < k1; ++k) {
        double2 v[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) v[a] = row(a, k);
        const double2 t = tgt(k);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            ax[a] = fma(t.x, v[a].x, ax[a]);
            ay[a] = fma(t.y, v[a].y, ay[a]);
        }
    }
}

// the lane's two components, then the butterfly: the same value in all 64 lanes
__device__ __forceinline__ double uf_dot_finish(double ax, double ay) {
    double s = ax + ay;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// ------------------------------------------------------------------------------------------------ prepare
// y: the target's N cadences; kept cadence i is y[keep_idx[i]] (keep_idx ascending) or y[i] (keep_idx == NULL, n == N).
__global__ __launch_bounds__(1024) void underfit_prepare_kernel(const double *__restrict__ flux, int N, int n,
                                                                const int32_t *__restrict__ keep_idx, int pitch,
                                                                double *__restrict__ z, double *__restrict__ gself) {
    __shared__ unsigned long long sh[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *y = flux + (size_t)b * N;
    auto val = [&](int i) { return keep_idx ? y[keep_idx[i]] : y[i]; };
    auto all = [&](int) { return true; };
    const double med = block_median(n, (long long)n, val, all, sh);
    // y / med - 1.0 as two separately rounded operations (a zero median gives non-finite z: the caller's business)
    auto zval = [&](int i) { return i < n ? __dsub_rn(__ddiv_rn(val(i), med), 1.0) : 0.0; };
    double *zb = z + (size_t)b * pitch;
    for (int i = tid; i < pitch; i += 1024) zb[i] = zval(i);
    // G(b,b) by the pair pass's own routine, one wavefront; the elements are formed again from y (the same two operations,
    // the same bits) rather than read back from the row just stored
    if (tid < 64) {
        double ax[UF_A] = {0.0, 0.0, 0.0, 0.0}, ay[UF_A] = {0.0, 0.0, 0.0, 0.0};
        auto own = [&](int k) {
            const int i = k * UF_STEP + 2 * tid;
            return make_double2(zval(i), zval(i + 1));
        };
        uf_dot_steps<1>(0, pitch / UF_STEP, own, [&](int, int k) { return own(k); }, ax, ay);
        const double g = uf_dot_finish(ax[0], ay[0]);
        if (tid == 0) gself[b] = g;
    }
}

// ------------------------------------------------------------------------------------------------ pair pass
// One workgroup per target t.  The target's row goes through LDS in chunks of UF_CHUNK elements (two buffers: the next
// chunk's global loads are issued before the current chunk's arithmetic and land in the other buffer after it, one barrier
// per chunk).  A trip handles UF_NW * UF_A = 32 list positions: wavefront w owns positions base + a * UF_NW + w, a < UF_A,
// and streams those neighbours' rows with 16-byte loads; a list longer than a trip takes more trips (the row is staged again
// from L2 each trip).  Padding (-1) and indices outside [0, Bn) read the target's own row and are discarded: correlation NaN,
// not counted in m.  The cubes of a trip are added in position order by one thread, so the metric is reproducible too.
// z / gself: the target rows and their self-products; zn / gn: the Bn neighbour rows and theirs (the same two arrays when the
// neighbours are targets of the batch).  A neighbour's row base is formed once per trip, outside the dot loop.
__global__ __launch_bounds__(UF_NT, 4) void underfit_pair_kernel(const double *__restrict__ z, const double *__restrict__ gself,
                                                              const double *__restrict__ zn, const double *__restrict__ gn,
                                                              int pitch, int Bn, int M, const int32_t *__restrict__ nbr,
                                                              double scale, double *__restrict__ corr,
                                                              double *__restrict__ metric) {
    __shared__ __attribute__((aligned(16))) double2 s_row[2][UF_CHUNK / 2];
    __shared__ double s_cube[UF_NW * UF_A];
    __shared__ int s_valid[UF_NW * UF_A];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *zt = z + (size_t)t * pitch;
    const double gtt = M > 0 ? gself[t] : 0.0;
    const int steps = pitch / UF_STEP, nchunk = (steps + UF_CSTEPS - 1) / UF_CSTEPS;
    double sum = 0.0;   // thread 0: sum of |c|^3 in position order
    int m = 0;          // thread 0: valid neighbours
    for (int base = 0; base < M; base += UF_NW * UF_A) {
        // this wavefront's neighbours of the trip
        int na = 0, jn[UF_A];
        bool ok[UF_A];
        const double *rows[UF_A];
#pragma unroll
        for (int a = 0; a < UF_A; ++a) {
            const int p = base + a * UF_NW + w;
            int j = -1;
            if (p < M) {
                na = a + 1;
                j = __builtin_amdgcn_readfirstlane(nbr[(size_t)t * M + p]);
            }
            ok[a] = j >= 0 && j < Bn;
            jn[a] = j;
            rows[a] = ok[a] ? zn + (size_t)j * pitch : zt;
        }
        double ax[UF_A] = {0.0, 0.0, 0.0, 0.0}, ay[UF_A] = {0.0, 0.0, 0.0, 0.0};
        auto row = [&](int a, int k) { return *reinterpret_cast<const double2 *>(rows[a] + (size_t)k * UF_STEP + 2 * lane); };
        // stage chunk 0 (UF_NT threads x two 16-byte loads cover a chunk; past the row's end nothing is staged or read)
        auto stage_load = [&](int c, double2 (&r)[2]) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = c * UF_CHUNK + 2 * (tid + u * UF_NT);
                r[u] = e < pitch ? *reinterpret_cast<const double2 *>(zt + e) : make_double2(0.0, 0.0);
            }
        };
        auto stage_store = [&](int buf, const double2 (&r)[2]) {
#pragma unroll
            for (int u = 0; u < 2; ++u) s_row[buf][tid + u * UF_NT] = r[u];
        };
        double2 r[2];
        stage_load(0, r);
        __syncthreads();   // the previous trip's readers of buffer 0 and of s_cube are done
        stage_store(0, r);
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) stage_load(c + 1, r);
            const int k0 = c * UF_CSTEPS, k1 = min(k0 + UF_CSTEPS, steps);
            const double2 *buf = s_row[c & 1];
            auto tgt = [&](int k) { return buf[(k - k0) * 64 + lane]; };
            switch (na) {   // (uniform over the wavefront)
                case 1: uf_dot_steps<1>(k0, k1, tgt, row, ax, ay); break;
                case 2: uf_dot_steps<2>(k0, k1, tgt, row, ax, ay); break;
                case 3: uf_dot_steps<3>(k0, k1, tgt, row, ax, ay); break;
                case 4: uf_dot_steps<4>(k0, k1, tgt, row, ax, ay); break;
                default: break;
            }
            if (more) stage_store((c + 1) & 1, r);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < UF_A; ++a) {
            if (a < na) {
                const double g = uf_dot_finish(ax[a], ay[a]);
                if (lane == 0) {
                    const int p = base + a * UF_NW + w;
                    const double gjj = ok[a] ? gn[jn[a]] : gtt;
                    const double c = (gtt == 0.0 || gjj == 0.0) ? 0.0 : g / sqrt(gtt * gjj);
                    const double ac = fabs(c);
                    if (corr) corr[(size_t)t * M + p] = ok[a] ? c : __longlong_as_double(0x7ff8000000000000ll);
                    s_cube[a * UF_NW + w] = ok[a] ? ac * ac * ac : 0.0;
                    s_valid[a * UF_NW + w] = ok[a] ? 1 : 0;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(UF_NW * UF_A, M - base);
            for (int s = 0; s < cnt; ++s) {
                sum += s_cube[s];
                m += s_valid[s];
            }
        }
    }
    if (tid == 0) metric[t] = 2.0 / (1.0 + exp(scale * sum / (double)(m + 1)));
}

static int underfit_shape_ok(int B, int N, int n, const int32_t *keep_idx) {
    LK_REQUIRE(B >= 1, "B must be >= 1 (got %d)", B);
    LK_REQUIRE(N >= 2 && n >= 2 && n <= N, "need 2 <= n <= N (got n=%d, N=%d): the metric needs at least two kept cadences", n, N);
    LK_REQUIRE(N < (1 << 30), "N=%d cadences outside 2..2^30", N);
    LK_REQUIRE(keep_idx != nullptr || n == N, "keep_idx is NULL (all cadences) but n=%d != N=%d", n, N);
    return LK_OK;
}

static inline int uf_pitch(int n) { return (n + UF_STEP - 1) / UF_STEP * UF_STEP; }

static double uf_scale(int n) {
    const double wgn = 0.0007 + 0.8083 * std::pow((double)n, -0.5023);
    return std::log(2.0 / 0.95 - 1.0) / wgn;
}

// Workspace: B x pitch doubles of z rows (pitch = n rounded up to 128) + B self-products.
int underfit_neighbors_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                              const int32_t *neighbors, double *corr, double *metric, hipStream_t stream) {
    if (const int rc = underfit_shape_ok(B, N, n, keep_idx)) return rc;
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    const int pitch = uf_pitch(n);
    double *d_z, *d_g;
    if (const int rc = Scratch(h, h->ws).buf(d_z, (size_t)B * pitch).buf(d_g, B).carve(stream)) return rc;
    if (M > 0)
        hipLaunchKernelGGL(underfit_prepare_kernel, dim3(B), dim3(1024), 0, stream, flux, N, n, keep_idx, pitch, d_z, d_g);
    hipLaunchKernelGGL(underfit_pair_kernel, dim3(B), dim3(UF_NT), 0, stream, (const double *)d_z, (const double *)d_g,
                       (const double *)d_z, (const double *)d_g, pitch, B, M, neighbors, uf_scale(n), corr, metric);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ prepared neighbour rows
// The block: Bn x pitch doubles of z rows, then Bn self-products (the row part is a multiple of 1 KiB: both 16-byte aligned).
int underfit_rows_bytes(int Bn, int n, int64_t *bytes) {
    LK_REQUIRE(Bn >= 1 && n >= 2 && n < (1 << 30), "need Bn >= 1 and 2 <= n < 2^30 (got Bn=%d, n=%d)", Bn, n);
    LK_REQUIRE(bytes != nullptr, "bytes is NULL");
    *bytes = ((int64_t)Bn * uf_pitch(n) + Bn) * 8;
    return LK_OK;
}

int underfit_rows_prepare_launch(lk_handle *h, int Bn, int N, const double *flux_nb, int n, const int32_t *keep_idx, void *rows,
                                 int64_t rows_bytes, hipStream_t stream) {
    (void)h;
    if (const int rc = underfit_shape_ok(Bn, N, n, keep_idx)) return rc;
    LK_REQUIRE(flux_nb != nullptr, "NULL buffer");
    LK_REQUIRE(rows != nullptr && ((uintptr_t)rows & 15) == 0, "rows must be a 16-byte aligned device buffer");
    const int pitch = uf_pitch(n);
    LK_REQUIRE(rows_bytes >= ((int64_t)Bn * pitch + Bn) * 8, "rows too small: %lld bytes given, %d rows of %d kept cadences need %lld "
               "(lk_underfit_rows_bytes)", (long long)rows_bytes, Bn, n, (long long)(((int64_t)Bn * pitch + Bn) * 8));
    double *z = static_cast<double *>(rows);
    hipLaunchKernelGGL(underfit_prepare_kernel, dim3(Bn), dim3(1024), 0, stream, flux_nb, N, n, keep_idx, pitch, z,
                       z + (size_t)Bn * pitch);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// Only the B target rows are prepared (in the handle's arena); the neighbours are read from `rows` as prepared above with the
// same n and keep_idx.  Here an index equal to the target's own row number names a row of the OTHER array: a neighbour.
int underfit_against_rows_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int Bn,
                                 const void *rows, int M, const int32_t *neighbors, double *corr, double *metric,
                                 hipStream_t stream) {
    if (const int rc = underfit_shape_ok(B, N, n, keep_idx)) return rc;
    LK_REQUIRE(Bn >= 1, "Bn must be >= 1 (got %d)", Bn);
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    LK_REQUIRE(rows != nullptr && ((uintptr_t)rows & 15) == 0, "rows must be a 16-byte aligned device buffer");
    const int pitch = uf_pitch(n);
    double *d_z, *d_g;
    if (const int rc = Scratch(h, h->ws).buf(d_z, (size_t)B * pitch).buf(d_g, B).carve(stream)) return rc;
    const double *zn = static_cast<const double *>(rows);
    if (M > 0)
        hipLaunchKernelGGL(underfit_prepare_kernel, dim3(B), dim3(1024), 0, stream, flux, N, n, keep_idx, pitch, d_z, d_g);
    hipLaunchKernelGGL(underfit_pair_kernel, dim3(B), dim3(UF_NT), 0, stream, (const double *)d_z, (const double *)d_g, zn,
                       zn + (size_t)Bn * pitch, pitch, Bn, M, neighbors, uf_scale(n), corr, metric);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace lk
