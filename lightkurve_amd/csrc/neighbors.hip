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
//
// Ragged targets that share only part of a cadence grid have their own two kernels at the end of this file (underfit_grid_*): rows
// on the grid layout, one presence bit per grid row, and dots over the rows a target and all of its neighbours have.
#include "block_select.hpp"
#include "lk_common.hpp"

#include <algorithm>
#include <climits>
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

// The B target rows are prepared in the handle's arena (workspace: B x pitch doubles of z rows, pitch = n rounded up to 128, + B
// self-products).  against == false: the neighbours are the batch itself.  against: they are read from `rows` (Bn of them, as
// underfit_rows_prepare_launch leaves them for the same n and keep_idx); then an index equal to the target's own row number names a
// row of the OTHER array: a neighbour.
static int underfit_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, bool against, int Bn,
                           const void *rows, int M, const int32_t *neighbors, double *corr, double *metric, hipStream_t stream) {
    if (const int rc = underfit_shape_ok(B, N, n, keep_idx)) return rc;
    if (against) LK_REQUIRE(Bn >= 1, "Bn must be >= 1 (got %d)", Bn);
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    if (against) LK_REQUIRE(rows != nullptr && ((uintptr_t)rows & 15) == 0, "rows must be a 16-byte aligned device buffer");
    const int pitch = uf_pitch(n);
    double *d_z, *d_g;
    if (const int rc = Scratch(h, h->ws).buf(d_z, (size_t)B * pitch).buf(d_g, B).carve(stream)) return rc;
    if (!against) Bn = B;
    const double *zn = against ? static_cast<const double *>(rows) : d_z, *gn = against ? zn + (size_t)Bn * pitch : d_g;
    if (M > 0)
        hipLaunchKernelGGL(underfit_prepare_kernel, dim3(B), dim3(1024), 0, stream, flux, N, n, keep_idx, pitch, d_z, d_g);
    hipLaunchKernelGGL(underfit_pair_kernel, dim3(B), dim3(UF_NT), 0, stream, (const double *)d_z, (const double *)d_g, zn, gn, pitch,
                       Bn, M, neighbors, uf_scale(n), corr, metric);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int underfit_neighbors_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                              const int32_t *neighbors, double *corr, double *metric, hipStream_t stream) {
    return underfit_launch(h, B, N, flux, n, keep_idx, false, 0, nullptr, M, neighbors, corr, metric, stream);
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

int underfit_against_rows_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int Bn,
                                 const void *rows, int M, const int32_t *neighbors, double *corr, double *metric,
                                 hipStream_t stream) {
    return underfit_launch(h, B, N, flux, n, keep_idx, true, Bn, rows, M, neighbors, corr, metric, stream);
}

// ================================================================================================ the metric on a cadence grid
// Ragged targets: light curve b holds n_b of the Nx cadences of a grid, its cadence i on grid row rows_b[i] (strictly increasing:
// lk_align_rows_batch), and is PRESENT at row r when it has that cadence and its own cadence_mask entry there is true.  The
// reference drops a cadence that the target or any of its neighbours lacks (the NaN rows of its flux matrix), so the set the dots
// run over belongs to the target: C_t = the rows where t and every valid neighbour of t are present, n_t = |C_t|, and
//
//     med_b = numpy.median(y_b[present]);  z_b[r] = y_b / med_b - 1.0 at present rows (the two operations of the uniform pass)
//     G_t(a,b) = sum_{r in C_t} z_a[r] z_b[r];  c(t,j) = G_t(t,j) / sqrt(G_t(t,t) G_t(j,j));  scale = uf_scale(n_t)
//
// GRID PREPARE (one workgroup per light curve): the exact median over the present cadences, the z row ON THE GRID LAYOUT (pitch =
// Nx rounded up to 128, 0.0 at absent rows and in the tail) and the presence bitmask, one 64-bit word per 64 grid rows (pitch / 64
// words; a wavefront's __ballot of the predicate is the word, no atomics).  A grid row's cadence comes from the inverse map pos
// (B x Nx int32, regress.hip's rows_pos_kernel, which also checks rows).
// GRID PAIR (one workgroup per target, the shape of underfit_pair_kernel): first C_t = the AND of the bitmask words of t and of
// its valid neighbours, kept in dynamic LDS (pitch / 8 bytes), and its population count.  Then the same trips; per step a lane
// takes its two bits of C_t, selects the target's and the neighbours' elements to 0.0 where the bit is clear, and adds
// fma(t, v, cross), fma(v, v, self) per neighbour and fma(t, t, own) for G_t(t,t): all three by the one routine, in the order
// written at the top of this file with i = the grid row.  Self-products cannot be taken once per row any more: they depend on t.
// With every light curve present at every row the selections change nothing: the bits are the uniform call's.
// n_t < 2: the metric and every correlation are NaN (no error: with a mask on the device the host does not know n_t); no valid
// neighbour: 1.0.  uf_scale(n_t) is read from a table made on the host (lk_handle::uf_scale_tab): the host's pow and log, not
// the device's, so that the scale is the uniform call's bits.
constexpr int UFG_MAX_NX = 245760;    // pitch / 8 bytes of dynamic LDS for C_t: at most 30 KiB beside the 32.5 KiB of static LDS

__global__ __launch_bounds__(1024) void underfit_grid_prepare_kernel(const double *__restrict__ flux,
                                                                     const uint8_t *__restrict__ cmask,
                                                                     const int64_t *__restrict__ n_off, const int *__restrict__ pos,
                                                                     int Nx, int pitch, double *__restrict__ z,
                                                                     unsigned long long *__restrict__ mk) {
    __shared__ unsigned long long sh[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = n_off[b];
    const int n = (int)(n_off[b + 1] - lo);
    const double *y = flux + lo;
    const uint8_t *cm = cmask ? cmask + lo : nullptr;
    auto val = [&](int i) { return y[i]; };
    auto keep = [&](int i) { return cm == nullptr || cm[i] != 0; };
    long long c = 0;
    for (int i = tid; i < n; i += 1024) c += keep(i) ? 1 : 0;
    const long long count = block_count_dyn(c, reinterpret_cast<long long *>(sh));
    const double med = block_median(n, count, val, keep, sh);   // (NaN when nothing is present: no row uses it then)
    const int *pb = pos + (size_t)b * Nx;
    double *zb = z + (size_t)b * pitch;
    unsigned long long *mb = mk + (size_t)b * (pitch / 64);
    // pitch is a multiple of 128 and tid of a wavefront a run of 64: a wavefront's 64 rows are one word, all lanes active
    for (int r = tid; r < pitch; r += 1024) {
        const int p = r < Nx ? pb[r] : -1;
        const bool present = p >= 0 && keep(p);
        zb[r] = present ? __dsub_rn(__ddiv_rn(y[p], med), 1.0) : 0.0;
        const unsigned long long word = __ballot(present);
        if ((tid & 63) == 0) mb[r >> 6] = word;
    }
}

// cross[a] = sum t v_a, self[a] = sum v_a v_a, own = sum t t over steps [k0, k1), every element selected by its bit of C_t:
// bits(k) returns the lane's two bits of step k (bit 0: component x, bit 1: component y)
template <int NA, class Tgt, class Row, class Bits>
__device__ __forceinline__ void ufg_dot_steps(int k0, int k1, Tgt tgt, Row row, Bits bits, double (&cx)[UF_A], double (&cy)[UF_A],
                                              double (&sx)[UF_A], double (&sy)[UF_A], double &ox, double &oy) {
#pragma unroll 1
    for (int k = k0; k < k1; ++k) {
        double2 v[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) v[a] = row(a, k);
        const double2 t = tgt(k);
        // the selection as a bitwise AND with all ones or zero (+0.0 where the bit is clear, whatever the element holds): a
        // conditional would be turned into conditional 8-byte loads, and the 16-byte stream would be gone
        const unsigned c = bits(k);
        const unsigned long long mx = 0ull - (unsigned long long)(c & 1u), my = 0ull - (unsigned long long)((c >> 1) & 1u);
        auto sel = [](double x, unsigned long long m) {
            return __longlong_as_double((long long)((unsigned long long)__double_as_longlong(x) & m));
        };
        const double tx = sel(t.x, mx), ty = sel(t.y, my);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const double vx = sel(v[a].x, mx), vy = sel(v[a].y, my);
            cx[a] = fma(tx, vx, cx[a]);
            cy[a] = fma(ty, vy, cy[a]);
            sx[a] = fma(vx, vx, sx[a]);
            sy[a] = fma(vy, vy, sy[a]);
        }
        ox = fma(tx, tx, ox);
        oy = fma(ty, ty, oy);
    }
}

// z / mk: the target rows and their presence words; zn / mkn: the Bn neighbour rows and theirs (the same arrays when the
// neighbours are targets of the batch).  scale_tab[n] = uf_scale(n), n <= Nx.  G_t(t,t) is formed by every wavefront beside its
// own dots in every trip (the target's elements are in LDS anyway): the same routine, the same order, the same bits each time.
__global__ __launch_bounds__(UF_NT, 4) void underfit_grid_pair_kernel(const double *__restrict__ z,
                                                                   const unsigned long long *__restrict__ mk,
                                                                   const double *__restrict__ zn,
                                                                   const unsigned long long *__restrict__ mkn, int pitch, int Bn,
                                                                   int M, const int32_t *__restrict__ nbr,
                                                                   const double *__restrict__ scale_tab, double *__restrict__ corr,
                                                                   int32_t *__restrict__ n_common, double *__restrict__ metric) {
    extern __shared__ unsigned long long s_C[];   // pitch / 64 words
    __shared__ __attribute__((aligned(16))) double2 s_row[2][UF_CHUNK / 2];
    __shared__ double s_cube[UF_NW * UF_A];
    __shared__ double s_sum;
    __shared__ int s_cnt[UF_NW + 1];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = pitch / 64;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int32_t *list = nbr + (size_t)t * M;
    // C_t and its population
    {
        const unsigned long long *mt = mk + (size_t)t * W;
        int cnt = 0;
        for (int wd = tid; wd < W; wd += UF_NT) {
            unsigned long long c = mt[wd];
            for (int p = 0; p < M; ++p) {
                const int j = list[p];
                if (j >= 0 && j < Bn) c &= mkn[(size_t)j * W + wd];
            }
            s_C[wd] = c;
            cnt += __popcll(c);
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) s_cnt[w] = cnt;
        if (tid == 0) {
            int mv = 0;
            for (int p = 0; p < M; ++p) mv += (list[p] >= 0 && list[p] < Bn) ? 1 : 0;
            s_cnt[UF_NW] = mv;
        }
    }
    __syncthreads();
    int nt = 0;
    for (int i = 0; i < UF_NW; ++i) nt += s_cnt[i];
    const int mvalid = s_cnt[UF_NW];
    if (tid == 0 && n_common) n_common[t] = nt;
    if (nt < 2 || mvalid == 0) {   // (uniform over the workgroup)
        if (corr)
            for (int p = tid; p < M; p += UF_NT) corr[(size_t)t * M + p] = nan;
        if (tid == 0) metric[t] = mvalid == 0 ? 1.0 : nan;
        return;
    }
    const double *zt = z + (size_t)t * pitch;
    const int steps = pitch / UF_STEP, nchunk = (steps + UF_CSTEPS - 1) / UF_CSTEPS;
    auto bits = [&](int k) { return (unsigned)(s_C[2 * k + (lane >> 5)] >> ((2 * lane) & 63)) & 3u; };
    // (thread 0's sum of |c|^3 in position order lives in LDS, s_sum: a register of every lane for all the trips otherwise)
    if (tid == 0) s_sum = 0.0;
    for (int base = 0; base < M; base += UF_NW * UF_A) {
        int na = 0;
        bool ok[UF_A];
        const double *rows[UF_A];
#pragma unroll
        for (int a = 0; a < UF_A; ++a) {
            const int p = base + a * UF_NW + w;
            int j = -1;
            if (p < M) {
                na = a + 1;
                j = __builtin_amdgcn_readfirstlane(list[p]);
            }
            ok[a] = j >= 0 && j < Bn;
            rows[a] = ok[a] ? zn + (size_t)j * pitch : zt;
        }
        double cx[UF_A] = {0.0, 0.0, 0.0, 0.0}, cy[UF_A] = {0.0, 0.0, 0.0, 0.0};
        double sx[UF_A] = {0.0, 0.0, 0.0, 0.0}, sy[UF_A] = {0.0, 0.0, 0.0, 0.0};
        double ox = 0.0, oy = 0.0;
        auto row = [&](int a, int k) { return *reinterpret_cast<const double2 *>(rows[a] + (size_t)k * UF_STEP + 2 * lane); };
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
            // two variants only (a slot past the wavefront's last position streams the target's own row from the cache and is
            // discarded): with one per count the compiler keeps a register set per variant and spills
            if (na > 2) ufg_dot_steps<4>(k0, k1, tgt, row, bits, cx, cy, sx, sy, ox, oy);
            else if (na > 0) ufg_dot_steps<2>(k0, k1, tgt, row, bits, cx, cy, sx, sy, ox, oy);
            if (more) stage_store((c + 1) & 1, r);
            __syncthreads();
        }
        const double gtt = uf_dot_finish(ox, oy);
#pragma unroll
        for (int a = 0; a < UF_A; ++a) {
            if (a < na) {
                const double g = uf_dot_finish(cx[a], cy[a]);
                const double gjj = uf_dot_finish(sx[a], sy[a]);
                if (lane == 0) {
                    const int p = base + a * UF_NW + w;
                    const double c = (gtt == 0.0 || gjj == 0.0) ? 0.0 : g / sqrt(gtt * gjj);
                    const double ac = fabs(c);
                    if (corr) corr[(size_t)t * M + p] = ok[a] ? c : nan;
                    s_cube[a * UF_NW + w] = ok[a] ? ac * ac * ac : 0.0;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(UF_NW * UF_A, M - base);
            double sum = s_sum;
            for (int s = 0; s < cnt; ++s) sum += s_cube[s];
            s_sum = sum;
        }
    }
    if (tid == 0) metric[t] = 2.0 / (1.0 + exp(scale_tab[nt] * s_sum / (double)(mvalid + 1)));
}

static int ufg_shape_ok(int B, const int64_t *n_off_host, int Nx, int64_t *nmax) {
    LK_REQUIRE(B >= 1 && n_off_host != nullptr, "B must be >= 1 (got %d) and n_off given", B);
    LK_REQUIRE(B <= 65535, "at most 65535 light curves per call on this path (got %d): split the batch", B);
    LK_REQUIRE(Nx >= 1 && Nx <= UFG_MAX_NX, "Nx=%d grid rows outside 1..%d", Nx, UFG_MAX_NX);
    LK_REQUIRE(n_off_host[0] == 0, "n_off must start at 0");
    *nmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t nb = n_off_host[b + 1] - n_off_host[b];
        LK_REQUIRE(nb >= 0 && nb <= Nx, "light curve %d: %lld cadences outside 0..Nx=%d (rows are strictly increasing)", b,
                   (long long)nb, Nx);
        *nmax = std::max(*nmax, nb);
    }
    return LK_OK;
}

static inline size_t ufg_words(int Nx) { return (size_t)uf_pitch(Nx) / 64; }

// uf_scale(0 .. Nx) on the host, kept in the handle
static const double *ufg_scale_table(lk_handle *h, int Nx) {
    std::vector<double> &tab = h->uf_scale_tab;
    for (int n = (int)tab.size(); n <= Nx; ++n) tab.push_back(n >= 1 ? uf_scale(n) : 0.0);
    return tab.data();
}

// pos from rows, the check of rows (the one wait of these calls: 4 bytes come back), then the prepare pass
static int ufg_prepare(int B, const int64_t *d_off, int64_t nmax, const int32_t *rows, int Nx, const double *flux,
                       const uint8_t *cmask, int32_t *d_pos, int *d_bad, double *z, unsigned long long *mk, hipStream_t stream) {
    if (const int rc = rows_pos_launch(B, d_off, nmax, rows, Nx, d_pos, d_bad, stream)) return rc;
    int bad = 0;
    LK_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream));
    LK_HIP_CHECK(hipStreamSynchronize(stream));
    LK_REQUIRE(bad == INT_MAX, "light curve %d: rows must be strictly increasing indices into the %d rows of the grid", bad, Nx);
    hipLaunchKernelGGL(underfit_grid_prepare_kernel, dim3(B), dim3(1024), 0, stream, flux, cmask, d_off, (const int *)d_pos, Nx,
                       uf_pitch(Nx), z, mk);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

static void ufg_pair(int B, const double *z, const unsigned long long *mk, const double *zn, const unsigned long long *mkn, int Nx,
                     int Bn, int M, const int32_t *neighbors, const double *d_tab, double *corr, int32_t *n_common, double *metric,
                     hipStream_t stream) {
    hipLaunchKernelGGL(underfit_grid_pair_kernel, dim3(B), dim3(UF_NT), ufg_words(Nx) * 8, stream, z, mk, zn, mkn, uf_pitch(Nx), Bn, M,
                       neighbors, d_tab, corr, n_common, metric);
}

// The B target rows are prepared in the handle's arena (workspace: B x pitch doubles of z rows + B x pitch / 64 presence words + the
// inverse map pos (B x Nx int32) + Nx + 1 scales).  against == false: the neighbours are the batch itself.  against: they are read
// from `block` (Bn of them, as underfit_grid_rows_prepare_launch leaves them on the same grid); then an index equal to the target's
// own row number names a row of the OTHER array: a neighbour.
static int underfit_grid_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, const double *flux,
                                const uint8_t *cmask, bool against, int Bn, const void *block, int M, const int32_t *neighbors,
                                double *corr, int32_t *n_common, double *metric, hipStream_t stream) {
    int64_t nmax = 0;
    if (const int rc = ufg_shape_ok(B, n_off_host, Nx, &nmax)) return rc;
    if (against) LK_REQUIRE(Bn >= 1, "Bn must be >= 1 (got %d)", Bn);
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(rows && flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    if (against) LK_REQUIRE(block != nullptr && ((uintptr_t)block & 15) == 0, "block must be a 16-byte aligned device buffer");
    const int pitch = uf_pitch(Nx), init = INT_MAX;
    int64_t *d_off;
    int32_t *d_pos;
    int *d_bad;
    double *d_z, *d_tab;
    unsigned long long *d_mk;
    Scratch ws(h, h->ws);
    ws.upload(d_off, n_off_host, (size_t)B + 1).upload(d_bad, &init, 1).buf(d_pos, (size_t)B * Nx)
        .buf(d_z, (size_t)B * pitch).buf(d_mk, (size_t)B * ufg_words(Nx)).upload(d_tab, ufg_scale_table(h, Nx), (size_t)Nx + 1);
    if (const int rc = ws.carve(stream)) return rc;
    if (const int rc = ufg_prepare(B, d_off, nmax, rows, Nx, flux, cmask, d_pos, d_bad, d_z, d_mk, stream)) return rc;
    if (!against) Bn = B;
    const double *zn = against ? static_cast<const double *>(block) : d_z;
    const unsigned long long *mkn = against ? reinterpret_cast<const unsigned long long *>(zn + (size_t)Bn * pitch) : d_mk;
    ufg_pair(B, d_z, d_mk, zn, mkn, Nx, Bn, M, neighbors, d_tab, corr, n_common, metric, stream);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

int underfit_grid_neighbors_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, const double *flux,
                                   const uint8_t *cmask, int M, const int32_t *neighbors, double *corr, int32_t *n_common,
                                   double *metric, hipStream_t stream) {
    return underfit_grid_launch(h, B, n_off_host, rows, Nx, flux, cmask, false, 0, nullptr, M, neighbors, corr, n_common, metric, stream);
}

// ------------------------------------------------------------------------------------------------ prepared neighbour rows, on a grid
// The block: Bn x pitch doubles of z rows, then Bn x pitch / 64 presence words (the row part is a multiple of 1 KiB).
int underfit_grid_rows_bytes(int Bn, int Nx, int64_t *bytes) {
    LK_REQUIRE(Bn >= 1 && Nx >= 1 && Nx <= UFG_MAX_NX, "need Bn >= 1 and 1 <= Nx <= %d (got Bn=%d, Nx=%d)", UFG_MAX_NX, Bn, Nx);
    LK_REQUIRE(bytes != nullptr, "bytes is NULL");
    *bytes = ((int64_t)Bn * uf_pitch(Nx) + (int64_t)Bn * (int64_t)ufg_words(Nx)) * 8;
    return LK_OK;
}

// Workspace: the inverse map pos (Bn x Nx int32).
int underfit_grid_rows_prepare_launch(lk_handle *h, int Bn, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                      const double *flux_nb, const uint8_t *cmask, void *block, int64_t block_bytes,
                                      hipStream_t stream) {
    int64_t nmax = 0, need = 0;
    if (const int rc = ufg_shape_ok(Bn, n_off_host, Nx, &nmax)) return rc;
    LK_REQUIRE(rows && flux_nb, "NULL buffer");
    LK_REQUIRE(block != nullptr && ((uintptr_t)block & 15) == 0, "block must be a 16-byte aligned device buffer");
    if (const int rc = underfit_grid_rows_bytes(Bn, Nx, &need)) return rc;
    LK_REQUIRE(block_bytes >= need, "block too small: %lld bytes given, %d rows on %d grid cadences need %lld "
               "(lk_underfit_grid_rows_bytes)", (long long)block_bytes, Bn, Nx, (long long)need);
    const int init = INT_MAX;
    int64_t *d_off;
    int32_t *d_pos;
    int *d_bad;
    Scratch ws(h, h->ws);
    ws.upload(d_off, n_off_host, (size_t)Bn + 1).upload(d_bad, &init, 1).buf(d_pos, (size_t)Bn * Nx);
    if (const int rc = ws.carve(stream)) return rc;
    double *z = static_cast<double *>(block);
    return ufg_prepare(Bn, d_off, nmax, rows, Nx, flux_nb, cmask, d_pos, d_bad, z,
                       reinterpret_cast<unsigned long long *>(z + (size_t)Bn * uf_pitch(Nx)), stream);
}

int underfit_grid_against_rows_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, const double *flux,
                                      const uint8_t *cmask, int Bn, const void *block, int M, const int32_t *neighbors, double *corr,
                                      int32_t *n_common, double *metric, hipStream_t stream) {
    return underfit_grid_launch(h, B, n_off_host, rows, Nx, flux, cmask, true, Bn, block, M, neighbors, corr, n_common, metric, stream);
}

}  // namespace lk
