// lk_common.hpp — handle, error plumbing and scratch workspace shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lkhip.h"

namespace lk {

void set_error(const char *fmt, ...);

#define LK_HIP_CHECK(expr)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            lk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,    \
                          __LINE__);                                                          \
            return e_ == hipErrorOutOfMemory ? LK_ENOMEM : LK_EHIP;                           \
        }                                                                                     \
    } while (0)

#define LK_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            lk::set_error(__VA_ARGS__);  \
            return LK_EINVAL;            \
        }                                \
    } while (0)

// Grow-only device scratch arena.  Sub-allocations are 256-byte aligned and valid until reset().
// reserve() and alloc() are called only by Scratch (below), by capi.hip's StagedCall and by pld.hip: pld_design_launch and
// dm_pca_launch use the arena as a stack (mark / rewind between phases, a maximum and not a sum), so they stay hand-carved.
struct Arena {
    static constexpr size_t round(size_t bytes) { return (bytes + 255) & ~size_t(255); }  // what one alloc() occupies
    char *base = nullptr;
    size_t cap = 0, used = 0;
    int reserve(size_t bytes);  // ensure capacity (may reallocate: only call before any alloc())
    void *alloc(size_t bytes) {
        size_t a = round(used);
        if (a + bytes > cap) return nullptr;
        used = a + bytes;
        return base + a;
    }
    void reset() { used = 0; }
    void release();
};

// Ring of pinned host buffers for small asynchronous host->device copies (batch offsets): the caller's buffer is
// captured before the entry point returns, and the device copy stays ordered on the caller's stream.
struct HostStage {
    static constexpr int SLOTS = 4;
    void *buf[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[SLOTS] = {0, 0, 0, 0};
    hipEvent_t ev[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int next = 0;
    int copy(void *dst, const void *src, size_t bytes, hipStream_t stream);
    void release();
};
}  // namespace lk

struct lk_handle {
    int device = 0;
    int num_cu = 256;
    int host_chunk_mb = 64;  // MiB of spectra per chunk of the pinned host pipeline (LK_HOST_CHUNK_MB at lk_init, lk_set_host_chunk_mb)
    lk::HostStage stage;
    lk::Arena ws;        // kernel scratch (prepped per-cadence records, per-target stats), carved once per launch through a
                         // lk::Scratch plan (pld.hip's two launchers carve it by hand)
    lk::Arena staging;   // device mirrors of host buffers for the *_batch (host pointer) entry points only, carved per call by
                         // capi.hip's StagedCall (the chunked LS 'fast' pipeline: a lk::Scratch plan of its double buffers)
    // host-pointer pipeline (lk_ls_fast_peaks_batch): copy-in, compute and copy-out streams + the events that order
    // the two halves of the double buffers; created on first use
    hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    int *h_plan = nullptr;         // 64 B of pinned host memory: device -> host plan words (lsfast.hip)
    std::vector<const void *> lds_attr_done;  // kernels whose dynamic-LDS attribute has been raised on this device
    int lds_attr_rc = 0;                      // first failure of want_lds inside a void launch helper (take_lds_error)
    int bls_attr_set = 0;          // bls.hip: kernel attributes set and the LDS-atomic order self-test run on this device
    int bls_serial_hist = 0;       // ... which found ds_add_f64 NOT lane-ordered: the histogram runs its atomic-free form
    int bls_force_serial_hist = 0; // lk_bls_set_ordered_histogram: the caller asked for that form (tests, diagnosis)
    double pld_eig_tol = 0.0;      // lk_pld_set_eig_tolerance: stop of the PLD blocks' subspace iteration (0: the built-in 1e-7)
    // side streams of the handle + fork / join events, created on first use: lsfast.hip runs its chunk loop on two streams, bls.hip
    // spreads the period groups of a small job over four; every call joins them back into the caller's stream before it returns
    hipStream_t s_ls_aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_ls_fork = nullptr, ev_ls_join[3] = {nullptr, nullptr, nullptr};
    // flatten.hip: the batch's two offset tables (cadence offsets | scratch-slab offsets) stay on the device between calls; a
    // call whose tables equal the previous call's (equal-shaped batches, the usual pipeline) skips the copy
    int64_t *flat_tab_dev = nullptr;
    size_t flat_tab_cap = 0;                // entries
    std::vector<int64_t> flat_tab_host;     // what flat_tab_dev holds (empty: nothing valid)
    hipStream_t flat_tab_stream = nullptr;  // the stream the table's upload was queued on (a call on another stream re-uploads)
    // device.hip: lk_shader_clock_mhz's own stream and 16 pinned bytes (kept: freeing either would synchronise the device)
    hipStream_t s_probe = nullptr;
    unsigned long long *clk_buf = nullptr;
    // lsfast.hip: the 1024th roots of unity (1024 x double2, cos | sin), filled once per handle: the column kernel's
    // workgroup-uniform pre-twiddles are read from it through scalar loads
    double *ls_roots = nullptr;
    // neighbors.hip, the metric on a cadence grid: uf_scale(n) for n = 0 .. size - 1, grown on the host as larger grids come (the
    // number of common cadences is known on the device only, and the scale must be the host's bits)
    std::vector<double> uf_scale_tab;
};

namespace lk {
// Kernels that use more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize once per DEVICE (a
// process may drive several GPUs, one handle each): remembered in the handle, not in a function-local static.
inline int want_lds_checked(lk_handle *h, const void *fn, int bytes) {
    LK_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    h->lds_attr_done.push_back(fn);
    return LK_OK;
}
// A failure is returned AND remembered in the handle (lds_attr_rc): launch helpers that return void cannot pass it up, the
// launcher that called them checks take_lds_error() before it reports success.
inline int want_lds(lk_handle *h, const void *fn, int bytes) {
    for (const void *f : h->lds_attr_done)
        if (f == fn) return LK_OK;
    const int rc = want_lds_checked(h, fn, bytes);
    if (rc) h->lds_attr_rc = rc;
    return rc;
}
inline int take_lds_error(lk_handle *h) {
    const int rc = h->lds_attr_rc;
    h->lds_attr_rc = 0;
    return rc;
}

// The device scratch of one launch, in one Arena (h->ws; h->staging for the chunked host pipeline).  The launcher declares
// its buffers in carving order, counts in elements of the pointer's type: buf() is device-only, upload() is also filled from
// host memory through h->stage at carve time; a false condition declares nothing and leaves the pointer null.  carve()
// resets the arena, reserves exactly the declared buffers at Arena::alloc's alignment, sets every pointer (non-null, also
// for a zero-length buffer) and queues the uploads on the stream in declaration order.  No heap allocation per call.
class Scratch {
  public:
    static constexpr int MAX_BUFS = 32;
    Scratch(lk_handle *h, Arena &arena) : h_(h), arena_(arena) {}
    template <class T> Scratch &buf(T *&dev, size_t n, bool on = true) { return add(dev, nullptr, n, on); }
    template <class T> Scratch &upload(T *&dev, const T *host, size_t n, bool on = true) { return add(dev, host, n, on); }
    int carve(hipStream_t stream);  // a failed reserve or placement (LK_ENOMEM / LK_EHIP) leaves every declared pointer null

  private:
    struct Buf {
        void *slot;  // the launcher's device-pointer variable, set through set()
        void (*set)(void *slot, void *dev);
        const void *src;  // upload: host source
        size_t bytes;
    };
    template <class T> static void set_ptr(void *slot, void *dev) { *static_cast<T **>(slot) = static_cast<T *>(dev); }
    template <class T> Scratch &add(T *&dev, const void *src, size_t n, bool on) {
        dev = nullptr;
        if (on && n_ < MAX_BUFS) bufs_[n_] = {&dev, set_ptr<T>, src, n * sizeof(T)};
        if (on) ++n_;  // past MAX_BUFS: counted, carve() refuses
        return *this;
    }
    lk_handle *h_;
    Arena &arena_;
    Buf bufs_[MAX_BUFS];
    int n_ = 0;
};
}  // namespace lk

// launchers implemented in the .hip files (device pointers, enqueue on stream, no sync)
namespace lk {
int ls_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y, const double *dy,
              const double *freq, double f0, double df, int64_t M, int fit_mean, int center_data,
              int normalization, const double *scale, double *power, hipStream_t stream);
int ls_chi2_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y, const double *dy,
                   const double *freq, double f0, double df, int64_t M, int nterms, int fit_mean, int center_data,
                   int normalization, const double *scale, double *power, hipStream_t stream);
int argmax_launch(lk_handle *h, int B, int64_t M, const double *x, double *max_out, int64_t *argmax_out,
                  hipStream_t stream);
int bls_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y, const double *ivar,
               const double *period_host, const double *period_dev, int64_t nP, const double *duration_host,
               int nD, int oversample, int use_likelihood, double *out7, hipStream_t stream);
int bls_max_period_host(const double *duration_host, int nD, int oversample, double *max_period);
int regress_launch(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *X, const double *y,
                   const double *err, const uint8_t *cmask, const double *prior_mu, const double *prior_sigma,
                   double clip_sigma, int niters, double *w, double *model, uint8_t *outl, hipStream_t stream,
                   double *w_cov = nullptr);
int regress_shared_launch(lk_handle *h, int B, int N, int K, const double *X, const double *y, const double *err,
                          const uint8_t *cmask, const double *prior_mu, const double *prior_sigma, double clip_sigma, int niters,
                          double *w, double *model, uint8_t *outl, double *w_cov, hipStream_t stream);
int ridge_prior_launch(lk_handle *h, int B, int N, int K, const double *err, double alpha, const double *alphas, double *prior_mu,
                       double *prior_sigma, hipStream_t stream);
// regress.hip, ragged targets on one shared matrix: cadence numbers -> rows of the grid (pos nullable: the inverse map, B x Nx);
// the fit with target b's cadence i on row rows[n_off[b] + i] of X; the ridge prior over each target's own errors
int align_rows_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *cadenceno, int Nx, const int32_t *grid,
                      int32_t *rows, int32_t *pos, hipStream_t stream);
int regress_shared_rows_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, int K, const double *X,
                               const double *y, const double *err, const uint8_t *cmask, const double *prior_mu,
                               const double *prior_sigma, double clip_sigma, int niters, double *w, double *model, uint8_t *outl,
                               double *w_cov, hipStream_t stream);
int ridge_prior_rows_launch(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *err, double alpha,
                            const double *alphas, double *prior_mu, double *prior_sigma, hipStream_t stream);
int subtract_launch(lk_handle *h, int64_t n, const double *a, const double *b, double *out, hipStream_t stream);
// interp.hip: K shared columns on Nx knots -> every target's own design matrix by PCHIP (include/lkhip.h); synchronises once, for
// the check of the knots.  X_out nullable: the inside bytes alone
int pchip_interp_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, int Nx, int K, const double *knot_time,
                        const double *Y, const uint8_t *knot_keep, int extrapolate, int append_constant, double *X_out,
                        uint8_t *inside, hipStream_t stream);
int underfit_neighbors_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                              const int32_t *neighbors, double *corr, double *metric, hipStream_t stream);
int underfit_rows_bytes(int Bn, int n, int64_t *bytes);
int underfit_rows_prepare_launch(lk_handle *h, int Bn, int N, const double *flux_nb, int n, const int32_t *keep_idx, void *rows,
                                 int64_t rows_bytes, hipStream_t stream);
int underfit_against_rows_launch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int Bn,
                                 const void *rows, int M, const int32_t *neighbors, double *corr, double *metric,
                                 hipStream_t stream);
// regress.hip's rows_pos_kernel: pos[b][rows[n_off[b] + i]] = i, -1 elsewhere (B x Nx); bad[0] (INT_MAX before) = the first target
// whose rows are not strictly increasing indices into [0, Nx).  d_off: the offsets on the device, nmax: the longest target
int rows_pos_launch(int B, const int64_t *d_off, int64_t nmax, const int32_t *rows, int Nx, int32_t *pos, int *bad,
                    hipStream_t stream);
// neighbors.hip, the same metric for ragged targets on a grid of Nx cadences (rows: lk_align_rows_batch's)
int underfit_grid_neighbors_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, const double *flux,
                                   const uint8_t *cmask, int M, const int32_t *neighbors, double *corr, int32_t *n_common,
                                   double *metric, hipStream_t stream);
int underfit_grid_rows_bytes(int Bn, int Nx, int64_t *bytes);
int underfit_grid_rows_prepare_launch(lk_handle *h, int Bn, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                      const double *flux_nb, const uint8_t *cmask, void *block, int64_t block_bytes,
                                      hipStream_t stream);
int underfit_grid_against_rows_launch(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, const double *flux,
                                      const uint8_t *cmask, int Bn, const void *block, int M, const int32_t *neighbors, double *corr,
                                      int32_t *n_common, double *metric, hipStream_t stream);
int overfit_scratch_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes, int *samples_per_round);
int overfit_noise_launch(lk_handle *h, int B, int n, int k, uint64_t seed, int64_t first_target, int64_t stream_id, double *out,
                         hipStream_t stream);
// overfit.hip's batch, two layouts.  uniform: every target has N cadences and keeps the n that ONE keep_idx names (NULL: all, n == N).
// rows: the batch's own offsets, n_off_host (B + 1), keep_idx (target-relative, packed by k_off_host; NULL: all cadences) and
// k_off_host (B + 1 offsets of the kept cadences; NULL with keep_idx == NULL).  The launchers check it.
struct OverfitBatch {
    bool ragged;
    int B, N, n;
    const int64_t *n_off_host, *k_off_host;
    const int32_t *keep_idx;
    static OverfitBatch uniform(int B, int N, int n, const int32_t *keep_idx) { return {false, B, N, n, nullptr, nullptr, keep_idx}; }
    static OverfitBatch rows(int B, const int64_t *n_off_host, const int32_t *keep_idx, const int64_t *k_off_host) {
        return {true, B, 0, 0, n_off_host, k_off_host, keep_idx};
    }
    size_t cad() const { return ragged ? (size_t)k_off_host[B] : (size_t)B * n; }   // the kept cadences of all targets (once checked)
};
int overfit_metric_launch(lk_handle *h, OverfitBatch bt, const double *time, const double *flux_orig, const double *flux_corr,
                          const double *err_corr, double f0, double df, int64_t M, int n_samples, uint64_t seed, int64_t first_target,
                          int64_t stream_id, void *scratch, int64_t scratch_bytes, double *metric, hipStream_t stream);
int overfit_session_begin_launch(lk_handle *h, OverfitBatch bt, const double *time, const double *flux_orig, double f0, double df,
                                 int64_t M, int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *session,
                                 int64_t session_bytes, hipStream_t stream);
int overfit_session_eval_launch(lk_handle *h, OverfitBatch bt, const double *flux_corr, const double *err_corr, double f0, double df,
                                int64_t M, int n_samples, void *session, int64_t session_bytes, double *metric, hipStream_t stream);
int overfit_scratch_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                               int *samples_per_round);
int model_part_launch(lk_handle *h, int B, int N, int K, int c0, int c1, const double *X, const double *w, double *out,
                      hipStream_t stream);
int flatten_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                   const uint8_t *user_mask, int window, int polyorder, double break_tol, int niters, double sigma,
                   double *trend, uint8_t *final_mask, hipStream_t stream);
int savgol_design_host(int window, int polyorder, double *coeffs, double *edge);
int gram_plain_launch(const double *A, const int64_t *d_off, int B, int K, double *G, hipStream_t stream,
                      lk_handle *h = nullptr);
int gram_plain_f32_launch(const float *pix, const float *div, const double *mean, int mode, const int64_t *d_off, int B, int K,
                          double *G, hipStream_t stream, lk_handle *h);
int pld_design_launch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                      const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                      int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, double *X,
                      double *prior_sigma, hipStream_t stream, const int32_t *p_count = nullptr,
                      const int32_t *pb_count = nullptr);
int pld_design_width(int P, int Pb, int pld_order, int pca_components, int n_knots);
int dm_pca_launch(lk_handle *h, int B, int N, int P, int k, const double *A, double *U, hipStream_t stream);
int dm_spline_launch(lk_handle *h, int B, int N, const double *x, const double *knots, int n_inner, int degree, double *out,
                     hipStream_t stream);
int dm_standardize_launch(lk_handle *h, int B, int N, int P, const double *A, double *out, hipStream_t stream);
int fold_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *period_host,
                const double *epoch_time_host, double epoch_phase, const double *wrap_phase_host, int normalize_phase,
                int ncols, const double *const *cols_in, double *const *cols_out, double *phase, int64_t *order,
                hipStream_t stream);
int pg_logmedian_launch(lk_handle *h, int B, int64_t M, const double *power, int K, const int *win_lo_host,
                        const int *win_hi_host, const int *klo_host, const int *khi_host, double corr, double *out,
                        hipStream_t stream);
int pg_boxsmooth_launch(lk_handle *h, int B, int64_t M, const double *power, const double *taps_host, int nk,
                        double *out, hipStream_t stream);
int sigma_clip_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma, int maxiters,
                      uint8_t *outlier, hipStream_t stream);
int ingest_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                  int normalize, double *t_out, double *f_out, double *e_out, int64_t *new_off_host, double *median_out,
                  hipStream_t stream);
// new_off[0..B] = exclusive prefix sums of kept[0..B), both on the device (ingest.hip's one-workgroup scan)
void exscan_i64_launch(const int64_t *kept, int B, int64_t *new_off, hipStream_t stream);
// select.hip: astropy.stats.sigma_clip(y, sigma_lower=, sigma_upper=, maxiters=, cenfunc=median, stdfunc=std).mask per ragged
// row (maxiters < 0: until nothing changes); nothing of the batch's size is carved
int outlier_mask_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma_lower, double sigma_upper,
                        int maxiters, uint8_t *outlier, hipStream_t stream);
// select.hip: lc[mask] (invert: lc[~mask]) for up to 8 columns of 4- or 8-byte elements; new_off_host is valid on return
// (synchronises `stream`)
int select_columns_launch(lk_handle *h, int B, const int64_t *n_off_host, const uint8_t *mask, int invert, int ncols,
                          const int *elem_bytes, const void *const *cols_in, void *const *cols_out, int64_t *new_off_host,
                          hipStream_t stream);
// select.hip: the tail of LightCurve.estimate_cdpp (lightcurve.py:1764-1833, utils.py:374-386) on the cadences outlier[]
// leaves (nullable: all), cdpp_out[B] on the device
int cdpp_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *flat_flux, const uint8_t *outlier,
                int transit_duration, double *cdpp_out, hipStream_t stream);
// fillgaps.hip: LightCurve.fill_gaps for a ragged batch in two calls (the plan synchronises: new_off_host is valid on return) and
// the segment gather of DeviceLightCurveBatch.stitch (include/lkhip.h)
int fill_gaps_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                          const int32_t *cadenceno, double *stats, int32_t *pos, int64_t *new_off_host, hipStream_t stream);
int fill_gaps_launch(lk_handle *h, int B, const int64_t *n_off_host, const int64_t *new_off_host, const double *time,
                     const double *flux, const double *flux_err, const int32_t *quality, const int32_t *cadenceno, const double *stats,
                     const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed, int64_t first_target,
                     int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out, int32_t *quality_out,
                     int32_t *cadenceno_out, uint8_t *inserted, hipStream_t stream);
int gather_segments_launch(lk_handle *h, int S, const int64_t *src_start_host, const int64_t *dst_off_host, int64_t n_src, int ncols,
                           const int *elem_bytes, const void *const *cols_in, void *const *cols_out, hipStream_t stream);
int fits_unpack_launch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                       const int64_t *bitmask_host, double *t_out, double *f_out, double *e_out, int32_t *q_out,
                       int64_t *new_off_host, hipStream_t stream);
int fits_int_column_launch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                           const int32_t *col_host, const int64_t *bitmask_host, const int64_t *new_off_host, int32_t *c_out,
                           hipStream_t stream);
int fits_cube_launch(lk_handle *h, const uint8_t *raw, int row_bytes, int n_rows, int off_time, int code_time, int off_qual,
                     int code_qual, int64_t bitmask, int keep_nan_time, int ncols, const int32_t *col_off_host, int npix,
                     double *t_out, int32_t *q_out, float *cubes_out, int64_t *kept_host, hipStream_t stream);
int transit_mask_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int *p_off_host,
                        const double *period_host, const double *duration_host, const double *transit_time_host,
                        uint8_t *mask, hipStream_t stream);
int bls_stats_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *ivar,
                     const double *period_host, const double *duration_host, const double *transit_time_host,
                     const int64_t *tr_off_host, double *stats, int32_t *tr_first, int32_t *tr_n, int32_t *tr_count, double *tr_ll,
                     double *model, hipStream_t stream);
// lsmodel.hip: LombScargle.model (mle.periodic_fit) of one frequency per target; model / residual nullable
int ls_model_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *dy,
                    const double *frequency_host, int nterms, int fit_mean, int center_data, int keep_mean, double *theta,
                    double *stats, double *model, double *residual, hipStream_t stream);
int ls_model_eval_launch(lk_handle *h, int B, const int64_t *m_off_host, const double *t_fit, const double *t_ref_host,
                         const double *frequency_host, int nterms, const double *theta, const double *stats, double *out,
                         hipStream_t stream);
int bin_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
               const int64_t *bin_off_host, const double *start_host, const double *edges_host, int64_t n_edges,
               double bin_size_sec, const uint8_t *has_err_host, double *t_out, double *f_out, double *e_out,
               hipStream_t stream);
// foldbin.hip: fold + bin by phase.  The plan (one pass, no sort; plan_host is valid on return), cycle / odd / even of a folded
// batch, the bins of a folded batch (median: nanmedian flux) and the fused form on the unfolded batch (include/lkhip.h)
int fold_bin_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                         const double *period_host, const double *epoch_time_host, int epoch_given, double epoch_phase,
                         const double *wrap_phase_host, int normalize_phase, const double *count_from_host, double *plan_host,
                         hipStream_t stream);
int fold_cycle_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int64_t *order,
                      const double *period_host, const double *cycle_epoch_host, const double *cycle_min_host, int64_t *cycle,
                      uint8_t *odd, uint8_t *even, hipStream_t stream);
int phase_bin_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *phase, const double *flux, const double *err,
                     const uint8_t *sel, int sel_value, const int64_t *bin_off_host, const double *start_host,
                     const double *size_sec_host, const double *edges_host, const uint8_t *has_err_host, int median,
                     double *phase_out, double *flux_out, double *err_out, int32_t *count_out, hipStream_t stream);
int fold_bin_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                    const double *period_host, const double *epoch_time_host, double epoch_phase, const double *wrap_phase_host,
                    int normalize_phase, const double *cycle_epoch_host, const double *plan_host, int which,
                    const int64_t *bin_off_host, const double *start_host, const double *size_sec_host, const double *edges_host,
                    double *phase_out, double *flux_out, double *err_out, int32_t *count_out, hipStream_t stream);
// river.hip: river diagrams (cycle x phase images) of the unfolded batch.  The plan (one pass; plan_host is valid on return) and
// the images on the layout the caller formed from it (include/lkhip.h); route nullable
int river_plan_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                      const double *period_host, const double *epoch_time_host, int epoch_given, double *plan_host,
                      hipStream_t stream);
int river_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *err,
                 const double *period_host, const double *epoch_time_host, const double *plan_host, int method,
                 const int32_t *n_bins_host, const int32_t *n_cycles_host, const int64_t *cell_off_host, const double *edges_host,
                 double *river, int32_t *count, int32_t *route, hipStream_t stream);
int pg_acf2d_launch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int *win_start_host, int W,
                    double *acf2d, double *metric, hipStream_t stream);
// pgsmooth.hip, the resident seismology chain: metric of the 2-D ACF alone; power / background; Gaussian smoothing and
// argmax of the metric (taps_host nullable: no smoothing); deltanu of B targets with their own windows (acf nullable)
int pg_acf_metric_launch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int *win_start_host, int W,
                         double *metric, hipStream_t stream);
int pg_snr_launch(lk_handle *h, int B, int64_t M, const double *power, const double *bkg, double *out,
                  hipStream_t stream);
int pg_numax_pick_launch(lk_handle *h, int B, int n_win, const double *metric, const double *taps_host, int nk,
                         double *metric_smooth, int64_t *argmax_out, hipStream_t stream);
int pg_deltanu_launch(lk_handle *h, int B, int64_t M, const double *power, const int *start_host, const int *width_host,
                      const double *emp_host, const double *distance_host, const double *step_host,
                      const double *stop_host, int max_sel, double *deltanu, int *n_peaks, int *status, int *sel_lo,
                      int *sel_len, double *acf, hipStream_t stream);
int cube_aperture_launch(lk_handle *h, int B, int N, int npix, const float *flux, const float *flux_err, const uint8_t *mask,
                         int mask_stride, float *flux_out, float *err_out, uint8_t *keep_out, int64_t *kept_host,
                         int64_t *nonfinite_host, hipStream_t stream);
int cube_median_image_launch(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *keep, double *median,
                             hipStream_t stream);
int pld_gather_launch(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time, const float *flux32,
                      const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx_host, int pld_idx_stride, int Pb,
                      const int32_t *bkg_idx_host, int bkg_idx_stride, int n_inner, const int32_t *knot_lo_host,
                      const double *knot_g_host, double *t_out, double *y_out, double *err_out, float *lcf_out, float *pld_out,
                      float *bkg_out, double *knots_out, int *nonfinite_host, hipStream_t stream,
                      const int32_t *pld_idx_dev = nullptr, const int32_t *bkg_idx_dev = nullptr);
int cube_threshold_mask_launch(lk_handle *h, int B, int ny, int nx, const double *median, double threshold, int use_ref,
                               double ref_col, double ref_row, int invert, uint8_t *mask, int32_t *count, int32_t *idx,
                               hipStream_t stream);
int pld_corrected_launch(lk_handle *h, int B, int N, const double *y, const double *model, const double *spline, double *out,
                         hipStream_t stream);
// pixcube.hip: TargetPixelFile.estimate_centroids(method='moments') per cadence of every cutout
int cube_centroids_launch(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask, int mask_stride,
                          double column0, double row0, double *col_out, double *row_out, hipStream_t stream);
// pixcube.hip: estimate_centroids(method='quadratic') per cadence (peak_out nullable); either estimator on B float64 images
int cube_centroids_quadratic_launch(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                    int mask_stride, double column0, double row0, double *col_out, double *row_out,
                                    int32_t *peak_out, hipStream_t stream);
int image_centroids_launch(lk_handle *h, int B, int npix, int nx, const double *image, const uint8_t *mask, int mask_stride,
                           double column0, double row0, int method, double *col_out, double *row_out, int32_t *peak_out,
                           hipStream_t stream);
// pixcube.hip: the transit difference images of B resident cutouts, one box per cutout (host arrays); then the centroid offsets
// and statuses of these (n_in / n_out, fit_status NULL) or of the amplitude images (fit_status, n_in / n_out NULL).  Everything
// else on the device; enqueued, no synchronisation
int cube_diffimage_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const float *flux_err,
                          const double *period_host, const double *transit_time_host, const double *duration_host, double in_width,
                          double out_inner, double out_outer, uint8_t *cls, double *mean_in, double *mean_out, double *diff,
                          double *diff_err, int32_t *n_in, int32_t *n_out, hipStream_t stream);
int centroid_offsets_launch(lk_handle *h, int B, const int32_t *fit_status, const int32_t *n_in, const int32_t *n_out,
                            const double *a_col, const double *a_row, const double *b_col, const double *b_row, double *offset,
                            double *offset_pix, int32_t *status, hipStream_t stream);
// pixcube.hip: TargetPixelFile.estimate_background per cadence (nanmedian of the masked pixels, their count, optionally the
// median absolute deviation) and, with cube_out, the subtracted cube from the same pass; cube - rows[b][i] for given rows.
// Enqueued, no synchronisation, no scratch
int cube_background_launch(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *mask, int mask_stride,
                           int want_scatter, float *bkg, int32_t *n_pixels, float *scatter, float *cube_out, hipStream_t stream);
int cube_subtract_rows_launch(lk_handle *h, int B, int N, int npix, const float *cube, const float *rows, float *cube_out,
                              hipStream_t stream);
// ampimage.hip: the per-pixel sinusoid fit of B resident cutouts at one frequency each (host arrays), coefficient- and harmonic-
// major images (offsets and statuses: centroid_offsets_launch).  Everything else on the device; enqueued, no synchronisation
int cube_ampimage_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency_host,
                         int nterms, const double *t_ref_host, double *theta, double *level, double *amplitude, double *phase,
                         double *amplitude_err, double *snr, double *chi2, int32_t *n_used, int32_t *fit_status,
                         hipStream_t stream);
// pixelpg.hip: the per-pixel Lomb-Scargle periodograms of B resident cutouts on one shared grid (host array, 1/d), their peak
// images and, where power is not NULL, the power cube [B][F][npix].  Everything else on the device; enqueued, no synchronisation
int cube_pixelpg_launch(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency_host,
                        int F, int normalization, double oversample_factor, const double *t_ref_host, double *power,
                        double *peak_power, int32_t *peak_index, int32_t *n_used, int32_t *status, hipStream_t stream);
// psfphot.hip: deblended PSF photometry per cadence of B resident cutouts — the fluxes of up to 8 stars at known positions (host
// arrays, NaN = no star) and a constant background by weighted least squares; star_off_host (nullable) receives the row
// offsets.  Everything else on the device; enqueued, no synchronisation
int cube_psfphot_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                        const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                        const double *sigma_host, const double *shift_col, const double *shift_row, double column0, double row0,
                        int use_flux_err, int32_t *star_off_host, double *time_out, double *flux_out, double *flux_err_out, double *background,
                        double *chi2, int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream);
// prfphot.hip: cube_psfphot_launch with a tabulated PRF in place of the widths — prf_table DEVICE float32 [n_prf][Ty][Tx],
// prf_index_host HOST [B] or NULL (table 0); Keys' cubic convolution on the table continued by zeros (lkhip.h)
int cube_prfphot_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                        const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                        const float *prf_table, int n_prf, int Ty, int Tx, int oversample, const int32_t *prf_index_host,
                        const double *shift_col, const double *shift_row, double column0, double row0, int use_flux_err,
                        int32_t *star_off_host, double *time_out, double *flux_out, double *flux_err_out, double *background,
                        double *chi2, int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream);
// psffit.hip: the same fit with one common (column, row) shift per cadence fitted next to the fluxes, by variable projection from
// shift0 (nullable device arrays): fluxes, background and chi2 at the fitted shift, the shifts, their errors, the iterations
// taken and the last step.  Everything but the stars on the device; enqueued, no synchronisation
int cube_psffit_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const double *sigma_host, const double *shift0_col, const double *shift0_row, int max_iter, double tol,
                       double max_step, double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off_host,
                       double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2, double *shift_col,
                       double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step, int32_t *n_iter,
                       int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream);
// prffit.hip: cube_psffit_launch with a tabulated PRF in place of the widths (the table arguments of cube_prfphot_launch): the
// model and its derivative by the shift come from the table by Keys' cubic convolution (lkhip.h)
int cube_prffit_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const float *prf_table, int n_prf, int Ty, int Tx, int oversample, const int32_t *prf_index_host,
                       const double *shift0_col, const double *shift0_row, int max_iter, double tol, double max_step,
                       double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off_host, double *time_out,
                       double *flux_out, double *flux_err_out, double *background, double *chi2, double *shift_col,
                       double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step, int32_t *n_iter,
                       int32_t *n_used, int8_t *cadence_status, int32_t *status, hipStream_t stream);
// psfwidth.hip: the PSF width (sigma_col, sigma_row) of every cutout, shared by its cadences, by variable projection from sigma0
// (host array) at given shifts (nullable device arrays) on the cadences of cadence_mask (nullable device bytes): max_iter + 1
// pairs of an evaluate and a step kernel.  Everything but the stars and sigma0 on the device; enqueued, no synchronisation
int cube_psfwidth_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                         const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                         const double *sigma0_host, const double *shift_col, const double *shift_row, const uint8_t *cadence_mask,
                         int max_iter, double tol, double max_step, double min_sigma, double max_sigma, double column0, double row0,
                         int use_flux_err, double *sigma, double *sigma_err, double *sigma_cov, double *chi2, double *last_step,
                         double *trace, int32_t *n_iter, int32_t *n_cadences, int64_t *n_pixels, int8_t *cadence_status,
                         int32_t *status, hipStream_t stream);
// psfpos.hip: the (column, row) of every fitted star of every cutout, shared by its cadences, by variable projection from the given
// positions (host arrays; fit_star_host nullable host bytes [B][S_max], non-zero = fitted) at given shifts (nullable device
// arrays) on the cadences of cadence_mask (nullable device bytes): max_iter + 1 pairs of an evaluate and a step kernel.
// Everything but the stars, sigma and fit_star on the device; enqueued, no synchronisation
int cube_psfpos_launch(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux, const float *flux_err,
                       const uint8_t *mask, int mask_stride, int S_max, const double *star_col_host, const double *star_row_host,
                       const double *sigma_host, const uint8_t *fit_star_host, const double *shift_col, const double *shift_row,
                       const uint8_t *cadence_mask, int max_iter, double tol, double max_step, double max_offset, double column0,
                       double row0, int use_flux_err, double *star_col, double *star_row, double *star_col_err, double *star_row_err,
                       double *position_cov, double *chi2, double *last_step, double *trace, int32_t *n_iter, int32_t *n_cadences,
                       int64_t *n_pixels, int8_t *cadence_status, int32_t *status, hipStream_t stream);
// sff.hip: SFFCorrector for a ragged resident batch.  The regression launcher owns h->ws, so the design matrices and everything
// else that lives across it sit in `scratch`, a device block of the caller's (sff_scratch_bytes); status_host is valid on
// return (the call synchronises once, to group the targets by their design width)
int sff_scratch_bytes(int B, const int64_t *n_off, const int32_t *n_knots, const int32_t *win_off, int bins, int degree,
                      int64_t max_scratch_bytes, int64_t *bytes, int *n_chunks);
int sff_arclength_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *col, const double *row, double *arc,
                         int32_t *flipped, hipStream_t stream);
int sff_design_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *err,
                      const double *arc, const int32_t *win_off_host, const int32_t *wp_host, int bins, int degree, int n_knots,
                      double *X, double *prior_mu, double *prior_sigma, double *knots_time, double *knots_win, double *f_out,
                      double *e_out, hipStream_t stream);
int sff_correct_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux, const double *err,
                       const double *col, const double *row, const uint8_t *cmask, const int32_t *win_off_host,
                       const int32_t *wp_host, int bins, int degree, double timescale, int restore_trend, double clip_sigma,
                       int niters, void *scratch, int64_t scratch_bytes, double *flux_out, double *err_out, uint8_t *outl_out,
                       int32_t *status_host, double *arclength, double *spline, double *sff, double *w, int w_pitch,
                       hipStream_t stream);
// rebase: t holds absolute times, the launcher works on t - t[first cadence] per target (carved in its own plan)
int lsfast_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y, const double *dy,
                  double f0, double df, int64_t M, int fit_mean, int center_data, int normalization,
                  const double *scale, int oversampling, double *power, hipStream_t stream, double *max_out = nullptr,
                  int64_t *arg_out = nullptr, bool rebase = false);
// out = t - t[first cadence] per target, out of place (device.hip); d_off is the batch's offsets on the device
int rebase_launch(int B, const int64_t *d_off, const double *t, double *out, hipStream_t stream);
int lsfastchi2_launch(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y, const double *dy,
                      double f0, double df, int64_t M, int nterms, int fit_mean, int center_data, int normalization,
                      const double *scale, int oversampling, double *power, hipStream_t stream);
}  // namespace lk
