/* lkhip.h — C ABI of liblkhip.so: the MI355X (gfx950) hot path of lightkurve's periodogram +
 * systematics-correction pipeline.  Plain pointers and sizes only; no torch / numpy types.
 *
 * lightkurve is pure Python and has no FFI of its own; each entry point below replaces the numerical
 * call the reference makes at one of its four seams:
 *
 *   lk_ls_power_batch*   <- astropy METHODS[method](t, y, dy, frequency, center_data, fit_mean, normalization)
 *                           reached from src/lightkurve/periodogram.py:961-964 (LS.power(frequency, method=ls_method)),
 *                           plus lightkurve's own normalisation lines periodogram.py:969-975 (fused).
 *   lk_argmax_batch*     <- Periodogram.max_power / frequency_at_max_power, periodogram.py:127-140 (nanmax/nanargmax).
 *   lk_bls_batch*        <- astropy methods.bls_fast(t, y, ivar, period, duration, oversample, use_likelihood)
 *                           == C run_bls(...), reached from periodogram.py:1169 (bls.power(period, duration, **kwargs)).
 *   lk_savgol_trend_batch* <- scipy.signal.savgol_filter + interp1d inside LightCurve.flatten,
 *                           src/lightkurve/lightcurve.py:996-1063.
 *   lk_regress_batch*    <- RegressionCorrector._fit_coefficients + the sigma-clip loop of .correct,
 *                           src/lightkurve/correctors/regressioncorrector.py:127-189, 243-279.
 *   lk_regress_shared_batch*  the same for B targets on ONE shared design matrix (CBVCorrector.correct_gaussian_prior).
 *   lk_regress_shared_rows_batch* / lk_align_rows_batch*  the same for RAGGED targets, each cadence on its own row of the
 *                           shared matrix (CotrendingBasisVectors.align(lc) by CADENCENO before the correction).
 *   lk_underfit_neighbors_batch* <- correctors.metrics.underfit_metric_neighbors + _compute_correlation,
 *                           src/lightkurve/correctors/metrics.py:141-257, 451-475, neighbours = other targets of the batch.
 *   lk_overfit_metric_batch* <- correctors.metrics.overfit_metric_lombscargle, src/lightkurve/correctors/metrics.py:24-138,
 *                           for B targets at once, the white noise made on the device (Philox4x32-10).
 *   lk_ls_fast_batch*    <- astropy lombscargle_fast (the DEFAULT ls_method="fast", periodogram.py:650): fast_impl.py.
 *   lk_ls_chi2_batch* / lk_ls_fastchi2_batch* <- astropy lombscargle_chi2 / lombscargle_fastchi2 (nterms > 1,
 *                           periodogram.py:948-967).
 *   lk_pld_design_batch* <- PLDCorrector.create_design_matrix, src/lightkurve/correctors/pldcorrector.py:125-287.
 *   lk_pld_correct_batch <- PLDCorrector.correct (pldcorrector.py:304-427) for a batch of cutouts: the two above fused, the
 *                           design matrices staying in device memory.
 *   lk_cube_aperture_batch_dev / lk_cube_median_image_batch_dev / lk_pld_gather_batch_dev <- what PLDCorrector does to a
 *                           TargetPixelFile before that (aperture photometry, NaN cadences, threshold-mask median image,
 *                           pixel series, knots) for cubes resident in device memory; lk_pld_correct_batch_dev follows.
 *   lk_cube_threshold_mask_batch_dev <- the rest of create_threshold_mask (MAD cut, 4-connected labelling, nearest region) on
 *                           those median images, in device memory: masks, pixel counts and index lists per cutout.
 *   lk_pld_gather_ragged_batch_dev / lk_pld_correct_ragged_batch* <- the same PLD call for cutouts whose PLD / background
 *                           masks select DIFFERENT numbers of pixels (the reference's K2 defaults: 'threshold' /
 *                           'background'): zero-padded pixel blocks of one row pitch plus per-cutout counts.  Limits that
 *                           remain: one kept-cadence count per call, every count >= pca_components.
 *   lk_fold_batch*       <- LightCurve.fold, src/lightkurve/lightcurve.py:1089-1214 (astropy TimeSeries.fold + sort).
 *   lk_fold_bin_plan_batch* / lk_fold_bin_batch* / lk_phase_bin_batch_dev / lk_fold_cycle_batch_dev <- lc.fold(...).bin(...),
 *                           optionally of the odd or even cycles only: fused without a sort, or on a folded batch (also nanmedian).
 *   lk_river_plan_batch* / lk_river_batch* <- the image behind LightCurve.plot_river (lightkurve 2.x): cycles x phase bins per target.
 *   lk_pg_logmedian_batch* / lk_pg_boxsmooth_batch* <- Periodogram.smooth, periodogram.py:182-284.
 *   lk_pg_snr_batch_dev / lk_pg_acf_metric_batch_dev / lk_pg_numax_pick_batch_dev / lk_pg_deltanu_batch* <- flatten,
 *                           estimate_numax and estimate_deltanu (seismology/) on spectra that stay in device memory.
 *   lk_sff_correct_batch* / lk_sff_arclength_batch* / lk_cube_centroids_batch_dev <- SFFCorrector.correct (correctors/
 *                           sffcorrector.py, lightkurve 2.x) and TargetPixelFile.estimate_centroids(method='moments') for a resident
 *                           batch: arclength, percentile knots, the block-structured design matrix, the fit, the components.
 *
 * Conventions
 *   - Every function returns an int status: LK_OK, LK_EINVAL (-> ValueError), LK_ENOMEM (-> MemoryError),
 *     LK_EHIP (-> RuntimeError; text from lk_last_error()).  Outputs are fully written on LK_OK.
 *   - Ragged batches: target b owns elements [n_off[b], n_off[b+1]) of the concatenated arrays.
 *   - `*_batch` takes HOST pointers (caller-owned numpy buffers; copied in/out inside the call).
 *     `*_batch_dev` takes DEVICE pointers (already resident in HBM) and enqueues on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream) without synchronising.
 *     Some `_dev` launchers synchronise `stream` internally where the host needs a device result to size
 *     the next launch (fold, flatten, BLS, Periodogram.smooth, PLD); treat "no sync" as not guaranteed.
 *   - One lk_handle drives one GPU (one process per GPU); it owns its scratch workspace and is not
 *     thread-safe.  ALL calls on one handle must use ONE stream (or be separated by a stream/device
 *     synchronisation): every launcher carves its kernel scratch from the handle's single arena, so two calls
 *     in flight on different streams would overwrite each other's live scratch.  Use one handle per stream /
 *     per thread if you need concurrency on one GPU.  (Inside a call the library may fork side streams of its own —
 *     lk_ls_fast_* runs its chunks on two, lk_bls_* spreads the period groups of a small job over four — and joins them
 *     back into `stream` by events before it returns: to the caller the call is still ordered on `stream`.)
 *     Multi-GPU = one handle per rank, targets sharded by the caller (no data-path collective).
 *   - Deviations from the ABI sketched in SURVEY.md §8(b), on purpose: lk_init takes ONE device id (one handle
 *     = one GPU = one process, the torch.distributed model; the sketch's device list would put multi-GPU fan-out
 *     inside the call); there is no `precision` argument (everything is fp64: the parity tolerance of 1e-9
 *     against the reference leaves no room for fp32/mixed variants); (max, argmax) come from lk_argmax_batch*
 *     or the fused lk_ls_fast_peaks_batch* rather than from extra outputs of lk_ls_power_batch.
 */
#ifndef LKHIP_H
#define LKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_OK 0
#define LK_EINVAL 1
#define LK_ENOMEM 2
#define LK_EHIP 3

/* LS normalisations: astropy 'standard', astropy 'psd', lightkurve 'amplitude' (periodogram.py:974-975),
 * lightkurve 'psd' (periodogram.py:969-973; needs per-target scale = 2/(N*oversample*fs)). */
#define LK_NORM_STANDARD 0
#define LK_NORM_PSD 1
#define LK_NORM_LK_AMPLITUDE 2
#define LK_NORM_LK_PSD 3

typedef struct lk_handle lk_handle;

int lk_version(void);
const char *lk_last_error(void);
int lk_device_count(int *count);
int lk_init(int device_id, lk_handle **out);
/* Chunk size (MiB of spectra) of the pinned, double-buffered host pipeline behind lk_ls_fast_*_batch; default 64, or the
 * environment variable LK_HOST_CHUNK_MB read once by lk_init — the library's only environment knob. */
int lk_set_host_chunk_mb(lk_handle *h, int mb);
/* BLS histogram form.  The fast form adds a wave's 64 cadences to their phase bins with one LDS ds_add_f64 per array and
 * relies on the hardware applying same-address lanes in lane order (checked on the device, once per handle); where that
 * check fails the library switches by itself to an atomic-free form in which one lane at a time updates its bins —
 * bit-identical results, ~64 x the LDS instructions in the histogram phase.  on != 0 forces that form (tests, diagnosis of
 * a suspected ordering problem); 0 returns to the automatic choice. */
int lk_bls_set_ordered_histogram(lk_handle *h, int on);
/* Stop criterion of the subspace iteration behind the PCA blocks of lk_pld_design_batch* / lk_pld_correct_batch
 * (DesignMatrix.pca inside PLDCorrector.create_design_matrix, correctors/designmatrix.py:252-282): residual
 * ||C r - theta r|| <= tol * theta_max * sqrt(k).  Default (tol = 0) 1e-7: two decades below the first visible change of the
 * corrected flux on the reference goldens (profiles/r05_pld_tol_sweep.txt).  lk_pca_batch (whose OUTPUT is the basis) always
 * uses 1e-10. */
int lk_pld_set_eig_tolerance(lk_handle *h, double tol);
void lk_destroy(lk_handle *h);
/* Block until every kernel / copy issued through this handle's GPU has finished (hipDeviceSynchronize): for callers
 * of the *_dev entry points that do not hold a HIP runtime of their own. */
int lk_synchronize(lk_handle *h);
/* bytes of device scratch currently held by the handle */
int64_t lk_workspace_bytes(const lk_handle *h);

/* ---- Lomb-Scargle (exact floating-mean GLS, direct trig sums) --------------------------------------
 * t: times relative to the target's first cadence [d] (astropy: lombscargle/core.py:119-126);
 * y: flux; dy: per-cadence errors or NULL (uniform weights, the lightkurve default);
 * freq: M frequencies [1/d] or NULL for the regular grid f0 + df*j, j<M (the fast path);
 * scale: per-target factor for LK_NORM_LK_PSD, or NULL (=1); power: B*M row-major, float64. */
int lk_ls_power_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                      const double *dy, const double *freq, double f0, double df, int64_t M,
                      int fit_mean, int center_data, int normalization, const double *scale,
                      double *power);
int lk_ls_power_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                          const double *dy, const double *freq, double f0, double df, int64_t M,
                          int fit_mean, int center_data, int normalization, const double *scale,
                          double *power, void *stream);

/* ---- Lomb-Scargle with nterms Fourier terms (lightkurve nterms > 1 with ls_method "chi2" / "fastchi2",
 * periodogram.py:948-967): astropy lombscargle_chi2 (chi2_impl.py:5-86), i.e. at every frequency the weighted
 * least-squares fit of [1,] sin(m w t), cos(m w t), m = 1..nterms; power = (X^T y)^T (X^T X)^-1 (X^T y), normalised as
 * above.  The trig sums are exact direct sums, so the result is what 'chi2' returns (which 'fastchi2' approximates by
 * extirpolation + FFT).  nterms = 1 is lk_ls_power_batch.  1 <= nterms <= LK_MAX_NTERMS. */
#define LK_MAX_NTERMS 8   /* 1..4: regular-grid and FFT kernels; 5..8: exact sums, one thread per frequency (both names) */
int lk_ls_chi2_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                     const double *freq, double f0, double df, int64_t M, int nterms, int fit_mean, int center_data,
                     int normalization, const double *scale, double *power);
int lk_ls_chi2_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                         const double *dy, const double *freq, double f0, double df, int64_t M, int nterms,
                         int fit_mean, int center_data, int normalization, const double *scale, double *power,
                         void *stream);

/* ---- Lomb-Scargle ls_method="fastchi2" with nterms Fourier terms (periodogram.py:948-967): astropy
 * lombscargle_fastchi2 (fastchi2_impl.py:60-137) — the multi-term fit of lk_ls_chi2_batch with every trig sum taken
 * from the extirpolated FFT grids (3 nterms grids per target), regular frequency grid only.  Agrees with the
 * reference's 'fastchi2' output to ~1e-9 where the fit is well posed.  nterms = 1 is lk_ls_fast_batch. */
int lk_ls_fastchi2_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                         double f0, double df, int64_t M, int nterms, int fit_mean, int center_data, int normalization,
                         const double *scale, int oversampling, double *power);
int lk_ls_fastchi2_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                             const double *dy, double f0, double df, int64_t M, int nterms, int fit_mean,
                             int center_data, int normalization, const double *scale, int oversampling, double *power,
                             void *stream);

/* ---- LightCurve.fold (src/lightkurve/lightcurve.py:1089-1214 over astropy TimeSeries.fold, timeseries/sampled.py:
 * 230-233) for B ragged targets: phase = ((t - epoch_time) + epoch_phase + (P - wrap)) % P - (P - wrap) (numpy `%`),
 * divided by P if normalize_phase (epoch_phase and wrap_phase are then in phase units), followed by a STABLE sort by
 * phase.  period / epoch_time / wrap_phase: one value per target (HOST arrays).  Outputs, all in sorted order:
 * phase[sum N], order[sum N] (index of the cadence, relative to its target, that lands at each sorted slot) and
 * cols_out[c][i] = cols_in[c][order[i]] for ncols value columns (flux, flux_err, ...).  The phases are bit-identical
 * to numpy's and the permutation equals np.argsort(phase, kind="stable"). */
int lk_fold_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *period,
                  const double *epoch_time, double epoch_phase, const double *wrap_phase, int normalize_phase,
                  int ncols, const double *const *cols_in, double *const *cols_out, double *phase, int64_t *order);
int lk_fold_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *period,
                      const double *epoch_time, double epoch_phase, const double *wrap_phase, int normalize_phase,
                      int ncols, const double *const *cols_in, double *const *cols_out, double *phase, int64_t *order,
                      void *stream);

/* ---- Periodogram.smooth / Periodogram.flatten (src/lightkurve/periodogram.py:182-284, 381-429) for B periodograms on
 * one shared frequency grid of M points, power row-major [B][M].
 *
 * lk_pg_logmedian_batch: method='logmedian' (:265-284).  The caller prepares the window bookkeeping from the
 * frequency grid exactly as the reference loop does (numpy log10 of the frequencies; window centres by the running
 * sum x0 += 0.5 * filter_width; membership |log10 f - x0| < filter_width): window k covers the frequency indices
 * [win_lo[k], win_hi[k]) and frequency j lies in the windows klo[j] .. khi[j] (inclusive; klo > khi = none).  Per
 * window: nanmedian(power) / corr (corr = (8/9)^3); per frequency: mean of its windows' values, summed in window
 * order.  All four tables are HOST arrays (also for the _dev flavour).
 *
 * lk_pg_boxsmooth_batch: method='boxkernel' (:236-263) = astropy.convolution.convolve(power, Box1DKernel(width)) with
 * its defaults boundary='fill' (zeros), normalize_kernel=True, nan_treatment='interpolate'.  taps = the kernel array
 * (flipped; nk odd), HOST array.  flatten = power / smooth is left to the caller (one division). */
int lk_pg_logmedian_batch(lk_handle *h, int B, int64_t M, const double *power, int K, const int32_t *win_lo,
                          const int32_t *win_hi, const int32_t *klo, const int32_t *khi, double corr, double *out);
int lk_pg_logmedian_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int K, const int32_t *win_lo,
                              const int32_t *win_hi, const int32_t *klo, const int32_t *khi, double corr, double *out,
                              void *stream);
int lk_pg_boxsmooth_batch(lk_handle *h, int B, int64_t M, const double *power, const double *taps, int nk,
                          double *out);
int lk_pg_boxsmooth_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const double *taps, int nk,
                              double *out, void *stream);

/* ---- seismology 2-D autocorrelation (src/lightkurve/seismology/numax_estimators.py:15-205 over seismology/utils.py:
 * 106-158): for n_win windows of W samples starting at win_start[k] (HOST array) of each of B periodograms on one grid,
 * the autocorrelation C[lag] = sum_i p[i] p[i + lag], lag < W, of the window minus its nanmean, and the mean collapsed
 * correlation metric[k] = (sum_lag |C[lag]| - 1) / W.  acf2d: B x n_win x W (window-major); metric: B x n_win. */
int lk_pg_acf2d_batch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start, int W,
                      double *acf2d, double *metric);
int lk_pg_acf2d_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start,
                          int W, double *acf2d, double *metric, void *stream);

/* ---- the seismology chain on spectra that stay in HBM (flatten -> estimate_numax -> estimate_deltanu of
 * src/lightkurve/seismology/; device.DevicePeriodogramBatch).  B periodograms on one grid of M points, row-major [B][M].
 *
 * lk_pg_snr_batch_dev: out = power / bkg, element by element in IEEE double (Periodogram.flatten's division,
 * periodogram.py:381-429, after lk_pg_logmedian_batch_dev or lk_pg_boxsmooth_batch_dev made bkg).
 *
 * lk_pg_acf_metric_batch_dev: the `metric` of lk_pg_acf2d_batch_dev, bit for bit, without its acf2d output (the numax
 * estimator reads nothing else; B x n_win doubles leave the chip instead of B x n_win x W).
 *
 * lk_pg_numax_pick_batch_dev: the tail of estimate_numax_acf2d (numax_estimators.py:181-186), one workgroup per target:
 * metric_smooth[b] = metric[b] convolved with the n_taps taps (HOST array: the normalised Gaussian1DKernel, n_taps odd;
 * boundary='extend', i.e. the end values replicated; products summed in tap order), or a copy of metric[b] when
 * n_taps == 0 (metric_smooth may then be metric itself); argmax_out[b] = np.argmax(metric_smooth[b]): the first maximum,
 * a NaN counts as the maximum.  metric, metric_smooth: B x n_win; argmax_out: int64[B].
 *
 * lk_pg_deltanu_batch(_dev): estimate_deltanu_acf2d (deltanu_estimators.py:18-153) for B targets, each with its OWN
 * window, one workgroup per target.  HOST tables, one entry per target, which the caller derives from the target's numax
 * with the reference's scalar arithmetic (lightkurve_amd/seismology.py::_deltanu_plan): start / width = first sample and
 * number W of samples of the window (numax -+ one envelope FWHM); deltanu_emp = 0.294 numax^0.772 (NaN: skip the target);
 * distance = floor(deltanu_emp / 2 / fs); step, stop = the reference's lags np.linspace(0, W fs, W): lag i = i * step,
 * the last one = stop (the grid spacing fs enters through these three only).  Per target: the window minus its nanmean,
 * C[0] and C[lag] for the lags with `lag > emp - 0.25 emp and lag < emp + 0.25 emp` alone (the same bits as
 * lk_pg_acf2d_batch gives that window), acf = (|C^2| / |C[0]^2|) / (3 / (2 W)), scipy.signal.find_peaks(acf[sel],
 * distance=distance) (plateau midpoints, no peak at either end of the slice, highest peak first and its neighbours
 * closer than ceil(distance) dropped; of peaks of exactly equal height the later one is served first, as a stable
 * argsort orders them -- scipy's own argsort is unstable and agrees with that on short peak lists), and
 * deltanu = the lag of the surviving peak closest to deltanu_emp (the first of equally close ones).
 * Outputs [B]: deltanu (NaN unless status 0), n_peaks (surviving peaks), sel_lo / sel_len (the selected lags), status:
 * 0 ok; 1 skipped (deltanu_emp NaN); 2 the window is not inside [0, M), has fewer than 2 or more than 16384 samples, or
 * does not fit the 160 KB of LDS together with its selection; 3 nothing to pick (no local maximum inside the
 * selection, or distance < 1, where scipy raises).  No error is raised for a target.  acf (nullable): B x max_sel, row b =
 * the rescaled ACF on the selection (sel_len[b] values, at most max_sel are written), NaN behind it. */
int lk_pg_snr_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const double *bkg, double *out,
                        void *stream);
int lk_pg_acf_metric_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start,
                               int W, double *metric, void *stream);
int lk_pg_numax_pick_batch_dev(lk_handle *h, int B, int n_win, const double *metric, const double *taps, int n_taps,
                               double *metric_smooth, int64_t *argmax_out, void *stream);
int lk_pg_deltanu_batch(lk_handle *h, int B, int64_t M, const double *power, const int32_t *start, const int32_t *width,
                        const double *deltanu_emp, const double *distance, const double *step, const double *stop,
                        int max_sel, double *deltanu, int32_t *n_peaks, int32_t *status, int32_t *sel_lo,
                        int32_t *sel_len, double *acf);
int lk_pg_deltanu_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const int32_t *start,
                            const int32_t *width, const double *deltanu_emp, const double *distance, const double *step,
                            const double *stop, int max_sel, double *deltanu, int32_t *n_peaks, int32_t *status,
                            int32_t *sel_lo, int32_t *sel_len, double *acf, void *stream);

/* ---- Lomb-Scargle, lightkurve's DEFAULT method ls_method="fast" (periodogram.py:650): Press & Rybicki extirpolation
 * + FFT evaluation of the trig sums (astropy fast_impl.py / utils.py trig_sum, extirpolate), regular grid only.
 * Agrees with the reference's 'fast' output to ~1e-10 (and, like it, is ~1e-3 of the peak from the exact methods).
 * oversampling: FFT grid oversampling (astropy default 5; Nfft = bitceil(M * oversampling)). */
int lk_ls_fast_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                     double f0, double df, int64_t M, int fit_mean, int center_data, int normalization,
                     const double *scale, int oversampling, double *power);
int lk_ls_fast_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                         const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                         int normalization, const double *scale, int oversampling, double *power, void *stream);

/* The same method followed by Periodogram.max_power / frequency_at_max_power (periodogram.py:127-140): per target
 * nanmax and nanargmax of the power row (first maximum wins; all-NaN row -> (nan, -1)).
 *
 * lk_ls_fast_peaks_batch (HOST pointers) is software-pipelined over chunks of targets: the H2D copy of chunk k+1,
 * the kernels of chunk k and the D2H copy of chunk k-1 run on three streams over double-buffered device memory.
 * Caller buffers that are pinned (lk_host_alloc, hipHostMalloc, hipHostRegister) are DMA'd directly; pageable
 * buffers go through the HIP runtime's staging.  power may be NULL (peaks only — the B x M spectra never cross PCIe);
 * max_power / argmax may both be NULL (spectra only: this is what lk_ls_fast_batch does).
 * lk_ls_fast_peaks_batch_dev: device pointers, power required, max_power / argmax nullable together. */
int lk_ls_fast_peaks_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                           const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                           int normalization, const double *scale, int oversampling, double *power,
                           double *max_power, int64_t *argmax);
int lk_ls_fast_peaks_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                               const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                               int normalization, const double *scale, int oversampling, double *power,
                               double *max_power, int64_t *argmax, void *stream);

/* The batch form of the loop `for lc in collection: lc.to_periodogram(frequency=...)` (reference collections.py:145 over
 * lightcurve.py:2490-2535 -> periodogram.py:869-967): `time` holds the ABSOLUTE times of the packed light curves; each
 * chunk is rebased on the device to t - t[first cadence of its light curve] (astropy lombscargle/core.py:119-126 does the
 * same subtraction per object) before the kernels of lk_ls_fast_peaks_batch run on it.  Everything else as above. */
int lk_ls_fast_peaks_lc_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux,
                              const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                              int normalization, const double *scale, int oversampling, double *power,
                              double *max_power, int64_t *argmax);

/* Pinned (page-locked) host memory for the host-pointer entry points: numpy arrays built over it are copied by DMA
 * without a staging pass.  Any host pointer is accepted everywhere; pinned ones are simply faster. */
int lk_host_alloc(void **ptr, size_t bytes);
int lk_host_free(void *ptr);

/* ---- device-resident batches ("FITS -> ragged device arrays ... on device") ----------------------
 * The reference chains its steps per object — lk.read(...) -> lc.remove_nans().normalize() -> lc.flatten() ->
 * lc.to_periodogram() -> lc.fold() (src/lightkurve/collections.py:145 over lightcurve.py:1300-1327, 1216-1292, 943-1078,
 * 2490-2535, 1089-1214); the batch form keeps the packed arrays in HBM between the `_dev` entry points.  For callers that do
 * not hold a HIP runtime of their own (ctypes, cgo, JNI): device memory, streams and copies by plain pointers.  Copies are
 * hipMemcpyAsync on `stream` (page-locked host buffers from lk_host_alloc make them truly asynchronous; pageable ones block
 * the host inside the call); lk_stream_synchronize (or lk_synchronize) before the host touches a d2h destination.
 * lk_dev_free synchronises the device (hipFree): recycle buffers in a pipeline (lightkurve_amd/device.py does). */
int lk_dev_alloc(lk_handle *h, void **ptr, size_t bytes);
int lk_dev_free(lk_handle *h, void *ptr);
int lk_stream_create(lk_handle *h, void **stream);
int lk_stream_destroy(lk_handle *h, void *stream);
int lk_stream_synchronize(lk_handle *h, void *stream);
int lk_memcpy_h2d(lk_handle *h, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int lk_memcpy_d2h(lk_handle *h, void *dst_host, const void *src_dev, size_t bytes, void *stream);
int lk_memcpy_d2d(lk_handle *h, void *dst_dev, const void *src_dev, size_t bytes, void *stream);
/* LightCurve.flatten's last lines (lightcurve.py:1064-1070): flux_out = flux / trend, flux_err_out = flux_err / trend over
 * the n packed cadences (flux_err nullable -> NaN errors; flux_err_out nullable; in-place allowed). */
int lk_flatten_apply_batch_dev(lk_handle *h, int64_t n, const double *flux, const double *flux_err, const double *trend,
                               double *flux_out, double *flux_err_out, void *stream);
/* lk_ls_fast_peaks_lc_batch with DEVICE pointers: `time` holds the light curves' own (absolute) times; they are rebased to
 * t - t[first cadence of the light curve] (astropy lombscargle/core.py:119-126) into scratch of the handle, `time` itself is
 * not modified.  power required; max_power / argmax nullable together. */
int lk_ls_fast_peaks_lc_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                                  const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                                  int normalization, const double *scale, int oversampling, double *power,
                                  double *max_power, int64_t *argmax, void *stream);
/* t_out = time - time[first cadence of its light curve] (out of place): what astropy's LombScargle hands every method,
 * for the exact entry points (lk_ls_power_batch_dev / lk_ls_chi2_batch_dev) of a device-resident batch. */
int lk_rebase_times_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, double *t_out,
                              void *stream);
/* Per light curve: descents_host[b] = number of cadences whose time is smaller than the previous one's (flatten, bin and
 * the bit-exact BLS need 0), finite_host[b] = number of finite values of x (LightCurve.bin's "has a finite error" test,
 * lightcurve.py:1712-1716).  time / descents_host and x / finite_host are nullable in pairs.  Synchronises `stream`. */
int lk_segment_probe_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *x,
                               int64_t *descents_host, int64_t *finite_host, void *stream);
/* What BoxLeastSquaresPeriodogram.from_lightcurve + astropy BoxLeastSquares hand to bls_fast (periodogram.py:1093-1100,
 * 1146-1169; astropy bls/core.py:277-327), per light curve of a packed batch WITHOUT NaN flux: t_out = (t - t[0]) -
 * min(t - t[0]); y_out = flux - numpy.median(flux); ivar_out = 1 / flux_err^2 if every error of the light curve is finite,
 * else ones (flux_err NULL: ones); t_ref_out[b] (device, nullable) = min(t - t[0]) + t[0], the zero of transit_time. */
int lk_bls_prepare_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                             const double *flux_err, double *t_out, double *y_out, double *ivar_out, double *t_ref_out,
                             void *stream);
/* Further per-cadence columns (quality flags, centroids, ...) through lk_ingest_batch's compaction: cols_out[c][new_off[b] +
 * k] = cols_in[c][...] for the k-th cadence of light curve b whose flux is not NaN.  ncols <= 8 device pointers in two
 * HOST arrays; elem_bytes 4 or 8; n_off / new_off: the offsets lk_ingest_batch_dev was given and returned. */
int lk_compact_columns_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int64_t *new_off_host,
                                 const double *flux, int ncols, int elem_bytes, const void *const *cols_in,
                                 void *const *cols_out, void *stream);
/* dst_host[i] = src_dev[idx_host[i]], i < n (the first / last time of every light curve for lightkurve's psd scale,
 * periodogram.py:865-868).  Synchronises `stream`. */
int lk_gather_f64_dev(lk_handle *h, int n, const int64_t *idx_host, const double *src_dev, double *dst_host, void *stream);
/* The shader clock [MHz] sustained over `spin_ms` milliseconds, measured ON the device (shader-cycle counter against the
 * constant-rate counter) by one wave on a stream of its own — i.e. under whatever load the caller has queued.  What
 * bench.py prints beside its roofline fractions: box-to-box spread of a bandwidth fraction is mostly this number. */
int lk_shader_clock_mhz(lk_handle *h, double spin_ms, double *mhz);

/* ---- batch ingest: the steps before the hot path, for B ragged light curves -------------------
 * lk_ingest_batch: LightCurve.remove_nans (src/lightkurve/lightcurve.py:1300-1327) + LightCurve.normalize (:1216-1292).
 * Cadences whose flux is NaN are dropped (order kept), the batch is repacked contiguously: new_off (B + 1, HOST, written
 * before the call returns: the call synchronises) addresses t_out / flux_out / flux_err_out (capacity: the input sizes);
 * median_out[b] = nanmedian(flux_b) (nullable); normalize != 0 divides flux and flux_err by it.  flux_err / flux_err_out
 * nullable (NaN errors are written when flux_err is NULL and flux_err_out is not). */
int lk_ingest_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                    int normalize, double *t_out, double *flux_out, double *flux_err_out, int64_t *new_off,
                    double *median_out);
int lk_ingest_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                        const double *flux_err, int normalize, double *t_out, double *flux_out, double *flux_err_out,
                        int64_t *new_off_host, double *median_out, void *stream);
/* LightCurve.remove_outliers (:1430-1556): astropy.stats.sigma_clip(y, sigma, maxiters, cenfunc=median, stdfunc=std).mask
 * for B ragged arrays: outlier[i] = 1 where the value is clipped or not finite. */
int lk_sigma_clip_batch(lk_handle *h, int B, const int64_t *n_off, const double *y, double sigma, int maxiters,
                        uint8_t *outlier);
int lk_sigma_clip_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma, int maxiters,
                            uint8_t *outlier, void *stream);
/* LightCurve.remove_outliers(sigma_lower=, sigma_upper=) (:1430-1556): astropy.stats.sigma_clip(y, sigma_lower=, sigma_upper=,
 * maxiters=, cenfunc=median, stdfunc=std).mask (astropy@4.3.1 stats/sigma_clipping.py:_sigmaclip_noaxis) per ragged row.  From
 * the finite values, each round keeps cen - std * sigma_lower <= x <= cen + std * sigma_upper (cen = median, std =
 * sqrt(mean((x - mean)^2)) of what is kept; equality keeps) until a round removes nothing or maxiters rounds have run
 * (maxiters < 0: no cap, astropy's maxiters=None).  outlier[i] = 1 where the value is not finite or outside the last bounds.
 * Empty rows and rows without a finite value are fine (every cadence of the latter is flagged). */
int lk_outlier_mask_batch(lk_handle *h, int B, const int64_t *n_off, const double *y, double sigma_lower, double sigma_upper,
                          int maxiters, uint8_t *outlier);
int lk_outlier_mask_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma_lower,
                              double sigma_upper, int maxiters, uint8_t *outlier, void *stream);
/* lc[mask] / lc[~mask] (boolean-array indexing of a LightCurve, as in the tutorial's second-planet search
 * lc[~bls.get_transit_mask(...)]) for the columns of a resident batch: cadence i is kept where (mask[i] != 0) != invert, order
 * preserved, cols_out[c][new_off[b] + k] = the k-th kept element of light curve b in cols_in[c].  ncols <= 8 device pointers
 * in two HOST arrays, elem_bytes[c] (HOST) 4 or 8; every cols_out[c] holds as many elements as cols_in[c] and overlaps no
 * input, no other output and not the mask (LK_EINVAL).  new_off_host (B + 1, HOST) is written before the call returns: the
 * call synchronises `stream`, as lk_ingest_batch_dev does. */
int lk_select_columns_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const uint8_t *mask, int invert, int ncols,
                                const int *elem_bytes, const void *const *cols_in, void *const *cols_out,
                                int64_t *new_off_host, void *stream);
/* The tail of LightCurve.estimate_cdpp (:1764-1833) per ragged row of an already flattened flux, on the cadences with
 * outlier[i] == 0 (outlier NULL: all of them) in their original order: ppm = kept / median(kept) * 1e6 (normalize("ppm"),
 * :1216-1292); the n_kept - w + 1 running means of w = min(transit_duration, n_kept) consecutive values (running_mean,
 * utils.py:374-386, as differences of a prefix sum); cdpp_out[b] = their population standard deviation (np.std, two passes).
 * n_kept == 0 gives NaN; transit_duration < 1 is LK_EINVAL.  The order of every sum follows from the row's own values alone:
 * a row's result has the same bits for any B, any position in the batch and any run.  cdpp_out: B doubles. */
int lk_cdpp_batch(lk_handle *h, int B, const int64_t *n_off, const double *flat_flux, const uint8_t *outlier,
                  int transit_duration, double *cdpp_out);
int lk_cdpp_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *flat_flux, const uint8_t *outlier,
                      int transit_duration, double *cdpp_out, void *stream);
/* ---- fill_gaps and stitch ------------------------------------------------------------------------------------------
 * LightCurve.fill_gaps(method="gaussian_noise") of lightkurve 2.x (lightcurve.py) for B ragged light curves whose NaN-flux
 * cadences are already removed, in two calls.  cadenceno == NULL is the reference's time path, cadenceno != NULL its cadence
 * path; built with -ffp-contract=off, every product and sum below rounds on its own.
 *
 * lk_fill_gaps_plan_batch: per light curve m = np.median(np.diff(time)) (exact; even count: mean of the two middle values),
 * mu = np.nanmean(flux), sd = np.nanstd(flux) and the number of inserted cadences -> stats[4 b + 0..3] (n_inserted as a double);
 * pos[n_off[b] + i] = index of original cadence i inside the filled light curve; new_off (B + 1, HOST) = offsets of the filled
 * batch, written before the call returns: the call synchronises `stream`, as lk_select_columns_batch_dev does.  A light curve
 * with fewer than 2 cadences comes back unchanged (m = NaN).
 *   time path   times must be non-decreasing.  prev = t[0]; for every next original t: while (t - prev) > 1.2 * m: insert
 *               prev + m, prev = that; then take t.  The inserted times are that chain of additions (one lane per gap).
 *   cadence path  cadence numbers must be strictly increasing; the filled light curve holds every c of [c_first, c_last],
 *               pos = c - c_first.
 * LK_EINVAL names the first light curve whose order is wrong, or whose median step is not positive / so small against a gap
 * that one gap would take more than 2^20 or the light curve 2^30 cadences (the reference does not return there).
 *
 * lk_fill_gaps_batch: the filled columns.  Originals keep flux, flux_err, quality, cadenceno; their time is t on the time path
 * and d + m * cf with cf = (double)c, d = t - m * cf on the cadence path (the reference recomputes them).  A cadence inserted
 * between originals j and j + 1:
 *   time      time path: its link of the chain.  Cadence path: slope = (d[j+1] - d[j]) / (cf[j+1] - cf[j]),
 *             nd = slope * (cf - cf[j]) + d[j], time = nd + m * cf  (np.interp's expression, plus m * cf)
 *   flux_err  slope = (e[j+1] - e[j]) / (t[j+1] - t[j]), slope * (time - t[j]) + e[j] with t the ORIGINAL times (np.interp)
 *   quality   65536;  cadenceno  c[j] + its place in the gap
 *   flux      noise_mean[b] + noise_std[b] * g.  g: the generator of lk_overfit_metric_batch, Philox4x32-10 with key (seed &
 *             0xffffffff, seed >> 32) and counter (i, 0, first_target + b, stream_id), i = the pair index over the inserted
 *             cadences of THAT light curve: inserted cadence 2 i takes the cosine normal, 2 i + 1 the sine normal.  (The
 *             reference draws from numpy's global generator: inserted fluxes match it in distribution only.)
 *   inserted  1 (0 for originals): out[~inserted] are the originals.
 * flux_err, quality (nullable) go with their outputs; the cadence-path outputs include cadenceno_out (the full range), the
 * time path takes cadenceno == cadenceno_out == NULL.  stats, pos, new_off: the plan's for the same batch and path (indices are
 * checked against the new lengths; a foreign plan leaves cadences unwritten).  noise_mean / noise_std: B doubles.  No
 * floating-point atomics; the order of every sum follows from the light curve's own length: a light curve's output has the
 * same bits for any B, any neighbours and any run.  Outputs hold new_off[B] elements. */
int lk_fill_gaps_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const int32_t *cadenceno,
                            double *stats, int32_t *pos, int64_t *new_off);
int lk_fill_gaps_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                                const int32_t *cadenceno, double *stats, int32_t *pos, int64_t *new_off_host, void *stream);
int lk_fill_gaps_batch(lk_handle *h, int B, const int64_t *n_off, const int64_t *new_off, const double *time, const double *flux,
                       const double *flux_err, const int32_t *quality, const int32_t *cadenceno, const double *stats,
                       const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed, int64_t first_target,
                       int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out, int32_t *quality_out,
                       int32_t *cadenceno_out, uint8_t *inserted);
int lk_fill_gaps_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int64_t *new_off_host, const double *time,
                           const double *flux, const double *flux_err, const int32_t *quality, const int32_t *cadenceno,
                           const double *stats, const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed,
                           int64_t first_target, int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out,
                           int32_t *quality_out, int32_t *cadenceno_out, uint8_t *inserted, void *stream);
/* LightCurveCollection.stitch's vstack for a resident batch: segment s, dst_off[s + 1] - dst_off[s] elements long, of every
 * column goes from cols_in[c][src_start[s] ..] to cols_out[c][dst_off[s] ..] in ONE launch.  src_start (S), dst_off (S + 1,
 * prefix offsets from 0) are HOST tables; n_src = elements per input column (every segment is checked against it); ncols <= 8
 * device pointers in two HOST arrays, elem_bytes[c] (HOST) 4 or 8; out of place. */
int lk_gather_segments_batch_dev(lk_handle *h, int S, const int64_t *src_start_host, const int64_t *dst_off_host, int64_t n_src,
                                 int ncols, const int *elem_bytes, const void *const *cols_in, void *const *cols_out, void *stream);
/* lk_fits_unpack_batch: what the reference's light-curve readers do per file through astropy — Table.read of the BINTABLE
 * (src/lightkurve/io/generic.py:21-207), drop the rows whose TIME is NaN (:98-101), drop the cadences whose quality flag
 * hits the bitmask (io/kepler.py:49-53, io/tess.py:45-48, utils.py:79-115) — for B files at once.  `raw`: the tables' bytes
 * exactly as in the files (big-endian records), file b at [raw_off[b], raw_off[b+1]) with raw_off[b] a multiple of 4 and
 * at least 3 spare bytes after its rows x record-length bytes.  desc: B x 10 int32 = {record length (<= 512), rows, byte
 * offset and TFORM code of TIME, of the flux column, of the flux-error column (offset -1: none -> NaN), of the quality
 * column (offset -1: none -> 0)}; codes 0 = D (float64), 1 = E (float32), 2 = J (int32), 3 = K (int64), 4 = I (int16),
 * 5 = B (uint8).  bitmask: B x int64.  Outputs (capacity: sum of rows): float64 time / flux / flux_err (nullable),
 * int32 quality (nullable), packed in file order; new_off (B + 1, HOST, valid when the call returns: it synchronises).
 * Header parsing stays on the host (lightkurve_amd/fitsio.py). */
int lk_fits_unpack_batch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off, const int32_t *desc,
                         const int64_t *bitmask, double *t_out, double *flux_out, double *flux_err_out,
                         int32_t *quality_out, int64_t *new_off);
int lk_fits_unpack_batch_dev(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                             const int64_t *bitmask_host, double *t_out, double *flux_out, double *flux_err_out,
                             int32_t *quality_out, int64_t *new_off_host, void *stream);
/* The CADENCENO column of the same tables for the rows lk_fits_unpack_batch kept (what CotrendingBasisVectors.align matches):
 * raw / raw_off / desc / bitmask as above (the keep rule is evaluated again from the same bytes; the flux columns of desc
 * are not read), col: B x 2 int32 = {byte offset, TFORM code 2..5} of the integer column, new_off: the B + 1 offsets the
 * unpack call returned (HOST), cadenceno_out: int32, new_off[B] entries, packed like the other columns.  No padding after a
 * table is needed.  The _dev call does not synchronise. */
int lk_fits_cadenceno_batch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off, const int32_t *desc,
                            const int32_t *col, const int64_t *bitmask, const int64_t *new_off, int32_t *cadenceno_out);
int lk_fits_cadenceno_batch_dev(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                                const int32_t *col_host, const int64_t *bitmask_host, const int64_t *new_off_host,
                                int32_t *cadenceno_out, void *stream);

/* lk_fits_unpack_cube: one target-pixel file -> what PLDCorrector reads from a TargetPixelFile: time, quality and the
 * float32 pixel cubes FLUX / FLUX_ERR / FLUX_BKG / ... of the cadences the reference keeps
 * (src/lightkurve/targetpixelfile.py:332, 372, 380, 386, 398: hdu[1].data[col][quality_mask]; quality_mask =
 * (QUALITY & bitmask) == 0, :2120-2122 for Kepler / K2; TESS additionally drops non-finite times when a bitmask is set,
 * :2794-2801 — pass keep_nan_time = 1 for Kepler files and for bitmask 0; a kept cadence without a finite TIME is
 * returned as 0.0 like TargetPixelFile.time does, :333-335).  raw: the BINTABLE's bytes as in the file;
 * ncols <= 4 pixel columns of npix big-endian float32 each at byte offsets col_off[]; cubes_out: ncols x n_rows x npix
 * float32 (column c starts at c * n_rows * npix, its first *kept cadences are valid); kept: HOST scalar. */
int lk_fits_unpack_cube(lk_handle *h, const uint8_t *raw, int row_bytes, int n_rows, int off_time, int code_time,
                        int off_quality, int code_quality, int64_t bitmask, int keep_nan_time, int ncols,
                        const int32_t *col_off, int npix, double *t_out, int32_t *quality_out, float *cubes_out,
                        int64_t *kept);
int lk_fits_unpack_cube_dev(lk_handle *h, const uint8_t *raw, int row_bytes, int n_rows, int off_time, int code_time,
                            int off_quality, int code_quality, int64_t bitmask, int keep_nan_time, int ncols,
                            const int32_t *col_off_host, int npix, double *t_out, int32_t *quality_out, float *cubes_out,
                            int64_t *kept_host, void *stream);

/* LightCurve.create_transit_mask (:2967-3037): target b has planets [planet_off[b], planet_off[b+1]) of the HOST arrays
 * period / duration / transit_time [d]; mask[i] = 1 where |((t - t0 + P/2) % P) - P/2| < duration/2 for any of them. */
int lk_transit_mask_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const int32_t *planet_off,
                          const double *period, const double *duration, const double *transit_time, uint8_t *mask);
int lk_transit_mask_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int32_t *planet_off,
                              const double *period, const double *duration, const double *transit_time, uint8_t *mask,
                              void *stream);
/* BoxLeastSquaresPeriodogram.compute_stats / get_transit_model (periodogram.py:1194-1269 over astropy
 * BoxLeastSquares.compute_stats / .model, bls/core.py:332-570) of ONE box per target: period / duration / transit_time
 * (absolute, like `time`) are HOST arrays of length B, positive and finite with duration < period.  time / flux / ivar: the
 * packed batch WITHOUT NaN flux, times sorted per light curve (unsorted input stays in bounds, its per-transit results are
 * unspecified); ivar NULL = ones.  stats[b][LK_BLS_NSTATS], in order:
 *    0 depth             1 its error        2 depth_phased       3 its error        4 depth_half      5 its error
 *    6 depth_odd         7 its error        8 depth_even         9 its error       10 harmonic_amplitude
 *   11 harmonic_delta_log_likelihood       12 y_in (model level inside)            13 y_out (outside)
 *   14 number of in-transit cadences       15 reserved, 0
 * A depth whose mask is empty (or whose out-of-transit variance is not finite) is (0, inf) as in the reference; columns 10
 * and 11 are NaN for a light curve of fewer than three cadences or a singular harmonic fit.
 * Per transit: target b owns entries [tr_off[b], tr_off[b+1]) of tr_count / tr_ll; floor((t_last - t_first) / period) + 3
 * entries always suffice.  tr_first[b] = the smallest transit id round((t - transit_time) / period) of an in-transit cadence
 * (may be negative), tr_n[b] = the number of ids up to the largest; entry k of the slot = cadence count and log-likelihood
 * gain of transit tr_first[b] + k (0 / 0.0 for a transit inside a data gap), the unused tail zeroed.  tr_n[b] = 0: no
 * cadence in transit; tr_n[b] = -1: the ids do not fit the slot (the slot is zeroed, nothing beyond it is written).
 * model: NULL, or [n] = y_in inside the transits and y_out outside.  Every sum's order depends on the target's own data
 * alone: a target's outputs do not change with B or with its neighbours in the batch. */
#define LK_BLS_NSTATS 16
int lk_bls_stats_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *ivar,
                       const double *period, const double *duration, const double *transit_time, const int64_t *tr_off,
                       double *stats, int32_t *tr_first, int32_t *tr_n, int32_t *tr_count, double *tr_ll, double *model);
int lk_bls_stats_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                           const double *ivar, const double *period, const double *duration, const double *transit_time,
                           const int64_t *tr_off_host, double *stats, int32_t *tr_first, int32_t *tr_n, int32_t *tr_count,
                           double *tr_ll, double *model, void *stream);
/* LombScarglePeriodogram.model (periodogram.py:991-1018 over astropy LombScargle.model -> mle.periodic_fit,
 * implementations/mle.py:58-114) at ONE frequency per target: frequency is a HOST array of length B [1/d].  time / flux /
 * dy: the packed batch WITHOUT NaN flux; the fit runs on t = time - time[first stored cadence of the target].  dy NULL = unit
 * weights; a target whose dy are not all finite gets unit weights too (the rule of the other stages), else w = dy^-2.
 * y_mean = sum w y / sum w (center_data) or 0; design columns [1 if fit_mean], sin(2 pi m f t), cos(2 pi m f t) for
 * m = 1 .. nterms (nterms 1 .. 8, anything else is LK_EINVAL); theta solves the weighted normal equations of y - y_mean by
 * LU with partial pivoting; model = y_mean + X theta.
 * theta[b][2 * nterms + 1]: slot 0 = the bias (0 when !fit_mean), then sin 1, cos 1, sin 2, cos 2, ...
 * stats[b][LK_LS_MODEL_NSTATS], in order:
 *    0 y_mean        1 chi2_ref = sum w (y - y_mean)^2        2 chi2_model = sum w (y - model)^2        3 status
 * status  1: fitted.   0: the frequency is NaN or <= 0, the target is skipped.   -1: fewer than 2 * nterms + fit_mean
 * cadences (an empty light curve included; nothing of it is read), or a pivot / coefficient that is zero or not finite
 * (astropy raises).  Where the status is not 1, theta and stats 0 .. 2 are NaN.
 * model: NULL, or [n] = the model (NaN where the status is not 1).  residual: NULL, or [n] = flux minus the periodic part
 * alone (keep_mean: the level y_mean + bias stays in the light curve) or flux - model (!keep_mean); where the status is not
 * 1 it is the flux, bit for bit.  Every sum's order depends on the target's own data alone: a target's outputs do not
 * change with B or with its neighbours in the batch.
 * lk_ls_model_eval_batch: the fitted series at other times.  Target b owns entries [m_off[b], m_off[b+1]) of t_fit / out;
 * out = y_mean + bias + series(t_fit - t_ref[b]) with t_ref (HOST, the target's first stored time) and frequency (HOST) as
 * given to the fit, theta / stats as the fit wrote them; NaN where the status is not 1. */
#define LK_LS_MODEL_NSTATS 4
int lk_ls_model_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *dy,
                      const double *frequency, int nterms, int fit_mean, int center_data, int keep_mean, double *theta,
                      double *stats, double *model, double *residual);
int lk_ls_model_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                          const double *dy, const double *frequency, int nterms, int fit_mean, int center_data, int keep_mean,
                          double *theta, double *stats, double *model, double *residual, void *stream);
int lk_ls_model_eval_batch(lk_handle *h, int B, const int64_t *m_off, const double *t_fit, const double *t_ref,
                           const double *frequency, int nterms, const double *theta, const double *stats, double *out);
int lk_ls_model_eval_batch_dev(lk_handle *h, int B, const int64_t *m_off_host, const double *t_fit, const double *t_ref,
                               const double *frequency, int nterms, const double *theta, const double *stats, double *out,
                               void *stream);
/* LightCurve.bin (:1558-1763) over astropy aggregate_downsample (astropy@4.3.1 timeseries/downsample.py:12-125), times
 * sorted.  Target b gets bins [bin_off[b], bin_off[b+1]) of the outputs; its bins start at time_bin_start[b] [d] and their
 * edges, in seconds relative to it, are edges_sec[0 .. n_bins_b] (HOST; numpy's cumsum of the bin size, shared by all
 * targets, n_edges entries).  A cadence at relative time r belongs to bin k when edges[k] < r <= edges[k+1] (r == 0: bin 0)
 * and r < edges[n_bins_b].  flux_out = nanmean; flux_err_out = sqrt(nansum(err^2) / #finite) where has_err[b] (the light
 * curve has at least one finite error), else nanstd of the flux in the bin; empty bins are NaN;
 * t_out = time_bin_start + (edges[k] + bin_size_sec / 2) / 86400. */
int lk_bin_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                 const int64_t *bin_off, const double *time_bin_start, const double *edges_sec, int64_t n_edges,
                 double bin_size_sec, const uint8_t *has_err, double *t_out, double *flux_out, double *flux_err_out);
int lk_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                     const double *flux_err, const int64_t *bin_off, const double *time_bin_start, const double *edges_sec,
                     int64_t n_edges, double bin_size_sec, const uint8_t *has_err, double *t_out, double *flux_out,
                     double *flux_err_out, void *stream);

/* ---- lc.fold(period, epoch_time).bin(...) (and FoldedLightCurve.cycle / odd_mask / even_mask, lightcurve.py:3213-3250) for
 * B ragged targets: LightCurve.bin's semantics above applied to the PHASE column, with the edges formed per target.
 *
 * Layout of the bins, shared by lk_phase_bin_batch_dev and lk_fold_bin_batch*: target b owns bins [bin_off[b], bin_off[b+1])
 * of the outputs; its bins start at phase start[b] and are size_sec[b] seconds wide; its n_bins_b + 1 edges, in seconds
 * relative to start[b] (numpy's cumsum of the bin size, beginning with 0 and strictly increasing), are
 * edges[bin_off[b] + b ...] (so edges holds bin_off[B] + B values).  All of these are HOST arrays.
 *
 * lk_fold_bin_plan_batch*: what the caller needs to form that layout, from ONE pass over the cadences and no sort.  period /
 * epoch_time / wrap_phase as in lk_fold_batch; plan (HOST, valid on return: the _dev form synchronises `stream`) receives
 * LK_FOLD_BIN_NPLAN doubles per target: [0] smallest phase (+inf: none), [1] largest phase, [2] number of phases >=
 * count_from[b] (count_from NULL: all that are not NaN), [3] 1 when a flux_err is finite (flux_err nullable), [4] the smallest
 * cycle, floor((t - (e - P/2)) / P) with e = epoch_time[b] when epoch_given and the smallest phase otherwise, [5] the largest
 * finite |flux|, [6] the largest finite |flux_err|, [7] largest minus smallest finite flux. */
#define LK_FOLD_BIN_NPLAN 8
int lk_fold_bin_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                           const double *period, const double *epoch_time, int epoch_given, double epoch_phase,
                           const double *wrap_phase, int normalize_phase, const double *count_from, double *plan);
int lk_fold_bin_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                               const double *flux_err, const double *period, const double *epoch_time, int epoch_given,
                               double epoch_phase, const double *wrap_phase, int normalize_phase, const double *count_from,
                               double *plan, void *stream);
/* cycle[i] = floor((t[order[i]] - (cycle_epoch[b] - P/2)) / P) - cycle_min[b] for every slot of a folded batch (t: the unfolded
 * times, order: lk_fold_batch's), odd[i] = cycle % 2 == 1, even[i] = cycle % 2 == 0 (bytes, the layout lk_select_batch_dev
 * takes); each of the three outputs may be NULL.  cycle_epoch / cycle_min (HOST): plan[0] (or epoch_time) and plan[4]. */
int lk_fold_cycle_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int64_t *order,
                            const double *period, const double *cycle_epoch, const double *cycle_min, int64_t *cycle, uint8_t *odd,
                            uint8_t *even, void *stream);
/* Bins of a folded batch (phase sorted; flux / flux_err in phase order).  sel (nullable): only the slots with sel[i] ==
 * sel_value take part.  phase_out = start + (edges[k] + size_sec / 2) / 86400, flux_out = nanmean (median != 0: np.nanmedian),
 * flux_err_out = sqrt(nansum(err^2) / #finite) where has_err[b], else nanstd of the flux in the bin (for both aggregates),
 * count_out = slots of the bin that take part; a bin with none holds NaN. */
int lk_phase_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *phase, const double *flux,
                           const double *flux_err, const uint8_t *sel, int sel_value, const int64_t *bin_off, const double *start,
                           const double *size_sec, const double *edges, const uint8_t *has_err, int median, double *phase_out,
                           double *flux_out, double *flux_err_out, int32_t *count_out, void *stream);
/* The fused form on the UNFOLDED batch: no sort, no n-sized intermediate, one workgroup per target (foldbin.hip).  plan: what
 * lk_fold_bin_plan_batch* wrote for the same arguments; cycle_epoch: as in lk_fold_cycle_batch_dev; which: 0 all cadences, 1 /
 * 2 only those of odd / even cycles.  Outputs as lk_phase_bin_batch_dev's with median == 0: the same layout, counts and NaN
 * pattern, values within rounding (sums of addends rounded to 2^-63 n max|x|, accumulated as integers: bitwise reproducible and
 * independent of B).  Up to LK_FOLD_BIN_LDS_BINS bins per target are accumulated in LDS, more in a slab of device scratch. */
#define LK_FOLD_BIN_LDS_BINS 1024
int lk_fold_bin_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                      const double *period, const double *epoch_time, double epoch_phase, const double *wrap_phase,
                      int normalize_phase, const double *cycle_epoch, const double *plan, int which, const int64_t *bin_off,
                      const double *start, const double *size_sec, const double *edges, double *phase_out, double *flux_out,
                      double *flux_err_out, int32_t *count_out);
int lk_fold_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                          const double *flux_err, const double *period, const double *epoch_time, double epoch_phase,
                          const double *wrap_phase, int normalize_phase, const double *cycle_epoch, const double *plan, int which,
                          const int64_t *bin_off, const double *start, const double *size_sec, const double *edges,
                          double *phase_out, double *flux_out, double *flux_err_out, int32_t *count_out, void *stream);

/* ---- River diagrams: per target an image (cycles x phase bins) of the UNFOLDED batch, the data behind LightCurve.plot_river
 * (lightkurve 2.x lightcurve.py).  y = flux / nanmedian(flux), u = flux_err / nanmedian(flux); phase = lk_fold_batch's with
 * epoch_phase 0, wrap_phase 0.5, normalize_phase 1 (the same bits); row = floor((t - (e - P/2)) / P) minus its minimum over the
 * target; a cadence is in column j when edges[j] < phase <= edges[j+1] (a phase equal to edges[0] is in none) and takes part
 * when its y is finite.  river = mean of the cell's y (method 0), np.median of it (1) or (mean - 1) / sqrt(nansum(u^2)) (2,
 * needs flux_err); count = cadences that take part; a cell with none holds NaN / 0.  Times must be non-decreasing per target.
 *
 * lk_river_plan_batch*: ONE workgroup per target streams time and flux once; plan (HOST, valid on return: the _dev form
 * synchronises `stream`) receives LK_RIVER_NPLAN doubles per target: [0] nanmedian(flux), [1] nanmedian(diff(t)) (both exact
 * order statistics), [2] / [3] smallest / largest cycle before the minimum is taken off (0 / -1: no finite time), [4] number of
 * finite fluxes, [5] 1 when every time is finite and none decreases, [6] the first time (NaN: no cadence), [7] / [8] the largest
 * finite |flux| / |flux_err|.  period (> 0) / epoch_time: HOST, B each; with epoch_given == 0 the epoch is the target's first time.
 *
 * lk_river_batch*: target b owns cells [cell_off[b], cell_off[b+1]) of river (float64) and count (int32), row-major as
 * (n_cycles[b], n_bins[b]); its n_bins[b] + 1 edges (strictly increasing phases) are edges[sum of n_bins[a < b] + b ...]; a
 * target with n_bins[b] == 0 or n_cycles[b] == 0 owns no cell and is not read.  plan: what lk_river_plan_batch* wrote for the
 * same period and epoch (its median, smallest and largest cycle and maxima are used); epoch_time: the epoch of every target (its
 * first time where none was given).  All of these are HOST arrays.  Every cell is written.  The rows of a target are cut into tiles
 * of at most LK_RIVER_LDS_CELLS cells (a row wider than that into column chunks), one workgroup each; sums are exact integer sums
 * of the addends rounded to a per-target quantum (lk_fold_bin_batch's scheme), medians exact: a target's cells have the same bits
 * alone, at any place in a batch and from run to run.  Median: a tile's values are collected in LDS, or in device scratch when more
 * than LK_RIVER_LDS_VALS take part; a cell of up to LK_RIVER_CELL_THREAD values is ranked by one thread, a larger one by the
 * workgroup.  route (DEVICE, int32[B], nullable) receives per target the OR of its tiles' LK_RIVER_ROUTE_* bits. */
#define LK_RIVER_NPLAN 9
#define LK_RIVER_LDS_CELLS 3072
#define LK_RIVER_LDS_VALS 4096
#define LK_RIVER_CELL_THREAD 32
#define LK_RIVER_ROUTE_ROWS 1         /* a tile of whole rows */
#define LK_RIVER_ROUTE_COLUMNS 2      /* a column chunk of one row (n_bins > LK_RIVER_LDS_CELLS) */
#define LK_RIVER_ROUTE_VALS_LDS 4     /* median: the tile's values collected in LDS */
#define LK_RIVER_ROUTE_VALS_SCRATCH 8 /* median: ... in device scratch */
#define LK_RIVER_ROUTE_CELL_THREAD 16 /* median: a cell ranked by one thread */
#define LK_RIVER_ROUTE_CELL_GROUP 32  /* median: a cell ranked by the workgroup */
int lk_river_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                        const double *period, const double *epoch_time, int epoch_given, double *plan);
int lk_river_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                            const double *flux_err, const double *period, const double *epoch_time, int epoch_given, double *plan,
                            void *stream);
int lk_river_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                   const double *period, const double *epoch_time, const double *plan, int method, const int32_t *n_bins,
                   const int32_t *n_cycles, const int64_t *cell_off, const double *edges, double *river, int32_t *count,
                   int32_t *route);
int lk_river_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *flux_err,
                       const double *period, const double *epoch_time, const double *plan, int method, const int32_t *n_bins,
                       const int32_t *n_cycles, const int64_t *cell_off, const double *edges, double *river, int32_t *count,
                       int32_t *route, void *stream);

/* ---- nanmax / nanargmax over each row of a B x M float64 matrix (first maximum wins) ---------------- */
int lk_argmax_batch(lk_handle *h, int B, int64_t M, const double *x, double *max_out, int64_t *argmax_out);
int lk_argmax_batch_dev(lk_handle *h, int B, int64_t M, const double *x, double *max_out,
                        int64_t *argmax_out, void *stream);

/* ---- Box Least Squares (astropy run_bls semantics; bit-exact for time-sorted input) -------------------
 * t: t - min(t); y: y - median(y); ivar: 1/dy^2 (ones if no errors) — exactly what bls/core.py:304-327
 * hands to bls_fast.  period[nP], duration[nD] shared by all targets.  use_likelihood: 1 'likelihood', 0 'snr'.
 * out7: 7 x B x nP row-major: power, depth, depth_err, duration, transit_time(phase), depth_snr, log_likelihood. */
int lk_bls_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                 const double *ivar, const double *period, int64_t nP, const double *duration, int nD,
                 int oversample, int use_likelihood, double *out7);
int lk_bls_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                     const double *ivar, const double *period_host, const double *period_dev, int64_t nP,
                     const double *duration_host, int nD, int oversample, int use_likelihood, double *out7,
                     void *stream);

/* Host-only helper (no GPU): the longest period whose phase bins (period / (min duration / oversample) of them) the LDS
 * kernels hold for these durations and this oversample.  Longer periods are accepted all the same (astropy's bls_fast has no
 * limit): they run a global-memory kernel, bit-identical, ~100 x the cost per (target, period) — a multi-year baseline
 * searched with short durations. */
int lk_bls_max_period(const double *duration, int nD, int oversample, double *max_period);

/* ---- RegressionCorrector: Gaussian-prior weighted least squares, iterated with sigma clipping ----------
 * X: (sum N) x K row-major design matrix (same K for every target of the batch); y: flux; err: flux errors or
 * NULL (ones, regressioncorrector.py:157-158); cadence_mask: 1 = use the cadence, or NULL (all);
 * prior_mu / prior_sigma: B x K (sigma may be +inf) or both NULL; clip_sigma / niters as in .correct().
 * Outputs: w B x K coefficients of the last iteration; model = X w - median(X w) per target (sum N);
 * outlier: (sum N) bytes, 1 = clipped in some iteration (regressioncorrector.py:243-279). */
int lk_regress_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *X, const double *y,
                     const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                     const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                     uint8_t *outlier);
int lk_regress_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *X, const double *y,
                         const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                         const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                         uint8_t *outlier, void *stream);

/* The same fit with propagate_errors=True (regressioncorrector.py:183-185): w_cov (B x K x K, nullable) receives
 * inv(X^T S^-1 X + diag(1/prior_sigma^2)) of the LAST iteration's fit — RegressionCorrector.coefficients_err. */
int lk_regress_cov_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *X, const double *y,
                         const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                         const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                         uint8_t *outlier, double *w_cov);
int lk_regress_cov_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *X, const double *y,
                             const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                             const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                             uint8_t *outlier, double *w_cov, void *stream);

/* ---- The same regression for B targets that share ONE design matrix (cotrending: the CBVs of a channel, spacecraft-wide
 * regressors).  X: N x K row-major, once for the whole batch, 1 <= K <= 64 (the kernel forms the K (K + 1) / 2 column
 * products of X on the fly and keeps a target tile's whole normal matrix in accumulator registers; a wider matrix goes through
 * lk_regress_batch with one copy per target); y, err (nullable = ones), cadence_mask (nullable): B x N; prior_mu /
 * prior_sigma: B x K or both NULL; w B x K, model and outlier B x N, w_cov B x K x K or NULL, all as lk_regress_cov_batch
 * gives them.  B <= 65535, N >= 1.  No buffer of B N K elements exists anywhere in the call.  A non-finite flux or a
 * non-finite or non-positive error is an error (LK_EINVAL; RegressionCorrector.__init__ raises
 * for the same light curve): the _dev call waits for that one answer before it queues the fit, then returns without
 * further synchronisation.  Results are bitwise reproducible and do not depend on B (partial sums over cadence slices are
 * added in slice order, no atomics). */
int lk_regress_shared_batch(lk_handle *h, int B, int N, int K, const double *X, const double *y, const double *err,
                            const uint8_t *cadence_mask, const double *prior_mu, const double *prior_sigma,
                            double clip_sigma, int niters, double *w, double *model, uint8_t *outlier, double *w_cov);
int lk_regress_shared_batch_dev(lk_handle *h, int B, int N, int K, const double *X, const double *y, const double *err,
                                const uint8_t *cadence_mask, const double *prior_mu, const double *prior_sigma,
                                double clip_sigma, int niters, double *w, double *model, uint8_t *outlier, double *w_cov,
                                void *stream);
/* CBVCorrector.correct_gaussian_prior's prior for B resident targets of N cadences: prior_mu = 0 and prior_sigma[b][:] =
 * numpy.median(flux_err[b]) / sqrt(|alpha|) (B x K each), alpha != 0.  Device pointers; nothing comes back to the host. */
int lk_ridge_prior_batch_dev(lk_handle *h, int B, int N, int K, const double *flux_err, double alpha, double *prior_mu,
                             double *prior_sigma, void *stream);
/* The same with one penalty per target: alpha = B doubles ON THE DEVICE, each finite and non-zero (the caller checks: nothing
 * comes back), prior_sigma[b][:] = numpy.median(flux_err[b]) / sqrt(|alpha[b]|) by the same two operations: row b has the bits
 * lk_ridge_prior_batch_dev gives at alpha[b]. */
int lk_ridge_prior_alphas_batch_dev(lk_handle *h, int B, int N, int K, const double *flux_err, const double *alpha,
                                    double *prior_mu, double *prior_sigma, void *stream);
/* ---- The shared-matrix regression for a RAGGED batch: target b has n_off[b + 1] - n_off[b] >= 1 cadences and its cadence i
 * uses row rows[n_off[b] + i] of the ONE matrix X (Nx x K, K <= 64).  rows: int32 (sum n), per target strictly increasing and
 * in [0, Nx) (checked: LK_EINVAL names the first offending target); y, err (nullable), cadence_mask (nullable), model and
 * outlier: (sum n), packed by n_off; priors, w and w_cov as lk_regress_shared_batch.  Per target the numerics are
 * RegressionCorrector.correct on X[rows_b]: the clip's median / std and the model's median are over the target's own cadences.
 * Rows of X that a target does not have add +0 to its sums, so its result has the bits its own rows alone give and, when
 * every target has every row, the bits of lk_regress_shared_batch.  The results of a target do not depend on the other
 * targets of the batch; the order of its partial sums depends on Nx alone.  Scratch: B x Nx int32 more than the uniform call.
 * Synchronisation as lk_regress_shared_batch_dev (one wait, for the rows and the input check). */
int lk_regress_shared_rows_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *rows, int Nx, int K, const double *X,
                                 const double *y, const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                                 const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                                 uint8_t *outlier, double *w_cov);
int lk_regress_shared_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, int K,
                                     const double *X, const double *y, const double *err, const uint8_t *cadence_mask,
                                     const double *prior_mu, const double *prior_sigma, double clip_sigma, int niters, double *w,
                                     double *model, uint8_t *outlier, double *w_cov, void *stream);
/* CotrendingBasisVectors.align for B targets: cadenceno (int32, (sum n), per target strictly increasing) against the grid's
 * cadence numbers (int32, Nx, strictly increasing) -> rows (int32 (sum n): the index into the grid, binary search per
 * cadence) and pos (int32 B x Nx, nullable: the target-relative cadence index at a grid row, -1 where the target has none).
 * A cadence that is not on the grid is LK_EINVAL with the first such target's index in lk_last_error (rows is then still
 * written, -1 at such cadences): drop those cadences first.  The call synchronises. */
int lk_align_rows_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *cadenceno, int Nx, const int32_t *grid_cadenceno,
                        int32_t *rows, int32_t *pos);
int lk_align_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *cadenceno, int Nx,
                            const int32_t *grid_cadenceno, int32_t *rows, int32_t *pos, void *stream);
/* lk_ridge_prior_batch_dev / lk_ridge_prior_alphas_batch_dev for a ragged batch: the median is over target b's own
 * flux_err[n_off[b] .. n_off[b + 1]), by the same two operations (a uniform batch gets the same bits). */
int lk_ridge_prior_rows_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *flux_err, double alpha,
                              double *prior_mu, double *prior_sigma);
int lk_ridge_prior_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *flux_err, double alpha,
                                  double *prior_mu, double *prior_sigma, void *stream);
int lk_ridge_prior_rows_alphas_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *flux_err, const double *alpha,
                                     double *prior_mu, double *prior_sigma);
int lk_ridge_prior_rows_alphas_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *flux_err,
                                         const double *alpha, double *prior_mu, double *prior_sigma, void *stream);
/* ---- CotrendingBasisVectors.interpolate for a ragged batch: K columns Y (Nx x K row-major) given at the knot times knot_time
 * (Nx) are interpolated to the times t ((sum n), packed by n_off; a target may have no cadence) with
 * scipy.interpolate.PchipInterpolator's piecewise cubic, and written as the targets' design matrices X_out, (sum n) x Kout
 * row-major, Kout = K + (append_constant != 0): the layout lk_regress_batch takes; the optional last column is all ones.
 * knot_keep (Nx bytes, nullable = all): the reference's ~gap_indicators, knots with 0 are left out (compacted on the device).
 * The LK_EINVAL cases: kept knot times not finite or not strictly increasing, fewer than 2 kept knots, a kept Y that is not
 * finite, K < 1.  A time outside [first kept knot, last kept knot], or not finite, gives NaN in the K columns when
 * extrapolate == 0, and the first / last cubic continued, as scipy does, otherwise (NaN for a NaN time).  A time bit-equal
 * to a kept knot gives that knot's values bit for bit.  inside ((sum n) bytes, nullable): 1 = the time lies in the kept knots'
 * span.  X_out may be NULL when inside is not: only the bytes are written.  Every element depends on its own time alone: a
 * target's rows have the same bits whatever else is in the batch.  The call waits once, for the check of the knots, before
 * it queues the interpolation; the _dev form returns without further synchronisation.  Nx K < 2^31, B <= 65535. */
int lk_pchip_interp_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, int Nx, int K, const double *knot_time,
                          const double *Y, const uint8_t *knot_keep, int extrapolate, int append_constant, double *X_out,
                          uint8_t *inside);
int lk_pchip_interp_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, int Nx, int K,
                              const double *knot_time, const double *Y, const uint8_t *knot_keep, int extrapolate,
                              int append_constant, double *X_out, uint8_t *inside, void *stream);
/* out[i] = a[i] - b[i] for n doubles on the device (flux - model: the corrected flux of RegressionCorrector.correct). */
int lk_subtract_f64_dev(lk_handle *h, int64_t n, const double *a, const double *b, double *out, void *stream);

/* ---- Under-fitting goodness metric of B targets whose neighbours are OTHER TARGETS OF THE SAME BATCH, given by index
 * (reference src/lightkurve/correctors/metrics.py:141-257 underfit_metric_neighbors over _compute_correlation, :451-475; the
 * reference fetches the neighbours' light curves from MAST — here they are the other corrected targets of the field, already
 * in device memory).  flux: B x N, NaN-free; keep_idx: the n kept cadences shared by every target (ascending indices into
 * [0, N): the reference's lc[cadence_mask]), or NULL = all cadences (then n == N); neighbors: B x M int32, -1 = padding.
 * Per target t, with z_b[i] = flux_b[keep_idx[i]] / numpy.median(flux_b[keep_idx]) - 1.0 and G(a,b) = sum_i z_a[i] z_b[i]:
 *   corr[t][p]  = G(t,j) / sqrt(G(t,t) G(j,j)) for j = neighbors[t][p] (0 when either self-product is 0: the reference's
 *                 rms -> inf rule; NaN at padding), B x M or NULL;
 *   metric[t]   = 2 / (1 + exp(scale * sum_p |corr[t][p]|^3 / (m + 1))), m = the valid neighbours of t,
 *                 scale = ln(2 / 0.95 - 1) / (0.0007 + 0.8083 n^-0.5023); 1.0 when m == 0.
 * A median of exactly zero gives non-finite z and a non-finite result, as in the reference.  The order in which G(a,b) is
 * summed depends on n alone (not on B, M, the position in the list or the workgroup): G(t,j) and G(j,t) are the same bits, a
 * run on a sub-batch gives the same bits, and so do two runs; no atomics.  B >= 1, 2 <= n <= N, M >= 0 (LK_EINVAL otherwise);
 * the host flavour also checks keep_idx and every neighbour index (-1, or in [0, B) and not the target itself) — the _dev
 * flavour treats any index outside [0, B) as padding and checks nothing else.  Scratch: B x ceil(n / 128) x 128 + B doubles of
 * the handle's arena.  The _dev call synchronises nothing. */
int lk_underfit_neighbors_batch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                                const int32_t *neighbors, double *corr, double *metric);
int lk_underfit_neighbors_batch_dev(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                                    const int32_t *neighbors, double *corr, double *metric, void *stream);
/* The same metric with the neighbours taken from ANOTHER array of Bn rows (flux_nb: Bn x N, NaN-free, the same cadences), prepared
 * once and used by any number of calls (a ridge search scores many corrections of the targets against fixed neighbours).
 * lk_underfit_rows_prepare_dev writes the Bn median-normalised rows z_j (pitch ceil(n / 128) x 128 doubles, zero tail) and then
 * the Bn self-products G(j,j) into `rows`, a 16-byte aligned device block of the caller's of lk_underfit_rows_bytes(Bn, n) bytes.
 * lk_underfit_against_rows_batch_dev prepares only the B target rows (B x ceil(n / 128) x 128 + B doubles of the handle's arena)
 * and runs the pair pass against `rows`, which must have been prepared with the same n and keep_idx; neighbors: B x M int32
 * indices into [0, Bn), anything else = padding; an index equal to the target's own row number is a neighbour like any other
 * (it names a row of the other array).  G(a,b) is summed in the order given above: with flux_nb == flux the results are the bits
 * of lk_underfit_neighbors_batch_dev.  Neither call synchronises anything. */
int lk_underfit_rows_bytes(int Bn, int n, int64_t *bytes);
int lk_underfit_rows_prepare_dev(lk_handle *h, int Bn, int N, const double *flux_nb, int n, const int32_t *keep_idx, void *rows,
                                 int64_t rows_bytes, void *stream);
int lk_underfit_against_rows_batch_dev(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int Bn,
                                       const void *rows, int M, const int32_t *neighbors, double *corr, double *metric,
                                       void *stream);
/* The same metric for a RAGGED batch on a grid of Nx cadences.  Light curve b holds n_off[b + 1] - n_off[b] cadences (0 .. Nx),
 * its cadence i on grid row rows[n_off[b] + i]: int32 (sum n), per light curve strictly increasing indices into [0, Nx), what
 * lk_align_rows_batch returns.  flux: (sum n), NaN-free.  cadence_mask: (sum n) bytes, non-zero = used, or NULL = all.  A light
 * curve is PRESENT at a grid row when it has that cadence and its own mask entry there is set.  med_b = numpy.median of its flux
 * over its present cadences and z_b[r] = flux / med_b - 1.0 there.  Per target t, C_t = the grid rows where t and every valid
 * neighbour of t are present (the reference drops a cadence any column lacks), n_t = |C_t|, and with G_t(a,b) = the sum of
 * z_a[r] z_b[r] over r in C_t:
 *   corr[t][p]  = G_t(t,j) / sqrt(G_t(t,t) G_t(j,j)) for j = neighbors[t][p] (0 when either self-product is 0; NaN at padding),
 *                 B x M or NULL;
 *   n_common[t] = n_t, int32 B or NULL;
 *   metric[t]   = 2 / (1 + exp(scale(n_t) * sum_p |corr[t][p]|^3 / (m + 1))) with the scale above at n = n_t; 1.0 when m == 0.
 * n_t < 2 (with m > 0): metric[t] and every corr[t][p] are NaN; that is no error, since with a mask in device memory the count is
 * not known to the host.  G_t is summed in the order given above with i = the grid row (step r / 128, lane (r / 2) % 64, component
 * r % 2), the elements outside C_t replaced by 0.0: when every light curve has every grid row and cadence_mask is NULL, metric and
 * corr are the bits of lk_underfit_neighbors_batch_dev on the same flux; a target's result does not depend on B, on rows it does
 * not list, on a neighbour's position in its list or on the run; no atomics.  B >= 1, B <= 65535, 1 <= Nx <= 245760, M >= 0
 * (LK_EINVAL otherwise).  The host flavour checks rows and every neighbour index on the host (as lk_regress_shared_rows_batch and
 * lk_underfit_neighbors_batch do).  The _dev flavours treat any index outside [0, B) (or [0, Bn)) as padding; they check rows on
 * the device and wait on `stream` ONCE, for the 4 bytes of that check (LK_EINVAL names the first offending light curve), before
 * the prepare pass is queued; nothing else is waited for, and the results are ordered on `stream` like any kernel's.  n_off_host
 * is read before the call returns.  Scratch in the handle's arena: B x Nx int32 (the inverse map) + B x P doubles + B x P / 64
 * words + Nx + 1 doubles, P = ceil(Nx / 128) x 128.
 * lk_underfit_grid_rows_prepare_dev writes Bn light curves of ANOTHER ragged array (their own n_off_host / rows on the same grid;
 * cadence_mask usually NULL) into `block`, a 16-byte aligned device block of the caller's of lk_underfit_grid_rows_bytes(Bn, Nx)
 * bytes: the Bn z rows on the grid layout (P doubles each, 0.0 at absent rows), then their presence bitmasks (P / 64 64-bit words
 * each, bit r % 64 of word r / 64 = present at grid row r).  lk_underfit_grid_against_rows_batch_dev prepares only the B targets
 * and runs the pair pass against `block` (prepared with the same Nx); neighbors then index [0, Bn) and a target's own row number
 * is a neighbour like any other.  With the block prepared from the batch itself the results are the bits of
 * lk_underfit_grid_neighbors_batch_dev.  Both wait once for their own check of rows, as above. */
int lk_underfit_grid_neighbors_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *rows, int Nx, const double *flux,
                                     const uint8_t *cadence_mask, int M, const int32_t *neighbors, double *corr, int32_t *n_common,
                                     double *metric);
int lk_underfit_grid_neighbors_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                         const double *flux, const uint8_t *cadence_mask, int M, const int32_t *neighbors,
                                         double *corr, int32_t *n_common, double *metric, void *stream);
int lk_underfit_grid_rows_bytes(int Bn, int Nx, int64_t *bytes);
int lk_underfit_grid_rows_prepare_dev(lk_handle *h, int Bn, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                      const double *flux_nb, const uint8_t *cadence_mask, void *block, int64_t block_bytes,
                                      void *stream);
int lk_underfit_grid_against_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                            const double *flux, const uint8_t *cadence_mask, int Bn, const void *block, int M,
                                            const int32_t *neighbors, double *corr, int32_t *n_common, double *metric,
                                            void *stream);

/* ---- Over-fitting goodness metric of B targets (reference src/lightkurve/correctors/metrics.py:24-138
 * overfit_metric_lombscargle, as CBVCorrector.over_fitting_metric calls it on lc[cadence_mask]).  time, flux_orig, flux_corr,
 * err_corr: B x N, NaN-free flux; keep_idx: the n kept cadences shared by every target (ascending indices into [0, N)), or
 * NULL = all cadences (then n == N).  Per target b on its kept cadences:
 *   z0 = flux_orig / numpy.median(flux_orig) - 1.0, z1 = flux_corr / numpy.median(flux_corr) - 1.0 (exact medians),
 *   mean_unc = nanmean(err_corr / median(flux_corr));
 *   P0, P1 = the default Lomb-Scargle ('fast', amplitude normalisation, fit_mean = center_data = 1, oversampling 5) of z0, z1
 *   at the times t - t[first kept] on the grid f0 + df * arange(M) [1/d];  Pn_k = the same of g_k = normal * mean_unc;
 *   change = P1 - P0 (NaN dropped), n_up = #(change > 0), S = sum of the positive changes;
 *   per_k = 0 if n_up == 0, inf if n_up * nanmean(Pn_k) == 0, else S / (n_up * nanmean(Pn_k));
 *   metric[b] = 2 / (1 + exp(max(mean_k per_k, 0))), NaN propagating as numpy's does.
 * NOISE.  The reference draws from the global numpy.random; here a counter-based generator gives any (target, sample,
 * cadence) the same number whatever B, the launch shape or the number of sample rounds: Philox4x32-10 (multipliers
 * 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter =
 * (i, k, first_target + b, stream_id): i the pair of kept cadences (2i, 2i + 1), k the sample, b the row.  From the output
 * words x0..x3: u1 = (((x0 >> 5) << 26) + (x1 >> 6) + 1) 2^-53, u2 = (((x2 >> 5) << 26) + (x3 >> 6)) 2^-53,
 * r = sqrt(-2 ln u1); cadence 2i gets r cos(2 pi u2), cadence 2i + 1 gets r sin(2 pi u2) (dropped for the last pair of an
 * odd n).  first_target + B <= 2^32, 0 <= stream_id < 2^32.
 * SCRATCH.  The periodograms run through the LS 'fast' launcher, which owns the handle's scratch arena, so rows, noise and
 * spectra live in `scratch`, a 256-byte aligned device block of the caller's: z0, z1 (B n each), and per round of R samples
 * R B n times + R B n noise + R B M spectra, plus P0, P1 (B M each).  lk_overfit_scratch_bytes returns the size for the
 * largest R <= n_samples that fits max_scratch_bytes (0: LK_OVERFIT_SCRATCH_DEFAULT), or for R = 1 when none does; the _dev
 * call takes the largest R that fits scratch_bytes.  R does not change a bit of the result; nor do B or the rows around a
 * target; two runs give the same bits (every sum has an order that depends on its length alone; no atomics).
 * B >= 1, 3 <= n <= N, M >= 2, n_samples >= 1, scratch_bytes >= the R = 1 size: LK_EINVAL otherwise.  The host flavour
 * stages its buffers and its scratch in the handle's staging arena and also checks keep_idx.  The _dev call enqueues on
 * `stream`; it adds no synchronisation to the LS launcher's own. */
#define LK_OVERFIT_SCRATCH_DEFAULT ((int64_t)4 << 30)
int lk_overfit_scratch_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                             int *samples_per_round);
int lk_overfit_metric_batch(lk_handle *h, int B, int N, const double *time, const double *flux_orig, const double *flux_corr,
                            const double *err_corr, int n, const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples,
                            uint64_t seed, int64_t first_target, int64_t stream_id, int64_t max_scratch_bytes, double *metric);
int lk_overfit_metric_batch_dev(lk_handle *h, int B, int N, const double *time, const double *flux_orig, const double *flux_corr,
                                const double *err_corr, int n, const int32_t *keep_idx, double f0, double df, int64_t M,
                                int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *scratch,
                                int64_t scratch_bytes, double *metric, void *stream);
/* The metric as a SESSION, for scoring many corrections of one original batch with one noise stream (a ridge search: common
 * random numbers).  `session` is a 256-byte aligned device block of the caller's with the size and the sample rounds of the
 * unsplit call's scratch (lk_overfit_session_bytes: the arguments and answers of lk_overfit_scratch_bytes); it is caller-owned
 * because the LS launcher resets the handle's arena.  begin does once what does not depend on the correction: z0, the rebased
 * times, P0 and u_k[b] = nanmean(LS of the UNIT normals of sample k).  eval, any number of times with the shapes, keep_idx and
 * grid of begin: z1, mean_unc, P1 (ONE LS launch of B rows), n_up and S against the kept P0, and the closed form with
 * nanmean(Pn_k) = |mean_unc| * u_k (the amplitude-normalised periodogram is homogeneous of degree one in its input).  P0 and P1
 * are the bits of the unsplit call, hence n_up and S too; the metric differs from it by the rounding of |mean_unc| * u_k against
 * nanmean(LS(normal * mean_unc)) alone.  A NaN mean_unc gives NaN and a zero one per_k = inf (metric 0) when n_up > 0; n_up == 0
 * gives per_k = 0.  eval allocates nothing, leaves everything begin wrote intact, and its result does not depend on the
 * evaluations before it. */
int lk_overfit_session_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                             int *samples_per_round);
int lk_overfit_session_begin_dev(lk_handle *h, int B, int N, const double *time, const double *flux_orig, int n,
                                 const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples, uint64_t seed,
                                 int64_t first_target, int64_t stream_id, void *session, int64_t session_bytes, void *stream);
int lk_overfit_session_eval_dev(lk_handle *h, int B, int N, const double *flux_corr, const double *err_corr, int n,
                                const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples, void *session,
                                int64_t session_bytes, double *metric, void *stream);
/* The over-fitting metric and its session for a RAGGED batch, on the batch's own offsets.  Each call is its uniform namesake with
 * (N, n, keep_idx) replaced by
 *   n_off_host: B + 1 int64, target b holds cadences [n_off[b], n_off[b + 1]) of time / flux_orig / flux_corr / err_corr (sum n);
 *   keep_idx:   int32 (sum kept), target-relative ascending indices of the kept cadences of every target, packed by k_off_host;
 *               NULL = all cadences;
 *   k_off_host: the B + 1 offsets into keep_idx (NULL, or n_off_host itself, when keep_idx is NULL).
 * lk_overfit_scratch_rows_bytes / lk_overfit_session_rows_bytes take k_off_host alone (the batch's own offsets when all cadences
 * are kept).  Per target the arithmetic, every summation order and the Philox counter (pair of kept cadences OF THAT TARGET,
 * sample, first_target + b, stream_id) are the uniform call's: target b gives the bits of the uniform call on a one-target batch
 * that holds its kept cadences with first_target + b as first_target, and a uniform batch gives the bits of the uniform entry
 * points.  The block holds what the uniform block holds with sum kept in place of B n, then the two offset tables (2 (B + 1)
 * int64).  Every target needs at least three kept cadences: LK_EINVAL names the first that has fewer.  The host flavour also
 * checks keep_idx.  Both offset tables are read before a call returns; session_begin_rows puts them into the block and
 * session_eval_rows reads them there, so an evaluation must be given begin's offsets (they size its plan and its periodogram
 * launch).  The _dev calls enqueue on `stream` and add no synchronisation to the LS launcher's own. */
int lk_overfit_scratch_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes,
                                  int64_t *bytes, int *samples_per_round);
int lk_overfit_metric_rows_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux_orig,
                                 const double *flux_corr, const double *err_corr, const int32_t *keep_idx, const int64_t *k_off,
                                 double f0, double df, int64_t M, int n_samples, uint64_t seed, int64_t first_target,
                                 int64_t stream_id, int64_t max_scratch_bytes, double *metric);
int lk_overfit_metric_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux_orig,
                                     const double *flux_corr, const double *err_corr, const int32_t *keep_idx,
                                     const int64_t *k_off_host, double f0, double df, int64_t M, int n_samples, uint64_t seed,
                                     int64_t first_target, int64_t stream_id, void *scratch, int64_t scratch_bytes, double *metric,
                                     void *stream);
int lk_overfit_session_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes,
                                  int64_t *bytes, int *samples_per_round);
int lk_overfit_session_begin_rows_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux_orig,
                                      const int32_t *keep_idx, const int64_t *k_off_host, double f0, double df, int64_t M,
                                      int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *session,
                                      int64_t session_bytes, void *stream);
int lk_overfit_session_eval_rows_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *flux_corr, const double *err_corr,
                                     const int32_t *keep_idx, const int64_t *k_off_host, double f0, double df, int64_t M,
                                     int n_samples, void *session, int64_t session_bytes, double *metric, void *stream);
/* out[b][c] = the standard normal of (target first_target + b, sample k, kept cadence c), B x n float64 on the device (16-byte
 * aligned): the generator of lk_overfit_metric_batch on its own. */
int lk_overfit_noise_batch_dev(lk_handle *h, int B, int n, int k, uint64_t seed, int64_t first_target, int64_t stream_id,
                               double *out, void *stream);

/* ---- LightCurve.flatten trend: masked, gap-segmented Savitzky-Golay + sigma-clip loop + linear re-interpolation
 * t (non-decreasing per target), flux (may hold NaN); mask: 1 = EXCLUDE the cadence from the fit (lightkurve's
 * `mask=` semantics) or NULL; window (odd), polyorder, break_tol (NaN = no gap splitting), niters, sigma as in
 * LightCurve.flatten (lightcurve.py:943).  trend: (sum N), what flatten divides flux and flux_err by;
 * fit_mask: (sum N) bytes or NULL, 1 = cadence survived every clip. */
int lk_savgol_trend_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux,
                          const uint8_t *mask, int window, int polyorder, double break_tol, int niters,
                          double sigma, double *trend, uint8_t *fit_mask);
int lk_savgol_trend_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                              const uint8_t *mask, int window, int polyorder, double break_tol, int niters,
                              double sigma, double *trend, uint8_t *fit_mask, void *stream);
/* Host-only helper (no GPU): the FIR taps (window doubles) and the two edge-refit operators
 * (2 x (window/2) x window doubles, left then right) the kernel uses == scipy savgol_coeffs / mode='interp' in exact
 * arithmetic: rows of the least-squares hat matrix, each entry within one ulp of the row's largest weight of the exact value
 * for every polyorder 0..15 (scipy's own taps lose all digits towards polyorder 15). */
int lk_savgol_design(int window, int polyorder, double *coeffs, double *edge);

/* ---- PLDCorrector.create_design_matrix (correctors/pldcorrector.py:186-287) for B same-shaped cutouts --------
 * pld_pix: B x N x P float32 pixel fluxes inside the PLD aperture (NULL / P = 0: no pixel block);
 * bkg_pix: B x N x Pb float32 background pixels; lc_flux: B x N float32 SAP flux; time: B x N;
 * knots: B x (n_inner + 2) = [min(t), interior knots (percentiles of t, as patsy's bs()), max(t)];
 * n_knots = n_inner + spline_degree + 1 spline columns (+1 constant).  normalize_bkg: divide background pixels
 * by their row sum.  X: B x N x K row-major with K = lk_pld_design_width(...):
 *   [ PCA(pixels/flux) | PCA(2-fold products) | ... | PCA(background) | B-splines | 1 ];  prior_sigma: B x K.
 * A block wider than 4096 columns before PCA (e.g. 29 components at order 3: 4495 products) is refused with LK_EINVAL.
 * normalize_bkg with Pb <= pca_components: the rows of the normalised block sum to 1, so the centred block has rank Pb - 1
 * and the last of its min(pca_components, Pb) columns is a quotient of rounding errors, as in the reference; the leading
 * Pb - 1 columns are the block's basis (tests/test_pld_blocks_gpu.py asserts on those). */
int lk_pld_design_width(int P, int Pb, int pld_order, int pca_components, int n_knots);
int lk_pld_design_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                        const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                        int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, double *X,
                        double *prior_sigma);
int lk_pld_design_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                            const float *lc_flux, const double *time, const double *knots, int n_inner,
                            int pld_order, int pca_components, int n_knots, int spline_degree, int normalize_bkg,
                            int K, double *X, double *prior_sigma, void *stream);

/* ---- PLDCorrector.correct (correctors/pldcorrector.py:304-427) for B same-shaped cutouts in ONE call: the design
 * matrices above, RegressionCorrector.correct over them (prior_mu = 0, prior_sigma from the design, y / err = the SAP
 * light curve in float64, cadence_mask nullable) and — `spline_part`, nullable — the spline block's share of the model
 * X[:, K-(n_knots+1):] w[K-(n_knots+1):] that restore_trend adds back (pldcorrector.py:418-420, before its median is
 * removed).  Host pointers; X stays in device memory between the two stages.  pld_pix == bkg_pix (same pointer, P == Pb)
 * is uploaded once.  Outputs as lk_regress_batch: w B x K, model B x N (median removed), outlier B x N bytes. */
int lk_pld_correct_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                         const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                         int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                         const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *w,
                         double *model, uint8_t *outlier, double *spline_part);
/* The same on DEVICE pointers, enqueued on `stream` (no synchronisation).  X (B x N x K doubles), prior_sigma and prior_mu
 * (B x K doubles each) are device scratch PROVIDED BY THE CALLER and must stay untouched until the stream has passed this
 * call: they are not parked in the handle's staging arena, which a later host-pointer call on the same handle re-carves.
 * pld_pix == bkg_pix (same pointer, P == Pb) for one aperture.  `corrected` (nullable, B x N) receives what
 * PLDCorrector.correct returns (pldcorrector.py:418-420): (y - model) + (spline_part - median(spline_part)) when
 * spline_part is given (restore_trend=True; np.median: the mean of the two middle values for an even N), else y - model. */
int lk_pld_correct_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                             const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                             int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                             const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *X,
                             double *prior_sigma, double *prior_mu, double *w, double *model, uint8_t *outlier,
                             double *spline_part, double *corrected, void *stream);

/* Ragged pixel blocks: lk_pld_correct_batch / lk_pld_correct_batch_dev for cutouts whose PLD and background masks differ in
 * size.  pld_pix is B x N x P and bkg_pix B x N x Pb with P / Pb the ROW PITCH (the largest count): cutout b's first
 * p_count[b] / pb_count[b] columns are its pixels, the columns behind them hold exactly +0.0f
 * (lk_pld_gather_ragged_batch_dev writes that layout).  p_count / pb_count: B int32 each — HOST arrays for
 * lk_pld_correct_ragged_batch, DEVICE arrays for the _dev form; NULL = every cutout uses all P / Pb columns (then the call is
 * the uniform one, same bits).  The result for cutout b equals the uniform call on that cutout's own columns to the PLD
 * parity of this library (1e-6 of the flux; measured: equal bits where the pitch is <= 138 columns, 3.3e-8 at 225): zero
 * columns have zero means and zero rows / columns in the Gram matrix, and every eigen-solver route works on matrix b's own
 * leading count x count block and gives the padding zero eigenvector rows.  K = lk_pld_design_width(P, Pb, ...).
 * LK_EINVAL if a count is below pca_components (the design width would differ between cutouts), below 1, or above the
 * pitch.  The _dev form copies the 2 B counts back for that check (it synchronises `stream` once more than the uniform
 * call). */
int lk_pld_correct_ragged_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                                const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                                int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                                const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *w,
                                double *model, uint8_t *outlier, double *spline_part, const int32_t *p_count,
                                const int32_t *pb_count);
int lk_pld_correct_ragged_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                                    const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                                    int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K,
                                    const double *y, const double *err, const uint8_t *cadence_mask, double clip_sigma,
                                    int niters, double *X, double *prior_sigma, double *prior_mu, double *w, double *model,
                                    uint8_t *outlier, double *spline_part, double *corrected, void *stream,
                                    const int32_t *p_count, const int32_t *pb_count);

/* ---- Resident pixel cubes: what PLDCorrector does to a target-pixel file BEFORE the design matrix, for B same-shaped
 * float32 cutouts flux / flux_err [B][N][npix] in device memory (npix = ny * nx row-major, the layout lk_fits_unpack_cube
 * writes per column).  All take device pointers and a stream.
 *
 * lk_cube_aperture_batch_dev <- TargetPixelFile.to_lightcurve(aperture_mask), flux_method='sum'
 *   (src/lightkurve/targetpixelfile.py:868-923) + the NaN-cadence mask of PLDCorrector.__init__
 *   (correctors/pldcorrector.py:109-120).  mask: npix bytes shared by the batch (mask_stride = 0) or B x npix
 *   (mask_stride = npix).  flux_out / err_out: B x N float32, bit-identical to numpy on float32 cubes: the aperture's pixels
 *   of a cadence are added one after the other in pixel order in float32, err = sqrt(sum(e * e)), NaN pixels count as 0, the
 *   flux is NaN where no aperture pixel is finite or the whole cadence image is 0.  keep_out: B x N bytes,
 *   !(isnan(flux) | isnan(err)).  kept_host[b]: kept cadences, nonfinite_host[b] (nullable): kept cadences with a non-finite
 *   pixel anywhere in the image — HOST arrays: the call synchronises `stream`.
 * lk_cube_median_image_batch_dev <- np.nanmedian(tpf.flux, axis=0) inside create_threshold_mask
 *   (targetpixelfile.py:680-742), over the cadences with keep != 0 (keep NULL: all): median B x npix float64, exact, NaN
 *   for a pixel without a value.  Enqueued, no synchronisation.
 * lk_pld_gather_batch_dev <- tpf[~nan_mask] and tpf.flux[:, mask] of PLDCorrector (pldcorrector.py:109-120, 203-227) + the
 *   percentile knots of its spline (np.percentile(time, ...), :262-268).  n: the kept cadences of EVERY cutout (LK_EINVAL
 *   if keep says otherwise).  Compacted t_out / y_out / err_out (float64, the float32 sums widened) / lcf_out (float32), each
 *   B x n and nullable; pld_out B x n x P / bkg_out B x n x Pb = the pixels listed in pld_idx_host / bkg_idx_host (HOST int32,
 *   ascending pixel numbers; stride 0: one list for the batch, stride P / Pb: one per cutout; NULL with P == npix: every
 *   pixel).  A block whose output is NULL is skipped (all pixels of all cadences kept: the block IS the cube, and
 *   lk_cube_aperture_batch_dev's nonfinite_host answers for its pixels).  knots_out (nullable) B x (n_inner + 2) = [t[0],
 *   lerp(t[lo_k], t[lo_k + 1], g_k) ..., t[n - 1]] with numpy's _lerp from the HOST plan knot_lo_host / knot_g_host (n_inner
 *   each; times must be non-decreasing).  *nonfinite_host = 1 if a gathered pixel is not finite.  Synchronises.
 * lk_cube_threshold_mask_batch_dev <- threshold_mask_from_median_image (targetpixelfile.py:700-742) on the B x (ny x nx)
 *   float64 median images of lk_cube_median_image_batch_dev, one workgroup per cutout, exactly: vals = the finite pixels,
 *   mad = median(|vals - median(vals)|) (np.median: mean of the two middle values), cut = (1.4826 * mad * threshold) +
 *   nanmedian(image) rounded product by product, mask = nan_to_num(image) >= cut; no finite pixel: empty mask.  use_ref != 0:
 *   only the 4-connected region holding the masked pixel nearest to (ref_col, ref_row) stays (squared distances; the first
 *   minimum in row-major order); an empty mask stays empty.  invert != 0 flips the result ('background' =
 *   ~threshold_mask(0, no reference pixel)).  mask: B x npix bytes, count: B int32, idx: B x npix int32 = the selected pixel
 *   numbers ascending, then -1.  ny * nx <= LK_CUBE_MASK_MAX_NPIX (64 x 64; the labels live in LDS), else LK_EINVAL.
 *   Enqueued, no synchronisation.
 * lk_pld_gather_ragged_batch_dev <- lk_pld_gather_batch_dev with per-cutout index lists of different lengths ON THE DEVICE:
 *   pld_idx / bkg_idx are B rows of pld_idx_stride / bkg_idx_stride (>= P / Pb) int32, ascending pixel numbers then -1
 *   (lk_cube_threshold_mask_batch_dev's idx with stride npix, or uploaded lists).  pld_out B x n x P / bkg_out B x n x Pb with
 *   P / Pb the largest count: a padded column holds exactly +0.0f and does not count for *nonfinite_host.  An entry >= npix
 *   is LK_EINVAL.  Everything else as lk_pld_gather_batch_dev.  Synchronises. */
#define LK_CUBE_MASK_MAX_NPIX 4096
int lk_cube_aperture_batch_dev(lk_handle *h, int B, int N, int npix, const float *flux, const float *flux_err,
                               const uint8_t *mask, int mask_stride, float *flux_out, float *err_out, uint8_t *keep_out,
                               int64_t *kept_host, int64_t *nonfinite_host, void *stream);
int lk_cube_median_image_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *keep,
                                   double *median, void *stream);
int lk_pld_gather_batch_dev(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time,
                            const float *flux32, const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx_host,
                            int pld_idx_stride, int Pb, const int32_t *bkg_idx_host, int bkg_idx_stride, int n_inner,
                            const int32_t *knot_lo_host, const double *knot_g_host, double *t_out, double *y_out,
                            double *err_out, float *lcf_out, float *pld_out, float *bkg_out, double *knots_out,
                            int *nonfinite_host, void *stream);
int lk_cube_threshold_mask_batch_dev(lk_handle *h, int B, int ny, int nx, const double *median, double threshold, int use_ref,
                                     double ref_col, double ref_row, int invert, uint8_t *mask, int32_t *count, int32_t *idx,
                                     void *stream);
int lk_pld_gather_ragged_batch_dev(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time,
                                   const float *flux32, const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx,
                                   int pld_idx_stride, int Pb, const int32_t *bkg_idx, int bkg_idx_stride, int n_inner,
                                   const int32_t *knot_lo_host, const double *knot_g_host, double *t_out, double *y_out,
                                   double *err_out, float *lcf_out, float *pld_out, float *bkg_out, double *knots_out,
                                   int *nonfinite_host, void *stream);

/* lk_cube_centroids_batch_dev <- TargetPixelFile.estimate_centroids(aperture_mask, method='moments') for the same resident
 *   cubes: col[b][i] = sum_p (column0 + x_p) m_p flux_p / sum_p m_p flux_p and row likewise with (row0 + y_p), pixel p at
 *   x_p = p % nx, y_p = p / nx; sums in float64, NaN pixels count as 0 (nansum), a zero or NaN total gives NaN.  mask /
 *   mask_stride as lk_cube_aperture_batch_dev.  col_out / row_out: B x N float64.  One wavefront per cadence; the order of
 *   its sums depends on npix alone.  Enqueued, no synchronisation. */
int lk_cube_centroids_batch_dev(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                int mask_stride, double column0, double row0, double *col_out, double *row_out, void *stream);

/* lk_cube_centroids_quadratic_batch_dev <- TargetPixelFile.estimate_centroids(aperture_mask, method='quadratic'), i.e.
 *   lightkurve.utils.centroid_quadratic(data, mask) per cadence of the same resident cubes (ny = npix / nx >= 3, nx >= 3, else
 *   LK_EINVAL):  z = data * mask (a masked-out finite pixel is 0, a masked-out NaN or inf pixel NaN);  k = nanargmax(z), the first
 *   flat index of the largest value that is not NaN;  (yy, xx) = divmod(k, nx) clamped into [1, ny - 2] x [1, nx - 2];  the 3 x 3
 *   patch of z around (yy, xx), row-major;  the least-squares quadratic P = a + b x + c y + d x^2 + e x y + f y^2 over x, y in
 *   {0, 1, 2} ((A^T A)^-1 A^T is an integer matrix over 36, hard-coded);  det = 4 d f - e^2, |det| < 1e-6 -> NaN, otherwise
 *   xm = -(2 f b - c e) / det, ym = -(2 d c - b e) / det and col = column0 + xx - 1 + xm, row = row0 + yy - 1 + ym: the pixel-
 *   index convention of lk_cube_centroids_batch_dev (a symmetric source centred on pixel (i, j) gives (i, j)).  A NaN inside the
 *   patch gives NaN; a cadence without any value gives NaN and peak -1 (nothing is raised).  All float64 after the float32 load.
 *   mask / mask_stride as lk_cube_aperture_batch_dev.  col_out / row_out: B x N float64; peak_out (nullable): B x N int32, k
 *   before the clamp or -1.  One wavefront per cadence, the cube is read once.  Enqueued, no synchronisation.
 * lk_image_centroids_batch_dev <- the same two estimators (method = LK_CENTROID_MOMENTS: the formula of
 *   lk_cube_centroids_batch_dev; LK_CENTROID_QUADRATIC: the one above) on B float64 images [B][npix], one wavefront per image.
 *   col_out / row_out: B float64; peak_out (nullable, B int32): the quadratic's k, -1 for the moments.  Enqueued.
 * lk_cube_diffimage_batch_dev <- the transit difference image of every cutout, one box (period, transit_time, duration: HOST
 *   arrays of B) per cutout.  Cadence i of cutout b with time t has x = np_mod(t - t0 + P/2, P) - P/2 (the expression of
 *   lk_transit_mask_batch) and the class 1 (in) where |x| < in_width D, 2 (out) where out_inner D <= |x| < out_outer D, 0
 *   otherwise and for a NaN time.  0 < in_width <= out_inner < out_outer and P != 0, else LK_EINVAL.  Per pixel p, summing the
 *   float32 values in float64: mean_in / mean_out = the mean of flux[p] over the in / out cadences where it is not NaN (n_in[p],
 *   n_out[p] of them); diff = mean_out - mean_in; diff_err = sqrt(sum_in e^2 / n_in[p]^2 + sum_out e^2 / n_out[p]^2) with e =
 *   flux_err[p] at the same cadences (a NaN error there gives NaN).  A pixel with n_in[p] == 0 or n_out[p] == 0 is NaN in every
 *   image that needs the missing count.  Outputs on the device: cadence_class B x N bytes; mean_in, mean_out, diff, diff_err
 *   B x npix float64; n_in, n_out B int32 = the CADENCES of each class.  A workgroup sums a chunk of 128 cadences of one cutout
 *   (lanes = pixels), a second kernel adds the chunks in index order: no floating-point atomics, the order of every sum depends
 *   on N alone, so a cutout's images have the same bits alone, in any batch and from run to run.  Cadences without a class are
 *   not read.  Scratch: B x ceil(N / 128) x npix x 40 bytes of the handle's arena.  Enqueued, no synchronisation.
 * lk_diffimage_offsets_batch_dev <- offset[b] = (diff_col - out_col, diff_row - out_row) (B x 2), offset_pix[b] = its norm and
 *   status[b] (all on the device): 1 n_in[b] == 0, 2 n_out[b] == 0, 3 a centroid that is NaN, else 0.  Enqueued. */
#define LK_CENTROID_MOMENTS 0
#define LK_CENTROID_QUADRATIC 1
int lk_cube_centroids_quadratic_batch_dev(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                          int mask_stride, double column0, double row0, double *col_out, double *row_out,
                                          int32_t *peak_out, void *stream);
int lk_image_centroids_batch_dev(lk_handle *h, int B, int npix, int nx, const double *image, const uint8_t *mask, int mask_stride,
                                 double column0, double row0, int method, double *col_out, double *row_out, int32_t *peak_out,
                                 void *stream);
int lk_cube_diffimage_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const float *flux_err,
                                const double *period, const double *transit_time, const double *duration, double in_width,
                                double out_inner, double out_outer, uint8_t *cadence_class, double *mean_in, double *mean_out,
                                double *diff, double *diff_err, int32_t *n_in, int32_t *n_out, void *stream);
int lk_diffimage_offsets_batch_dev(lk_handle *h, int B, const int32_t *n_in, const int32_t *n_out, const double *diff_col,
                                   const double *diff_row, const double *out_col, const double *out_row, double *offset,
                                   double *offset_pix, int32_t *status, void *stream);

/* lk_cube_ampimage_batch_dev <- the amplitude images of every cutout (PixelCube.amplitude_image is the numpy mirror): a truncated
 *   Fourier series of ONE frequency per cutout (frequency: HOST array of B, 1/d) fitted to every pixel's time series, the
 *   periodic twin of lk_cube_diffimage_batch_dev.  nterms in 1 .. 3, K = 2 nterms + 1; nterms outside that, a NULL buffer or
 *   N * npix >= 2^31 give LK_EINVAL.  flux_err is not read.
 *   Cadences: t_ref (HOST array of B) is the reference time of each cutout, by convention its first finite time.  Cadences with
 *   a non-finite time are dropped (their rows are not loaded); pixel p is fitted on the remaining cadences where its own flux is
 *   not NaN, n_used[p] of them, unweighted.
 *   Design: that of lk_ls_model_batch with fit_mean, center_data and unit weights — columns [1, sin(2 pi m f (t - t_ref)),
 *   cos(2 pi m f (t - t_ref))], m = 1 .. nterms, y centred on the pixel's own mean y_mean; pixel p equals
 *   ls_model_host(t[ok], y[ok, p], None, f, nterms, singular="nan") on its own cadences (with that function's phases referred
 *   to t_ref).  All float64 after the float32 load.
 *   Images, coefficient- or harmonic-major so that each is one block of B images (what lk_image_centroids_batch_dev takes):
 *   theta [K][B][npix] (slot 0 the bias, then sin 1, cos 1, ...); level [B][npix] = y_mean + bias, the mean image under the
 *   signal; amplitude [nterms][B][npix] = hypot(s_m, c_m); phase = atan2(c_m, s_m), of the periodic part A sin(w t + phase);
 *   chi2 [B][npix] = sum (y - model)^2, from the residuals of a second pass over the cube; with sigma2 = chi2 / (n_used - K) and C
 *   the inverse of the pixel's normal matrix, amplitude_err [nterms][B][npix] = sqrt(sigma2 (s^2 C_ss + 2 s c C_sc + c^2 C_cc)) /
 *   amplitude and snr = amplitude / amplitude_err; n_used [B][npix] int32.
 *   Degenerate pixels: n_used < K, or a pivot or coefficient that is zero / not finite -> NaN in every float image; n_used == K
 *   -> NaN amplitude_err and snr.  Nothing is raised per pixel.
 *   fit_status [B] int32: 0 fitted; 1 the frequency is NaN or <= 0; 2 fewer than K + 1 cadences with a finite time.  Where it is
 *   not 0 the cutout is skipped: its float images are NaN, its n_used 0.
 *   A workgroup sums a chunk of 128 cadences of one cutout (lanes = pixels, the chunk's sines and cosines staged in LDS, float64
 *   partials against a per-pixel pivot), further kernels add the chunks in index order and solve per pixel: no floating-point
 *   atomics, the order of every sum depends on N alone, so a cutout's images have the same bits alone, in any batch position
 *   and from run to run.  Scratch: about B x ceil(N / 128) x npix x (K + (K + 1) K / 2 + 2) x 8 bytes plus B x N x (16 nterms + 1)
 *   of the handle's arena.  Enqueued, no synchronisation.
 * lk_ampimage_offsets_batch_dev <- offset[b] = (amp_col - level_col, amp_row - level_row) (B x 2), offset_pix[b] = its norm and
 *   status[b] (all on the device): fit_status[b] where that is not 0, 3 a centroid that is NaN, else 0.  The centroids are
 *   lk_image_centroids_batch_dev's of amplitude[0] and level.  Enqueued. */
int lk_cube_ampimage_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency,
                               int nterms, const double *t_ref, double *theta, double *level, double *amplitude, double *phase,
                               double *amplitude_err, double *snr, double *chi2, int32_t *n_used, int32_t *fit_status,
                               void *stream);
int lk_ampimage_offsets_batch_dev(lk_handle *h, int B, const int32_t *fit_status, const double *amp_col, const double *amp_row,
                                  const double *level_col, const double *level_row, double *offset, double *offset_pix,
                                  int32_t *status, void *stream);

/* lk_cube_pixel_ls_batch_dev <- one Lomb-Scargle spectrum per pixel of every cutout on ONE shared grid, and its peak (PixelCube.
 *   pixel_periodogram is the numpy mirror): which pixels vary and at which frequency, what TargetPixelFile.plot_pixels(
 *   periodogram=True) loops for.  frequency: HOST array of F, 1/d, every entry finite and > 0.  normalization: LK_NORM_LK_AMPLITUDE
 *   or LK_NORM_LK_PSD.  A NULL non-nullable buffer, B, N, npix or F < 1, B > 65535, N * npix >= 2^31, F * npix >= 2^31, a bad
 *   frequency, another normalization or an oversample_factor that is not finite and > 0 give LK_EINVAL.  flux_err is not read.
 *   Cadences: t_ref (HOST array of B) is the reference time of each cutout, by convention its first finite time (NaN where it
 *   has none).  Cadences with a non-finite time are dropped (their rows are not loaded); pixel p is taken on the remaining
 *   cadences where its own flux is not NaN, n_used[p] of them, with unit weights.
 *   Spectrum: astropy's floating-mean GLS (fit_mean, center_data) from the exact sums with weights 1 / n_used[p], then
 *   P_psd = P * n_used / 2 and LK_NORM_LK_AMPLITUDE: sqrt(P_psd) sqrt(4 / n_used); LK_NORM_LK_PSD: P_psd * 2 / (n_used *
 *   oversample_factor * fs), fs = 1 / (t_last - t_first) / oversample_factor * 1e6 / 86400 from the pixel's own first and last
 *   used time — what lk_ls_batch gives for that light curve with the same normalization.  S, C, S2, C2 are summed once per
 *   (cutout, frequency) and shared by the pixels; only sum y sin and sum y cos are per pixel, taken against a per-pixel pivot
 *   (its first value), the mean put back through S and C; what a pixel's missing cadences added to the shared sums is
 *   accumulated on the NaN branch and taken off.  Phases from (t - t_ref) with the product f (t - t_ref) reduced exactly, one
 *   sine / cosine pair per (cadence, frequency), no recurrence.  All float64 after the float32 load.
 *   Outputs on the device: power (nullable) [B][F][npix] float64, pixel fastest; peak_index [B][npix] int32, the first index of
 *   the largest non-NaN power, -1 without one; peak_power [B][npix] float64, the bits of power there, NaN without one; n_used
 *   [B][npix] int32; status [B] int32.  With power == NULL nothing of the size F * npix is written.
 *   Degenerate cases: a pixel with n_used < 4 has a NaN spectrum; a cutout with fewer than 4 finite times has status 2, every
 *   spectrum NaN and n_used 0 (status 0 otherwise).  Nothing is raised per pixel.
 *   One wavefront owns (cutout, 16 frequencies, up to 128 adjacent pixels, two per lane) and walks all N cadences in chunks of 32
 *   whose sines and cosines it stages in LDS; pixel groups in which a pixel lacks cadences take a second instantiation with one
 *   pixel per lane.  No floating-point atomics, the order of every sum depends on N alone, so a cutout's outputs have the same
 *   bits alone, at any batch position, with or without power and from run to run.  Scratch: B x npix x (24 + 12 ceil(F / 16))
 *   bytes plus 8 F of the handle's arena.  Enqueued, no synchronisation. */
int lk_cube_pixel_ls_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency,
                               int F, int normalization, double oversample_factor, const double *t_ref, double *power,
                               double *peak_power, int32_t *peak_index, int32_t *n_used, int32_t *status, void *stream);

/* lk_cube_psf_photometry_batch_dev <- deblended PSF photometry per cadence of every cutout (PixelCube.psf_photometry is the numpy
 *   mirror and the definition): the fluxes of up to 8 stars at KNOWN positions and one constant background, by weighted linear
 *   least squares on every cadence's image.  What TargetPixelFile.to_lightcurve(method="prf") is used for, in its linear form: no
 *   position or width is fitted, the PSF is a pixel-integrated Gaussian and not a tabulated PRF.
 *   Stars: star_col / star_row are HOST arrays [B][S_max], 1 <= S_max <= 8, in the coordinates of lk_cube_centroids_batch_dev
 *   (pixel (iy, ix) covers [column0 + ix - 1/2, column0 + ix + 1/2] x [row0 + iy - 1/2, row0 + iy + 1/2]).  A star with a NaN
 *   coordinate is not part of its cutout; the others keep their order: cutout b has S_b of them and owns the output rows
 *   star_off[b] .. star_off[b] + S_b - 1, star_off the prefix sums of S_b (written to the HOST array star_off of B + 1 int32 when
 *   that is not NULL).  sigma: HOST array [B][2] = (sigma_col, sigma_row) in pixels.  shift_col / shift_row (nullable, both or
 *   neither): DEVICE arrays [B][N] added to every star's position at that cadence.
 *   PSF of star s at cadence n: with c = star_col[s] + shift_col[n] - column0 and E_c(k) = erf((k - 1/2 - c) / (sqrt(2)
 *   sigma_col)), k = 0 .. nx, the column factor is (E_c(ix + 1) - E_c(ix)) / 2; the row factor likewise from r and sigma_row;
 *   g[iy][ix] = their product.  Without shifts the nx + ny factors of a star are formed once per cutout, with shifts once per
 *   cadence.
 *   Fit: the design of a cadence is A = [g_0 ... g_{S-1}, 1] over its used pixels: those in the mask (mask / mask_stride as
 *   lk_cube_aperture_batch_dev) whose flux is finite and, with use_flux_err != 0, whose flux_err is finite and > 0.  Weights
 *   w = 1 / flux_err^2 in float64 from the float32 value, or 1 (flux_err is then not read).  G = A^T W A and rhs = A^T W y are
 *   summed over the used pixels, G is factored by Cholesky without pivoting in index order; the cadence is SINGULAR
 *   when a pivot d_k is not finite or d_k <= 1e-12 G_kk.  flux[s] = theta_s, flux_err[s] = sqrt((G^-1)_ss), background =
 *   theta_S, chi2 = sum w (y - A theta)^2 from the residuals, n_used = the used pixels.  All float64 after the float32 load.
 *   Outputs on the device: flux_out / flux_err_out [star_off[B]][N] float64 (row-major: every star is one light curve of N
 *   cadences); time_out (nullable) [star_off[B]][N] float64: every row's times, those of its cutout; background, chi2 [B][N]
 *   float64; n_used [B][N] int32; cadence_status [B][N] int8: 0 ok, 1 the time or a shift is not finite, 2 n_used < S + 2, 3
 *   singular (in that order of precedence) — a cadence that is not ok has NaN in flux, flux_err, background and chi2, nothing
 *   is raised; status [B] int32: 0, or 1 when no cadence of the cutout is ok.
 *   LK_EINVAL: a NULL required buffer, B < 1 or > 65535, N, ny or nx < 1, N * npix >= 2^31, S_max outside 1 .. 8, a cutout
 *   without a star, an infinite star coordinate, a sigma that is not finite and > 0, one shift array without the other, a
 *   mask_stride that is neither 0 nor npix, or a cutout too large for the LDS tile: 16 x 8 pitch + npix + 8 S_max (nx + ny) x
 *   (16 with shifts, else 1) bytes must not exceed 160 KiB, pitch = npix rounded up to 4 x an odd number (4 pitch instead of
 *   8 with use_flux_err == 0).
 *   Four lanes per cadence: a workgroup of one wavefront stages 16 consecutive cadences of flux and flux_err in LDS; lane k of
 *   a cadence walks the pixel rows k, k + 4, ... in index order with the (S + 1)(S + 2) / 2 + S + 1 sums in registers (the
 *   kernel is instantiated on S; the cutouts of a batch are grouped by their star count), the four partial sums are added in
 *   a fixed order, every lane solves, and chi2 is taken from the same tile: flux and flux_err are read from HBM once.  No
 *   atomics; the order of every sum depends on the cutout's own data alone, so a cutout's outputs have the same bits alone,
 *   at any batch position and from run to run.  Scratch: B x (S_max (nx + ny + 2) + 2) x 8 + 12 B bytes of the handle's
 *   arena.  Enqueued, no synchronisation. */
int lk_cube_psf_photometry_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                     const float *flux_err, const uint8_t *mask, int mask_stride, int S_max,
                                     const double *star_col, const double *star_row, const double *sigma, const double *shift_col,
                                     const double *shift_row, double column0, double row0, int use_flux_err, int32_t *star_off,
                                     double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                                     int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream);

/* lk_cube_prf_photometry_batch_dev <- lk_cube_psf_photometry_batch_dev with a TABULATED PRF in place of the Gaussian
 *   (TabulatedPRF.evaluate and PixelCube.psf_photometry(prf=) are the numpy mirror and the definition): what
 *   TargetPixelFile.to_lightcurve(method="prf") evaluates through KeplerPRF, in its linear form.  No position, shift or width is
 *   fitted, no mission file is read and the corner tables of a channel are not blended: the caller passes the blended array.
 *   Inputs, stars, shifts, mask, used pixels, weights, the design A = [g_0 ... g_{S-1}, 1], the Cholesky with its pivot cut
 *   1e-12 G_kk, the outputs, star_off and the statuses 0 .. 3 are those of lk_cube_psf_photometry_batch_dev; sigma is not taken.
 *   prf_table: DEVICE float32 [n_prf][Ty][Tx], row-major, every value finite (not checked here); oversample = os >= 1, an
 *   integer; Ty, Tx >= 1 of any parity.  prf_index: HOST int32 [B], the table of every cutout, or NULL: table 0 for all.
 *   Sample (j, i) is the fraction of a star's flux collected by a pixel whose centre lies ((i - (Tx - 1) / 2) / os, (j - (Ty - 1)
 *   / 2) / os) px from the star's centre — already pixel-integrated; nothing is normalised.
 *   Model of star s at cadence n: Keys' cubic convolution (a = -1/2, Catmull-Rom) on the table continued by zeros, float64.  With
 *   c = star_col[s] + shift_col[n] - column0, u = (0 - c) os + (Tx - 1) / 2, i0 = floor(u), f = u - i0 (likewise r, v, j0, g from
 *   star_row, shift_row, row0 and Ty):
 *     w_-1 = ((-f + 2) f - 1) f / 2   w_0 = ((3 f - 5) f f + 2) / 2   w_1 = ((-3 f + 4) f + 1) f / 2   w_2 = (f - 1) f f / 2
 *     g[iy][ix] = sum_{jj = -1 .. 2} w_jj(g) (sum_{ii = -1 .. 2} w_ii(f) T[j0 + iy os + jj][i0 + ix os + ii]),  T = 0 outside,
 *   both sums in that order.  os is an integer, so the pixels of a cutout share f and g: they are formed once per (star,
 *   cadence), at pixel 0.  A star with |u| or |v| >= 1e9, or a NaN shift, has no tap on the table.  A star whose model is zero on
 *   every used pixel makes the cadence singular (status 3) through the pivot cut; there is no status of its own.
 *   LK_EINVAL: as lk_cube_psf_photometry_batch_dev without the sigma case, and n_prf, Ty, Tx or oversample < 1, a prf_index
 *   outside 0 .. n_prf - 1, n_prf os^2 ceil(Ty / os) ceil(Tx / os) >= 2^30, max(ny, nx) os >= 2^30, or a cutout too large for
 *   the LDS of one workgroup: tile + images must not exceed 160 KiB, where tile = 16 x 8 pitch + npix (4 pitch instead of 8 with
 *   use_flux_err == 0), pitch = npix rounded up to 4 x an odd number, and images = 8 S_max npix without shifts, 16 x (8 mpitch +
 *   128 S_max) with them, mpitch = S_max npix rounded up to 4 x an odd number.
 *   The table is first re-laid in polyphase order, Tp[table][py][px][Y][X] = T[table][Y os + py][X os + px], so that each of
 *   the 16 taps of a cutout's pixels is one contiguous sub-image.  Without shifts a star's image is the same at every cadence:
 *   one workgroup per cutout forms the S images once, and the fit kernel — the four-lanes-per-cadence workgroup of
 *   lk_cube_psf_photometry_batch_dev, instantiated on S — copies them to LDS.  With shifts the fit kernel forms the images of
 *   its 16 cadences itself, lane = pixel, and parks them in LDS for both walks.  No atomics; the order of every sum depends on
 *   the cutout's own data alone, so a cutout's outputs have the same bits alone, at any batch position, with prf_index NULL,
 *   shared or per cutout, and from run to run.  Scratch: B x (2 S_max + 2) x 8 + 16 B + 4 n_prf os^2 ceil(Ty / os) ceil(Tx / os)
 *   bytes of the handle's arena, and 8 B S_max npix more without shifts.  Enqueued, no synchronisation. */
int lk_cube_prf_photometry_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                     const float *flux_err, const uint8_t *mask, int mask_stride, int S_max,
                                     const double *star_col, const double *star_row, const float *prf_table, int n_prf, int Ty,
                                     int Tx, int oversample, const int32_t *prf_index, const double *shift_col,
                                     const double *shift_row, double column0, double row0, int use_flux_err, int32_t *star_off,
                                     double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                                     int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream);

/* lk_cube_psf_fit_batch_dev <- PSF photometry that fits each cadence's pointing shift (PixelCube.psf_fit is the numpy mirror and the
 *   definition): per cadence the fluxes of up to 8 stars, one constant background and ONE common (column, row) shift u = (dc, dr)
 *   of all stars, by variable projection in Kaufman's form.  The per-cadence motion shift of TargetPixelFile.to_lightcurve(method=
 *   "prf"); per-star positions, the PSF width, rotation and a background gradient are not fitted; with a tabulated PRF in place
 *   of the Gaussian the call is lk_cube_prf_fit_batch_dev.
 *   Inputs, stars, sigma, mask, PSF, used pixels, weights, design A(u) = [g_0 ... g_{S-1}, 1], K = S + 1, and the output rows are
 *   those of lk_cube_psf_photometry_batch_dev.  shift0_col / shift0_row (nullable, both or neither): DEVICE arrays [B][N], the
 *   initial shift u0 of every cadence (0 without them).  The used pixels do not depend on u.
 *   Per cadence, from u = u0, for it = 1 .. max_iter:
 *     1. G = A^T W A, rhs = A^T W y at u; G = L L^T by the unpivoted Cholesky of lk_cube_psf_photometry_batch_dev with its pivot
 *        cut 1e-12 G_kk (a failed pivot: status 3); theta = G^-1 rhs.
 *     2. r = y - A theta; D = [sum_s theta_s dg_s/ddc, sum_s theta_s dg_s/ddr] over the used pixels, where the derivative of a
 *        column factor (E(ix + 1) - E(ix)) / 2 by the centre is -(P(ix + 1) - P(ix)), P(k) = exp(-z_k^2) / (sqrt(2 pi) sigma_col),
 *        z_k = (k - 1/2 - c) / (sqrt(2) sigma_col), rows likewise.  C = A^T W D (K x 2), E = D^T W D (2 x 2), g = D^T W r,
 *        S2 = E - (L^-1 C)^T (L^-1 C), factored by the same Cholesky with the pivot cut 1e-12 E_kk (a failed pivot: status 3);
 *        du = S2^-1 g.
 *     3. each component of du is clamped to +-max_step; u += du; n_iter = it; last_step = max |du| after the clamp.  If
 *        max |u - u0| > max_shift: status 5, stop.  If tol > 0 and last_step < tol: converged, stop.
 *   After max_iter iterations a cadence that has not converged has status 4 when tol > 0; tol == 0 means "take exactly max_iter
 *   steps" and is status 0.  A status 0 cadence is evaluated once more at the final u: flux, flux_err = sqrt((G^-1)_ss),
 *   background and chi2 are those of lk_cube_psf_photometry_batch_dev at shifts = u (errors conditional on the shift), and
 *   shift_col_err / shift_row_err = sqrt((S2^-1)_kk) of that evaluation (a failed pivot there: status 3).
 *   cadence_status [B][N] int8: 0 ok, 1 the time or u0 is not finite, 2 n_used < S + 4, 3 singular, 4 not converged, 5 left
 *   max_shift.  A cadence that is not ok is NaN in flux, flux_err, background, chi2, shift_col, shift_row and their errors;
 *   n_iter [B][N] int32 (the shift updates made) and last_step [B][N] float64 are written for every cadence (0 / NaN for
 *   statuses 1 and 2, and NaN before the first update); n_used [B][N] int32; status [B] int32: 0, or 1 when no cadence of the
 *   cutout is ok.  shift_col, shift_row, shift_col_err, shift_row_err: [B][N] float64, the layout the shifts of
 *   lk_cube_psf_photometry_batch_dev take.  Nothing is raised per cadence.
 *   LK_EINVAL: as lk_cube_psf_photometry_batch_dev, and max_iter outside 1 .. 64, tol not finite or < 0, max_step or max_shift
 *   not > 0, or a cutout too large for the LDS tile: 16 x 8 pitch + npix + 2 x 16 x 8 S_max (nx + ny) bytes (factor and
 *   derivative tables) must not exceed 160 KiB (4 pitch instead of 8 with use_flux_err == 0); nothing is launched then.
 *   One wavefront per tile of 16 cadences, four lanes per cadence, instantiated on S: flux, flux_err and the mask are staged in
 *   LDS once and every iteration reads LDS alone; per evaluation the lanes of a cadence rebuild its factor and derivative
 *   tables (every edge's erf and exp serve both pixels it separates), walk the tile for G and rhs, solve, and walk it again
 *   for C, E, g and chi2; the loop runs until every cadence of the tile has stopped.  No atomics; a cutout's outputs have the
 *   same bits alone, at any batch position and from run to run.  Scratch: B x (2 S_max + 2) x 8 + 12 B bytes of the handle's
 *   arena.  Enqueued, no synchronisation. */
int lk_cube_psf_fit_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                              const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                              const double *star_row, const double *sigma, const double *shift0_col, const double *shift0_row,
                              int max_iter, double tol, double max_step, double max_shift, double column0, double row0,
                              int use_flux_err, int32_t *star_off, double *time_out, double *flux_out, double *flux_err_out,
                              double *background, double *chi2, double *shift_col, double *shift_row, double *shift_col_err,
                              double *shift_row_err, double *last_step, int32_t *n_iter, int32_t *n_used, int8_t *cadence_status,
                              int32_t *status, void *stream);

/* lk_cube_prf_fit_batch_dev <- lk_cube_psf_fit_batch_dev with a TABULATED PRF in place of the Gaussian (PixelCube.psf_fit(prf=) and
 *   TabulatedPRF.evaluate_with_gradient are the numpy mirror and the definition): the per-cadence shift fitted with the model
 *   that lk_cube_prf_photometry_batch_dev then takes at shifts = (shift_col, shift_row).  The argument list is
 *   lk_cube_psf_fit_batch_dev's with sigma replaced by the table arguments of lk_cube_prf_photometry_batch_dev (prf_table DEVICE
 *   float32 [n_prf][Ty][Tx], oversample, prf_index HOST int32 [B] or NULL).  Steps 1 to 3 of lk_cube_psf_fit_batch_dev, the used
 *   pixels, the weights, both pivot cuts, the clamp, tol, max_shift, the evaluation at the final u, the statuses 0 .. 5 (2: n_used <
 *   S + 4) and every output hold word for word, with
 *     A_s = g_s of lk_cube_prf_photometry_batch_dev at c = star_col[s] + dc - column0, r = star_row[s] + dr - row0, and
 *     D = [sum_s theta_s dg_s/dc, sum_s theta_s dg_s/dr], s in index order — a shift and a centre enter as one sum, so the
 *     derivative by the shift is the derivative by the centre: the same 16 taps with the derivative weights of the same f,
 *       w'_-1 = ((-3 f + 4) f - 1) / 2   w'_0 = (9 f - 10) f / 2   w'_1 = ((-9 f + 8) f + 1) / 2   w'_2 = (3 f - 2) f / 2,
 *     each times du/dc = -os; dg/dc = sum_jj w_jj(g) (sum_ii w'_ii(f) T), dg/dr = sum_jj w'_jj(g) (sum_ii w_ii(f) T), in the order
 *     of g.  Keys' interpolant is C1: the derivative is continuous, which is what Gauss-Newton needs.
 *   A cadence whose stars all have a zero model or a zero derivative on the used pixels fails a pivot cut: status 3.
 *   LK_EINVAL: where either parent returns it (max_iter outside 1 .. 64, a prf_index outside 0 .. n_prf - 1, max(ny, nx) os >=
 *   2^30, ...), or a cutout too large for the LDS of one workgroup.  A workgroup holds a tile of 16 cadences, or of 8 where 16 do
 *   not fit; per cadence 8 (mpitch + dpitch + S + 3) + 192 S + 8 pitch bytes (4 pitch with use_flux_err == 0), plus 8 + npix per
 *   workgroup, where pitch, mpitch and dpitch are npix, S npix and 2 npix rounded up to 4 x an odd number.  The launch of S stars
 *   takes 16 cadences when they fit 160 KiB and 8 otherwise; the call is refused, before anything is launched or written, only
 *   when 8 cadences at S_max do not fit.  At 11 x 11 with flux_err: 16 cadences up to 6 stars (160 513 bytes), 8 cadences at 7
 *   and 8 (89 601 and 98 881).  A cadence's outputs do not depend on the tile length.
 *   One workgroup per tile, instantiated on S: 512 threads (eight wavefronts) up to 6 stars, 256 threads (four wavefronts) at 7
 *   and 8 stars, where the fit's registers leave no room for eight; the polyphase copy of the table is made once per call.  Per
 *   evaluation all wavefronts form the S model images of every cadence in LDS, wavefront 0 — the four-lanes-per-cadence
 *   wavefront of lk_cube_psf_fit_batch_dev — solves for theta, all wavefronts form the two theta-weighted derivative images (2
 *   npix doubles per cadence, not 2 S npix), and wavefront 0 walks again for C, E, g and chi2 and takes the step; the loop runs
 *   until every cadence of the tile has stopped.  No atomics; a cutout's outputs have the same bits alone, at any batch position,
 *   with prf_index NULL, shared or per cutout, and from run to run.  Scratch: B x (2 S_max + 2) x 8 + 16 B + 4 n_prf os^2 ceil(Ty /
 *   os) ceil(Tx / os) bytes of the handle's arena.  Enqueued, no synchronisation. */
int lk_cube_prf_fit_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                              const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                              const double *star_row, const float *prf_table, int n_prf, int Ty, int Tx, int oversample,
                              const int32_t *prf_index, const double *shift0_col, const double *shift0_row, int max_iter, double tol,
                              double max_step, double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off,
                              double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                              double *shift_col, double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step,
                              int32_t *n_iter, int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream);

/* lk_cube_psf_width_batch_dev <- the PSF width of every cutout, fitted (PixelCube.psf_width is the numpy mirror and the definition):
 *   ONE pair v = (sigma_col, sigma_row) per cutout, shared by all its cadences, by variable projection in Kaufman's form with the
 *   linear unknowns (the fluxes of up to 8 stars and one background PER CADENCE) projected out.  The PSF scale of
 *   TargetPixelFile.to_lightcurve(method="prf"); the chain is lk_cube_psf_fit_batch_dev(a guess of sigma) -> this call at the
 *   fitted shifts -> lk_cube_psf_fit_batch_dev or lk_cube_psf_photometry_batch_dev at the fitted sigma.  Per-star positions, a
 *   width that varies with time or across the cutout, tabulated PRFs, rotation and a background gradient are not fitted.
 *   Inputs, stars, mask, PSF, used pixels, weights, design A = [g_0 ... g_{S-1}, 1], K = S + 1, the Cholesky and its pivot cut
 *   1e-12 G_kk are those of lk_cube_psf_photometry_batch_dev.  sigma0: HOST array [B][2], the start.  shift_col / shift_row
 *   (nullable, both or neither): DEVICE arrays [B][N] added to every star's position at that cadence.  cadence_mask (nullable):
 *   DEVICE array [B][N] uint8, non-zero = the width is fitted on this cadence.
 *   A cadence is ELIGIBLE when cadence_mask selects it, its time and its shift are finite and n_used >= S + 2; that does not
 *   depend on v.  One EVALUATION at v, per eligible cadence n: G = A^T W A, rhs = A^T W y, G = L L^T, theta = G^-1 rhs, r = y - A
 *   theta; D = [sum_s theta_s dg_s/dsigma_col, sum_s theta_s dg_s/dsigma_row] over the used pixels, where the derivative of a
 *   column factor (erf(z_{k+1}) - erf(z_k)) / 2, z_k = (k - 1/2 - c) / (sqrt(2) sigma_col), by sigma_col is -(Q(k + 1) - Q(k)),
 *   Q(k) = (k - 1/2 - c) exp(-z_k^2) / (sqrt(2 pi) sigma_col^2), rows likewise; C = A^T W D (K x 2), E = D^T W D, g_n = D^T W r,
 *   S2_n = E - (L^-1 C)^T (L^-1 C), chi2_n = sum w r^2.  A cadence whose G fails a pivot is singular at this evaluation and
 *   contributes nothing.  The cutout's sums g = sum g_n, H = sum S2_n, chi2 = sum chi2_n, n_cadences and n_pixels = sum n_used
 *   run over the contributing cadences in an order fixed by N alone.
 *   Per cutout, from v = sigma0, for it = 1 .. max_iter:
 *     1. evaluate at v;
 *     2. n_cadences == 0: status 1, stop;
 *     3. H = L2 L2^T by the 2 x 2 Cholesky without pivoting; singular when H_00 is not finite and > 0 or d_11 is not finite and
 *        > 1e-12 H_11: status 3, stop;
 *     4. dv = H^-1 g, each component clamped to +-max_step;
 *     5. v += dv, n_iter = it, last_step = max |dv| after the clamp;
 *     6. a component of v not in [min_sigma, max_sigma]: status 5, stop;
 *     7. tol > 0 and last_step < tol: converged, stop.
 *   After max_iter steps without convergence the status is 4; tol == 0 means "take exactly max_iter steps" and is status 0.  A
 *   status 0 cutout is evaluated once more at its final v (no cadence there: status 1; H singular: status 3): sigma [B][2] = v,
 *   sigma_err [B][2] = sqrt((H^-1)_kk) (not scaled by chi2 and conditional on the shifts, the convention of flux_err),
 *   sigma_cov [B] = (H^-1)_01 and chi2 [B] are those of that evaluation.  A failed cutout is NaN in these four; nothing is raised.
 *   Written for every cutout: status [B] int32; n_iter [B] int32 (the updates made); last_step [B] float64 (NaN before the first
 *   update); n_cadences [B] int32 and n_pixels [B] int64 of the last evaluation made; trace [B][max_iter + 1][2] float64: row k
 *   is the v of evaluation k + 1, NaN beyond the evaluations made — the final evaluation is made at, and rewrites, row n_iter,
 *   so a status 0 cutout has n_iter + 1 rows that are not NaN, a failed one the points it evaluated, and a v that left the bounds
 *   (status 5) is not in it; cadence_status [B][N] int8 from the last evaluation made, in this order of precedence: 6 not
 *   selected by cadence_mask, 1 the time or a shift is not finite, 2 n_used < S + 2, 3 singular, 0 contributed.
 *   LK_EINVAL: where lk_cube_psf_fit_batch_dev returns it (its LDS bound included: 16 x 8 pitch + npix + 2 x 16 x 8 S_max (nx +
 *   ny) bytes, a factor and a derivative table per cadence, must not exceed 160 KiB), and max_iter outside 1 .. 64, tol not
 *   finite or < 0, max_step not > 0, min_sigma or max_sigma not finite, or not 0 < min_sigma <= sigma0 <= max_sigma; nothing is
 *   launched then.
 *   Two kernels per evaluation, enqueued max_iter + 1 times with no synchronisation and no host read in between.  Evaluate: one
 *   wavefront per tile of 16 cadences, four lanes per cadence, instantiated on S, the staging, the tables and the two walks of
 *   lk_cube_psf_fit_batch_dev with the derivatives by the width; it reads v from the cutout's state record and returns at once
 *   when the cutout has stopped, and a tile that cadence_mask leaves out entirely is not read; the tile's 16 cadences are added by a fixed butterfly (a cadence that does not contribute
 *   enters as +0) into one 64-byte record per tile.  Step: one wavefront per cutout adds the tile records lane-strided in index
 *   order and then by the butterfly, factors H, applies the rules above and advances the state.  No atomics; a cutout's outputs
 *   have the same bits alone, at any batch position, with any other cutouts in the batch and from run to run.  Scratch: B x
 *   ceil(N / 16) x 64 bytes of tile records, 40 B of state, B x (2 S_max + 2) x 8 + 12 B of the stars, of the handle's arena.
 *   Enqueued, no synchronisation. */
int lk_cube_psf_width_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                                const double *star_row, const double *sigma0, const double *shift_col, const double *shift_row,
                                const uint8_t *cadence_mask, int max_iter, double tol, double max_step, double min_sigma,
                                double max_sigma, double column0, double row0, int use_flux_err, double *sigma, double *sigma_err,
                                double *sigma_cov, double *chi2, double *last_step, double *trace, int32_t *n_iter,
                                int32_t *n_cadences, int64_t *n_pixels, int8_t *cadence_status, int32_t *status, void *stream);

/* lk_cube_psf_positions_batch_dev <- the positions of every cutout's stars, fitted (PixelCube.psf_positions is the numpy mirror and
 *   the definition): ONE (column, row) per fitted star, shared by all the cutout's cadences, by variable projection in Kaufman's
 *   form with the linear unknowns (the fluxes of up to 8 stars and one background PER CADENCE) projected out.  The last unknown of
 *   TargetPixelFile.to_lightcurve(method="prf") that the calls above take as given; the chain is lk_cube_psf_fit_batch_dev(a
 *   guess) -> this call at the fitted shifts -> lk_cube_psf_width_batch_dev at the same shifts -> lk_cube_psf_fit_batch_dev or
 *   lk_cube_psf_photometry_batch_dev.  THE FIT IS CONDITIONAL ON THE SHIFTS (and the width): a translation common to all stars
 *   is the same model as a constant added to every shift; the call never frees both, and fit_star can pin an anchor star.
 *   Inputs, stars (NaN = an empty slot), mask, sigma (HOST [B][2], given and not fitted), PSF, used pixels, weights, design A =
 *   [g_0 ... g_{S-1}, 1], K = S + 1, the Cholesky and its pivot cut 1e-12 G_kk are those of lk_cube_psf_photometry_batch_dev;
 *   shift_col / shift_row and cadence_mask those of lk_cube_psf_width_batch_dev.  fit_star (nullable): HOST array [B][S_max]
 *   uint8 in the caller's slot layout, non-zero = the star of that slot is fitted; NULL = every star present is fitted.  A star
 *   that is not fitted stays at its given position.
 *   The unknowns v are (column, row) of the fitted stars in slot order, v[2j] the column and v[2j + 1] the row of the j-th
 *   fitted star, P = 2 x their number <= 16; v starts at the given positions.  A cadence is ELIGIBLE when cadence_mask selects
 *   it, its time and its shift are finite and n_used >= S + 2; that does not depend on v.  One EVALUATION at v, per eligible
 *   cadence n: G = A^T W A, rhs = A^T W y, G = L L^T, theta = G^-1 rhs, r = y - A theta; D has one column per unknown, for star s
 *   theta_s (dg_s^col/dc) g_s^row and theta_s g_s^col (dg_s^row/dc) over the used pixels, the derivative of a factor (erf(z_{k+1})
 *   - erf(z_k)) / 2, z_k = (k - 1/2 - c) / (sqrt(2) sigma), by its centre c being -(P(k + 1) - P(k)), P(k) = exp(-z_k^2) /
 *   (sqrt(2 pi) sigma) (lk_cube_psf_fit_batch_dev's derivative by the shift: a shift and a centre enter as one sum); C = A^T W D
 *   (K x P), E = D^T W D, g_n = D^T W r, S2_n = E - (L^-1 C)^T (L^-1 C), chi2_n = sum w r^2.  A cadence whose G fails a pivot is
 *   singular at this evaluation and contributes nothing.  The cutout's sums g = sum g_n, H = sum S2_n, chi2 = sum chi2_n,
 *   n_cadences and n_pixels = sum n_used run over the contributing cadences in an order fixed by N alone.
 *   Per cutout, for it = 1 .. max_iter:
 *     1. evaluate at v;
 *     2. n_cadences == 0: status 1, stop;
 *     3. H = L2 L2^T by the P x P Cholesky without pivoting; singular when a pivot d_k is not finite and > 1e-12 H_kk: status 3,
 *        stop;
 *     4. dv = H^-1 g, each component clamped to +-max_step;
 *     5. v += dv, n_iter = it, last_step = max |dv| after the clamp;
 *     6. a component of v farther than max_offset from its start: status 5, stop;
 *     7. tol > 0 and last_step < tol: converged, stop.
 *   After max_iter steps without convergence the status is 4; tol == 0 means "take exactly max_iter steps" and is status 0.  A
 *   status 0 cutout is evaluated once more at its final v (no cadence there: status 1; H singular: status 3) for the outputs,
 *   all in the caller's slot layout: star_col_out / star_row_out [B][S_max]: the fitted values, the given value bit for bit for
 *   a star that is not fitted, NaN in an empty slot; star_col_err / star_row_err [B][S_max] = sqrt((H^-1)_kk) (not scaled by
 *   chi2, conditional on the shifts and the width), NaN where the star is not fitted; position_cov [B][2 S_max][2 S_max] = H^-1
 *   at index 2 slot + axis, NaN rows and columns where the star is not fitted; chi2 [B].  A failed cutout is NaN in the fitted
 *   stars' positions, their errors, position_cov and chi2; nothing is raised.
 *   Written for every cutout: status [B] int32; n_iter [B] int32 (the updates made); last_step [B] float64 (NaN before the first
 *   update); n_cadences [B] int32 and n_pixels [B] int64 of the last evaluation made; trace [B][max_iter + 1][2 S_max] float64:
 *   row k holds the positions of evaluation k + 1 at index 2 slot + axis (a star that is not fitted at its given value, NaN in an
 *   empty slot), NaN beyond the evaluations made — the final evaluation is made at, and rewrites, row n_iter, so a status 0
 *   cutout has n_iter + 1 rows that are not NaN, a failed one the points it evaluated, and a v that left max_offset (status 5)
 *   is not in it; cadence_status [B][N] int8 from the last evaluation made, in this order of precedence: 6 not selected by
 *   cadence_mask, 1 the time or a shift is not finite, 2 n_used < S + 2, 3 singular, 0 contributed.
 *   LK_EINVAL: where lk_cube_psf_width_batch_dev returns it for the arguments they share, with this call's LDS bound: 16 x 8
 *   pitch + npix + 2 x 16 x 8 S_max (nx + ny) + 16 x 8 (S_max + 1) 2 S_max bytes (the tile, a factor and a derivative table per
 *   cadence, and the parked L^-1 C) must not exceed 160 KiB; max_offset not > 0; a cutout without a fitted star; nothing is
 *   launched then.
 *   Two kernels per evaluation, enqueued max_iter + 1 times with no synchronisation and no host read in between.  Evaluate: one
 *   wavefront per tile of 16 cadences, four lanes per cadence, instantiated on S, the staging, the tables and walk 1 of
 *   lk_cube_psf_fit_batch_dev; it reads v from the cutout's state record and returns at once when the cutout has stopped, and
 *   a tile that cadence_mask leaves out entirely is not read; all 2 S columns are evaluated (the Schur complement over the fitted
 *   subset is the submatrix of S2), walk 2 once per star in panels of two rows of E with L^-1 C parked in LDS; the tile's 16
 *   cadences are added entry by entry by a fixed butterfly (a cadence that does not contribute enters as +0) into one record per
 *   tile, P + P (P + 1) / 2 + 1 doubles (P = 2 S) stored entry-major, and two 64-bit counts.  Step: one wavefront per cutout adds
 *   every entry lane-strided over the tile records in index order and then by the butterfly, selects the fitted rows and columns,
 *   factors H, applies the rules above and advances the state.  No atomics; a cutout's outputs have the same bits alone, at any
 *   batch position, with any other cutouts in the batch and from run to run.  Scratch: B x ceil(N / 16) x (8 (2 S_max + S_max (2
 *   S_max + 1) + 1) + 16) bytes of tile records, 152 B of state, B x ((2 S_max + 2) x 8 + 12 + 4 S_max) of the stars, of the
 *   handle's arena.  Enqueued, no synchronisation. */
int lk_cube_psf_positions_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                    const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                                    const double *star_row, const double *sigma, const uint8_t *fit_star, const double *shift_col,
                                    const double *shift_row, const uint8_t *cadence_mask, int max_iter, double tol, double max_step,
                                    double max_offset, double column0, double row0, int use_flux_err, double *star_col_out,
                                    double *star_row_out, double *star_col_err, double *star_row_err, double *position_cov,
                                    double *chi2, double *last_step, double *trace, int32_t *n_iter, int32_t *n_cadences,
                                    int64_t *n_pixels, int8_t *cadence_status, int32_t *status, void *stream);

/* lk_cube_background_batch_dev <- TargetPixelFile.estimate_background(aperture_mask) per cadence of the same resident cubes,
 *   and the subtraction of that background, in one pass (PixelCube.estimate_background / subtract_background are the numpy
 *   mirror).  mask / mask_stride as lk_cube_aperture_batch_dev; sel = the masked pixels of cadence i of cutout b.
 *   bkg[b][i] (B x N float32) = np.nanmedian(sel) in float32: NaN is the only excluded value, +-inf are values, an even count
 *   gives float32(a + b) / 2 of the two middle values, no value (or an empty mask) gives NaN.  n_pixels[b][i] (B x N int32) =
 *   the values of sel that are not NaN.  want_scatter != 0: scatter[b][i] (B x N float32) = np.nanmedian(|sel - bkg|), all in
 *   float32, NaN differences excluded; otherwise scatter is not touched and may be NULL.  cube_out (nullable, B x N x npix
 *   float32, not the cube itself): cube[b][i][p] - bkg[b][i] for ALL npix pixels of the cadence.  Selection is exact: every
 *   output equals numpy's value for value, and a cutout's outputs have the same bits alone, at any position of a batch and
 *   from run to run.  Two routes, chosen from npix alone: npix <= 224 stages 64 cadences per workgroup in LDS, one wavefront
 *   per cadence ranks the selected pixels by counting; wider cutouts take one workgroup per cadence and a radix select.  The
 *   cube is read once (and written once).  No scratch.  Enqueued, no synchronisation.
 * lk_cube_subtract_rows_batch_dev <- cube_out[b][i][p] = cube[b][i][p] - rows[b][i] for rows (B x N float32) of the caller's.
 *   Enqueued, no synchronisation.
 * Both: B, N, npix >= 1, B <= 65535 and N * npix < 2^31, no NULL buffer but the nullable ones, else LK_EINVAL. */
int lk_cube_background_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *mask, int mask_stride,
                                 int want_scatter, float *bkg, int32_t *n_pixels, float *scatter, float *cube_out, void *stream);
int lk_cube_subtract_rows_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const float *rows, float *cube_out,
                                    void *stream);

/* ---- SFFCorrector.correct (self-flat-fielding, the K2 roll-motion correction; reference lightkurve 2.x
 * src/lightkurve/correctors/sffcorrector.py) for B ragged light curves.  Per target, all float64, inputs finite:
 *   f = flux / median(flux), e = flux_err / median(flux); raw_mean = mean(flux);
 *   arclength (_estimate_arclength): c = col - min(col), r = row - min(row); c = max(c) - c if the least-squares slope of r on
 *     c is negative (the sign of sum (c - mean c)(r - mean r)); arc = sqrt(c c + r r);
 *   windows: window_points are ascending cut indices in (0, N); window j = [lo_j, up_j), lo = [0, wp...], up = [wp..., N],
 *     W = number of points + 1;
 *   design matrix, K = n_knots + W (bins + degree) columns [ spline | window 1 | ... | window W ]:
 *     spline   = create_spline_matrix(time, n_knots), n_knots = int((time[-1] - time[0]) / timescale): the clamped cubic
 *                B-spline basis with n_knots - 4 interior knots at equally spaced percentiles of time; prior_mu[k] = mean of
 *                the k-th chunk of np.array_split(f, n_knots), prior_sigma = 1000 std(f) + 1e-6 (np.std);
 *     window j = the clamped B-spline basis (degree `degree`, intercept kept) of x = arc inside the window and -1 outside, with
 *                bins - 1 interior knots np.percentile(arc[lo_j:up_j], linspace(0, 100, bins + 1)[1:-1]) and boundary knots
 *                min(x), max(x): a cadence outside the window has [1, 0, ..., 0] there (the 1 as the basis itself evaluates at
 *                its lower boundary knot: 1 up to the rounding of the recursion); prior_mu = 0, prior_sigma = 10000
 *                std(f) + 1e-6.  "Outside" is decided BY INDEX; the reference decides it by value (~np.in1d(ar, ar[a:b])): the
 *                two differ only when an arclength outside the window is bit-equal to one inside it;
 *   fit = lk_regress_batch_dev on that matrix (clip_sigma, niters; cadence_mask nullable, 1 = used);
 *   corrected = f - model; spline / sff = the two column groups' shares of the model, each minus its median;
 *   restore_trend: corrected += spline - nanmedian(spline); finally corrected and e are multiplied by raw_mean.
 * status (HOST int32[B], valid on return: the _dev call synchronises `stream` once, to learn every target's n_knots):
 *   0 corrected; 1 too short (n_knots < 4); 2 a non-finite time, flux, flux_err or centroid; 3 K > 4095.  A target whose status
 *   is not 0 gets NaN flux / flux_err / spline / sff / w and outlier 0; no error is raised for it.
 * Outputs: flux_out, err_out (sum N), outlier (sum N bytes); nullable arclength, spline, sff (sum N) and w (B x w_pitch, row b
 *   = its K coefficients, NaN behind them; w_pitch >= the widest K).
 * win_off (B + 1) / window_points (int32, ragged): HOST arrays, target b owns [win_off[b], win_off[b+1]).
 * GROUPS AND SCRATCH.  K must be uniform per regression, so targets are grouped by (n_knots, W) and each group runs in chunks
 *   of targets; nothing is padded.  The regression launcher owns the handle's arena, so the design matrices (N K 8 bytes per
 *   target: ~6 GB for 1000 x 3500 x 213) and the other per-chunk arrays live in `scratch`, a 256-byte aligned device block of
 *   the caller's.  lk_sff_scratch_bytes(n_knots per target, as above) returns the block size whose chunks are the largest that
 *   fit max_scratch_bytes (0: LK_SFF_SCRATCH_DEFAULT) and their number; a budget below one target's own need is LK_EINVAL.
 *   A target's result has the same bits in any batch, at any position and for any chunk size; two runs give the same bits
 *   (every sum's order depends on the target's own sizes; no atomics).
 * lk_sff_correct_batch: host pointers; stages everything and its scratch (max_scratch_bytes) in the handle's staging arena.
 * lk_sff_arclength_batch(_dev): the arclength alone (the host needs it to choose windows); flipped (nullable) int32[B].
 * lk_sff_design_batch_dev: stops after the design matrix, for B targets of ONE group (n_knots given, the same W): X (sum N x
 *   K), prior_mu / prior_sigma (B x K), knots_time (B x (n_knots - 2): [min, interior..., max]), knots_win (B x W x (bins + 1)),
 *   f_out / e_out (sum N: the normalised flux and errors).  Its spline blocks are what lk_spline_basis_batch_dev gives for the
 *   same x and knots, bit for bit (one shared device function).  Enqueued, no synchronisation. */
#define LK_SFF_SCRATCH_DEFAULT ((int64_t)4 << 30)
int lk_sff_scratch_bytes(int B, const int64_t *n_off, const int32_t *n_knots, const int32_t *win_off, int bins, int degree,
                         int64_t max_scratch_bytes, int64_t *bytes, int *n_chunks);
int lk_sff_arclength_batch(lk_handle *h, int B, const int64_t *n_off, const double *centroid_col, const double *centroid_row,
                           double *arclength, int32_t *flipped);
int lk_sff_arclength_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *centroid_col,
                               const double *centroid_row, double *arclength, int32_t *flipped, void *stream);
int lk_sff_design_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                            const double *flux_err, const double *arclength, const int32_t *win_off, const int32_t *window_points,
                            int bins, int degree, int n_knots, double *X, double *prior_mu, double *prior_sigma,
                            double *knots_time, double *knots_win, double *f_out, double *e_out, void *stream);
int lk_sff_correct_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *flux_err,
                         const double *centroid_col, const double *centroid_row, const uint8_t *cadence_mask,
                         const int32_t *win_off, const int32_t *window_points, int bins, int degree, double timescale,
                         int restore_trend, double clip_sigma, int niters, int64_t max_scratch_bytes, double *flux_out,
                         double *err_out, uint8_t *outlier, int32_t *status, double *arclength, double *spline, double *sff,
                         double *w, int w_pitch);
int lk_sff_correct_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                             const double *flux_err, const double *centroid_col, const double *centroid_row,
                             const uint8_t *cadence_mask, const int32_t *win_off, const int32_t *window_points, int bins,
                             int degree, double timescale, int restore_trend, double clip_sigma, int niters, void *scratch,
                             int64_t scratch_bytes, double *flux_out, double *err_out, uint8_t *outlier, int32_t *status_host,
                             double *arclength, double *spline, double *sff, double *w, int w_pitch, void *stream);

/* ---- Standalone design-matrix operations (correctors/designmatrix.py) for B same-shaped matrices ----------------
 * lk_pca_batch          <- DesignMatrix.pca(nterms), designmatrix.py:252-282 (fbpca.pca(values, nterms) -> U): the first
 *                          k = nterms left singular vectors of the column-centred matrix; A: B x N x P row-major,
 *                          U: B x N x k.  A basis of the same subspace as the reference's (fbpca is a randomised range
 *                          finder: columns are defined up to sign, and up to rotation inside a degenerate cluster).
 *                          1 <= k <= min(48, P), P <= 4096.
 * lk_spline_basis_batch <- create_spline_matrix, designmatrix.py:952-997 (patsy bs(x, ..., include_intercept=True) - 1):
 *                          x: B x N; knots: B x (n_inner + 2) = [lower bound, interior knots, upper bound];
 *                          out: B x N x (n_inner + degree + 1).  (include_intercept=False drops column 0.)
 * lk_standardize_batch  <- DesignMatrix.standardize, designmatrix.py:215-250: per column, zeros are missing values;
 *                          (x - nanmedian) / nanstd of the rest, missing -> 0.  A column whose remaining values are all equal
 *                          (min == max, whether the value is representable or not) is left unchanged; a column holding
 *                          +-inf (no finite median or deviation) comes back as zeros. */
int lk_pca_batch(lk_handle *h, int B, int N, int P, int k, const double *A, double *U);
int lk_pca_batch_dev(lk_handle *h, int B, int N, int P, int k, const double *A, double *U, void *stream);
int lk_spline_basis_batch(lk_handle *h, int B, int N, const double *x, const double *knots, int n_inner, int degree,
                          double *out);
int lk_spline_basis_batch_dev(lk_handle *h, int B, int N, const double *x, const double *knots, int n_inner, int degree,
                              double *out, void *stream);
int lk_standardize_batch(lk_handle *h, int B, int N, int P, const double *A, double *out);
int lk_standardize_batch_dev(lk_handle *h, int B, int N, int P, const double *A, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LKHIP_H */
