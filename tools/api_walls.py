#!/usr/bin/env python
"""Wall time of the product's OTHER per-batch Python entry points (bench.py's `api_end_to_end` block covers the LS ones):
`batch.flatten_batch`, `batch.regression_correct_batch`, `batch.pld_correct_batch`, `batch.bls_batch`, one call each on a
list of objects, median of `reps` after one warm-up, with a cProfile of the last call (top entries by cumulative time) so
that host-side costs can be told from the GPU calls.  Usage: python tools/api_walls.py [flatten|regress|pld|bls ...]

`pld_dev`: the resident PLD path (`DevicePixelCubeBatch`) against `pld_correct_batch` on the same cutouts, 100 and 500 cutouts of
3500 x 11 x 11 (`LK_WALLS_SIZES`, default 100,500) in ONE process, the two paths alternating, median and min-max of `LK_WALLS_REPS` (default 5) repetitions each;
every timed region ends in a stream synchronise.  `pld_host`: only the `pld_correct_batch` rows (also runs on a checkout
that has no resident path: the baseline).  `pld_dev_trace`: only resident calls on `LK_WALLS_B` (default 500) cutouts — the
run to put under `rocprofv3 --kernel-trace --stats` for the kernel-time sum of one call (total / the printed call count).
`pld_ragged`: the resident call on `LK_WALLS_B` (default 500) cutouts whose threshold masks have five different sizes, three ways in
ONE process, alternating: R the ragged call (K2 default masks, `ragged_masks=True`), U the uniform call on the same cutouts with
every pixel in both masks, G what a user writes without the keyword — one call per group of equal mask size, on resident batches
built beforehand (their upload is not timed).

`underfit`: the under-fitting goodness metric of `LK_WALLS_B` (default 1000) cotrended targets x `LK_WALLS_N` (default 20000)
cadences with `LK_WALLS_M` (default 50) neighbours each, two ways in ONE process, alternating, `LK_WALLS_REPS` (default 3) times:
R the resident call (`cbv_correct(...)[0].under_fitting_metric(neighbors, cadence_mask)`: 8 bytes per target come back), R' the
same with `to_host=False` plus a synchronise, H the host route (download the corrected flux, then `underfit_metric_neighbors` per
target on 16 threads).  Every timed region ends in a synchronise.  `underfit_trace`: only resident calls — the run to put
under `rocprofv3 --kernel-trace --stats` for the two kernels' times.

`overfit`: the over-fitting goodness metric of `LK_WALLS_B` (default 1000) cotrended targets x `LK_WALLS_N` (default 20000)
cadences on the default grid with `LK_WALLS_SAMPLES` (default 10) noise samples, in ONE process, alternating, `LK_WALLS_REPS`
(default 3) times: R the resident call (`cbv_correct(...)[0].over_fitting_metric(batch)`), R' the same with `to_host=False` plus
a synchronise, H the host route (download both batches, then `overfit_metric_lombscargle` per target; its noise is numpy's, so H
and R agree in distribution, not in value; the loop is sequential: every one of its calls launches on the one handle, which serves
one call at a time, so the 16 threads of `underfit`'s host route, which is host arithmetic only, do not apply).  `overfit_trace`: only resident calls — the run to put under
`rocprofv3 --kernel-trace --stats`, in a run of its own, for the split between the LS passes and the metric's own kernels.

`cbvopt`: the per-target ridge search (`DeviceLightCurveBatch.cbv_correct_optimized`) of `LK_WALLS_B` (default 1000) targets x
`LK_WALLS_N` (default 20000) cadences on `LK_WALLS_K` (default 16) basis vectors + constant with `LK_WALLS_M` (default 50)
neighbours each and the default bounds, in ONE process, alternating, `LK_WALLS_REPS` (default 3) times after one warm-up: O the
whole call (the neighbours' own correction, the session's begin, the search, the final fit and its scores), S
`cbv_goodness_scan(n_samples=1)` over as many penalties as the search took lockstep evaluations (what driving the resident calls
one penalty at a time costs: three periodograms, the noise and the medians of all rows per penalty).  Prints the evaluation
counts.  `cbvopt_trace`: one search cut at `LK_WALLS_ITERS` (default 6) evaluations — the run to put under
`rocprofv3 --kernel-trace --stats`, in a run of its own, for what lies between two regressions.

`blsstats`: the vetting tail of a resident BLS survey on `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000)
cadences after a search on `LK_WALLS_P` (default 256) periods x 3 durations (the search is not timed), with `wall()`'s
repetitions: R the resident tail `result.compute_stats()` (peaks, the statistics kernel, the per-target numbers back), H the host
route (download time, flux and ivar, then `bls_compute_stats_host` per target at the same boxes).

`clean`: the transit-search front of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000) cadences with 0.5 % of
up-going outliers, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 3) times after one warm-up.  C the resident
chain `normalize().flatten(401).remove_outliers().to_periodogram_peaks(f)` on `LK_WALLS_M` (default 4096) frequencies; C_H the
same with the clip staged through the host, as it had to be without `remove_outliers`: `to_host()`, the sigma clip in numpy per
target, boolean indexing, `from_arrays`.  S `bls_search(periods, n_signals=2)` on `LK_WALLS_P` (default 64) periods x 3
durations of the flattened batch; S_H the same loop with `to_host()`, numpy `~mask` indexing and `from_arrays` between the
rounds.  `cdpp`: R `batch.estimate_cdpp()`; H `to_host()` + `lightcurve.estimate_cdpp_batch` on the list of light curves
(flatten and clip on the GPU from host arrays, the tail in numpy per target).  Results: profiles/clean_walls.txt.

`prewhiten`: `batch.prewhiten(frequency, n_signals=3)` of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000)
cadences on the benchmark's grid of `LK_WALLS_M` (default 100000) frequencies, in ONE process, the routes alternating,
`LK_WALLS_REPS` (default 3) times after one warm-up.  W the resident loop; W_H the same loop through the host: the peaks from
the resident periodogram, then `to_host()`, `ls_model_host` per target, `from_arrays` per round.  L one round's periodogram
pass alone (`to_periodogram_power(to_host=False, want_peaks=True)`), F one round's fit alone
(`ls_model(want_model=False, want_residual=True)`).  Results: profiles/prewhiten_walls.txt.

`seismology`: numax and deltanu of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000) two-minute cadences on
the natural grid (oversample_factor 1, up to the Nyquist frequency), in ONE process, the routes alternating, `LK_WALLS_REPS`
(default 3) times after one warm-up.  S the resident chain `batch.to_periodogram(f, "psd").estimate_seismology()`; S_H the
spectra brought to the host, then per target `Periodogram.flatten`, `estimate_numax_acf2d`, `estimate_deltanu_acf2d`; L the
periodogram pass alone.  Results: profiles/seismology_walls.txt.

`sff`: the SFF correction of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 3500) cadences with windows = 20 (one set
of window points, chosen once, for both routes), in ONE process, the routes alternating, `LK_WALLS_REPS` (default 2) times after
one warm-up.  R the resident call `batch.sff_correct(...)`; H the host route: `to_host()`, `SFFCorrector(lc).correct(...)` per
target, `from_arrays`.  Written to profiles/sff_walls.txt.

`cbvragged`: the CBV correction of a RAGGED batch, `LK_WALLS_B` (default 1000) targets on a grid of `LK_WALLS_N` (default
20000) cadences with about 3 % of them missing per target, `LK_WALLS_K` (default 17) columns, in ONE process, the routes
alternating, `LK_WALLS_REPS` (default 2) times after one warm-up.  S `from_arrays(cadenceno=)` ->
`cbv_correct(cadenceno=grid)`: one shared matrix; T the route a ragged batch had before: `X[rows_b]` per target ->
`regression_correct_batch` on the stacked copies.  Written to profiles/cbvragged_walls.txt.

`underfit_ragged`: the under-fitting metric of a RAGGED batch of that shape (`LK_WALLS_M`, default 50, nearest neighbours), in ONE
process, the routes alternating, `LK_WALLS_REPS` (default 3) times after one warm-up.  R the resident call
`under_fitting_metric(neighbors, cadenceno=grid)`; H the route a ragged batch had before: `to_host()`, the neighbours brought onto
each target's cadences (NaN where a neighbour lacks one) and `underfit_metric_neighbors` per target, 16 threads.  Written to
profiles/underfit_ragged_walls.txt.

`cbvopt_ragged`: the per-target ridge search of a ragged batch of that shape (`LK_WALLS_K`, default 16, basis vectors; `LK_WALLS_M`
neighbours), `LK_WALLS_REPS` (default 2) times after one warm-up.  O `cbv_correct_optimized(cadenceno=grid)`, the whole search; H
ONE evaluation of its objective the way a ragged batch had it: the resident ragged fit, `to_host()`, then
`underfit_metric_neighbors` (16 threads) and `overfit_metric_lombscargle` (sequential) per target on the host, over the first
`LK_WALLS_HOST_TARGETS` (default: all) targets.  Written to profiles/cbvopt_ragged_walls.txt.

`foldbin`: the phase-binned folded light curve of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000) cadences, one
period per target, `bins=LK_WALLS_BINS` (default 201), in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times
after one warm-up.  F the fused `batch.fold_bin(period, bins=)`; S `batch.fold(period).bin(bins=)` (sort, gathers, bins); H the host
route: `to_host()`, then numpy fold + bin per target on 16 threads.  Every timed region ends with the binned curves on the host.
Written to profiles/foldbin_walls.txt.

`river`: the river diagrams (cycle x phase images) of `LK_WALLS_B` (default 1000) targets x `LK_WALLS_N` (default 20000) cadences,
one period per target, default arguments (`LK_WALLS_METHOD`, default mean), in ONE process, the routes alternating, `LK_WALLS_REPS`
(default 5) times after one warm-up.  D `batch.river(period)` and a synchronise (images resident); T the same with `to_host()`; H
the host route: `to_host()` of the batch, then the numpy mirror per target on 16 threads.  Written to profiles/river_walls.txt.

`stitch`: `LK_WALLS_B` (default 1000) targets observed in `LK_WALLS_SEGMENTS` (default 4) sectors of `LK_WALLS_N` (default 5000)
cadences each, TESS-like cadence numbers that continue across a one-day gap between sectors, 3 % of the cadences missing inside
them, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  R `from_arrays(cadenceno=)`
-> `stitch(group)` -> `fill_gaps()` (the default noise: the resident CDPP of the stitched targets); R' the same with
`fill_gaps(noise_std="std")`; G as R' on the segments in sector-major order (the gather route of `stitch`); H the host route: `to_host()` of the resident segments, numpy normalize + concatenate + fill_gaps
by cadence number per target on 16 threads (noise of nanstd width from numpy's generator), then `from_arrays`.  Every timed
region ends with a synchronise.  Written to profiles/stitch_walls.txt.  `stitch_trace`: resident calls only (four with
`noise_std="std"`, then one with the CDPP), the run to put under `rocprofv3 --kernel-trace --stats`
(`profiles/stitch_kernel_stats.txt`).

`cbvinterp`: the CBV correction of a batch whose cadences are NOT rows of the CBV table, two shapes in ONE process: `LK_WALLS_B`
(default 1000) targets of about 3600 ten-minute cadences, each offset by a few seconds, on 18000 two-minute knots; and the same
number of two-minute targets (about 18000 cadences) on 1200 thirty-minute knots; `LK_WALLS_K` (default 16) basis vectors +
constant, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  I `from_arrays` ->
`cbv_correct(cbv_time=)`; H the route such a batch had before: `to_host()` of the resident batch,
`scipy.interpolate.PchipInterpolator` per target on 16 threads, `regression_correct_batch` on the per-target matrices.  Every timed
region ends with a synchronise.  Written to profiles/cbvinterp_walls.txt.  `cbvroutes`: the two older routes, U uniform
`cbv_correct` and C `cbv_correct(cadenceno=)` of `LK_WALLS_B` x `LK_WALLS_N` (default 1000 x 20000), printed only (run on a commit
and on its parent to show they did not move).

`diffimage`: the transit difference images of `LK_WALLS_B` (default 500) resident cutouts x `LK_WALLS_N` (default 4000) cadences x
`LK_WALLS_SIDE`^2 (default 11 x 11) pixels, one box per cutout, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5)
times after one warm-up.  R `cubes.difference_images(period, transit_time, duration)`; H the host route: `to_host()`, then
`PixelCube.difference_image` per cutout on 16 threads.  Every timed region ends with a synchronise.  Written to
profiles/diffimage_walls.txt.

`ampimage`: the amplitude images of the same batch shape (`LK_WALLS_B` x `LK_WALLS_N` x `LK_WALLS_SIDE`^2, defaults 500 x 4000 x
11 x 11), one frequency per cutout, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.
R `cubes.amplitude_images(frequency, nterms=1)` and R3 the same with `nterms=3`, images on the host at the end; D
`cubes.difference_images(...)` of the same cubes, the other kernel family with this chunking (it reads the rows of the in- and
out-of-transit cadences of two cubes; the floor of R is two reads of every row of the flux cube); H the host route: `to_host()`, then `PixelCube.amplitude_image` per cutout on 16 threads.  Every
timed region ends with a synchronise.  Written to profiles/ampimage_walls.txt.

`psfphot`: deblended PSF photometry of the same batch shape with `LK_WALLS_STARS` (default 4) stars per cutout, in ONE process, the
routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  R `cubes.psf_photometry(star_col, star_row, sigma)`, Rs
the same with resident shifts, everything left in HBM; H / Hs the host route: `PixelCube.psf_photometry` per cutout on 16
threads over the first `LK_WALLS_MIRROR_B` (default 16) cutouts, scaled to the batch in the ratios.  Every timed region ends with
a synchronise.  Written to profiles/psfphot_walls.txt.  `psfphot_trace`: R and Rs twice and nothing else, for `rocprofv3
--kernel-trace --stats` (profiles/psfphot_kernel_stats.txt).

`psffit`: the PSF fit with a pointing shift per cadence on the same batch shape and star count, the cubes rendered with true
shifts uniform in +-0.3 px, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  F
`cubes.psf_fit(star_col, star_row, sigma)` with the defaults; Rs `cubes.psf_photometry` of the same cubes at the true shifts
(resident); H the mirror `PixelCube.psf_fit` per cutout on 16 threads over the first `LK_WALLS_MIRROR_B` (default 16) cutouts.
Every timed region ends with a synchronise.  Written to profiles/psffit_walls.txt.  `psffit_trace`: F and Rs twice and nothing
else, for `rocprofv3 --kernel-trace --stats` (profiles/psffit_kernel_stats.txt).

`psfwidth`: the fit of the PSF width per cutout on the same batch shape and star count, the cubes rendered with true shifts uniform
in +-0.3 px (given to the fit) and a true width of 1.1 px, `sigma0` 15 % off (1.15 x the truth in columns, 0.85 x in rows), in ONE
process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  W `cubes.psf_width(star_col, star_row,
sigma0, shifts=)` with the defaults; Wm the same with a `cadence_mask` that selects every tenth cadence; Rs
`cubes.psf_photometry` of the same cubes at the same shifts (one evaluation pass should cost about one such call); H the mirror
`PixelCube.psf_width` per cutout on 16 threads over the first `LK_WALLS_MIRROR_B` (default 16) cutouts.  Every timed region ends
with a synchronise.  Written to profiles/psfwidth_walls.txt.  `psfwidth_trace`: W, Wm, Wb and Rs twice and nothing else, for `rocprofv3
--kernel-trace --stats` (profiles/psfwidth_kernel_stats.txt).

`psfpos`: the fit of the stars' positions per cutout on the same batch shape and star count, the cubes rendered at the true positions
with true shifts uniform in +-0.3 px (given to the fit as `DeviceBuffer`s) and the true width 1.1 px (given), the starts 0.2 px off
per star and axis with either sign, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  P
`cubes.psf_positions(star_col, star_row, sigma, shifts=)` with the defaults; W `cubes.psf_width` and Rs `cubes.psf_photometry` of
the same cubes at the same shifts and the same (offset) positions; H the mirror `PixelCube.psf_positions` per cutout on 16 threads
over the first `LK_WALLS_MIRROR_B` (default 16) cutouts, scaled to the batch in the report.  Every timed region ends with a
synchronise.  Written to profiles/psfpos_walls.txt.  `psfpos_trace`: P and W twice and nothing else, for `rocprofv3 --kernel-trace
--stats` (profiles/psfpos_kernel_stats.txt).

`prfphot`: PSF photometry with a tabulated PRF on the same batch shape and star count, the cubes rendered by the Gaussian of width
1.1 px with true shifts uniform in +-0.3 px, the table `TabulatedPRF.from_gaussian(1.1, 1.1, 50, 5.5)` (os = 50, 551 x 551), in ONE
process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  P `cubes.psf_photometry(star_col, star_row,
prf=)`, Ps the same with resident shifts; G / Gs `cubes.psf_photometry(star_col, star_row, sigma)` of the same cubes, the yardstick;
H / Hs the mirror `PixelCube.psf_photometry(prf=)` per cutout on 16 threads over the first `LK_WALLS_MIRROR_B` (default 16) cutouts,
scaled to the batch in the report.  Every timed region ends with a synchronise.  Written to profiles/prfphot_walls.txt.
`prfphot_trace`: P and Ps twice and nothing else, for `rocprofv3 --kernel-trace --stats` (profiles/prfphot_kernel_stats.txt).

`prffit`: the PSF fit with a pointing shift per cadence and a tabulated PRF on the same batch shape, star count, cubes and table as
`prfphot`, in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  F `cubes.psf_fit(star_col,
star_row, prf=)` with the defaults, from shifts 0; Ps `cubes.psf_photometry(prf=)` of the same cubes GIVEN the true shifts; Fg
`cubes.psf_fit(star_col, star_row, sigma)`, the Gaussian fit; H the mirror `PixelCube.psf_fit(prf=)` per cutout on 16 threads over the
first `LK_WALLS_MIRROR_B` (default 16) cutouts, scaled to the batch in the report.  Every timed region ends with a synchronise.
Written to profiles/prffit_walls.txt.  `prffit_trace`: F and Ps twice and nothing else, for `rocprofv3 --kernel-trace --stats`
(profiles/prffit_kernel_stats.txt).

`background`: the per-cadence background of the same batch shape with 'background' masks, in ONE process, the routes alternating,
`LK_WALLS_REPS` (default 5) times after one warm-up.  F `cubes.subtract_background()` (median images, masks, the fused estimate +
subtraction) and Fm the same with the masks given; E `cubes.estimate_background()`, Em with the masks given, Es with the scatter
too; S `cubes.subtract_background(background=DeviceBuffer)`, the streaming subtraction alone; H the host route: `to_host()`,
`PixelCube.subtract_background` per cutout on 16 threads, `from_cubes`.  Every timed region ends with a synchronise.  Written to
profiles/background_walls.txt.

`pixelpg`: the per-pixel Lomb-Scargle periodograms of the same batch shape on one grid of `LK_WALLS_F` (default 2000) frequencies,
in ONE process, the routes alternating, `LK_WALLS_REPS` (default 5) times after one warm-up.  R
`cubes.pixel_periodograms(grid, to_host=False)`, the power cube resident; P the same with `return_power=False`; L the route
without the kernel: `to_host()`, the host transpose into B x npix light curves, `DeviceLightCurveBatch.from_arrays`, then
`to_periodogram_power(grid, ls_method="slow", to_host=False)`; H the mirror `PixelCube.pixel_periodogram` on 16 threads for the
first `LK_WALLS_MIRROR_B` (default 16) cutouts only (a cutout takes seconds), scaled to the batch in the report.  Every timed
region ends with a synchronise.  Written to profiles/pixelpg_walls.txt.  `pixelpg_trace`: R and P once each after a warm-up, for a
`rocprofv3 --kernel-trace --stats` run of its own (profiles/pixelpg_kernel_stats.txt)."""
import cProfile
import io
import os
import pstats
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(fn, reps=3, profile=True):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    txt = ""
    if profile:
        pr = cProfile.Profile()
        pr.enable()
        fn()
        pr.disable()
        s = io.StringIO()
        pstats.Stats(pr, stream=s).sort_stats("cumulative").print_stats(14)
        txt = "\n".join(l for l in s.getvalue().splitlines() if l.strip() and "function calls" not in l and "Ordered by" not in l)
    return 1e3 * float(np.median(ts)), txt


def pld_cubes(B, distinct=100):
    """B K2-like cutouts of 3500 x 11 x 11 (the first `distinct` synthetic ones, repeated: the walls do not depend on the
    pixels' values, and 500 distinct cutouts take a minute of host time to draw)."""
    from lightkurve_amd import synth
    from lightkurve_amd.correctors.pldcorrector import PixelCube
    base = []
    for i in range(min(B, distinct)):
        t, flux, err, _ = synth.pld_cutout(4, i, n=3500, npix=11)
        base.append(PixelCube(t, flux, err, mission="K2"))
    return [base[i % len(base)] for i in range(B)]


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    return "%8.2f ms (min %.2f, max %.2f, n=%d)" % (float(np.median(ts)), ts.min(), ts.max(), len(ts))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def pld_dev(which):
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors.pldcorrector import pld_correct_batch
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    kw = dict(pld_order=3, pca_components=16)
    sync = _capi.Handle.get(0).synchronize
    if "pld_dev_trace" in which:
        from lightkurve_amd.device import DevicePixelCubeBatch
        B = int(os.environ.get("LK_WALLS_B", "500"))
        batch = DevicePixelCubeBatch.from_cubes(pld_cubes(B))
        calls = 1 + reps
        for _ in range(calls):
            batch.pld_correct(**kw)
        sync()
        print("pld_dev_trace: %d resident pld_correct calls on %d cutouts x 3500 x 11 x 11 (order 3, 16 components)" % (calls, B))
        return
    resident = "pld_dev" in which
    if resident:
        from lightkurve_amd.device import DevicePixelCubeBatch
    for B in (int(v) for v in os.environ.get("LK_WALLS_SIZES", "100,500").split(",")):
        cubes = pld_cubes(B)
        A, U, R, R2 = [], [], [], []
        ref = pld_correct_batch(cubes, **kw)                       # warm-up of this shape, both paths
        if resident:
            batch = DevicePixelCubeBatch.from_cubes(cubes)
            got = batch.pld_correct(**kw)
            batch.pld_correct(to_host=False, **kw)[0].synchronize()
            same = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
        for _ in range(reps):
            A.append(timed(lambda: (pld_correct_batch(cubes, **kw), sync()))[0])
            if not resident:
                continue
            dt, batch = timed(lambda: DevicePixelCubeBatch.from_cubes(cubes))      # (from_cubes ends in a synchronise)
            U.append(dt)
            R.append(timed(lambda: (batch.pld_correct(**kw), sync()))[0])
            R2.append(timed(lambda: batch.pld_correct(to_host=False, **kw)[0].synchronize())[0])
        print("PLD, %d cutouts x 3500 x 11 x 11, order 3, 16 components, all pixels" % B)
        print("  A  pld_correct_batch(list of PixelCube)            %s" % spread(A))
        if resident:
            print("  U  DevicePixelCubeBatch.from_cubes (once per batch) %s" % spread(U))
            print("  R  batch.pld_correct() -> host arrays              %s" % spread(R))
            print("  R' batch.pld_correct(to_host=False) + synchronise  %s" % spread(R2))
            print("  resident result == pld_correct_batch result: %s; R / A = %.3f" % (same, np.median(R) / np.median(A)))
        sys.stdout.flush()


def pld_ragged():
    from lightkurve_amd import _capi, synth
    from lightkurve_amd.correctors.pldcorrector import PixelCube
    from lightkurve_amd.device import DevicePixelCubeBatch
    reps = int(os.environ.get("LK_WALLS_REPS", "7"))
    B = int(os.environ.get("LK_WALLS_B", "500"))
    sync = _capi.Handle.get(0).synchronize
    base = []
    for i, amp in enumerate((0, 30, 100, 300, 1000)):      # a static pattern of growing amplitude shrinks the threshold mask
        t, flux, err, _ = synth.pld_cutout(4, 20 + i, n=3500, npix=11)
        pattern = (amp * np.abs(np.random.default_rng(100 + i).standard_normal((11, 11)))).astype(np.float32)
        base.append(PixelCube(t, (flux + pattern).astype(np.float32), err, mission="K2"))
    counts = [int(c.create_threshold_mask(3).sum()) for c in base]
    bcounts = [int((~c.create_threshold_mask(0, None)).sum()) for c in base]
    G = len(base)
    batch = DevicePixelCubeBatch.from_cubes([base[i % G] for i in range(B)])
    groups = [DevicePixelCubeBatch.from_cubes([base[g]] * len(range(g, B, G))) for g in range(G)]
    k2 = dict(aperture_mask=None, pld_aperture_mask="threshold", background_aperture_mask="background", pld_order=3, pca_components=16)
    fns = {"R": lambda: batch.pld_correct(ragged_masks=True, **k2),
           "U": lambda: batch.pld_correct(pld_order=3, pca_components=16),
           "G": lambda: [g.pld_correct(**k2) for g in groups]}
    for _ in range(2):                                     # warm-up of every shape the timed window uses
        for fn in fns.values():
            fn()
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    r, gl = fns["R"](), fns["G"]()
    worst, masks = 0.0, True
    for g in range(G):
        rows = np.arange(g, B, G)
        masks = masks and bool(np.array_equal(r[1][rows], gl[g][1]))
        worst = max(worst, float(np.max(np.abs(r[0][rows] - gl[g][0]) / np.median(gl[g][0], axis=1)[:, None])))
    print("PLD, %d cutouts x 3500 x 11 x 11, order 3, 16 components; threshold masks of %s pixels, background masks of %s, cycled"
          % (B, counts, bcounts))
    print("  R  ragged call (K2 default masks, ragged_masks=True)        %s" % spread(ts["R"]))
    print("  U  uniform call, every pixel in both masks                  %s" % spread(ts["U"]))
    print("  G  one call per group of equal mask size (%d groups)         %s" % (G, spread(ts["G"])))
    print("  R / U = %.3f, R / G = %.3f; R against G: outlier masks equal %s, max |delta| / median %.3e"
          % (np.median(ts["R"]) / np.median(ts["U"]), np.median(ts["R"]) / np.median(ts["G"]), masks, worst))
    sys.stdout.flush()


def underfit(which):
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors import metrics
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, N, M = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_M", "50")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    rng = np.random.default_rng(7)
    t = np.linspace(0, 27, N)
    S = np.column_stack([np.sin(2 * np.pi * t / 13.7), (t / 27 - 0.5) ** 2])
    y = 1000.0 * rng.uniform(0.5, 2, (B, 1)) * (1 + rng.normal(0, 0.01, (B, 2)) @ S.T + 1e-3 * rng.normal(0, 1, (B, N)))
    cm = rng.random(N) > 0.1
    nb = metrics.nearest_neighbors(rng.uniform(0, 1, B), rng.uniform(0, 1, B), M)
    M = nb.shape[1]
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), y.reshape(-1), (1e-3 * y).reshape(-1), np.arange(B + 1) * N).remove_nans()
    cor = raw.cbv_correct(S, cbv_indices=[1, 2], cadence_mask=np.broadcast_to(cm, (B, N)))[0]
    cor.synchronize()
    sync = _capi.Handle.get(0).synchronize
    n = int(cm.sum())
    pitch = -(-n // 128) * 128
    model = "pair pass reads %.2f GB of z rows (B M pitch 8), scratch %.1f MB" % (B * M * pitch * 8 / 1e9, (B * pitch * 8 + B * 8) / 1e6)
    if "underfit_trace" in which:
        calls = 1 + max(reps, 5)
        for _ in range(calls):
            cor.under_fitting_metric(nb, cadence_mask=cm, to_host=False)
        sync()
        print("underfit_trace: %d resident under_fitting_metric calls on %d x %d, M = %d, %d kept cadences; per call the %s"
              % (calls, B, N, M, n, model))
        return

    def host_route():
        flux = cor.flux_host().reshape(B, N)
        z = flux[:, cm] / np.median(flux[:, cm], axis=1)[:, None] - 1.0
        tk = t[cm]
        with ThreadPoolExecutor(max_workers=16) as ex:
            return np.array(list(ex.map(lambda b: metrics.underfit_metric_neighbors(LightCurve(tk, flux[b, cm]), z[nb[b]].T), range(B))))

    got = cor.under_fitting_metric(nb, cadence_mask=cm)                     # warm-up of both routes
    cor.under_fitting_metric(nb, cadence_mask=cm, to_host=False)
    sync()
    ref = host_route()
    R, R2, H = [], [], []
    for _ in range(reps):
        R.append(timed(lambda: cor.under_fitting_metric(nb, cadence_mask=cm))[0])          # (the download synchronises)
        R2.append(timed(lambda: (cor.under_fitting_metric(nb, cadence_mask=cm, to_host=False), sync()))[0])
        H.append(timed(host_route)[0])
    print("under-fitting metric, %d cotrended targets x %d cadences (%d kept), %d neighbours each; %s" % (B, N, n, M, model))
    print("  R  batch.under_fitting_metric() -> metric[B] on the host        %s" % spread(R))
    print("  R' the same, to_host=False + synchronise                        %s" % spread(R2))
    print("  H  download + underfit_metric_neighbors per target, 16 threads  %s" % spread(H))
    print("  max |R - H| = %.3e; metric min %.4f median %.4f; H / R = %.0f"
          % (float(np.max(np.abs(got - ref))), got.min(), float(np.median(got)), np.median(H) / np.median(R)))
    sys.stdout.flush()


def overfit(which):
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors import metrics
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, N, ns = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_SAMPLES", "10")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    rng = np.random.default_rng(7)
    t = np.linspace(0, 27, N)
    S = np.column_stack([np.sin(2 * np.pi * t / 13.7), (t / 27 - 0.5) ** 2])
    y = 1000.0 * rng.uniform(0.5, 2, (B, 1)) * (1 + rng.normal(0, 0.01, (B, 2)) @ S.T + 1e-3 * rng.normal(0, 1, (B, N)))
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), y.reshape(-1), (1e-3 * y).reshape(-1), np.arange(B + 1) * N).remove_nans()
    cor = raw.cbv_correct(S, cbv_indices=[1, 2])[0]
    cor.synchronize()
    sync = _capi.Handle.get(0).synchronize
    M = len(_capi.overfit_default_grid(t))
    nbytes, per_round = _capi.overfit_scratch_bytes(B, N, M, ns)
    model = "%d frequencies, scratch %.2f GB in rounds of %d samples, %d LS passes of %d rows" % (M, nbytes / 1e9, per_round, 2 + ns, B)
    if "overfit_trace" in which:
        calls = 1 + max(reps, 3)
        for _ in range(calls):
            cor.over_fitting_metric(raw, n_samples=ns, to_host=False)
        sync()
        print("overfit_trace: %d resident over_fitting_metric calls on %d x %d, n_samples = %d; per call %s" % (calls, B, N, ns, model))
        return

    def host_route():
        f0, f1, e1 = raw.flux_host().reshape(B, N), cor.flux_host().reshape(B, N), cor.flux_err_host().reshape(B, N)
        return np.array([metrics.overfit_metric_lombscargle(LightCurve(t, f0[b], e1[b]), LightCurve(t, f1[b], e1[b]), n_samples=ns)
                         for b in range(B)])

    got = cor.over_fitting_metric(raw, n_samples=ns)                       # warm-up of both routes
    cor.over_fitting_metric(raw, n_samples=ns, to_host=False)
    sync()
    ref = host_route()
    R, R2, H = [], [], []
    for _ in range(reps):
        R.append(timed(lambda: cor.over_fitting_metric(raw, n_samples=ns))[0])            # (the download synchronises)
        R2.append(timed(lambda: (cor.over_fitting_metric(raw, n_samples=ns, to_host=False), sync()))[0])
        H.append(timed(host_route)[0])
    print("over-fitting metric, %d cotrended targets x %d cadences, n_samples = %d; %s" % (B, N, ns, model))
    print("  R  corrected.over_fitting_metric(batch) -> metric[B] on the host        %s" % spread(R))
    print("  R' the same, to_host=False + synchronise                                %s" % spread(R2))
    print("  H  download both + overfit_metric_lombscargle per target, sequential    %s" % spread(H))
    print("  median metric R %.4f, H %.4f (different noise: equal in distribution); max |R - H| = %.3e; H / R = %.0f"
          % (float(np.median(got)), float(np.median(ref)), float(np.max(np.abs(got - ref))), np.median(H) / np.median(R)))
    sys.stdout.flush()


def cbvopt(which):
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors import metrics
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N, K, M = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_K", "16"),
                                                         ("LK_WALLS_M", "50")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    rng = np.random.default_rng(7)
    t = np.linspace(0, 27, N)
    x = t / 27 - 0.5
    S = np.column_stack([np.sin(2 * np.pi * t / p) for p in np.linspace(3.1, 41.0, K - 1)] + [x ** 2])
    amp = rng.normal(0, 0.01, (B, K)) * (np.arange(K) < 4)          # four vectors carry systematics, the rest can only over-fit
    y = 1000.0 * rng.uniform(0.5, 2, (B, 1)) * (1 + amp @ S.T + 1e-3 * rng.normal(0, 1, (B, N)))
    nb = metrics.nearest_neighbors(rng.uniform(0, 1, B), rng.uniform(0, 1, B), M)
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), y.reshape(-1), (1e-3 * y).reshape(-1), np.arange(B + 1) * N).remove_nans()
    raw.synchronize()
    sync = _capi.Handle.get(0).synchronize
    kw = dict(neighbors=nb, cbv_indices=np.arange(1, K + 1))
    shape = "%d targets x %d cadences, %d basis vectors + constant, %d neighbours, bounds (1e-4, 1e4)" % (B, N, K, nb.shape[1])
    if "cbvopt_trace" in which:
        iters = int(os.environ.get("LK_WALLS_ITERS", "6"))
        _out, info = raw.cbv_correct_optimized(S, max_iter=iters, **kw)
        sync()
        print("cbvopt_trace: one search cut at %d evaluations (status %s) on %s" % (iters, sorted(set(info["status"].tolist())), shape))
        return
    _out, info = raw.cbv_correct_optimized(S, **kw)                          # warm-up; the search is deterministic
    steps = int(info["nfev"].max())
    alphas = np.logspace(-4, 4, steps)
    raw.cbv_goodness_scan(S, alphas[:2], neighbors=nb, cbv_indices=np.arange(1, K + 1), n_samples=1)
    sync()
    O, Sc = [], []
    for _ in range(reps):
        O.append(timed(lambda: (raw.cbv_correct_optimized(S, **kw), sync()))[0])
        Sc.append(timed(lambda: (raw.cbv_goodness_scan(S, alphas, neighbors=nb, cbv_indices=np.arange(1, K + 1), n_samples=1), sync()))[0])
    print("per-target ridge search, %s" % shape)
    print("  evaluations per target: min %d median %d max %d (= lockstep evaluations); status counts %s"
          % (info["nfev"].min(), int(np.median(info["nfev"])), steps, np.bincount(info["status"], minlength=3).tolist()))
    print("  alpha: min %.3g median %.3g max %.3g; over-fitting score median %.4f, under-fitting score median %.4f"
          % (info["alpha"].min(), float(np.median(info["alpha"])), info["alpha"].max(), float(np.median(info["over_fitting_score"])),
             float(np.median(info["under_fitting_score"]))))
    print("  O  batch.cbv_correct_optimized(), the whole call                  %s" % spread(O))
    print("  S  batch.cbv_goodness_scan(%d penalties, n_samples=1)             %s" % (steps, spread(Sc)))
    print("  O per lockstep evaluation %.2f ms, S per penalty %.2f ms; S / O = %.2f"
          % (1e3 * np.median(O) / steps, 1e3 * np.median(Sc) / steps, np.median(Sc) / np.median(O)))
    sys.stdout.flush()


def blsstats():
    from lightkurve_amd import _capi, synth
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.periodogram import bls_compute_stats_host
    B, N, nP = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_P", "256")))
    cols = [synth.bls_target(3, i, N)[:3] for i in range(B)]
    n_off = np.arange(B + 1, dtype=np.int64) * N
    raw = DeviceLightCurveBatch.from_arrays(*(np.concatenate([c[k] for c in cols]) for k in range(3)), n_off)
    periods = 1.0 / np.linspace(1 / 13.0, 1 / 0.6, nP)[::-1]
    res = raw.bls(periods, duration=[0.05, 0.1, 0.2])
    pk = res.peaks()
    sync = _capi.Handle.get(0).synchronize
    sync()
    src = res._batch

    def host_route():
        t, y = src.time_host(), src.flux_host()
        w = res.d_ivar.download(np.float64, src.n_cadences, stream=src.stream)
        out = []
        for b in range(B):
            a, z = int(src.n_off[b]), int(src.n_off[b + 1])
            out.append(bls_compute_stats_host(t[a:z], y[a:z], w[a:z], pk["period"][b], pk["duration"][b], pk["transit_time"][b]))
        return out

    r_ms, r_prof = wall(lambda: (res.compute_stats(), sync()))
    h_ms, h_prof = wall(host_route)
    print("BLS vetting statistics after a resident search, %d targets x %d cadences (search: %d periods x 3 durations, not timed)"
          % (B, N, nP))
    print("  R  result.compute_stats(), resident tail                              %10.1f ms per call" % r_ms)
    print("  H  download 3 columns + bls_compute_stats_host per target             %10.1f ms per call" % h_ms)
    print("  H / R = %.1f\n%s\n%s\n" % (h_ms / r_ms, r_prof, h_prof))
    sys.stdout.flush()


def clean_field():
    """(resident batch of B x N with transits, noise and 0.5 % up-going outliers, B, N)."""
    from lightkurve_amd import synth
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000")))
    rng = np.random.default_rng(11)
    cols = [synth.bls_target(3, i, N)[:3] for i in range(B)]
    t, f, e = (np.concatenate([c[k] for c in cols]) for k in range(3))
    f = f + np.where(rng.random(f.size) < 0.005, 8.0 * np.median(e), 0.0)
    return DeviceLightCurveBatch.from_arrays(t, f, e, np.arange(B + 1, dtype=np.int64) * N), B, N


def clean():
    from lightkurve_amd import _capi
    from lightkurve_amd.device import DeviceLightCurveBatch
    from oracle import np_oracle as O
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    M, nP = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_M", "4096"), ("LK_WALLS_P", "64")))
    raw, B, N = clean_field()
    sync = _capi.Handle.get(0).synchronize
    freq = 0.02 + 0.002 * np.arange(M)
    periods = 1.0 / np.linspace(1 / 13.0, 1 / 0.6, nP)[::-1]
    durations = [0.05, 0.1, 0.2]

    def without(batch, mask):
        """``batch`` without the cadences of ``mask`` (host bool), through the host."""
        host = batch.to_host()
        keep = ~mask
        off = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[host.n_off]
        return DeviceLightCurveBatch.from_arrays(host.time[keep], host.flux[keep], host.flux_err[keep], off)

    def chain():
        return raw.normalize().flatten(401).remove_outliers().to_periodogram_peaks(freq)

    def chain_host():
        flat = raw.normalize().flatten(401)
        flux, off = flat.flux_host(), flat.n_off
        with np.errstate(all="ignore"):
            mask = np.concatenate([O.sigma_clip_mask(flux[off[b]:off[b + 1]]) for b in range(B)])
        return without(flat, mask).to_periodogram_peaks(freq)

    flat = raw.normalize().flatten(401)
    flat.synchronize()

    def search():
        return flat.bls_search(periods, n_signals=2, duration=durations)

    def search_host():
        cur, signals = flat, []
        for _ in range(2):
            res = cur.bls(periods, duration=durations)
            pk = res.peaks()
            signals.append(pk)
            cur = without(res._batch, res.transit_mask(pk["period"], pk["duration"], pk["transit_time"]))
        return signals, cur

    fns = {"C": chain, "C_H": chain_host, "S": search, "S_H": search_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    same_c = bool(np.array_equal(first["C"], first["C_H"]))
    same_s = all(np.array_equal(a[k], b[k]) for a, b in zip(first["S"][0], first["S_H"][0]) for k in a) and bool(
        np.array_equal(first["S"][1].flux_host(), first["S_H"][1].flux_host()))
    print("transit-search front, %d targets x %d cadences (%.0f MB per float64 column)" % (B, N, B * N * 8 / 1e6))
    print("  C    normalize().flatten(401).remove_outliers().to_periodogram_peaks(%d frequencies)   %s" % (M, spread(ts["C"])))
    print("  C_H  the same, the clip through the host (to_host, numpy per target, from_arrays)       %s" % spread(ts["C_H"]))
    print("  S    flattened.bls_search(%d periods x 3 durations, n_signals=2)                        %s" % (nP, spread(ts["S"])))
    print("  S_H  the same loop, to_host / numpy ~mask / from_arrays between the rounds               %s" % spread(ts["S_H"]))
    print("  C == C_H: %s; S == S_H: %s; C_H / C = %.2f; S_H / S = %.2f"
          % (same_c, same_s, np.median(ts["C_H"]) / np.median(ts["C"]), np.median(ts["S_H"]) / np.median(ts["S"])))
    sys.stdout.flush()


def cdpp():
    from lightkurve_amd import _capi
    from lightkurve_amd.lightcurve import estimate_cdpp_batch
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    raw, B, N = clean_field()
    sync = _capi.Handle.get(0).synchronize

    def host_route():
        return estimate_cdpp_batch(raw.to_host().to_lightcurves())

    got, ref = raw.estimate_cdpp(), host_route()                          # warm-up of both routes
    sync()
    R, H = [], []
    for _ in range(reps):
        R.append(timed(lambda: raw.estimate_cdpp())[0])                    # (the download synchronises)
        H.append(timed(host_route)[0])
    print("estimate_cdpp, %d targets x %d cadences" % (B, N))
    print("  R  batch.estimate_cdpp() -> cdpp[B] on the host                               %s" % spread(R))
    print("  H  to_host() + estimate_cdpp_batch(list of light curves)                      %s" % spread(H))
    print("  max |R - H| / H = %.3e; median CDPP %.1f ppm; H / R = %.1f"
          % (float(np.max(np.abs(got - ref) / ref)), float(np.median(got)), np.median(H) / np.median(R)))
    sys.stdout.flush()


def prewhiten():
    from lightkurve_amd import _capi, synth
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.periodogram import ls_model_host
    B, N, M = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_M", "100000")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    cols = [synth.ls_target(1, i, N)[:3] for i in range(B)]
    n_off = np.arange(B + 1, dtype=np.int64) * N
    raw = DeviceLightCurveBatch.from_arrays(np.concatenate([c[0] for c in cols]), 1.0 + np.concatenate([c[1] for c in cols]),
                                            np.concatenate([c[2] for c in cols]), n_off).remove_nans()
    freq = synth.ls_frequency_grid(M)
    sync = _capi.Handle.get(0).synchronize

    def resident():
        return raw.prewhiten(freq, n_signals=3)

    def through_host():
        cur, signals = raw, []
        for _ in range(3):
            _pow, peaks = cur.to_periodogram_power(freq, to_host=False, want_peaks=True)
            f = freq[peaks[:, 1].astype(np.int64)]
            host = cur.to_host()
            flux, theta = host.flux.copy(), np.empty((B, 3))
            for b in range(B):
                a, z = int(host.n_off[b]), int(host.n_off[b + 1])
                m = ls_model_host(host.time[a:z], host.flux[a:z], None, f[b])
                flux[a:z] -= m["model"] - (m["y_mean"] + m["theta"][0])
                theta[b] = m["theta"]
            signals.append(dict(frequency=f, theta=theta, power=peaks[:, 0]))
            cur = DeviceLightCurveBatch.from_arrays(host.time, flux, host.flux_err, host.n_off)
            cur.nan_free = True
        return signals, cur

    def ls_pass():
        return raw.to_periodogram_power(freq, to_host=False, want_peaks=True)

    peaks = ls_pass()[1]
    f_peak = freq[peaks[:, 1].astype(np.int64)]

    def fit():
        return raw.ls_model(f_peak, want_model=False, want_residual=True)

    fns = {"W": resident, "W_H": through_host, "L": ls_pass, "F": fit}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    (sig_w, res_w), (sig_h, res_h) = first["W"], first["W_H"]
    same_f = all(np.array_equal(a["frequency"], b["frequency"]) for a, b in zip(sig_w, sig_h))
    d_theta = max(float(np.max(np.abs(a["theta"] - b["theta"]))) for a, b in zip(sig_w, sig_h))
    d_res = float(np.max(np.abs(res_w.flux_host() - res_h.flux_host())))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    print("prewhitening, %d targets x %d cadences (%.0f MB per float64 column), %d frequencies, n_signals = 3"
          % (B, N, B * N * 8 / 1e6, M))
    print("  W    batch.prewhiten(frequency, n_signals=3), resident                                  %s" % spread(ts["W"]))
    print("  W_H  the same loop, to_host / ls_model_host per target / from_arrays between the rounds   %s" % spread(ts["W_H"]))
    print("  L    one round's periodogram pass: to_periodogram_power(to_host=False, want_peaks=True)   %s" % spread(ts["L"]))
    print("  F    one round's fit: ls_model(want_model=False, want_residual=True)                      %s" % spread(ts["F"]))
    print("  same frequencies: %s; max |theta W - W_H| = %.3e; max |residual W - W_H| = %.3e" % (same_f, d_theta, d_res))
    print("  W_H / W = %.1f; W per round / L = %.2f; F / L = %.3f" % (med["W_H"] / med["W"], med["W"] / 3 / med["L"], med["F"] / med["L"]))
    sys.stdout.flush()


def seismology():
    from lightkurve_amd import _capi
    from lightkurve_amd import seismology as seis
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.periodogram import Periodogram
    B, N = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    rng = np.random.default_rng(11)
    t = np.arange(N) * (2.0 / 1440.0)
    fs = 1e6 / 86400.0 / (t[-1] - t[0])                      # microhertz: oversample_factor = 1
    M = int(1e6 / 240.0 / fs)                                # up to the Nyquist frequency of two-minute cadences
    freq = fs * np.arange(1, M + 1)
    flux = np.empty((B, N))
    for b in range(B):
        numax = rng.uniform(800.0, 3000.0)
        dnu = 0.294 * numax ** 0.772
        y = 1.0 + 2e-4 * rng.standard_normal(N)
        for n in range(-4, 5):
            y += 1e-4 * np.exp(-0.5 * (n / 2.5) ** 2) * np.sin(2 * np.pi * (numax + n * dnu) * 0.0864 * t + rng.uniform(0, 6.28))
        flux[b] = y
    n_off = np.arange(B + 1, dtype=np.int64) * N
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), flux.ravel(), None, n_off).remove_nans()
    sync = _capi.Handle.get(0).synchronize

    def resident():
        return raw.to_periodogram(freq, normalization="psd").estimate_seismology()

    def through_host():
        power = raw.to_periodogram_power(freq, normalization="psd", to_host=True)
        numax, deltanu = np.empty(B), np.full(B, np.nan)
        for b in range(B):
            snr = Periodogram(freq, power[b], frequency_unit="uHz").flatten()
            numax[b] = seis.estimate_numax_acf2d(snr)["numax"]
            try:
                deltanu[b] = seis.estimate_deltanu_acf2d(snr, numax[b])["deltanu"]
            except ValueError:                              # no peak in the selection: the resident route's status 3
                pass
        return dict(numax=numax, deltanu=deltanu)

    def ls_pass():
        return raw.to_periodogram_power(freq, normalization="psd", to_host=False)

    fns = {"S": resident, "S_H": through_host, "L": ls_pass}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    r, hst = first["S"], first["S_H"]
    med = {k: float(np.median(v)) for k, v in ts.items()}
    print("seismology chain, %d targets x %d two-minute cadences, %d frequencies of %.3f uHz (oversample_factor 1)" % (B, N, M, fs))
    print("  S    batch.to_periodogram(f, 'psd').estimate_seismology(), resident                         %s" % spread(ts["S"]))
    print("  S_H  to_periodogram_power(to_host=True), then per target flatten / numax / deltanu          %s" % spread(ts["S_H"]))
    print("  L    the periodogram pass alone: to_periodogram_power(to_host=False)                        %s" % spread(ts["L"]))
    print("  same numax: %s; same deltanu: %s; status counts 0..3: %s"
          % (np.array_equal(r["numax"], hst["numax"]), np.array_equal(r["deltanu"], hst["deltanu"], equal_nan=True),
             np.bincount(r["status"], minlength=4).tolist()))
    print("  S_H / S = %.1f; (S - L) = %.2f ms for flatten, numax and deltanu" % (med["S_H"] / med["S"], 1e3 * (med["S"] - med["L"])))
    sys.stdout.flush()


def sff():
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors import SFFCorrector, sff_window_points
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, N = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "3500")))
    reps, windows = int(os.environ.get("LK_WALLS_REPS", "2")), 20
    rng = np.random.default_rng(17)
    i = np.arange(N)
    t = 2000.0 + 0.0204 * i
    roll = (i % 12) / 12.0
    col = 10.3 + roll[None] * 0.8 + 2e-5 * i[None] + 1e-3 * rng.standard_normal((B, N))
    row = 20.7 + roll[None] * 0.55 + 1e-5 * i[None] + 1e-3 * rng.standard_normal((B, N))
    flux = 1000.0 * (1.0 + 0.003 * np.sin(2 * np.pi * (t - t[0]) / rng.uniform(4.0, 9.0, (B, 1))) + 0.006 * (roll[None] - 0.4) ** 2
                     + 3e-4 * rng.standard_normal((B, N)))
    err = np.full((B, N), 0.3)
    n_off = np.arange(B + 1, dtype=np.int64) * N
    wp = sff_window_points(N, windows, thrusters=np.arange(11, N, 12))        # the same windows for both routes, chosen once
    wps = [wp] * B
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), flux.ravel(), err.ravel(), n_off)
    raw.nan_free = True
    d_col, d_row = raw._centroid_buffer(col, "centroid_col"), raw._centroid_buffer(row, "centroid_row")
    sync = _capi.Handle.get(0).synchronize

    def resident():
        return raw.sff_correct(d_col, d_row, windows=windows, window_points=wps, diagnostics=False)["lc"]

    def through_host():
        host = raw.to_host()
        c, r = d_col.download(np.float64, B * N), d_row.download(np.float64, B * N)
        out = np.empty(B * N)
        for b in range(B):
            a, z = int(host.n_off[b]), int(host.n_off[b + 1])
            lc = LightCurve(time=host.time[a:z], flux=host.flux[a:z], flux_err=host.flux_err[a:z])
            out[a:z] = SFFCorrector(lc).correct(c[a:z], r[a:z], windows=windows, window_points=wp).flux
        return DeviceLightCurveBatch.from_arrays(host.time, out, host.flux_err, host.n_off)

    fns = {"R": resident, "H": through_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    same = np.array_equal(first["R"].flux_host(), first["H"].flux_host())
    K = int((t[-1] - t[0]) / 1.5) + (len(wp) + 1) * 8
    nbytes, chunks = _capi.sff_scratch_bytes(n_off, np.full(B, int((t[-1] - t[0]) / 1.5), np.int32),
                                             np.arange(B + 1, dtype=np.int32) * len(wp), 5, 3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    lines = ["SFF correction, %d targets x %d cadences, windows = %d (%d window points), bins = 5: K = %d columns per target, "
             "design matrices %.2f GB in %d chunk(s) of a %.2f GB scratch block" % (B, N, windows, len(wp), K, B * N * K * 8 / 1e9,
                                                                                  chunks, nbytes / 1e9),
             "  R    batch.sff_correct(d_col, d_row, window_points=...), resident                         %s" % spread(ts["R"]),
             "  H    to_host(), SFFCorrector(lc).correct(...) per target, from_arrays                      %s" % spread(ts["H"]),
             "  same corrected flux, bit for bit: %s" % same,
             "  H / R = %.1f" % (med["H"] / med["R"])]
    print("\n".join(lines))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sff_walls.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.stdout.flush()


def cbvragged():
    from lightkurve_amd import _capi, batch
    from lightkurve_amd.correctors import DesignMatrix
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, N, K = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_K", "17")))
    reps, alpha = int(os.environ.get("LK_WALLS_REPS", "2")), 1e-4
    rng = np.random.default_rng(23)
    t = np.linspace(0.0, 27.0, N)
    cbvs = np.column_stack([np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(K - 1)])
    grid = 100000 + np.arange(N, dtype=np.int32)
    rows = [np.flatnonzero(rng.random(N) >= 0.03).astype(np.int32) for _ in range(B)]      # ~3 % of the cadences missing per target
    n_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    allrows = np.concatenate(rows)
    ntot = int(n_off[-1])
    err = rng.uniform(0.5, 2.0, ntot) * 2e-4
    w = rng.normal(0, 1e-3, (B, K - 1))
    flux = np.concatenate([1.0 + cbvs[r] @ w[b] for b, r in enumerate(rows)]) + rng.standard_normal(ntot) * err
    time_, cad = t[allrows], grid[allrows]
    sync = _capi.Handle.get(0).synchronize

    def shared():
        dev = DeviceLightCurveBatch.from_arrays(time_, flux, err, n_off, cadenceno=cad)
        return dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha, cadenceno=grid)[0]

    def stacked():
        X = np.column_stack([cbvs, np.ones(N)])
        lcs, dms = [], []
        for b, r in enumerate(rows):
            a, z = int(n_off[b]), int(n_off[b + 1])
            lcs.append(LightCurve(time=time_[a:z], flux=flux[a:z], flux_err=err[a:z]))
            dms.append(DesignMatrix(X[r], name="cbv", prior_mu=np.zeros(K), prior_sigma=np.full(K, np.median(err[a:z]) / np.sqrt(alpha))))
        return batch.regression_correct_batch(lcs, dms)[0]

    fns = {"S": shared, "T": stacked}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    a, b = first["S"].flux_host(), np.concatenate(first["T"])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    lines = ["CBV correction of a ragged batch: %d targets on a grid of %d cadences (%d kept in all, %.1f %% missing), K = %d columns, "
             "alpha = %g" % (B, N, ntot, 100.0 * (1 - ntot / (B * N)), K, alpha),
             "  S    from_arrays(cadenceno=) -> cbv_correct(cadenceno=grid): ONE %.1f MB matrix goes up              %s"
             % (N * K * 8 / 1e6, spread(ts["S"])),
             "  T    X[rows_b] per target -> regression_correct_batch: %.2f GB of stacked copies go up             %s"
             % (ntot * K * 8 / 1e9, spread(ts["T"])),
             "  max |S - T| / median flux: %.2e" % (np.max(np.abs(a - b)) / np.median(flux)),
             "  T / S = %.1f" % (med["T"] / med["S"])]
    print("\n".join(lines))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cbvragged_walls.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.stdout.flush()


def cbvinterp():
    from concurrent.futures import ThreadPoolExecutor
    from scipy.interpolate import PchipInterpolator
    from lightkurve_amd import _capi, batch
    from lightkurve_amd.correctors import DesignMatrix
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, K = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_K", "16")))
    reps, alpha = int(os.environ.get("LK_WALLS_REPS", "5")), 1e-4
    sync = _capi.Handle.get(0).synchronize
    lines = []
    # (name, knots, knot step [two-minute cadences], cadences per target, target step)
    for name, Nx, kstep, n0, tstep in (("ten-minute targets on two-minute knots", 18000, 1, 3590, 5),
                                       ("two-minute targets on thirty-minute knots", 1200, 15, 17900, 1)):
        rng = np.random.default_rng(29)
        x = 2000.0 + kstep * np.arange(Nx) / 720.0
        cbvs = np.column_stack([np.sin(2 * np.pi * (x - x[0]) * rng.uniform(0.05, 1.0) + rng.uniform(0, 6)) for _ in range(K)])
        ns = rng.integers(n0 - 90, n0 + 1, B)
        n_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        ntot = int(n_off[-1])
        time_ = np.concatenate([x[0] + (rng.integers(1, 6) + tstep * np.arange(n)) / 720.0 + rng.uniform(-30, 30) / 86400.0 for n in ns])
        assert time_.min() >= x[0] and time_.max() <= x[-1]
        err = rng.uniform(0.5, 2.0, ntot) * 2e-4
        w = rng.normal(0, 1e-3, (B, K))
        true = PchipInterpolator(x, cbvs, axis=0)
        flux = np.concatenate([1.0 + true(time_[n_off[b]:n_off[b + 1]]) @ w[b] for b in range(B)]) + rng.standard_normal(ntot) * err
        resident = DeviceLightCurveBatch.from_arrays(time_, flux, err, n_off)
        resident.synchronize()

        def interpolated():
            dev = DeviceLightCurveBatch.from_arrays(time_, flux, err, n_off)
            return dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha, cbv_time=x)[0]

        def through_host():
            host = resident.to_host()

            def one(b):
                a, z = int(host.n_off[b]), int(host.n_off[b + 1])
                Xb = np.column_stack([PchipInterpolator(x, cbvs, axis=0, extrapolate=False)(host.time[a:z]), np.ones(z - a)])
                sg = np.full(K + 1, np.median(host.flux_err[a:z]) / np.sqrt(alpha))
                return (LightCurve(time=host.time[a:z], flux=host.flux[a:z], flux_err=host.flux_err[a:z]),
                        DesignMatrix(Xb, name="cbv", prior_mu=np.zeros(K + 1), prior_sigma=sg))

            with ThreadPoolExecutor(max_workers=16) as ex:
                pairs = list(ex.map(one, range(B)))
            return batch.regression_correct_batch([p[0] for p in pairs], [p[1] for p in pairs])[0]

        fns = {"I": interpolated, "H": through_host}
        first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
        sync()
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                ts[k].append(timed(lambda: (fn(), sync()))[0])
        a, b = first["I"].flux_host(), np.concatenate(first["H"])
        med = {k: float(np.median(v)) for k, v in ts.items()}
        lines += ["CBV correction on interpolated CBVs, %s: %d targets, %d cadences in all, %d knots, K = %d + constant, alpha = %g"
                  % (name, B, ntot, Nx, K, alpha),
                  "  I    from_arrays -> cbv_correct(cbv_time=): the %.2f GB of interpolated matrices are written and read in HBM   %s"
                  % (ntot * (K + 1) * 8 / 1e9, spread(ts["I"])),
                  "  H    to_host() -> PchipInterpolator per target, 16 threads -> regression_correct_batch (%.2f GB go up)      %s"
                  % (ntot * (K + 1) * 8 / 1e9, spread(ts["H"])),
                  "  max |I - H| / median flux: %.2e" % (np.max(np.abs(a - b)) / np.median(flux)),
                  "  H / I = %.1f" % (med["H"] / med["I"]), "  kernels alone: not measured", ""]
        print("\n".join(lines[-7:]))
        sys.stdout.flush()
        del resident, first
    write_walls("cbvinterp_walls.txt", lines[:-1])


def cbvroutes():
    from lightkurve_amd import _capi
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N, K = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_K", "16")))
    reps, alpha = int(os.environ.get("LK_WALLS_REPS", "5")), 1e-4
    label = os.environ.get("LK_WALLS_LABEL", "this commit")
    rng = np.random.default_rng(31)
    t = np.linspace(0.0, 27.0, N)
    cbvs = np.column_stack([np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(K)])
    grid = 100000 + np.arange(N, dtype=np.int32)
    err = rng.uniform(0.5, 2.0, B * N) * 2e-4
    flux = (1.0 + rng.normal(0, 1e-3, (B, K)) @ cbvs.T).reshape(-1) + rng.standard_normal(B * N) * err
    time_, cad = np.tile(t, B), np.tile(grid, B)
    n_off = N * np.arange(B + 1, dtype=np.int64)
    sync = _capi.Handle.get(0).synchronize
    uni = DeviceLightCurveBatch.from_arrays(time_, flux, err, n_off)
    rag = DeviceLightCurveBatch.from_arrays(time_, flux, err, n_off, cadenceno=cad)
    fns = {"U": lambda: uni.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha),
           "C": lambda: rag.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha, cadenceno=grid)}
    for fn in fns.values():
        fn()
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(lambda: (fn(), sync()))[0])
    print("cbvroutes  %-11s  U  resident cbv_correct(), uniform, %d x %d x %d + constant          %s" % (label, B, N, K, spread(ts["U"])))
    print("cbvroutes  %-11s  C  resident cbv_correct(cadenceno=grid), every cadence on the grid    %s" % (label, spread(ts["C"])))
    sys.stdout.flush()


def ragged_field_for_walls(B, N, M, K):
    """B targets on a grid of N cadences, ~3 % of them missing per target (the shape of `cbvragged`), K basis vectors of which four
    carry systematics, M nearest neighbours -> dict of packed host arrays."""
    from lightkurve_amd.correctors import metrics
    rng = np.random.default_rng(23)
    t = np.linspace(0.0, 27.0, N)
    x = t / 27 - 0.5
    S = np.column_stack([np.sin(2 * np.pi * t / p) for p in np.linspace(3.1, 41.0, K - 1)] + [x ** 2])
    amp = rng.normal(0, 0.01, (B, K)) * (np.arange(K) < 4)
    scale = 1000.0 * rng.uniform(0.5, 2, B)
    grid = 100000 + np.arange(N, dtype=np.int32)
    rows = [np.flatnonzero(rng.random(N) >= 0.03).astype(np.int32) for _ in range(B)]
    n_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flux = np.concatenate([scale[b] * (1 + S[r] @ amp[b] + 1e-3 * rng.standard_normal(len(r))) for b, r in enumerate(rows)])
    allrows = np.concatenate(rows)
    nb = metrics.nearest_neighbors(rng.uniform(0, 1, B), rng.uniform(0, 1, B), M)
    return dict(t=t, S=S, grid=grid, rows=rows, n_off=n_off, flux=flux, err=1e-3 * flux, time=t[allrows], cad=grid[allrows], nb=nb)


def host_underfit_ragged(lcb, rows, nb, t, Nx, targets):
    """The route a ragged batch had before: the downloaded batch (``to_host()``), the neighbours brought onto each target's cadences
    (NaN where a neighbour lacks one) and ``underfit_metric_neighbors`` per target, 16 threads -> metric[len(targets)]."""
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.correctors import metrics
    from lightkurve_amd.lightcurve import LightCurve
    B = len(rows)
    z = np.full((B, Nx), np.nan)
    for b in range(B):
        f = lcb.flux[lcb.n_off[b]:lcb.n_off[b + 1]]
        z[b, rows[b]] = f / np.median(f) - 1.0

    def one(b):
        r = rows[b]
        f = lcb.flux[lcb.n_off[b]:lcb.n_off[b + 1]]
        return metrics.underfit_metric_neighbors(LightCurve(t[r], f), z[nb[b][nb[b] >= 0]][:, r].T)

    with ThreadPoolExecutor(max_workers=16) as ex:
        return np.array(list(ex.map(one, targets)))


def write_walls(name, lines):
    print("\n".join(lines))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", name), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.stdout.flush()


def underfit_ragged():
    from lightkurve_amd import _capi
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N, M = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_M", "50")))
    reps = int(os.environ.get("LK_WALLS_REPS", "3"))
    f = ragged_field_for_walls(B, N, M, 3)
    nb, grid, M = f["nb"], f["grid"], f["nb"].shape[1]
    raw = DeviceLightCurveBatch.from_arrays(f["time"], f["flux"], f["err"], f["n_off"], cadenceno=f["cad"]).remove_nans()
    cor = raw.cbv_correct(f["S"], cbv_indices=[1, 2], cadenceno=grid)[0]
    cor.synchronize()
    sync = _capi.Handle.get(0).synchronize
    pitch = -(-N // 128) * 128

    def host_route():
        return host_underfit_ragged(cor.to_host(), f["rows"], nb, f["t"], N, range(B))

    got, n_common = cor.under_fitting_metric(nb, cadenceno=grid, return_common=True)          # warm-up of both routes
    cor.under_fitting_metric(nb, cadenceno=grid, to_host=False)
    sync()
    ref = host_route()
    R, R2, H = [], [], []
    for _ in range(reps):
        R.append(timed(lambda: cor.under_fitting_metric(nb, cadenceno=grid))[0])              # (the download synchronises)
        R2.append(timed(lambda: (cor.under_fitting_metric(nb, cadenceno=grid, to_host=False), sync()))[0])
        H.append(timed(host_route)[0])
    write_walls("underfit_ragged_walls.txt", [
        "under-fitting metric of a ragged batch: %d cotrended targets on a grid of %d cadences (%d kept in all, %.1f %% missing), "
        "%d neighbours each; common cadences per target %d..%d" % (B, N, int(f["n_off"][-1]), 100.0 * (1 - f["n_off"][-1] / (B * N)), M,
                                                                   n_common.min(), n_common.max()),
        "  the pair pass reads %.2f GB of z rows (B M pitch 8) and %.1f MB of presence words; scratch %.1f MB (rows + words + the "
        "inverse map)" % (B * M * pitch * 8 / 1e9, B * M * pitch / 8 / 1e6, (B * pitch * 8 + B * pitch / 8 + B * N * 4) / 1e6),
        "  R  batch.under_fitting_metric(cadenceno=grid) -> metric[B] on the host (aligns, prepares, pairs)   %s" % spread(R),
        "  R' the same, to_host=False + synchronise                                                          %s" % spread(R2),
        "  H  to_host() + neighbours onto each target's cadences + underfit_metric_neighbors, 16 threads     %s" % spread(H),
        "  max |R - H| = %.3e; metric min %.4f median %.4f; H / R = %.0f"
        % (float(np.max(np.abs(got - ref))), got.min(), float(np.median(got)), np.median(H) / np.median(R))])


def cbvopt_ragged():
    from lightkurve_amd import _capi
    from lightkurve_amd.correctors import metrics
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    B, N, K, M = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_K", "16"),
                                                         ("LK_WALLS_M", "50")))
    reps = int(os.environ.get("LK_WALLS_REPS", "2"))
    Hn = min(B, int(os.environ.get("LK_WALLS_HOST_TARGETS", str(B))))       # the host route's over-fitting loop is sequential
    f = ragged_field_for_walls(B, N, M, K)
    nb, grid, S = f["nb"], f["grid"], f["S"]
    raw = DeviceLightCurveBatch.from_arrays(f["time"], f["flux"], f["err"], f["n_off"], cadenceno=f["cad"]).remove_nans()
    raw.synchronize()
    sync = _capi.Handle.get(0).synchronize
    kw = dict(neighbors=nb, cbv_indices=np.arange(1, K + 1), cadenceno=grid)
    out, info = raw.cbv_correct_optimized(S, **kw)                                       # warm-up; the search is deterministic
    steps = int(info["nfev"].max())
    alpha = float(np.median(info["alpha"]))

    def host_evaluation():
        """ONE evaluation of the objective the way a ragged batch had it: the resident ragged fit, then both metrics per target on
        the host (the under-fitting metric against the other targets of the same correction)."""
        cor = raw.cbv_correct(S, cbv_indices=np.arange(1, K + 1), alpha=alpha, cadenceno=grid)[0]
        lcb, lc0 = cor.to_host(), raw.to_host()
        under = host_underfit_ragged(lcb, f["rows"], nb, f["t"], N, range(Hn))
        over = np.empty(Hn)
        for b in range(Hn):
            a, z = int(lcb.n_off[b]), int(lcb.n_off[b + 1])
            over[b] = metrics.overfit_metric_lombscargle(LightCurve(lcb.time[a:z], lc0.flux[a:z], lcb.flux_err[a:z]),
                                                         LightCurve(lcb.time[a:z], lcb.flux[a:z], lcb.flux_err[a:z]), n_samples=1)
        return over, under

    scan = raw.cbv_goodness_scan(S, [alpha], neighbors=nb, cbv_indices=np.arange(1, K + 1), n_samples=1, cadenceno=grid)
    sync()
    h_over, h_under = host_evaluation()
    O, H = [], []
    for _ in range(reps):
        O.append(timed(lambda: (raw.cbv_correct_optimized(S, **kw), sync()))[0])
        H.append(timed(host_evaluation)[0])
    write_walls("cbvopt_ragged_walls.txt", [
        "per-target ridge search of a ragged batch: %d targets on a grid of %d cadences (%d kept in all, %.1f %% missing), %d basis "
        "vectors + constant, %d neighbours, bounds (1e-4, 1e4)" % (B, N, int(f["n_off"][-1]), 100.0 * (1 - f["n_off"][-1] / (B * N)), K,
                                                                    nb.shape[1]),
        "  evaluations per target: min %d median %d max %d (= lockstep evaluations); status counts %s; common cadences %d..%d"
        % (info["nfev"].min(), int(np.median(info["nfev"])), steps, np.bincount(info["status"], minlength=3).tolist(),
           info["n_common"].min(), info["n_common"].max()),
        "  alpha: min %.3g median %.3g max %.3g; over-fitting score median %.4f, under-fitting score median %.4f"
        % (info["alpha"].min(), float(np.median(info["alpha"])), info["alpha"].max(), float(np.median(info["over_fitting_score"])),
           float(np.median(info["under_fitting_score"]))),
        "  O  batch.cbv_correct_optimized(cadenceno=grid), the whole call (%d lockstep evaluations)                  %s"
        % (steps, spread(O)),
        "  H  ONE evaluation at alpha = %.3g the way it was: cbv_correct(cadenceno=) + to_host() + both metrics per target on the "
        "host, %d of %d targets (under-fitting 16 threads, over-fitting sequential)   %s" % (alpha, Hn, B, spread(H)),
        "  O per lockstep evaluation %.2f ms; H per evaluation / O per evaluation = %.0f (H over %d targets, O over %d)"
        % (1e3 * np.median(O) / steps, np.median(H) / (np.median(O) / steps), Hn, B),
        "  at that alpha, resident scan against the host route: max |under-fitting R - H| = %.3e; over-fitting median R %.4f, H %.4f "
        "(different noise: equal in distribution), max |R - H| = %.3e"
        % (float(np.max(np.abs(scan["under_fitting"][0][:Hn] - h_under))), float(np.median(scan["over_fitting"][0][:Hn])),
           float(np.median(h_over)), float(np.max(np.abs(scan["over_fitting"][0][:Hn] - h_over))))])


def foldbin():
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N, bins = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000"), ("LK_WALLS_BINS", "201")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    rng = np.random.default_rng(23)
    t = 1000.0 + 0.0204 * np.arange(N)
    period = rng.uniform(0.7, 12.0, B)
    flux = 1.0 + 3e-4 * rng.standard_normal((B, N)) - 0.005 * (np.abs((t[None] - t[0]) / period[:, None] % 1.0 - 0.5) > 0.49)
    err = np.full((B, N), 3e-4)
    n_off = np.arange(B + 1, dtype=np.int64) * N
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), flux.ravel(), err.ravel(), n_off)

    def fused():
        return raw.fold_bin(period, bins=bins).to_host()

    def sorted_then_binned():
        return raw.fold(period).bin(bins=bins).to_host()

    def one(host, b):
        a, z = int(host.n_off[b]), int(host.n_off[b + 1])
        tt, ff, ee, P = host.time[a:z], host.flux[a:z], host.flux_err[a:z], period[b]
        ph = np.mod((tt - tt[0]) + P / 2.0, P) - P / 2.0
        o = np.argsort(ph, kind="stable")
        ph, ff, ee = ph[o], ff[o], ee[o]
        size = (ph[-1] - ph[0]) * ph.size / ((ph.size - 1) * bins) * 86400.0
        rel = (ph - ph[0]) * 86400.0
        nb = int(np.ceil(rel[-1] / size))
        edges = np.cumsum(np.hstack([0.0, np.repeat(size, nb)]))
        keep = rel < edges[-1]
        idx = np.searchsorted(edges, rel[keep]) - 1
        idx[rel[keep] == 0.0] = 0
        cnt = np.bincount(idx, minlength=nb)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (np.bincount(idx, ff[keep], minlength=nb) / cnt, np.sqrt(np.bincount(idx, ee[keep] ** 2, minlength=nb) / cnt), cnt)

    def through_host():
        host = raw.to_host()
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda b: one(host, b), range(B)))

    fns = {"F": fused, "S": sorted_then_binned, "H": through_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    f, s2 = first["F"], first["S"]
    same_layout = np.array_equal(f["bin_off"], s2["bin_off"]) and np.array_equal(f["count"], s2["count"]) \
        and np.array_equal(f["phase"], s2["phase"])
    rel = float(np.nanmax(np.abs(f["flux"] - s2["flux"]) / np.abs(s2["flux"])))
    hf = np.concatenate([h[0] for h in first["H"]])
    hc = np.concatenate([h[2] for h in first["H"]])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    write_walls("foldbin_walls.txt", [
        "phase-binned folded light curves, %d targets x %d cadences, one period per target, bins = %d (%.1f MB of input columns, "
        "%.2f MB of result)" % (B, N, bins, 3 * B * N * 8 / 1e6, f["flux"].size * 28 / 1e6),
        "  F    batch.fold_bin(period, bins=).to_host(): plan kernel + fused kernel, no sort                %s" % spread(ts["F"]),
        "  S    batch.fold(period).bin(bins=).to_host(): bitonic sort, two gathers, plan, bin kernel        %s" % spread(ts["S"]),
        "  H    to_host(), numpy fold + argsort + bin per target on 16 threads                              %s" % spread(ts["H"]),
        "  F and S: same layout, counts and bin centres: %s; max relative difference of the binned flux %.2e" % (same_layout, rel),
        "  F and H: same counts: %s; max relative difference of the binned flux %.2e"
        % (np.array_equal(hc, f["count"]), float(np.nanmax(np.abs(hf - f["flux"]) / np.abs(f["flux"]))) if hf.size == f["flux"].size else np.nan),
        "  S / F = %.2f; H / F = %.1f" % (med["S"] / med["F"], med["H"] / med["F"])])


def river():
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd import _capi, river as rv
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, N = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_N", "20000")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    method = os.environ.get("LK_WALLS_METHOD", "mean")
    rng = np.random.default_rng(29)
    t = 1000.0 + 0.0204 * np.arange(N)
    period = rng.uniform(0.7, 12.0, B)
    flux = 1.0 + 3e-4 * rng.standard_normal((B, N)) - 0.005 * (np.abs((t[None] - t[0]) / period[:, None] % 1.0 - 0.5) > 0.49)
    err = np.full((B, N), 3e-4)
    n_off = np.arange(B + 1, dtype=np.int64) * N
    raw = DeviceLightCurveBatch.from_arrays(np.tile(t, B), flux.ravel(), err.ravel(), n_off)
    raw.synchronize()
    sync = _capi.Handle.get(0).synchronize

    def resident():
        out = raw.river(period, method=method)
        sync()
        return out

    def to_host():
        return raw.river(period, method=method).to_host()

    def through_host():
        host = raw.to_host()

        def one(b):
            a, z = int(host.n_off[b]), int(host.n_off[b + 1])
            return rv.river_numpy(host.time[a:z], host.flux[a:z], host.flux_err[a:z], period[b], method=method)
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(one, range(B)))

    fns = {"D": resident, "T": to_host, "H": through_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    d, h = first["T"], first["H"]
    same = all(np.array_equal(d["count"][b], h[b]["count"]) for b in range(B)) and all(int(s) == 0 for s in d["status"])
    worst = 0.0
    for b in range(B):
        fin = np.isfinite(h[b]["river"])
        if fin.any():
            worst = max(worst, float(np.max(np.abs(d["river"][b][fin] - h[b]["river"][fin]) / np.maximum(1.0, np.abs(h[b]["river"][fin])))))
    cells = int(d["cell_off"][-1])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    write_walls("river_walls.txt", [
        "river diagrams, %d targets x %d cadences, one period per target, default arguments, method = %s (%.1f MB of input columns, "
        "%d cells = %.1f MB of images)" % (B, N, method, 3 * B * N * 8 / 1e6, cells, cells * 12 / 1e6),
        "  D    batch.river(period) + synchronise: plan kernel + image kernel, images resident              %s" % spread(ts["D"]),
        "  T    batch.river(period).to_host(): the same and the images copied to the host                   %s" % spread(ts["T"]),
        "  H    to_host(), LightCurve.river's numpy mirror per target on 16 threads                         %s" % spread(ts["H"]),
        "  D and H: same shapes, statuses and counts: %s; max |difference| / max(1, |H|) of the images %.2e" % (same, worst),
        "  H / D = %.1f; H / T = %.1f" % (med["H"] / med["D"], med["H"] / med["T"])])


def diffimage():
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    rng = np.random.default_rng(29)
    t = 1000.0 + np.arange(N) / 48.0
    period, duration = rng.uniform(1.5, 9.0, B), rng.uniform(0.1, 0.3, B)
    t0 = t[0] + rng.uniform(0.0, 1.0, B) * period
    yy, xx = np.indices((side, side))
    c = side // 2
    star = 1000.0 * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / 1.62) + 300.0 * np.exp(-((xx - c - 2) ** 2 + (yy - c) ** 2) / 1.62)
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # (drawn per cutout: 1.9 GB of cubes in all)
        flux[b] = star + 20.0 + rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.ones_like(flux)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err

    def resident():
        out = cubes.difference_images(period, t0, duration)
        cubes.synchronize()
        return out

    def through_host():
        host = cubes.to_host()
        with ThreadPoolExecutor(max_workers=16) as ex:
            out = list(ex.map(lambda b: host[b].difference_image(period[b], t0[b], duration[b]), range(B)))
        cubes.synchronize()
        return out

    fns = {"R": resident, "H": through_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    r, h = first["R"], first["H"]
    scale = np.nanmax(np.abs(r["diff"]), axis=(1, 2))
    rel = max(float(np.nanmax(np.abs(h[b]["diff"] - r["diff"][b])) / scale[b]) for b in range(B) if scale[b] == scale[b])
    pix = np.array([h[b]["offset_pix"] for b in range(B)])
    ok = ~np.isnan(pix)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    write_walls("diffimage_walls.txt", [
        "transit difference images, %d cutouts x %d cadences x %d x %d float32, one box per cutout (%.1f MB of cubes resident, "
        "%.2f MB of images)" % (B, N, side, side, 2 * B * N * side * side * 4 / 1e6, 4 * B * side * side * 8 / 1e6),
        "  R    cubes.difference_images(period, transit_time, duration): classes, chunk sums, images, 4 centroids   %s" % spread(ts["R"]),
        "  H    to_host(), PixelCube.difference_image per cutout on 16 threads                                      %s" % spread(ts["H"]),
        "  R and H: same counts and statuses: %s; max |diff_R - diff_H| / max |diff| %.2e; max |offset_pix_R - offset_pix_H| %.2e px"
        % (all(np.array_equal(r[k], [h[b][k] for b in range(B)]) for k in ("n_in", "n_out", "status")), rel,
           float(np.max(np.abs(pix[ok] - r["offset_pix"][ok]))) if ok.any() else np.nan),
        "  H / R = %.1f" % (med["H"] / med["R"])])


def ampimage():
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    rng = np.random.default_rng(37)
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    freq = rng.uniform(5.0, 60.0, B)                                     # [1/d]: 28 to 330 cycles in the baseline
    period, duration = rng.uniform(1.5, 5.0, B), rng.uniform(0.1, 0.3, B)
    t0 = t[0] + rng.uniform(0.0, 1.0, B) * period
    yy, xx = np.indices((side, side))
    c = side // 2
    star = (1e4 + 3000.0 * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / 1.62)).astype(np.float32)
    neighbour = (800.0 * np.exp(-((xx - c - 3) ** 2 + (yy - c) ** 2) / 1.62)).astype(np.float32)
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # (drawn per cutout: 1.9 GB of cubes in all)
        signal = (1.0 + 0.05 * np.sin(2 * np.pi * freq[b] * (t - t[0]) + 0.7)).astype(np.float32)
        flux[b] = star + neighbour * signal[:, None, None] + 2.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 2.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err

    def resident(nterms=1):
        out = cubes.amplitude_images(freq, nterms)
        cubes.synchronize()
        return out

    def difference():
        out = cubes.difference_images(period, t0, duration)
        cubes.synchronize()
        return out

    def through_host():
        host = cubes.to_host()
        with ThreadPoolExecutor(max_workers=16) as ex:
            out = list(ex.map(lambda b: host[b].amplitude_image(freq[b]), range(B)))
        cubes.synchronize()
        return out

    fns = {"R": resident, "R3": lambda: resident(3), "D": difference, "H": through_host}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    r, h = first["R"], first["H"]
    rel = {}
    for key in ("theta", "level", "amplitude", "amplitude_err", "chi2"):
        rel[key] = max(float(np.nanmax(np.abs(h[b][key] - r[key][b])) / np.nanmax(np.abs(h[b][key]))) for b in range(B))
    pix = np.array([h[b]["offset_pix"] for b in range(B)])
    ok = ~np.isnan(pix)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    write_walls("ampimage_walls.txt", [
        "amplitude images, %d cutouts x %d cadences x %d x %d float32, one frequency per cutout (%.1f MB of flux resident, read twice; "
        "%.2f MB of images at nterms = 1)" % (B, N, side, side, B * N * side * side * 4 / 1e6, 10.5 * B * side * side * 8 / 1e6),
        "  R    cubes.amplitude_images(frequency, nterms=1): trig, pivots, chunk sums, solve, residual pass, 4 centroids  %s" % spread(ts["R"]),
        "  R3   the same with nterms=3 (K = 7)                                                                           %s" % spread(ts["R3"]),
        "  D    cubes.difference_images(period, transit_time, duration) of the same cubes: classed rows of two cubes     %s" % spread(ts["D"]),
        "  H    to_host(), PixelCube.amplitude_image per cutout on 16 threads                                            %s" % spread(ts["H"]),
        "  R and H: same counts and statuses: %s; max |R - H| / max |image|: %s; max |offset_pix_R - offset_pix_H| %.2e px"
        % (all(np.array_equal(r[k], [h[b][k] for b in range(B)]) for k in ("n_used", "status")),
           ", ".join("%s %.2e" % kv for kv in rel.items()), float(np.max(np.abs(pix[ok] - r["offset_pix"][ok]))) if ok.any() else np.nan),
        "  R / D = %.2f; R3 / D = %.2f; H / R = %.1f; kernel times alone: profiles/ampimage_kernels.txt" % (med["R"] / med["D"], med["R3"] / med["D"], med["H"] / med["R"])])


def pixelpg(which):
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch
    B, N, side, F = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_F", "2000")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(53)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    grid = np.linspace(1.5 / (t[-1] - t[0]), 0.25 * 720.0, F)            # [1/d]: 1.5 cycles per baseline to a quarter of the sampling rate
    freq = rng.uniform(5.0, 60.0, B)
    yy, xx = np.indices((side, side))
    c = side // 2
    star = (1e4 + 3000.0 * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / 1.62)).astype(np.float32)
    neighbour = (800.0 * np.exp(-((xx - c - 3) ** 2 + (yy - c) ** 2) / 1.62)).astype(np.float32)
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # (drawn per cutout: 1.9 GB of cubes in all)
        signal = (1.0 + 0.05 * np.sin(2 * np.pi * freq[b] * (t - t[0]) + 0.7)).astype(np.float32)
        flux[b] = star + neighbour * signal[:, None, None] + 2.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 2.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err

    def resident(return_power=True):
        out = cubes.pixel_periodograms(grid, return_power=return_power, to_host=False)
        cubes.synchronize()
        return out

    if "pixelpg_trace" in which:
        resident()
        resident()
        resident(False)
        return

    def per_light_curve():
        host = cubes.to_host()
        y = np.empty((B, npix, N), dtype=np.float64)
        for b in range(B):                                              # the transpose: every pixel becomes a light curve
            y[b] = host[b].flux.reshape(N, npix).T
        lcs = DeviceLightCurveBatch.from_arrays(np.tile(t, B * npix), y.reshape(-1), np.ones(B * npix * N),
                                                np.arange(B * npix + 1, dtype=np.int64) * N)
        out = lcs.to_periodogram_power(grid, ls_method="slow", to_host=False)
        lcs.synchronize()
        return out

    host_m = cubes.to_host()[:Bm]

    def mirror():
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda cube: cube.pixel_periodogram(grid), host_m))

    fns = {"R": resident, "P": lambda: resident(False), "L": per_light_curve, "H": mirror}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    r = first["R"]["power"].download(np.float64, Bm * F * npix, stream=cubes.stream).reshape(Bm, F, npix)
    l = first["L"].download(np.float64, Bm * npix * F).reshape(Bm, npix, F).transpose(0, 2, 1)
    h = np.stack([o["power"].reshape(F, npix) for o in first["H"]])
    top = np.max(h, axis=1, keepdims=True)
    rel = {"R - H": float(np.max(np.abs(r - h) / top)), "L - H": float(np.max(np.abs(l - h) / top)), "R - L": float(np.max(np.abs(r - l) / top))}
    pk = first["P"]["peak_index"].download(np.int32, B * npix, stream=cubes.stream)
    same_peaks = np.array_equal(pk, first["R"]["peak_index"].download(np.int32, B * npix, stream=cubes.stream))
    peaks_h = np.array_equal(pk[:Bm * npix].reshape(Bm, npix), np.stack([o["peak_index"].reshape(npix) for o in first["H"]]))
    first.clear()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    write_walls("pixelpg_walls.txt", [
        "per-pixel Lomb-Scargle periodograms, %d cutouts x %d cadences x %d x %d float32, one grid of %d frequencies (%.1f MB of flux "
        "resident, %.1f MB of power)" % (B, N, side, side, F, B * N * npix * 4 / 1e6, B * F * npix * 8 / 1e6),
        "  R    cubes.pixel_periodograms(grid, to_host=False): stats, spectra, peaks; the power cube resident            %s" % spread(ts["R"]),
        "  P    the same with return_power=False: the peak images alone                                                   %s" % spread(ts["P"]),
        "  L    to_host(), host transpose, DeviceLightCurveBatch.from_arrays, to_periodogram_power(ls_method='slow')    %s" % spread(ts["L"]),
        "  H    PixelCube.pixel_periodogram on 16 threads, the first %d cutouts only                                      %s" % (Bm, spread(ts["H"])),
        "  max |difference| / max of the pixel's spectrum over the first %d cutouts: %s" % (Bm, ", ".join("%s %.2e" % kv for kv in rel.items())),
        "  P and R: the same peak_index: %s; P and H (first %d cutouts): the same peak_index: %s" % (same_peaks, Bm, peaks_h),
        "  L / R = %.2f; L / P = %.2f; H scaled to %d cutouts / R = %.0f; kernel times alone: profiles/pixelpg_kernel_stats.txt"
        % (med["L"] / med["R"], med["L"] / med["P"], B, med["H"] * B / Bm / med["R"])])


def psfphot(which):
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(61)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma = 1.1
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    shifts = (0.2 * np.sin(2 * np.pi * (t - t[0]) / 3.1)[None, :] * rng.uniform(0.5, 1.0, (B, 1)),
              0.2 * np.cos(2 * np.pi * (t - t[0]) / 3.1)[None, :] * rng.uniform(0.5, 1.0, (B, 1)))
    edges = np.arange(side + 1) - 0.5
    from scipy.special import erf
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # (drawn per cutout: 1.9 GB of flux in all; the stars do not move)
        img = np.full((side, side), 100.0)
        for s in range(S):
            gx = np.diff(erf((edges - col[b, s]) / (np.sqrt(2) * sigma))) / 2
            gy = np.diff(erf((edges - row[b, s]) / (np.sqrt(2) * sigma))) / 2
            img += rng.uniform(2000.0, 20000.0) * gy[:, None] * gx[None, :]
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)

    def resident(sh=None):
        out = cubes.psf_photometry(col, row, sigma, shifts=sh)
        cubes.synchronize()
        return out

    if "psfphot_trace" in which:
        for _ in range(2):
            resident()
            resident(d_shifts)
        return

    host_m = cubes.to_host()[:Bm]

    def mirror(with_shifts=False):
        def one(b):
            return host_m[b].psf_photometry(col[b], row[b], sigma, shifts=(shifts[0][b], shifts[1][b]) if with_shifts else None)
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(one, range(Bm)))

    fns = {"R": resident, "Rs": lambda: resident(d_shifts), "H": mirror, "Hs": lambda: mirror(True)}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    rel = {}
    for k, hk in (("R", "H"), ("Rs", "Hs")):
        f = first[k][0].flux_host().reshape(B * S, N)[:Bm * S].reshape(Bm, S, N)
        h = np.stack([o["flux"] for o in first[hk]])
        rel[k + " - " + hk] = float(np.max(np.abs(f - h) / np.max(np.abs(h), axis=(1, 2), keepdims=True)))
    first.clear()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    floor = B * N * npix * 8 + B * N * (3 * S * 8 + 8 + 8 + 4 + 1)
    write_walls("psfphot_walls.txt", [
        "PSF photometry, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout, sigma %.1f px (%.1f MB of flux and flux_err "
        "resident, read once; %.1f MB of outputs)" % (B, N, side, side, S, sigma, B * N * npix * 8 / 1e6, (floor - B * N * npix * 8) / 1e6),
        "  R    cubes.psf_photometry(star_col, star_row, sigma): tables per cutout, fit, statuses; everything resident     %s" % spread(ts["R"]),
        "  Rs   the same with shifts=(DeviceBuffer, DeviceBuffer): tables per cadence                                      %s" % spread(ts["Rs"]),
        "  H    PixelCube.psf_photometry on 16 threads, the first %d cutouts only                                          %s" % (Bm, spread(ts["H"])),
        "  Hs   the same with shifts                                                                                        %s" % spread(ts["Hs"]),
        "  max |flux difference| / max |flux| of the cutout over the first %d cutouts: %s" % (Bm, ", ".join("%s %.2e" % kv for kv in rel.items())),
        "  H scaled to %d cutouts / R = %.0f; Hs scaled / Rs = %.0f; floor bytes of the fit kernel %.1f MB; kernel times alone: "
        "profiles/psfphot_kernel_stats.txt" % (B, med["H"] * B / Bm / med["R"], med["Hs"] * B / Bm / med["Rs"], floor / 1e6)])


def prfphot(which):
    from concurrent.futures import ThreadPoolExecutor
    from scipy.special import erf
    from lightkurve_amd.correctors import TabulatedPRF
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(71)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma = 1.1
    prf = TabulatedPRF.from_gaussian(sigma, sigma, 50, 5.5)
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))     # the true pointing of every cadence
    edges = np.arange(side + 1) - 0.5
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # every cadence rendered at its own shift
        gx = np.diff(erf((edges[None, None, :] - col[b][None, :, None] - shifts[0][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        gy = np.diff(erf((edges[None, None, :] - row[b][None, :, None] - shifts[1][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        img = 100.0 + np.einsum("s,nsy,nsx->nyx", rng.uniform(2000.0, 20000.0, S), gy, gx)
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)

    def resident(sh=None, table=True):
        out = cubes.psf_photometry(col, row, shifts=sh, prf=prf) if table else cubes.psf_photometry(col, row, sigma, shifts=sh)
        cubes.synchronize()
        return out

    if "prfphot_trace" in which:
        for _ in range(2):
            resident()
            resident(d_shifts)
        return

    host_m = cubes.to_host()[:Bm]

    def mirror(with_shifts=False):
        def one(b):
            return host_m[b].psf_photometry(col[b], row[b], prf=prf, shifts=(shifts[0][b], shifts[1][b]) if with_shifts else None)
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(one, range(Bm)))

    fns = {"P": resident, "Ps": lambda: resident(d_shifts), "G": lambda: resident(None, False), "Gs": lambda: resident(d_shifts, False),
           "H": mirror, "Hs": lambda: mirror(True)}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    dev = {k: first[k][0].flux_host().reshape(B * S, N)[:Bm * S].reshape(Bm, S, N) for k in ("P", "Ps", "G", "Gs")}
    rel = {}
    for k, other in (("P", "H"), ("Ps", "Hs"), ("Ps", "Gs")):
        h = dev[other] if other in dev else np.stack([o["flux"] for o in first[other]])
        rel[k + " - " + other] = float(np.max(np.abs(dev[k] - h) / np.max(np.abs(h), axis=(1, 2), keepdims=True)))
    first.clear()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    floor = B * N * npix * 8 + B * N * (3 * S * 8 + 8 + 8 + 4 + 1)
    write_walls("prfphot_walls.txt", [
        "PSF photometry with a tabulated PRF, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout, table %d x %d at os = %d "
        "from the Gaussian of %.1f px (%.1f MB of flux and flux_err resident, read once; %.1f MB of outputs)"
        % ((B, N, side, side, S) + prf.samples.shape[1:] + (prf.oversample, sigma, B * N * npix * 8 / 1e6, (floor - B * N * npix * 8) / 1e6)),
        "  P    cubes.psf_photometry(star_col, star_row, prf=): polyphase table, images per cutout, fit, statuses; resident  %s" % spread(ts["P"]),
        "  Ps   the same with shifts=(DeviceBuffer, DeviceBuffer): images per cadence, formed in the fit kernel               %s" % spread(ts["Ps"]),
        "  G    cubes.psf_photometry(star_col, star_row, sigma) of the same cubes, the same run                               %s" % spread(ts["G"]),
        "  Gs   the same with the same shifts                                                                                 %s" % spread(ts["Gs"]),
        "  H    PixelCube.psf_photometry(prf=) on 16 threads, the first %d cutouts only                                       %s" % (Bm, spread(ts["H"])),
        "  Hs   the same with shifts                                                                                          %s" % spread(ts["Hs"]),
        "  max |flux difference| / max |flux| of the cutout over the first %d cutouts: %s" % (Bm, ", ".join("%s %.2e" % kv for kv in rel.items())),
        "  P / G = %.2f; Ps / Gs = %.2f; H scaled to %d cutouts / P = %.0f; Hs scaled / Ps = %.0f; floor bytes of the fit kernel %.1f MB; "
        "kernel times alone: profiles/prfphot_kernel_stats.txt"
        % (med["P"] / med["G"], med["Ps"] / med["Gs"], B, med["H"] * B / Bm / med["P"], med["Hs"] * B / Bm / med["Ps"], floor / 1e6)])


def prffit(which):
    from concurrent.futures import ThreadPoolExecutor
    from scipy.special import erf
    from lightkurve_amd.correctors import TabulatedPRF
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(73)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma = 1.1
    prf = TabulatedPRF.from_gaussian(sigma, sigma, 50, 5.5)
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))     # the true pointing of every cadence
    edges = np.arange(side + 1) - 0.5
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # every cadence rendered at its own shift
        gx = np.diff(erf((edges[None, None, :] - col[b][None, :, None] - shifts[0][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        gy = np.diff(erf((edges[None, None, :] - row[b][None, :, None] - shifts[1][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        img = 100.0 + np.einsum("s,nsy,nsx->nyx", rng.uniform(2000.0, 20000.0, S), gy, gx)
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)

    def fit(table=True):
        out = cubes.psf_fit(col, row, prf=prf) if table else cubes.psf_fit(col, row, sigma)
        cubes.synchronize()
        return out

    def given():
        out = cubes.psf_photometry(col, row, prf=prf, shifts=d_shifts)
        cubes.synchronize()
        return out

    if "prffit_trace" in which:
        for _ in range(2):
            fit()
            given()
        return

    host_m = cubes.to_host()[:Bm]

    def mirror():
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda b: host_m[b].psf_fit(col[b], row[b], prf=prf), range(Bm)))

    fns = {"F": fit, "Ps": given, "Fg": lambda: fit(False), "H": mirror}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    lcs, info = first["F"]
    n_iter = info["n_iter"].download(np.int32, B * N, stream=lcs.stream).reshape(B, N)
    cstat = info["cadence_status"].download(np.int8, B * N, stream=lcs.stream).reshape(B, N)
    got = tuple(info[k].download(np.float64, B * N, stream=lcs.stream).reshape(B, N) for k in ("shift_col", "shift_row"))
    gauss = tuple(first["Fg"][1][k].download(np.float64, B * N, stream=lcs.stream).reshape(B, N) for k in ("shift_col", "shift_row"))
    off = float(max(np.nanmax(np.abs(g - s)) for g, s in zip(got, shifts)))
    off_g = float(max(np.nanmax(np.abs(g - s)) for g, s in zip(got, gauss)))
    f = lcs.flux_host().reshape(B * S, N)[:Bm * S].reshape(Bm, S, N)
    h = np.stack([o["flux"] for o in first["H"]])
    rel = float(np.max(np.abs(f - h) / np.max(np.abs(h), axis=(1, 2), keepdims=True)))
    rel_u = float(max(np.max(np.abs(g[:Bm] - np.stack([o[k] for o in first["H"]]))) for g, k in zip(got, ("shift_col", "shift_row"))))
    same_iter = bool(np.array_equal(n_iter[:Bm], np.stack([o["n_iter"] for o in first["H"]])))
    first.clear()
    del lcs, info
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    evals = float(np.mean(np.max(np.pad(n_iter, ((0, 0), (0, -N % 16))).reshape(B, -1, 16), axis=2))) + 1
    write_walls("prffit_walls.txt", [
        "PSF fit with a pointing shift per cadence and a tabulated PRF, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout, "
        "table %d x %d at os = %d from the Gaussian of %.1f px, true shifts uniform in +-0.3 px (%.1f MB of flux and flux_err resident, "
        "read once)" % ((B, N, side, side, S) + prf.samples.shape[1:] + (prf.oversample, sigma, B * N * npix * 8 / 1e6)),
        "  F    cubes.psf_fit(star_col, star_row, prf=), defaults, from shifts 0; everything resident                      %s" % spread(ts["F"]),
        "  Ps   cubes.psf_photometry(prf=, shifts=(DeviceBuffer, DeviceBuffer)) at the TRUE shifts, the same run           %s" % spread(ts["Ps"]),
        "  Fg   cubes.psf_fit(star_col, star_row, sigma) of the same cubes, the same run                                   %s" % spread(ts["Fg"]),
        "  H    PixelCube.psf_fit(prf=) on 16 threads, the first %d cutouts only                                           %s" % (Bm, spread(ts["H"])),
        "  cadence statuses: %s; iterations per cadence: mean %.2f, max %d; evaluations per tile of 16 cadences (its slowest cadence + 1): "
        "mean %.2f" % (dict(zip(*(a.tolist() for a in np.unique(cstat, return_counts=True)))), float(n_iter.mean()), int(n_iter.max()), evals),
        "  largest |fitted - true shift| %.4f px, |shift(prf) - shift(sigma)| %.2e px; first %d cutouts against the mirror: max |flux "
        "difference| / max |flux| %.2e, max |shift difference| %.2e px, the same n_iter: %s" % (off, off_g, Bm, rel, rel_u, same_iter),
        "  F / Ps = %.2f (%.2f per evaluation of a tile); F / Fg = %.2f; H scaled to %d cutouts / F = %.0f; kernel times alone: "
        "profiles/prffit_kernel_stats.txt" % (med["F"] / med["Ps"], med["F"] / med["Ps"] / evals, med["F"] / med["Fg"], B,
                                              med["H"] * B / Bm / med["F"])])


def psffit(which):
    from concurrent.futures import ThreadPoolExecutor
    from scipy.special import erf
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(67)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma = 1.1
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))     # the true pointing of every cadence
    edges = np.arange(side + 1) - 0.5
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # every cadence rendered at its own shift
        gx = np.diff(erf((edges[None, None, :] - col[b][None, :, None] - shifts[0][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        gy = np.diff(erf((edges[None, None, :] - row[b][None, :, None] - shifts[1][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        img = 100.0 + np.einsum("s,nsy,nsx->nyx", rng.uniform(2000.0, 20000.0, S), gy, gx)
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)

    def fit():
        out = cubes.psf_fit(col, row, sigma)
        cubes.synchronize()
        return out

    def given():
        out = cubes.psf_photometry(col, row, sigma, shifts=d_shifts)
        cubes.synchronize()
        return out

    if "psffit_trace" in which:
        for _ in range(2):
            fit()
            given()
        return

    host_m = cubes.to_host()[:Bm]

    def mirror():
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda b: host_m[b].psf_fit(col[b], row[b], sigma), range(Bm)))

    fns = {"F": fit, "Rs": given, "H": mirror}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    lcs, info = first["F"]
    n_iter = info["n_iter"].download(np.int32, B * N, stream=lcs.stream).reshape(B, N)
    cstat = info["cadence_status"].download(np.int8, B * N, stream=lcs.stream).reshape(B, N)
    got = tuple(info[k].download(np.float64, B * N, stream=lcs.stream).reshape(B, N) for k in ("shift_col", "shift_row"))
    off = float(max(np.nanmax(np.abs(g - s)) for g, s in zip(got, shifts)))
    f = lcs.flux_host().reshape(B * S, N)[:Bm * S].reshape(Bm, S, N)
    h = np.stack([o["flux"] for o in first["H"]])
    rel = float(np.max(np.abs(f - h) / np.max(np.abs(h), axis=(1, 2), keepdims=True)))
    rel_u = float(max(np.max(np.abs(g[:Bm] - np.stack([o[k] for o in first["H"]]))) for g, k in zip(got, ("shift_col", "shift_row"))))
    same_iter = bool(np.array_equal(n_iter[:Bm], np.stack([o["n_iter"] for o in first["H"]])))
    first.clear()
    del lcs, info
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    evals = float(np.mean(np.max(np.pad(n_iter, ((0, 0), (0, -N % 16))).reshape(B, -1, 16), axis=2))) + 1
    write_walls("psffit_walls.txt", [
        "PSF fit with a pointing shift per cadence, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout, sigma %.1f px, true "
        "shifts uniform in +-0.3 px (%.1f MB of flux and flux_err resident, read once)" % (B, N, side, side, S, sigma, B * N * npix * 8 / 1e6),
        "  F    cubes.psf_fit(star_col, star_row, sigma), defaults, from shifts 0; everything resident                     %s" % spread(ts["F"]),
        "  Rs   cubes.psf_photometry(..., shifts=(DeviceBuffer, DeviceBuffer)) at the TRUE shifts, the same run            %s" % spread(ts["Rs"]),
        "  H    PixelCube.psf_fit on 16 threads, the first %d cutouts only                                                 %s" % (Bm, spread(ts["H"])),
        "  cadence statuses: %s; iterations per cadence: mean %.2f, max %d; evaluations per tile of 16 cadences (its slowest cadence + 1): "
        "mean %.2f" % (dict(zip(*(a.tolist() for a in np.unique(cstat, return_counts=True)))), float(n_iter.mean()), int(n_iter.max()), evals),
        "  largest |fitted - true shift| %.4f px; first %d cutouts against the mirror: max |flux difference| / max |flux| %.2e, max |shift "
        "difference| %.2e px, the same n_iter: %s" % (off, Bm, rel, rel_u, same_iter),
        "  F / Rs = %.2f (%.2f per evaluation of a tile); H scaled to %d cutouts / F = %.0f; kernel times alone: "
        "profiles/psffit_kernel_stats.txt" % (med["F"] / med["Rs"], med["F"] / med["Rs"] / evals, B, med["H"] * B / Bm / med["F"])])


def psfwidth(which):
    from concurrent.futures import ThreadPoolExecutor
    from scipy.special import erf
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(71)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma, sigma0 = 1.1, (1.1 * 1.15, 1.1 * 0.85)                        # the truth; the start, 15 % off on either side
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))     # the true pointing of every cadence, given
    edges = np.arange(side + 1) - 0.5
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # every cadence rendered at its own shift
        gx = np.diff(erf((edges[None, None, :] - col[b][None, :, None] - shifts[0][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        gy = np.diff(erf((edges[None, None, :] - row[b][None, :, None] - shifts[1][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        img = 100.0 + np.einsum("s,nsy,nsx->nyx", rng.uniform(2000.0, 20000.0, S), gy, gx)
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)
    tenth = np.zeros((B, N), dtype=bool)
    tenth[:, ::10] = True
    from lightkurve_amd.devmem import _upload
    d_tenth, keep = _upload(cubes.handle, tenth.astype(np.uint8), cubes.stream, np.uint8)
    block = np.zeros((B, N), dtype=bool)
    block[:, :N // 10] = True                                            # as many cadences, in whole tiles
    d_block, keep2 = _upload(cubes.handle, block.astype(np.uint8), cubes.stream, np.uint8)
    cubes.synchronize()
    del keep, keep2

    def width(mask=None):
        out = cubes.psf_width(col, row, sigma0, shifts=d_shifts, cadence_mask=mask, to_host=False)
        cubes.synchronize()
        return out

    def given():
        out = cubes.psf_photometry(col, row, sigma0, shifts=d_shifts)
        cubes.synchronize()
        return out

    if "psfwidth_trace" in which:
        for _ in range(2):
            width()
            width(d_tenth)
            width(d_block)
            given()
        return

    host_m = cubes.to_host()[:Bm]

    def mirror():
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda b: host_m[b].psf_width(col[b], row[b], sigma0, shifts=(shifts[0][b], shifts[1][b])), range(Bm)))

    fns = {"W": width, "Wm": lambda: width(d_tenth), "Wb": lambda: width(d_block), "Rs": given, "H": mirror}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    get = lambda out, k, dt, shape: out[k].download(dt, int(np.prod(shape)), stream=cubes.stream).reshape(shape)
    res = {k: (get(first[k], "status", np.int32, (B,)), get(first[k], "n_iter", np.int32, (B,)), get(first[k], "sigma", np.float64, (B, 2)),
               get(first[k], "sigma_err", np.float64, (B, 2))) for k in ("W", "Wm", "Wb")}
    status, n_iter, sg, sg_err = res["W"]
    h_sigma = np.stack([o["sigma"] for o in first["H"]])
    rel = float(np.max(np.abs(sg[:Bm] - h_sigma)))
    same_iter = bool(np.array_equal(n_iter[:Bm], [o["n_iter"] for o in first["H"]]))
    first.clear()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    evals = int(n_iter.max()) + 1                                        # passes in which a tile of the batch still works
    evals_m = int(res["Wm"][1].max()) + 1
    write_walls("psfwidth_walls.txt", [
        "PSF width per cutout, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout, true sigma %.1f px, sigma0 (%.3f, %.3f), "
        "true shifts uniform in +-0.3 px given (%.1f MB of flux and flux_err resident, read once per evaluation)"
        % (B, N, side, side, S, sigma, sigma0[0], sigma0[1], B * N * npix * 8 / 1e6),
        "  W    cubes.psf_width(star_col, star_row, sigma0, shifts=(DeviceBuffer, DeviceBuffer)), defaults; everything resident  %s" % spread(ts["W"]),
        "  Wm   the same with cadence_mask = every tenth cadence (DeviceBuffer)                                                 %s" % spread(ts["Wm"]),
        "  Wb   the same with cadence_mask = the first tenth of the cadences: the other tiles are left out entirely             %s" % spread(ts["Wb"]),
        "  Rs   cubes.psf_photometry(star_col, star_row, sigma0, shifts=) at the same shifts, the same run                      %s" % spread(ts["Rs"]),
        "  H    PixelCube.psf_width on 16 threads, the first %d cutouts only                                                    %s" % (Bm, spread(ts["H"])),
        "  W: statuses %s; updates per cutout: mean %.2f, max %d; evaluations made by the slowest cutout (updates + the final one): %d of "
        "the %d passes enqueued" % (dict(zip(*(a.tolist() for a in np.unique(status, return_counts=True)))), float(n_iter.mean()),
                                    int(n_iter.max()), evals, 21),
        "  Wm: statuses %s; evaluations made by the slowest cutout: %d"
        % (dict(zip(*(a.tolist() for a in np.unique(res["Wm"][0], return_counts=True)))), evals_m),
        "  largest |fitted - true sigma| %.5f px (W), %.5f px (Wm); mean sigma_err %.5f px (W), %.5f px (Wm); first %d cutouts against the "
        "mirror: max |sigma difference| %.2e px, the same n_iter: %s"
        % (float(np.nanmax(np.abs(sg - sigma))), float(np.nanmax(np.abs(res["Wm"][2] - sigma))), float(np.nanmean(sg_err)),
           float(np.nanmean(res["Wm"][3])), Bm, rel, same_iter),
        "  Wb: statuses %s; evaluations made by the slowest cutout: %d; W / Wb = %.2f"
        % (dict(zip(*(a.tolist() for a in np.unique(res["Wb"][0], return_counts=True)))), int(res["Wb"][1].max()) + 1, med["W"] / med["Wb"]),
        "  W / Rs = %.2f (%.2f per evaluation made); Wm / Rs = %.2f; H scaled to %d cutouts / W = %.0f; kernel times alone: "
        "profiles/psfwidth_kernel_stats.txt" % (med["W"] / med["Rs"], med["W"] / med["Rs"] / evals, med["Wm"] / med["Rs"], B,
                                                med["H"] * B / Bm / med["W"])])


def psfpos(which):
    from concurrent.futures import ThreadPoolExecutor
    from scipy.special import erf
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side, S = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11"),
                                                            ("LK_WALLS_STARS", "4")))
    reps, Bm = int(os.environ.get("LK_WALLS_REPS", "5")), min(B, int(os.environ.get("LK_WALLS_MIRROR_B", "16")))
    rng = np.random.default_rng(73)
    npix = side * side
    t = 1000.0 + np.arange(N) / 720.0                                    # two-minute cadences
    sigma, off = 1.1, 0.2                                                # the true width, given; the starts' distance from the truth
    cells = int(np.ceil(np.sqrt(S)))
    lattice = np.array([((i + 0.5) * side / cells - 0.5, (j + 0.5) * side / cells - 0.5) for j in range(cells) for i in range(cells)][:S])
    col = lattice[None, :, 0] + rng.uniform(-0.3, 0.3, (B, S))           # the truth
    row = lattice[None, :, 1] + rng.uniform(-0.3, 0.3, (B, S))
    col0, row0 = col + off * rng.choice([-1.0, 1.0], (B, S)), row + off * rng.choice([-1.0, 1.0], (B, S))
    shifts = (rng.uniform(-0.3, 0.3, (B, N)), rng.uniform(-0.3, 0.3, (B, N)))     # the true pointing of every cadence, given
    edges = np.arange(side + 1) - 0.5
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # every cadence rendered at its own shift
        gx = np.diff(erf((edges[None, None, :] - col[b][None, :, None] - shifts[0][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        gy = np.diff(erf((edges[None, None, :] - row[b][None, :, None] - shifts[1][b][:, None, None]) / (np.sqrt(2) * sigma)), axis=2) / 2
        img = 100.0 + np.einsum("s,nsy,nsx->nyx", rng.uniform(2000.0, 20000.0, S), gy, gx)
        flux[b] = img.astype(np.float32) + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    d_shifts = tuple(_upload_f64(cubes, a) for a in shifts)

    def positions():
        out = cubes.psf_positions(col0, row0, sigma, shifts=d_shifts, to_host=False)
        cubes.synchronize()
        return out

    def width():
        out = cubes.psf_width(col0, row0, sigma, shifts=d_shifts, to_host=False)
        cubes.synchronize()
        return out

    def given():
        out = cubes.psf_photometry(col0, row0, sigma, shifts=d_shifts)
        cubes.synchronize()
        return out

    if "psfpos_trace" in which:
        for _ in range(2):
            positions()
            width()
        return

    host_m = cubes.to_host()[:Bm]

    def mirror():
        with ThreadPoolExecutor(max_workers=16) as ex:
            return list(ex.map(lambda b: host_m[b].psf_positions(col0[b], row0[b], sigma, shifts=(shifts[0][b], shifts[1][b])), range(Bm)))

    fns = {"P": positions, "W": width, "Rs": given, "H": mirror}
    first = {k: fn() for k, fn in fns.items()}                           # warm-up of every route
    get = lambda out, k, dt, shape: out[k].download(dt, int(np.prod(shape)), stream=cubes.stream).reshape(shape)
    status, n_iter = get(first["P"], "status", np.int32, (B,)), get(first["P"], "n_iter", np.int32, (B,))
    pc, pr = get(first["P"], "star_col", np.float64, (B, S)), get(first["P"], "star_row", np.float64, (B, S))
    pe = get(first["P"], "star_col_err", np.float64, (B, S))
    w_iter = get(first["W"], "n_iter", np.int32, (B,))
    rel = float(max(np.max(np.abs(pc[:Bm] - np.stack([o["star_col"] for o in first["H"]]))),
                    np.max(np.abs(pr[:Bm] - np.stack([o["star_row"] for o in first["H"]])))))
    same_iter = bool(np.array_equal(n_iter[:Bm], [o["n_iter"] for o in first["H"]]))
    first.clear()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    evals, evals_w = int(n_iter.max()) + 1, int(w_iter.max()) + 1        # passes in which a tile of the batch still works
    write_walls("psfpos_walls.txt", [
        "Star positions per cutout, %d cutouts x %d cadences x %d x %d float32, %d stars per cutout (%d unknowns), sigma %.1f px given, "
        "starts %.1f px off per star and axis, true shifts uniform in +-0.3 px given (%.1f MB of flux and flux_err resident, read once "
        "per evaluation)" % (B, N, side, side, S, 2 * S, sigma, off, B * N * npix * 8 / 1e6),
        "  P    cubes.psf_positions(star_col, star_row, sigma, shifts=(DeviceBuffer, DeviceBuffer)), defaults; everything resident  %s" % spread(ts["P"]),
        "  W    cubes.psf_width(star_col, star_row, sigma, shifts=) on the same cubes at the same (offset) positions, the same run     %s" % spread(ts["W"]),
        "  Rs   cubes.psf_photometry(star_col, star_row, sigma, shifts=) likewise                                                     %s" % spread(ts["Rs"]),
        "  H    PixelCube.psf_positions on 16 threads, the first %d cutouts only                                                      %s" % (Bm, spread(ts["H"])),
        "  P: statuses %s; updates per cutout: mean %.2f, max %d; evaluations made by the slowest cutout (updates + the final one): %d of "
        "the %d passes enqueued; W: %d" % (dict(zip(*(a.tolist() for a in np.unique(status, return_counts=True)))), float(n_iter.mean()),
                                           int(n_iter.max()), evals, 21, evals_w),
        "  largest |fitted - true position| %.5f px; mean star_col_err %.5f px; first %d cutouts against the mirror: max |position "
        "difference| %.2e px, the same n_iter: %s" % (float(max(np.nanmax(np.abs(pc - col)), np.nanmax(np.abs(pr - row)))),
                                                      float(np.nanmean(pe)), Bm, rel, same_iter),
        "  P / Rs = %.2f (%.2f per evaluation made); W / Rs = %.2f (%.2f per evaluation made); P per evaluation / W per evaluation = %.2f "
        "(S = %d); H scaled to %d cutouts (measured on %d, not run on all) / P = %.0f; kernel times alone: profiles/psfpos_kernel_stats.txt"
        % (med["P"] / med["Rs"], med["P"] / med["Rs"] / evals, med["W"] / med["Rs"], med["W"] / med["Rs"] / evals_w,
           (med["P"] / evals) / (med["W"] / evals_w), S, B, Bm, med["H"] * B / Bm / med["P"])])


def _upload_f64(cubes, a):
    from lightkurve_amd.devmem import _upload
    buf, keep = _upload(cubes.handle, np.ascontiguousarray(a, dtype=np.float64), cubes.stream, np.float64)
    cubes.synchronize()
    del keep
    return buf


def background():
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd.device import DevicePixelCubeBatch
    B, N, side = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "500"), ("LK_WALLS_N", "4000"), ("LK_WALLS_SIDE", "11")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    rng = np.random.default_rng(43)
    t = 1000.0 + np.arange(N) / 48.0
    yy, xx = np.indices((side, side))
    c = side // 2
    star = (1000.0 * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / 1.62)).astype(np.float32)
    flux = np.empty((B, N, side, side), dtype=np.float32)
    for b in range(B):                                                  # (drawn per cutout: 1.9 GB of cubes in all)
        sky = (150.0 + 60.0 * np.sin(2 * np.pi * (t - t[0]) / 13.7 + b)).astype(np.float32)     # scattered light, per cadence
        flux[b] = star * np.float32(0.5 + rng.random()) + sky[:, None, None] + 3.0 * rng.standard_normal((N, side, side), dtype=np.float32)
    err = np.full_like(flux, 3.0)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(t, (B, 1)), flux, err)
    cubes.synchronize()
    del flux, err
    masks = cubes.estimate_background()["mask"]                          # the 'background' masks, made once for Fm / Em
    given = cubes.estimate_background(to_host=False)["flux"]             # a resident background for S

    def synced(fn):
        def run():
            out = fn()
            cubes.synchronize()
            return out
        return run

    def through_host():
        host = cubes.to_host()
        with ThreadPoolExecutor(max_workers=16) as ex:
            sub = list(ex.map(lambda c: c.subtract_background(), host))
        out = DevicePixelCubeBatch.from_cubes(sub)
        out.synchronize()
        return out

    fns = {"F": synced(lambda: cubes.subtract_background()), "Fm": synced(lambda: cubes.subtract_background(aperture_mask=masks)),
           "E": synced(lambda: cubes.estimate_background()), "Em": synced(lambda: cubes.estimate_background(masks)),
           "Es": synced(lambda: cubes.estimate_background(masks, return_scatter=True)),
           "S": synced(lambda: cubes.subtract_background(background=given)), "H": through_host}
    first = {}
    for k, fn in fns.items():                                            # warm-up of every route; F and H are compared below
        out = fn()
        if k in ("F", "H"):
            first[k] = [np.array(c.flux) for c in out.to_host()[::max(B // 8, 1)]]
        del out
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    cube_mb = B * N * side * side * 4 / 1e6
    same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first["F"], first["H"]))
    write_walls("background_walls.txt", [
        "per-cadence background, %d cutouts x %d cadences x %d x %d float32, 'background' masks of %d .. %d pixels (%.1f MB of flux; "
        "a fused call reads it once and writes it once)" % (B, N, side, side, masks.reshape(B, -1).sum(axis=1).min(),
                                                         masks.reshape(B, -1).sum(axis=1).max(), cube_mb),
        "  F    cubes.subtract_background(): median images, masks, estimate + subtraction in one launch, B x N values back  %s" % spread(ts["F"]),
        "  Fm   the same with the masks given (B, ny, nx): the fused launch and the B x N values back                      %s" % spread(ts["Fm"]),
        "  E    cubes.estimate_background(): median images, masks, estimate; flux and n_pixels on the host                 %s" % spread(ts["E"]),
        "  Em   the same with the masks given                                                                              %s" % spread(ts["Em"]),
        "  Es   Em with return_scatter=True                                                                                %s" % spread(ts["Es"]),
        "  S    cubes.subtract_background(background=DeviceBuffer): the streaming subtraction, B x N values back           %s" % spread(ts["S"]),
        "  H    to_host(), PixelCube.subtract_background per cutout on 16 threads, from_cubes                              %s" % spread(ts["H"]),
        "  F and H: the same subtracted pixels in every 1 of 8 cutouts compared: %s" % same,
        "  bytes / wall: Fm %.0f GB/s of %.1f MB, S %.0f GB/s of %.1f MB, Em %.0f GB/s of %.1f MB; H / F = %.1f; F - Fm = %.2f ms of masks"
        % (2 * cube_mb / 1e3 / med["Fm"], 2 * cube_mb, 2 * cube_mb / 1e3 / med["S"], 2 * cube_mb, cube_mb / 1e3 / med["Em"], cube_mb,
           med["H"] / med["F"], 1e3 * (med["F"] - med["Fm"]))])


def stitch(which=("stitch",)):
    from concurrent.futures import ThreadPoolExecutor
    from lightkurve_amd import _capi
    from lightkurve_amd.device import DeviceLightCurveBatch
    B, S, N = (int(os.environ.get(k, d)) for k, d in (("LK_WALLS_B", "1000"), ("LK_WALLS_SEGMENTS", "4"), ("LK_WALLS_N", "5000")))
    reps = int(os.environ.get("LK_WALLS_REPS", "5"))
    rng = np.random.default_rng(31)
    step = 2.0 / 1440.0 * 10.0                       # a 20-minute-like cadence [d]; one day between sectors
    day = int(round(1.0 / step))
    keep = rng.random((B * S, N)) >= 0.03
    keep[:, 0] = keep[:, -1] = True
    c_seg = (np.arange(S)[:, None] * (N + day) + np.arange(N)[None, :]).astype(np.int64)          # (S, N): continuing numbers
    cad = (100000 + np.tile(c_seg, (B, 1)))[keep].astype(np.int32)
    time = 1325.0 + step * cad * (1.0 + 1e-6 * np.sin(cad / 900.0))
    level = np.repeat(rng.uniform(800.0, 1200.0, B * S), keep.sum(axis=1))
    flux = level * (1.0 + 1e-3 * rng.standard_normal(cad.size))
    err = level * 1e-3
    n_off = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    group = np.repeat(np.arange(B), S)
    sync = _capi.Handle.get(0).synchronize

    def resident(noise_std="auto"):
        out = DeviceLightCurveBatch.from_arrays(time, flux, err, n_off, cadenceno=cad).stitch(group).fill_gaps(noise_std=noise_std)
        sync()
        return out

    # the same segments sector by sector (all targets' first sector, then their second, ...), as a survey delivers them: the groups
    # interleave, so the gather kernel moves every column
    order = np.arange(B * S).reshape(B, S).T.ravel()
    counts = np.diff(n_off)
    idx = np.concatenate([np.arange(n_off[s], n_off[s + 1]) for s in order])
    time_s, flux_s, err_s, cad_s = time[idx], flux[idx], err[idx], cad[idx]
    n_off_s = np.concatenate([[0], np.cumsum(counts[order])]).astype(np.int64)
    group_s = group[order]

    def resident_gather():
        out = DeviceLightCurveBatch.from_arrays(time_s, flux_s, err_s, n_off_s, cadenceno=cad_s).stitch(group_s).fill_gaps(noise_std="std")
        sync()
        return out

    def one(host, b, gen):
        ts, fs, es, cs = [], [], [], []
        for s in range(b * S, (b + 1) * S):                              # LightCurveCollection.stitch: normalize, then vstack
            a, z = int(host.n_off[s]), int(host.n_off[s + 1])
            f = host.flux[a:z]
            ok = ~np.isnan(f)
            med = np.median(f[ok])
            ts.append(host.time[a:z][ok]), fs.append(f[ok] / med), es.append(host.flux_err[a:z][ok] / med), cs.append(host.cadenceno[a:z][ok])
        t, f, e, c = (np.concatenate(x) for x in (ts, fs, es, cs))
        m = np.median(np.diff(t))                                        # LightCurve.fill_gaps, the cadence path
        cf = c.astype(np.float64)
        nc = np.arange(c[0], c[-1] + 1)
        ncf = nc.astype(np.float64)
        nt = np.interp(ncf, cf, t - m * cf) + m * ncf
        ins = np.ones(nc.size, dtype=bool)
        ins[c - c[0]] = False
        nf, ne = np.empty(nc.size), np.empty(nc.size)
        nf[~ins], ne[~ins] = f, e
        nf[ins] = gen.normal(np.nanmean(f), np.nanstd(f), int(ins.sum()))
        ne[ins] = np.interp(nt[ins], t, e)
        return nt, nf, ne, nc.astype(np.int32), ins

    def through_host(src):
        host = src.to_host()
        gens = [np.random.default_rng(1000 + b) for b in range(B)]
        with ThreadPoolExecutor(max_workers=16) as ex:
            parts = list(ex.map(lambda b: one(host, b, gens[b]), range(B)))
        off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
        out = DeviceLightCurveBatch.from_arrays(*(np.concatenate([p[k] for p in parts]) for k in range(3)), off,
                                                cadenceno=np.concatenate([p[3] for p in parts]))
        sync()
        return out, np.concatenate([p[4] for p in parts])

    if "stitch_trace" in which:
        for _ in range(4):
            resident("std")
        resident_gather()
        resident()
        print("stitch_trace: 4 resident from_arrays -> stitch -> fill_gaps(noise_std='std') calls, one on sector-major segments (gather) and one "
              "with the CDPP on %d x %d x %d"
              % (B, S, N))
        return
    src = DeviceLightCurveBatch.from_arrays(time, flux, err, n_off, cadenceno=cad)     # the resident segments the host route starts from
    src.synchronize()
    r, r2, g = resident(), resident("std"), resident_gather()           # warm-up of every route
    (h, h_ins) = through_host(src)
    R, R2, G, H = [], [], [], []
    for _ in range(reps):
        R.append(timed(resident)[0])
        R2.append(timed(lambda: resident("std"))[0])
        G.append(timed(resident_gather)[0])
        H.append(timed(lambda: through_host(src))[0])
    gather_same = all(np.array_equal(a, b) for a, b in ((g.n_off, r2.n_off), (g.time_host(), r2.time_host()),
                                                       (g.flux_host(), r2.flux_host()), (g.flux_err_host(), r2.flux_err_host()),
                                                       (g.cadenceno_host(), r2.cadenceno_host())))
    same_layout = np.array_equal(r.n_off, h.n_off) and np.array_equal(r.cadenceno_host(), h.cadenceno_host())
    rt, ht, re_, he, rf, hf = r.time_host(), h.time_host(), r.flux_err_host(), h.flux_err_host(), r2.flux_host(), h.flux_host()
    dt = float(np.max(np.abs(rt - ht) / np.spacing(np.abs(ht)))) if same_layout else np.nan
    de = float(np.nanmax(np.abs(re_ - he) / np.abs(he))) if same_layout else np.nan
    df = float(np.max(np.abs(rf[~h_ins] - hf[~h_ins]) / np.abs(hf[~h_ins]))) if same_layout else np.nan
    med = {k: float(np.median(v)) for k, v in (("R", R), ("R2", R2), ("H", H))}
    n_in, n_out = int(n_off[-1]), int(r.n_off[-1])
    write_walls("stitch_walls.txt", [
        "stitch + fill_gaps: %d targets x %d sectors x %d cadences, one day (%d cadences) between sectors, 3 %% missing inside: %d "
        "cadences in (%.0f MB of columns), %d out, %d inserted" % (B, S, N, day, n_in, n_in * 28 / 1e6, n_out, n_out - n_in),
        "  R   from_arrays(cadenceno=) -> stitch(group) -> fill_gaps() + synchronise (noise: resident CDPP)        %s" % spread(R),
        "  R'  the same with fill_gaps(noise_std='std')                                                            %s" % spread(R2),
        "  G   R' on the segments in sector-major order: the groups interleave, the gather kernel moves 5 columns   %s" % spread(G),
        "  H   to_host(), numpy normalize + concatenate + fill_gaps per target on 16 threads, from_arrays          %s" % spread(H),
        "  G and R': every column and offset bitwise equal: %s" % gather_same,
        "  R and H: same offsets and cadence numbers: %s; largest difference of the times %.2f ulp, of flux_err %.2e relative, of "
        "the originals' flux %.2e relative (R'); inserted flux: different generators, equal in distribution (std of the inserted "
        "flux R' %.3e, H %.3e)" % (same_layout, dt, de, df, float(np.std(rf[h_ins])) if same_layout else np.nan, float(np.std(hf[h_ins]))),
        "  H / R = %.2f; H / R' = %.2f; R / R' = %.2f (the CDPP: flatten + clip of every stitched target); kernels alone not measured"
        % (med["H"] / med["R"], med["H"] / med["R2"], med["R"] / med["R2"])])


def main():
    import torch  # noqa: F401  (before liblkhip.so)
    from lightkurve_amd import batch, synth
    from lightkurve_amd.lightcurve import LightCurve
    which = sys.argv[1:] or ["flatten", "regress", "pld", "bls"]
    if {"pld_dev", "pld_host", "pld_dev_trace"} & set(which):
        pld_dev(which)
    if "pld_ragged" in which:
        pld_ragged()
    if {"underfit", "underfit_trace"} & set(which):
        underfit(which)
    if {"overfit", "overfit_trace"} & set(which):
        overfit(which)
    if {"cbvopt", "cbvopt_trace"} & set(which):
        cbvopt(which)
    if "blsstats" in which:
        blsstats()
    if "clean" in which:
        clean()
    if "cdpp" in which:
        cdpp()
    if "prewhiten" in which:
        prewhiten()
    if "seismology" in which:
        seismology()
    if "sff" in which:
        sff()
    if "cbvragged" in which:
        cbvragged()
    if "cbvinterp" in which:
        cbvinterp()
    if "cbvroutes" in which:
        cbvroutes()
    if "underfit_ragged" in which:
        underfit_ragged()
    if "cbvopt_ragged" in which:
        cbvopt_ragged()
    if "foldbin" in which:
        foldbin()
    if "river" in which:
        river()
    if "diffimage" in which:
        diffimage()
    if "ampimage" in which:
        ampimage()
    if "background" in which:
        background()
    if {"psfphot", "psfphot_trace"} & set(which):
        psfphot(which)
    if {"prfphot", "prfphot_trace"} & set(which):
        prfphot(which)
    if {"prffit", "prffit_trace"} & set(which):
        prffit(which)
    if {"psffit", "psffit_trace"} & set(which):
        psffit(which)
    if {"psfwidth", "psfwidth_trace"} & set(which):
        psfwidth(which)
    if {"psfpos", "psfpos_trace"} & set(which):
        psfpos(which)
    if {"pixelpg", "pixelpg_trace"} & set(which):
        pixelpg(which)
    if {"stitch", "stitch_trace"} & set(which):
        stitch(which)
    if "flatten" in which:
        lcs = []
        for i in range(1000):
            t, y, e, _ = synth.ls_target(1, i, 20000)
            lcs.append(LightCurve(time=t, flux=1.0 + y, flux_err=e))
        ms, prof = wall(lambda: batch.flatten_batch(lcs, window_length=401))
        print("flatten_batch(1000 x 20000, window 401): %.1f ms per call (kernel alone 1.8 ms; 320 MB in, 160 MB out)\n%s\n" % (ms, prof))
    if "regress" in which:
        from lightkurve_amd.correctors import DesignMatrix
        rng = np.random.default_rng(2)
        lcs, dms = [], []
        for i in range(256):
            t, y, e, _ = synth.ls_target(1, i, 4000)
            X = np.column_stack([np.sin(2 * np.pi * t / p) for p in np.linspace(0.7, 12.0, 19)] + [np.ones(4000)])
            yr = 1 + X[:, :19] @ (1e-3 * rng.standard_normal(19)) + 3e-4 * rng.standard_normal(4000)
            lcs.append(LightCurve(time=t, flux=yr, flux_err=np.full(4000, 3e-4)))
            dms.append(DesignMatrix(X, name="X"))
        ms, prof = wall(lambda: batch.regression_correct_batch(lcs, dms))
        print("regression_correct_batch(256 x 4000 x K=20): %.1f ms per call\n%s\n" % (ms, prof))
    if "pld" in which:
        from lightkurve_amd.correctors.pldcorrector import PixelCube
        cubes = []
        for i in range(100):
            t, flux, err, _ = synth.pld_cutout(4, i, n=3500, npix=11)
            cubes.append(PixelCube(t, flux.astype(np.float32), err.astype(np.float32), mission="K2"))
        ms, prof = wall(lambda: batch.pld_correct_batch(cubes, pld_order=3, pca_components=16), reps=2)
        print("pld_correct_batch(100 cutouts x 3500 x 11 x 11): %.1f ms per call (device step: 6.8 ms per 100)\n%s\n" % (ms, prof))
    if "bls" in which:
        lcs = []
        for i in range(64):
            t, y, e, _ = synth.bls_target(3, i, 20000)
            lcs.append(LightCurve(time=t, flux=y, flux_err=e))
        periods = 1.0 / np.linspace(1 / 13.0, 1 / 0.6, 5000)[::-1]
        ms, prof = wall(lambda: batch.bls_batch(lcs, periods, duration=[0.05, 0.1, 0.2]))
        print("bls_batch(64 x 20000, 5000 periods x 3 durations): %.1f ms per call\n%s\n" % (ms, prof))


if __name__ == "__main__":
    main()
