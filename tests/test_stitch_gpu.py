"""GPU: ``DeviceLightCurveBatch.stitch`` (``lk_gather_segments_batch_dev``) against numpy concatenation.

Seven light curves with 0, 1, 64, 65, 1500, 300 and 300 cadences in three groups that interleave in batch order; with and
without flux_err / quality / cadence numbers; ``corrector=None`` and ``"normalize"`` (the latter must be this class's
``normalize()`` per segment bit for bit); ``order="given"`` and ``"start_time"``.  A stitch only moves numbers: every column and
every offset is exact.  Then the chain the feature exists for: stitch -> fill_gaps by cadence number -> flatten -> periodogram."""
import functools

import numpy as np
import pytest

from lightkurve_amd import device as D
from lightkurve_amd.device import DeviceLightCurveBatch
from lightkurve_amd.ingest import LightCurveBatch

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 64, 65, 1500, 300, 300)
GROUP = (4, 9, 4, 2, 9, 2, 4)                    # -> targets 0 (4), 1 (9), 2 (2) by first appearance
START = (0.0, 30.0, 50.0, 0.0, 5.0, 20.0, 10.0)  # first time of every segment (step 0.01 d): no two segments of a target overlap
GIVEN = ((0, 2, 6), (1, 4), (3, 5))              # the segments of every target in batch order
BY_START = ((6, 2, 0), (4, 1), (3, 5))           # ... by their first time, the empty one last


@functools.lru_cache(maxsize=None)
def segments():
    out = []
    for s, n in enumerate(LENGTHS):
        rng = np.random.default_rng(40 + s)
        t = START[s] + 0.01 * np.arange(n)
        f = (100.0 + 50.0 * s) * (1.0 + 0.01 * rng.standard_normal(n))
        if n > 100:
            f[rng.choice(n, 5, replace=False)] = np.nan        # normalize() drops these
        e = 0.5 + 0.1 * rng.random(n)
        q = rng.integers(0, 1 << 12, n).astype(np.int32)
        c = (1000 * s + np.arange(n)).astype(np.int32)
        out.append(dict(time=t, flux=f, flux_err=e, quality=q, cadenceno=c))
    return tuple(out)


def _device(order=tuple(range(len(LENGTHS))), with_err=True, with_quality=True, with_cad=True):
    segs = [segments()[s] for s in order]
    n_off = np.concatenate([[0], np.cumsum([len(x["time"]) for x in segs])]).astype(np.int64)
    cat = lambda k: np.concatenate([x[k] for x in segs])      # noqa: E731
    meta = [{"SEGMENT": int(s)} for s in order]
    b = DeviceLightCurveBatch.from_arrays(cat("time"), cat("flux"), cat("flux_err") if with_err else None, n_off, meta=meta,
                                          cadenceno=cat("cadenceno") if with_cad else None)
    if with_quality:
        b.d_quality, k = D._upload(b.handle, cat("quality"), b.stream, np.int32)
        b._keep.append(k)
    return b


def _columns(b):
    return dict(time=b.time_host(), flux=b.flux_host(), flux_err=b.flux_err_host(), quality=b.quality_host(),
                cadenceno=b.cadenceno_host())


def _check(out, src, order_of, what):
    """``out`` against the numpy concatenation of the light curves of ``src`` (a batch with the 7 segments in batch order)."""
    got, col = _columns(out), _columns(src)
    want_off = [0]
    for k in col:
        if col[k] is None:
            assert got[k] is None, "%s: column %s must not appear" % (what, k)
            continue
        parts = [col[k][src.n_off[s]:src.n_off[s + 1]] for segs in order_of for s in segs]
        want = np.concatenate(parts)
        diff = int(np.sum(~((got[k] == want) | ((got[k] != got[k]) & (want != want)))))
        print("%s, %s: %d of %d values differ" % (what, k, diff, want.size))
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want, equal_nan=want.dtype.kind == "f"), (what, k)
    for segs in order_of:
        want_off.append(want_off[-1] + sum(int(src.n_off[s + 1] - src.n_off[s]) for s in segs))
    assert np.array_equal(out.n_off, want_off), what
    assert [m["STITCHED_FROM"] for m in out.meta] == [list(segs) for segs in order_of]
    assert [m.get("SEGMENT") for m in out.meta] == [segs[0] for segs in order_of]


@pytest.mark.parametrize("corrector", [None, "normalize"])
@pytest.mark.parametrize("order", ["given", "start_time"])
@pytest.mark.parametrize("with_err,with_quality,with_cad", [(True, True, True), (False, False, False), (True, False, True)])
def test_stitch_is_numpy_concatenation(corrector, order, with_err, with_quality, with_cad):
    b = _device(with_err=with_err, with_quality=with_quality, with_cad=with_cad)
    out = b.stitch(GROUP, corrector=corrector, order=order)
    src = b.normalize() if corrector == "normalize" else b           # this class's normalize() per segment, bit for bit
    _check(out, src, GIVEN if order == "given" else BY_START, "stitch(%s, %s)" % (corrector, order))
    assert len(out) == 3 and out.median_flux is None
    assert out.nan_free == (corrector == "normalize")
    assert all(bool(m.get("NORMALIZED")) == (corrector == "normalize") for m in out.meta)
    # ordered, non-overlapping segments are sorted; target 0 in batch order has its later segment first
    assert out.is_sorted == (order == "start_time")


def test_contiguous_groups_share_the_columns_and_equal_the_gather_route():
    flat = tuple(s for segs in GIVEN for s in segs)                   # the batch already in stitched order
    labels = [g for g, segs in enumerate(GIVEN) for _ in segs]
    for corrector in (None, "normalize"):
        shared_src = _device(order=flat)
        shared = shared_src.stitch(labels, corrector=corrector)
        gathered = _device().stitch(GROUP, corrector=corrector)
        if corrector is None:
            assert shared.d_time is shared_src.d_time and shared.d_flux is shared_src.d_flux      # no data moved
        a, g = _columns(shared), _columns(gathered)
        for k in a:
            assert np.array_equal(a[k], g[k], equal_nan=a[k].dtype.kind == "f"), (corrector, k)
        assert np.array_equal(shared.n_off, gathered.n_off)
        assert [m["STITCHED_FROM"] for m in shared.meta] == [[0, 1, 2], [3, 4], [5, 6]]
    print("contiguous route == gather route, bitwise")


def test_group_none_is_one_target_and_sorted_probe():
    b = _device()
    one = b.stitch(corrector=None)
    assert len(one) == 1 and np.array_equal(one.n_off, [0, b.n_cadences])
    assert one.meta[0]["STITCHED_FROM"] == list(range(7)) and one.d_time is b.d_time
    assert one.is_sorted is False                                   # 30, then 50 .., then 0 ..: the time steps back
    ordered = b.stitch(corrector=None, order="start_time")
    assert ordered.is_sorted is False                               # segment 6 (10 .. 13) starts inside segment 4 (5 .. 20)
    two = _device(order=(3, 5)).stitch(corrector=None)
    assert two.is_sorted is True and len(two) == 1


def test_stitch_fill_gaps_flatten_periodogram_chain():
    """Two targets, three sectors each, cadence numbers continuing across a 50-cadence gap between sectors and a few cadences
    missing inside: stitch + fill_gaps gives one even cadence grid per target, and the usual chain runs on it."""
    rng = np.random.default_rng(3)
    n_seg, gap, step = 400, 50, 0.02
    t, f, e, c, off, group = [], [], [], [], [0], []
    for target in range(2):
        for s in range(3):
            cad = 5000 * target + s * (n_seg + gap) + np.arange(n_seg)
            keep = np.ones(n_seg, dtype=bool)
            keep[rng.choice(np.arange(1, n_seg - 1), 7, replace=False)] = False
            cad = cad[keep]
            tt = step * cad
            t.append(tt), c.append(cad.astype(np.int32))
            f.append((1000.0 + 300.0 * s) * (1.0 + 0.01 * np.sin(2 * np.pi * tt / 1.7) + 1e-3 * rng.standard_normal(cad.size)))
            e.append(np.full(cad.size, 1.0))
            off.append(off[-1] + cad.size)
            group.append(target)
    b = DeviceLightCurveBatch.from_arrays(np.concatenate(t), np.concatenate(f), np.concatenate(e), off, cadenceno=np.concatenate(c))
    even = b.stitch(group).fill_gaps(seed=1)
    span = 3 * n_seg + 2 * gap
    assert np.array_equal(even.n_off, [0, span, 2 * span])
    cad = even.cadenceno_host().reshape(2, span)
    assert np.array_equal(cad, np.array([[0], [5000]]) + np.arange(span))
    time = even.time_host().reshape(2, span)
    print("even grid: max |time - step * c| %.3g" % np.max(np.abs(time - step * cad)))
    assert np.allclose(time, step * cad, rtol=0, atol=1e-9)
    flux = even.flux_host()
    assert np.all(np.isfinite(flux)) and abs(np.median(flux) - 1.0) < 0.01       # normalised sectors, noise around their mean
    peaks = even.flatten(101).to_periodogram_peaks(np.arange(1, 400) * 0.01)
    assert peaks.shape == (2, 2) and np.all(np.isfinite(peaks))
    print("periodogram peaks", peaks.ravel())


def test_host_mirror_of_stitch():
    segs = segments()
    n_off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    cat = lambda k: np.concatenate([x[k] for x in segs])      # noqa: E731
    hb = LightCurveBatch(cat("time"), cat("flux"), cat("flux_err"), n_off)
    hb.quality, hb.cadenceno = cat("quality"), cat("cadenceno")
    got = hb.stitch(GROUP, order="start_time")
    want = _device().stitch(GROUP, order="start_time")
    w = _columns(want)
    for k in w:
        assert np.array_equal(getattr(got, k), w[k], equal_nan=w[k].dtype.kind == "f"), k
    assert np.array_equal(got.n_off, want.n_off) and [m["STITCHED_FROM"] for m in got.meta] == [list(s) for s in BY_START]
