"""CPU: bench.py's options.  A plain run times the headline alone, `--full` keeps every other block on, and
`--dump-outputs` keeps a seeded sample of an output larger than its share of 64 MB and writes finite values only."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_options", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_times_the_headline_alone_and_full_keeps_the_rest():
    bench = _bench()
    plain = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (plain.steps, plain.warmup, plain.full, plain.dump_outputs) == (7, 2, False, None)
    assert plain.no_cpu_baseline and plain.no_bls and plain.no_pld and plain.no_flatten and plain.no_host
    assert plain.no_api and plain.no_pipeline and plain.c2_targets == 0 and plain.repeats == 1 and plain.ls_method == "fast"
    full = bench.parse(["--full"])
    assert not (full.no_cpu_baseline or full.no_bls or full.no_pld or full.no_flatten or full.no_host or full.no_api
                or full.no_pipeline)
    assert full.c2_targets == 10000 and full.repeats == 5 and full.ls_method == "both"
    # the headline metric names the BLS block in both, as it did before --full existed
    assert plain.metric_bls and full.metric_bls and not bench.parse(["--full", "--no-bls"]).metric_bls
    # --workload api: the API block is the headline, so a plain run keeps it
    assert not bench.parse(["--workload", "api"]).no_api


def test_dump_sample_is_capped_seeded_and_float():
    bench = _bench()
    big = torch.arange(10_000_000, dtype=torch.float64)
    small = torch.arange(1000, dtype=torch.int64).reshape(10, 100)
    a = bench.sample_outputs([("big", big), ("small", small), ("mask", torch.ones(5, dtype=torch.uint8))])
    b = bench.sample_outputs([("big", big), ("small", small), ("mask", torch.ones(5, dtype=torch.uint8))])
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(a["big"], b["big"]) and np.all(np.diff(a["big"]) > 0)   # same sorted flat indices every run
    assert a["small"].shape == (10, 100) and a["small"].dtype == np.float64 and np.array_equal(a["small"].ravel(), np.arange(1000))
    assert a["mask"].dtype == np.float64
    assert bench.sample_outputs([("f", torch.zeros(3, dtype=torch.float32))])["f"].dtype == np.float32


def test_dump_values_are_finite_and_non_finite_ones_are_recorded():
    bench = _bench()
    p = torch.tensor([[1.0, float("nan"), 2.0], [float("inf"), 3.0, float("-inf")]], dtype=torch.float64)
    d = bench.sample_outputs([("power", p), ("clean", torch.ones(4, dtype=torch.float64))])
    assert sorted(d) == ["clean", "power", "power_nonfinite"]
    assert all(np.all(np.isfinite(a)) for a in d.values())
    assert np.array_equal(d["power"], [[1.0, 0.0, 2.0], [0.0, 3.0, 0.0]])
    assert np.array_equal(d["power_nonfinite"], [[1, 0], [3, 1], [5, -1]])
    # a sampled output whose every element is NaN still fits the budget with its record
    d = bench.sample_outputs([("nan", torch.full((20_000_000,), float("nan"), dtype=torch.float64))])
    assert sum(a.nbytes for a in d.values()) <= bench.DUMP_LIMIT_BYTES and not np.any(d["nan"])
