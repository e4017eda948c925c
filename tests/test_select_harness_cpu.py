"""CPU: tests/select_harness.hip — the test-only driver of lightkurve_amd/csrc/block_select.hpp — compiles for gfx950 against the
header as it is now and exports its entry points (hipcc cross-compiles; no GPU, no launch).  Keeps the harness from rotting when
the header changes on a machine without a GPU; tests/test_block_select_gpu.py runs it."""
from tests import select_harness as SH


def test_harness_compiles_and_exports_its_entry_points(tmp_path):
    lib = SH.load(SH.compile_harness(tmp_path))
    for name in SH.ENTRY_POINTS:
        assert hasattr(lib, name), name
    names = SH.route_names()
    assert lib.selh_route_count() == len(names) == len(set(names)) <= 32   # one bit of the route word per enum value
    assert lib.selh_prob_size() == SH.PROB.itemsize
    # the release build of the header sees no hook: the macro is defined empty unless the includer defines it
    src = open(SH.CSRC + "/block_select.hpp").read()
    assert "#ifndef LK_SEL_ROUTE\n#define LK_SEL_ROUTE(id) ((void)0)\n#endif" in src
    assert "LK_SEL_ROUTE" not in "".join(open(SH.CSRC + "/" + f).read() for f in ("flatten.hip", "regress.hip", "ingest.hip",
                                                                                 "device.hip", "pgsmooth.hip"))
    # preconditions are refused on the host, before any device call: a rank outside the kept values, a block that is no multiple of 64
    import numpy as np
    h = SH.Harness(SH.compile_harness(tmp_path))
    import pytest
    with pytest.raises(RuntimeError):
        h.select(SH.OP_KTH, 256, 4096, h.pack([SH.Problem(np.arange(10.0), k=10)]))
    with pytest.raises(RuntimeError):
        h.select(SH.OP_KTH, 100, 4096, h.pack([SH.Problem(np.arange(10.0), k=3)]))
    with pytest.raises(RuntimeError):
        h.select(SH.OP_MEDIAN, 256, 4096, h.pack([SH.Problem(np.array([1.0, np.nan]))]))
    with pytest.raises(RuntimeError):
        h.sort(256, np.zeros((1, 48), np.uint64))
