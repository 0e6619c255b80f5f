"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the distance-transform kernels (pnr_amd/csrc/edt.hip), read from the
compiler's own resource report with the mechanism of test_kernel_resources.py: every kernel is there exactly once, none uses scratch, and
the three passes -- memory bound, so that only resident waves hide the latency -- leave room for at least four waves per SIMD."""
import pytest
from test_kernel_resources import compile_isa

KERNELS = ("edt_x", "edt_y", "edt_z", "edt_stats", "edt_sample")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "edt.hip")[0]


def test_every_edt_kernel_is_in_the_report(usage):
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)


def test_the_passes_leave_four_waves_per_simd(usage):
    for name, u in usage.items():
        if any(k in name for k in ("edt_x", "edt_y", "edt_z")):
            assert u["Occupancy"] >= 4, (name, u)
