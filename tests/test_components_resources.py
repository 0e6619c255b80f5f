"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the connected-component kernels (pnr_amd/csrc/components.hip), read
from the compiler's own resource report with the mechanism of test_kernel_resources.py: every kernel is there, none uses scratch, and
the local and merge kernels -- which wait on LDS and on atomics, so that only resident waves hide the latency -- leave room for at
least four waves per SIMD."""
import pytest
from test_kernel_resources import compile_isa

KERNELS = ("cc_local", "cc_merge", "cc_flatten", "cc_number", "cc_stats", "cc_finish")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "components.hip")[0]


def test_every_components_kernel_is_in_the_report(usage):
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)


def test_local_and_merge_leave_four_waves_per_simd(usage):
    for name, u in usage.items():
        if "cc_local" in name or "cc_merge" in name:
            assert u["Occupancy"] >= 4, (name, u)
