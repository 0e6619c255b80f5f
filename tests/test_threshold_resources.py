"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the threshold kernels (pnr_amd/csrc/threshold.hip), read from the
compiler's own resource report with the mechanism of test_kernel_resources.py: every kernel is there exactly once and none uses
scratch."""
import pytest
from test_kernel_resources import compile_isa

KERNELS = ("thr_hist", "lt_x", "lt_y", "lt_z")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "threshold.hip")[0]


def test_every_threshold_kernel_is_in_the_report(usage):
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
