"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the pre-filter kernels (pnr_amd/csrc/filter.hip), read from the
compiler's own resource report (-Rpass-analysis=kernel-resource-usage) with the mechanism of test_kernel_resources.py: no kernel
uses scratch, and the median kernels -- bound by instruction issue -- leave room for at least four waves per SIMD."""
import pytest
from test_kernel_resources import compile_isa


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "filter.hip")[0]


def test_every_filter_kernel_is_in_the_report(usage):
    for frag, count in (("median_k", 2), ("th_x", 2), ("th_col", 4)):
        hit = [k for k in usage if frag in k]
        assert len(hit) == count, (frag, sorted(usage))


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)


def test_median_leaves_four_waves_per_simd(usage):
    for name, u in usage.items():
        if "median_k" in name:
            assert u["VGPRs"] <= 128 and u.get("AGPRs", 0) == 0 and u["Occupancy"] >= 4, (name, u)
