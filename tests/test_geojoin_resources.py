"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the two meet kernels of pnr_geodesic_bridges (pnr_amd/csrc/geojoin.hip),
read from the compiler's own resource report with the mechanism of test_kernel_resources.py: exactly the two kernels are there, and
neither uses scratch.  (What the compiler reports for registers, LDS and occupancy is written down in DESIGN.md, not pinned.)"""
import pytest
from test_kernel_resources import compile_isa

KERNELS = ("gj_meet_w", "gj_meet_e")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "geojoin.hip")[0]


def test_exactly_the_two_meet_kernels_are_in_the_report(usage):
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        print(name, u)
