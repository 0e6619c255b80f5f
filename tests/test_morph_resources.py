"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the morphological reconstruction kernels (pnr_amd/csrc/morph.hip), read
from the compiler's own resource report with the mechanism of test_kernel_resources.py: every kernel is there exactly once, none uses
scratch, and the relaxation -- LDS latency bound, hidden only by resident waves -- leaves room for at least four waves per SIMD."""
import pytest
from test_kernel_resources import compile_isa

KERNELS = ("morph_init", "morph_relax", "morph_finish")  # (the compaction is tilework.hip's: test_tilework_resources.py)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "morph.hip")[0]


def test_every_morph_kernel_is_in_the_report(usage):
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch(usage):
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)


def test_the_relaxation_leaves_four_waves_per_simd(usage):
    hit = [u for name, u in usage.items() if "morph_relax" in name]
    assert len(hit) == 1 and hit[0]["Occupancy"] >= 4, hit
