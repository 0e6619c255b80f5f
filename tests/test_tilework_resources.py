"""CPU (hipcc cross-compiles gfx950 without a GPU): the one compaction kernel of the flagged-tile relaxations (pnr_amd/csrc/tilework.hip),
read from the compiler's own resource report with the mechanism of test_kernel_resources.py: tile_compact is the only kernel of the
file, runs without scratch and light enough for eight waves per SIMD -- and the three tools that run on it carry no compaction kernel of
their own (their own reports: test_morph_resources.py, test_watershed_resources.py, test_geodesic_resources.py)."""
import pytest
from test_kernel_resources import compile_isa, find


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return compile_isa(tmp_path_factory, "tilework.hip")[0]


def test_the_compaction_is_the_only_kernel_without_scratch_at_eight_waves(usage):
    u, _ = find(usage, "tile_compact")
    assert len(usage) == 1, sorted(usage)
    assert u["ScratchSize"] == 0 and u["VGPRs"] <= 16 and u["Occupancy"] == 8, u
