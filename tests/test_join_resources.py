"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the join's kernels, read from the compiler's own report
(-Rpass-analysis=kernel-resource-usage) -- the ones the tree distance's kernels are held to: eight waves per SIMD, no scratch, no LDS."""
import pytest
from test_kernel_resources import compile_isa, find


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "join.hip")


def test_budgets(compiled):
    usage, _ = compiled
    for frag in ("join_prep", "join_min", "join_finish"):
        u, _ = find(usage, frag)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u["Occupancy"] == 8 and u["LDS"] == 0, (frag, u)
