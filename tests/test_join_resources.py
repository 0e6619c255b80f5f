"""CPU (hipcc cross-compiles gfx950 without a GPU): what the join's inner loop rests on, read from the compiler's own report
(-Rpass-analysis=kernel-resource-usage) and the ISA (-S) -- what the tree distance's kernels are held to: pair_min<JoinRule> (pairmin.h)
runs eight waves per SIMD without scratch or LDS, fetches its targets with scalar loads only (one 16-byte load per target, four targets
in one 64-byte load where the loop is unrolled), spends at most 12 vector instructions per (point, target) pair (11 measured), and ends in
one 64-bit atomic minimum without a compare-and-swap loop."""
import pytest
from test_kernel_resources import compile_isa, find, kernel_body
from test_distance_resources import inner_loops


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "join.hip")


def test_budgets(compiled):
    usage, _ = compiled
    for frag in ("join_prep", "pair_min", "pair_finish"):
        u, _ = find(usage, frag)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u["Occupancy"] == 8 and u["LDS"] == 0, (frag, u)


def test_inner_loop_reads_targets_through_scalar_loads(compiled):
    usage, asm = compiled
    assert "JoinRule" in find(usage, "pair_min")[1]
    body = kernel_body(usage, asm, "pair_min")
    loops = inner_loops(body)
    assert len(loops) == 2, len(loops)  # the loop unrolled by four and its remainder
    for ins in loops:
        pairs = 4 * sum(i == "s_load_dwordx16" for i in ins) + sum(i == "s_load_dwordx4" for i in ins)
        valu = sum(i.startswith("v_") for i in ins)
        assert pairs in (1, 4) and sum(i.startswith("s_load") for i in ins) == 1, ins
        assert not [i for i in ins if i.startswith(("global_", "flat_", "buffer_", "ds_", "scratch_"))], ins
        assert valu <= 12 * pairs, (valu, pairs)
    atom = [ln for ln in body if "atomic" in ln]
    assert len(atom) == 1 and "global_atomic_umin_x2" in atom[0], atom
    assert not [ln for ln in body if "cmpswap" in ln]
