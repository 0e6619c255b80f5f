"""CPU (hipcc cross-compiles gfx950 without a GPU): what the tree distance's inner loop rests on, read from the compiler's own report
(-Rpass-analysis=kernel-resource-usage) and the ISA (-S): pair_min<DistRule> (pairmin.h) runs eight waves per SIMD without scratch, fetches its segments
with scalar loads only (the segment index is wave-uniform: no vector load and no LDS access inside the loop), spends at most 24 vector
instructions per (point, segment) pair, and ends in one 64-bit atomic minimum without a compare-and-swap loop."""
import pytest
from test_kernel_resources import compile_isa, find, kernel_body


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "distance.hip")


def test_budgets(compiled):
    usage, _ = compiled
    for frag in ("dist_prep", "pair_min", "pair_finish"):
        u, _ = find(usage, frag)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u["Occupancy"] == 8 and u["LDS"] == 0, (frag, u)


def inner_loops(body):
    loops, cur = [], None
    for ln in body:  # the instructions of every innermost loop: from its header to its backward branch
        if ln.startswith(".LBB"):
            cur = None
            if "Inner Loop Header" in ln:
                cur = []
                loops.append(cur)
        elif cur is not None and ln.startswith("\t") and not ln.startswith("\t."):
            cur.append(ln.split()[0])
            if cur[-1].startswith("s_cbranch"):
                cur = None
    return loops


def test_inner_loop_reads_segments_through_scalar_loads(compiled):
    usage, asm = compiled
    assert "DistRule" in find(usage, "pair_min")[1]
    body = kernel_body(usage, asm, "pair_min")
    loops = inner_loops(body)
    assert len(loops) == 2, len(loops)  # the loop unrolled by four and its remainder
    for ins in loops:
        pairs = sum(i == "s_load_dwordx8" for i in ins)  # one scalar load of 32 bytes per segment
        valu = sum(i.startswith("v_") for i in ins)
        assert pairs in (1, 4), ins
        assert not [i for i in ins if i.startswith(("global_", "flat_", "buffer_", "ds_", "scratch_"))], ins
        assert valu <= 24 * pairs, (valu, pairs)
    atom = [ln for ln in body if "atomic" in ln]
    assert len(atom) == 1 and "global_atomic_umin_x2" in atom[0], atom
    assert not [ln for ln in body if "cmpswap" in ln]
