"""CPU (hipcc cross-compiles gfx950 without a GPU): the budgets of the pruning kernels (pnr_amd/csrc/prune.hip), read from the compiler's
own resource report and the ISA with the mechanism of test_kernel_resources.py: every kernel without scratch and LDS at eight waves
per SIMD, the height and continuing-child kernels ending in ONE native atomic max (no compare-and-swap loop anywhere), and a jump
that costs two 8-byte loads and one 8-byte store per node."""
import re
import pytest
from test_kernel_resources import compile_isa, kernel_body

KERNELS = ("prune_edges", "prune_up", "prune_child", "prune_down_init", "prune_downE", "prune_finish")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "prune.hip")


def test_every_prune_kernel_is_in_the_report(compiled):
    usage, _ = compiled
    for frag in KERNELS:
        hit = [k for k in usage if frag in k]
        assert len(hit) == 1, (frag, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_scratch_no_lds_eight_waves(compiled):
    usage, _ = compiled
    assert usage
    for name, u in usage.items():
        assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["Occupancy"] == 8, (name, u)


def _ops(body, pattern):
    return [ln.split()[0] for ln in body if re.match(r"\s+" + pattern, ln)]


def test_one_atomic_max_and_no_compare_and_swap(compiled):
    usage, asm = compiled
    assert not [ln for ln in asm if "cmpswap" in ln]
    for frag, op in (("prune_up", "global_atomic_umax"), ("prune_child", "global_atomic_umax_x2")):
        body = kernel_body(usage, asm, frag)
        atomics = _ops(body, r"(global|flat|buffer)_atomic")
        assert atomics == [op], (frag, atomics)
        after = _ops(body[next(i for i, ln in enumerate(body) if op in ln) + 1:], r"(global|flat|buffer|scratch)_(load|store|atomic)")
        assert not after, (frag, after)  # the kernel ends in it


def test_a_jump_is_two_8_byte_loads_and_one_8_byte_store(compiled):
    usage, asm = compiled
    for frag in ("prune_up", "prune_downE"):
        body = kernel_body(usage, asm, frag)
        assert len(_ops(body, r"global_load_dwordx2")) <= 2 and len(_ops(body, r"global_store_dwordx2")) == 1, frag
        assert not _ops(body, r"global_(load|store)_dwordx[34]"), frag
