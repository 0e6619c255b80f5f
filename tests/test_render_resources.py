"""CPU (hipcc cross-compiles gfx950 without a GPU): what the render kernels rest on, read from the compiler's own report
(-Rpass-analysis=kernel-resource-usage) and the ISA (-S): every kernel of render.hip is there and runs without scratch; rn_scatter reads
its item and its segment through scalar loads only -- the one vector load of its loop is the voxel's current label -- and ends in one
32-bit atomic minimum without a compare-and-swap loop; rn_finish reads the labels 16 bytes at a time and has no compare-and-swap loop
around its 64-bit adds."""
import pytest
from test_kernel_resources import compile_isa, find, kernel_body

KERNELS = ("rn_scatter", "rn_finish")  # (the byte sum behind thr = -1 is volume.hip's: test_volume_resources.py)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "render.hip")


def test_every_kernel_is_reported_without_scratch(compiled):
    usage, _ = compiled
    assert len(usage) == len(KERNELS), sorted(usage)
    for frag in KERNELS:
        u, _ = find(usage, frag)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u["Occupancy"] == 8, (frag, u)


def instructions(body):
    return [ln.split()[0] for ln in body if ln.startswith("\t") and not ln.startswith("\t.")]


def test_scatter_reads_item_and_segment_through_scalar_loads(compiled):
    usage, asm = compiled
    ins = instructions(kernel_body(usage, asm, "rn_scatter"))
    assert sum(i.startswith("s_load_dwordx4") or i.startswith("s_load_dwordx8") for i in ins) >= 3, ins  # two int4 of the item, three float4 of the segment
    vec = [i for i in ins if i.startswith(("global_load", "flat_load", "buffer_load", "ds_", "scratch_"))]
    assert vec == ["global_load_dword"], vec  # the current label
    atom = [i for i in ins if "atomic" in i]
    assert atom == ["global_atomic_umin"], atom
    assert not [i for i in ins if "cmpswap" in i]


def test_finish_reads_wide_and_adds_without_a_swap_loop(compiled):
    usage, asm = compiled
    ins = instructions(kernel_body(usage, asm, "rn_finish"))
    assert "global_load_dwordx4" in ins and "global_store_dwordx4" in ins
    assert [i for i in ins if "atomic" in i] and all(i.startswith("global_atomic_add_x2") for i in ins if "atomic" in i)
    assert not [i for i in ins if "cmpswap" in i]
