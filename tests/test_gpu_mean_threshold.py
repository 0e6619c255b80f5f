"""The one threshold rule "thr = -1" (pnr_mean_threshold, volume.hip) behind measure_radii, tree_coverage and label_components: on the
same borrowed volume all three report thr_used = max(1, floor of the exact mean).  Integer-exact: no tolerance.

The shapes (w x h x l) are where the byte sum vol_sum can go wrong: fewer than 16 bytes (head and tail only), exactly one 16-byte vector,
one vector and a tail, several work-groups, more than 2048 x 256 x 16 bytes (the grid-stride loop iterates), and a sum above 2^32; the
byte shifts move the scalar head of the sum.  label_components is called with cap=0: one library call, as the other two (the default
cap=None calls the library a second time for the component list, which would sum again)."""
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1), (5, 3, 1), (4, 4, 1), (3, 3, 2), (64, 64, 33), (256, 256, 129)]  # (w, h, l)
FULL = (512, 512, 65)  # filled with 255: the sum is 4 345 036 800 > 2^32
GROUPS = {"radius": 1, "render_finish": 2, "components_threshold": 1}  # launches of one trio of calls: the sum; the sum + rn_finish; the sum


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    # the shell table of measure_radii stays cached in the context (grow-only): sized here, by the larger 3-D table, not inside a case
    c.set_volume(np.zeros((2, 2, 2), np.uint8))
    c.measure_radii(np.zeros((0, 3), np.float32), thr=-1, rel_pct=0)
    c.set_profiling(True)
    yield c
    c.close()


def trio(ctx, V, shift):
    """the three thr_used on V borrowed at byte `shift` of a torch buffer; timers and live bytes checked on the way"""
    import torch
    l, h, w = V.shape
    flat = torch.empty(shift + V.size + 16, dtype=torch.uint8, device="cuda")
    flat[shift:shift + V.size] = torch.from_numpy(V.reshape(-1)).cuda()
    torch.cuda.synchronize()
    ctx.set_volume_device(flat.data_ptr() + shift, (l, h, w), keepalive=flat)
    ctx.reset_kernel_ms()
    before = lib.live_bytes()
    none = np.zeros((0, 3), np.float32)
    got = (ctx.measure_radii(none, thr=-1, rel_pct=0)[1], ctx.tree_coverage(none, [], [], thr=-1)["thr_used"],
           ctx.label_components(thr=-1, labels=False, cap=0)[0]["thr_used"])
    assert lib.live_bytes() == before
    counts = {g: ctx.kernel_ms(g)[1] for g in GROUPS}
    print("thr_used", got, "launches", counts)
    assert counts == GROUPS
    return got


@pytest.mark.parametrize("shift", [0, 1, 15])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_three_tools_one_threshold(ctx, shape, shift):
    w, h, l = shape
    V = np.random.default_rng(w * 1000 + l).integers(0, 256, (l, h, w), dtype=np.uint8)
    want = max(1, int(V.sum(dtype=np.int64)) // V.size)
    assert trio(ctx, V, shift) == (want, want, want)


def test_sum_above_2_to_32(ctx):
    w, h, l = FULL
    V = np.full((l, h, w), 255, np.uint8)
    want = max(1, int(V.sum(dtype=np.int64)) // V.size)
    assert int(V.sum(dtype=np.int64)) == 4345036800 and want == 255
    assert trio(ctx, V, 0) == (want, want, want)
