"""GPU parity of what the seed stage hands from the device to the host's flood fill (test tap pnr_seed_handover: layer_minmax,
layer_maxima<COUNT / WRITE>, row_scan, the chunked download and LayerFinder::load / restore) against the numpy reference of
tests/seeds_ref.py, at the shapes where the index arithmetic of those kernels changes.  Integer and byte work: everything exact."""
import numpy as np
import pytest
import pnr_amd
import seeds_ref as sr

pytestmark = pytest.mark.gpu

CASES = [(s, k) for s in sr.SHAPES for k in sr.KINDS]


def assert_handover(got, J8, what=""):
    """got: Context.seed_handover of the layers J8 (n, h, w)"""
    ref = sr.handover(J8)
    for k in ("vmin", "vmax", "ltot"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.flatnonzero(got[k] != ref[k])[:8], got[k][:8], ref[k][:8])
    bad = np.flatnonzero((got["layers"] != J8).reshape(len(J8), -1).any(1))
    assert len(bad) == 0, (what, "rebuilt layers differ", bad[:8], np.argwhere(got["layers"][bad[0]] != J8[bad[0]])[:4])
    assert np.array_equal(got["key_off"], ref["key_off"]), (what, "key_off", got["key_off"][:8], ref["key_off"][:8])
    assert np.array_equal(got["keys"], ref["keys"]), (what, "keys")
    assert got["restored"].all(), (what, "restore left pixels behind in layers", np.flatnonzero(got["restored"] == 0)[:8])


@pytest.fixture(scope="module")
def ctx():
    """one context for all the shapes: its scratch and pinned buffers are reused from stack to stack, as in a long-lived host"""
    c = pnr_amd.Context(pnr_amd.make_params(), 0)
    yield c
    c.close()


def load_stack(c, J8):
    if c.shape != J8.shape:
        c.set_volume(np.zeros(J8.shape, np.uint8))  # dimensions only
    z = np.zeros(J8.shape, np.uint8)
    c.set_j8_v(J8, z, z, z)


@pytest.mark.parametrize("shape,kind", CASES, ids=["%s-%s" % (sr.shape_id(s), k) for s, k in CASES])
def test_handover_matches_reference(ctx, shape, kind):
    J8 = sr.stack(shape, kind)
    if shape[0] < 2 or shape[1] < 2:  # the library takes no volume under 2 x 2 x 1: there is no layer to hand over
        with pytest.raises(pnr_amd.PnrError, match="at least 2x2x1"):
            ctx.set_volume(np.zeros(J8.shape, np.uint8))
        return
    load_stack(ctx, J8)
    assert_handover(ctx.seed_handover(), J8, (shape, kind))


LM_PARTS = 8  # seeds.hip: work-groups per layer of layer_minmax


def extremes_positions(base, wh):
    """byte offsets inside a layer that starts `base` bytes into the (16-byte aligned) J8 buffer at which layer_minmax changes from
    one loop to the next: name -> offset.  Per part [i0, i1): a byte head up to the first 16-byte boundary, uint4 loads, a byte tail."""
    per = -(-wh // LM_PARTS)
    pos = {"first": 0, "last": wh - 1}
    for part in range(LM_PARTS):
        i0, i1 = part * per, min(part * per + per, wh)
        pos["part%d_first" % part], pos["part%d_last" % part] = i0, i1 - 1
        if part in (2, LM_PARTS - 1):
            head = min(i0 + (16 - (base + i0) % 16) % 16, i1)
            body_end = head + (i1 - head) // 16 * 16
            pos["part%d_body_first" % part], pos["part%d_body_last" % part] = head, body_end - 1
            pos["part%d_head_last" % part] = head - 1 if head > i0 else None   # (no head: the part starts on a boundary)
            pos["part%d_tail_first" % part] = body_end if body_end < i1 else None
    return pos


def test_extremes_at_every_loop_boundary_of_layer_minmax(ctx):
    """layers of 37 x 31 = 1147 bytes (odd: every layer starts at another residue modulo 16), constant 100 but for one 200 and one
    50, which sweep the first and last byte of the layer, of each of the 8 parts, and of the byte head / vector body / byte tail of
    two parts; taken as the range [1, l) of the stack, so that z0 enters the addresses.  set_j8_v uploads to the start of the
    context's J8 buffer, a device allocation of its own and so aligned to far more than 16 bytes: layer z starts z * 1147 bytes in."""
    w, h = 37, 31
    wh = w * h
    names = sorted(extremes_positions(0, wh))
    n = 2 * len(names)  # every position carries the maximum twice and the minimum twice, in layers of different alignment
    J8 = np.full((1 + n, h, w), 100, np.uint8)
    J8[0] = np.random.RandomState(5).randint(0, 256, (h, w))  # the layer in front: not part of the range
    hit = {"max": set(), "min": set()}
    for j in range(n):
        pos = extremes_positions((1 + j) * wh, wh)
        na, nb = names[j % len(names)], names[(j + len(names) // 2 + j // len(names)) % len(names)]
        a, b = pos[na], pos[nb]
        if a is None:
            a, na = 0, "first"
        if b is None or b == a:
            b, nb = (a + 577) % wh, None
        J8[1 + j].flat[a], J8[1 + j].flat[b] = 200, 50
        hit["max"].add(na)
        hit["min"].add(nb)
    assert hit["max"] == set(names) and hit["min"] >= set(names) - {None}, (set(names) - hit["max"], set(names) - hit["min"])
    load_stack(ctx, J8)
    got = ctx.seed_handover(1, 1 + n)
    assert got["vmax"].tolist() == [200] * n and got["vmin"].tolist() == [50] * n, (got["vmax"], got["vmin"])
    assert_handover(got, J8[1:])


def test_layer_ranges_concatenate_and_calls_repeat(oracle):
    """[0, 5) + [5, 5) + [5, 12) is [0, 12), and a second call returns the same arrays: the scratch and pinned buffers of the context
    are reused, grown ([0, 5) -> [5, 12) -> [0, 12)) and not grown (the repeat); the tap leaves the seed list alone"""
    import orc
    rs = np.random.RandomState(12)
    J8 = (rs.randint(0, 6, (12, 31, 37)) * rs.randint(0, 50, (12, 31, 37))).astype(np.uint8)
    V = [rs.randint(0, 256, J8.shape).astype(np.uint8) for _ in range(3)]
    c = pnr_amd.Context(pnr_amd.make_params(), 0)
    c.set_volume(np.zeros(J8.shape, np.uint8))
    c.set_j8_v(J8, *V)
    parts = [c.seed_handover(z0, z1) for z0, z1 in ((0, 5), (5, 5), (5, 12))]
    assert len(parts[1]["vmin"]) == 0 and parts[1]["key_off"].tolist() == [0] and len(parts[1]["keys"]) == 0
    assert_handover(parts[0], J8[:5], "[0,5)")
    assert_handover(parts[2], J8[5:], "[5,12)")
    whole = c.seed_handover()
    assert_handover(whole, J8, "[0,12)")
    for k in ("vmin", "vmax", "ltot", "keys", "layers", "restored"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert np.array_equal(np.concatenate([parts[0]["key_off"], parts[0]["key_off"][-1] + parts[2]["key_off"][1:]]), whole["key_off"])
    seeds = c.extract_seeds()
    again = c.seed_handover(0, 12)
    for k in whole:
        assert np.array_equal(again[k], whole[k]), k
    want = orc.extract_seeds(oracle, 5, J8, *V)
    after = c.extract_seeds()
    for s in (seeds, after):
        assert np.array_equal(np.stack([s[k] for k in s.dtype.names], 1), want, equal_nan=True) and len(want) > 0
    c.close()


def test_handover_argument_checks():
    c = pnr_amd.Context(pnr_amd.make_params(), 0)
    c.set_volume(np.zeros((4, 8, 8), np.uint8))
    with pytest.raises(pnr_amd.PnrError, match="pnr_frangi"):
        c.seed_handover()
    z = np.zeros((4, 8, 8), np.uint8)
    c.set_j8_v(z, z, z, z)
    for z0, z1 in ((-1, 2), (0, 5), (3, 2)):
        with pytest.raises(pnr_amd.PnrError, match="layer range"):
            c.seed_handover(z0, z1)
    c.close()
