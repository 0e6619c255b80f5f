"""The numpy reference of the seed hand-over (tests/seeds_ref.py) against the oracle, on the CPU: the oracle accepts a seed only at
a pixel that the reference lists as a candidate, on every stack the GPU tests use; and the stacks are what their names say."""
import numpy as np
import pytest
import seeds_ref as sr


@pytest.mark.parametrize("kind", sr.KINDS)
def test_oracle_seeds_lie_in_reference_candidates(oracle, kind):
    seen = 0
    for shape in sr.SHAPES:
        w, h, l = shape
        ref = sr.stack_handover(shape, kind)
        cand = [set((ref["keys"][ref["key_off"][z]:ref["key_off"][z + 1]] & 0xffffffff).tolist()) for z in range(l)]
        for tol in (0, 5, 254):
            s = sr.oracle_seeds(oracle, shape, kind, tol)
            for x, y, z in s[:, :3].astype(np.int64):
                assert y * w + x in cand[z], (shape, kind, tol, x, y, z)
            seen += len(s)
        if not sr.has_interior(shape):
            assert ref["key_off"][-1] == 0
    assert seen > 100


def test_reference_on_a_layer_worked_by_hand():
    L = np.array([[2, 2, 2, 2, 2],
                  [2, 1, 5, 5, 2],   # the 5 | 5 plateau: both are candidates (no greater neighbour)
                  [2, 1, 1, 3, 2],   # the 1s and the 3 have a greater neighbour; border pixels never count
                  [2, 2, 2, 2, 0]], np.uint8)  # minimum 0, maximum 5, 19 pixels above the minimum
    got = sr.layer_keys(L)
    vf = np.float32(2e9 / 5.0)
    want = sorted((int(np.int32(np.float32(5) * vf)) << 32) | p for p in (1 * 5 + 2, 1 * 5 + 3))
    assert got.tolist() == want
    ref = sr.handover(L[None])
    assert (ref["vmin"][0], ref["vmax"][0], ref["ltot"][0]) == (0, 5, 19) and ref["key_off"].tolist() == [0, 2]
    assert len(sr.layer_keys(np.full((4, 4), 9, np.uint8))) == 0


def test_stacks_are_what_the_kinds_promise():
    for shape in sr.SHAPES:
        w, h, l = shape
        sp, de, ed = (sr.stack(shape, k) for k in ("sparse", "dense", "edge"))
        if l < 15:
            assert de.reshape(l, -1).min(1).tolist() == [7] * l and np.count_nonzero(de == 7) == l
            if w * h >= 2:
                assert all(L.max() == 255 and L.min() == 0 for L in ed)
            if sr.has_interior(shape):
                assert all(L[1:-1, 1:-1].max() == 255 for L in sp)
        else:
            per = -(-l // sr.J8_CHUNKS)
            for J8 in (sp, de, ed):
                assert not J8[2 * per:3 * per].any()
                assert all(J8[z].min() == J8[z].max() for z in range(2, l, 3))
                assert any(J8[z].min() == 9 for z in range(2, l, 3))
        if w * h >= 1000:
            assert 0.03 < np.count_nonzero(sp) / sp.size < 0.07
