"""GPU parity: extractSeeds through the C ABI (GPU candidate kernels + host flood-fill) vs the
golden vectors of the reference's seed.cpp and the oracle.  Integer/byte work: bit-exact."""
import numpy as np
import pytest
import orc
import synth
import pnr_amd
import seeds_ref as sr
from pnr_amd import SeedExtractor

pytestmark = pytest.mark.gpu


def as_mat(s):
    return np.stack([s[k] for k in s.dtype.names], 1)


def test_seeds_vs_golden(golden):
    s = SeedExtractor.extractSeeds(float(golden["tol"]), golden["J8_restated"], golden["Vx"], golden["Vy"], golden["Vz"])
    assert np.array_equal(as_mat(s), golden["seeds"])


def test_seeds_random_layers(oracle):
    rs = np.random.RandomState(11)
    for tol in (0.0, 1.0, 5.0, 40.0):
        J8 = (rs.randint(0, 6, (5, 31, 37)) * rs.randint(0, 50, (5, 31, 37))).astype(np.uint8)
        J8[1] = 0          # empty layer
        J8[2] = np.clip(J8[2], 0, 3)
        J8[3] = 9          # flat non-zero layer
        V = [rs.randint(0, 256, J8.shape).astype(np.uint8) for _ in range(3)]
        want = orc.extract_seeds(oracle, tol, J8, *V)
        got = SeedExtractor.extractSeeds(tol, J8, *V)
        assert np.array_equal(as_mat(got), want, equal_nan=True), tol


def test_seeds_wide_layer_and_ranges(oracle):
    """w > 256 (several x tiles), and the layer-range entry point used for multi-GPU sharding"""
    img = synth.synth(300, 64, 12, seed=8)
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, [2.0], 2.0)
    J8 = orc.j8(oracle, J, jmin, jmax)
    want = orc.extract_seeds(oracle, 5, J8, Vx, Vy, Vz)
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0]), 0)
    c.set_volume(img)
    c.set_j8_v(J8, Vx, Vy, Vz)
    assert np.array_equal(as_mat(c.extract_seeds()), want) and len(want) > 0
    parts = [as_mat(c.extract_seeds(z0, z1)) for z0, z1 in ((0, 5), (5, 5), (5, 12))]
    assert np.array_equal(np.concatenate(parts), want)


def test_seeds_require_frangi_first():
    c = pnr_amd.Context(pnr_amd.make_params(), 0)
    c.set_volume(np.zeros((4, 8, 8), np.uint8))
    with pytest.raises(pnr_amd.PnrError, match="pnr_frangi"):
        c.extract_seeds()


@pytest.mark.parametrize("world", [2, 3])
def test_zslab_sharding_equals_whole_stack(world):
    """Frangi + seeds of a stack cut into z-slabs with halo (pnr_frangi_slab / pnr_quantise_j8 / pnr_extract_seeds_range, one
    'rank' after the other on this GPU): same Jmin / Jmax, same seeds in the same order as the unsharded extraction"""
    import torch
    from pnr_amd import multigpu
    img = synth.synth(64, 56, 48, seed=3)
    p = pnr_amd.make_params(sigmas=[2.0, 4.0], zdist=2.0, np_=20, ni=5)
    c = pnr_amd.Context(p, 0)
    c.set_volume(img)
    jmin, jmax = c.frangi()
    want = c.extract_seeds()
    dimg = torch.from_numpy(img).cuda()
    # pass 1: every rank's extremes; pass 2: quantise with the reduced ones (what the all-reduce does)
    ext = []
    for r in range(world):
        ctx = pnr_amd.Context(p, 0)
        _, a, b = multigpu.frangi_seeds_sharded(ctx, dimg.data_ptr(), img.shape, None, r, world, reduce_fn=lambda a, b: (a, b))
        ext.append((a, b))
        ctx.close()
    gmin, gmax = min(e[0] for e in ext), max(e[1] for e in ext)
    assert gmin == jmin and gmax == jmax
    got = []
    for r in range(world):
        ctx = pnr_amd.Context(p, 0)
        s, _, _ = multigpu.frangi_seeds_sharded(ctx, dimg.data_ptr(), img.shape, None, r, world, reduce_fn=lambda a, b: (gmin, gmax))
        got.append(s)
        ctx.close()
    got = np.concatenate(got)
    assert len(got) == len(want) > 20
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


# ---- end to end on the stacks of the hand-over tests (tests/seeds_ref.py): the shapes at which the index arithmetic of the seed
# kernels changes, and the tolerances around the fill's early break (a 255 over a minimum of 0 survives 254, nothing survives 255) ----
E2E_CASES = [(s, k) for s in sr.SHAPES for k in sr.E2E_KINDS]
_e2e_ctx = {}


def e2e_context(tol, shape):
    """one context per tolerance for the whole sweep, moved from stack to stack"""
    if tol not in _e2e_ctx:
        _e2e_ctx[tol] = pnr_amd.Context(pnr_amd.make_params(tolerance=tol), 0)
    c = _e2e_ctx[tol]
    w, h, l = shape
    if c.shape != (l, h, w):
        c.set_volume(np.zeros((l, h, w), np.uint8))  # dimensions only
    return c


@pytest.mark.parametrize("shape,kind", E2E_CASES, ids=["%s-%s" % (sr.shape_id(s), k) for s, k in E2E_CASES])
def test_seeds_at_kernel_edge_shapes(oracle, shape, kind):
    J8, V = sr.stack(shape, kind), sr.directions(shape)
    if shape[0] < 2 or shape[1] < 2:  # no volume under 2 x 2 x 1: the library refuses it, the oracle finds nothing in it
        with pytest.raises(pnr_amd.PnrError, match="at least 2x2x1"):
            e2e_context(5, shape)
        assert all(len(sr.oracle_seeds(oracle, shape, kind, tol)) == 0 for tol in sr.TOLERANCES)
        return
    for tol in sr.TOLERANCES:
        want = sr.oracle_seeds(oracle, shape, kind, tol)
        c = e2e_context(tol, shape)
        c.set_j8_v(J8, *V)
        assert np.array_equal(as_mat(c.extract_seeds()), want, equal_nan=True), (tol, len(want))
        if not sr.has_interior(shape):
            assert len(want) == 0
        if tol == 5:  # one fill thread, and three: more than some of the layer counts, fewer than others
            before = c.get_option("host_threads")
            for nt in (1, 3):
                c.set_option("host_threads", nt)
                got = as_mat(c.extract_seeds())
                c.set_option("host_threads", before)
                assert np.array_equal(got, want, equal_nan=True), ("host_threads", nt)


def test_edge_shape_sweep_is_not_vacuous(oracle):
    """the sweep above compares seed lists: it must contain seeds -- for every shape with an interior, and at tolerance 254 (the last
    one in front of the fill's early break) in at least three shapes"""
    n254 = 0
    for shape in sr.SHAPES:
        counts = {tol: sum(len(sr.oracle_seeds(oracle, shape, k, tol)) for k in sr.E2E_KINDS) for tol in sr.TOLERANCES}
        if sr.has_interior(shape):
            assert max(counts.values()) > 0, shape
        else:
            assert max(counts.values()) == 0, shape
        assert counts[255] == 0 and counts[1000] == 0, shape
        n254 += counts[254] > 0
    assert n254 >= 3
    for c in _e2e_ctx.values():
        c.close()
    _e2e_ctx.clear()
