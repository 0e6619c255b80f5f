"""The device path on image content the synthetic tubes never produce (tests/imgclass.py; tests/test_image_classes_host.py shows on
the oracle what each class brings): every class through fuzzcase.check_stack against the oracle, stage by stage and for EQUALITY OF
BYTES -- J, J8, Vx / Vy / Vz, the pruned run's J8 and extremes, seeds, scores with the order of ties, every trace iteration, the
streamed against the one-shot graph, replay, reconstruct.  Which of hessian_tile's analytic shortcuts settles a voxel, how full the
survivor queue gets, how dense the J8 bitmap of the seed extraction is and whether the seed sort meets ties all depend on the image.

Shapes (w x h x l): 83 x 29 x 41 -- two x tiles of hessian_tile with a ragged second one, h no multiple of 8, two z marches;
83 x 29 x 70 -- deeper than two marches, so the pruned first scale runs the middle march first (also with frangi_prune = 0 and with
hess_chunk = 32: same bytes); 83 x 29 x 1 -- the 2-D kernels.  Further down: ZNCC and traces in exactly flat regions, and the edges
of the seed kernels (wave tiles, lane groups, non-zero layer minima) on hand-made J8 layers."""
import numpy as np
import pytest
import orc
import fuzzcase
import imgclass
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu
SHAPES = {"41": ((83, 29, 41), [2.0, 3.0]), "70": ((83, 29, 70), [2.0, 4.0]), "2d": ((83, 29, 1), [2.0, 3.0])}
NSEL = 3
_ref = {}  # the oracle's Frangi, seeds and scores of a (class, shape, threshold, somaradius): computed once, never changed


def _params(sigs, znccth=0.3, somaradius=0):
    return dict(sigmas=sigs, somaradius=somaradius, step=2, kappa=3.0, zdist=2.0, np_=50, ni=12, tolerance=5, znccth=znccth, nodepervol=4, vol=1)


def _check(oracle, name, shape, knobs=None, driver="phased", znccth=0.3, somaradius=0):
    (w, h, l), sigs = SHAPES[shape]
    img = imgclass.make(name, w, h, l)
    stats = {}
    ref = _ref.setdefault((name, shape, znccth, somaradius), {})
    fuzzcase.check_stack(oracle, img, _params(sigs, znccth, somaradius), knobs or {}, None, stats, driver=driver, nsel=NSEL, ref=ref)
    assert stats["voxels"] == img.size and stats.get("traces", 0) == 2 * min(NSEL, stats.get("kept", 0)), stats
    return stats


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", imgclass.CLASSES)
def test_class_bit_exact(oracle, name, shape):
    stats = _check(oracle, name, shape)
    if name == "noise" and shape != "2d":  # nothing survives the filter: the end-to-end path on an empty list
        assert stats["seeds"] >= 500 and stats.get("kept", 0) == 0 and stats["nodes"] == 0, stats
    else:
        assert stats["kept"] >= 2 and stats["iters"] >= 4, stats


@pytest.mark.parametrize("knobs", [{"frangi_prune": 0}, {"hess_chunk": 32}], ids=["noprune", "chunk32"])
@pytest.mark.parametrize("name", imgclass.CLASSES)
def test_class_bit_exact_frangi_forms(oracle, name, knobs):
    """without the J8 shortcut, and with the Hessian stage cut into z-chunks of one march: the same bytes"""
    _check(oracle, name, "70", knobs=knobs)


@pytest.mark.parametrize("name", ["noise", "blocks", "saturated"])
def test_class_bit_exact_persistent_driver(oracle, name):
    _check(oracle, name, "41", driver="persistent")


@pytest.mark.parametrize("shape", ["41", "70"])
def test_noise_at_the_lowest_threshold(oracle, shape):
    """znccth = 0, the lowest the parameter check accepts: hundreds of noise seeds pass the filter and are sorted"""
    with pytest.raises(pnr_amd.PnrError, match="znccth"):
        pnr_amd.Context(pnr_amd.make_params(znccth=-1), 0)
    stats = _check(oracle, "noise", shape, znccth=0.0)
    assert stats["kept"] >= 100, stats


def test_blocks_with_somas(oracle):
    """somaradius = 3 on the blocks: the oracle decides what the somas are"""
    stats = _check(oracle, "blocks", "41", somaradius=3)
    assert stats["kept"] >= 2, stats


# ---- ZNCC and traces where the image is exactly flat ----
# blocks at 83 x 29 x 41: the 255 block is x 10..59, y 2..26, z 5..35; the slab x 70..71 over every y and z
POSES = {"in_x": (35, 14, 20, 1, 0, 0), "in_y": (35, 14, 20, 0, 1, 0), "in_z": (35, 14, 20, 0, 0, 1),
         "black": (65, 14, 20, 1, 0, 0), "black_border": (80, 14, 20, 0, 1, 0),
         "face": (10, 14, 20, 1, 0, 0), "face_along": (10, 14, 20, 0, 1, 0), "edge": (10, 2, 20, 0, 0, 1), "corner": (10, 2, 5, 1, 0, 0),
         "slab_y": (70.5, 14, 20, 0, 1, 0), "slab_z": (70, 14, 20, 0, 0, 1)}


def test_zncc_and_traces_in_flat_regions(oracle):
    """a template over a constant neighbourhood has zero variance: the oracle scores it exactly 0 at the first sigma, and a trace
    from there ends at once (T = 0, stop reason 2); the device gives the same bytes, the record of iteration 0 included"""
    (w, h, l), sigs = SHAPES["41"]
    img = imgclass.make("blocks", w, h, l)
    T = orc.Tracker(oracle, sigs, 2, 50, 12, 3.0, 0.3, zdist=2.0)
    c = pnr_amd.Context(pnr_amd.make_params(**_params(sigs)), 0)
    c.set_volume(img)
    pd = np.array(list(POSES.values()), np.float32)
    co, so = T.zncc(img, pd)
    flat = [list(POSES).index(k) for k in ("in_x", "in_y", "in_z", "black")]
    assert np.all(co[flat] == 0) and np.all(so[flat] == sigs[0]), (co, so)
    assert np.all(co[[list(POSES).index(k) for k in ("slab_y", "slab_z")]] > 0.3), co
    cg, sg = c.zncc(pd)
    assert np.array_equal(cg, co) and np.array_equal(sg, so), (cg, co, sg, so)
    seeds = np.zeros(3, lib.SEED_DT)
    for i, k in enumerate(lib.SEED_DT.names[:6]):
        seeds[k] = pd[:3, i]
    for driver in ("phased", "persistent"):
        c.set_smc_driver(driver)
        Tg, stop, xc, _ = c.trace_batch(seeds)
        for i in range(3):
            for d_, sgn in enumerate((1, -1)):
                q = pd[i].copy(); q[3:] *= sgn
                Tn, st, xco, *_ = T.trace(img, q)
                j = 2 * i + d_
                assert (Tn, st) == (0, 2), (i, d_, Tn, st)
                assert Tg[j] == Tn and stop[j] == st and np.array_equal(fuzzcase.mat(xc[j])[:1], xco[:1], equal_nan=True), (driver, j, Tg[j], stop[j], xc[j][:1], xco[:1])
    c.close()


# ---- the seed kernels' edges: hand-made J8 layers through set_j8_v ----
def _seed_layers(w, rs):
    """two J8 stacks [3][9][w]: dense layers with a non-zero minimum; sparse layers with maxima and plateaus at the wave-tile edge
    x = 255 | 256, at the 4-pixel lane groups and next to the image border (positions past the width are left out)"""
    h = 9
    dense = np.zeros((3, h, w), np.uint8)
    dense[0] = rs.randint(1, 256, (h, w))    # layer minimum 1, not flat
    dense[1] = rs.randint(200, 256, (h, w))  # layer minimum 200
    dense[2] = 255                           # 255 everywhere except 5 pixels
    for x, y, v in ((0, 0, 0), (w - 1, h - 1, 7), (w // 2, 4, 254), (min(255, w - 1), 3, 100), (min(256, w - 1), 5, 250)):
        dense[2, y, x] = v
    sparse = np.zeros((3, h, w), np.uint8)

    def put(z, y, x, v):
        if 0 <= x < w:
            sparse[z, y, x] = v

    # isolated maxima, no two of them neighbours: both sides of a wave tile, next to the border and on it, at a lane-group edge
    for y, x, v in ((1, 255, 90), (3, 256, 80), (5, 1, 70), (5, w - 2, 60), (7, 128, 30), (8, 0, 50), (8, w - 1, 40)):
        put(0, y, x, v)
    for x0, v in ((254, 120), (2, 110), (126, 100), (510, 95)):  # 2 x 3 plateaus across 255 | 256 and across lane groups 3 | 4, 127 | 128, 511 | 512
        for dy in (0, 1):
            for dx in (0, 1, 2):
                put(1, 1 + dy, x0 + dx, v)
    for x0, v in ((255, 77),):  # 3 x 2: upright across the tile edge
        for dy in (0, 1, 2):
            for dx in (0, 1):
                put(1, 4 + dy, x0 + dx, v)
    # two equal maxima across the tile edge, joined by pixels 3 below them: one seed at tolerance 5 and 40, two at 0
    for x, v in ((254, 100), (255, 97), (256, 97), (257, 100)):
        put(2, 2, x, v)
    for x, v in ((253, 200), (254, 170), (255, 165), (256, 170), (257, 200)):  # joined at 40 only
        put(2, 4, x, v)
    return dense, sparse


@pytest.mark.parametrize("w", [255, 256, 257, 259, 513])
def test_seed_kernel_edges(oracle, w):
    rs = np.random.RandomState(w)
    stacks = [(J8, [rs.randint(0, 256, J8.shape).astype(np.uint8) for _ in range(3)]) for J8 in _seed_layers(w, rs)]
    counts = []
    for tol in (0, 5, 40):
        c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], tolerance=tol), 0)
        c.set_volume(np.zeros((3, 9, w), np.uint8))
        for J8, V in stacks:
            c.set_j8_v(J8, *V)
            want = orc.extract_seeds(oracle, tol, J8, *V)
            got = fuzzcase.mat(c.extract_seeds())
            assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (w, tol, len(got), len(want))
            counts.append(len(want))
        c.close()
    assert counts[1] >= counts[3] > counts[5] > 0, counts  # (sparse layers: a wider tolerance joins maxima)
