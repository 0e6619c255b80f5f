"""The placement logic of the tests above 2^31 voxels (bigvol.py), without a GPU: on the 96 x 64 x 41 stack, for each of the six tools, the
numpy restatement run on the whole stack equals the restatements on the crops around the two blocks, translated and combined by the
code the GPU tests call.  Also the placement rules themselves at both shapes, and the width of the translations.

Further down the same for the tracing path (bigtrace.py, 2048 x 2048 x 536 and 160 x 96 x 72): the oracle's Frangi on a crop is the
oracle's Frangi on the whole stack, the crops' seeds are the stack's, and the counts that the GPU tests lean on, at both shapes."""
import numpy as np
import pytest
import bigtrace
import bigvol
import geodesic_ref
import orc
import thin_ref
import ws_ref

SMALL, SHAPE = bigvol.SMALL, bigvol.SHAPE


@pytest.mark.parametrize("shape", [SMALL, SHAPE], ids=["small", "large"])
def test_the_placement_rules(shape):
    l, h, w = shape
    tiles = {"thin": bigvol.tile_of("thin.h", "THIN"), "ws": bigvol.tile_of("watershed.h", "WS"), "geo": bigvol.tile_of("geodesic.h", "GEO")}
    assert tiles["thin"] == thin_ref.tile()[::-1] and tiles["ws"] == ws_ref.tile()
    blocks = [(o, np.zeros(s, np.uint8)) for o, s in zip(bigvol.origins(shape), (bigvol.NEAR, bigvol.FAR))]
    for tile in tiles.values():
        first = bigvol.check_placement(blocks, shape, tile)
        assert (first > 2**31) == (shape == SHAPE)
    assert bigvol.index_of(w - 1, h - 1, l - 1, shape) == l * h * w - 1
    assert all(2000 < B.size < 8000 for _, B in blocks)


def test_translations_are_64_bit():
    """an index of the far block of the large stack survives the translation, and the last voxel is N - 1"""
    l, h, w = SHAPE
    o = bigvol.origins(SHAPE)[1]
    got = bigvol.abs_index(np.array([0, bigvol.FAR[2] * bigvol.FAR[1] - 1], np.int32), o, bigvol.FAR, SHAPE)
    assert got.dtype == np.int64 and got.tolist() == [o[2] + w * (o[1] + h * o[0]), l * h * w - 1] and got[0] > 2**31
    crop, lo = bigvol.stack_crop([(o, np.ones(bigvol.FAR, np.uint8))], SHAPE, [p - 2 for p in o], [p + n + 2 for p, n in zip(o, bigvol.FAR)])
    assert lo == (o[0] - 2, o[1] - 2, o[2] - 2) and crop.shape == (3, bigvol.FAR[1] + 2, bigvol.FAR[2] + 2) and crop[2, 2:, 2:].all() and not crop[:2].any()
    parts, other = bigvol.split_points(np.array([(w - 1, h - 1, l - 1), (w + 9, h, l + 2), (0, 0, 0), (np.inf, 0, 0)], np.float32), [(crop, lo)], SHAPE)
    assert parts[0][0].tolist() == [0, 1] and parts[0][1].tolist() == [[crop.shape[2] - 1, crop.shape[1] - 1, 2]] * 2 and other.tolist() == [2, 3]


def test_skeleton():
    case = bigvol.thin_case(SMALL)
    info, vox, deg = bigvol.thin_want(case)
    winfo, wvox, wdeg = bigvol.thin_whole(case)
    assert info == winfo and info["rounds"] >= 3 and info["n_skel"] > 10
    assert np.array_equal(vox, wvox) and np.array_equal(deg, wdeg)


def test_geodesic():
    case = bigvol.geo_case(SMALL)
    got, want = bigvol.geo_want(case), bigvol.geo_whole(case)
    assert got["info"] == want["info"] and got["info"]["n_src_dropped"] == 1 and got["info"]["n_src"] == len(case["sources"]) - 1
    assert np.array_equal(got["d"], want["d"]) and np.array_equal(got["label"], want["label"])
    assert sorted(got["paths"]) == sorted(want["paths"]) == case["walks"].tolist() and got["path_len"] == want["path_len"]
    assert all(np.array_equal(got["paths"][k], want["paths"][k]) for k in got["paths"])
    reached = got["d"] != geodesic_ref.UNREACHED
    first_far = int(np.prod(bigvol.NEAR))
    assert reached[:first_far].sum() > 1000 and reached[first_far:].sum() > 1000 and (~reached).any()
    assert max(got["path_len"].values()) > 5 and min(got["path_len"].values()) >= 0 and (got["label"][reached] > 2**31 - 12).all()


def test_geodesic_join():
    case = bigvol.join_case(SMALL)
    bridges, vox, info, per_block = bigvol.join_want(case)
    wb, wvox, winfo = bigvol.join_whole(case)
    assert bridges.tobytes() == wb.tobytes() and np.array_equal(vox, wvox) and info == winfo
    assert all(i["n_bridges"] >= 1 for i in per_block) and info["n_trees_out"] == info["n_trees_in"] - info["n_bridges"] >= 2
    far = bridges[bridges["p"] >= bigvol.index_of(0, 0, SMALL[0] - 1, SMALL)]
    assert len(far) >= 2 and len(set(far["w"].tolist())) < len(far), "a tie on W in the far block"


@pytest.mark.parametrize("conn", [26, 6])
def test_watershed(conn):
    case = bigvol.ws_case(SMALL)
    info, parts = bigvol.ws_want(case, conn)
    winfo, L, M = bigvol.ws_whole(case, conn)
    assert info == winfo and info["n_reached"] > 2000 and info["n_regions"] >= 6
    seen = np.zeros(SMALL, bool)
    for (z0, y0, x0), cl, cm in parts:
        at = (slice(z0, z0 + cl.shape[0]), slice(y0, y0 + cl.shape[1]), slice(x0, x0 + cl.shape[2]))
        assert np.array_equal(L[at], cl) and np.array_equal(M[at], cm)
        seen[at] = True
    assert not L[~seen].any() and not M[~seen].any()


def test_coverage():
    case = bigvol.render_case(SMALL)
    got, want = bigvol.render_want(case), bigvol.render_whole(case)
    assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    assert (got[1] > 0).sum() >= 8 and got[0]["n_both"] > 100


@pytest.mark.parametrize("rel_pct", [0, 50])
def test_radius(rel_pct):
    case = bigvol.radius_case(SMALL)
    k = bigvol.radius_want(case, rel_pct)
    assert np.array_equal(k, bigvol.radius_whole(case, rel_pct))
    assert (k == -1).sum() == 1 and len(set(k.tolist())) >= 4


# ---- the tracing path (bigtrace.py) ----
@pytest.mark.parametrize("shape", [bigtrace.SMALL, bigtrace.SHAPE], ids=["small", "large"])
def test_tracing_placement_rules(shape):
    l, h, w = shape
    first = bigtrace.check_placement(bigtrace.blocks(shape), shape)
    assert (first > 2**31) == (shape == bigtrace.SHAPE)
    if shape == bigtrace.SHAPE:
        assert l * h * w == 2248146944 and first == 2**31 + (h * w + (h - 64) * w + w - 96)
        assert bigtrace.chunk_planes(shape, bigtrace.ht_z()) == bigtrace.chunk_planes(shape) == 32
    else:
        assert bigtrace.chunk_planes(shape) == 96 and bigtrace.chunk_planes(shape, bigtrace.ht_z()) == 32  # one chunk, or three marches
    assert bigtrace.HALO == (7, 11, 11)
    (cn, on), (cf, of) = bigtrace.crops(bigtrace.blocks(shape), shape)
    assert on == (0, 0, 15) and cn.shape == (2 + 16 + 7, 4 + 64 + 11, 11 + 96 + 11), "the near crop is cut at the near faces in z and y"
    assert of == (l - 47, h - 75, w - 107) and cf.shape == (47, 75, 107), "the far crop has a halo on its near sides and ends at the far faces"
    assert not cn[-7:].any() and not cn[:, -11:].any() and not cn[:, :, :11].any() and not cn[:, :, -11:].any() and not cf[:7].any() and not cf[:, :11].any() and not cf[:, :, :11].any()
    assert cn.max() > 150 and cf.max() > 150 and np.count_nonzero(cf[7:, 11:, 11:]) > 200000, "tubes over noise"


def test_tracing_indices_are_64_bit():
    """centroids in the far corner of the large stack: their voxel indices, formed in INDEX, lie above 2^31 and end at N - 1"""
    l, h, w = bigtrace.SHAPE
    xc = np.array([(w - 1, h - 1, l - 1), (0.4, 0.2, l - 24), (w - 96, h - 64, l - 23), (w + 7.0, -3.0, l + 2.0)], np.float32)
    idx = bigtrace.centroid_index(xc, 4, bigtrace.SHAPE)
    assert idx.dtype == np.int64 and idx.tolist() == [l * h * w - 1, 2**31, bigtrace.check_placement(bigtrace.blocks(bigtrace.SHAPE), bigtrace.SHAPE), (l - 1) * h * w + w - 1]
    assert int(bigtrace.index_of(w - 1, h - 1, l - 1, bigtrace.SHAPE)) == l * h * w - 1 > 2**31


def test_frangi_of_a_crop_is_frangi_of_the_stack(oracle):
    """J, J8, Vx, Vy, Vz of the oracle on each crop of the small stack, with the extremes over both crops, equal the oracle's on the
    whole stack -- on the whole crop, its halo included: a cut side repeats a plane of zeros -- and the whole stack's J8 is 0 outside
    the crops; then the seeds: the crops' seeds, translated, are the stack's, and each compared layer as a one-slice stack gives its rows"""
    shape = bigtrace.SMALL
    fw, W = bigtrace.frangi_want(oracle, shape), bigtrace.frangi_whole(oracle, shape)
    assert (fw["jmin"], fw["jmax"]) == (W["jmin"], W["jmax"]) and fw["jmin"] == 0 < fw["jmax"]
    assert fw["crops"][0]["ext"][1] != fw["crops"][1]["ext"][1], "the extremes are the stack's, not a crop's own"
    for c in fw["crops"]:
        at = bigtrace.region(c["o"], c["J"])
        for k in ("J", "J8", "Vx", "Vy", "Vz"):
            assert np.array_equal(W[k][at], c[k]), (k, c["o"])
        assert (c["J8"] > 0).sum() > 5000
    assert np.count_nonzero(W["J8"][bigtrace.outside(shape, [(c["o"], c["J8"]) for c in fw["crops"]])]) == 0
    seeds = bigtrace.seeds_want(oracle, fw)
    assert np.array_equal(seeds, orc.extract_seeds(oracle, bigtrace.PARAMS["tolerance"], W["J8"], W["Vx"], W["Vy"], W["Vz"])[:, :6]) and len(seeds) > 200
    for z in bigtrace.compared_layers(shape):
        assert np.array_equal(bigtrace.layer_want(oracle, fw, shape, z), seeds[seeds[:, 2] == z]), z


@pytest.mark.parametrize("shape", [bigtrace.SMALL, bigtrace.SHAPE], ids=["small", "large"])
def test_tracing_conditions(oracle, shape):
    """what the GPU tests rely on, from the oracle on the whole host stack (EXPERIMENTS.md has the counts): each compared far layer
    has more than 5 seeds, at least 3 far seeds at z >= l - 20 (516) pass znccth, at least two of their traces run 8 iterations or
    more with every centroid's voxel index above that of plane l - 24 (2^31), at least one trace crosses below that plane"""
    l, h, w = shape
    r = bigtrace.reference(oracle, shape)
    n = r["counts"]
    print(shape, n)
    layers = bigtrace.compared_layers(shape)
    assert layers[1] == l - 24 and all(n["layer_seeds"][z] > 5 for z in layers[1:]) and n["layer_seeds"][layers[0]] > 5
    for z in layers:
        assert np.array_equal(bigtrace.layer_want(oracle, r["frangi"], shape, z), r["seeds"][r["seeds"][:, 2] == z]), z
    assert n["far_kept"] >= 3 and n["traces_above"] >= 2 and n["traces_crossing"] >= 1
    sel6 = r["sorted6"][r["sel"]]
    assert len(sel6) == bigtrace.NSEL + 1 and (sel6[:-1, 2] >= l - 20).all() and sel6[-1, 2] < 18 and len(r["traces"]) == 2 * len(sel6)
    far_rows = [bigtrace.centroid_index(xc, min(T + 1, bigtrace.PARAMS["ni"]), shape) for T, _, xc in r["traces"][:-2]]
    sign = int(bigtrace.index_of(0, 0, l - 24, shape))
    assert (sign == 2**31) == (shape == bigtrace.SHAPE) and all(i.dtype == np.int64 for i in far_rows)
    above = np.concatenate(far_rows) > sign
    assert above.sum() > 0.5 * len(above) and (~above).sum() >= 1, "most of the far centroids lie above the sign plane, some below"
    assert {st for _, st, _ in r["traces"]} >= {0, 1}, "traces that run out of iterations and traces that end early"
    if shape == bigtrace.SHAPE:  # the blocks are the same and so are the responses: the small stack's seeds, moved
        s = bigtrace.reference(oracle, bigtrace.SMALL)
        d = np.array([w - bigtrace.SMALL[2], h - bigtrace.SMALL[1], l - bigtrace.SMALL[0]], np.float32)
        far = r["seeds"][:, 2] >= l - 40
        assert np.array_equal(r["seeds"][~far], s["seeds"][~far]) and np.array_equal(r["seeds"][far][:, :3] - d, s["seeds"][far][:, :3]) and np.array_equal(r["seeds"][:, 3:], s["seeds"][:, 3:])
