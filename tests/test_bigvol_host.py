"""The placement logic of the tests above 2^31 voxels (bigvol.py), without a GPU: on the 96 x 64 x 41 stack, for each of the six tools, the
numpy restatement run on the whole stack equals the restatements on the crops around the two blocks, translated and combined by the
code the GPU tests call.  Also the placement rules themselves at both shapes, and the width of the translations."""
import numpy as np
import pytest
import bigvol
import geodesic_ref
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
