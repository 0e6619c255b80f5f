"""GPU: the return code and the full pnr_last_error() text of the argument and state checks at the C boundary of the volume and tree
tools, per tool one call for each of its checks in source order, and one call with two bad arguments that pins which check runs first.
One context holds a 4 x 4 x 2 random volume, a second one never had a volume; the trees have two nodes.

Not reached here: the voxel limit ("%lld voxels, at most 2^32 - 2") needs a volume of 4 GiB; it is one helper, read it instead."""
import ctypes as C
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu

XYZ2 = np.array([[0, 0, 0], [2, 2, 1]], np.float32)
PAR2 = np.array([-1, 0], np.int32)
RAD2 = np.ones(2, np.float32)
NAN2 = np.array([[0, 0, 0], [2, np.nan, 1]], np.float32)
COST0 = np.ones(256, np.uint16)
COST0[5] = 0


def ptr(a):
    return None if a is None else a.ctypes.data


def fails(code, text, call, *args, **kw):
    """a method of Context raises PnrError with the code and the text; an entry point called directly returns the code and leaves the text"""
    try:
        rc = call(*args, **kw)
    except lib.PnrError as e:
        assert str(e) == f"libpnr_hip error {code}: {text}"
        return
    assert rc == code and lib.load().pnr_last_error().decode() == text, (rc, lib.load().pnr_last_error().decode())


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), ni=4, np_=8), 0)
    c.set_volume(np.random.default_rng(3).integers(0, 256, (2, 4, 4), dtype=np.uint8))
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare():
    """a context that never had a volume"""
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), ni=4, np_=8), 0)
    yield c
    c.close()


def test_components(ctx):
    L = ctx.L
    for who, run in (("pnr_label_components", lambda **kw: ctx.label_components(labels=False, **kw)), ("pnr_despeckle_volume", lambda **kw: ctx.despeckle(kw.pop("min_size", 1), **kw))):
        fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256)
        fails(-1, f"{who}: thr = -2 outside [-1, 255]", run, thr=-2)
        fails(-1, f"{who}: connectivity = 7, not 6 or 26", run, connectivity=7)
        fails(-1, f"{who}: min_size = 0 must be at least 1", run, min_size=0)
        fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256, connectivity=7)
        fails(-1, f"{who}: connectivity = 7, not 6 or 26", run, connectivity=7, min_size=0)
    who = "pnr_label_components"
    bad = lib.ComponentsOpts(256, 26, 1)
    fails(-1, f"{who}: cap = -1 is negative", L.pnr_label_components, ctx.h, None, None, None, None, -1)
    fails(-1, f"{who}: cap = -1 is negative", L.pnr_label_components, ctx.h, C.byref(bad), None, None, None, -1)  # the capacity before the options
    fails(-1, f"{who}: cap = -1 is negative", L.pnr_label_components, None, None, None, None, None, -1)  # and before the context
    fails(-1, "null ctx", L.pnr_label_components, None, C.byref(bad), None, None, None, 0)
    fails(-1, "null ctx", L.pnr_despeckle_volume, None, C.byref(bad), None)
    assert ctx.label_components(labels=False)[0]["n_vox"] == 32


def test_distance_transform(ctx):
    L, who = ctx.L, "pnr_distance_transform"
    run = lambda **kw: ctx.distance_transform(volume=False, **kw)
    at = np.zeros(1, np.float32)
    fails(-1, "null ctx", L.pnr_distance_transform, None, None, None, None, None, -1, None)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256)
    fails(-1, f"{who}: rmax = 0 outside [1, 1024]", run, rmax=0)
    fails(-1, f"{who}: rmax = 1025 outside [1, 1024]", run, rmax=1025)
    fails(-1, f"{who}: n = -1 positions (at most 2^28) need xyz and d2_at", L.pnr_distance_transform, ctx.h, None, None, None, None, -1, None)
    fails(-1, f"{who}: n = 1 positions (at most 2^28) need xyz and d2_at", L.pnr_distance_transform, ctx.h, None, None, None, None, 1, ptr(at))
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256, rmax=0)
    bad = lib.EdtOpts(-1, 0)
    fails(-1, f"{who}: rmax = 0 outside [1, 1024]", L.pnr_distance_transform, ctx.h, C.byref(bad), None, None, None, -1, None)


def test_skeletonize(ctx):
    L, who = ctx.L, "pnr_skeletonize"
    run = lambda **kw: ctx.skeletonize(volume=False, voxels=False, **kw)
    fails(-1, "null ctx", L.pnr_skeletonize, None, None, None, None, None, None, -1)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256)
    fails(-1, f"{who}: max_rounds = -1 is negative", run, max_rounds=-1)
    fails(-1, f"{who}: cap = -1 is negative", L.pnr_skeletonize, ctx.h, None, None, None, None, None, -1)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256, max_rounds=-1)
    bad = lib.ThinOpts(-1, -1)
    fails(-1, f"{who}: max_rounds = -1 is negative", L.pnr_skeletonize, ctx.h, C.byref(bad), None, None, None, None, -1)


def test_geodesic_distance(ctx):
    L, who = ctx.L, "pnr_geodesic_distance"
    run = lambda src=XYZ2, **kw: ctx.geodesic(src, volume=False, **kw)

    def direct(o=None, src=XYZ2, lab=None, n=2, at=None, m=0, d_at=None, path_cap=0, path_len=None, path_vox=None, h=ctx.h):
        return L.pnr_geodesic_distance(h, ptr(src), ptr(lab), n, None if o is None else C.byref(o), None, None, None, ptr(at), m, ptr(d_at), None, path_cap, ptr(path_len), ptr(path_vox))

    d_at, plen = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    fails(-1, "null ctx", direct, h=None, n=-1)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256)
    fails(-1, f"{who}: dmax = 0 outside [1, 2^31 - 1]", run, dmax=0)
    fails(-1, f"{who}: dmax = 2147483648 outside [1, 2^31 - 1]", run, dmax=1 << 31)
    fails(-1, f"{who}: cost[5] = 0, every entry is at least 1", run, cost=COST0)
    fails(-1, f"{who}: n_src = -1 sources (at most 2^28) need src_xyz", direct, n=-1)
    fails(-1, f"{who}: n_src = 2 sources (at most 2^28) need src_xyz", direct, src=None)
    fails(-1, f"{who}: label[1] = -3 is negative", run, labels=[0, -3])
    fails(-1, f"{who}: path_cap = -1 outside [0, 65536]", run, targets=XYZ2, path_cap=-1)
    fails(-1, f"{who}: path_cap = 65537 outside [0, 65536]", direct, path_cap=65537)
    fails(-1, f"{who}: m = -1 targets (at most 2^28) need at_xyz and one of d_at, label_at and path_cap > 0", direct, m=-1)
    fails(-1, f"{who}: m = 1 targets (at most 2^28) need at_xyz and one of d_at, label_at and path_cap > 0", direct, m=1, d_at=d_at)
    fails(-1, f"{who}: m = 1 targets (at most 2^28) need at_xyz and one of d_at, label_at and path_cap > 0", direct, m=1, at=XYZ2)
    fails(-1, f"{who}: path_cap = 4 needs path_len and path_vox", direct, m=1, at=XYZ2, path_cap=4, path_len=plen)
    # the order: thr, dmax, the cost table, the sources, their labels, path_cap, the targets, the path buffers
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256, dmax=0)
    fails(-1, f"{who}: dmax = 0 outside [1, 2^31 - 1]", run, dmax=0, cost=COST0)
    fails(-1, f"{who}: cost[5] = 0, every entry is at least 1", run, cost=COST0, labels=[0, -3])
    fails(-1, f"{who}: n_src = -1 sources (at most 2^28) need src_xyz", direct, n=-1, path_cap=-1)
    fails(-1, f"{who}: label[1] = -3 is negative", run, labels=[0, -3], targets=XYZ2, path_cap=-1)
    fails(-1, f"{who}: path_cap = -1 outside [0, 65536]", direct, path_cap=-1, m=-1)


def test_measure_radii(ctx):
    L, who = ctx.L, "pnr_measure_radii"
    fails(-1, "null ctx", L.pnr_measure_radii, None, None, -1, None, None, None)
    fails(-1, f"{who}: rmax = 0 outside [1, 64]", ctx.measure_radii, XYZ2, rmax=0)
    fails(-1, f"{who}: rmax = 65 outside [1, 64]", ctx.measure_radii, XYZ2, rmax=65)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", ctx.measure_radii, XYZ2, thr=256)
    fails(-1, f"{who}: rel_pct = 101 outside [0, 100]", ctx.measure_radii, XYZ2, rel_pct=101)
    fails(-1, f"{who}: bg_permille = 1000 outside [0, 999]", ctx.measure_radii, XYZ2, bg_permille=1000)
    fails(-1, f"{who}: n = -1 positions (at most 2^28) need xyz and k_out", L.pnr_measure_radii, ctx.h, None, -1, None, None, None)
    fails(-1, f"{who}: n = 2 positions (at most 2^28) need xyz and k_out", L.pnr_measure_radii, ctx.h, ptr(XYZ2), 2, None, None, None)
    fails(-1, f"{who}: rmax = 0 outside [1, 64]", ctx.measure_radii, XYZ2, rmax=0, thr=256)  # rmax before thr
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", ctx.measure_radii, XYZ2, thr=256, rel_pct=101)
    fails(-1, f"{who}: rel_pct = 101 outside [0, 100]", ctx.measure_radii, XYZ2, rel_pct=101, bg_permille=1000)


def test_point_segment_distance_and_nearest_other(ctx):
    L, who = ctx.L, "pnr_point_segment_distance"
    d = np.zeros(2, np.float32)
    fails(-1, "null ctx", L.pnr_point_segment_distance, None, None, -1, None, None, 0, None, None)
    fails(-1, f"{who}: m = 0 segments (1 to 2^22) need seg_a and seg_b", ctx.point_segment_distance, XYZ2, XYZ2[:0], XYZ2[:0])
    fails(-1, f"{who}: m = 2 segments (1 to 2^22) need seg_a and seg_b", L.pnr_point_segment_distance, ctx.h, ptr(XYZ2), 2, ptr(XYZ2), None, 2, ptr(d), None)
    fails(-1, f"{who}: n = -1 points (at most 2^22) need pts and d_out", L.pnr_point_segment_distance, ctx.h, None, -1, ptr(XYZ2), ptr(XYZ2), 2, None, None)
    fails(-1, f"{who}: n = 2 points (at most 2^22) need pts and d_out", L.pnr_point_segment_distance, ctx.h, ptr(XYZ2), 2, ptr(XYZ2), ptr(XYZ2), 2, None, None)
    fails(-1, f"{who}: a coordinate is not finite", ctx.point_segment_distance, NAN2, XYZ2, XYZ2)
    fails(-1, f"{who}: a coordinate is not finite", ctx.point_segment_distance, XYZ2, XYZ2, NAN2)
    fails(-1, f"{who}: m = 0 segments (1 to 2^22) need seg_a and seg_b", L.pnr_point_segment_distance, ctx.h, None, -1, ptr(XYZ2), ptr(XYZ2), 0, None, None)  # m before n
    who = "pnr_nearest_other"
    lab = np.array([0, 1], np.int32)
    fails(-1, "null ctx", L.pnr_nearest_other, None, None, None, 0, None, None)
    fails(-1, f"{who}: n = 0 points (1 to 2^22) need xyz, label, d_out and j_out", ctx.nearest_other, XYZ2[:0], lab[:0])
    fails(-1, f"{who}: n = 2 points (1 to 2^22) need xyz, label, d_out and j_out", L.pnr_nearest_other, ctx.h, ptr(XYZ2), ptr(lab), 2, ptr(d), None)
    fails(-1, f"{who}: a coordinate is not finite", ctx.nearest_other, NAN2, lab)


def test_tree_distance(ctx):
    L, who = ctx.L, "pnr_tree_distance"
    run = lambda a=XYZ2, b=XYZ2, **kw: ctx.tree_distance(a, PAR2[:len(a)], b, PAR2[:len(b)], **kw)
    res = lib.DistanceResult()

    def direct(o=None, r=res, capA=0, capB=0, h=ctx.h):
        return L.pnr_tree_distance(h, ptr(XYZ2), ptr(PAR2), 2, ptr(XYZ2), ptr(PAR2), 2, None if o is None else C.byref(o), None if r is None else C.byref(r), None, None, capA, None, None, capB)

    fails(-1, "null argument", direct, h=None)
    fails(-1, "null argument", direct, r=None)
    fails(-1, f"{who}: zscale = 0 must be positive", run, zscale=0)
    fails(-1, f"{who}: zscale = inf must be positive", run, zscale=np.inf)
    fails(-1, f"{who}: step = -1 must not be negative", run, step=-1)
    fails(-1, f"{who}: thr is not finite", run, thr=np.inf)
    fails(-1, f"{who}: negative capacity", direct, capA=-1)
    fails(-1, f"{who}: negative capacity", direct, capB=-1)
    fails(-1, f"{who}: tree A has 0 nodes (1 to 2^22)", run, a=XYZ2[:0])
    fails(-1, f"{who}: tree B has 0 nodes (1 to 2^22)", run, b=XYZ2[:0])
    # the order: zscale, step, thr, the capacities, tree A, tree B
    fails(-1, "null argument", direct, r=None, o=lib.DistanceOpts(0, 1, 2))
    fails(-1, f"{who}: zscale = 0 must be positive", run, zscale=0, step=-1)
    fails(-1, f"{who}: step = -1 must not be negative", run, step=-1, thr=np.inf)
    fails(-1, f"{who}: thr is not finite", direct, o=lib.DistanceOpts(1, 1, np.inf), capA=-1)
    fails(-1, f"{who}: tree A has 0 nodes (1 to 2^22)", run, a=XYZ2[:0], b=XYZ2[:0])
    assert run()["ab"]["n"] == 4  # the two nodes and the two interior points of a segment of length 3


def test_join_trees(ctx):
    L, who = ctx.L, "pnr_join_trees"
    forest = np.array([-1, -1], np.int32)
    run = lambda xyz=XYZ2, **kw: ctx.join_trees(xyz, forest[:len(xyz)], **kw)
    nb = C.c_int64()

    def direct(o=None, n=2, cap=0, count=C.byref(nb), h=ctx.h):
        return L.pnr_join_trees(h, ptr(XYZ2), ptr(forest), n, None if o is None else C.byref(o), None, None, None, None, cap, count, None, None)

    fails(-1, "null argument", direct, h=None)
    fails(-1, "null argument", direct, count=None)
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz and parent", run, xyz=XYZ2[:0])
    fails(-1, f"{who}: zscale = 0 must be positive", run, zscale=0)
    fails(-1, f"{who}: gap = -1 must not be negative", run, gap=-1)
    fails(-1, f"{who}: gap = inf must not be negative", run, gap=np.inf)
    fails(-1, f"{who}: root = 2 outside [-1, 2)", run, root=2)
    fails(-1, f"{who}: cap_bridges = 1 needs bridges_out", direct, cap=1)
    fails(-1, f"{who}: cap_bridges = -1 needs bridges_out", direct, cap=-1)
    fails(-1, f"{who}: node 1 has a coordinate that is not finite", run, xyz=NAN2)
    # the order: the count, n, zscale, gap, root, the capacity, the coordinates
    fails(-1, "null argument", direct, count=None, n=0)
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz and parent", direct, n=0, o=lib.JoinOpts(0, 0, -1))
    fails(-1, f"{who}: zscale = 0 must be positive", run, zscale=0, gap=-1)
    fails(-1, f"{who}: gap = -1 must not be negative", run, gap=-1, root=2)
    fails(-1, f"{who}: root = 2 outside [-1, 2)", direct, o=lib.JoinOpts(1, 0, 2), cap=1)
    fails(-1, f"{who}: root = 5 outside [-1, 2)", run, xyz=NAN2, root=5)
    assert len(run()[3]) == 1


def test_geodesic_bridges(ctx):
    L, who = ctx.L, "pnr_geodesic_bridges"
    forest = np.array([-1, -1], np.int32)
    run = lambda **kw: ctx.join_trees_geodesic(XYZ2, forest, **kw)
    nb, npath = C.c_int64(), C.c_int64()
    br = np.zeros(1, lib.GEO_BRIDGE)

    def direct(o=None, n=2, out=None, cap=0, cap_path=0, count=C.byref(nb), h=ctx.h):
        return L.pnr_geodesic_bridges(h, ptr(XYZ2), ptr(forest), n, None if o is None else C.byref(o), None, ptr(out), cap, count, None, cap_path, C.byref(npath))

    fails(-1, "null argument", direct, h=None)
    fails(-1, "null argument", direct, count=None)
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz and parent", direct, n=0)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256)
    fails(-1, f"{who}: step = -1 must not be negative", run, step=-1)
    fails(-1, f"{who}: step = inf must not be negative", run, step=np.inf)
    fails(-1, f"{who}: cost[5] = 0, every entry is at least 1", run, cost=COST0)
    fails(-1, f"{who}: cap_bridges = 1 needs bridges_out", direct, cap=1)
    fails(-1, f"{who}: cap_path = 1 needs path_vox", direct, cap_path=1)
    fails(-1, f"{who}: cap_path = -1 needs path_vox", direct, cap_path=-1)
    # the order: the counts, n, thr, step, the cost table, the two capacities
    fails(-1, "null argument", direct, count=None, n=0)
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz and parent", direct, n=0, o=lib.GeoJoinOpts(256, 0, 1, None))
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", run, thr=256, step=-1)
    fails(-1, f"{who}: step = -1 must not be negative", run, step=-1, cost=COST0)
    fails(-1, f"{who}: cost[5] = 0, every entry is at least 1", direct, o=lib.GeoJoinOpts(0, 0, 1, COST0.ctypes.data_as(C.POINTER(C.c_uint16))), cap=1)
    fails(-1, f"{who}: cap_bridges = -1 needs bridges_out", direct, cap=-1, cap_path=1)
    fails(-1, f"{who}: cap_path = 1 needs path_vox", direct, out=br, cap=1, cap_path=1)


def test_render_tree_and_coverage(ctx):
    L, who = ctx.L, "pnr_render_tree"

    def direct(o=None, n=2, w=4, h=4, l=2, ctx_h=ctx.h):
        return L.pnr_render_tree(ctx_h, ptr(XYZ2), ptr(RAD2), ptr(PAR2), n, w, h, l, None if o is None else C.byref(o), None, None)

    fails(-1, "null ctx", direct, ctx_h=None, n=-1)
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, radius and parent", direct, n=-1)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", direct, o=lib.RenderOpts(1, 1, 0, 256))
    fails(-1, f"{who}: the grid 0 x 3 x 2 needs sides from 1 and at most 2^40 voxels", ctx.render_tree, XYZ2, RAD2, PAR2, (2, 3, 0))
    fails(-1, f"{who}: zscale = 0 must be positive", ctx.render_tree, XYZ2, RAD2, PAR2, (2, 4, 4), zscale=0)
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, radius and parent", direct, n=-1, o=lib.RenderOpts(1, 1, 0, 256))
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", direct, o=lib.RenderOpts(1, 1, 0, 256), w=0)
    fails(-1, f"{who}: the grid 0 x 3 x 2 needs sides from 1 and at most 2^40 voxels", ctx.render_tree, XYZ2, RAD2, PAR2, (2, 3, 0), zscale=0)
    who = "pnr_tree_coverage"
    fails(-1, "null ctx", L.pnr_tree_coverage, None, None, None, None, -1, None, None, None, None, None, None, None)
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, radius and parent", L.pnr_tree_coverage, ctx.h, None, None, None, -1, None, None, None, None, None, None, None)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", ctx.tree_coverage, XYZ2, RAD2, PAR2, thr=256)
    fails(-1, f"{who}: zscale = 0 must be positive", ctx.tree_coverage, XYZ2, RAD2, PAR2, zscale=0)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", ctx.tree_coverage, XYZ2, RAD2, PAR2, thr=256, zscale=0)
    assert ctx.tree_coverage(XYZ2, RAD2, PAR2)["n_vox"] == 32


def test_filter_volume(ctx):
    L, who = ctx.L, "pnr_filter_volume"
    fails(-1, "null argument", L.pnr_filter_volume, ctx.h, None)
    fails(-1, "null argument", L.pnr_filter_volume, None, C.byref(lib.FilterOpts(1, 0)))
    fails(-1, f"{who}: median = 1, not 0, 2 or 3", ctx.filter_volume, median=1)
    fails(-1, f"{who}: tophat_r = 65 outside [0, 64]", ctx.filter_volume, tophat=65)
    fails(-1, f"{who}: tophat_r = -1 outside [0, 64]", ctx.filter_volume, tophat=-1)
    fails(-1, f"{who}: median = 1, not 0, 2 or 3", ctx.filter_volume, median=1, tophat=65)


def test_frangi_family_on_a_volume(ctx):
    L = ctx.L
    fails(-1, "kept planes [1,1) outside [0,2)", ctx.frangi_slab, 1, 1)
    fails(-1, "kept planes [0,3) outside [0,2)", ctx.frangi_slab, 0, 3)
    fails(-1, "sigma must be positive", ctx.gaussian, 0.0)
    fails(-1, "sigma must be positive", ctx.hessian, 0.0)
    # a null output of pnr_gaussian is answered as a missing volume is (PNR_E_STATE), a null context of a tool as an argument (PNR_E_ARG)
    fails(-4, "pnr_gaussian: no volume set", L.pnr_gaussian, ctx.h, 1.0, None)
    fails(-4, "pnr_gaussian: no volume set", L.pnr_gaussian, ctx.h, 0.0, None)  # before sigma
    fails(-1, "null ctx", L.pnr_skeletonize, None, None, None, None, None, None, 0)


def test_null_context_of_the_frangi_family():
    L = lib.load()
    a, b = C.c_float(), C.c_float()
    F = np.zeros(32, np.float32)
    fails(-4, "pnr_frangi: no volume set", L.pnr_frangi, None, C.byref(a), C.byref(b))
    fails(-4, "pnr_frangi_slab: no volume set", L.pnr_frangi_slab, None, 0, 1, C.byref(a), C.byref(b))
    fails(-4, "pnr_quantise_j8: no volume set", L.pnr_quantise_j8, None, 0.0, 1.0)
    fails(-4, "pnr_gaussian: no volume set", L.pnr_gaussian, None, 1.0, ptr(F))
    fails(-4, "pnr_hessian: no volume set", L.pnr_hessian, None, 1.0, None, None, None, None, None, None)


def test_no_volume_set(bare):
    """the state check comes after every argument check of a call (an argument error wins), and before any work"""
    L, h = bare.L, bare.h
    forest = np.array([-1, -1], np.int32)
    a, b, n = C.c_float(), C.c_float(), C.c_int64()
    F = np.zeros(32, np.float32)
    fails(-4, "pnr_frangi: no volume set", bare.frangi)
    fails(-4, "pnr_frangi_slab: no volume set", bare.frangi_slab, 0, 1)
    fails(-4, "pnr_quantise_j8: no volume set", bare.quantise_j8, 0.0, 1.0)
    fails(-4, "pnr_gaussian: no volume set", L.pnr_gaussian, h, 1.0, ptr(F))
    fails(-4, "pnr_hessian: no volume set", L.pnr_hessian, h, 1.0, None, None, None, None, None, None)
    fails(-4, "pnr_get_volume: no volume set", L.pnr_get_volume, h, ptr(F))
    fails(-4, "pnr_filter_volume: no volume set", bare.filter_volume)  # (before "nothing to do")
    fails(-4, "pnr_filter_volume: no volume set", bare.filter_volume, median=3)
    fails(-1, "pnr_filter_volume: median = 1, not 0, 2 or 3", bare.filter_volume, median=1)
    fails(-4, "pnr_label_components: no volume set", bare.label_components, labels=False)
    fails(-1, "pnr_label_components: min_size = 0 must be at least 1", bare.label_components, labels=False, min_size=0)
    fails(-4, "pnr_despeckle_volume: no volume set", bare.despeckle, 1)
    fails(-4, "pnr_distance_transform: no volume set", L.pnr_distance_transform, h, None, None, None, None, 0, None)
    fails(-1, "pnr_distance_transform: n = -1 positions (at most 2^28) need xyz and d2_at", L.pnr_distance_transform, h, None, None, None, None, -1, None)
    fails(-4, "pnr_skeletonize: no volume set", L.pnr_skeletonize, h, None, None, None, None, None, 0)
    fails(-1, "pnr_skeletonize: cap = -1 is negative", L.pnr_skeletonize, h, None, None, None, None, None, -1)
    fails(-4, "pnr_geodesic_distance: no volume set", L.pnr_geodesic_distance, h, ptr(XYZ2), None, 2, None, None, None, None, None, 0, None, None, 0, None, None)
    fails(-1, "pnr_geodesic_distance: path_cap = -1 outside [0, 65536]", L.pnr_geodesic_distance, h, ptr(XYZ2), None, 2, None, None, None, None, None, 0, None, None, -1, None, None)
    fails(-4, "pnr_measure_radii: no volume set", bare.measure_radii, XYZ2)
    fails(-1, "pnr_measure_radii: bg_permille = 1000 outside [0, 999]", bare.measure_radii, XYZ2, bg_permille=1000)
    fails(-4, "pnr_geodesic_bridges: no volume set", bare.join_trees_geodesic, XYZ2, forest)
    fails(-1, "pnr_geodesic_bridges: cap_path = 1 needs path_vox", L.pnr_geodesic_bridges, h, ptr(XYZ2), ptr(forest), 2, None, None, None, 0, C.byref(n), None, 1, C.byref(n))
    fails(-4, "pnr_tree_coverage: no volume set", L.pnr_tree_coverage, h, ptr(XYZ2), ptr(RAD2), ptr(PAR2), 2, None, None, None, None, None, None, None)
    fails(-1, "pnr_tree_coverage: zscale = 0 must be positive", L.pnr_tree_coverage, h, ptr(XYZ2), ptr(RAD2), ptr(PAR2), 2, C.byref(lib.RenderOpts(0, 1, 0, -1)), None, None, None, None, None, None)
    fails(-4, "no volume set", bare.trace_replay, np.zeros(0, lib.SEED_DT))
    fails(-4, "no volume set", bare.replay, np.zeros(0, lib.SEED_DT), np.zeros(0, np.int32), np.zeros((0, 4), lib.XEST_DT))
    # the tools that need no volume run on this context
    assert bare.render_tree(XYZ2, RAD2, PAR2, (2, 4, 4)).shape == (2, 4, 4)
    assert len(bare.join_trees(XYZ2, forest)[3]) == 1
