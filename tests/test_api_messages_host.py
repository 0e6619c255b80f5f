"""CPU: the return code and the full pnr_last_error() text of every argument check the pure-host entry points of the C boundary make,
one bad value per check and in the order the checks run (two bad values: the earlier check's text wins); and pnr_skeleton_forest on a
grid small enough to restate Kruskal beside it."""
import ctypes as C
import numpy as np
import pnr_amd
from pnr_amd import lib


def fails(code, text, call, *args, **kw):
    """a wrapper of lib.py raises PnrError with the code and the text; an entry point called directly returns the code and leaves the text"""
    try:
        rc = call(*args, **kw)
    except lib.PnrError as e:
        assert str(e) == f"libpnr_hip error {code}: {text}"
        return
    assert rc == code and lib.load().pnr_last_error().decode() == text, (rc, lib.load().pnr_last_error().decode())


def ptr(a):
    return a.ctypes.data


XYZ2 = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
PAR2 = np.array([-1, 0], np.int32)
RAD2 = np.ones(2, np.float32)


def test_tree_sample():
    L, n = lib.load(), C.c_int64()
    who = "pnr_tree_sample"
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, parent and n_out", L.pnr_tree_sample, None, None, -1, 1.0, 1.0, None, None, 0, C.byref(n))
    fails(-1, f"{who}: n = 2 nodes (at most 2^22) need xyz, parent and n_out", L.pnr_tree_sample, ptr(XYZ2), ptr(PAR2), 2, 1.0, 1.0, None, None, -1, C.byref(n))
    fails(-1, f"{who}: n = 2 nodes (at most 2^22) need xyz, parent and n_out", L.pnr_tree_sample, ptr(XYZ2), ptr(PAR2), 2, 0.0, 1.0, None, None, 0, None)
    fails(-1, f"{who}: zscale = 0 must be positive", lib.tree_sample, XYZ2, PAR2, zscale=0)
    fails(-1, f"{who}: zscale = inf must be positive", lib.tree_sample, XYZ2, PAR2, zscale=np.inf)
    fails(-1, f"{who}: step = -1 must not be negative", lib.tree_sample, XYZ2, PAR2, step=-1)
    fails(-1, f"{who}: step = inf must not be negative", lib.tree_sample, XYZ2, PAR2, step=np.inf)
    fails(-1, f"{who}: zscale = -2 must be positive", lib.tree_sample, XYZ2, PAR2, zscale=-2, step=-1)  # zscale before step
    assert lib.tree_sample(XYZ2, PAR2, count_only=True) == 3


def test_join_reroot():
    L = lib.load()
    who = "pnr_join_reroot"
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need parent", lib.join_reroot, np.zeros(0, np.int32))
    fails(-1, f"{who}: n = 2 nodes (1 to 2^22) need parent", L.pnr_join_reroot, None, 2, None, 0, -1, None, None, None)
    fails(-1, f"{who}: 2 bridges (0 to n - 1) need bridges", lib.join_reroot, PAR2, [(0, 1), (0, 1)])
    fails(-1, f"{who}: 1 bridges (0 to n - 1) need bridges", L.pnr_join_reroot, ptr(PAR2), 2, None, 1, -1, None, None, None)
    fails(-1, f"{who}: -1 bridges (0 to n - 1) need bridges", L.pnr_join_reroot, ptr(PAR2), 2, None, -1, -1, None, None, None)
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need parent", L.pnr_join_reroot, ptr(PAR2), 0, None, -1, -1, None, None, None)  # n before nb


def test_skeleton_forest():
    L, n = lib.load(), C.c_int64()
    who = "pnr_skeleton_forest"
    vox = np.array([3, 5], np.int64)

    def call(v=vox, k=2, w=4, h=3, l=2, cap=0, count=C.byref(n)):
        return L.pnr_skeleton_forest(None if v is None else ptr(v), k, w, h, l, None, cap, count)

    fails(-1, "null argument", call, count=None)
    fails(-1, f"{who}: k = -1 voxels (0 to 2^31 - 1) need vox", call, k=-1)
    fails(-1, f"{who}: k = 2 voxels (0 to 2^31 - 1) need vox", call, v=None)
    fails(-1, f"{who}: grid 4 x 3 x 0", call, l=0)
    fails(-1, f"{who}: grid 2147483648 x 3 x 2", call, w=1 << 31)
    fails(-1, f"{who}: grid 2097152 x 1048576 x 2", call, w=1 << 21, h=1 << 20)  # more than 2^40 voxels
    fails(-1, f"{who}: cap = -1 is negative", call, cap=-1)
    fails(-1, f"{who}: voxel 24 of node 1 is outside the grid", call, v=np.array([3, 24], np.int64))
    fails(-1, f"{who}: voxel -1 of node 0 is outside the grid", call, v=np.array([-1, 24], np.int64))
    fails(-1, f"{who}: voxel 3 is listed twice", call, v=np.array([3, 3], np.int64))
    # the order of the checks: count, k, grid, cap, the voxels
    fails(-1, "null argument", call, count=None, k=-1)
    fails(-1, f"{who}: k = -1 voxels (0 to 2^31 - 1) need vox", call, k=-1, l=0)
    fails(-1, f"{who}: grid 4 x 3 x 0", call, l=0, cap=-1)
    fails(-1, f"{who}: cap = -1 is negative", call, cap=-1, v=np.array([3, 3], np.int64))
    fails(-1, f"{who}: voxel 99 of node 2 is outside the grid", call, v=np.array([3, 3, 99], np.int64), k=3)  # the range before the duplicates


def test_skeleton_forest_small_grid_against_kruskal():
    """3 x 3 x 2 grid, 6 voxels in no order: the unit square of the x = 0 face (four steps of len2 = 1 and two of len2 = 2 tie) and a
    diagonal pair on the x = 2 face, which no 26-step reaches from x = 0"""
    shape, w, h = (2, 3, 3), 3, 3
    at = lambda x, y, z: (z * h + y) * w + x
    vox = np.array([at(0, 1, 1), at(2, 0, 0), at(0, 0, 0), at(0, 1, 0), at(2, 1, 1), at(0, 0, 1)], np.int64)
    p = [(v % w, v // w % h, v // (w * h)) for v in vox.tolist()]
    pairs = sorted((sum((a - b) ** 2 for a, b in zip(p[i], p[j])), i, j) for i in range(6) for j in range(i + 1, 6)
                   if max(abs(a - b) for a, b in zip(p[i], p[j])) == 1)
    assert [e[0] for e in pairs] == [1, 1, 1, 1, 2, 2, 2]
    up, want = list(range(6)), []
    find = lambda a: a if up[a] == a else find(up[a])
    for len2, i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
            want.append((i, j, len2))
    want.sort()
    got = pnr_amd.skeleton_forest(vox, shape)
    assert len(got) == 4 == len(vox) - 2
    assert [(int(e["lo"]), int(e["hi"])) for e in got] == [(i, j) for i, j, _ in want]
    assert np.array_equal(got["d"], np.sqrt(np.array([len2 for _, _, len2 in want], np.float32)))
    # a capacity below the count: the full count, the first edges
    L, n, part = lib.load(), C.c_int64(), np.zeros(2, lib.BRIDGE)
    assert L.pnr_skeleton_forest(ptr(vox), 6, 3, 3, 2, ptr(part), 2, C.byref(n)) == 0 and n.value == 4 and np.array_equal(part, got[:2])


def test_join_expand():
    L, n2 = lib.load(), C.c_int64()
    who = "pnr_join_expand"
    br = np.zeros(1, lib.GEO_BRIDGE)
    path = np.zeros(1, np.int64)

    def call(xyz=XYZ2, par=PAR2, n=2, b=None, nb=0, pv=None, n_path=0, w=4, h=3, l=2, cap=0, count=C.byref(n2)):
        a = [None if v is None else ptr(v) for v in (xyz, par, b, pv)]
        return L.pnr_join_expand(a[0], a[1], n, a[2], nb, a[3], n_path, w, h, l, None, None, None, cap, count, None)

    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz, parent and n_nodes", call, n=0)
    fails(-1, f"{who}: n = 2 nodes (1 to 2^22) need xyz, parent and n_nodes", call, count=None)
    fails(-1, f"{who}: 2 bridges (0 to n - 1) need bridges", call, b=br, nb=2)
    fails(-1, f"{who}: 1 bridges (0 to n - 1) need bridges", call, nb=1)
    fails(-1, f"{who}: 1 bridges need path_vox", call, b=br, nb=1)
    fails(-1, f"{who}: 0 bridges need path_vox", call, n_path=-1)
    fails(-1, f"{who}: 0 bridges need path_vox", call, cap=-1)
    fails(-1, f"{who}: the grid 0 x 3 x 2 needs sides from 1 and below 2^24", call, w=0)
    fails(-1, f"{who}: the grid 4 x 16777216 x 2 needs sides from 1 and below 2^24", call, h=1 << 24)
    fails(-1, f"{who}: parent[1] = 5 outside [-1, 2)", call, par=np.array([-1, 5], np.int32))
    # the order of the checks: n, the bridges, the paths, the grid, the parents
    fails(-1, f"{who}: n = 0 nodes (1 to 2^22) need xyz, parent and n_nodes", call, n=0, nb=-1)
    fails(-1, f"{who}: -1 bridges (0 to n - 1) need bridges", call, nb=-1, n_path=-1)
    fails(-1, f"{who}: 1 bridges need path_vox", call, b=br, nb=1, w=0)
    fails(-1, f"{who}: the grid 4 x 3 x 0 needs sides from 1 and below 2^24", call, l=0, par=np.array([-1, 5], np.int32))
    assert call(b=br, nb=0, pv=path) == 0 and n2.value == 2


def test_render_items():
    L, k = lib.load(), C.c_int64()
    who = "pnr_render_items"

    def call(n=2, w=4, h=3, l=2, o=None, piece=0, box=0, cap=0, count=C.byref(k)):
        return L.pnr_render_items(ptr(XYZ2), ptr(RAD2), ptr(PAR2), n, w, h, l, None if o is None else C.byref(o), piece, box, None, cap, count)

    fails(-1, f"{who}: piece and box (not negative) need a count, and items_out for cap = 0", call, piece=-1)
    fails(-1, f"{who}: piece and box (not negative) need a count, and items_out for cap = 0", call, box=-1)
    fails(-1, f"{who}: piece and box (not negative) need a count, and items_out for cap = 0", call, count=None)
    fails(-1, f"{who}: piece and box (not negative) need a count, and items_out for cap = 3", call, cap=3)
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, radius and parent", call, n=-1)
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", call, o=lib.RenderOpts(1, 1, 0, 256))
    fails(-1, f"{who}: thr = -2 outside [-1, 255]", call, o=lib.RenderOpts(1, 1, 0, -2))
    fails(-1, f"{who}: the grid 0 x 3 x 2 needs sides from 1 and at most 2^40 voxels", call, w=0)
    fails(-1, f"{who}: the grid 2147483648 x 3 x 2 needs sides from 1 and at most 2^40 voxels", call, w=1 << 31)
    fails(-1, f"{who}: the grid 2097152 x 1048576 x 2 needs sides from 1 and at most 2^40 voxels", call, w=1 << 21, h=1 << 20)
    fails(-1, f"{who}: zscale = 0 must be positive", call, o=lib.RenderOpts(0, 1, 0, -1))
    fails(-1, f"{who}: zscale = 0 must be positive", lib.render_items, XYZ2, RAD2, PAR2, (2, 3, 4), zscale=0)
    # the order of the checks: the capacity line, the tree (n, thr), the grid, the tree's values
    fails(-1, f"{who}: piece and box (not negative) need a count, and items_out for cap = 0", call, piece=-1, n=-1)
    fails(-1, f"{who}: n = -1 nodes (at most 2^22) need xyz, radius and parent", call, n=-1, o=lib.RenderOpts(1, 1, 0, 256))
    fails(-1, f"{who}: thr = 256 outside [-1, 255]", call, o=lib.RenderOpts(1, 1, 0, 256), w=0)
    fails(-1, f"{who}: the grid 4 x 3 x 0 needs sides from 1 and at most 2^40 voxels", call, l=0, o=lib.RenderOpts(0, 1, 0, -1))
    assert len(lib.render_items(XYZ2, RAD2, PAR2, (2, 3, 4))) >= 1


def test_pair_tiles_and_radius_offsets():
    L, k = lib.load(), C.c_int64()
    text = "pnr_pair_tiles: %d x %d (at least 1 x 1), split = %d and budget = %d (not negative) need a count, and tiles for cap = %d"
    fails(-1, text % (0, 1, 0, 0, 0), lib.pair_tiles, 0, 1)
    fails(-1, text % (1, 0, 0, 0, 0), lib.pair_tiles, 1, 0)
    fails(-1, text % (1, 1, -1, 0, 0), lib.pair_tiles, 1, 1, split=-1)
    fails(-1, text % (1, 1, 0, -1, 0), lib.pair_tiles, 1, 1, budget=-1)
    fails(-1, text % (1, 1, 0, 0, 0), L.pnr_pair_tiles, 1, 1, 0, 0, None, 0, None)
    fails(-1, text % (1, 1, 0, 0, 2), L.pnr_pair_tiles, 1, 1, 0, 0, None, 2, C.byref(k))
    assert len(lib.pair_tiles(1, 1)) == 1
    fails(-1, "pnr_radius_offsets: rmax = 0 outside [1, 64], or null count", lib.radius_offsets, 2.0, 0)
    fails(-1, "pnr_radius_offsets: rmax = 65 outside [1, 64], or null count", lib.radius_offsets, 2.0, 65)
    fails(-1, "pnr_radius_offsets: rmax = 3 outside [1, 64], or null count", L.pnr_radius_offsets, 2.0, 3, 0, None, None, None, None, 0, None)


def test_replay():
    L = lib.load()
    p = pnr_amd.make_params(sigmas=(2,), ni=4, np_=8)
    seeds, T, xc = np.zeros(1, lib.SEED_DT), np.zeros(2, np.int32), np.zeros((2, 4), lib.XEST_DT)
    fails(-1, "bad dimensions", lib.replay, p, (0, 8, 8), seeds, T, xc)
    fails(-1, "bad dimensions", lib.replay, p, (8, 8, -1), seeds, T, xc)
    n = C.c_int64()
    fails(-1, "null argument", L.pnr_replay_traces, None, 8, 8, 8, None, 0, None, None, None, 0, C.byref(n), None, 0, C.byref(n), None)
    fails(-1, "null argument", L.pnr_replay_traces, C.byref(p), 8, 8, 8, None, 1, None, None, None, 0, C.byref(n), None, 0, C.byref(n), None)
    fails(-1, "null argument", L.pnr_replay_traces, None, 0, 8, 8, None, 0, None, None, None, 0, C.byref(n), None, 0, C.byref(n), None)  # before the dimensions
    nodes, links, used = lib.replay(p, (8, 8, 8), seeds[:0], T[:0], xc[:0])
    assert len(links) == 0 and used == 0


def test_sched_playback_window():
    """a window below 2: pnr_sched_playback2 (behind lib.sched_playback) refuses it, pnr_sched_playback clamps it"""
    L = lib.load()
    p = pnr_amd.make_params(sigmas=(2,), ni=4, np_=8)
    called = []
    trace = lambda pd: called.append(1) or (0, np.zeros((0, 8), np.float32))
    fails(-1, "playback engine: a window of 1 trace slots", lib.sched_playback, p, (8, 8, 8), np.zeros(1, lib.SEED_DT), trace, window=1)
    fails(-1, "playback engine: a window of -3 trace slots", lib.sched_playback, p, (8, 8, 8), np.zeros(0, lib.SEED_DT), trace, window=-3)
    fails(-1, "bad dimensions", lib.sched_playback, p, (0, 8, 8), np.zeros(1, lib.SEED_DT), trace, window=1)  # the dimensions before the window
    fails(-1, "bad rank / world / exchange", lib.sched_playback, p, (8, 8, 8), np.zeros(1, lib.SEED_DT), trace, rank=1, world=1, window=1)
    assert not called
    n = [C.c_int64() for _ in range(4)]
    cb = lib.TRACE_FN(lambda user, pd, T, xc: 1)
    rc = L.pnr_sched_playback(C.byref(p), 8, 8, 8, None, 0, 0, 1, C.cast(None, lib.ALLGATHER_FN), None, 0, cb, None, 1, 1, 4, 0, -1, None, 0, C.byref(n[0]), None, 0,
                              C.byref(n[1]), C.byref(n[2]), C.byref(n[3]))
    assert rc == 0 and n[1].value == 0 and n[2].value == 0


def test_reconstruct_link_out_of_range():
    nodes = np.zeros(3, lib.NODE_DT)
    fails(-1, "link index out of range", lib.reconstruct, nodes, [[1, 3]])
    fails(-1, "link index out of range", lib.reconstruct, nodes, [[-1, 2]])
    fails(-1, "link index out of range", lib.reconstruct_stage, nodes, [[1, 3]], 2)
    fails(-1, "stage 5 outside [1, 4]", lib.reconstruct_stage, nodes, [[1, 3]], 5)  # the stage before the links
    fails(-1, "null argument", lib.reconstruct, nodes[:0], [])
