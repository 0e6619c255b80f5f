"""The stack of 2048 x 2048 x 513 voxels (N > 2^31) that takes six volume tools -- skeleton, geodesic, geodesic join, watershed, coverage, radius --
above the sign bit of a 32-bit voxel index, and a stack of 96 x 64 x 41 with the same relative placement that numpy can restate as a whole.

The stack is background (0) but for two small blocks: one in the first planes, one in the last plane z = l - 1, in the corner of the
three far faces, so that it holds the stack's last voxel.  l - 1 is a multiple of every tool's tile depth: the far block lies in the
one-plane partial tile at the end, and every voxel of it has an index above 2^31 on the large stack.  Both blocks start at even
coordinates (the thinning rule's subfields are the parities of the absolute coordinates) and cross tile faces in x and y; the near block
crosses them in z too.  Every tool is called with a threshold of at least 1, so what lies outside the blocks is outside the mask,
impassable or background: nothing floods from one block to the other, and the numpy restatement of the rule on a crop around each block,
translated, is the whole answer.

Per tool: X_case(shape) -> the blocks and the call's arguments in absolute coordinates; X_want(case) -> the expected result from the
restatement on the crops, combined; X_whole(case) -> the same from the restatement on the whole stack (the small shape only).
test_bigvol_host.py holds X_want against X_whole on the CPU; the GPU tests hold the kernels against X_want at both shapes."""
import numpy as np
import radius_ref

SHAPE = (513, 2048, 2048)  # (l, h, w)
SMALL = (41, 64, 96)
NEAR, FAR = (10, 14, 44), (1, 30, 70)  # the extents of the two blocks
ZD = 2.0
INDEX = np.int64  # the type of every absolute voxel index formed here
F = np.float32


def tile_of(header, prefix):
    """(TZ, TY, TX) of pnr_amd/csrc/<header>"""
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pnr_amd", "csrc", header)).read()
    t = dict(re.findall(r"constexpr int %s_(TX|TY|TZ) = (\d+);" % prefix, txt))
    return int(t["TZ"]), int(t["TY"]), int(t["TX"])


def origins(shape):
    """(z0, y0, x0) of the near and of the far block"""
    l, h, w = shape
    return (2, 4, 26), (l - 1, h - FAR[1], w - FAR[2])


def check_placement(blocks, shape, tile):
    """the placement rules for a tool whose tile is `tile` = (TZ, TY, TX); -> the smallest absolute voxel index of the far block"""
    l, h, w = shape
    (on, near), (of, far) = blocks
    for o in (on, of):
        assert all(v % 2 == 0 for v in o), o
    crosses = lambda o, n, t: (o + n - 1) // t > o // t
    assert all(crosses(o, n, t) for o, n, t in zip(on, near.shape, tile)), "the near block crosses a tile face on every axis"
    assert all(crosses(o, n, t) for o, n, t in list(zip(of, far.shape, tile))[1:]), "the far block crosses a tile face in y and x"
    assert (l - 1) % tile[0] == 0 and of[0] == l - 1 and far.shape[0] == 1, "the far block lies in the one-plane partial tile"
    assert tuple(o + n for o, n in zip(of, far.shape)) == (l, h, w), "the far block holds the last voxel"
    assert on[0] + near.shape[0] < of[0]
    return int(INDEX(of[2]) + INDEX(w) * (INDEX(of[1]) + INDEX(h) * INDEX(of[0])))


def stack_crop(blocks, shape, lo, hi):
    """the part [lo, hi) of the stack, cut at the stack's faces -> (array, its origin (z0, y0, x0))"""
    lo = tuple(max(int(a), 0) for a in lo)
    hi = tuple(min(int(b), n) for b, n in zip(hi, shape))
    A = np.zeros(tuple(b - a for a, b in zip(lo, hi)), np.uint8)
    for o, B in blocks:
        s = [max(a, p) for a, p in zip(lo, o)]
        e = [min(b, p + n) for b, p, n in zip(hi, o, B.shape)]
        if all(a < b for a, b in zip(s, e)):
            A[tuple(slice(a - c, b - c) for a, b, c in zip(s, e, lo))] = B[tuple(slice(a - p, b - p) for a, b, p in zip(s, e, o))]
    return A, lo


def whole(blocks, shape):
    return stack_crop(blocks, shape, (0, 0, 0), shape)[0]


def crops(blocks, shape, margin=2):
    """a crop around every block: the block and `margin` (even: the origins stay even) voxels of background, or up to the stack's face"""
    assert margin % 2 == 0
    return [stack_crop(blocks, shape, [p - margin for p in o], [p + n + margin for p, n in zip(o, B.shape)]) for o, B in blocks]


def abs_index(idx, origin, cshape, shape):
    """linear indices of a crop -> linear indices of the stack"""
    idx = np.asarray(idx).astype(INDEX)
    _, ch, cw = cshape
    _, h, w = shape
    x, y, z = idx % INDEX(cw), idx // INDEX(cw) % INDEX(ch), idx // INDEX(cw * ch)
    return (x + INDEX(origin[2])) + INDEX(w) * ((y + INDEX(origin[1])) + INDEX(h) * (z + INDEX(origin[0])))


def index_of(x, y, z, shape):
    _, h, w = shape
    return INDEX(x) + INDEX(w) * (INDEX(y) + INDEX(h) * INDEX(z))


def split_points(xyz, regions, shape):
    """positions (x, y, z) of the stack, by the crop their centre voxel lies in -> ([(indices, float32 positions in the crop)] per crop,
    the indices of the others).  A position of a crop is its centre voxel minus the crop's origin: whole numbers, which every
    restatement centres on themselves."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    fin, c = radius_ref.centres(xyz, shape)
    taken = np.zeros(len(xyz), bool)
    out = []
    for C, o in regions:
        lo = np.array(o[::-1])
        inside = fin & ((c >= lo) & (c < lo + np.array(C.shape[::-1]))).all(1)
        assert not (inside & taken).any()
        taken |= inside
        out.append((np.flatnonzero(inside), (c[inside] - lo).astype(F)))
    return out, np.flatnonzero(~taken)


def open_stack(blocks, shape):
    """the zero stack with the blocks on the device, borrowed by a new context with zdist = ZD -> (tensor, context)"""
    import torch
    import pnr_amd
    t = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    for (z0, y0, x0), B in blocks:
        t[z0:z0 + B.shape[0], y0:y0 + B.shape[1], x0:x0 + B.shape[2]] = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    torch.cuda.synchronize()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=ZD), 0)
    c.set_volume_device(t.data_ptr(), shape, keepalive=t)
    return t, c


def untouched(t, blocks):
    """the borrowed tensor is as it was: nothing but the blocks' voxels is set"""
    import torch
    torch.cuda.synchronize()
    return int(torch.count_nonzero(t)) == sum(int(np.count_nonzero(B)) for _, B in blocks)


def _blocks(shape, near, far):
    on, of = origins(shape)
    assert near.shape == NEAR and far.shape == FAR
    return [(on, np.ascontiguousarray(near, np.uint8)), (of, np.ascontiguousarray(far, np.uint8))]


# ---- skeleton: outside the volume is background under the rule, so a block surrounded by background thins like the crop on its own; the
# crop's origin is even, so its voxels keep their subfields ----
def thin_case(shape):
    import thin_ref
    near = thin_ref.objects(NEAR, "blobs") | thin_ref.ball(NEAR, (5, 7, 8), 4) | thin_ref.ball(NEAR, (4, 6, 33), 4)
    far = thin_ref.objects(FAR, "blobs") | thin_ref.ball(FAR, (0, 12, 30), 7) | thin_ref.ball(FAR, (0, 27, 66), 5)
    assert far[-1, -1, -1]
    return dict(shape=shape, thr=100, blocks=_blocks(shape, np.where(near, 200, 0), np.where(far, 220, 0)))


THIN_SUMS = ("n_fg", "n_skel", "n_end", "n_branch", "n_isolated")


def thin_want(case):
    """-> (info, vox, deg): the sums over the crops, the rounds of the slowest (a block that has converged deletes nothing later)"""
    import thin_ref
    shape = case["shape"]
    per, vox, deg = [], [], []
    for C, o in crops(case["blocks"], shape):
        i, _, v, d = thin_ref.skeletonize(C, case["thr"])
        per.append(i)
        vox.append(abs_index(v, o, C.shape, shape))
        deg.append(d)
    vox, deg = np.concatenate(vox), np.concatenate(deg)
    order = np.argsort(vox, kind="stable")
    info = {k: sum(i[k] for i in per) for k in THIN_SUMS}
    info.update(n_vox=int(np.prod(shape, dtype=np.int64)), rounds=max(i["rounds"] for i in per), thr_used=case["thr"])
    return info, vox[order].astype(np.int64), deg[order]


def thin_whole(case):
    import thin_ref
    info, _, vox, deg = thin_ref.skeletonize(whole(case["blocks"], case["shape"]), case["thr"])
    return info, vox, deg


# ---- geodesic: a step needs both voxels passable, so no path leaves a block; sources, targets and the walk back stay in its crop ----
GEO_INFO = ("n_vox", "n_pass", "n_reached", "n_src", "n_src_dropped", "first_max", "d_max", "thr_used", "max_at")


def geo_case(shape):
    l, h, w = shape
    rng = np.random.default_rng(11)
    thr = 100
    near, far = (np.where(rng.random(s) < 0.85, rng.integers(thr, 256, s), rng.integers(0, thr, s)).astype(np.uint8) for s in (NEAR, FAR))
    blocks = _blocks(shape, near, far)
    # whole voxels (x, y, z): on the faces of the 32 x 8 x 4 tiles and inside them; the last one is dropped (background); two share a voxel
    at = [(31, 7, 3), (32, 8, 4), (60, 12, 9), (27, 5, 2), (60, 12, 9), (w - 1, h - 1, l - 1), (w - 33, h - 9, l - 1), (w - 32, h - 8, l - 1), (w - 60, h - 20, l - 1),
          (w - 50, h - 15, l - 1)]
    for (o, B) in blocks:
        for k, (x, y, z) in enumerate(at):
            if all(0 <= v - p < n for v, p, n in zip((z, y, x), o, B.shape)):
                B[z - o[0], y - o[1], x - o[2]] = 0 if k == len(at) - 1 else 200
    nudge = np.array([(0.25, -0.25, 0), (-0.5, 0.25, 0.25), (0, 0, -0.25)], F)
    src = (np.array(at, F) + nudge[np.arange(len(at)) % 3]).astype(F)
    labels = (2**31 - 1 - np.arange(len(at))).astype(np.int32)
    targets = np.concatenate([np.stack([xx + o[2], yy + o[1], zz + o[0]], 1) for o, B in blocks for zz, yy, xx in [np.nonzero(np.ones(B.shape, bool))]]).astype(F)
    first_far = int(np.prod(NEAR))
    walks = np.concatenate([rng.choice(first_far, 5, replace=False), first_far + rng.choice(int(np.prod(FAR)), 5, replace=False)])
    return dict(shape=shape, thr=thr, blocks=blocks, sources=src, labels=labels, targets=targets, path_cap=512, walks=np.sort(walks))


def _geo_result(parts, case, dropped_elsewhere):
    """parts: (V, origin, K, t, n kept, n dropped, target indices, positions in V) per crop (or the whole stack) -> the expected result"""
    import geodesic_ref as geo
    shape = case["shape"]
    m = len(case["targets"])
    out = dict(d=np.full(m, geo.UNREACHED, np.uint32), label=np.full(m, -1, np.int32), path_len={}, paths={})
    info = dict(n_vox=int(np.prod(shape, dtype=np.int64)), n_pass=0, n_reached=0, n_src=0, n_src_dropped=dropped_elsewhere, first_max=-1, d_max=0, thr_used=case["thr"],
                max_at=None)
    for V, o, K, t, kept, dropped, ti, tp in parts:
        i = geo.info(V, K, t, kept, dropped)
        for k in ("n_pass", "n_reached", "n_src", "n_src_dropped"):
            info[k] += i[k]
        if i["first_max"] >= 0:
            first = int(abs_index(i["first_max"], o, V.shape, shape))
            if info["first_max"] < 0 or (i["d_max"], -first) > (info["d_max"], -info["first_max"]):
                x, y, z = i["max_at"]
                info.update(first_max=first, d_max=i["d_max"], max_at=(x + o[2], y + o[1], z + o[0]))
        out["d"][ti], out["label"][ti] = geo.at(K, tp)
        sel = np.flatnonzero(np.isin(ti, case["walks"]))
        lens, walks = geo.paths(V, K, tp[sel], case["path_cap"], case["thr"], ZD)
        for j, n, wk in zip(ti[sel], lens, walks):
            out["path_len"][int(j)], out["paths"][int(j)] = int(n), abs_index(wk, o, V.shape, shape).astype(np.int64)
    out["info"] = info
    return out


def _geo_part(V, o, case, si, sp, ti, tp):
    import geodesic_ref as geo
    t = geo.threshold(V, case["thr"])
    src, kept, dropped = geo.sources(V, t, sp, case["labels"][si])
    K = geo.sweeps(V, src, case["thr"], ZD, inplace=True)[0]
    return V, o, K, t, kept, dropped, ti, tp


def geo_want(case):
    regions = crops(case["blocks"], case["shape"])
    (srcs, elsewhere), (tgts, none) = split_points(case["sources"], regions, case["shape"]), split_points(case["targets"], regions, case["shape"])
    assert len(none) == 0
    return _geo_result([_geo_part(V, o, case, si, sp, ti, tp) for (V, o), (si, sp), (ti, tp) in zip(regions, srcs, tgts)], case, len(elsewhere))


def geo_whole(case):
    V = whole(case["blocks"], case["shape"])
    all_src, all_tgt = np.arange(len(case["sources"])), np.arange(len(case["targets"]))
    return _geo_result([_geo_part(V, (0, 0, 0), case, all_src, case["sources"], all_tgt, case["targets"])], case, 0)


# ---- geodesic join: the flood is the geodesic one, so no meet edge and no bridge joins the blocks; Kruskal's algorithm over the union of
# two edge sets that share no tree is the merge of the two runs by key; the raster order of the voxels of a crop is that of their
# absolute indices (both lexicographic in z, y, x), so the tie-break (W, p, o) carries over ----
JOIN_INFO = ("n_trees_in", "n_trees_lost", "n_trees_out", "n_bridges", "n_inserted", "n_src", "n_src_dropped", "w_max", "thr_used")


def join_case(shape):
    l, h, w = shape
    rng = np.random.default_rng(12)
    near = rng.integers(105, 126, NEAR).astype(np.uint8)
    far = np.full(FAR, 110, np.uint8)  # uniform: ties on W everywhere
    blocks = _blocks(shape, near, far)
    z = l - 1
    # axis-parallel fragments of whole-voxel nodes (their sample points are whole voxels too), the near and the far ones in turn; the far
    # ones F1, F2, F3 lie 10 voxels apart in one row: W(F1, F2) = W(F2, F3)
    frags = [[(28, 6, 3), (34, 6, 3), (34, 10, 3)], [(w - 64, h - 15, z), (w - 58, h - 15, z)], [(44, 10, 6), (50, 10, 6)], [(w - 48, h - 15, z), (w - 42, h - 15, z)],
             [(66, 16, 10), (66, 16, 11), (68, 16, 11)], [(w - 32, h - 15, z), (w - 26, h - 15, z)], [(w - 3, h - 1, z), (w - 1, h - 1, z)]]
    xyz, parent = [], []
    for f in frags:
        parent += [-1] + list(range(len(xyz), len(xyz) + len(f) - 1))
        xyz += f
    xyz, parent = np.array(xyz, F), np.array(parent, np.int32)
    import distance_ref
    pts, _ = distance_ref.tree_sample(xyz, parent, 1, 1)
    assert np.array_equal(pts, np.rint(pts))
    for o, B in blocks:  # the fragments are bright
        for x, y, zz in pts.astype(int):
            if all(0 <= v - p < n for v, p, n in zip((zz, y, x), o, B.shape)):
                B[zz - o[0], y - o[1], x - o[2]] = 220
    return dict(shape=shape, thr=100, limit=160000, blocks=blocks, xyz=xyz, parent=parent)


def _join_sorted(bridges, chains, info):
    import geojoin_ref
    order = sorted(range(len(bridges)), key=lambda k: (int(bridges[k]["w"]), int(bridges[k]["p"]), int(bridges[k]["o"])))
    out = np.zeros(len(order), geojoin_ref.GEO_BRIDGE)
    vox = []
    for j, k in enumerate(order):
        out[j] = bridges[k]
        out[j]["path_off"] = len(vox)
        vox += [int(v) for v in chains[k]]
    return out, np.array(vox, np.int64), info


def join_want(case):
    import geojoin_ref
    shape = case["shape"]
    regions = crops(case["blocks"], shape)
    nodes, elsewhere = split_points(case["xyz"], regions, shape)
    assert len(elsewhere) == 0
    bridges, chains, infos = [], [], []
    for (V, o), (ni, np_) in zip(regions, nodes):
        local = {int(g): k for k, g in enumerate(ni)}
        par = np.array([local[int(p)] if p >= 0 else -1 for p in case["parent"][ni]], np.int32)  # (a tree lies in one block)
        b, vox, info, _ = geojoin_ref.solve(V, np_, par, ZD, case["limit"], case["thr"])
        for e in b:
            e = e.copy()
            chains.append(abs_index(vox[int(e["path_off"]):int(e["path_off"]) + int(e["path_len"])], o, V.shape, shape))
            e["a"], e["b"], e["p"] = ni[int(e["a"])], ni[int(e["b"])], abs_index(int(e["p"]), o, V.shape, shape)
            bridges.append(e)
        infos.append(info)
    info = {k: sum(i[k] for i in infos) for k in JOIN_INFO}
    info.update(w_max=max(i["w_max"] for i in infos), thr_used=case["thr"])
    return _join_sorted(bridges, chains, info) + (infos,)


def join_whole(case):
    import geojoin_ref
    b, vox, info, _ = geojoin_ref.solve(whole(case["blocks"], case["shape"]), case["xyz"], case["parent"], ZD, case["limit"], case["thr"])
    return b, vox, info


# ---- watershed: a key passes between neighbours inside the mask only, so no region leaves a block ----
def ws_case(shape):
    import ws_ref
    TZ, TY, TX = ws_ref.tile()
    rng = np.random.default_rng(13)
    blocks, points, labels = [], [], []
    for o, s in zip(origins(shape), (NEAR, FAR)):
        # the "rand3" content with relief = 255 - V: holes in the mask, three levels of relief, ties everywhere; markers with labels 1..5 ...
        V = np.where(rng.random(s) < 0.2, 0, rng.choice(np.array([255, 127, 1], np.uint8), s)).astype(np.uint8)
        n = max(2, V.size // 150)
        at = rng.choice(V.size, n, replace=False)
        zz, yy, xx = np.unravel_index(at, s)
        pts = [(x + o[2], y + o[1], z + o[0]) for x, y, z in zip(xx, yy, zz)]
        lab = list(rng.integers(1, 6, n))
        # ... and the "adjacent" pair: two markers on either side of a tile face in x
        xa = (o[2] // TX + 1) * TX - 1
        ya, za = o[1] + s[1] // 2, o[0] + s[0] // 2
        V[za - o[0], ya - o[1], xa - o[2]:xa - o[2] + 2] = (90, 140)
        pts += [(xa, ya, za), (xa + 1, ya, za)]
        lab += [8, 6]
        blocks.append(V)
        points += pts
        labels += lab
    points = np.array(points, F)
    points[::3] += F(0.25)  # (the centre voxel stays)
    return dict(shape=shape, thr=1, blocks=_blocks(shape, *blocks), points=points, labels=np.array(labels, np.int32))


WS_SUMS = ("n_mask", "n_marker_vox", "n_dropped", "n_reached", "n_unreached")


def _ws_info(infos, labels, case, conn):
    import ws_ref
    TZ, TY, TX = ws_ref.tile()
    l, h, w = case["shape"]
    info = {k: sum(i[k] for i in infos) for k in WS_SUMS}
    info.update(n_vox=l * h * w, n_regions=len(set().union(*labels)), tiles=-(-l // TZ) * -(-h // TY) * -(-w // TX), m_max=max(i["m_max"] for i in infos),
                d_max=max(i["d_max"] for i in infos), thr_used=case["thr"], connectivity=conn)
    return info


def ws_want(case, conn):
    """-> (info of the exact fields, [(origin, L, M)] per crop)"""
    import ws_ref
    regions = crops(case["blocks"], case["shape"])
    pts, elsewhere = split_points(case["points"], regions, case["shape"])
    assert len(elsewhere) == 0
    infos, labels, out = [], [], []
    for (V, o), (pi, pp) in zip(regions, pts):
        i, L, M, _ = ws_ref.run(V, case["thr"], conn, points=pp, labels=case["labels"][pi], solver=ws_ref.flood_sweeps)
        infos.append(i)
        labels.append(set(np.unique(L[L > 0]).tolist()))
        out.append((o, L, M))
    return _ws_info(infos, labels, case, conn), out


def ws_whole(case, conn):
    import ws_ref
    i, L, M, _ = ws_ref.run(whole(case["blocks"], case["shape"]), case["thr"], conn, points=case["points"], labels=case["labels"], solver=ws_ref.flood_sweeps)
    return {k: i[k] for k in ws_ref.EXACT}, L, M


# ---- coverage: a voxel's label depends on its absolute coordinates and the segments alone; the crops hold every voxel a segment can reach
# (its nodes' boxes, widened by the largest radius and 2), cut where the stack cuts them, and every block ----
REN_ZS = 2
REN_COUNTS = ("n_tree", "n_fg", "n_both", "sum_fg", "sum_both")


def render_case(shape):
    import render_ref
    l, h, w = shape
    rng = np.random.default_rng(14)
    near, far = (np.where(rng.random(s) < 0.6, rng.integers(100, 256, s), rng.integers(0, 100, s)).astype(np.uint8) for s in (NEAR, FAR))
    # a tree per block, positions on a quarter-voxel grid; the far one ends beside the last voxel: its capsules are cut by all three far faces
    a = np.array([(30, 8, 3), (36.5, 9.25, 4), (44, 12, 6.5), (52.25, 10, 8), (60, 15.5, 10), (40, 5, 9.75)], F)
    b = np.array([(w - 60, h - 20, l - 2), (w - 48.5, h - 14.25, l - 1), (w - 30, h - 9, l - 1.5), (w - 12.25, h - 5, l - 1), (w - 2, h - 1.5, l - 1), (w - 40, h - 26, l - 3)], F)
    pa, pb = [-1, 0, 1, 2, 3, 1], [-1, 0, 1, 2, 3, 1]
    xyz = np.concatenate([a, b])
    parent = np.array(pa + [p + len(a) if p >= 0 else -1 for p in pb], np.int32)
    radius = np.concatenate([render_ref.radius_mix(rng, len(a), "mix"), render_ref.radius_mix(rng, len(b), "mix")])
    radius[len(a) + 4] = 12  # the thick node of the far tree is the one in the corner
    assert np.array_equal(xyz * 4, np.rint(xyz * 4))
    return dict(shape=shape, thr=100, blocks=_blocks(shape, near, far), xyz=xyz, radius=radius, parent=parent, trees=[np.arange(len(a)), len(a) + np.arange(len(b))])


def render_regions(case):
    """a crop per tree: the box of its nodes and of its block, widened by the largest radius + 2 (in z: over the z scale), cut at the stack's faces"""
    shape = case["shape"]
    out = []
    for nodes, (o, B) in zip(case["trees"], case["blocks"]):
        p = case["xyz"][nodes].astype(np.float64)
        r = float(case["radius"][nodes].max()) + 2
        lo = [min(np.floor(p[:, 2].min() - r / REN_ZS), o[0]), min(np.floor(p[:, 1].min() - r), o[1]), min(np.floor(p[:, 0].min() - r), o[2])]
        hi = [max(np.ceil(p[:, 2].max() + r / REN_ZS) + 1, o[0] + B.shape[0]), max(np.ceil(p[:, 1].max() + r) + 1, o[1] + B.shape[1]),
              max(np.ceil(p[:, 0].max() + r) + 1, o[2] + B.shape[2])]
        out.append(stack_crop(case["blocks"], shape, lo, hi))
    (A, oa), (B, ob) = out
    assert oa[0] + A.shape[0] <= ob[0], "the crops share no voxel"
    return out


def _render_result(parts, case):
    import render_ref
    n = len(case["xyz"])
    seg = [np.zeros(n, np.int64) for _ in range(3)]
    cov = dict.fromkeys(REN_COUNTS, 0)
    for V, o in parts:
        L = render_ref.render(case["xyz"], case["radius"], case["parent"], V.shape, REN_ZS, origin=o)
        c, sv, sf, ss, _ = render_ref.coverage(V, L, n, case["thr"])
        for k in REN_COUNTS:
            cov[k] += c[k]
        for acc, v in zip(seg, (sv, sf, ss)):
            acc += v
    cov.update(n_vox=int(np.prod(case["shape"], dtype=np.int64)), thr_used=case["thr"])
    return cov, seg[0], seg[1], seg[2]


def render_want(case):
    return _render_result(render_regions(case), case)


def render_whole(case):
    return _render_result([(whole(case["blocks"], case["shape"]), (0, 0, 0))], case)


# ---- radius: a shell voxel outside the volume is not counted, one inside counts by its value; a crop that reaches rmax beyond every
# centre, or to the stack's face where that comes first, holds every voxel the measurement reads, and its far faces are the stack's ----
RAD_RMAX = 12


def radius_case(shape):
    import thin_ref
    l, h, w = shape
    near = np.where(thin_ref.ball(NEAR, (5, 7, 8), 4) | thin_ref.ball(NEAR, (4, 6, 33), 3) | (np.abs(np.arange(NEAR[1]) - 7) <= 2)[None, :, None] & (np.arange(NEAR[0]) == 5)[:, None, None],
                    200, 0)
    far = np.where(thin_ref.ball(FAR, (0, 12, 30), 7) | thin_ref.ball(FAR, (0, 27, 66), 5) | (np.abs(np.arange(FAR[1]) - 20) <= 1)[None, :, None], 180, 40)
    rng = np.random.default_rng(15)
    near, far = near.astype(np.uint8), far.astype(np.uint8)
    near[near > 0] -= rng.integers(0, 60, int((near > 0).sum())).astype(np.uint8)
    # tube and ball centres, off-centre positions, the far faces and beyond them, and one position that is not finite
    xyz = [(26 + 8, 4 + 7, 2 + 5), (26 + 33, 4 + 6, 2 + 4), (26 + 20.3, 4 + 7.4, 2 + 5.2), (26.5, 4.5, 2), (w - 70 + 30, h - 30 + 12, l - 1), (w - 70 + 66, h - 30 + 27, l - 1),
           (w - 1, h - 1, l - 1), (w + 5, h - 10, l + 3), (w - 20.25, h - 1, l - 0.75), (np.nan, 5, 5), (w - 45, h - 10, l - 1)]
    return dict(shape=shape, thr=100, blocks=_blocks(shape, near, far), xyz=np.array(xyz, F))


def radius_want(case, rel_pct):
    """-> k int32[n]"""
    shape = case["shape"]
    fin, c = radius_ref.centres(case["xyz"], shape)
    regions = []
    for o, B in case["blocks"]:  # the centres that lie within rmax of the block
        near = fin & ((c[:, ::-1] >= np.array(o) - RAD_RMAX) & (c[:, ::-1] < np.array(o) + np.array(B.shape) + RAD_RMAX)).all(1)
        lo, hi = c[near][:, ::-1].min(0) - RAD_RMAX, c[near][:, ::-1].max(0) + RAD_RMAX + 1
        regions.append(stack_crop(case["blocks"], shape, np.minimum(lo, o), np.maximum(hi, np.array(o) + np.array(B.shape))))
    parts, elsewhere = split_points(case["xyz"], regions, shape)
    assert not fin[elsewhere].any()
    k = np.full(len(case["xyz"]), -1, np.int32)
    for (V, o), (pi, pp) in zip(regions, parts):
        assert all(a == 0 or a <= m - RAD_RMAX for a, m in zip(o, c[pi][:, ::-1].min(0))) and all(
            a + n == e or a + n > m + RAD_RMAX for a, n, e, m in zip(o, V.shape, shape, c[pi][:, ::-1].max(0)))
        k[pi] = radius_ref.measure(V, ZD, pp, case["thr"], rel_pct, RAD_RMAX)[0]
    return k


def radius_whole(case, rel_pct):
    return radius_ref.measure(whole(case["blocks"], case["shape"]), ZD, case["xyz"], case["thr"], rel_pct, RAD_RMAX)[0]
