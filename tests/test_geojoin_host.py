"""CPU: the rule of pnr_geodesic_bridges restated in numpy (geojoin_ref.py) has the property the feature rests on -- the minimum spanning
forest of the meet graph of ONE geodesic pass weighs what Kruskal's algorithm over the true pairwise geodesic distances gives (Mehlhorn
1988) --, and pnr_join_expand (pure host, through ctypes) against the reference, followed by pnr_join_reroot."""
import ctypes as C
import functools
import os
import re
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import geojoin_ref as ref
import join_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZDS = (1.0, 2.0, 3.3)


def random_case(seed):
    """a stack of at most 8^3 voxels (every second one with impassable voxels under thr = 128, every fourth one with mostly such) and 2 to 5 trees of 1 to 3 nodes on distinct
    passable voxels"""
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(2, 9, 3))
    walls = seed % 2 == 0
    V = rng.integers(0, 256, shape).astype(np.uint8)
    thr = 0
    if walls:
        thr = 128
        V = np.where(rng.random(shape) < (0.7 if seed % 4 else 0.12), np.maximum(V, 128), np.minimum(V, 127)).astype(np.uint8)
    ok = np.argwhere(V >= thr)[:, ::-1]
    trees = int(rng.integers(2, 6))
    sizes = rng.integers(1, 4, trees)
    pick = ok[rng.permutation(len(ok))[:int(sizes.sum())]]
    xyz, parent = [], []
    for s in sizes:
        for j in range(int(s)):
            if len(xyz) == len(pick):
                break
            parent.append(len(xyz) - 1 if j else -1)
            xyz.append(pick[len(xyz)])
    return V, thr, np.array(xyz, np.float32), np.array(parent, np.int32), ZDS[seed % 3]


@functools.lru_cache(maxsize=None)
def unlimited(seed):
    V, thr, xyz, parent, zd = random_case(seed)
    return ref.solve(V, xyz, parent, zd, thr=thr, step=0)


@pytest.mark.parametrize("seed", range(30))
def test_the_meet_graph_forest_weighs_what_the_true_distances_give(seed):
    V, thr, xyz, parent, zd = random_case(seed)
    bridges, vox, info, K = unlimited(seed)
    w = sorted(int(v) for v in bridges["w"])
    assert w == ref.brute_force_weights(V, xyz, parent, zd, thr=thr, step=0), (seed, V.shape)
    assert info["n_trees_lost"] == 0 and info["n_trees_in"] == int((parent < 0).sum()) and info["n_bridges"] == len(w) == info["n_trees_in"] - info["n_trees_out"]
    if len(w) >= 2 and w[0] < w[-1]:  # with a limit: the median bridge keeps some and drops some
        limit = w[(len(w) - 1) // 2]
        cut = sorted(int(v) for v in ref.solve(V, xyz, parent, zd, limit=limit, thr=thr, step=0)[0]["w"])
        assert cut == ref.brute_force_weights(V, xyz, parent, zd, limit=limit, thr=thr, step=0) == [v for v in w if v <= limit] and 0 < len(cut) < len(w)
    # every chain starts and ends on a source voxel of its two nodes' trees and its cost is W
    tree = join_ref.input_trees(parent)
    for b in bridges:
        chain = vox[b["path_off"]:b["path_off"] + b["path_len"]]
        assert tree[b["a"]] != tree[b["b"]] and len(chain) >= 2 and 13 <= b["o"] <= 25 and int(b["p"]) in chain.tolist()


def test_the_random_cases_cover_walls_every_zdist_limits_and_unjoined_trees():
    seen, limits, unjoined = set(), 0, 0
    for seed in range(30):
        V, thr, xyz, parent, zd = random_case(seed)
        w = np.sort(unlimited(seed)[0]["w"])
        seen.add((thr > 0, zd))
        limits += len(w) >= 2 and w[0] < w[-1]
        unjoined += unlimited(seed)[2]["n_trees_out"] > 1
    assert len(seen) == 6 and limits >= 10 and unjoined >= 1, (seen, limits, unjoined)


def _expand(xyz, parent, bridges, vox, shape, cap=None):
    L = lib.load()
    l, h, w = shape
    n, nb = len(xyz), len(bridges)
    n2 = C.c_int64()
    args = (xyz.ctypes.data, parent.ctypes.data, n, bridges.ctypes.data if nb else None, nb, vox.ctypes.data if len(vox) else None, len(vox), w, h, l)
    rc = L.pnr_join_expand(*args, None, None, None, 0, C.byref(n2), None)
    if rc:
        return rc
    total = n2.value
    cap = total if cap is None else cap
    xyz2, parent2, of, join = np.full((cap, 3), -7, np.float32), np.full(cap, -7, np.int32), np.full(max(cap - n, 1), -7, np.int32), np.zeros(nb, join_ref.BRIDGE)
    rc = L.pnr_join_expand(*args, xyz2.ctypes.data, parent2.ctypes.data, of.ctypes.data, cap, C.byref(n2), join.ctypes.data)
    assert rc == 0 and n2.value == total
    return xyz2, parent2, of[:max(cap - n, 0)], join, total


def _cases():
    rng = np.random.default_rng(5)
    # k = 0: two one-node trees on adjacent voxels
    yield np.full((1, 1, 2), 200, np.uint8), np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.array([-1, -1], np.int32), 1.0
    # k > 0: three fragments in a random stack, one of them with a negative parent other than -1
    V = rng.integers(0, 256, (4, 9, 12)).astype(np.uint8)
    xyz = np.array([[0, 0, 0], [2, 1, 0], [11, 8, 3], [10, 6, 3], [5, 4, 1], [0, 8, 3]], np.float32)
    yield V, xyz, np.array([-1, 0, -5, 2, -1, -1], np.int32), 2.0
    yield np.full((2, 5, 17), 255, np.uint8), np.array([[0, 0, 0], [16, 4, 1], [8, 2, 0], [8, 3, 0]], np.float32), np.array([-1, -1, -1, -1], np.int32), 3.3


@pytest.mark.parametrize("case", range(3))
def test_expand_against_the_reference_then_reroot(case):
    V, xyz, parent, zd = list(_cases())[case]
    bridges, vox, info, _ = ref.solve(V, xyz, parent, zd)
    want = ref.expand(xyz, parent, bridges, vox, V.shape)
    xyz2, parent2, of, join, total = _expand(xyz, parent, bridges, vox, V.shape)
    assert total == len(xyz) + info["n_inserted"] and (info["n_inserted"] == 0) == (case == 0) and info["n_bridges"] == int((parent < 0).sum()) - 1
    assert np.array_equal(xyz2, want[0]) and np.array_equal(parent2, want[1]) and np.array_equal(of, want[2])
    assert join.tobytes() == want[3].tobytes()
    got = pnr_amd.join_expand(xyz, parent, bridges, {"vox": vox, "shape": V.shape})
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3].tobytes() == want[3].tobytes()
    # too small a capacity: the count alone
    small = _expand(xyz, parent, bridges, vox, V.shape, cap=max(total - 1, 0))
    assert small[4] == total and (small[0] == -7).all() and (small[1] == -7).all()
    # every new node sits on its voxel, hangs off the previous one, and the chain's ends are the voxels of a and b
    l, h, w = V.shape
    for k, b in enumerate(bridges):
        chain = vox[b["path_off"]:b["path_off"] + b["path_len"]]
        mine = len(xyz) + np.flatnonzero(of == k)
        assert len(mine) == len(chain) - 2
        for j, i in enumerate(mine):
            g = int(chain[j + 1])
            assert xyz2[i].tolist() == [g % w, g // w % h, g // (w * h)] and parent2[i] == (b["a"] if j == 0 else i - 1)
    # ... then the re-rooting: one component, every parent before its children
    po, order, comp = pnr_amd.join_reroot(parent2, join)
    rpo, rorder, rcomp, trees_out = join_ref.reroot(parent2, join)
    assert np.array_equal(po, rpo) and np.array_equal(order, rorder) and np.array_equal(comp, rcomp) and trees_out == 1 and (comp == 0).all()
    pos = np.empty(total, np.int64)
    pos[order] = np.arange(total)
    assert (po < 0).sum() == 1 and all(po[i] < 0 or pos[po[i]] < pos[i] for i in range(total))


def test_a_limit_leaves_one_component_per_joined_group():
    V = np.full((1, 3, 40), 255, np.uint8)
    xyz = np.array([[0, 1, 0], [3, 1, 0], [30, 1, 0], [34, 1, 0], [39, 1, 0]], np.float32)
    parent = np.full(5, -1, np.int32)
    full = ref.solve(V, xyz, parent, 1.0)[0]
    limit = int(np.sort(full["w"])[len(full) // 2])
    bridges, vox, info, _ = ref.solve(V, xyz, parent, 1.0, limit=limit)
    assert 0 < len(bridges) < len(full) and info["n_trees_out"] == 5 - len(bridges)
    xyz2, parent2, of, join = pnr_amd.join_expand(xyz, parent, bridges, {"vox": vox, "shape": V.shape})
    po, order, comp = pnr_amd.join_reroot(parent2, join)
    assert len(np.unique(comp)) == info["n_trees_out"] == int((po < 0).sum())
    pos = np.empty(len(po), np.int64)
    pos[order] = np.arange(len(po))
    assert all(po[i] < 0 or pos[po[i]] < pos[i] for i in range(len(po)))


def test_argument_errors():
    L = lib.load()
    V, xyz, parent, zd = list(_cases())[1]
    bridges, vox, _, _ = ref.solve(V, xyz, parent, zd)
    shape = V.shape
    assert isinstance(_expand(xyz, parent, bridges, vox, shape), tuple)

    def bad(**kw):
        b = bridges.copy()
        for k, v in kw.items():
            b[k][0] = v
        return _expand(xyz, parent, b, vox, shape)

    assert bad(a=-1) == -1 and bad(a=len(xyz)) == -1 and bad(b=len(xyz)) == -1 and bad(a=int(bridges["b"][0])) == -1
    assert bad(path_len=1) == -1 and bad(path_off=-1) == -1 and bad(path_off=len(vox)) == -1 and bad(path_len=len(vox) + 1) == -1
    v2 = vox.copy()
    v2[1] = V.size
    assert _expand(xyz, parent, bridges, v2, shape) == -1 and b"outside" in L.pnr_last_error()
    v2[1] = -1
    assert _expand(xyz, parent, bridges, v2, shape) == -1
    assert _expand(xyz, parent, bridges, vox, (0, 3, 3)) == -1 and _expand(xyz, parent, bridges, vox, (1, 1, 1 << 24)) == -1
    p2 = parent.copy()
    p2[1] = len(xyz)
    assert _expand(xyz, p2, bridges, vox, shape) == -1
    n2 = C.c_int64()
    assert L.pnr_join_expand(None, None, 0, None, 0, None, 0, 3, 3, 3, None, None, None, 0, C.byref(n2), None) == -1
    assert L.pnr_join_expand(xyz.ctypes.data, parent.ctypes.data, len(xyz), None, 0, None, 0, 3, 3, 3, None, None, None, 0, None, None) == -1  # no n_nodes
    assert L.pnr_join_expand(xyz.ctypes.data, parent.ctypes.data, len(xyz), None, len(xyz), None, 0, 3, 3, 3, None, None, None, 0, C.byref(n2), None) == -1  # nb >= n
    assert L.pnr_join_expand(xyz.ctypes.data, parent.ctypes.data, len(xyz), None, 0, None, 0, 3, 3, 3, None, None, None, 0, C.byref(n2), None) == 0 and n2.value == len(xyz)
    # pnr_geodesic_bridges checks its arguments before it needs a context's state
    nb, npath = C.c_int64(), C.c_int64()
    assert L.pnr_geodesic_bridges(None, xyz.ctypes.data, parent.ctypes.data, len(xyz), None, None, None, 0, C.byref(nb), None, 0, C.byref(npath)) == -1


def test_header_and_exports():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    for name in ("pnr_geodesic_bridges", "pnr_join_expand"):
        assert name in lib.PRODUCT_EXPORTS and re.search(r"^int %s\(" % name, hdr, re.M)
    assert C.sizeof(lib.GeoJoinOpts) == 32 and C.sizeof(lib.GeoJoinInfo) == 72 and lib.GEO_BRIDGE.itemsize == 40 == ref.GEO_BRIDGE.itemsize
    assert "geojoin_tiles_per_launch" in hdr and "geojoin_rounds" in hdr and '"geojoin"' in hdr
