"""reconstruct() with its neighbour stages on the GPU (pnr_reconstruct_ctx, Context.reconstruct): the mean-shift and the ball lists
of the sphere grouping run in recon.hip, and the output equals the host form's (lib.reconstruct, pnr_reconstruct) byte for byte --
and the oracle's O(n^2) scan where the graph is small enough for it."""
import numpy as np
import pytest
import orc
import synth
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4), np_=32, ni=40, zdist=2), 0)
    yield c
    c.close()


def _same(a, b):
    (an, ap), (bn, bp) = a, b
    assert len(an) == len(bn) and np.array_equal(ap, bp)
    for k in an.dtype.names:
        assert np.array_equal(an[k], bn[k], equal_nan=True), k


def _both(ctx, nodes, links, **kw):
    nodes = np.ascontiguousarray(nodes, lib.NODE_DT)
    dev = ctx.reconstruct(nodes, links, **kw)
    host = lib.reconstruct(nodes, links, **kw)
    _same(dev, host)
    return dev


def _same_stages(ctx, nodes, links, **kw):
    nodes = np.ascontiguousarray(nodes, lib.NODE_DT)
    for stage in (2, 3):
        dn, dl = ctx.reconstruct_stage(nodes, links, stage, **kw)
        hn, hl = lib.reconstruct_stage(nodes, links, stage, **kw)
        assert len(dn) == len(hn) and np.array_equal(dl, hl), stage
        for k in dn.dtype.names:
            assert np.array_equal(dn[k], hn[k], equal_nan=True), (stage, k)


def _dense_graph(oracle):
    """the random-walk graph of test_host.test_reconstruct_dense_graph_matches_oracle: crossing traces, six corr values"""
    rs = np.random.RandomState(5)
    shape = (40, 64, 72)
    l, h, w = shape
    ni, nseed = 50, 45
    s = np.zeros((nseed, 8), np.float32)
    s[:, 0] = rs.uniform(20, w - 20, nseed); s[:, 1] = rs.uniform(20, h - 20, nseed); s[:, 2] = rs.uniform(12, l - 12, nseed)
    s[:, 3:6] = rs.randn(nseed, 3); s[:, 6] = 0.9; s[:, 7] = 2.0
    T = rs.randint(30, ni + 1, 2 * nseed).astype(np.int32)
    xc = np.zeros((2 * nseed, ni, 8), np.float32)
    for t in range(2 * nseed):
        d = rs.randn(3); d /= np.linalg.norm(d)
        pos = s[t // 2, :3] + np.cumsum(1.3 * d + 0.4 * rs.randn(ni, 3), 0)
        pos[:, 0] = np.clip(pos[:, 0], 0, w - 1.01); pos[:, 1] = np.clip(pos[:, 1], 0, h - 1.01); pos[:, 2] = np.clip(pos[:, 2], 0, l - 1.01)
        xc[t, :, 0:3] = pos
        xc[t, :, 3:6] = d
        xc[t, :, 6] = rs.choice([2.0, 4.0, 6.0], ni)
        xc[t, :, 7] = np.round(rs.uniform(0.4, 0.9, ni), 1)
    nodes, links, _ = orc.replay(oracle, s, T, xc, ni, shape, 4, 5)
    return nodes, links


def test_dense_graph_matches_host_and_oracle(ctx, oracle):
    nodes, links = _dense_graph(oracle)
    assert len(nodes) > 2500
    want = orc.reconstruct(oracle, nodes, links, tree_size_min=4)
    got = _both(ctx, nodes, links, tree_size_min=4)
    assert len(got[0]) > 300
    _same(got, want)


def test_stage_taps_match_host(ctx, oracle):
    nodes, links = _dense_graph(oracle)
    _same_stages(ctx, nodes, links)
    _same_stages(ctx, nodes, links, sig2radius=2.5, group_radius=3.0)


@pytest.fixture(scope="module")
def synth_graph(ctx):
    img = synth.synth(96, 96, 64, seed=3)
    res = pnr_amd.advantra.run_pipeline(ctx, img, reconstruct=False)
    assert len(res["nodes"]) > 100
    return res["nodes"], res["links"]


def test_traced_graph_matches_host(ctx, synth_graph):
    nodes, links = synth_graph
    got = _both(ctx, nodes, links)
    assert len(got[0]) > 10
    one = _both(ctx, nodes, links, tree_size_min=-1)  # ENFORCE_SINGLE_TREE: the largest tree only
    assert 1 < len(one[0]) <= len(got[0])
    _same_stages(ctx, nodes, links)


def test_recon_kernels_are_timed(ctx, synth_graph):
    """the device stages' kernels are timed under the pnr_get_kernel_ms group "recon" """
    nodes, links = synth_graph
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_ms()
        _both(ctx, nodes, links)
        ms, launches = ctx.kernel_ms("recon")
    finally:
        ctx.set_profiling(False)
    assert launches >= 8 and ms > 0


def test_nondefault_parameters(ctx, synth_graph, oracle):
    nodes, links = synth_graph
    kw = dict(trace_rsmpl=0.7, sig2radius=2.2, refine_iter=9, epsilon2=1e-6, group_radius=3.1, tree_size_min=5)
    _both(ctx, nodes, links, **kw)
    dense_n, dense_l = _dense_graph(oracle)
    _both(ctx, dense_n, dense_l, **kw)
    _same_stages(ctx, dense_n, dense_l, **{k: v for k, v in kw.items() if k != "tree_size_min"})


def _traces_from_oracle(oracle, img, sigs, np_, ni, zdist, nseeds=12):
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, sigs, zdist)
    J8 = orc.j8(oracle, J, jmin, jmax)
    s = orc.extract_seeds(oracle, 5, J8, Vx, Vy, Vz)
    T = orc.Tracker(oracle, sigs, 2, np_, ni, 3.0, 0.3, zdist=zdist)
    corr, _ = T.zncc(img, s[:, :6])
    s[:, 7] = corr
    s = s[corr >= 0.3]
    s = s[np.argsort(-s[:, 7], kind="stable")][:nseeds]
    Ts, xcs = [], []
    for sd in s:
        for sgn in (1, -1):
            q = sd[:6].copy()
            q[3:] *= sgn
            Tn, stop, xc, *_ = T.trace(img, q)
            Ts.append(Tn)
            xcs.append(xc)
    return s, np.array(Ts, np.int32), np.stack(xcs)


def test_soma_nodes_match_host_and_oracle(ctx, oracle):
    img = synth.add_somas(synth.synth(64, 56, 32, seed=2), ((20, 28, 16, 6), (48, 20, 14, 5)))
    E8, th, smap, n4 = orc.soma_extract(oracle, img, 3)
    assert len(n4) >= 1
    s, T, xc = _traces_from_oracle(oracle, img, [2.0], 24, 30, 2.0, nseeds=40)
    l, h, w = img.shape
    vox = np.round(s[:, 2]).astype(np.int64) * w * h + np.round(s[:, 1]).astype(np.int64) * w + np.round(s[:, 0]).astype(np.int64)
    keep = smap.reshape(-1)[vox] == 0
    s, T, xc = s[keep], T.reshape(-1, 2)[keep].reshape(-1), xc.reshape(len(keep), 2, 30, 8)[keep].reshape(-1, 30, 8)
    nodes, links, _ = orc.replay(oracle, s, T, xc, 30, img.shape, 4, 1, smap=smap, soma4=n4)
    assert np.all(nodes["type"][1:1 + len(n4)] == 1)
    got = _both(ctx, nodes, links, tree_size_min=3)
    _same(got, orc.reconstruct(oracle, nodes, links, tree_size_min=3))
    assert (got[0]["type"] == 1).sum() >= 1


def _chain(n, rng, flat=False):
    nodes = np.zeros(n + 1, lib.NODE_DT)
    t = np.arange(n)
    nodes["x"][1:] = 5 + 0.8 * t % 60
    nodes["y"][1:] = 5 + (t // 75) * 1.5 + rng.random(n).astype(np.float32)
    nodes["z"][1:] = 7.0 if flat else 5 + rng.random(n).astype(np.float32)
    nodes["vx"][1:] = 1
    nodes["sig"][1:] = rng.choice([1.0, 2.0, 3.5], n).astype(np.float32)
    nodes["corr"][1:] = np.round(rng.uniform(0.3, 0.95, n), 1).astype(np.float32)  # many ties
    nodes["type"][1:] = 3
    links = np.array([(i, i + 1) for i in range(1, n) if i % 75], np.int32).reshape(-1, 2)
    return nodes, links


def test_edge_cases_match_host(ctx):
    rng = np.random.default_rng(11)
    # NaN corr and tied corr values
    nodes, links = _chain(400, rng)
    nodes["corr"][rng.choice(np.arange(1, 401), 60, replace=False)] = np.nan
    _both(ctx, nodes, links, tree_size_min=3)
    _same_stages(ctx, nodes, links)
    # only the dummy node; the dummy and isolated nodes
    _both(ctx, nodes[:1], np.zeros((0, 2), np.int32))
    _both(ctx, nodes[:40], np.zeros((0, 2), np.int32))
    _same_stages(ctx, nodes[:40], np.zeros((0, 2), np.int32))
    # self links, duplicate links and links in both directions
    extra = np.array([(5, 5), (9, 9), (10, 11), (11, 10), (10, 11), (3, 300), (300, 3)], np.int32)
    _both(ctx, nodes, np.concatenate([links, extra]), tree_size_min=2)
    # a flat graph (2-D mode: z constant)
    flat, fl = _chain(300, rng, flat=True)
    _both(ctx, flat, fl, tree_size_min=2)
    _same_stages(ctx, flat, fl)
    # a node with a NaN scale (an empty ball: the mean-shift divides 0 by 0) and one with a NaN position
    odd = nodes.copy()
    odd["sig"][17] = np.nan
    odd["x"][23] = np.nan
    _both(ctx, odd, links, tree_size_min=3)
    _same_stages(ctx, odd, links)


def test_balls_larger_than_the_lds_lists(ctx):
    """several thousand nodes in one mean-shift ball and one grouping ball: the bitmap kernels, same bits as the host"""
    rng = np.random.default_rng(7)
    nodes, links = _chain(600, rng)
    m = 3000
    blob = np.zeros(m, lib.NODE_DT)
    blob["x"] = 40 + rng.random(m).astype(np.float32)
    blob["y"] = 20 + rng.random(m).astype(np.float32)
    blob["z"] = 6 + rng.random(m).astype(np.float32)
    blob["sig"] = rng.choice([2.0, 3.0], m).astype(np.float32)
    blob["corr"] = rng.uniform(0.3, 0.95, m).astype(np.float32)
    blob["type"] = 3
    n0 = len(nodes)
    allnodes = np.concatenate([nodes, blob])
    bl = np.stack([np.arange(n0, n0 + m - 1), np.arange(n0 + 1, n0 + m)], 1).astype(np.int32)
    alllinks = np.concatenate([links, bl, np.array([(n0 - 1, n0)], np.int32)])
    _both(ctx, allnodes, alllinks, tree_size_min=2)
    _same_stages(ctx, allnodes, alllinks)


def test_resize_and_bitmap_passes_take_the_same_launches(ctx):
    """1100 nodes in one unit cube: every grouping ball holds the other 1099, so the lists need 1100 x 1099 > max(2^20, 16 n) entries
    and the resize pass runs, and both stages leave their large balls to the bitmap kernels.  Same bits as the host, and the launches
    the timer group "recon" counts are those of the passes, one by one."""
    rng = np.random.default_rng(13)
    nodes, links = _chain(200, rng)
    m = 1100
    blob = np.zeros(m, lib.NODE_DT)
    blob["x"] = 40 + rng.random(m).astype(np.float32)
    blob["y"] = 20 + rng.random(m).astype(np.float32)
    blob["z"] = 6 + rng.random(m).astype(np.float32)
    blob["sig"] = rng.choice([2.0, 3.0], m).astype(np.float32)
    blob["corr"] = rng.uniform(0.3, 0.95, m).astype(np.float32)
    blob["type"] = 3
    n0 = len(nodes)
    allnodes = np.concatenate([nodes, blob])
    bl = np.stack([np.arange(n0, n0 + m - 1), np.arange(n0 + 1, n0 + m)], 1).astype(np.int32)
    alllinks = np.concatenate([links, bl, np.array([(n0 - 1, n0)], np.int32)])
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_ms()
        _both(ctx, allnodes, alllinks, tree_size_min=2)
        _, launches = ctx.kernel_ms("recon")
    finally:
        ctx.set_profiling(False)
    print(f"recon launches of one reconstruct: {launches}")
    # pnr_recon_shift: toc("recon", 4) the grid's bin, scan and scatter with k_shift, toc("recon", 1) k_shift_big           = 5
    # pnr_recon_balls: toc("recon", 3) the grid; then per pass toc("recon", 1) k_balls and toc("recon", 1) k_balls_big,
    #                  and there are two passes, the first with too small a list                                           = 3 + 2 * 2
    assert launches == 12


def test_large_traced_stack_matches_host():
    """the full trace loop on a 384^3 synthetic stack: balls span many grid cells, as on the CLI's full stacks"""
    import torch
    w = h = l = 384
    vol = synth.synth_torch(w, h, l, seed=4)
    torch.cuda.synchronize()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6)), 0)
    try:
        c.set_volume_device(vol.data_ptr(), (l, h, w), keepalive=vol)
        res = pnr_amd.advantra.run_pipeline(c, vol, reconstruct=False)
        nodes, links = res["nodes"], res["links"]
        assert len(nodes) > 5000
        got = _both(c, nodes, links)
        assert len(got[0]) > 1000
        _same_stages(c, nodes, links)
    finally:
        c.close()


def test_argument_errors(ctx):
    rng = np.random.default_rng(3)
    nodes, links = _chain(50, rng)
    with pytest.raises(pnr_amd.PnrError, match="refine_iter"):
        ctx.reconstruct(nodes, links, refine_iter=1001)
    with pytest.raises(pnr_amd.PnrError, match="refine_iter"):
        ctx.reconstruct_stage(nodes, links, 2, refine_iter=1001)
    _both(ctx, nodes, links, refine_iter=1000)
    bad = np.concatenate([links, np.array([(3, 51)], np.int32)])
    for f in (ctx.reconstruct, lib.reconstruct):
        with pytest.raises(pnr_amd.PnrError, match="link index out of range"):
            f(nodes, bad)
