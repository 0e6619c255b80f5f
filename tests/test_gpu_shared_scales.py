"""GPU: option share_scales (a scale whose template grid nests in another's is not sampled; its ordered sums are formed from the
host's stash, tables.cpp find_scale_pairs) gives bit for bit what sampling every scale gives -- per-chain corr through the particle
states, node graphs, the sharded form, ragged last chain groups, 2-D and a chain of nested scales."""
import threading
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib, multigpu

pytestmark = pytest.mark.gpu


def _ctx(p, img, share, **opts):
    c = pnr_amd.Context(p, 0)
    c.set_volume(img)
    c.set_option("share_scales", share)
    c.set_option("share_min", 0)  # share in launches of every size
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _graph_equal(a, b):
    return len(a[0]) == len(b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[0][k], b[0][k], equal_nan=True) for k in a[0].dtype.names)


def _dbg_equal(T, da, db, ni):
    # xfilt holds every particle's corr and sigma (the max over the scales of the per-chain corr), iteration by iteration; rows
    # past a trace's end are not written
    for j in range(len(T)):
        rows = min(int(T[j]) + 1, ni)
        for k in ("xfilt", "neff"):
            assert np.array_equal(da[k][j, :rows], db[k][j, :rows], equal_nan=True), (k, j)


def _seeds(p, img, n):
    c = pnr_amd.Context(p, 0)
    c.set_volume(img)
    c.frangi()
    s = c.score_filter_sort(c.extract_seeds())
    c.close()
    return s[:: max(1, len(s) // n)][:n]


# AT MOST np + 1 chains -- 51 (last group 64 wide), 41, 21 (32), 11 (16), 64 + 1 (a full group and a last one of one chain): exact
# duplicates among the particles share a chain, so what a step really has is whatever the resampling left.  The chain counts and
# stash strides themselves are pinned, as inputs, by tests/test_gpu_phased_likelihood.py.
@pytest.mark.parametrize("sigs,np_", [((2.0, 4.0, 6.0), 50), ((2.0, 4.0, 6.0), 40), ((2.0, 4.0), 20), ((4.0, 2.0), 10),
                                      ((2.0, 4.0, 6.0), 64), ((2.0, 3.0, 4.0), 30)])
def test_trace_batch_per_chain_corr(sigs, np_):
    img = synth.synth(72, 64, 40, seed=3)
    p = pnr_amd.make_params(sigmas=list(sigs), np_=np_, ni=14, zdist=2.0)
    seeds = _seeds(p, img, 12)
    out = []
    for share in (0, 1):
        c = _ctx(p, img, share)
        out.append(c.trace_batch(seeds, dbg_iters=p.ni))
        c.close()
    (Ta, sa, xa, da), (Tb, sb, xb, db) = out
    assert np.array_equal(Ta, Tb) and np.array_equal(sa, sb) and Ta.max() > 3
    for k in xa.dtype.names:
        assert np.array_equal(xa[k], xb[k], equal_nan=True), k
    _dbg_equal(Ta, da, db, p.ni)


@pytest.mark.parametrize("groups", [1, 2])
def test_node_graph_512(groups):
    img = synth.synth(512, 512, 48, seed=5)
    p = pnr_amd.make_params(sigmas=[2.0, 4.0, 6.0], np_=50, ni=40, zdist=2.0)
    seeds = _seeds(p, img, 120)
    res = []
    for share, smin in ((0, 0), (1, 0), (1, 16)):
        c = _ctx(p, img, share, groups=groups)
        c.set_option("share_min", smin)
        res.append(c.trace_replay(seeds)[:3])
        c.close()
    assert len(res[0][0]) > 100
    for r in res[1:]:
        assert r[2] == res[0][2] and _graph_equal(r[:2], res[0][:2])


def test_sharded_eight_logical_ranks():
    img = synth.synth(96, 80, 40, seed=11)
    p = pnr_amd.make_params(sigmas=[2.0, 4.0, 6.0], np_=48, ni=30, zdist=2.0, nodepervol=3, vol=5)
    seeds = _seeds(p, img, 40)
    c0 = _ctx(p, img, 0)
    n1, l1, nt1, _ = c0.trace_replay(seeds)
    world = 8
    X = multigpu.ThreadExchange(world)
    ctxs, out = [_ctx(p, img, 1) for _ in range(world)], [None] * world

    def run(r):
        try:
            out[r] = ctxs[r].trace_replay_sharded(seeds, r, world, X.callback(r))
        except Exception as e:  # noqa: BLE001
            out[r] = e
            X.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive()
    for r in range(world):
        assert not isinstance(out[r], Exception), out[r]
        assert out[r][2] == nt1 and _graph_equal((out[r][0], out[r][1]), (n1, l1)), f"rank {r}"


def test_two_d():
    vol = synth.synth(96, 80, 9, seed=4)
    img = np.ascontiguousarray(vol.max(0, keepdims=True))
    p = pnr_amd.make_params(sigmas=[2.0, 4.0, 6.0], np_=30, ni=12, zdist=2.0)
    seeds = _seeds(p, img, 10)
    out = []
    for share in (0, 1):
        c = _ctx(p, img, share)
        out.append(c.trace_batch(seeds, dbg_iters=p.ni))
        c.close()
    (Ta, _, xa, da), (Tb, _, xb, db) = out
    assert np.array_equal(Ta, Tb) and Ta.max() > 2
    for k in xa.dtype.names:
        assert np.array_equal(xa[k], xb[k], equal_nan=True), k
    _dbg_equal(Ta, da, db, p.ni)
