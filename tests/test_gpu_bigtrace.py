"""The tracing path above 2^31 voxels (tests/bigtrace.py): Frangi (Gaussian, Hessian chunks, J8, direction bytes), seed extraction, ZNCC
scores, the SMC tracer under both drivers, the replay's density map and the streaming scheduler on a sparse stack of 2048 x 2048 x 536
whose far block crosses voxel index 2^31 = plane 512 = the face between Hessian chunks 15 and 16 and holds the stack's last voxel --
and on its 160 x 96 x 72 sibling through the same code, so that a failure at the large shape alone points at index width.  Every
expected value is the oracle's: Frangi on the crops (test_bigvol_host.py proves that equal to Frangi on the stack), scores, traces and
replay on the whole host stack, which the oracle indexes in 64 bits."""
import numpy as np
import pytest
import bigtrace as bt
import orc

pytestmark = pytest.mark.gpu
SHAPES = {"small": bt.SMALL, "large": bt.SHAPE}
mat = lambda a: np.stack([a[k] for k in a.dtype.names], -1)


@pytest.fixture(scope="module", params=list(SHAPES))
def stack(request, oracle):
    """the device stack of one shape, a context that borrows it, and the oracle's reference (computed once, read-only)"""
    import torch
    shape = SHAPES[request.param]
    t, c = bt.open_stack(shape)
    S = dict(shape=shape, t=t, c=c, ref=bt.reference(oracle, shape))
    yield S
    c.close()
    S.clear()
    del t
    torch.cuda.empty_cache()


def _sorted_seeds(S):
    """frangi -> extract_seeds -> score_filter_sort on the stack's context, once per stack: (all seeds, sorted seeds)"""
    if "sorted" not in S:
        c = S["c"]
        assert c.frangi() == (S["ref"]["frangi"]["jmin"], S["ref"]["frangi"]["jmax"])
        S["seeds"] = c.extract_seeds()
        S["sorted"] = c.score_filter_sort(S["seeds"])
    return S["seeds"], S["sorted"]


def _selected(S):
    r = S["ref"]
    _, ss = _sorted_seeds(S)
    assert np.array_equal(mat(ss)[:, :6], r["sorted6"]), "the sorted seeds are the oracle's"
    sel = ss[r["sel"]]
    n = r["counts"]
    assert len(sel) == bt.NSEL + 1 and n["far_kept"] >= 3 and n["traces_above"] >= 2 and n["traces_crossing"] >= 1, n
    return sel


def test_frangi(stack):
    c, fw = stack["c"], stack["ref"]["frangi"]
    assert bt.check_placement(bt.blocks(stack["shape"]), stack["shape"]) > 0
    assert c.frangi() == (fw["jmin"], fw["jmax"]), "the extremes are the oracle's over the crops"
    bt.check_frangi(c, fw)
    assert int(stack["t"].count_nonzero()) == sum(int(np.count_nonzero(B)) for _, B in bt.blocks(stack["shape"])), "the borrowed stack is as it was"


@pytest.mark.parametrize("knob", ["frangi_prune", "hess_chunk"])
def test_frangi_forms(stack, knob):
    """without the J8 shortcut, and with the Hessian stage cut into chunks of one march (HT_Z planes): the same bytes"""
    c, fw = stack["c"], stack["ref"]["frangi"]
    value, default = {"frangi_prune": (0, 1), "hess_chunk": (bt.ht_z(), 0)}[knob]
    c.set_option(knob, value)
    try:
        assert c.frangi() == (fw["jmin"], fw["jmax"])
        bt.check_frangi(c, fw)
    finally:
        c.set_option(knob, default)
        stack.pop("sorted", None)


def test_seeds(stack, oracle):
    shape, r = stack["shape"], stack["ref"]
    sg, _ = _sorted_seeds(stack)
    got = mat(sg)[:, :6]
    inside = np.zeros(len(got), bool)
    for o, B in bt.blocks(shape):
        lo, hi = np.array(o[::-1]), np.array(o[::-1]) + np.array(B.shape[::-1])
        inside |= ((got[:, :3] >= lo) & (got[:, :3] < hi)).all(1)
    assert inside.all() and len(got) > 200, "no seed outside the two blocks"
    assert np.array_equal(got, r["seeds"]), "the seeds of every layer are the crops' seeds, translated"
    for z in bt.compared_layers(shape):
        want = bt.layer_want(oracle, r["frangi"], shape, z)
        assert len(want) > 5 and np.array_equal(got[got[:, 2] == z], want), z


def test_scores(stack):
    r = stack["ref"]
    sg, ss = _sorted_seeds(stack)
    assert np.array_equal(mat(sg)[:, :6], r["seeds"])
    assert len(ss) == len(r["corr6"]) and np.array_equal(ss["corr"], r["corr6"]), "scores"
    assert np.array_equal(mat(ss)[:, :6], r["sorted6"]), "order of the sorted seeds"
    cg, _ = stack["c"].zncc(r["seeds"])
    assert np.array_equal(cg, r["corr"]), "the scores of the seeds below znccth too"


@pytest.mark.parametrize("driver", ["phased", "persistent"])
def test_traces(stack, driver):
    c, r, ni = stack["c"], stack["ref"], bt.PARAMS["ni"]
    sel = _selected(stack)
    c.set_smc_driver(driver)
    try:
        Tg, stop, xc, _ = c.trace_batch(sel)
    finally:
        c.set_smc_driver("phased")
    for j, (Tn, st, xco) in enumerate(r["traces"]):
        rows = min(Tn + 1, ni)
        assert Tg[j] == Tn and stop[j] == st and np.array_equal(mat(xc[j])[:rows], xco[:rows], equal_nan=True), (driver, j, Tg[j], Tn, stop[j], st)


def test_replay_and_streaming(stack, oracle):
    c, r, shape, p = stack["c"], stack["ref"], stack["shape"], bt.PARAMS
    l, h, w = shape
    sel = _selected(stack)
    Tg, stop, xc, _ = c.trace_batch(sel)
    n1, l1, nt1 = c.replay(sel, Tg, xc)
    To, xo = np.array([t[0] for t in r["traces"]], np.int32), np.stack([t[2] for t in r["traces"]])
    no, lo, nto = orc.replay(oracle, mat(sel).astype(np.float32), To, xo, p["ni"], shape, p["nodepervol"], p["vol"])
    same = lambda a, b: len(a) == len(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in b.dtype.names)
    assert same(n1, no) and np.array_equal(l1, lo) and nt1 == nto and len(n1) > 60, "replay vs the oracle's on the full shape"
    for tentative in (1, 0):
        c.set_option("tentative", tentative)
        try:
            n2, l2, nt2, _ = c.trace_replay(sel)
        finally:
            c.set_option("tentative", 1)
        assert nt2 == nt1 and np.array_equal(l2, l1) and same(n2, n1), ("streamed", tentative)
    far = n1[1:][n1["z"][1:] >= l - 40 - 1]
    idx = bt.centroid_index(np.stack([far["x"], far["y"], far["z"]], -1), len(far), shape)
    sign = int(bt.index_of(0, 0, l - bt.TAIL, shape))
    assert idx.dtype == np.int64 and (sign == 2**31) == (shape == bt.SHAPE)
    assert len(far) > 40 and (idx > sign).sum() > 0.5 * len(far), "more than half of the far traces' nodes lie above 2^31"
