"""CPU: the half of tests/test_gpu_phased_likelihood.py that needs no GPU -- the oracle's per-scale correlations reproduce orc_zncc,
and the inputs of the GPU cases reach the regimes they are there for (tests/phased_ref.py): chain counts and duplicate placements by
numpy on the pose words, fast / clamped / volume-only scales, clamped cube origins and the spread chain groups by float64 geometry."""
import numpy as np
import pytest
import orc
import phased_ref as R


@pytest.mark.parametrize("stack,sset", [("wide_thin_z", "s246"), ("slice", "s234"), ("thin", "s3_12")])
def test_per_scale_values_reproduce_orc_zncc(oracle, stack, sset):
    """300 poses, out-of-volume and degenerate-direction ones among them: orc_zncc's corr is the first maximum of the per-scale
    values and its sigma that scale's, bit for bit; the batch form is the single-pose form"""
    sigs, zdist = R.SCALE_SETS[sset]
    img = R.make_stack(stack)
    l, h, w = img.shape
    T = orc.Tracker(oracle, sigs, 2, 20, 10, 3.0, 0.3, zdist=zdist, is2d=l == 1)
    rng = np.random.RandomState(3)
    pd = np.zeros((300, 6), np.float32)
    pd[:, :3] = rng.uniform(-0.2, 1.2, (300, 3)) * [w, h, l]  # a third of them outside the volume
    v = rng.normal(size=(300, 3))
    pd[:, 3:] = v / np.linalg.norm(v, axis=1, keepdims=True)
    pd[:8, 3:] = [(0, 0, 1), (0, 0, -1), (0, 0, 0), (1e-5, 0, 1), (1, 0, 0), (0, -1, 0), (0, 1e-4, 1), (-0.0, -0.0, 1)]  # no u axis of their own / axis-aligned
    pd[8, :3], pd[9, :3], pd[10, :3] = (-40, 3, 2), (w + 400, -300, l + 1000), (1e6, -1e6, 3e5)
    pd[11] = 0
    corr, sig, per = T.zncc_scales(img, pd)
    c0, s0 = T.zncc(img, pd)
    assert np.array_equal(corr.view(np.uint32), c0.view(np.uint32)) and np.array_equal(sig.view(np.uint32), s0.view(np.uint32))
    assert per.shape == (300, len(sigs))
    finite = ~np.isnan(per).any(1)
    assert finite.all()
    best = np.full(300, -np.finfo(np.float32).max, np.float32)
    bsig = np.zeros(300, np.float32)
    for s in range(len(sigs)):  # the first maximum: a later scale wins only if strictly greater
        win = per[:, s] > best
        best[win], bsig[win] = per[win, s], np.float32(sigs[s])
    assert np.array_equal(best.view(np.uint32), corr.view(np.uint32)) and np.array_equal(bsig[finite], sig[finite])
    assert len(np.unique(per[finite].argmax(1))) == len(sigs) or len(sigs) == 1  # every scale wins somewhere
    assert np.abs(per[finite]).max() <= 1.0001 and np.abs(per[finite]).max() > 0.3


@pytest.mark.parametrize("n_p,stack", sorted({(n, s) for n, s, _ in R.COUNT_CASES}))
def test_chain_count_inputs(n_p, stack):
    R.count_case(n_p, stack)  # (asserts)


def test_arrange_and_numbering():
    rng = np.random.RandomState(1)
    d = rng.rand(5, 6).astype(np.float32)
    d[3] = d[1]
    d[3, 2] = -d[3, 2]
    zero = np.zeros((2, 6), np.float32)
    zero[1, 0] = -0.0  # another word than +0: another chain
    assert R.chain_numbering(zero, R.REGULAR)[0] == 3
    nan = np.full((3, 6), np.nan, np.float32)  # the same NaN words: one chain
    assert R.chain_numbering(nan, R.REGULAR)[0] == 2
    for placement in ("first", "last", "interleaved"):
        p = R.arrange(d, 12, placement, rng)
        nch, uidx, cmap = R.chain_numbering(p, R.REGULAR)
        assert nch == 6 and uidx[-1] == 12 and np.array_equal(p[uidx[cmap]], p) and (np.diff(uidx) > 0).all()
        assert all(not np.array_equal(p[uidx[a]], p[uidx[b]]) for a in range(5) for b in range(a))
    assert R.chain_numbering(p, R.TAIL)[0] == 1
    assert [R.chain_regime(n) for n in (1, 16, 17, 32, 33, 64, 65)] == [(1, 16, 64, 0), (16, 16, 4, 0), (17, 32, 3, 0), (32, 32, 2, 0), (33, 64, 1, 0), (0, 0, 1, 1), (1, 16, 64, 1)]


@pytest.mark.parametrize("stack", list(R.STACKS))
@pytest.mark.parametrize("sset", list(R.SCALE_SETS))
def test_cluster_geometry_decides_the_fast_bits(oracle, stack, sset):
    """every pose cluster of the GPU module leaves no scale between 'surely fast' and 'surely not' (0.01 voxel either side), and the
    clusters are where they claim to be: against their face, past the last row, wider than the cube with one chain group inside it"""
    d = R.STACKS[stack]
    dims, is2d = (d["w"], d["h"], d["l"]), d["l"] == 1
    sigs, zdist = R.SCALE_SETS[sset]
    T = orc.Tracker(oracle, sigs, 2, 200, 10, 3.0, 0.3, zdist=zdist, is2d=is2d)
    models = [T.model(s)[0] for s in range(len(sigs))]
    for vuw in models:  # full grids: the corners of the offset box bound every sample
        ax = [np.unique(vuw[:, a]) for a in range(3)]
        assert len(vuw) == len(ax[0]) * len(ax[1]) * len(ax[2])
    assert all(models[-1].max(0)[a] >= m.max(0)[a] for m in models for a in range(3))  # the largest scale bounds the box of all
    traces = R.cluster_traces(stack, 200, np.random.RandomState(7), jitter=R.cluster_jitter(stack, sset))
    kinds = set()
    for name, t in traces.items():
        g = R.trace_geometry(t["poses"], t["centroid"], t["mode"], models, dims, is2d)
        assert None not in g["fast"], (name, g["fast"], g["lo"], g["hi"])
        kinds |= {"fast" if f else "volume" if v else "clamped" if v is False else "?" for f, v in zip(g["fast"], g["vol"])}
        if "clamped" in t:  # the templates cross that face, and all of them end within 48 voxels of it: the origin is clamped
            a, o, side = t["clamped"]
            assert (g["lo"][:, a].min() < -1 and g["hi"][:, a].max() < 48) if side == "low" else (g["hi"][:, a].max() > dims[a] and g["lo"][:, a].min() > dims[a] - 48), (name, g["lo"], g["hi"])
            assert o == (0 if side == "low" else max(0, dims[a] - R.CS))
        if t.get("last_row"):
            assert all(g["hi"][:, a].max() > dims[a] - 1 for a in ((0, 1) if is2d else (0, 1, 2))), name
        if name.startswith("interior"):
            assert g["fast"][0] and g["finite"]
        if name == "nan_pose":
            assert not g["finite"] and not any(g["fast"]) and R.chain_numbering(t["poses"], t["mode"])[0] == 31
    assert {"fast", "clamped"} <= kinds and "?" not in kinds
    if "spread" in traces:
        groups = R.spread_groups(traces["spread"], models[0], dims, is2d)
        assert groups == ["out", "in", "out"], groups  # mixed item_fast: the middle chain group alone passes the item-wise test
        assert R.chain_regime(R.chain_numbering(traces["spread"]["poses"], R.REGULAR)[0]) == (1, 16, 64, 3)
    else:
        assert dims[0] <= 54  # (no room for a spread wider than the cube)
    if stack in ("wide_thin_z", "slice"):
        assert "volume" in kinds


def test_launch_form_inputs():
    traces = R.mixed_traces(70, 20, [47.5, 39.5, 19.5], False, np.random.RandomState(5))
    assert len(traces) == 70
    for t in traces:
        assert R.chain_numbering(t["poses"], t["mode"])[0] == t["nch"]
    assert {(t["nch"], t["mode"]) for t in traces} == {(n, m) for n in range(2, 22) for m in (R.REGULAR, R.FIRST)} | {(1, R.TAIL)}
    assert {t["mode"] for t in traces} == {R.FIRST, R.REGULAR, R.TAIL}
    assert {R.chain_regime(t["nch"])[1] for t in traces} == {16, 32}
