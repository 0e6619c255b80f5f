"""GPU: the likelihood half of the phased SMC step (ph_predict's placement and duplicate search, ph_cube, ph_sample, ph_sums of
pnr_amd/csrc/smc_phased.hip) on GIVEN poses, regime by regime, through the test tap pnr_phased_likelihood -- the production
kernels and launchers; only the drawing of the particles is compiled out of ph_predict.

Every case asserts, per trace: uidx / cmap are the first-occurrence numbering of the distinct poses (numpy, on the six float words)
closed by the centroid, FL_NCH is that count, and corr[s][c] of every chain c equals the oracle's per-scale correlation of the
chain's pose BIT FOR BIT (NaN equal) -- the contract of DESIGN.md section 2, so there is no tolerance.  Which regime a case is in
(chain groups, stash strides, packed parts; which scales are fast; where the cube lands) is computed on the CPU from the inputs
(tests/phased_ref.py) and asserted BEFORE the GPU result is looked at; tests/test_phased_likelihood_host.py runs that half alone."""
import numpy as np
import pytest
import orc
import phased_ref as R
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stacks():
    return {name: R.make_stack(name) for name in R.STACKS}


def _setup(oracle, stacks, stack, sset, n_p, **opts):
    sigs, zdist = R.SCALE_SETS[sset]
    img = stacks[stack]
    is2d = img.shape[0] == 1
    p = pnr_amd.make_params(sigmas=list(sigs), np_=n_p, ni=10, zdist=zdist)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver("phased")
    c.set_volume(img)
    c.set_option("share_min", 0)  # guest scales read their hosts' stash in launches of every size
    for k, v in opts.items():
        c.set_option(k, v)
    T = orc.Tracker(oracle, sigs, 2, n_p, 10, 3.0, 0.3, zdist=zdist, is2d=is2d)
    models = [T.model(s)[0] for s in range(len(sigs))]
    dims = (img.shape[2], img.shape[1], img.shape[0])
    return c, T, img, models, dims, is2d


def _expect(traces, models, dims, is2d):
    """the CPU half: numbering and geometry of every trace"""
    return [(R.chain_numbering(t["poses"], t["mode"]), R.trace_geometry(t["poses"], t["centroid"], t["mode"], models, dims, is2d)) for t in traces]


def _check(out, ref_ok, expect, traces, dims, is2d, n_p):
    """the assertion of every case; returns the set of chain regimes and of fast-word kinds the launch met"""
    S = out["corr"].shape[1]
    ref, ok = ref_ok
    met_chain, met_fast = set(), set()
    for j, (t, ((nch, uidx, cmap), geo)) in enumerate(zip(traces, expect)):
        fl = out["flags"][j]
        assert fl[lib.PHL_NCH] == nch, (j, fl[lib.PHL_NCH], nch)
        assert np.array_equal(out["uidx"][j, :nch], uidx) and (out["uidx"][j, nch:] == -1).all(), j
        if cmap is None:
            assert (out["cmap"][j] == -1).all(), j
        else:
            assert np.array_equal(out["cmap"][j, :n_p], cmap) and (out["cmap"][j, n_p:] == -1).all(), j
        got = out["corr"][j, :, :nch]
        # (a chain whose pose is not finite has no reference value, a first step's closing chain is never read -- phased_ref.oracle_per_chain)
        same = (got.view(np.uint32) == ref[j].view(np.uint32)) | (np.isnan(got) & np.isnan(ref[j])) | ~ok[j][None, :]
        assert same.all(), (j, t.get("name"), nch, np.argwhere(~same)[:8], got[~same][:8], ref[j][~same][:8])
        assert (out["corr"][j, :, nch:] == 0).all(), (j, "a chain the trace does not have was written")
        fw = int(fl[lib.PHL_FAST])
        assert fw >> 16 == 0 and (fw & 0xff) >> S == 0 and (fw & 0xff) & ~(fw >> 8) == 0, (j, hex(fw))  # fast implies inside the volume
        for s in range(S):
            if geo["fast"][s] is not None:
                assert bool(fw >> s & 1) == geo["fast"][s], (j, t.get("name"), s, hex(fw), geo["fast"], geo["lo"][s], geo["hi"][s], fl[5:8])
            if geo["vol"][s] is not None:
                assert bool(fw >> (8 + s) & 1) == geo["vol"][s], (j, t.get("name"), s, hex(fw), geo["vol"])
            met_fast.add("fast" if fw >> s & 1 else "volume" if fw >> (8 + s) & 1 else "clamped")
        bad = R.cube_sound(fl, geo, dims, is2d, OX=lib.PHL_OX, FAST=lib.PHL_FAST)
        assert not bad, (j, t.get("name"), bad)
        assert 0 <= fl[lib.PHL_Y0] < fl[lib.PHL_Y1] <= R.CS and 0 <= fl[lib.PHL_Z0] < fl[lib.PHL_Z1] <= R.CS, (j, fl)
        met_chain.add(R.chain_regime(nch))
    return met_chain, met_fast


def _run(oracle, stacks, stack, sset, n_p, traces, **opts):
    c, T, img, models, dims, is2d = _setup(oracle, stacks, stack, sset, n_p, **opts)
    try:
        expect = _expect(traces, models, dims, is2d)  # (before the GPU result exists)
        ref = R.oracle_per_chain(T, img, traces)[:2]
        share_tab = c.table("scale_share")
        out = c.phased_likelihood(*R.pack(traces))
    finally:
        c.close()
    met = _check(out, ref, expect, traces, dims, is2d, n_p)
    return out, expect, met, share_tab


def _named(d):
    return [dict(t, name=k) for k, t in d.items()]


@pytest.mark.parametrize("n_p,stack,sset", R.COUNT_CASES)
def test_chain_counts(oracle, stacks, n_p, stack, sset):
    """every chain count of phased_ref.NCH_ALL that n_p particles can give (tail pass, one distinct pose, both sides of the stride
    steps 16 -> 32 -> 64, rem == 0 and rem == 1 behind one to three full groups), the duplicates first, last and interleaved, traces
    with one chain group beside traces with four in ONE launch"""
    traces, want = R.count_case(n_p, stack)  # (asserts what the inputs reach)
    out, expect, (met_chain, met_fast), share_tab = _run(oracle, stacks, stack, sset, n_p, traces)
    assert met_chain == want
    guests = sum(1 << s for s in range(out["info"]["S"]) if share_tab[s] >= 0)
    if sset in ("s246", "s2468"):
        assert guests != 0  # a nested scale: its sums read the host's stash rows (strides 16 / 32 / 64 of the last group included)
    assert out["info"]["share"] == (1 if guests else 0) and out["info"]["rounds"] == 1
    assert out["info"]["ng"] == (n_p + 1 + 63) // 64  # traces with fewer chain groups sit beside full ones
    if stack == "wide_thin_z" and sset == "s246":
        assert met_fast == {"fast", "volume", "clamped"}  # full chain groups went through all three sampling forms


CLUSTER_CASES = [(stack, sset) for stack in R.STACKS for sset in R.SCALE_SETS]


@pytest.mark.parametrize("stack,sset", CLUSTER_CASES)
def test_pose_clusters(oracle, stacks, stack, sset):
    """where the cube lands and which scales are fast: tight interior clusters, the six faces and two corners (clamped origin, the
    byte-load tail of the staging at the volume's last row), a spread wider than the cube, a NaN pose, a centroid far outside"""
    d = R.STACKS[stack]
    dims, is2d = (d["w"], d["h"], d["l"]), d["l"] == 1
    traces = _named(R.cluster_traces(stack, 200, np.random.RandomState(7), jitter=R.cluster_jitter(stack, sset)))
    out, expect, (met_chain, met_fast), _ = _run(oracle, stacks, stack, sset, 200, traces)
    for j, (t, (_, geo)) in enumerate(zip(traces, expect)):
        assert None not in geo["fast"], (t["name"], geo["fast"])  # the geometry alone decided every bit that was asserted
        fl = out["flags"][j]
        if "clamped" in t:
            a, o, _ = t["clamped"]
            assert fl[lib.PHL_OX + a] == o, (t["name"], fl[5:8])
        if t.get("last_row"):  # the staged rows end at the volume's last row of its last plane, 56 bytes wide: past the volume's end
            assert fl[lib.PHL_OY] + fl[lib.PHL_Y1] == dims[1] and fl[lib.PHL_OZ] + fl[lib.PHL_Z1] == dims[2] and fl[lib.PHL_OX] + 56 > dims[0], fl
        if t["name"] == "nan_pose":
            # two chains without a reference value; the other 28 distinct particles and the centroid have one
            assert (~np.isfinite(R.chain_poses(t["poses"], t["centroid"], t["mode"])).all(1)).sum() == 2 and fl[lib.PHL_NCH] == 31
            assert fl[lib.PHL_Y0] == 0 and fl[lib.PHL_Y1] == R.CS and fl[lib.PHL_Z0] == 0 and fl[lib.PHL_Z1] == R.CS, fl  # all rows
    assert "fast" in met_fast and "clamped" in met_fast
    if stack in ("wide_thin_z", "slice"):
        assert "volume" in met_fast  # the spread cluster: inside the volume, not inside the cube


FORMS = [dict(max_split=ms, cube_copy=cc, sums_deep=sd, share_scales=sh) for ms in (1, 2, 7, None) for cc in (0, 1) for sd in (0, 1) for sh in (0, 1)]


def test_launch_forms(oracle, stacks):
    """70 traces of 20 particles in one launch, every (chain count, mode) they can give among them, under every launch form: 1, 2, 7 and the default number of
    sampling work-groups per trace, the cube staged by every work-group or copied from ph_cube's, both forms of the ordered sums,
    guest scales sampled or read from their hosts' stash -- the same bits in all of them, and the oracle's"""
    n_p, stack, sset = 20, "wide_thin_z", "s246"
    d = R.STACKS[stack]
    centre = [(d["w"] - 1) / 2, (d["h"] - 1) / 2, (d["l"] - 1) / 2]
    traces = R.mixed_traces(70, n_p, centre, False, np.random.RandomState(5))
    assert {(t["nch"], t["mode"]) for t in traces} == {(n, m) for n in range(2, 22) for m in (R.REGULAR, R.FIRST)} | {(1, R.TAIL)}
    assert {t["mode"] for t in traces} == {R.FIRST, R.REGULAR, R.TAIL}
    assert {R.chain_regime(t["nch"])[1] for t in traces} == {16, 32}
    c, T, img, models, dims, is2d = _setup(oracle, stacks, stack, sset, n_p)
    try:
        expect = _expect(traces, models, dims, is2d)
        ref = R.oracle_per_chain(T, img, traces)[:2]
        default_split = c.get_option("max_split")
        args = R.pack(traces)
        first, seen = None, set()
        for f in FORMS:
            for k, v in f.items():
                c.set_option(k, default_split if v is None else v)
            out = c.phased_likelihood(*args)
            i = out["info"]
            assert i["cube_copy"] == f["cube_copy"] and i["deep"] == f["sums_deep"] and i["share"] == f["share_scales"] and i["rounds"] == 1, (f, i)
            assert i["nsplit"] == f["max_split"] if f["max_split"] else i["nsplit"] > 7, (f, i)
            seen.add((i["nsplit"], i["cube_copy"], i["deep"], i["share"]))
            if first is None:
                first = out
                _check(out, ref, expect, traces, dims, is2d, n_p)  # the oracle's, in one of them
            else:
                for k in ("corr", "uidx", "cmap", "flags"):
                    assert np.array_equal(out[k].view(np.uint32), first[k].view(np.uint32)), (f, k)
        assert len(seen) == len(FORMS)
    finally:
        c.close()


def test_arguments():
    img = np.zeros((8, 16, 16), np.uint8)
    p = pnr_amd.make_params(sigmas=[2.0], np_=4, ni=10)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver("phased")
    poses, cen = np.zeros((1, 4, 6), np.float32), np.zeros((1, 6), np.float32)
    try:
        with pytest.raises(pnr_amd.PnrError, match="no volume"):
            c.phased_likelihood(poses, cen, [lib.PHL_REGULAR])
        c.set_volume(img)
        with pytest.raises(pnr_amd.PnrError, match="number of traces"):
            c.phased_likelihood(poses[:0], cen[:0], [])
        for bad in (-1, 3):
            with pytest.raises(pnr_amd.PnrError, match="mode"):
                c.phased_likelihood(poses, cen, [bad])
        c.set_smc_driver("persistent")
        with pytest.raises(pnr_amd.PnrError, match="phased driver"):
            c.phased_likelihood(poses, cen, [lib.PHL_REGULAR])
        c.set_smc_driver("phased")
        out = c.phased_likelihood(poses, cen, [lib.PHL_REGULAR])  # four identical particles and the centroid with the same pose
        assert out["flags"][0, lib.PHL_NCH] == 2 and list(out["uidx"][0, :2]) == [0, 4] and list(out["cmap"][0, :4]) == [0, 0, 0, 0]
    finally:
        c.close()
