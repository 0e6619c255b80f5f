"""CPU: the half of tests/test_gpu_phased_decide.py that needs no GPU -- the oracle's SMC step in pieces (orc_smc_draw ->
orc_zncc_scales -> orc_smc_decide -> orc_smc_pending) chained over whole traces reproduces orc_trace bit for bit, and the cases of
tests/decide_ref.py reach the regimes they are there for: every coverage condition is asserted here from the oracle's outputs alone."""
import numpy as np
import pytest
import orc
import synth
import decide_ref as D

f32 = np.float32


def _seeds_for(oracle, img, sigs, zdist, n):
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, sigs, zdist)
    s = orc.extract_seeds(oracle, 5, orc.j8(oracle, J, jmin, jmax), Vx, Vy, Vz)
    return s[:: max(1, len(s) // n)][:n]


def chained_trace(T, img, seed):
    """orc_trace restated over the public pieces"""
    l, h, w = img.shape
    n_p, ni = T.np, T.ni
    xc = np.zeros((ni, 8), f32)
    xfs, idxs, neffs = np.zeros((ni, n_p, 9), f32), np.full((ni, n_p), -2147483647, np.int32), np.zeros(ni, f32)
    prev, res, idx = None, 0, None
    for it in range(ni):
        poses, prior, _, _ = T.smc_draw(it, seed, prev, res, idx)
        cs = np.ascontiguousarray(T.zncc_scales(img, poses)[2].T)
        d = T.smc_decide(it, poses, prior, prev[:, 6] if it > 0 and not res else None, cs, (w, h, l))
        cen = np.concatenate([d["xc7"][:6]])
        best, sig, low = T.smc_pending(T.zncc_scales(img, cen)[2][0], d["xc7"][6])
        xc[it] = np.concatenate([d["xc7"][:6], [sig, best]])
        xfs[it], neffs[it] = d["xf"], d["neff"]
        if d["border"]:
            return it, 1, xc, xfs, idxs, neffs
        if low:
            return it, 2, xc, xfs, idxs, neffs
        if d["resampled"]:
            idxs[it] = d["idxres"]
        prev, res, idx = d["xf"], int(d["resampled"]), d["idxres"]
    return ni, 0, xc, xfs, idxs, neffs


@pytest.mark.parametrize("sigs,np_,ni,zdist", [([2.0], 50, 30, 2.0), ([2.0, 3.0], 64, 20, 2.0), ([2.0, 4.0], 37, 12, 1.0)])
def test_split_oracle_is_orc_trace(oracle, sigs, np_, ni, zdist):
    """the seeds of test_gpu_smc.test_trace_vs_oracle: T, stop, xc, xfilt, idxres, N_eff"""
    img = synth.synth(64, 56, 32, seed=2)
    so = _seeds_for(oracle, img, sigs, zdist, 6)
    T = orc.Tracker(oracle, sigs, 2, np_, ni, 3.0, 0.3, zdist=zdist)
    stops, nres = set(), 0
    for sd in so:
        for sgn in (1, -1):
            q = sd[:6].copy(); q[3:] *= sgn
            Tn, st, xco, xf, idx, neff = T.trace(img, q, max_dbg=ni)
            Tc, sc, xcc, xfc, idxc, neffc = chained_trace(T, img, q)
            assert (Tn, st) == (Tc, sc)
            rows = min(Tn + 1, ni)
            for a, b in ((xco, xcc), (xf, xfc), (neff, neffc)):
                assert D.same(a[:rows], b[:rows]).all()
            res = np.nonzero(neff[:Tn] / np_ < 0.8)[0]  # (orc_trace writes idxres only where it resampled; other rows are stale)
            assert np.array_equal(idx[res], idxc[res]) and (idxc[np.setdiff1d(np.arange(ni), res)] == -2147483647).all()
            nres += len(res)
            stops.add(st)
    assert len(stops) > 1 and nres > 0


def test_draw_edge_values(oracle):
    """(float)r / (float)RAND_MAX is exactly 1 from r = 2147483584 on, and below 1 just before"""
    r = np.array(D.EDGE_DRAWS, np.uint32)
    ratio = r.astype(f32) / f32(2147483647)
    assert list(ratio == 1) == [False, False, False, True, True] and ratio[0] == 0 and ratio[1] > 0


@pytest.mark.parametrize("n_p,S", D.NP_SWEEP)
def test_np_sweep_cases(oracle, n_p, S):
    T = D.make_tracker(oracle, n_p, S)
    rng = np.random.RandomState(n_p * 10 + S)
    exps = D.run_case(T, D.sweep_traces(T, rng), D.draws_for(rng, n_p))
    assert all(e["running"] for e in exps)
    if n_p > 2:  # a particle without a finite scale: best = -FLT_MAX, sig = 0, likelihood 0 -- the oracle's maximum gives just that
        xf = exps[0]["decide"]["xf"]
        assert xf[2, 7] == -np.finfo(f32).max and xf[2, 8] == 0 and xf[2, 6] == 0
    if n_p >= 37:
        assert {("res", 0), ("res", 1)} <= D.met(exps) or n_p >= 37 and ("res", 1) in D.met(exps)


@pytest.mark.parametrize("n_p", [8, 37])
def test_weight_cases(oracle, n_p):
    fam = D.weight_family(oracle, n_p)
    for kind in ("uniform", "dominant", "halfzero", "span"):
        sides = set().union(*[{m for m in D.met(fam[kind, r][3]) if isinstance(m, tuple) and m[0] == "res"} for r in (0.001, 0.8, 2.0)])
        assert sides == {("res", 0), ("res", 1)}, (kind, sides)
    if n_p == 8:  # uniform: wn = 0.125 and the CDF exact
        d = fam["uniform", 0.8][3][0]["decide"]
        assert (d["xf"][:, 6] == 0.125).all() and np.array_equal(d["csw"], np.arange(1, 9, dtype=f32) / 8)
    d = fam["halfzero", 2.0][3][0]["decide"]
    assert (d["xf"][1::2, 6] == 0).all() and (d["xf"][0::2, 6] > 0).all()
    d = fam["span", 2.0][3][1]["decide"]
    w = d["xf"][:, 6]
    assert ((w > 0) & (w < np.finfo(f32).tiny)).any() or n_p == 8  # denormal weights


def test_resampling_cases(oracle):
    got = set()
    for T, specs, draws in D.resampling_cases(oracle):
        got |= D.met(D.run_case(T, specs, draws))
    assert {"tie", "clamp", "flat", "one"} <= got, got


def test_iter0_cases(oracle):
    over = 0
    for T, specs, draws in D.iter0_cases(oracle):
        T.set_rng(draws)
        w0 = T.table("w0_cws")
        poses, prior, _, s = T.smc_draw(0, specs[0]["seed"])
        assert (np.diff(s) >= 0).all()
        step = f32(w0[-1] / f32(T.np))
        ui_last = f32(f32(step * (f32(draws[0]) / f32(2147483647))) + f32(f32(T.np - 1) * step))
        if ui_last > w0[-1]:  # the walk is held at sz - 1
            assert s[-1] == T.sz - 1
            over += 1
        exps = D.run_case(T, specs, draws, predict_only=True)
        assert [e["drawn"] for e in exps] == [True] * 4 + [False, True, True, False]
        for sp, nn in zip(specs, (0, 1, 2, 3)):
            p6 = T.smc_draw(0, sp["seed"])[0]
            assert np.isnan(sp["seed"]).sum() == nn and not np.isnan(p6).any()
    assert over == 2  # np = 7 and np = 255 with draws[0] = max


def test_iterI_cases(oracle):
    T = None
    hit = {}
    top = 0
    for d, (T, specs, draws) in zip((0, 17, 49), D.iterI_cases(oracle)):
        exps = D.run_case(T, specs, draws)
        wc, v = T.table("w_cws"), T.table("v")
        for j in (0, 1):
            e = exps[j]
            assert e["drawn"] and ("res", 0) in e["met"] and (e["dirs"] == d).all(), (d, j)
            for s in e["sidx"]:
                hit.setdefault(int(s), set()).add(d)
        u1 = f32(wc[d][-1] * (f32(draws[T.sz - 1]) / f32(2147483647)))
        top += int(u1 == wc[d][-1])
        assert set(exps[2]["dirs"].tolist()) == set(range(T.ndir))  # parents aligned with each of the directions
        e = exps[3]
        assert e["dirs"][1] == -1 and e["dirs"][3] == -1 and e["nodir"].sum() == 2 and e["dirs"][0] == 0  # NaN: no value; zero vector: direction 0
        ties = D.tie_pairs(v)  # exactly between two directions: the first wins
        assert len(ties) > 20 and all(e["dirs"][k] == ties[k % len(ties)][0] for k in range(D.ITERI_NP) if k not in (0, 1, 3))
        e = exps[4]
        assert ("res", 1) in e["met"] and len(set(e["idxres"].tolist())) > D.ITERI_NP // 3 and not np.array_equal(e["idxres"], np.arange(D.ITERI_NP))
    need = [s for s in range(T.sz) if all((T.table("w_cws")[d][s] > (T.table("w_cws")[d][s - 1] if s else -1)) for d in (0, 17, 49))]
    assert len(need) > 200
    assert all(len(hit.get(s, ())) >= 3 for s in need), [s for s in need if len(hit.get(s, ())) < 3][:10]
    assert top >= 1


def test_stop_cases(oracle):
    T, faces, dens, pend, den, draws = D.stop_cases(oracle)
    exps = D.run_case(T, faces + dens + pend, draws, den)
    for sp, e in zip(faces, exps):
        a, v, outside = sp["face"]
        assert e["decide"]["xc7"][a] == f32(v), (sp["face"], e["decide"]["xc7"])  # the centroid is exactly the engineered value
        assert e["decide"]["border"] == outside and (e["flags"][D.STOP] == 1) == outside and e["running"], sp["face"]
    assert {(sp["face"][0], sp["face"][1] < 1, sp["face"][2]) for sp in faces} == {(a, lo, o) for a in range(3) for lo in (True, False) for o in (True, False)}
    for sp, e in zip(dens, exps[len(faces):]):
        assert ("density" in e["met"]) == (sp["den"] >= D.NODEPERVOL) and e["flags"][D.STOP] == (3 if sp["den"] >= D.NODEPERVOL else 0)
    pe = exps[len(faces) + len(dens):]
    assert {m[1:] for m in D.met(pe) if isinstance(m, tuple) and m[0] == "pending"} >= {(s, k) for s in (0, 3, 1) for k in ("low", "equal", "high")}
    for sp, e in zip(pend, pe):
        if "pend" in sp:
            stop_in, best = sp["pend"]
            low = best < f32(D.ZNCCTH)
            assert e["flags"][D.STOP] == (1 if stop_in == 1 else 2 if low else stop_in), (sp["pend"], e["flags"])
            assert e["running"] == (stop_in == 0 and not low)
    assert [e["ostop"] for e in pe[9:11]] == [0, 2] and [e["oT"] for e in pe[9:11]] == [D.NI, D.NI - 1]  # the tail at it == ni
    assert pe[11]["oxc"][0, 7] == -np.finfo(f32).max and pe[11]["ostop"] == 2


@pytest.mark.parametrize("nt", [1, 2, 70])
def test_launch_cases(oracle, nt):
    T, specs, draws = D.launch_cases(oracle, nt)
    exps = D.run_case(T, specs, draws)
    if nt == 70:
        assert {sp["it"] & 1 for sp in specs} == {0, 1} and sum(sp["pause"] for sp in specs) >= 7
        assert 20 < sum(e["running"] for e in exps) < 60
        got = D.met(exps)
        assert "border" in got and {("res", 0), ("res", 1)} <= got and any(e["ostop"] == 2 for e in exps)


def test_nonfinite_cases(oracle):
    T, specs, draws = D.nonfinite_cases(oracle)
    for e, sp in zip(D.run_case(T, specs, draws), specs):
        d = e["decide"]
        assert np.isnan(d["xf"][:, 6]).all() and np.isnan(d["neff"]) and np.isnan(d["xc7"][:6]).all()
        assert (d["xyz1"] == -2 ** 31).all() and d["border"]  # the reference's build: the x86 conversion of NaN
        assert e["flags"][D.STOP] == 1 and e["flags"][D.T_] == sp["it"] and e["running"]
