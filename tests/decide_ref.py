"""What tests/test_gpu_phased_decide.py and tests/test_phased_decide_host.py know about the decision half of the phased SMC step
(ph_update and the drawing branch of ph_predict, pnr_amd/csrc/smc_phased.hip) WITHOUT running it: the traces that put a launch into
a chosen regime, the expected state after ph_update and after the following step's ph_predict -- every number from the oracle
(orc_smc_draw / orc_smc_decide / orc_smc_pending), only the control flow around them restated here -- and the regimes a case
reaches, read from the oracle's outputs.  numpy and the oracle only; both modules see the same cases.

A trace is a dict: it, seed (6), cur (np, 6) and prior (np,) the particles of `it`, prev (np, 9) those of it - 1, res_prev / idx_prev
the resampling of it - 1, pending (8) the centroid of it - 1, cs (S, np) the GIVEN per-scale correlations of the particles, cen_cs
(S,) those of the pending centroid, stop_in / T_in / pause the flag words on entry, share: particles with the same correlations on
one chain (as the duplicate search maps them)."""
import numpy as np
import phased_ref as R

NI = 6
DIMS = (24, 20, 12)  # w, h, l: the image matters only for its dimensions and the density map
SIGS = {1: (2.0,), 3: (2.0, 4.0, 6.0), 4: (2.0, 4.0, 6.0, 8.0)}
ZNCCTH = 0.3
NODEPERVOL = 4
RES, STOP, T_, IT, DONE, NCH, PAUSE = 0, 1, 2, 3, 4, 13, 14  # pnr_amd.lib.PHL_*
KEEP = (RES, STOP, T_, IT, DONE, NCH, PAUSE)  # the flag words of the decision half (the others belong to the likelihood half)
RMAX = 2147483647
EDGE_DRAWS = (0, 1, 2147483583, 2147483584, 2147483647)  # (float)r / (float)RAND_MAX is exactly 1 from 2147483584 on
NP_SWEEP = [(n, S) for n in (1, 7, 8, 9, 37, 63, 64, 65, 255, 256, 257, 500) for S in (1, 3)] + [(50, 4)]
JUNK = np.float32(5.0)  # fills what must not be read: it would win every maximum
f32 = np.float32


def make_tracker(L, n_p, S, neff_ratio=0.8):
    import orc
    return orc.Tracker(L, SIGS[S], 2, n_p, NI, 3.0, ZNCCTH, neff_ratio=neff_ratio, zdist=2.0, nodespervol=NODEPERVOL)


def make_context(n_p, S, neff_ratio=0.8):
    import pnr_amd
    p = pnr_amd.make_params(sigmas=list(SIGS[S]), np_=n_p, ni=NI, znccth=ZNCCTH, zdist=2, nodepervol=NODEPERVOL, neff_ratio=neff_ratio)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver("phased")
    c.set_volume(np.zeros((DIMS[2], DIMS[1], DIMS[0]), np.uint8))
    return c


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(f32)


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# traces
# ---------------------------------------------------------------------------------------------------------------------------------
def random_cs(rng, S, n_p, ties=True):
    """correlations in [-1, 1] with exact ties between scales, NaN scales and (np > 2) one particle without any finite scale"""
    cs = rng.uniform(-1, 1, (S, n_p)).astype(f32)
    if ties:
        for k in range(0, n_p, 5):
            if S > 1:
                cs[(k // 5) % (S - 1) + 1, k] = cs[0, k] if k % 2 else cs[:, k].max()  # a later scale ties the first / the maximum
        for k in range(3, n_p, 7):
            cs[rng.randint(S), k] = np.nan
        if n_p > 2:
            cs[:, 2] = np.nan
    return cs


def base_trace(T, rng, it, carry=True, **over):
    """a trace in the middle of the volume at iteration `it` whose particles are the oracle's own draw"""
    n_p, S = T.np, len(T.sigs)
    w, h, l = DIMS
    centre = np.array([w / 2, h / 2, l / 2])
    seed = np.concatenate([centre + rng.uniform(-1, 1, 3), unit(rng.normal(size=3))]).astype(f32)
    sp = dict(it=it, seed=seed, stop_in=0, T_in=NI, pause=0, share=False)
    prev = np.zeros((n_p, 9), f32)
    if it == 0:
        sp.update(prev=prev, res_prev=0, idx_prev=np.zeros(n_p, np.int32), pending=np.zeros(8, f32))
        cur, prior, _, _ = T.smc_draw(0, seed)
    else:
        prev[:, :3] = centre + rng.uniform(-2, 2, (n_p, 3))
        prev[:, 3:6] = unit(rng.normal(size=(n_p, 3)))
        wts = rng.uniform(0.5, 1.5, n_p)
        prev[:, 6] = wts / wts.sum()
        prev[:, 7] = rng.uniform(-1, 1, n_p)
        prev[:, 8] = rng.choice(T.sigs, n_p)
        idx_prev = np.sort(rng.randint(0, n_p, n_p)).astype(np.int32)
        pending = np.concatenate([centre + rng.uniform(-1, 1, 3), unit(rng.normal(size=3)), [rng.choice(T.sigs), 0]]).astype(f32)
        sp.update(prev=prev, res_prev=0 if carry else 1, idx_prev=idx_prev, pending=pending)
        cur, prior, _, _ = T.smc_draw(it, seed, prev, sp["res_prev"], idx_prev)
    sp.update(cur=cur, prior=prior, cs=random_cs(rng, S, n_p), cen_cs=rng.uniform(0.4, 1, S).astype(f32))
    sp.update(over)
    return sp


def sweep_traces(T, rng):
    """iterations 0, 1 and 2, carry on and off, one trace with shared chains"""
    tr = [base_trace(T, rng, 0), base_trace(T, rng, 1, True), base_trace(T, rng, 1, False), base_trace(T, rng, 2, True),
          base_trace(T, rng, 2, False)]
    sh = base_trace(T, rng, 1, True, share=True)
    sh["cs"][:, 1::2] = sh["cs"][:, 0:2 * (T.np // 2):2]  # odd particles repeat their even neighbour: one chain for both
    return tr + [sh]


def weight_traces(T, rng, kind):
    """it = 0 (1 / np base) and it = 1 with the previous weights carried: the likelihoods and priors of `kind`"""
    n_p, S = T.np, len(T.sigs)
    out = []
    for it, carry in ((0, True), (1, True), (1, False)):
        sp = base_trace(T, rng, it, carry)
        cs = np.full((S, n_p), 0.25, f32)
        prior = np.full(n_p, 0.5, f32)
        if kind == "uniform":
            if it:
                sp["prev"][:, 6] = f32(1.0 / n_p)
        elif kind == "dominant":
            cs[:] = -1
            cs[:, n_p // 2] = 1
        elif kind == "halfzero":  # every other weight exactly 0: through a zero prior and through a likelihood of exp(-inf)
            cs = rng.uniform(0.2, 0.3, (S, n_p)).astype(f32)
            prior[1::4] = 0
            cs[:, 3::4] = np.nan
        elif kind == "span":  # 2^-120 .. 1: denormal products
            e = np.round(np.linspace(0, 120, n_p))
            prior = (2.0 ** -e).astype(f32)
            sp["prev"][:, 6] = (2.0 ** -np.round(e / 5)).astype(f32)  # carried: products down to 2^-144 x the likelihood
            cs = rng.uniform(0.2, 0.3, (S, n_p)).astype(f32)
        sp.update(cs=cs, prior=prior)
        out.append(sp)
    return out


def stop_traces(T, rng):
    """np = 2, weights 1/2 and 1/2, exactly representable coordinates: centroids onto, just inside and half a voxel off each of the six
    faces; each as two equal particles and as a pair one voxel to either side"""
    assert T.np == 2
    out, want = [], []
    for a in range(3):
        d = DIMS[a]
        # (value of the centroid, outside?, the two particles one voxel to either side of it instead of on it)
        vals = [(-0.5, True, 0), (-0.5, True, 1), (np.nextafter(f32(-0.5), f32(0)), False, 0), (0.0, False, 1), (-1.0, True, 1), (d - 1.0, False, 1),
                (d - 0.5, True, 0), (d - 0.5, True, 1), (np.nextafter(f32(d - 0.5), f32(0)), False, 0), (float(d), True, 1), (0.5, False, 1),
                (0.5, False, 0), (d - 1.5, False, 0), (d - 1.5, False, 1)]
        for i, (v, outside, spread) in enumerate(vals):
            sp = base_trace(T, rng, i % 3, True)
            sp["cs"][:] = 0.5
            sp["prior"][:] = 0.25
            sp["prev"][:, 6] = 0.5
            centre = np.array([DIMS[0] / 2, DIMS[1] / 2, DIMS[2] / 2], f32)
            sp["cur"][:, :3] = centre
            sp["cur"][0, a] = f32(v) - f32(spread)
            sp["cur"][1, a] = f32(v) + f32(spread)
            sp.update(face=(a, float(v), outside))
            out.append(sp)
    return out


def pending_traces(T, rng, n=1):
    """the pending centroid's test: best below, equal to and above znccth from the entry states FL_STOP 0, 3 and 1; it == ni"""
    out = []
    th = f32(ZNCCTH)
    S = len(T.sigs)
    for stop_in in (0, 3, 1):
        for best in (np.nextafter(th, f32(-1)), th, np.nextafter(th, f32(1))):
            it = 2 + len(out) % 2
            sp = base_trace(T, rng, it, True, stop_in=stop_in, T_in=NI if stop_in == 0 else it - 1 if stop_in == 1 else it)
            cen = np.full(S, -0.5, f32)
            cen[S - 1] = best
            if S > 1:
                cen[0] = np.nan
            sp.update(cen_cs=cen, pend=(stop_in, float(best)))
            out.append(sp)
    out.append(base_trace(T, rng, NI, True, cen_cs=np.full(S, 0.9, f32)))  # the tail at it == ni, centroid fine
    out.append(base_trace(T, rng, NI, True, cen_cs=np.full(S, 0.1, f32)))  # ... and failing
    out.append(base_trace(T, rng, 1, True, cen_cs=np.full(S, np.nan, f32)))  # no scale wins: best = -FLT_MAX, sig = the weighted sum
    return out


def mixed_traces(T, rng, n):
    """n traces for one launch: iterations of both parities, carry on and off, shared chains, some paused, some stopping"""
    out = []
    pen = pending_traces(T, rng)
    for j in range(n):
        m = j % 10
        if m == 3:
            sp = base_trace(T, rng, 1 + j % 3, True, pause=1)
        elif m == 6:
            sp = pen[(j // 10) % len(pen)]
        elif m == 8:  # leaves the volume
            sp = base_trace(T, rng, j % 3, True)
            sp["cur"][:, 0] = -3
        elif m == 9 and j % 20 == 9:
            sp = base_trace(T, rng, 2, False, pause=1, stop_in=3, T_in=2)
        else:
            sp = base_trace(T, rng, (j // 2) % 4, j % 2 == 0)
            if m == 5:
                sp["share"] = True
                sp["cs"][:, 1::2] = sp["cs"][:, 0:2 * (T.np // 2):2]
            if m == 7:
                sp["cs"] = rng.uniform(0.5, 0.6, sp["cs"].shape).astype(f32)
        out.append(sp)
    return out


def invert_table(cws, s):
    """a draw r with cws[s - 1] < cws[sz - 1] * ((float)r / RAND_MAX) <= cws[s] (the walk stops at s), or None"""
    tot = f32(cws[-1])
    lo = f32(cws[s - 1]) if s else f32(-1)
    hi = f32(cws[s])
    if not hi > lo:
        return None
    mid = (float(max(lo, 0)) + float(hi)) / 2
    r0 = int(round(mid / float(tot) * 2147483648.0))
    for dr in sorted(range(-300, 301), key=abs):
        r = min(max(r0 + dr * 64, 0), RMAX)
        u1 = f32(tot * (f32(r) / f32(2147483647)))
        if lo < u1 <= hi:
            return r
    return None


def tie_pairs(v):
    """(a, b, p): vectors p whose dot products with the directions a < b are the maximum and EQUAL in float32, evaluated in the
    order of getdirection (x, then y, then z)"""
    out = []
    for a in range(len(v)):
        for b in range(a + 1, len(v)):
            p = (v[a] + v[b]).astype(f32)
            dp = (v[:, 0] * p[0] + v[:, 1] * p[1]) + v[:, 2] * p[2]
            if dp[a] == dp[b] == dp.max() and (dp == dp.max()).sum() == 2:
                out.append((a, b, p))
    return out


def direction_parents(T, rng, sp, kind, d=0):
    """put the parents of the NEXT step (the particles of sp) onto chosen directions of the predictor's table"""
    v = T.table("v")
    n_p = T.np
    if kind == "aligned":
        sp["cur"][:, 3:6] = v[d]
    elif kind == "each":
        sp["cur"][:, 3:6] = v[np.arange(n_p) % T.ndir]
    elif kind == "edge":  # exactly between two directions (the first wins), a zero vector, a NaN direction
        ties = tie_pairs(v)
        for k in range(n_p):
            sp["cur"][k, 3:6] = ties[k % len(ties)][2]
        sp["cur"][0, 3:6] = 0
        if n_p > 1:
            sp["cur"][1, 3:6] = np.nan
        if n_p > 3:
            sp["cur"][3, 4] = np.nan
    return sp


# ---------------------------------------------------------------------------------------------------------------------------------
# expectations: the oracle's numbers inside the product's control flow
# ---------------------------------------------------------------------------------------------------------------------------------
def layout(sp, n_p):
    """the chains of a trace as the tap uploads them: nch, uidx (chain -> particle), cmap"""
    if not sp["share"]:
        return n_p + 1, np.arange(n_p + 1, dtype=np.int32), np.arange(n_p, dtype=np.int32)
    words = np.ascontiguousarray(sp["cs"].T).view(np.uint32)
    seen, uidx, cmap = {}, [], np.zeros(n_p, np.int32)
    for k in range(n_p):
        key = words[k].tobytes()
        if key not in seen:
            seen[key] = len(uidx)
            uidx.append(k)
        cmap[k] = seen[key]
    return len(uidx) + 1, np.array(uidx + [n_p], np.int32), cmap


def pack(specs, n_p, S):
    nt = len(specs)
    np_pad = (n_p + 1 + 63) // 64 * 64
    a = dict(flags=np.zeros((nt, 16), np.int32), seeds=np.zeros((nt, 6), f32), part=np.full((nt, 2, n_p, 9), 7.0, f32),
             prior=np.zeros((nt, n_p), f32), idxres=np.zeros((nt, n_p), np.int32), xcs=np.full((nt, 2, 8), 3.0, f32),
             corr=np.full((nt, S, np_pad), JUNK, f32), cmap=np.full((nt, np_pad), -1, np.int32))
    for j, sp in enumerate(specs):
        it = sp["it"]
        nch, uidx, cmap = layout(sp, n_p)
        fl = a["flags"][j]
        fl[5:13] = 77  # (the likelihood half's words: the decision half leaves them alone)
        fl[RES], fl[STOP], fl[T_], fl[IT], fl[NCH], fl[PAUSE] = sp["res_prev"], sp["stop_in"], sp["T_in"], it, nch, sp["pause"]
        a["seeds"][j] = sp["seed"]
        a["part"][j, it & 1, :, :6] = sp["cur"]
        a["part"][j, (it & 1) ^ 1] = sp["prev"]
        a["prior"][j] = sp["prior"]
        a["idxres"][j] = sp["idx_prev"]
        a["xcs"][j, (it & 1) ^ 1] = sp["pending"]
        a["corr"][j, :, :nch - 1] = sp["cs"][:, uidx[:-1]]
        a["corr"][j, :, nch - 1] = sp["cen_cs"]
        a["cmap"][j, :n_p] = cmap
    return a


def resample_regimes(d):
    """what a resampling met, from the oracle's csw, ui and idxres"""
    if not d["resampled"]:
        return set()
    csw, ui, idx = d["csw"], d["ui"], d["idxres"]
    got = set()
    if (ui == csw[idx]).any():
        got.add("tie")
    if (ui > csw[-1]).any():
        got.add("clamp")
    flat = [m for m in range(1, len(csw)) if csw[m] == csw[m - 1]]
    if any(idx.min() < m < idx.max() and m not in idx for m in flat):
        got.add("flat")
    if len(set(idx.tolist())) == 1 and len(idx) > 1:
        got.add("one")
    return got


def expect(T, sp, a, j, den=None):
    """the state of trace j after ph_update and after the next step's ph_predict, as arrays in the tap's layout (a = pack(...))"""
    n_p, S, it = T.np, len(T.sigs), sp["it"]
    e = {k: a[k][j].copy() for k in ("flags", "part", "prior", "idxres", "xcs")}
    e.update(neff=np.zeros(NI, f32), oxc=np.zeros((NI, 8), f32), oT=-1, ostop=-1, running=False, drawn=False, met=set(), decide=None, nodir=None)
    if sp["pause"]:
        return e
    fl = e["flags"]
    tail = it == NI or sp["stop_in"] != 0
    if it >= 1:
        best, sig, low = T.smc_pending(sp["cen_cs"], sp["pending"][6])
        e["oxc"][it - 1] = np.concatenate([sp["pending"][:6], [sig, best]]).astype(f32)
        e["met"].add(("pending", sp["stop_in"], "low" if low else "equal" if best == f32(ZNCCTH) else "high"))
        if fl[STOP] in (0, 3) and low:
            fl[STOP], fl[T_] = 2, it - 1
    if tail or fl[STOP] != 0:
        e["oT"], e["ostop"], fl[DONE] = int(fl[T_]), int(fl[STOP]), 1
        return e
    carry = it > 0 and not sp["res_prev"]
    d = T.smc_decide(it, sp["cur"], sp["prior"], sp["prev"][:, 6] if carry else None, sp["cs"], DIMS)
    e["decide"] = d
    e["part"][it & 1] = d["xf"]
    e["neff"][it] = d["neff"]
    e["xcs"][it & 1, :7] = d["xc7"]
    res = 0
    x1, y1, z1 = (int(v) for v in d["xyz1"])
    if d["border"]:
        fl[STOP], fl[T_] = 1, it
        e["met"].add("border")
    elif den is not None and den[z1, y1, x1] >= NODEPERVOL:
        fl[STOP], fl[T_] = 3, it + 1
        e["met"].add("density")
    elif d["resampled"]:
        res = 1
        e["idxres"] = d["idxres"].copy()
        e["met"] |= resample_regimes(d)
    e["met"].add(("res", res))
    fl[RES], fl[IT] = res, it + 1
    e["running"] = True
    # ---- the next step's ph_predict
    e["part_p"], e["prior_p"] = e["part"].copy(), e["prior"].copy()
    if it + 1 == NI or fl[STOP] != 0:
        e["nch_p"] = 1
        return e
    poses2, prior2, dirs, sidx = T.smc_draw(it + 1, sp["seed"], d["xf"], res, e["idxres"])
    e["part_p"][(it + 1) & 1, :, :6] = poses2
    e["prior_p"] = prior2
    e.update(drawn=True, nodir=dirs < 0, dirs=dirs, sidx=sidx)
    return e


def expect_predict(T, sp, a, j):
    """trace j after ph_predict ALONE at its own iteration (iteration 0: iter0New's draw from the seed)"""
    it = sp["it"]
    e = dict(part_p=a["part"][j].copy(), prior_p=a["prior"][j].copy(), flags=a["flags"][j].copy(), listed=not sp["pause"], drawn=False, nodir=None)
    if sp["pause"] or it == NI or sp["stop_in"] != 0:
        return e
    poses, prior, dirs, sidx = T.smc_draw(it, sp["seed"], sp["prev"], sp["res_prev"], sp["idx_prev"])
    e["part_p"][it & 1, :, :6] = poses
    e.update(prior_p=prior, drawn=True, nodir=dirs < 0, dirs=dirs, sidx=sidx)
    return e


def compare_predict(out, specs, exps, n_p, lp=0):
    assert out["cnt_p"][lp] == len(specs) and out["cnt_p"][lp ^ 1] == 0, out["cnt_p"]
    for j, (sp, e) in enumerate(zip(specs, exps)):
        tag, h = (j, sp["it"]), sp["it"] & 1
        fp = out["flags_p"][j]
        assert np.array_equal(fp[list(KEEP[:-2]) + [PAUSE]], e["flags"][list(KEEP[:-2]) + [PAUSE]]), (tag, fp, e["flags"])
        valid = np.ones(n_p, bool) if e["nodir"] is None else ~e["nodir"]
        ok = same(out["part_p"][j], e["part_p"])
        ok[h, ~valid, :6] = True
        assert ok.all(), (tag, "part_p", np.argwhere(~ok)[:6], out["part_p"][j][~ok][:6], e["part_p"][~ok][:6])
        assert (same(out["prior_p"][j], e["prior_p"]) | ~valid).all(), (tag, "prior_p")
        if not e["listed"]:
            assert np.array_equal(fp, e["flags"]) and (out["uidx"][j] == -1).all() and (out["cmap_p"][j] == -1).all(), tag
        elif e["drawn"]:
            nch, uidx, cmap = R.chain_numbering(out["part_p"][j, h, :, :6], R.REGULAR)
            assert fp[NCH] == nch and np.array_equal(out["uidx"][j, :nch], uidx) and np.array_equal(out["cmap_p"][j, :n_p], cmap), tag
        else:
            assert fp[NCH] == 1 and out["uidx"][j, 0] == n_p and (out["cmap_p"][j] == -1).all(), tag


def compare(out, specs, exps, a, n_p, lp=0):
    """every word the tap returns against the expectation; returns nothing, asserts"""
    nt = len(specs)
    running = [j for j in range(nt) if exps[j]["running"]]
    assert out["cnt_next"][0] == len(running), (out["cnt_next"], len(running))
    assert sorted(out["list_next"][:len(running)].tolist()) == running and (out["list_next"][len(running):] == -1).all(), out["list_next"]
    assert out["cnt_p"][lp] == 0 and out["cnt_p"][lp ^ 1] == len(running), out["cnt_p"]
    for j, (sp, e) in enumerate(zip(specs, exps)):
        tag = (j, sp["it"], sp.get("name"))
        for k, key in (("part_u", "part"), ("xcs_u", "xcs"), ("idxres_u", "idxres"), ("prior_u", "prior"), ("neff", "neff"), ("oxc", "oxc")):
            ok = same(out[k][j], e[key])
            assert ok.all(), (tag, k, np.argwhere(~ok)[:6], out[k][j][~ok][:6], e[key][~ok][:6])
        assert out["oT"][j] == e["oT"] and out["ostop"][j] == e["ostop"], (tag, out["oT"][j], out["ostop"][j], e["oT"], e["ostop"])
        assert np.array_equal(out["flags_u"][j], e["flags"]), (tag, out["flags_u"][j], e["flags"])
        # ---- after ph_predict
        fp = out["flags_p"][j]
        assert np.array_equal(fp[list(KEEP[:-2]) + [PAUSE]], e["flags"][list(KEEP[:-2]) + [PAUSE]]), (tag, fp, e["flags"])
        if not e["running"]:
            assert np.array_equal(fp, e["flags"]), (tag, fp)
            assert same(out["part_p"][j], e["part"]).all() and same(out["prior_p"][j], e["prior"]).all(), tag
            assert (out["uidx"][j] == -1).all() and (out["cmap_p"][j] == -1).all(), tag
            continue
        valid = np.ones(n_p, bool) if e["nodir"] is None else ~e["nodir"]
        ok = same(out["part_p"][j], e["part_p"])
        ok[(sp["it"] + 1) & 1, ~valid, :6] = True  # (a NaN parent direction: no reference value)
        assert ok.all(), (tag, "part_p", np.argwhere(~ok)[:6], out["part_p"][j][~ok][:6], e["part_p"][~ok][:6])
        ok = same(out["prior_p"][j], e["prior_p"]) | ~valid
        assert ok.all(), (tag, "prior_p", np.argwhere(~ok)[:6])
        if e["drawn"]:
            nch, uidx, cmap = R.chain_numbering(out["part_p"][j, (sp["it"] + 1) & 1, :, :6], R.REGULAR)
            assert np.array_equal(out["cmap_p"][j, :n_p], cmap) and (out["cmap_p"][j, n_p:] == -1).all(), tag
        else:
            nch, uidx = 1, np.array([n_p], np.int32)
            assert (out["cmap_p"][j] == -1).all(), tag
        assert fp[NCH] == nch and np.array_equal(out["uidx"][j, :nch], uidx) and (out["uidx"][j, nch:] == -1).all(), (tag, fp[NCH], nch)


def run_case(T, specs, draws=None, den=None, ctx=None, lp=0, predict_only=False):
    """expectations of a launch, and -- with a context -- the launch itself, compared; returns the expectations.  predict_only:
    ph_predict alone at the traces' own iterations"""
    n_p, S = T.np, len(T.sigs)
    if draws is not None:
        T.set_rng(draws)
    else:
        draws = T.rng()
    a = pack(specs, n_p, S)
    if predict_only:
        exps = [expect_predict(T, sp, a, j) for j, sp in enumerate(specs)]
        if ctx is not None:
            compare_predict(ctx.phased_decide(draws=draws, lp=lp, predict_only=True, **a), specs, exps, n_p, lp)
        return exps
    exps = [expect(T, sp, a, j, den) for j, sp in enumerate(specs)]  # (before the GPU result exists)
    if ctx is not None:
        out = ctx.phased_decide(draws=draws, den=den, lp=lp, **a)
        compare(out, specs, exps, a, n_p, lp)
    return exps


def met(exps):
    return set().union(*[e["met"] for e in exps])


def draws_for(rng, n_p, **fixed):
    d = rng.randint(0, 2 ** 31 - 1, n_p + 1).astype(np.uint32)
    for k, v in fixed.items():
        d[int(k[1:])] = v
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the case sets (what each reaches is asserted in tests/test_phased_decide_host.py)
# ---------------------------------------------------------------------------------------------------------------------------------
ITERI_NP = 256


def weight_family(oracle, n_p, gpu=False):
    """(kind, ratio) -> (tracker, traces, draws, expectations) over the four kinds of weights under three values of neff_ratio, so
    that N_eff lands on either side of neff_ratio * np for each kind; with gpu: run and compared on a context per ratio"""
    fam = {}
    for ratio in (0.001, 0.8, 2.0):
        T = make_tracker(oracle, n_p, 3, ratio)
        ctx = make_context(n_p, 3, ratio) if gpu else None
        try:
            for kind in ("uniform", "dominant", "halfzero", "span"):
                rng = np.random.RandomState(n_p + len(kind))
                specs = weight_traces(T, rng, kind)
                draws = draws_for(rng, n_p)
                fam[kind, ratio] = (T, specs, draws, run_case(T, specs, draws, ctx=ctx))
        finally:
            if ctx is not None:
                ctx.close()
    return fam


def resampling_cases(oracle):
    """(tracker, traces, draws) of the resampling launches; the draws of the resampling are draws[1] at iteration 0, draws[np] later"""
    cases = []
    n_p = 8
    T = make_tracker(oracle, n_p, 1, 2.0)  # neff_ratio 2: every step resamples, the uniform weights included
    for r in EDGE_DRAWS + (1 << 28, 1 << 30, 3 << 29):  # uniform np = 8: u1 = r / 2^34 exactly, ui = u1 + k / 8 against csw = k / 8
        rng = np.random.RandomState(r % 1000)
        specs = weight_traces(T, rng, "uniform") + weight_traces(T, rng, "halfzero") + weight_traces(T, rng, "dominant")
        cases.append((T, specs, draws_for(rng, n_p, d1=r, d8=r)))
    for n_p in (37, 255):  # csw[np - 1] < 1 by rounding, ui beyond it: the CPU looks for such weights
        T = make_tracker(oracle, n_p, 1, 2.0)
        found = None
        for sd in range(200):
            rng = np.random.RandomState(sd)
            specs = [base_trace(T, rng, 0), base_trace(T, rng, 1, True)]
            for sp in specs:
                sp["cs"] = rng.uniform(0.4, 0.6, sp["cs"].shape).astype(f32)
            draws = draws_for(rng, n_p, d1=RMAX, **{"d%d" % n_p: RMAX})
            if "clamp" in met(run_case(T, specs, draws)):
                found = (T, specs, draws)
                break
        assert found, n_p
        cases.append(found)
    return cases


def iter0_cases(oracle):
    """np whose last ui passes w0cws[sz - 1] with the largest draw (the CPU finds them: 7 and 255 among others), draws[0] 0 and max,
    seed directions with none, one, two and three NaN components"""
    cases = []
    nan = np.nan
    for n_p in (7, 255):
        T = make_tracker(oracle, n_p, 1)
        for r in (0, RMAX):
            rng = np.random.RandomState(n_p)
            specs = []
            for comps in ((), (3,), (3, 5), (3, 4, 5)):
                sp = base_trace(T, rng, 0)
                sp["seed"][list(comps)] = nan
                specs.append(sp)
            specs += [base_trace(T, rng, 0, pause=1), base_trace(T, rng, 1, True), base_trace(T, rng, 2, False), base_trace(T, rng, 0, stop_in=1, T_in=0)]
            cases.append((T, specs, draws_for(rng, n_p, d0=r)))
    return cases


def iterI_cases(oracle):
    """np = sz = 256: in launch d particle k's draw inverts direction d's table at offset k, so parents aligned with d draw every
    offset; the other traces put parents on each direction, between two, on a zero and on a NaN vector, read with and without idxres"""
    cases = []
    T = make_tracker(oracle, ITERI_NP, 1)
    wc = T.table("w_cws")
    for d in (0, 17, 49):
        rng = np.random.RandomState(d)
        draws = draws_for(rng, ITERI_NP)
        for k in range(T.sz):
            r = invert_table(wc[d], k)
            if r is not None:
                draws[k] = r
        draws[T.sz - 1] = RMAX  # ratio exactly 1: u1 == cws[sz - 1]
        specs = [direction_parents(T, rng, base_trace(T, rng, 1, True), "aligned", d),
                 direction_parents(T, rng, base_trace(T, rng, 2, False), "aligned", d),
                 direction_parents(T, rng, base_trace(T, rng, 1, True), "each"),
                 direction_parents(T, rng, base_trace(T, rng, 2, True), "edge"),
                 direction_parents(T, rng, base_trace(T, rng, 1, False), "each")]
        for sp in specs[:4]:  # even weights: no resampling, particle k is its own parent
            sp["cs"][:] = 0.5
            sp["prior"][:] = 0.5
            sp["prev"][:, 6] = f32(1.0 / ITERI_NP)
        specs[4]["cs"] = rng.uniform(0.5, 0.6, specs[4]["cs"].shape).astype(f32)  # resamples onto many parents
        cases.append((T, specs, draws))
    return cases


def stop_cases(oracle):
    T = make_tracker(oracle, 2, 3)
    rng = np.random.RandomState(3)
    faces = stop_traces(T, rng)
    den = np.zeros((DIMS[2], DIMS[1], DIMS[0]), np.uint8)
    dens = []
    for i, (val, pos) in enumerate(((NODEPERVOL - 1, (5, 6, 3)), (NODEPERVOL, (7, 6, 3)), (255, (9, 6, 3)))):
        sp = base_trace(T, rng, i % 3, True)
        sp["cs"][:] = 0.5
        sp["prior"][:] = 0.25
        sp["prev"][:, 6] = 0.5
        sp["cur"][:, :3] = np.array(pos, f32) + f32(0.25)
        den[pos[2], pos[1], pos[0]] = val
        sp["den"] = val
        dens.append(sp)
    return T, faces, dens, pending_traces(T, rng), den, draws_for(rng, 2)


def launch_cases(oracle, nt):
    T = make_tracker(oracle, 20, 3)
    rng = np.random.RandomState(nt)
    return T, mixed_traces(T, rng, nt), draws_for(rng, 20)


def nonfinite_cases(oracle):
    """wsum == 0 (every likelihood exp(-inf) = 0) and a NaN prior sum: every weight NaN, the centroid NaN"""
    T = make_tracker(oracle, 9, 3)
    rng = np.random.RandomState(1)
    specs = []
    for it in (0, 1, 2):
        sp = base_trace(T, rng, it, True)
        sp["cs"][:] = np.nan
        specs.append(sp)
        sp = base_trace(T, rng, it, it != 2)
        sp["prior"][it] = np.nan
        specs.append(sp)
    return T, specs, draws_for(rng, 9)
