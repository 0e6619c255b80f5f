"""What tests/test_gpu_phased_likelihood.py and tests/test_phased_likelihood_host.py know about the likelihood half of the phased SMC
step (pnr_amd/csrc/smc_phased.hip) WITHOUT running it: the chain numbering, the chain-group regimes, a float64 restatement of where
the template samples of a pose lie, and the traces (poses, duplicates, clusters) that put a launch into a chosen regime.  numpy only;
everything is a pure function of its arguments, so both modules see the same cases.

Geometry.  A pose (x, y, z, v) has the local frame of Tracker::znccBBB (u in the x-y plane, w = u x v); the samples of scale s are
p + ov (-v) + ou u + ow w over a full grid of offsets (Tracker.model(s): nv x nu x nw), so on every axis the extremes lie at the eight
corners of the grid's offset box.  `extents` evaluates those corners in float64.  The kernels do it in float32 on poses of a few
hundred voxels at most: the two differ by less than 1e-3 voxel, far inside the 0.01 margin used below.

What decides FL_FAST bit s (ph_predict): every template of scale s, grown by 0.5 voxel, lies inside [0, dim - 1.001] on every axis
(the z axis is not tested on a single slice) and inside the cube: floor(lo - 0.5) >= origin and floor(hi + 0.5) + 1 <= origin + 53.
The cube's origin is the midpoint of the box of ALL scales' templates (each grown by 1.5 and rounded outwards by at most 1 below and
3 above, then cut to [0, dim - 1]) minus 27, held inside [0, max(0, dim - 54)].  Hence, with U the extent of all scales' samples cut
to [0, dim - 1] and mid its midpoint, the kernel's midpoint lies within 2.5 voxels of mid, and
  - bit s is certainly SET when scale s is at least 0.51 inside the volume and inside [mid - 24, mid + 24] (or the axis is thinner
    than the cube: origin 0, the cube holds the whole axis);
  - bit s is certainly CLEAR when a pose of the trace is not finite, or a sample of s lies more than 0.01 outside [0, dim - 1.001], or
    the samples of s span more than 54.01 voxels on an axis.
Anything between the two is `None`: a cluster that leaves a scale there is no test of the bit, and the host test refuses it."""
import numpy as np

CS = 54           # edge of the sampling cube (PH_CS)
MARGIN = 0.01     # voxels on either side of a threshold inside which the float64 geometry does not decide
FIRST, REGULAR, TAIL = 0, 1, 2  # pnr_amd.lib.PHL_*

# chain counts the issue names, with what each reaches
NCH_ALL = (1, 2, 16, 17, 32, 33, 63, 64, 65, 80, 97, 128, 129, 201)
STACKS = {"wide_thin_z": dict(w=96, h=80, l=40, zdist=1.0), "deep_z": dict(w=72, h=64, l=60, zdist=1.0),
          "thin": dict(w=40, h=36, l=20, zdist=1.0), "slice": dict(w=96, h=80, l=1, zdist=1.0)}
# (sigmas, the tracker's zdist)
SCALE_SETS = {"s2": ((2.0,), 2.0), "s246": ((2.0, 4.0, 6.0), 2.0), "s234": ((2.0, 3.0, 4.0), 2.0), "s3_12": ((3.0, 12.0), 2.0),
              "s2468": ((2.0, 4.0, 6.0, 8.0), 4.0)}


def cluster_jitter(stack, sset):
    """half-width of the position box of a pose cluster: 1 voxel, and with sigma 8 as much as puts that scale's templates clearly past
    the cube's 54 voxels (its 48-voxel slab would otherwise end between 'surely fast' and 'surely not')"""
    return 1.0 if sset != "s2468" else 3.2 if stack == "slice" else 2.5


def make_stack(name):
    import synth
    d = STACKS[name]
    if name == "slice":
        return np.ascontiguousarray(synth.synth(d["w"], d["h"], 9, seed=4).max(0, keepdims=True))
    return synth.synth(d["w"], d["h"], d["l"], zdist=d["zdist"])


# ---------------------------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_regime(nch):
    """(rem, stride of the last group's stash rows, parts of its packed sampling, full groups) as ph_sample / ph_sums derive them"""
    ngf, rem = divmod(int(nch), 64)
    stride = 0 if rem == 0 else 64 if rem > 32 else 32 if rem > 16 else 16
    return rem, stride, (64 // rem if rem else 1), ngf


def chain_numbering(poses, mode):
    """first-occurrence numbering of the distinct poses on their six float words, closed by the centroid (index np):
    nch, uidx [nch] chain -> particle, cmap [np] particle -> chain (None in a tail pass)"""
    n_p = len(poses)
    if mode == TAIL:
        return 1, np.array([n_p], np.int32), None
    words = np.ascontiguousarray(poses, np.float32).view(np.uint32).reshape(n_p, 6)
    seen, uidx, cmap = {}, [], np.zeros(n_p, np.int32)
    for k in range(n_p):
        key = words[k].tobytes()
        if key not in seen:
            seen[key] = len(uidx)
            uidx.append(k)
        cmap[k] = seen[key]
    return len(uidx) + 1, np.array(uidx + [n_p], np.int32), cmap


def chain_poses(poses, centroid, mode):
    """the pose of every chain in chain order [nch][6] (a first step's closing chain reads zeros)"""
    nch, uidx, _ = chain_numbering(poses, mode)
    cen = np.zeros(6, np.float32) if mode == FIRST else np.asarray(centroid, np.float32)
    return np.concatenate([np.asarray(poses, np.float32)[uidx[:-1]], cen[None]], 0)


def arrange(distinct, n_p, placement, rng):
    """n_p particles that take exactly the poses `distinct` [m][6] (m <= n_p); where the n_p - m copies stand: 'last' behind the
    distinct poses (the first occurrences are particles 0 .. m - 1), 'first' each right behind its original from the front on (the
    first occurrences thin out: chain c is not particle c), 'interleaved' anywhere (a copy's original may stand far behind others)"""
    m = len(distinct)
    d = n_p - m
    assert 1 <= m <= n_p
    if placement == "last":
        order = list(range(m)) + [int(i) for i in rng.randint(0, m, d)]
    elif placement == "first":
        order = [i for i in range(m) for _ in range(1 + d // m + (1 if i < d % m else 0))]
    else:
        order = list(range(m)) + [int(i) for i in rng.randint(0, m, d)]
        order = [order[i] for i in rng.permutation(n_p)]
    assert len(order) == n_p
    out = np.ascontiguousarray(np.asarray(distinct, np.float32)[order])
    assert len(np.unique(out.view(np.uint32).reshape(n_p, 6), axis=0)) == m
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def frames64(pd, is2d):
    """v-, u-, w-axis of the sampling frame of poses pd [n][6] in float64 (make_frame; the reference's 2-D frame has no w)"""
    pd = np.asarray(pd, np.float32).astype(np.float64)
    vx, vy, vz = pd[:, 3], pd[:, 4], pd[:, 5]
    nrm = np.sqrt(vx * vx + vy * vy)
    ok = nrm > 0.0001
    sg = np.where(vy < 0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        ux = np.where(ok, sg * vy / nrm, 1.0)
        uy = np.where(ok, -sg * vx / nrm, 0.0)
    uz = np.zeros_like(ux)
    u = np.stack([ux, uy, uz], 1)
    w = np.stack([uy * vz - uz * vy, -ux * vz + uz * vx, ux * vy - uy * vx], 1)
    if is2d:
        w = np.zeros_like(w)
    return -pd[:, 3:6], u, w


def extents(pd, vuw, is2d):
    """lo, hi [n][3]: the extremes of the sample positions of every pose over the offset grid vuw [M][3] (a full grid: the extremes
    lie at the corners of its offset box)"""
    pd64 = np.asarray(pd, np.float32).astype(np.float64)
    nv, u, w = frames64(pd, is2d)
    o0, o1 = vuw.min(0).astype(np.float64), vuw.max(0).astype(np.float64)
    lo = np.full((len(pd64), 3), np.inf)
    hi = np.full((len(pd64), 3), -np.inf)
    with np.errstate(all="ignore"):
        for a in (o0[0], o1[0]):
            for b in (o0[1], o1[1]):
                for c in (o0[2], o1[2]):
                    pos = pd64[:, :3] + a * nv + b * u + c * w
                    lo, hi = np.fmin(lo, pos), np.fmax(hi, pos)
                    bad = ~np.isfinite(pos)
                    lo[bad], hi[bad] = np.nan, np.nan
    return lo, hi


def trace_geometry(poses, centroid, mode, models, dims, is2d):
    """Per scale the extent of the samples of every pose ph_predict places (lo, hi [S][3]; NaN where a pose is not finite), and the
    verdict of the module docstring on every FL_FAST bit: fast [S] of True / False / None (undecided)."""
    P = []
    if mode != TAIL:
        P.append(np.asarray(poses, np.float32))
    if mode != FIRST:
        P.append(np.asarray(centroid, np.float32)[None])
    P = np.concatenate(P, 0)
    finite = bool(np.isfinite(P).all())
    axes = (0, 1) if is2d else (0, 1, 2)
    S = len(models)
    lo, hi = np.zeros((S, 3)), np.zeros((S, 3))
    for s, vuw in enumerate(models):
        l_, h_ = extents(P, vuw, is2d)
        lo[s] = l_.min(0) if finite else np.nan
        hi[s] = h_.max(0) if finite else np.nan
    fast, vol = [False] * S, [False] * S
    if finite:
        Ulo, Uhi = lo.min(0), hi.max(0)
        for s in range(S):
            sure_set, sure_clear, vol_set, vol_clear = True, False, True, False
            for a in axes:
                lim = dims[a] - 1.001
                if lo[s, a] < -MARGIN or hi[s, a] > lim + MARGIN:
                    sure_clear = vol_clear = True
                if hi[s, a] - lo[s, a] > CS + MARGIN:
                    sure_clear = True
                inside = lo[s, a] - 0.5 >= MARGIN and hi[s, a] + 0.5 <= lim - MARGIN
                vol_set = vol_set and inside
                if dims[a] > CS:
                    mid = 0.5 * (min(max(Ulo[a], 0.0), dims[a] - 1.0) + min(max(Uhi[a], 0.0), dims[a] - 1.0))
                    inside = inside and lo[s, a] >= mid - 24.0 and hi[s, a] <= mid + 24.0
                sure_set = sure_set and inside
            assert not (sure_set and sure_clear)
            fast[s] = True if sure_set else False if sure_clear else None
            vol[s] = True if vol_set else False if vol_clear else None
    return dict(lo=lo, hi=hi, fast=fast, vol=vol, finite=finite)


def spread_groups(trace, vuw, dims, is2d):
    """for the spread trace (distinct poses in particle order, so chain c is particle c): per full chain group of 64 whether the
    samples of the scale with offsets vuw lie surely inside the cube along x (within 24 of the middle of the poses' extent: the
    item-wise corner test of ph_sample passes), surely outside it (more than 30 away), or neither"""
    nch, uidx, _ = chain_numbering(trace["poses"], trace["mode"])
    assert np.array_equal(uidx[:-1], np.arange(nch - 1))
    P = np.concatenate([trace["poses"][:nch - 1], np.asarray(trace["centroid"], np.float32)[None]], 0)
    U = [extents(P, m, is2d) for m in [vuw]][0]
    mid = 0.5 * (max(U[0][:, 0].min(), 0.0) + min(U[1][:, 0].max(), dims[0] - 1.0))
    out = []
    for g in range(nch // 64):
        lo, hi = U[0][64 * g:64 * g + 64, 0].min(), U[1][64 * g:64 * g + 64, 0].max()
        out.append("in" if lo >= mid - 24 and hi <= mid + 24 else "out" if lo < mid - 30 or hi > mid + 30 else "?")
    return out


def fast_bits(fast):
    return sum(1 << s for s, f in enumerate(fast) if f)


def cube_sound(flags, geo, dims, is2d, OX=5, FAST=12):
    """the soundness of a returned placement: 0 <= origin <= max(0, dim - 54), and wherever a fast bit is set every sample of that
    scale lies inside [origin, origin + 53) and inside the volume.  Returns a list of complaints (empty: sound)."""
    bad = []
    org = [int(flags[OX + a]) for a in range(3)]
    for a in range(3):
        if not 0 <= org[a] <= max(0, dims[a] - CS):
            bad.append(f"origin[{a}] = {org[a]} outside [0, {max(0, dims[a] - CS)}]")
    for s in range(len(geo["fast"])):
        if not (int(flags[FAST]) >> s) & 1:
            continue
        for a in ((0, 1) if is2d else (0, 1, 2)):
            lo, hi = geo["lo"][s, a], geo["hi"][s, a]
            if not (lo >= org[a] and hi < org[a] + CS - 1 and lo >= 0 and hi <= dims[a] - 1.001 + 1e-3):
                bad.append(f"scale {s} fast, axis {a}: samples [{lo:.3f}, {hi:.3f}] cube [{org[a]}, {org[a] + CS - 1})")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# pose clusters
# ---------------------------------------------------------------------------------------------------------------------------------
def directions(n, tilt, is2d, rng):
    """n unit directions whose templates stay nearly axis-aligned boxes (a template slab turned by 45 degrees about its normal is
    1.41 times as wide: the cluster's extent would hang on the draw).  3-D: +-z tilted by `tilt` towards an azimuth of k * 90 + 4.6 ..
    5.7 degrees, the first four exactly 5.7 degrees past the four axes, then +z and -z themselves (degenerate: no u axis of their
    own).  2-D: in-plane, at those azimuths."""
    k = np.arange(n) % 4
    dphi = np.concatenate([np.full(4, 0.1), rng.uniform(0.08, 0.1, max(n - 4, 0))])[:n]
    phi = k * (np.pi / 2) + dphi
    if is2d:
        v = np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], 1)
    else:
        sz = np.where((np.arange(n) // 4) % 2 == 0, 1.0, -1.0)
        v = np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), sz * np.cos(tilt)], 1)
        if n > 6:
            v[4], v[5] = (0, 0, 1), (0, 0, -1)
    v = v.astype(np.float32)
    return v / np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)


def cluster(m, centre, jitter, tilt, is2d, rng):
    """m distinct poses around `centre`: positions within +-jitter (per axis; the first six sit on the faces of that box), directions
    from `directions`"""
    jit = np.broadcast_to(np.asarray(jitter, np.float64), (3,))
    off = rng.uniform(-1, 1, (m, 3))
    for i in range(min(m, 6)):
        off[i] = 0
        off[i, i // 2] = -1.0 if i % 2 == 0 else 1.0
    pos = np.asarray(centre, np.float64) + off * jit
    if is2d:
        pos[:, 2] = 0.0
    pd = np.concatenate([pos.astype(np.float32), directions(m, tilt, is2d, rng)], 1).astype(np.float32)
    assert len(np.unique(pd.view(np.uint32).reshape(m, 6), axis=0)) == m
    return pd


def cluster_traces(stack, n_p, rng, jitter=1.0):
    """The pose clusters of the issue for a stack, one trace each: name -> dict(poses [n_p][6], centroid [6], mode, and what the
    cluster is there for).  30 distinct poses per trace (duplicates interleaved), 192 sorted along x in the spread one:
    three full chain groups, of which the outer two reach past the cube and the middle one lies inside."""
    d = STACKS[stack]
    w, h, l = d["w"], d["h"], d["l"]
    is2d = l == 1
    mid = np.array([(w - 1) / 2, (h - 1) / 2, 0.0 if is2d else (l - 1) / 2])
    out = {}

    def add(name, centre, jitter=jitter, tilt=0.12, m=30, mode=REGULAR, centroid=None, **why):
        pd = cluster(m + 1, centre, jitter, tilt, is2d, rng)
        poses = arrange(pd[:m], n_p, "interleaved", rng)
        out[name] = dict(poses=poses, centroid=pd[m] if centroid is None else np.asarray(centroid, np.float32), mode=mode, **why)

    add("interior", mid)
    add("interior_first", mid, mode=FIRST)
    faces = [("x0", 0, 1.0), ("x1", 0, w - 2.0), ("y0", 1, 1.0), ("y1", 1, h - 2.0)] + ([] if is2d else [("z0", 2, 1.0), ("z1", 2, l - 2.0)])
    for name, a, at in faces:
        c = mid.copy()
        c[a] = at
        add("face_" + name, c, clamped=(a, 0 if at < 2 else max(0, (w, h, l)[a] - CS), "low" if at < 2 else "high"))
    add("corner_low", [1.0, 1.0, 0.0 if is2d else 1.0])
    add("corner_last_row", [w - 1.5, h - 1.5, 0.0 if is2d else l - 1.5], jitter=0.4, last_row=True)
    add("tail_corner_last_row", [w - 1.5, h - 1.5, 0.0 if is2d else l - 1.5], mode=TAIL, centroid=[w - 1.25, h - 1.25, 0.0 if is2d else l - 1.25, 0.6, 0.0, 0.8 if not is2d else 0.0])
    pn = cluster(31, mid, jitter, 0.12, is2d, rng)
    pn[3, 0] = np.nan
    pn[7, 4] = np.nan
    out["nan_pose"] = dict(poses=arrange(pn[:30], n_p, "interleaved", rng), centroid=pn[30], mode=REGULAR)
    add("centroid_far_out", mid, centroid=[w + 400.0, -300.0, 0.0 if is2d else l + 1000.0, 0.0, 0.6, 0.8 if not is2d else 0.0])
    add("tail_far_out", mid, mode=TAIL, centroid=[-2.0e6, 5.0e5, 0.0 if is2d else -77.0, 1.0, 0.0, 0.0])
    if w >= 72:  # spread over more than the cube along x, sorted: chain groups at the ends lie outside the cube, the middle one inside
        m = min(192, n_p)
        pd = cluster(m + 1, mid, [31.0, jitter, jitter], 0.12, is2d, rng)
        pd[:m] = pd[np.argsort(pd[:m, 0], kind="stable")]
        pd[m, :3] = mid
        out["spread"] = dict(poses=arrange(pd[:m], n_p, "last", rng), centroid=pd[m], mode=REGULAR, spread=True)
    return out


def count_traces(n_p, nchs, centre, is2d, dims, rng, wide_x=None):
    """One trace per chain count and duplicate placement: name -> dict(poses, centroid, mode, nch).  nch == 1 is a tail pass.  The
    placements go with three clusters so that full chain groups meet all sampling forms: 'first' tight and interior (fast), 'last'
    against the low x face (clamped), 'interleaved' spread along x where the volume is wider than the cube (no clamp, no cube
    promise), else interior."""
    out = {}
    for nch in nchs:
        if nch > n_p + 1:
            continue
        for placement in ("first", "last", "interleaved"):
            c, jit = np.array(centre, np.float64), 1.0
            if placement == "last":
                c[0] = 1.0
            elif placement == "interleaved" and wide_x:
                jit = [wide_x, 1.0, 1.0]
            if nch == 1:
                pd = cluster(1, c, jit, 0.12, is2d, rng)
                out[f"nch1_{placement}"] = dict(poses=np.zeros((n_p, 6), np.float32), centroid=pd[0], mode=TAIL, nch=1)
                continue
            m = nch - 1
            pd = cluster(m + 1, c, jit, 0.12, is2d, rng)
            mode = FIRST if (placement == "first" and nch in (17, 65)) else REGULAR
            out[f"nch{nch}_{placement}"] = dict(poses=arrange(pd[:m], n_p, placement, rng), centroid=pd[m], mode=mode, nch=nch)
    return out


# (particles, stack, scale set) of the chain-count launches
COUNT_CASES = [(200, "wide_thin_z", "s246"), (64, "wide_thin_z", "s246"), (200, "slice", "s246"), (64, "deep_z", "s234"),
               (200, "thin", "s2"), (200, "wide_thin_z", "s3_12"), (64, "slice", "s2468"), (200, "deep_z", "s2468")]


def count_case(n_p, stack):
    """the traces of a chain-count launch (named) and the set of chain regimes they must reach; asserts on the inputs alone that
    they do, and that the numbering is no identity where the copies do not stand last"""
    d = STACKS[stack]
    dims, is2d = (d["w"], d["h"], d["l"]), d["l"] == 1
    centre = [(d["w"] - 1) / 2, (d["h"] - 1) / 2, 0.0 if is2d else (d["l"] - 1) / 2]
    traces = [dict(t, name=k) for k, t in count_traces(n_p, NCH_ALL, centre, is2d, dims, np.random.RandomState(11), wide_x=31.0 if d["w"] >= 90 else None).items()]
    want = {chain_regime(n) for n in NCH_ALL if n <= n_p + 1}
    assert len(traces) == 3 * len(want)
    if n_p == 200:  # (rem, stride, parts, full groups): what the list is there to reach
        assert want == {(1, 16, 64, 0), (2, 16, 32, 0), (16, 16, 4, 0), (17, 32, 3, 0), (32, 32, 2, 0), (33, 64, 1, 0), (63, 64, 1, 0), (0, 0, 1, 1),
                        (1, 16, 64, 1), (16, 16, 4, 1), (33, 64, 1, 1), (0, 0, 1, 2), (1, 16, 64, 2), (9, 16, 7, 3)}
    if n_p == 64:
        assert want == {(1, 16, 64, 0), (2, 16, 32, 0), (16, 16, 4, 0), (17, 32, 3, 0), (32, 32, 2, 0), (33, 64, 1, 0), (63, 64, 1, 0), (0, 0, 1, 1),
                        (1, 16, 64, 1)}
    got = set()
    for t in traces:
        nch, uidx, cmap = chain_numbering(t["poses"], t["mode"])  # from the poses, not from what the generator meant
        assert nch == t["nch"], t["name"]
        got.add(chain_regime(nch))
        if 2 < nch <= n_p and not t["name"].endswith("_last"):
            assert not np.array_equal(uidx[:-1], np.arange(nch - 1)), t["name"]
        if nch > 2 and t["name"].endswith("_interleaved") and nch <= n_p:
            assert (np.diff(cmap) < 0).any(), t["name"]  # a copy stands behind later originals
    assert got == want
    assert {t["mode"] for t in traces} == {FIRST, REGULAR, TAIL}
    return traces, want


def mixed_traces(n, n_p, centre, is2d, rng):
    """n traces of n_p particles for the launch-form test's step list: every (chain count, mode) that n_p particles can give --
    2 .. n_p + 1 chains in a regular and in a first step, the tail pass -- at least once (n_p = 20: 41 of them), the rest again with
    other poses, shuffled so that neighbours in the list differ"""
    out, combos = [], [(nch, mode) for nch in range(2, n_p + 2) for mode in (REGULAR, FIRST)] + [(1, TAIL)]
    assert n >= len(combos)
    combos = combos + [combos[int(i)] for i in rng.randint(0, len(combos), n - len(combos))]
    pick = rng.permutation(n)
    for j, i in enumerate(pick):
        nch, mode = combos[i]
        c = np.array(centre, np.float64)
        if j % 3 == 1:
            c[0] = 1.0  # against the low x face
        pd = cluster(max(nch - 1, 1) + 1, c, 1.0 if j % 3 else [31.0, 1.0, 1.0], 0.12, is2d, rng)
        poses = np.zeros((n_p, 6), np.float32) if mode == TAIL else arrange(pd[:nch - 1], n_p, ("first", "last", "interleaved")[j % 3], rng)
        out.append(dict(poses=poses, centroid=pd[-1], mode=mode, nch=nch))
    return out


def pack(traces):
    """the tap's arguments from a list of trace dicts"""
    return (np.stack([t["poses"] for t in traces]), np.stack([np.asarray(t["centroid"], np.float32) for t in traces]),
            np.array([t["mode"] for t in traces], np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's per-scale values
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_per_chain(tracker, img, traces):
    """per trace: ref [S][nch] the oracle's per-scale correlation of every chain's pose, and ok [nch]: False for a chain whose pose
    is not finite -- the reference's interp indexes the image with (int)NaN there, it HAS no value for such a pose -- and for the
    closing chain of a first step, which the step evaluates on zeros and never reads; every distinct pose is evaluated once.  Returns (refs, oks, distinct poses evaluated)."""
    chains = [chain_poses(t["poses"], t["centroid"], t["mode"]) for t in traces]
    allp = np.concatenate(chains, 0)
    fin = np.isfinite(allp).all(1)
    uniq, inv = np.unique(allp[fin].view(np.uint32).reshape(-1, 6), axis=0, return_inverse=True)
    _, _, per_u = tracker.zncc_scales(img, uniq.view(np.float32))
    per = np.zeros((len(allp), per_u.shape[1]), np.float32)
    per[fin] = per_u[inv.reshape(-1)]
    refs, oks, at = [], [], 0
    for c in chains:
        refs.append(np.ascontiguousarray(per[at:at + len(c)].T))
        oks.append(fin[at:at + len(c)].copy())
        if traces[len(oks) - 1]["mode"] == FIRST:
            oks[-1][-1] = False  # no centroid yet: the closing chain is evaluated on zeros outside the rows staged for the particles, and discarded
        at += len(c)
    return refs, oks, len(uniq)
