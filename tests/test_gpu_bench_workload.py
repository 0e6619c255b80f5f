"""The bench.py workload at its real size against the oracle: what `bench.py --steps 1 --warmup 1 --dump-outputs DIR` computes on
the 1024^3 stack (scales {2,4,6}, zdist 2, np 200, ni 200, the first 2000 sorted seeds traced by the streaming scheduler), and
the same stack rebuilt in this process, stage by stage:

  * Frangi: the pruned run's extremes are the bench run's and the exact re-run's; its J8 and seeds are the exact re-run's over
    the whole volume (work-groups of 8 Hessian z-chunks in whatever order they run); J / J8 / V against the oracle on sub-volumes
    cut with the halo the stencils need, around the volume faces, the z-chunk boundaries of every scale (128-plane chunks; the
    pruned first scale's middle march [512, 544) and the chunks after it), an x / y corner and the maximum of J.
  * seeds of all 1024 layers against the oracle's extractSeeds; znccBBB scores, threshold and stable sort of all of them against
    the oracle's; the first 2000 are the seeds the bench run traced.
  * the one-shot traces of those 2000 seeds: every iteration of a sample of them against the oracle's tracker on the full stack,
    to full depth in both directions; the replayed node graph against the oracle's replay and against the bench run's streamed
    graph.
The oracle's Frangi of the whole stack (~35 min on one core) stays out: sub-volumes stand in for it."""
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import orc
import synth
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, SIGS, ZDIST, NP, NI, NSEEDS = 1024, (2.0, 4.0, 6.0), 2.0, 200, 200, 2000  # bench.py main() and its defaults
J_RTOL = 2e-6  # (tests/test_gpu_frangi.py: fp64 exp of the device library vs glibc)
HX, HZ = 20, 11  # halo of a sub-volume: ceil(3 * 6) + 2 in x / y, ceil(3 * 6 / zdist) + 2 in z
IX, IZ = 96, 24  # interior of a sub-volume
# interiors in z across the boundaries of the Hessian z-chunks (128 planes at 1024 x 1024): 127 | 128 (every scale), 511 | 512 and
# 543 | 544 (the pruned first scale's middle march, run first), 895 | 896 (the other scales), 927 | 928 (the first scale's last chunk)
Z_CUTS = ((116, 140), (506, 550), (884, 908), (916, 940))
BUDGET_S = 300
THREADS = min(16, len(os.sched_getaffinity(0)))
mat = lambda a: np.stack([a[k] for k in a.dtype.names], -1)


def _pool(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:  # (the oracle's ctypes calls release the GIL)
        return list(ex.map(fn, items))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import torch
    t0 = time.time()
    out = tmp_path_factory.mktemp("bench_dump")
    # the bench step itself, in a process of its own, before this one sets up a context of its own
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(out))
    assert files == ["jminmax.npy", "links.npy", "nodes.npy", "seeds.npy", "traces_used.npy"], files  # (no *_rows.npy: dumped whole)
    dump = {f[:-4]: np.load(out / f) for f in files}
    t_bench = time.time() - t0
    # the same stack and parameters in this process
    vol = synth.synth_torch(S, S, S, seed=3, device="cuda")
    torch.cuda.synchronize()
    p = pnr_amd.make_params(sigmas=SIGS, np_=NP, ni=NI, zdist=ZDIST)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver("phased")
    c.set_volume_device(vol.data_ptr(), (S, S, S), keepalive=vol)
    st = dict(t0=t0, t_bench=t_bench, dump=dump, c=c, p=p, img=vol.cpu().numpy())
    st["jminmax"] = c.frangi()  # what the pipeline runs: the J8 shortcut (option frangi_prune)
    st["fast8"] = c.get_frangi(J=False, J8=True, V=False)["J8"]
    st["seeds_fast"] = c.extract_seeds()
    rec = c.get_option("frangi_recomputes")
    st.update(c.get_frangi(J=True, J8=True, V=True))  # the exact response of every voxel: one more Frangi pass without the shortcut
    st["recomputes"] = c.get_option("frangi_recomputes") - rec
    st["seeds"] = c.extract_seeds()
    st["sorted"] = c.score_filter_sort(st["seeds"])
    sel = st["sorted"][:NSEEDS]
    t1 = time.time()
    st["T"], st["stop"], st["xc"], _ = c.trace_batch(sel)  # one-shot: every trace to its map-free end
    st["graph"] = c.replay(sel, st["T"], st["xc"])
    st["t_trace"] = time.time() - t1
    yield st
    c.close()
    del vol, st
    torch.cuda.empty_cache()


def test_pruned_frangi_is_the_exact_one_and_the_bench_runs(run):
    jmin, jmax = run["jminmax"]
    assert np.array_equal(np.float32(run["dump"]["jminmax"]), np.float32([jmin, jmax])), (run["dump"]["jminmax"], jmin, jmax)
    assert jmin == 0.0 and jmax > 0
    assert run["recomputes"] == 1
    # which voxels the shortcut skips depends on the order the work-groups run in; J8, the extremes and the seeds do not
    assert np.array_equal(run.pop("fast8"), run["J8"])
    J = run["J"]
    assert J.min() == jmin and J.max() == jmax
    a, b = run["seeds_fast"], run["seeds"]
    assert len(a) == len(b) > 10000 and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a.dtype.names)


def test_frangi_subvolumes_vs_oracle(run, oracle):
    """J / J8 / V on sub-volumes across the z-chunk boundaries: every scale's at 128 | 896 (chunks of 128 planes), the pruned first
    scale's middle march 511 | 512 ... 543 | 544 and its next chunks' 927 | 928; the two volume faces (cut at the face: the oracle
    applies the same one-sided borders), each at an x / y corner; the voxel of the maximum"""
    img, J, J8, jmin, jmax = run["img"], run["J"], run["J8"], *run["jminmax"]
    s = run["seeds"]
    vessel = {}  # sub-volumes with tubes: interior centred on the strongest seed of their planes

    def around(z0, z1):
        k = np.flatnonzero((s["z"] >= z0) & (s["z"] < z1))
        assert len(k), (z0, z1)
        k = k[np.argmax(J8[s["z"][k].astype(int), s["y"][k].astype(int), s["x"][k].astype(int)])]
        x0 = int(np.clip(int(s["x"][k]) - IX // 2, 0, S - IX))
        y0 = int(np.clip(int(s["y"][k]) - IX // 2, 0, S - IX))
        return (z0, z1, y0, y0 + IX, x0, x0 + IX)

    for z0, z1 in Z_CUTS:
        vessel[(z0, z1)] = around(z0, z1)
    zc, yc, xc = np.unravel_index(int(np.argmax(J)), J.shape)
    box = lambda c_, n: (int(np.clip(c_ - n // 2, 0, S - n)), int(np.clip(c_ - n // 2, 0, S - n)) + n)
    cases = list(vessel.values()) + [(0, IZ, 0, IX, 0, IX), (S - IZ, S, S - IX, S, S - IX, S), (*box(zc, IZ), *box(yc, IX), *box(xc, IX))]

    def check(b):
        z0, z1, y0, y1, x0, x1 = b
        Z0, Y0, X0 = max(0, z0 - HZ), max(0, y0 - HX), max(0, x0 - HX)
        sub = np.ascontiguousarray(img[Z0:min(S, z1 + HZ), Y0:min(S, y1 + HX), X0:min(S, x1 + HX)])
        Jo, _, _, Vxo, Vyo, Vzo = orc.frangi3d(oracle, sub, list(SIGS), ZDIST)
        inner = (slice(z0 - Z0, z1 - Z0), slice(y0 - Y0, y1 - Y0), slice(x0 - X0, x1 - X0))
        full = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        Jo = np.ascontiguousarray(Jo[inner])
        out = dict(J=np.allclose(J[full], Jo, rtol=J_RTOL, atol=0), nz=int((Jo > 0).sum()), J8=np.array_equal(J8[full], orc.j8(oracle, Jo, jmin, jmax)),
                   nz8=int((J8[full] > 0).sum()))
        for k, Vo in (("Vx", Vxo), ("Vy", Vyo), ("Vz", Vzo)):
            out[k] = np.array_equal(run[k][full], Vo[inner])
        if z0 <= zc < z1 and y0 <= yc < y1 and x0 <= xc < x1:
            out["Jo_at_max"] = float(Jo[zc - z0, yc - y0, xc - x0])
        return out

    res = _pool(check, cases)
    for b, r in zip(cases, res):
        assert r["J"] and r["J8"] and r["Vx"] and r["Vy"] and r["Vz"] and r["nz"] > 1000, (b, r)
        if b[:2] in vessel:
            assert r["nz8"] > 100, (b, r)
    assert abs(res[-1]["Jo_at_max"] - jmax) <= J_RTOL * jmax, (res[-1], jmax)
    assert J[zc, yc, xc] == jmax
    del run["J"]  # (4 GB of host memory)


def test_seeds_of_every_layer_vs_oracle(run, oracle):
    """SeedExtractor::extractSeeds is per layer (seed.cpp:574): the oracle on each of the 1024 layers as a one-slice stack, in layer
    order, gives the whole stack's seeds"""
    J8, Vx, Vy, Vz = (run[k] for k in ("J8", "Vx", "Vy", "Vz"))

    def layer(z):
        so = orc.extract_seeds(oracle, 5, J8[z:z + 1], Vx[z:z + 1], Vy[z:z + 1], Vz[z:z + 1])
        so[:, 2] = z
        return so

    so = np.concatenate(_pool(layer, range(S)))
    sg = run["seeds"]
    assert len(sg) == len(so) > 10000 and np.array_equal(mat(sg)[:, :6], so[:, :6])
    print(f"\n[bench workload] seeds {len(so)}")
    for k in ("J8", "Vx", "Vy", "Vz"):
        del run[k]


def test_scores_and_sort_vs_oracle(run, oracle):
    """znccBBB of every seed on the full stack, the znccth threshold and a stable descending sort, against score_filter_sort(); the
    first 2000 are the seeds the bench run traced"""
    img, sg, ss = run["img"], run["seeds"], run["sorted"]
    pd = mat(sg)[:, :6]
    parts = np.array_split(np.arange(len(pd)), THREADS)
    corr = np.concatenate(_pool(lambda ix: orc.Tracker(oracle, SIGS, 2, NP, NI, 3.0, 0.3, zdist=ZDIST).zncc(img, pd[ix])[0], parts))
    keep = corr >= np.float32(run["p"].znccth)
    order = np.argsort(-corr[keep], kind="stable")
    assert len(ss) == keep.sum() >= NSEEDS
    assert np.array_equal(ss["corr"], corr[keep][order]) and np.array_equal(mat(ss)[:, :6], pd[keep][order])
    assert np.array_equal(mat(ss[:NSEEDS]).astype(np.float64), run["dump"]["seeds"], equal_nan=True)
    print(f"\n[bench workload] scores {len(corr)}, kept {len(ss)}")


def test_traces_vs_oracle(run, oracle):
    """every estimate, T and stop reason of the one-shot traces of the first three sorted seeds and five drawn from the 2000, to full
    depth in both directions, against the oracle's tracker on the full stack (one tracker per thread).  At most 16 x ni = 3200 oracle
    iterations of 25 - 72 ms each (np 200, three scales), 16 traces on as many threads."""
    img, sel, T, stop, xc = run["img"], run["sorted"][:NSEEDS], run["T"], run["stop"], run["xc"]
    rows = np.minimum(T + 1, NI)  # iterations a trace runs: its nodes and the one that stopped it
    pick = [0, 1, 2] + sorted(np.random.default_rng(7).choice(np.arange(3, NSEEDS), 5, replace=False).tolist())
    its = int(sum(rows[2 * i] + rows[2 * i + 1] for i in pick))
    jobs = [(i, d_) for i in pick for d_ in (0, 1)]

    def trace(job):
        i, d_ = job
        q = np.array([sel[k][i] for k in lib.SEED_DT.names[:6]], np.float32)
        q[3:] *= (1, -1)[d_]
        Tn, so, xco, *_ = orc.Tracker(oracle, SIGS, 2, NP, NI, 3.0, 0.3, zdist=ZDIST).trace(img, q)
        return Tn, so, xco

    for (i, d_), (Tn, so, xco) in zip(jobs, _pool(trace, jobs)):
        j = 2 * i + d_
        n = min(Tn + 1, NI)
        assert T[j] == Tn and stop[j] == so and np.array_equal(mat(xc[j])[:n], xco[:n], equal_nan=True), (i, d_, T[j], Tn, stop[j], so)
    assert its > 300, (pick, its)
    print(f"\n[bench workload] traces {len(jobs)} of seeds {pick}, oracle iterations {its}")


def test_graph_vs_oracle_and_the_bench_run(run, oracle):
    """the replay of the 2000 seeds' one-shot traces against the oracle's replay, and against the graph the bench run's streaming
    scheduler (two trace groups, early DENSITY stops) built"""
    p, sel, T, xc = run["p"], run["sorted"][:NSEEDS], run["T"], run["xc"]
    nodes, links, nt = run["graph"]
    xcm = np.ascontiguousarray(xc).view(np.float32).reshape(len(T), NI, 8)
    no, lo, nto = orc.replay(oracle, mat(sel).astype(np.float32), T.astype(np.int32), xcm, NI, (S, S, S), p.nodepervol, p.vol)
    assert nt == nto and len(no) == len(nodes) and np.array_equal(lo, links)
    assert all(np.array_equal(nodes[k], no[k], equal_nan=True) for k in nodes.dtype.names)
    d = run["dump"]
    got = np.stack([nodes[k].astype(np.float64) for k in lib.NODE_DT.names], 1)
    assert got.shape == d["nodes"].shape and np.array_equal(got, d["nodes"], equal_nan=True)
    assert np.array_equal(links.astype(np.float64), d["links"]) and int(d["traces_used"][0]) == nt
    wall = time.time() - run["t0"]
    print(f"\n[bench workload] nodes {len(nodes) - 1}, links {len(links)}, traces used {nt}; bench run {run['t_bench']:.1f} s, "
          f"one-shot tracing + replay {run['t_trace']:.1f} s, module {wall:.1f} s")
    assert wall < BUDGET_S, "this module is meant to stay well inside the GPU test budget"
