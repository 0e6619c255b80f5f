"""Device time of pnr_geodesic_distance per phase on the SIZE^3 bench stack, from the sample points of the bench tree: once with every voxel
passable (thr = 0, dmax unbounded: the cost alone steers the front through the whole stack) and once over the foreground only (thr = -1:
the stack's mean), with the rounds, the tile visits, the voxels reached and the bytes the relaxation moves per round against the 8 N bytes
of the keys.
On an MI355X:   python scripts/geodesic_timing.py [size] > profiles/rNN_geodesic_SIZE.txt   (default size 1024; the committed records
are profiles/r12_geodesic_256.txt, profiles/r12_geodesic_512.txt, profiles/r19_geodesic_512_*.txt and profiles/r19_geodesic_1024_*.txt)

Device time: the library's "geodesic_*" kernel timers (HIP events on the context's stream around each launch of one call), warmed up
first.  The stack is borrowed (pnr_set_volume_device); the call never writes it; D and L stay on the device (volume=False: summary only).
The bench tree: the bench stack traced and reconstructed with the README parameters (rng_seed 42).  A tile visit reads the keys (8 B) and
bytes (1 B) of its (TX + 2) (TY + 2) (TZ + 2) cells and writes at most 8 TX TY TZ bytes back: that is the traffic counted.  If scipy is
present, the CPU time of scipy.sparse.csgraph.dijkstra on a 128^3 crop goes beside it for orientation only."""
import os
import re
import sys
import time
import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import synth  # noqa: E402
import pnr_amd  # noqa: E402
from pnr_amd import lib  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = S ** 3
REPS = 3
ZD = 2.0
PHASES = ("threshold", "init", "compact", "relax", "stats", "split", "sample", "paths")
TILE = {k: int(v) for k, v in re.findall(r"constexpr int (GEO_TX|GEO_TY|GEO_TZ) = (\d+);", open(os.path.join(R, "pnr_amd", "csrc", "geodesic.h")).read())}
TX, TY, TZ = TILE["GEO_TX"], TILE["GEO_TY"], TILE["GEO_TZ"]
VISIT_BYTES = 9 * (TX + 2) * (TY + 2) * (TZ + 2) + 8 * TX * TY * TZ
img = synth.synth_torch(S, S, S, seed=3, zdist=ZD)
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), np_=200, ni=200, zdist=ZD, rng_seed=42), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
t0 = time.time()
res = pnr_amd.advantra.run_pipeline(ctx, None)
tree, parent = res["tree"], res["parent"]
xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:].astype(np.float32)
par = np.where(parent[1:] > 0, parent[1:] - 1, -1).astype(np.int32)
src, owner = lib.tree_sample(xyz, par, 1, 1)
print(f"pnr_geodesic_distance on {S}^3 u8 ({N / 1e9:.3f} G voxels), zdist = {ZD}, tiles of {TX} x {TY} x {TZ}")
print(f"bench tree: {len(xyz)} nodes, {len(src)} sample points at step 1 = sources, labelled with their owner node (pipeline {time.time() - t0:.2f} s)")
ctx.set_profiling(True)
pts = np.random.default_rng(1).uniform(0, S, (10000, 3)).astype(np.float32)


def once(thr):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info, _, _, _ = ctx.geodesic(src, owner, thr=thr, volume=False, targets=pts)
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("geodesic_" + p) for p in PHASES}, ctx.kernel_ms("geodesic")[0], wall, ctx.get_option("geo_visits")


def report(name, thr):
    once(thr)  # warm-up: code objects, first allocations
    runs = [once(thr) for _ in range(REPS)]
    info, visits = runs[0][0], runs[0][4]
    print(f"{name}: thr = {thr} (used: {info['thr_used']}), dmax unbounded, 10000 targets, {REPS} repeats after a warm-up")
    print(f"passable {info['n_pass']} of {info['n_vox']} voxels, reached {info['n_reached']}, sources kept {info['n_src']} dropped {info['n_src_dropped']}, "
          f"d_max {info['d_max']} (= {info['d_max'] / 64:.1f} xy voxels at cost 1) at {info['max_at']}")
    print(f"{'phase':<10} {'device ms med':>14} {'min':>10} {'max':>10} {'launches':>9}")
    for p in PHASES:
        ms = np.array([r[1][p][0] for r in runs])
        print(f"{p:<10} {float(np.median(ms)):>14.3f} {ms.min():>10.3f} {ms.max():>10.3f} {runs[0][1][p][1]:>9}")
    tot = np.array([r[2] for r in runs])
    walls = np.array([r[3] for r in runs])
    rounds = info["rounds"]
    per_round = visits * VISIT_BYTES / max(rounds, 1)
    print(f"{'all':<10} {float(np.median(tot)):>14.3f} {tot.min():>10.3f} {tot.max():>10.3f}   call wall ms (host loop, no download) {float(np.median(walls)):.3f}")
    print(f"rounds {rounds}, tile visits {visits} ({visits / max(rounds, 1):.0f} per round; the stack has {-(-S // TX) * -(-S // TY) * -(-S // TZ)} tiles), "
          f"bytes per round {per_round / 1e6:.1f} MB = {per_round / (8 * N):.4f} of 8 N, all rounds {visits * VISIT_BYTES / 1e9:.2f} GB = {visits * VISIT_BYTES / (8 * N):.2f} x 8 N\n")
    sys.stdout.flush()
    return info


print()
report("every voxel passable", 0)
info = report("foreground only", -1)
ctx.close()
C = min(S, 128)
host = img[:C, :C, :C].cpu().numpy()
inside = (src < C).all(1)
try:
    from scipy import sparse
    from scipy.sparse import csgraph
    sys.path.insert(0, os.path.join(R, "tests"))
    import geodesic_ref as ref
    cost = (256 - host.astype(np.int64)).ravel()
    idx = np.arange(C ** 3).reshape(C, C, C)
    rows, cols, wts = [], [], []
    for (dx, dy, dz), le in zip(ref.OFFSETS, ref.lengths(ZD)):
        (px, qx), (py, qy), (pz, qz) = ref._slices(dx, C), ref._slices(dy, C), ref._slices(dz, C)
        p, q = idx[pz, py, px].ravel(), idx[qz, qy, qx].ravel()
        rows.append(p), cols.append(q), wts.append(le * (cost[p] + cost[q]))
    G = sparse.csr_matrix((np.concatenate(wts).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(C ** 3, C ** 3))
    c = np.minimum(np.maximum(src[inside] + np.float32(0.5), 0), C - 1).astype(np.int64)
    start = np.unique(c[:, 0] + C * (c[:, 1] + C * c[:, 2]))
    t0 = time.perf_counter()
    d = csgraph.dijkstra(G, indices=start, min_only=True) if len(start) else np.zeros(1)
    print(f"orientation only: scipy.sparse.csgraph.dijkstra on the CPU, a {C}^3 crop with every voxel passable, {len(start)} source voxels: "
          f"{time.perf_counter() - t0:.2f} s (without building the graph), d_max {int(d[np.isfinite(d)].max())}")
except ImportError:
    print("orientation only: scipy is not installed, no CPU time")
