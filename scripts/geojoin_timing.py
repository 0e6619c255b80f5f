"""Device time of pnr_geodesic_bridges on the SIZE^3 bench stack: the forest is the bench tree as reconstruct() leaves it (every fragment
a tree); reported are the Boruvka rounds and bridges, the inserted nodes, the time of the two meet passes per sweep and their achieved
bytes/s against the floor of 8 N bytes of keys per sweep, "geojoin" as a share of "geodesic" + "geojoin", and beside it what geo_stats --
a plain 8 N-byte sweep of the same keys in geodesic.hip -- achieves on the same stack: that comparison is the yardstick.
On an MI355X:   python scripts/geojoin_timing.py [size] > profiles/rNN_geojoin_SIZE.txt   (default size 512)

Device time: the library's kernel timers (HIP events on the context's stream around the launches of one call), warmed up first.  The stack
is borrowed (pnr_set_volume_device); the call never writes it.  The bench tree: the bench stack traced and reconstructed with the README
parameters (rng_seed 42).  A sweep also reads the N bytes of the volume; the floor counts the keys alone."""
import os
import sys
import time
import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import synth  # noqa: E402
import pnr_amd  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N = S ** 3
REPS = 3
ZD = 2.0
img = synth.synth_torch(S, S, S, seed=3, zdist=ZD)
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), np_=200, ni=200, zdist=ZD, rng_seed=42), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
t0 = time.time()
res = pnr_amd.advantra.run_pipeline(ctx, None)
tree, parent = res["tree"], res["parent"]
xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:].astype(np.float32)
par = np.where(parent[1:] > 0, parent[1:] - 1, -1).astype(np.int32)
print(f"pnr_geodesic_bridges on {S}^3 u8 ({N / 1e9:.3f} G voxels), zdist = {ZD}")
print(f"bench forest: {len(xyz)} nodes in {int((par < 0).sum())} trees (pipeline {time.time() - t0:.2f} s)")
ctx.set_profiling(True)


def once(thr, limit):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    bridges, paths, info = ctx.join_trees_geodesic(xyz, par, limit=limit, thr=thr)
    wall = (time.perf_counter() - t0) * 1e3
    groups = {g: ctx.kernel_ms(g) for g in ("geojoin_meet_w", "geojoin_meet_e", "geojoin", "geodesic", "geodesic_relax", "geodesic_stats", "geodesic_paths")}
    return info, groups, wall, bridges


def report(name, thr, limit):
    once(thr, limit)  # warm-up: code objects, first allocations
    runs = [once(thr, limit) for _ in range(REPS)]
    info, bridges = runs[0][0], runs[0][3]
    rounds = info["rounds"]
    print(f"{name}: thr = {thr} (used: {info['thr_used']}), limit = {limit}, {REPS} repeats after a warm-up")
    print(f"trees {info['n_trees_in']} -> {info['n_trees_out']} ({info['n_trees_lost']} lost), bridges {info['n_bridges']}, inserted nodes {info['n_inserted']}, "
          f"rounds {rounds}, w_max {info['w_max']} (= {info['w_max'] / 64:.1f} xy voxels at cost 1), sources kept {info['n_src']} dropped {info['n_src_dropped']}, "
          f"longest chain {int(bridges['path_len'].max()) if len(bridges) else 0} voxels")
    print(f"{'group':<16} {'device ms med':>14} {'min':>10} {'max':>10} {'launches':>9} {'ms / sweep':>11} {'GB/s of 8 N':>12}")
    med = {}
    for g in ("geojoin_meet_w", "geojoin_meet_e", "geodesic_stats", "geodesic_relax", "geodesic_paths", "geodesic", "geojoin"):
        ms = np.array([r[1][g][0] for r in runs])
        med[g] = float(np.median(ms))
        launches = runs[0][1][g][1]
        sweeps = rounds if g.startswith("geojoin_meet") else 1 if g == "geodesic_stats" else 0
        per = f"{med[g] / sweeps:>11.3f} {8 * N / (med[g] / sweeps * 1e-3) / 1e9:>12.1f}" if sweeps and med[g] > 0 else ""
        print(f"{g:<16} {med[g]:>14.3f} {ms.min():>10.3f} {ms.max():>10.3f} {launches:>9} {per}")
    walls = np.array([r[2] for r in runs])
    both = med["geodesic"] + med["geojoin"]
    print(f"geojoin / (geodesic + geojoin) = {med['geojoin'] / both:.4f}; bytes per sweep 8 N = {8 * N / 1e6:.1f} MB, {2 * rounds} sweeps = {2 * rounds * 8 * N / 1e9:.2f} GB; "
          f"call wall ms (host loops, sampling, paths, download) {float(np.median(walls)):.1f}\n")
    sys.stdout.flush()
    return info


print()
full = report("every voxel passable, no limit", 0, 0)
report("every voxel passable, half of w_max", 0, max(1, full["w_max"] // 2))
report("foreground only, no limit", -1, 0)
ctx.close()
