"""Device time of pnr_watershed per kernel on the SIZE^3 bench stack, markers from the sample points of the bench tree (the sources of
scripts/geodesic_timing.py, so that the two can stand side by side): once with every voxel in the mask (thr = 0) and once over the
foreground only (thr = -1: the stack's mean), relief = 255 - V, C = 26, with the rounds and tile visits of both passes and the bytes each
pass stages per round against the floor of one key read and write per visited voxel.
On an MI355X:   python scripts/watershed_timing.py [size] > profiles/rNN_watershed_SIZE.txt   (default size 512; run it under `timeout`,
one size per process)

Device time: the library's "watershed_*" kernel timers (HIP events on the context's stream around each launch of one call), warmed up
first.  The stack is borrowed (pnr_set_volume_device); the call never writes it; L and M stay on the device (volume=False: summary only).
The bench tree: the bench stack traced and reconstructed with the README parameters (rng_seed 42).  A visit of ws_flood reads the keys
(4 B) and the stack's bytes (1 B) of its (TX + 2) (TY + 2) (TZ + 2) cells and the relief (1 B) of its TX TY TZ voxels and writes at most
4 TX TY TZ bytes back; a visit of ws_label reads keys and labels (8 B) of all cells and the relief of its own: that is the traffic counted.
There is no parent to compare with: the project had no watershed before."""
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
from pnr_amd import lib  # noqa: E402
import ws_ref  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N = S ** 3
REPS = 3
ZD = 2.0
PARTS = ("init", "compact", "flood", "label", "finish")
TZ, TY, TX = ws_ref.tile()
TILES = -(-S // TX) * -(-S // TY) * -(-S // TZ)
CELLS, OWN = (TX + 2) * (TY + 2) * (TZ + 2), TX * TY * TZ
VISIT_BYTES = {"flood": 5 * CELLS + OWN + 4 * OWN, "label": 8 * CELLS + OWN + 4 * OWN}
FLOOR = 8 * OWN  # one key (or label) read and written per visited voxel
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
print(f"pnr_watershed on {S}^3 u8 ({N / 1e9:.3f} G voxels), relief = 255 - V, C = 26, tiles of {TX} x {TY} x {TZ}: {TILES} tiles")
print(f"bench tree: {len(xyz)} nodes, {len(src)} sample points at step 1 = markers, labelled with 1 + their owner node (pipeline {time.time() - t0:.2f} s)")
ctx.set_profiling(True)


def once(thr):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info, _, _ = ctx.watershed(points=src, labels=owner + 1, thr=thr, connectivity=26, volume=False)
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("watershed_" + p) for p in PARTS}, ctx.kernel_ms("watershed")[0], wall


def report(name, thr):
    once(thr)  # warm-up: code objects, first allocations
    runs = [once(thr) for _ in range(REPS)]
    info = runs[0][0]
    print(f"\n{name}: thr = {thr} (used: {info['thr_used']}), {REPS} repeats after a warm-up")
    print(f"mask {info['n_mask']} of {info['n_vox']} voxels, reached {info['n_reached']}, unreached {info['n_unreached']}, marker voxels {info['n_marker_vox']}, "
          f"dropped {info['n_dropped']}, regions {info['n_regions']}, m_max {info['m_max']}, d_max {info['d_max']}")
    print(f"{'kernel':<10} {'device ms med':>14} {'min':>10} {'max':>10} {'launches':>9}")
    for p in PARTS:
        ms = np.array([r[1][p][0] for r in runs])
        print(f"{p:<10} {float(np.median(ms)):>14.3f} {ms.min():>10.3f} {ms.max():>10.3f} {runs[0][1][p][1]:>9}")
    tot = np.array([r[2] for r in runs])
    walls = np.array([r[3] for r in runs])
    print(f"{'all':<10} {float(np.median(tot)):>14.3f} {tot.min():>10.3f} {tot.max():>10.3f}   call wall ms (host loop, no download) {float(np.median(walls)):.3f}")
    for k, r in enumerate(runs):  # (the visits of a run depend on what its tiles saw of one another inside a launch)
        for p in ("flood", "label"):
            rounds, visits, ms = r[0][p + "_rounds"], r[0][p + "_visits"], r[1][p][0]
            staged = visits * VISIT_BYTES[p]
            print(f"run {k} {p}: rounds {rounds}, tile visits {visits} ({visits / TILES:.2f} per tile, {visits / max(rounds, 1):.0f} per round), bytes per round "
                  f"{staged / max(rounds, 1) / 1e6:.1f} MB, all rounds {staged / 1e9:.2f} GB = {VISIT_BYTES[p] / FLOOR:.2f} x the floor of {visits * FLOOR / 1e9:.2f} GB, "
                  f"{staged / 1e9 / max(ms, 1e-9) * 1e3:.0f} GB/s over the pass")
    sys.stdout.flush()


report("every voxel in the mask", 0)
report("foreground only", -1)
ctx.close()
