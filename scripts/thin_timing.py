"""Device time of pnr_skeletonize per kernel group on the SIZE^3 bench stack (thr = -1) and on the same stack with a radius-40 ball in
it (the soma case: neurites are thin after a round or two, the ball takes tens), with what the shrinking work saves: the tiles the passes
visited against 8 * rounds * tiles, and the state bytes read per round against N.
On an MI355X:   timeout 600 python scripts/thin_timing.py [size] > profiles/r14_thin_SIZE.txt

Device time: the library's "thin_*" kernel timers (HIP events on the context's stream around each kernel of one call), warmed up first;
one process, no retry.  The stack is borrowed (pnr_set_volume_device); the call never writes it; neither the 0 / 255 volume nor the
voxel list is handed out (volume=False, voxels=False: the summary only).  The floor to compare with is one read of the state per visited tile per pass."""
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
import thin_ref  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N = S ** 3
REPS = 3
PHASES = ("threshold", "init", "mark", "pass", "list", "finish")
TX, TY, TZ = thin_ref.tile()
TILE = TX * TY * TZ
HALO = (TX + 2) * (TY + 2) * (TZ + 2)
ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), zdist=2.0), 0)
ctx.set_profiling(True)


def once(thr):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info = ctx.skeletonize(thr, volume=False, voxels=False)[0]
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("thin_" + p) for p in PHASES}, ctx.kernel_ms("thin")[0], wall


def report(name, img, thr):
    ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
    once(thr)  # warm-up: code objects, first allocations
    runs = [once(thr) for _ in range(REPS)]
    info = runs[0][0]
    assert all(r[0] == info for r in runs)  # tile_visits included
    rounds, tiles, visits = info["rounds"], info["tiles"], info["tile_visits"]
    print(f"{name}: thr = {thr} (used: {info['thr_used']}), {REPS} repeats after a warm-up")
    print(f"foreground {info['n_fg']} of {info['n_vox']} voxels -> skeleton {info['n_skel']} (ends {info['n_end']}, branches {info['n_branch']}, isolated {info['n_isolated']}), "
          f"{rounds} rounds")
    print(f"tile visits {visits} of 8 * rounds * tiles = {8 * rounds * tiles} ({100 * visits / (8 * rounds * tiles):.1f} %), first round {8 * tiles}")
    print(f"state read by the passes {visits * HALO / 1e9:.3f} GB = {visits * HALO / rounds / N:.2f} N per round (one tile with its halo: {HALO} B for {TILE} voxels;"
          f" all tiles in all eight passes: {8 * HALO / TILE:.1f} N)")
    print(f"{'group':<10} {'device ms med':>14} {'min':>8} {'max':>8} {'launches':>9}")
    for p in PHASES:
        ms = np.array([r[1][p][0] for r in runs])
        print(f"{p:<10} {float(np.median(ms)):>14.3f} {ms.min():>8.3f} {ms.max():>8.3f} {runs[0][1][p][1]:>9d}")
    tot = np.array([r[2] for r in runs])
    walls = np.array([r[3] for r in runs])
    med, pas = float(np.median(tot)), float(np.median([r[1]["pass"][0] for r in runs]))
    print(f"{'all':<10} {med:>14.3f} {tot.min():>8.3f} {tot.max():>8.3f}   passes: {visits * HALO / 1e9 / (pas / 1e3):.0f} GB/s of state, {pas / rounds:.3f} ms per round;"
          f"   call wall ms {float(np.median(walls)):.1f} (one read-back per round)\n")
    sys.stdout.flush()


print(f"pnr_skeletonize on {S}^3 u8 ({N / 1e9:.3f} G voxels), tiles of {TX} x {TY} x {TZ}")
img = synth.synth_torch(S, S, S, seed=3, zdist=2.0)
torch.cuda.synchronize()
report("bench stack", img, -1)
soma = img.clone()
yy, xx = torch.meshgrid(torch.arange(S, device="cuda"), torch.arange(S, device="cuda"), indexing="ij")
for k in range(max(S // 2 - 40, 0), min(S // 2 + 41, S)):  # the ball plane by plane
    soma[k][(k - S // 2) ** 2 + (yy - S // 2) ** 2 + (xx - S // 2) ** 2 <= 40 * 40] = 255
torch.cuda.synchronize()
report("bench stack with a radius-40 ball (the soma case)", soma, -1)
ctx.close()
