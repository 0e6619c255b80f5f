"""Device time of the morphological reconstruction per part on the SIZE^3 bench stack: the 3-D grey fill (PNR_MORPH_FILL, C = 6) and the
h-maxima at h = 16 (PNR_MORPH_HMAX, C = 26), with the rounds, the tile visits against rounds x tiles, and the bytes the relaxation stages per
second against the one-pass floor of 3 N bytes (read V, read and write the state).
On an MI355X:   python scripts/morph_timing.py [size] > profiles/rNN_morph_SIZE.txt   (default size 512; run it under `timeout`, one size
per process)

Device time: the library's "morph_*" kernel timers (HIP events on the context's stream around each launch of one call), warmed up first.
The stack is borrowed (pnr_set_volume_device); pnr_morph_reconstruct never writes it; the result stays on the device (volume=False:
summary only).  A tile visit stages the state of its (TX + 2) (TY + 2) (TZ + 2) cells and the mask of its TX TY TZ voxels and writes at most
TX TY TZ bytes back: that is the traffic counted.  There is no parent to compare with: the project had no reconstruction before."""
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
import morph_ref  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N = S ** 3
REPS = 3
PARTS = ("init", "compact", "relax", "finish")
TZ, TY, TX = morph_ref.tile()
TILES = -(-S // TX) * -(-S // TY) * -(-S // TZ)
VISIT_BYTES = (TX + 2) * (TY + 2) * (TZ + 2) + 2 * TX * TY * TZ
img = synth.synth_torch(S, S, S, seed=3, zdist=2.0)
torch.cuda.synchronize()
ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), zdist=2.0), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
ctx.set_profiling(True)
print(f"pnr_morph_reconstruct on the {S}^3 u8 bench stack ({N / 1e9:.3f} G voxels), tiles of {TX} x {TY} x {TZ}: {TILES} tiles")


def once(op, h, conn):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info, _ = ctx.morph_reconstruct(op=op, h=h, connectivity=conn, volume=False)
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("morph_" + p) for p in PARTS}, ctx.kernel_ms("morph")[0], wall


def report(name, op, h, conn):
    once(op, h, conn)  # warm-up: code objects, first allocations
    runs = [once(op, h, conn) for _ in range(REPS)]
    info = runs[0][0]
    print(f"\n{name}: op = {op}, h = {h}, C = {info['connectivity']}, {REPS} repeats after a warm-up")
    print(f"changed {info['n_changed']} of {info['n_vox']} voxels, non-zero {info['n_nonzero']}, sum {info['sum_in']} -> {info['sum_out']}, max delta {info['max_delta']}")
    print(f"{'part':<10} {'device ms med':>14} {'min':>10} {'max':>10} {'launches':>9}")
    for p in PARTS:
        ms = np.array([r[1][p][0] for r in runs])
        print(f"{p:<10} {float(np.median(ms)):>14.3f} {ms.min():>10.3f} {ms.max():>10.3f} {runs[0][1][p][1]:>9}")
    tot = np.array([r[2] for r in runs])
    walls = np.array([r[3] for r in runs])
    print(f"{'all':<10} {float(np.median(tot)):>14.3f} {tot.min():>10.3f} {tot.max():>10.3f}   call wall ms (host loop, no download) {float(np.median(walls)):.3f}")
    for k, r in enumerate(runs):  # (the visits of a run depend on what its tiles saw of one another inside a launch)
        rounds, visits, relax = r[0]["rounds"], r[0]["tile_visits"], r[1]["relax"][0]
        staged = visits * VISIT_BYTES
        print(f"run {k}: rounds {rounds}, tile visits {visits} = {visits / (rounds * TILES):.4f} of rounds x tiles ({visits / TILES:.2f} visits per tile), staged "
              f"{staged / 1e9:.2f} GB = {staged / (3 * N):.2f} x the floor of 3 N, {staged / 1e9 / max(relax, 1e-9) * 1e3:.0f} GB/s over the relaxation; the floor alone at "
              f"that rate: {3 * N / 1e9 / max(staged / 1e9 / max(relax, 1e-9) * 1e3, 1e-9) * 1e3:.3f} ms")
    sys.stdout.flush()


report("grey fill-holes, 3-D", "fill", 0, 6)
report("h-maxima", "hmax", 16, 26)
ctx.close()
