"""Device time of pnr_distance_transform per kernel on the SIZE^3 bench stack (thr = -1, rmax = 64) and on an all-foreground stack of the
same size (thr = 0: every bounded scan of the y and z passes runs to rmax, the adversarial case), and the bytes per second of the whole
call against its floor: N bytes of V read and 4 N bytes of D2 written.
On an MI355X:   python scripts/edt_timing.py [size] > profiles/edt_SIZE.txt

Device time: the library's "edt_*" kernel timers (HIP events on the context's stream around each kernel of one call), warmed up first.
The stack is borrowed (pnr_set_volume_device); the call never writes it; D2 stays on the device (volume=False: summary only).  If scipy
is present, the CPU time of scipy.ndimage.distance_transform_edt on a 256^3 crop of the same foreground goes beside them for orientation
only."""
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

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = S ** 3
REPS = 5
ZD = 2.0
RMAX = 64
PHASES = ("threshold", "x", "y", "z", "stats", "sample")
img = synth.synth_torch(S, S, S, seed=3, zdist=ZD)
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), zdist=ZD), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
ctx.set_profiling(True)
pts = np.random.default_rng(1).uniform(0, S, (10000, 3)).astype(np.float32)


def once(thr):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info, _, _ = ctx.distance_transform(thr, RMAX, volume=False, points=pts)
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("edt_" + p)[0] for p in PHASES}, ctx.kernel_ms("edt")[0], wall


def report(name, thr):
    once(thr)  # warm-up: code objects, first allocations
    runs = [once(thr) for _ in range(REPS)]
    info = runs[0][0]
    print(f"{name}: thr = {thr} (used: {info['thr_used']}), rmax = {RMAX}, zdist = {ZD}, 10000 points, {REPS} repeats after a warm-up")
    print(f"foreground {info['n_fg']} of {info['n_vox']} voxels, capped {info['n_capped']}, d_max {info['d_max']:.3f} at {info['max_at']}")
    print(f"{'kernel':<10} {'device ms med':>14} {'min':>8} {'max':>8}")
    for p in PHASES:
        ms = np.array([r[1][p] for r in runs])
        print(f"{p:<10} {float(np.median(ms)):>14.3f} {ms.min():>8.3f} {ms.max():>8.3f}")
    tot = np.array([r[2] for r in runs])
    walls = np.array([r[3] for r in runs])
    med = float(np.median(tot))
    print(f"{'all':<10} {med:>14.3f} {tot.min():>8.3f} {tot.max():>8.3f}   floor N + 4 N = {5 * N / 1e9:.2f} GB -> {5 * N / 1e9 / (med / 1e3):.0f} GB/s"
          f"   call wall ms (no D2 download) {float(np.median(walls)):.3f}\n")
    sys.stdout.flush()
    return med, info


print(f"pnr_distance_transform on {S}^3 u8 ({N / 1e9:.3f} G voxels)")
bench, info = report("bench stack", -1)
full, _ = report("all foreground", 0)
print(f"all foreground / bench stack: {full / bench:.1f} x")
t0 = time.perf_counter()
ctx.distance_transform(-1, RMAX)
print(f"with D2 downloaded ({4 * N / 1e9:.2f} GB): call wall {(time.perf_counter() - t0) * 1e3:.1f} ms")
sys.stdout.flush()
ctx.close()
C = min(S, 256)
host = img[:C, :C, :C].cpu().numpy()
try:
    from scipy import ndimage
    t0 = time.perf_counter()
    d = ndimage.distance_transform_edt(host >= info["thr_used"], sampling=(ZD, 1, 1))
    print(f"orientation only: scipy.ndimage.distance_transform_edt on the CPU, a {C}^3 crop of the same foreground: {time.perf_counter() - t0:.2f} s, d_max {d.max():.3f}")
except ImportError:
    print("orientation only: scipy is not installed, no CPU time")
