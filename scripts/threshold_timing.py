"""Device time of the two threshold kernels on the SIZE^3 u8 bench stack built on the GPU, each beside what the tree had before them.
On an MI355X:   python scripts/threshold_timing.py [size] > profiles/r17_threshold_SIZE.txt

  "threshold" (pnr_auto_threshold: the 256-bin histogram, one read of N bytes) beside the byte-sum pass that "thr = -1" costs
  (the "components_threshold" timer of pnr_label_components with thr = -1: vol_sum alone, also one read of N bytes);
  "local_threshold" (pnr_local_threshold: three passes per slab) at R = 8 and 32 beside the top-hat of the same R ("filter": six passes).

Device time: the library's kernel timers (HIP events on the context's stream around the kernels of one call), every case warmed up
first, the repeats alternating over the cases.  The stack is borrowed (pnr_set_volume_device) anew for every filter call, so each call
works on the same bytes.  Floors: N bytes read for the histogram and the byte sum; 2 N for the local threshold (N read, N written; its
structure moves 21 N, threshold.hip) and 13 N for the six in-place passes of the top-hat.  Stack: the bench stack (tests/synth.py seed 3)
with a background pedestal and shot noise."""
import os
import sys
import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import synth  # noqa: E402
import pnr_amd  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N = S ** 3
REPS = 10
ZD = 2.0
g = torch.Generator(device="cuda").manual_seed(11)
img = synth.synth_torch(S, S, S, seed=3, zdist=ZD).to(torch.int16)
for z in range(0, S, 64):  # pedestal 20 + noise in [0, 24) + 1 % salt, in slabs (bounded temporaries)
    sl = img[z:z + 64]
    sl += 20 + torch.randint(0, 24, sl.shape, device="cuda", generator=g, dtype=torch.int16)
    sl[torch.rand(sl.shape, device="cuda", generator=g) < 0.01] = 255
img = img.clamp_(0, 255).to(torch.uint8)
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), zdist=ZD), 0)
ctx.set_profiling(True)


def borrow():
    ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)


def timed(group, call):
    borrow()
    ctx.reset_kernel_ms()
    call()
    return ctx.kernel_ms(group)


# name, timer group, the call, floor bytes
cases = [("histogram (otsu)", "threshold", lambda: ctx.auto_threshold("otsu"), N),
         ("byte sum (thr = -1)", "components_threshold", lambda: ctx.label_components(thr=-1, labels=False, cap=0), N)]
for r in (8, 32):
    cases.append((f"local threshold R={r}", "local_threshold", lambda r=r: ctx.local_threshold(r, 5, 260, volume=False), 2 * N))
    cases.append((f"top-hat R={r}", "filter", lambda r=r: ctx.filter_volume(0, r), 13 * N))

for _, group, call, _ in cases:  # warm-up: code objects, first allocations
    timed(group, call)
res = {c[0]: [] for c in cases}
for rep in range(REPS):
    for name, group, call, _ in (cases if rep % 2 == 0 else cases[::-1]):
        res[name].append(timed(group, call))
borrow()
thr = {m: ctx.auto_threshold(m, 0, ppm) for m, ppm in (("mean", None), ("otsu", None), ("triangle", None), ("top", 10000))}
print(f"thresholds on the {S}^3 u8 bench stack ({N / 1e9:.3f} G voxels, zdist {ZD}), {REPS} repeats per case after a warm-up, alternating")
print("device time = the named kernel timer of one call")
print("thr / share kept: " + ", ".join(f"{m} {i['thr']} / {i['n_fg'] / N:.4f}" for m, i in thr.items()))
print(f"{'case':<24} {'timer':<22} {'launches':>8} {'device ms med':>14} {'min':>8} {'max':>8} {'floor GB':>9} {'floor GB/s (med)':>17}")
for name, group, _, nbytes in cases:
    r = res[name]
    ms = np.array([x[0] for x in r])
    med = float(np.median(ms))
    print(f"{name:<24} {group:<22} {r[0][1]:>8} {med:>14.3f} {ms.min():>8.3f} {ms.max():>8.3f} {nbytes / 1e9:>9.2f} {nbytes / 1e9 / (med / 1e3):>17.0f}")
med = {name: float(np.median([x[0] for x in res[name]])) for name in res}
print(f"histogram / byte sum: {med['histogram (otsu)'] / med['byte sum (thr = -1)']:.2f} x")
for r in (8, 32):
    print(f"local threshold / top-hat at R={r}: {med[f'local threshold R={r}'] / med[f'top-hat R={r}']:.2f} x")
ctx.close()
