"""Device time of pnr_filter_volume per stage on a SIZE^3 u8 stack built on the GPU, and the CLI's wall time on that stack with and
without the pre-filter flags.  On an MI355X:   python scripts/filter_timing.py [size] > profiles/filter_SIZE.txt

Device time: the library's "filter" kernel timer (HIP events on the context's stream around the kernels of one call), every case
warmed up first, the repeats alternating over the cases.  The stack is borrowed anew for every call (pnr_set_volume_device), so each
call filters the same bytes.  Floor: the passes of the stage times one read and one write of the volume (2 N bytes per pass; the
subtracting pass reads the volume once more), so GB/s = floor bytes / device time.  Stack: the bench stack (tests/synth.py seed 3)
with a background pedestal and shot noise."""
import os
import re
import subprocess
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


def passes(R_):
    return 6 if int(np.float32(R_) / np.float32(ZD)) else 4


# name, median, tophat, floor bytes
cases = [("median 2d", 2, 0, 2 * N), ("median 3d", 3, 0, 2 * N)]
cases += [(f"top-hat R={r}", 0, r, (2 * passes(r) + 1) * N) for r in (4, 16, 64)]
cases += [("median 3d + R=16", 3, 16, (2 + 2 * passes(16) + 1) * N)]


def once(median, tophat):
    ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    ctx.filter_volume(median, tophat)
    wall = time.perf_counter() - t0
    ms, n = ctx.kernel_ms("filter")
    return ms, n, wall * 1e3


for name, m, t, _ in cases:  # warm-up: code objects, first allocations
    once(m, t)
res = {c[0]: [] for c in cases}
for rep in range(REPS):
    for name, m, t, _ in (cases if rep % 2 == 0 else cases[::-1]):
        res[name].append(once(m, t))
print(f"pnr_filter_volume on {S}^3 u8 ({N / 1e9:.3f} G voxels, zdist {ZD}), {REPS} repeats per case after a warm-up, alternating")
print("device time = the 'filter' kernel timer of one call; call wall = the host's clock around the call (allocation, kernels, free)")
print(f"{'case':<18} {'launches':>8} {'device ms med':>14} {'min':>8} {'max':>8} {'floor GB':>9} {'GB/s (med)':>11} {'call wall ms':>13}")
for name, m, t, nbytes in cases:
    r = res[name]
    ms = np.array([x[0] for x in r])
    wall = np.array([x[2] for x in r])
    med = float(np.median(ms))
    print(f"{name:<18} {r[0][1]:>8} {med:>14.3f} {ms.min():>8.3f} {ms.max():>8.3f} {nbytes / 1e9:>9.2f} {nbytes / 1e9 / (med / 1e3):>11.0f} {float(np.median(wall)):>13.3f}")
sys.stdout.flush()
ctx.close()

# ---- CLI wall time: the same raw file with and without the flags, README parameters, alternating pairs ----
path = f"/tmp/pnr_filter_{S}.raw"
img.cpu().numpy().tofile(path)
del img
torch.cuda.empty_cache()
cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
paras = ["2,4,6", "0", "5", "0.3", "3", "2", "200", "200", "2", "4", "1"]
tail = ["-d", f"{S},{S},{S}", "-f", "advantra_func", "-i", path, "-p", *paras]
runs = {"plain": [cli, *tail], "filtered": [cli, "--median", "3d", "--subtract-background", "16", "--timing", *tail]}
pat = re.compile(r"wall: load ([\d.]+) s, context \+ upload ([\d.]+) s, .* total ([\d.]+) s")
fpat = re.compile(r"\[pnr host\] filter: ([\d.]+) s, kernels ([\d.]+) ms")
print(f"\nadvantra_cli on the {S}^3 stack (README parameters 2,4,6 0 5 0.3 3 2 200 200 2 4 1), plain vs --median 3d --subtract-background 16; "
      "three pairs, alternating (the two runs trace different bytes: the totals differ by more than the filter)")
print(f"{'run':<9} {'pair':>4} {'load s':>7} {'context+upload(+filter) s':>26} {'filter call s':>14} {'filter kernels ms':>18} {'total s':>8} {'process wall s':>15}")
for rep in range(3):
    for k in (("plain", "filtered") if rep % 2 == 0 else ("filtered", "plain")):
        t0 = time.time()
        pr = subprocess.run(runs[k], capture_output=True, text=True)
        wall = time.time() - t0
        m = pat.search(pr.stdout)
        if pr.returncode != 0 or not m:
            print(pr.stdout[-2000:], pr.stderr[-2000:])
            sys.exit(1)
        f = fpat.search(pr.stderr)
        print(f"{k:<9} {rep:>4} {float(m.group(1)):>7.3f} {float(m.group(2)):>26.3f} {(f.group(1) if f else '-'):>14} {(f.group(2) if f else '-'):>18} "
              f"{float(m.group(3)):>8.3f} {wall:>15.3f}")
for f in (path, path + "_Advantra.swc"):
    if os.path.exists(f):
        os.remove(f)
