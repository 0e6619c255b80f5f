"""Device time of pnr_label_components per phase on the SIZE^3 bench stack (thr = -1, 26-connected), the component count, the achieved
bytes/s against the algorithmic bytes of DESIGN.md, and the CLI's wall time on that stack with and without --despeckle.
On an MI355X:   python scripts/components_timing.py [size] > profiles/components_SIZE.txt

Device time: the library's "components_*" kernel timers (HIP events on the context's stream around each kernel of one call), warmed
up first.  The stack is borrowed (pnr_set_volume_device); label_components never writes it.  Algorithmic bytes per voxel: threshold 1
(V), local 5 (V, the link written), merge 4 (the links), flatten 8 (the links read and rewritten), number 4, stats 5 (link, V),
finish 8 (link read, label written): 35 in all, the N x 4 label download not counted.  If scipy is present, the CPU time of
scipy.ndimage.label on the same foreground goes beside them as context only."""
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
REPS = 5
ZD = 2.0
PHASES = (("threshold", 1), ("local", 5), ("merge", 4), ("flatten", 8), ("number", 4), ("stats", 5), ("finish", 8))
img = synth.synth_torch(S, S, S, seed=3, zdist=ZD)
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), zdist=ZD), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
ctx.set_profiling(True)


def once(labels):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    info, lab, comps = ctx.label_components(-1, 26, labels=labels, cap=0)
    wall = (time.perf_counter() - t0) * 1e3
    return info, {p: ctx.kernel_ms("components_" + p)[0] for p, _ in PHASES}, ctx.kernel_ms("components")[0], wall


once(False)  # warm-up: code objects, first allocations
runs = [once(False) for _ in range(REPS)]
info = runs[0][0]
print(f"pnr_label_components on {S}^3 u8 ({N / 1e9:.3f} G voxels), thr = -1 (used: {info['thr_used']}), 26-connected, {REPS} repeats after a warm-up")
print(f"foreground {info['n_fg']} voxels, {info['n_comp']} components, largest {info['largest']}")
print(f"{'phase':<10} {'device ms med':>14} {'min':>8} {'max':>8} {'bytes/voxel':>12} {'GB/s (med)':>11}")
for p, b in PHASES:
    ms = np.array([r[1][p] for r in runs])
    med = float(np.median(ms))
    rate = b * N / 1e9 / (med / 1e3) if med > 0 else 0.0
    print(f"{p:<10} {med:>14.3f} {ms.min():>8.3f} {ms.max():>8.3f} {b:>12} {rate:>11.0f}")
tot = np.array([r[2] for r in runs])
walls = np.array([r[3] for r in runs])
print(f"{'all':<10} {float(np.median(tot)):>14.3f} {tot.min():>8.3f} {tot.max():>8.3f} {sum(b for _, b in PHASES):>12} "
      f"{sum(b for _, b in PHASES) * N / 1e9 / (float(np.median(tot)) / 1e3):>11.0f}   call wall ms (no label download) {float(np.median(walls)):.3f}")
_, _, _, wall_lab = once(True)
print(f"with the label volume downloaded ({4 * N / 1e9:.2f} GB): call wall {wall_lab:.3f} ms")
sys.stdout.flush()
ctx.close()
host = img.cpu().numpy()
try:
    from scipy import ndimage
    t0 = time.perf_counter()
    _, n = ndimage.label(host >= info["thr_used"], ndimage.generate_binary_structure(3, 3))
    print(f"context only: scipy.ndimage.label on the CPU, the same foreground: {time.perf_counter() - t0:.2f} s, {n} components")
except ImportError:
    print("context only: scipy is not installed, no CPU time")

# ---- CLI wall time: the same raw file with and without --despeckle, README parameters, alternating pairs ----
path = f"/tmp/pnr_components_{S}.raw"
host.tofile(path)
del img, host
torch.cuda.empty_cache()
cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
paras = ["2,4,6", "0", "5", "0.3", "3", "2", "200", "200", "2", "4", "1"]
tail = ["-d", f"{S},{S},{S}", "-f", "advantra_func", "-i", path, "-p", *paras]
runs = {"plain": [cli, *tail], "despeckle": [cli, "--despeckle", "30", "--timing", *tail]}
pat = re.compile(r"wall: load ([\d.]+) s, context \+ upload ([\d.]+) s, .* total ([\d.]+) s")
dpat = re.compile(r"\[pnr host\] despeckle: ([\d.]+) s")
print(f"\nadvantra_cli on the {S}^3 stack (README parameters 2,4,6 0 5 0.3 3 2 200 200 2 4 1), plain vs --despeckle 30; three pairs, alternating")
print(f"{'run':<10} {'pair':>4} {'load s':>7} {'context+upload(+despeckle) s':>29} {'despeckle call s':>17} {'total s':>8} {'process wall s':>15}")
for rep in range(3):
    for k in (("plain", "despeckle") if rep % 2 == 0 else ("despeckle", "plain")):
        t0 = time.time()
        pr = subprocess.run(runs[k], capture_output=True, text=True)
        wall = time.time() - t0
        m = pat.search(pr.stdout)
        if pr.returncode != 0 or not m:
            print(pr.stdout[-2000:], pr.stderr[-2000:])
            sys.exit(1)
        d = dpat.search(pr.stderr)
        print(f"{k:<10} {rep:>4} {float(m.group(1)):>7.3f} {float(m.group(2)):>29.3f} {(d.group(1) if d else '-'):>17} {float(m.group(3)):>8.3f} {wall:>15.3f}")
for f in (path, path + "_Advantra.swc"):
    if os.path.exists(f):
        os.remove(f)
