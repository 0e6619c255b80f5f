"""Device time of pnr_set_volume_u16 on 1024^3 u16 stacks built on the GPU, and the CLI's wall time on a 16-bit file against the
8-bit file of the same (mapped) stack.  On an MI355X:   python scripts/volume16_timing.py [size] > profiles/rNN_volume16_1024.txt

Device time: the library's "volume" kernel timer (HIP events on the context's stream around the kernels of one call), every case
warmed up first, the repeats alternating over the cases.  Bytes: what the kernels must move (u16 reads of every pass over the
samples they touch, the u8 write), so GB/s = bytes / device time.  Stacks:
  deep12   the bench stack (tests/synth.py seed 3) as a 12-bit stack: 15 * u8 + 40 + noise in [0, 15)
  dark12   12-bit, a dark background (100 + exponential(60)) with 2 % bright voxels: the worst case of the histograms' LDS counters
  uniform  16-bit uniform noise
  rgb3     deep12, dark12, uniform interleaved (3 samples per voxel), channel 1 (dark12)"""
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
g = torch.Generator(device="cuda").manual_seed(11)
img8 = synth.synth_torch(S, S, S, seed=3)
deep = (img8.to(torch.int32) * 15 + 40 + torch.randint(0, 15, (S, S, S), device="cuda", generator=g, dtype=torch.int32)).to(torch.int16)
u = torch.rand((S, S, S), device="cuda", generator=g)
dark = (100 - 60 * torch.log1p(-u)).clamp(max=4095)
dark = torch.where(torch.rand((S, S, S), device="cuda", generator=g) < 0.02, torch.randint(0, 4096, (S, S, S), device="cuda", generator=g).float(), dark)
dark = dark.to(torch.int16)
del u
uniform = torch.randint(-32768, 32768, (S, S, S), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
rgb = torch.stack([deep, dark, uniform], dim=-1).contiguous()
torch.cuda.synchronize()

ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6)), 0)
ctx.set_profiling(True)
SAT = {"saturate": (0, 0.35)}
# name, tensor, nchan, channel, window, bytes moved
cases = [("minmax deep12", deep, 1, 0, None, 5 * N), ("minmax dark12", dark, 1, 0, None, 5 * N),
         ("saturated deep12", deep, 1, 0, SAT, 7 * N), ("saturated dark12", dark, 1, 0, SAT, 7 * N), ("saturated uniform", uniform, 1, 0, SAT, 7 * N),
         ("fixed deep12", deep, 1, 0, (40, 3000), 3 * N), ("minmax rgb3 ch1", rgb, 3, 1, None, 13 * N), ("saturated rgb3 ch1", rgb, 3, 1, SAT, 19 * N)]


def once(t, nchan, ch, win):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    ctx.set_volume_device(t.data_ptr(), (S, S, S), dtype=np.uint16, nchan=nchan, channel=ch, window=win)
    wall = time.perf_counter() - t0
    ms, n = ctx.kernel_ms("volume")
    return ms, n, wall * 1e3


for name, t, nchan, ch, win, _ in cases:  # warm-up: code objects, first touch of the owned volume
    once(t, nchan, ch, win)
res = {c[0]: [] for c in cases}
for rep in range(REPS):
    for name, t, nchan, ch, win, _ in (cases if rep % 2 == 0 else cases[::-1]):
        res[name].append(once(t, nchan, ch, win) + (ctx.window,))
print(f"pnr_set_volume_u16_device on {S}^3 u16 ({N / 1e9:.3f} G voxels), {REPS} repeats per case after a warm-up, alternating")
print(f"device time = the 'volume' kernel timer of one call; call wall = the host's clock around the call (+ window read-back)")
print(f"{'case':<22} {'launches':>8} {'device ms med':>14} {'min':>7} {'max':>7} {'GB moved':>9} {'GB/s (med)':>11} {'call wall ms':>13}  window")
for name, t, nchan, ch, win, nbytes in cases:
    r = res[name]
    ms = np.array([x[0] for x in r])
    wall = np.array([x[2] for x in r])
    med = float(np.median(ms))
    print(f"{name:<22} {r[0][1]:>8} {med:>14.3f} {ms.min():>7.3f} {ms.max():>7.3f} {nbytes / 1e9:>9.2f} {nbytes / 1e9 / (med / 1e3):>11.0f} "
          f"{float(np.median(wall)):>13.3f}  {r[0][3]}")
sys.stdout.flush()

# ---- CLI wall time: the 16-bit raw file against the 8-bit raw file of the mapped stack ([min, max] window), README parameters ----
ctx.set_volume_device(deep.data_ptr(), (S, S, S), dtype=np.uint16)
mapped = ctx.get_volume()
lo, hi = ctx.window
ctx.close()
p16, p8 = f"/tmp/pnr_v16_{S}.raw", f"/tmp/pnr_v8_{S}.raw"
deep.cpu().numpy().view(np.uint16).astype("<u2").tofile(p16)
mapped.tofile(p8)
del mapped, rgb, uniform, dark, deep, img8
torch.cuda.empty_cache()
cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
paras = ["2,4,6", "0", "5", "0.3", "3", "2", "200", "200", "2", "4", "1"]
runs = {"u16": [cli, "--raw-type", "u16", "-d", f"{S},{S},{S}", "-f", "advantra_func", "-i", p16, "-p", *paras],
        "u8": [cli, "-d", f"{S},{S},{S}", "-f", "advantra_func", "-i", p8, "-p", *paras]}
pat = re.compile(r"wall: load ([\d.]+) s, context \+ upload ([\d.]+) s, .* total ([\d.]+) s")
print(f"\nadvantra_cli on the {S}^3 stack (README parameters 2,4,6 0 5 0.3 3 2 200 200 2 4 1): 16-bit raw ({2 * N / 1e9:.2f} GB, window "
      f"[{lo}, {hi}]) vs the 8-bit raw of its mapped bytes ({N / 1e9:.2f} GB); two runs each, alternating")
print(f"{'file':<5} {'run':>3} {'load s':>7} {'context+upload s':>17} {'total s':>8} {'process wall s':>15}")
swc = {}
for rep in range(2):
    for k in (("u16", "u8") if rep == 0 else ("u8", "u16")):
        t0 = time.time()
        pr = subprocess.run(runs[k], capture_output=True, text=True)
        wall = time.time() - t0
        m = pat.search(pr.stdout)
        if pr.returncode != 0 or not m:
            print(pr.stdout[-2000:], pr.stderr[-2000:])
            sys.exit(1)
        print(f"{k:<5} {rep:>3} {float(m.group(1)):>7.3f} {float(m.group(2)):>17.3f} {float(m.group(3)):>8.3f} {wall:>15.3f}")
        swc[k] = open(runs[k][runs[k].index("-i") + 1] + "_Advantra.swc").read()
extra = f"#bits=16\n#window={lo},{hi}\n"
print("SWC of the 16-bit file = SWC of the 8-bit file apart from the two window lines:", swc["u16"].replace(extra, "") == swc["u8"])
for f in (p16, p8, p16 + "_Advantra.swc", p8 + "_Advantra.swc"):
    if os.path.exists(f):
        os.remove(f)
