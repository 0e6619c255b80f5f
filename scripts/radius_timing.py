"""Cost of advantra_cli --measure-radius on the 1024^3 bench stack (tests/synth.py seed 3, README parameters).  On an MI355X:
    python scripts/radius_timing.py [size] > profiles/rNN_radius_1024.txt

Records the "radius" device time (the library's kernel timer, from one --timing run), the node count, the distribution of k*, and the
CLI's wall time with and without --measure-radius in alternating pairs.  The run without the flag is the baseline: it is what the
CLI did before the flag existed (no radius kernel is launched, the SWC has the same bytes)."""
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

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
PAIRS = int(sys.argv[2]) if len(sys.argv) > 2 else 4
raw = f"/tmp/pnr_radius_{S}.raw"
synth.synth_torch(S, S, S, seed=3).cpu().numpy().tofile(raw)
torch.cuda.empty_cache()
cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
paras = ["2,4,6", "0", "5", "0.3", "3", "2", "200", "200", "2", "4", "1"]
tail = ["-d", f"{S},{S},{S}", "-f", "advantra_func", "-i", raw, "-p", *paras]
swc = raw + "_Advantra.swc"
pat = re.compile(r"wall: .* reconstruct ([\d.]+) s, write ([\d.]+) s \| total ([\d.]+) s")


def run(*flags):
    t0 = time.time()
    pr = subprocess.run([cli, *flags, *tail], capture_output=True, text=True)
    wall = time.time() - t0
    m = pat.search(pr.stdout)
    if pr.returncode != 0 or not m:
        print(pr.stdout[-2000:], pr.stderr[-2000:])
        sys.exit(1)
    return pr, float(m.group(3)), wall, open(swc).read()


run()  # warm-up: the file in the page cache, the code objects
pr, _, _, measured = run("--measure-radius", "--timing")
dev = re.search(r"\[pnr host\] radius: ([\d.]+) s, kernels ([\d.]+) ms in (\d+) launches", pr.stderr)
rows = [ln.split() for ln in measured.splitlines() if ln and ln[0] != "#"]
r = np.array([float(x[5]) for x in rows])
types = np.array([int(x[1]) for x in rows])
print(f"advantra_cli --measure-radius on the {S}^3 bench stack (README parameters {' '.join(paras)}; defaults: rel_pct 50, rmax 32, bg 1 permille)")
print(f"tree nodes {len(rows)} (soma-typed, not measured: {int((types == 1).sum())})")
print(f"radius stage (host clock: positions up, shell table built and uploaded, kernel, k back) {float(dev.group(1)) * 1e3:.3f} ms; "
      f"'radius' kernel timer {float(dev.group(2)):.3f} ms in {dev.group(3)} launch(es)")
vals, cnt = np.unique(r, return_counts=True)
print("radius column (0.5 = k* 0): " + ", ".join(f"{v:g}: {c}" for v, c in zip(vals, cnt)))
print(f"comment line: {[ln for ln in measured.splitlines() if ln.startswith('#radius=')]}")
print(f"\n{PAIRS} alternating pairs, CLI total (its own clock) and process wall, seconds")
print(f"{'pair':>4} {'plain total':>12} {'measured total':>15} {'plain wall':>11} {'measured wall':>14}")
tot = {"plain": [], "measured": []}
wl = {"plain": [], "measured": []}
plain_swc = None
for pair in range(PAIRS):
    order = ("plain", "measured") if pair % 2 == 0 else ("measured", "plain")
    for k in order:
        _, t, w, text = run(*(("--measure-radius",) if k == "measured" else ()))
        tot[k].append(t)
        wl[k].append(w)
        if k == "plain":
            assert plain_swc in (None, text)
            plain_swc = text
        else:
            assert text == measured
    print(f"{pair:>4} {tot['plain'][-1]:>12.3f} {tot['measured'][-1]:>15.3f} {wl['plain'][-1]:>11.3f} {wl['measured'][-1]:>14.3f}")
mp, mm = float(np.median(tot["plain"])), float(np.median(tot["measured"]))
print(f"median total: plain {mp:.3f} s, measured {mm:.3f} s ({(mm / mp - 1) * 100:+.1f} %); "
      f"median wall: plain {float(np.median(wl['plain'])):.3f} s, measured {float(np.median(wl['measured'])):.3f} s")
same = [a.split()[:5] + a.split()[6:] for a in plain_swc.splitlines() if a and a[0] != "#"] == [x[:5] + x[6:] for x in rows]
print("ids, types, coordinates and parents of the measured file = the plain file's:", same)
for f in (raw, swc):
    if os.path.exists(f):
        os.remove(f)
