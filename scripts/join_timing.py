"""Cost of the join (pnr_join_trees, advantra_cli --join) on a trace of the bench stack.  On an MI355X:
    python scripts/join_timing.py [size] > profiles/rNN_join_1024.txt

Traces the size^3 bench stack (tests/synth.py seed 3, README parameters, every sorted seed) and reconstructs; prints the forest's size,
the "join" kernel time of one nearest-other pass over the input trees (the library's kernel timer, median of REPS calls after a
warm-up) with its (point, target) pairs per second, the kernel time, rounds and wall time of the whole join at gap 0 and at GAP, and
the wall time of advantra_cli on the stack with and without --join."""
import os
import subprocess
import sys
import tempfile
import time
import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import synth  # noqa: E402
import pnr_amd  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS = 5
ZDIST = 2.0
GAP = 10.0

img = synth.synth_torch(S, S, S, seed=3)
torch.cuda.synchronize()
ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), np_=200, ni=200, zdist=ZDIST), 0)
ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
t0 = time.time()
res = pnr_amd.advantra.run_pipeline(ctx, None)
print(f"{len(res['seeds'])} seeds, {res['ntraces']} traces, {len(res['nodes']) - 1} graph nodes, {len(res['tree']) - 1} tree nodes, pipeline {time.time() - t0:.2f} s", flush=True)
tree, parent = res["tree"], res["parent"]
xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:]  # without the dummy node
par = np.where(parent[1:] > 0, parent[1:] - 1, -1).astype(np.int32)
n = len(xyz)

# the context that traced (Frangi state and all) does the join
ctx.set_profiling(True)
label = np.full(n, -1, np.int32)
for i in range(n):  # the input trees: every node takes the index of its root as its label (each chain is walked once)
    path, v = [], i
    while label[v] < 0 and par[v] >= 0:
        path.append(v)
        v = par[v]
    label[v] = label[v] if label[v] >= 0 else v
    if path:
        label[path] = label[v]
scaled = xyz.copy()
scaled[:, 2] *= np.float32(ZDIST)
print(f"forest: {n} nodes in {len(np.unique(label))} trees (zscale {ZDIST})")
ctx.nearest_other(scaled, label)  # warm-up
ms = []
for _ in range(REPS):
    ctx.reset_kernel_ms()
    t0 = time.perf_counter()
    ctx.nearest_other(scaled, label)
    wall = 1e3 * (time.perf_counter() - t0)
    k, launches = ctx.kernel_ms("join")
    ms.append((k, wall, launches))
k, wall, launches = sorted(ms)[len(ms) // 2]
pairs = n * n
print(f"one pass: {n} x {n} = {pairs:.4g} pairs; 'join' kernels {k:.3f} ms in {launches} launches (all {REPS}: {', '.join(f'{m[0]:.3f}' for m in ms)}); "
      f"{pairs / (k * 1e-3):.4g} pairs/s; call wall {wall:.2f} ms")
for gap in (0.0, GAP):
    ctx.join_trees(xyz, par, zscale=ZDIST, gap=gap)  # warm-up
    ms = []
    for _ in range(REPS):
        ctx.reset_kernel_ms()
        t0 = time.perf_counter()
        po, order, comp, bridges, cnt = ctx.join_trees(xyz, par, zscale=ZDIST, gap=gap, counts=True)
        wall = 1e3 * (time.perf_counter() - t0)
        ms.append((ctx.kernel_ms("join")[0], wall))
    k, wall = sorted(ms)[len(ms) // 2]
    rounds = max(cnt["rounds"], 1)
    print(f"join gap {gap:g}: {cnt['trees_in']} -> {cnt['trees_out']} trees, {len(bridges)} bridges (longest {float(bridges['d'].max()) if len(bridges) else 0:.3f}), {cnt['rounds']} rounds; "
          f"'join' kernels {k:.3f} ms = {k / rounds:.3f} ms per round, {rounds * pairs / (k * 1e-3):.4g} pairs/s; call wall {wall:.2f} ms "
          f"(all {REPS}: {', '.join(f'{m[0]:.3f}/{m[1]:.2f}' for m in ms)})")
ctx.close()

with tempfile.TemporaryDirectory() as d:
    raw = os.path.join(d, "stack.raw")
    img.cpu().numpy().tofile(raw)
    del img
    torch.cuda.empty_cache()
    cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
    paras = f"2,4,6 0 5 0.3 3 2 200 200 {ZDIST:g} 4 1".split()
    walls = {(): [], ("--join", "0"): []}
    for _ in range(2):  # alternating
        for flags in walls:
            t0 = time.perf_counter()
            pr = subprocess.run([cli, "-d", f"{S},{S},{S}", *flags, "-f", "advantra_func", "-i", raw, "-p", *paras], capture_output=True, text=True)
            walls[flags].append(time.perf_counter() - t0)
            if pr.returncode != 0:
                print(pr.stderr[-2000:])
                sys.exit(1)
            if flags:
                print([ln for ln in pr.stdout.splitlines() if ln.startswith("join...")])
    for flags, w in walls.items():
        print(f"advantra_cli {' '.join(flags) or '(no --join)'}: wall {', '.join(f'{x:.3f}' for x in w)} s")
