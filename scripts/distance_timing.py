"""Cost of the tree distance (pnr_tree_distance, advantra_cli --distance) on two traces of the bench stack.  On an MI355X:
    python scripts/distance_timing.py [size] > profiles/rNN_distance_1024.txt

Traces the size^3 bench stack (tests/synth.py seed 3, README parameters, every sorted seed) twice with two rng_seed values and
reconstructs; prints the tree sizes, the "distance" kernel time of either direction (the library's kernel timer, median of REPS
calls after a warm-up), the (point, segment) pairs per second, the result, and the wall time of advantra_cli --distance on the two
SWC files."""
import json
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
from pnr_amd import lib  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS = 5
ZDIST = 2.0
SEEDS = (42, 7)

img = synth.synth_torch(S, S, S, seed=3)
torch.cuda.synchronize()
trees = []
for seed in SEEDS:
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4, 6), np_=200, ni=200, zdist=ZDIST, rng_seed=seed), 0)
    ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
    t0 = time.time()
    res = pnr_amd.advantra.run_pipeline(ctx, None)
    print(f"rng_seed {seed}: {len(res['seeds'])} seeds, {res['ntraces']} traces, {len(res['nodes']) - 1} graph nodes, {len(res['tree']) - 1} tree nodes, "
          f"pipeline {time.time() - t0:.2f} s", flush=True)
    trees.append((res["tree"], res["parent"]))
    ctx.close()
del img
torch.cuda.empty_cache()


def plain(tree, parent):
    """positions and parent indices without the dummy node"""
    return np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:], np.where(parent[1:] > 0, parent[1:] - 1, -1).astype(np.int32)


(xa, pa), (xb, pb) = plain(*trees[0]), plain(*trees[1])
ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
ctx.set_profiling(True)
sides = {}
for name, (x, p) in (("A", (xa, pa)), ("B", (xb, pb))):
    pts, _ = lib.tree_sample(x, p, ZDIST, 1)
    a = x.copy()
    a[:, 2] *= np.float32(ZDIST)
    sides[name] = (pts, a, a[np.where(p < 0, np.arange(len(p)), p)])
    print(f"tree {name}: {len(x)} nodes = segments, {len(pts)} sample points at step 1 (zscale {ZDIST})")
for src, dst in (("A", "B"), ("B", "A")):
    pts, (_, a, b) = sides[src][0], sides[dst]
    ctx.point_segment_distance(pts, a, b)  # warm-up
    ms = []
    for _ in range(REPS):
        ctx.reset_kernel_ms()
        t0 = time.perf_counter()
        ctx.point_segment_distance(pts, a, b)
        wall = 1e3 * (time.perf_counter() - t0)
        k, launches = ctx.kernel_ms("distance")
        ms.append((k, wall, launches))
    k, wall, launches = sorted(ms)[len(ms) // 2]
    pairs = len(pts) * len(a)
    print(f"{src} -> {dst}: {len(pts)} points x {len(a)} segments = {pairs:.4g} pairs; 'distance' kernels {k:.3f} ms in {launches} launches "
          f"(all {REPS}: {', '.join(f'{m[0]:.3f}' for m in ms)}); {pairs / (k * 1e-3):.4g} pairs/s; call wall {wall:.2f} ms")
t0 = time.perf_counter()
r = ctx.tree_distance(xa, pa, xb, pb, zscale=ZDIST)
print(f"tree_distance (both directions, sampling and sums on the host) {1e3 * (time.perf_counter() - t0):.2f} ms: {json.dumps(r)}")
ctx.close()

with tempfile.TemporaryDirectory() as d:
    fa, fb = os.path.join(d, "a.swc"), os.path.join(d, "b.swc")
    pnr_amd.write_swc_tree(fa, *trees[0])
    pnr_amd.write_swc_tree(fb, *trees[1])
    cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        pr = subprocess.run([cli, "--distance", fa, fb, "--zscale", str(ZDIST)], capture_output=True, text=True)
        walls.append(time.perf_counter() - t0)
        if pr.returncode != 0:
            print(pr.stderr[-2000:])
            sys.exit(1)
    print(f"advantra_cli --distance a.swc b.swc --zscale {ZDIST}: wall {', '.join(f'{w:.3f}' for w in walls)} s (process start, context, two files of %.3f "
          f"coordinates); {pr.stdout.strip()}")
