"""Cost of the render (pnr_tree_coverage, advantra_cli --mask --coverage) on a trace of the bench stack.  On an MI355X:
    python scripts/render_timing.py [size] > profiles/rNN_render_1024.txt

Traces the size^3 bench stack (tests/synth.py seed 3, README parameters, every sorted seed) and reconstructs; renders the tree with the
radii the SWC would carry (SIG2RADIUS * the winning scale) on the traced volume and prints the "render" kernel time of one
pnr_tree_coverage (the library's kernel timer, median of REPS calls after a warm-up) split into scatter and finish, the work items,
the (voxel, segment) tests and tests per second, n_tree and the coverage, the bytes of the finish pass against its time, and the wall
time of advantra_cli on the stack with and without --mask --coverage, in alternating pairs."""
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
SIG2RADIUS = 1.5

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
radius = (np.float32(SIG2RADIUS) * tree["sig"][1:]).astype(np.float32)
n = len(xyz)
N = S ** 3

# the context that traced (Frangi state and all) renders
ctx.set_profiling(True)
for what, kw in (("coverage", {}), ("coverage + mask + residual + per node", dict(per_node=True, mask=True, residual=True))):
    ctx.tree_coverage(xyz, radius, par, zscale=ZDIST, **kw)  # warm-up
    ms = []
    for _ in range(REPS):
        ctx.reset_kernel_ms()
        t0 = time.perf_counter()
        cov = ctx.tree_coverage(xyz, radius, par, zscale=ZDIST, **kw)
        wall = 1e3 * (time.perf_counter() - t0)
        (ks, ls), (kf, lf) = ctx.kernel_ms("render_scatter"), ctx.kernel_ms("render_finish")
        ms.append((ks + kf, ks, kf, ls, lf, wall))
    k, ks, kf, ls, lf, wall = sorted(ms)[len(ms) // 2]
    items, pairs = ctx.get_option("render_items"), ctx.get_option("render_pairs")
    # the finish pass reads 4 N label bytes and N volume bytes (the sum before it: N more) and writes N per mask / residual
    fbytes = N * (4 + 1 + 1 + (2 if kw else 0))
    print(f"{what}: {n} nodes, {items} items, {pairs:.4g} pair tests; 'render' kernels {k:.3f} ms = scatter {ks:.3f} ms in {ls} launches + finish {kf:.3f} ms in {lf} "
          f"launches (all {REPS}: {', '.join(f'{m[0]:.3f}' for m in ms)}); {pairs / (ks * 1e-3):.4g} pair tests/s; finish {fbytes / 2 ** 30:.2f} GiB = "
          f"{fbytes / (kf * 1e-3) / 1e12:.2f} TB/s; call wall {wall:.2f} ms")
print(f"n_tree {cov['n_tree']} of {cov['n_vox']} voxels, threshold {cov['thr_used']}, covered {cov['covered']:.4f}, on signal {cov['on_signal']:.4f}, "
      f"intensity {cov['covered_intensity']:.4f}")
ctx.close()

with tempfile.TemporaryDirectory() as d:
    raw = os.path.join(d, "stack.raw")
    img.cpu().numpy().tofile(raw)
    del img
    torch.cuda.empty_cache()
    cli = os.path.join(R, "pnr_amd", "host", "advantra_cli")
    paras = f"2,4,6 0 5 0.3 3 2 200 200 {ZDIST:g} 4 1".split()
    walls = {(): [], ("--mask", os.path.join(d, "mask.raw"), "--coverage"): []}
    for _ in range(2):  # alternating
        for flags in walls:
            t0 = time.perf_counter()
            pr = subprocess.run([cli, "-d", f"{S},{S},{S}", *flags, "-f", "advantra_func", "-i", raw, "-p", *paras], capture_output=True, text=True)
            walls[flags].append(time.perf_counter() - t0)
            if pr.returncode != 0:
                print(pr.stderr[-2000:])
                sys.exit(1)
            if flags:
                print([ln for ln in pr.stdout.splitlines() if ln.startswith("render...")])
    for flags, w in walls.items():
        print(f"advantra_cli {'--mask --coverage' if flags else '(no render)'}: wall {', '.join(f'{x:.3f}' for x in w)} s")
