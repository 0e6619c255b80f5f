"""Where the pruning on the GPU (Context.prune_tree) overtakes the sequential host pass (prune_tree_host), and what it spends its time on.
On an MI355X:   python scripts/prune_timing.py [size] > profiles/r18_prune_SIZE.txt

Inputs: generated forests of n = 10^4, 10^5, 10^6 and 10^7 nodes (8 trees; a node grows from the previous one with probability 0.98,
else from a random earlier one, by one of the 26 lattice steps -- tests/prune_ref.py's generator with the positions summed by pointer
doubling in numpy -- and the indices permuted), and the skeleton tree of the SIZE^3 bench stack (tests/synth.py seed 3; --skeleton
--swc's way: pnr_skeletonize, pnr_skeleton_forest, pnr_join_reroot at the thickest voxel, radius = the distance transform).

Per input, with min_length = 5, radius_factor = 1.5, min_tree = 10: the "prune" kernel timer of one call (HIP events on the context's
stream around its launches), both round counts, the wall time of Context.prune_tree -- argument checks with the cycle check, staging,
launches, read-backs --, and the wall time of prune_tree_host on the same arrays, one thread.  Every case is warmed up once; the
median of REPS calls, GPU and host alternating.  Every step has a time limit of its own (SIGALRM): a step that overruns ends the script."""
import os
import signal
import sys
import time
import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import synth  # noqa: E402
import prune_ref  # noqa: E402
import pnr_amd  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REPS = 5
OPTS = dict(zscale=2, min_length=5, radius_factor=1.5, min_tree=10)


class limit:
    """a time limit for one step"""
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"time limit of {self.seconds} s: {self.what}"))
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def forest(n, trees=8, chain=0.98, seed=1):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    parent = np.where(rng.random(n) < chain, i - 1, (rng.random(n) * i).astype(np.int64))
    parent[:trees] = -1
    pos = prune_ref.STEPS[rng.integers(0, 26, n)].astype(np.float64)
    pos[:trees] = rng.integers(0, 64, (trees, 3))
    anc = parent.copy()
    while (anc >= 0).any():  # pos = the sum of the steps down from the root, by pointer doubling
        live = anc >= 0
        pos[live] += pos[anc[live]]
        anc[live] = anc[anc[live]]
    new = rng.permutation(n)
    xyz, par = np.empty((n, 3), np.float32), np.empty(n, np.int32)
    xyz[new] = pos
    par[new] = np.where(parent >= 0, new[np.maximum(parent, 0)], -1)
    radius = np.empty(n, np.float32)
    radius[new] = rng.integers(1, 5, n)
    return xyz, radius, par


def skeleton_tree(ctx):
    img = synth.synth_torch(S, S, S, seed=3, zdist=2.0)
    torch.cuda.synchronize()
    ctx.set_volume_device(img.data_ptr(), (S, S, S), keepalive=img)
    info, _, vox, _ = ctx.skeletonize(-1, volume=False)
    if len(vox) > 1 << 22:  # pnr_join_reroot takes 2^22 nodes
        print(f"skeleton {S}^3: {len(vox)} skeleton voxels at threshold {info['thr_used']}, more than the 2^22 nodes pnr_join_reroot takes: not timed")
        return None
    xyz = np.stack([vox % S, vox // S % S, vox // (S * S)], 1).astype(np.float32)
    _, _, d2 = ctx.distance_transform(info["thr_used"], 64, volume=False, points=xyz)
    edges = pnr_amd.skeleton_forest(vox, (S, S, S))
    parent, _, _ = pnr_amd.join_reroot(np.full(len(vox), -1, np.int32), edges, int(np.argmax(d2)))
    return xyz, np.sqrt(d2), parent


def depth_of(parent):
    d, anc = (parent >= 0).astype(np.int64), parent.astype(np.int64)
    while (anc >= 0).any():  # (pointer doubling, as for the positions)
        live = anc >= 0
        d[live] += d[anc[live]]
        anc[live] = anc[anc[live]]
    return int(d.max())


ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
ctx.set_profiling(True)
print(f"pruning: Context.prune_tree on one MI355X beside prune_tree_host on one CPU thread; {OPTS}; median of {REPS} calls after a warm-up")
print(f"{'input':<22} {'nodes':>9} {'depth':>7} {'removed':>8} {'up':>3} {'down':>4} {'launches':>8} {'kernels ms':>11} {'gpu call ms':>12} {'host ms':>9} {'host / gpu':>10}")
inputs = [(f"forest 1e{k}", lambda k=k: forest(10 ** k)) for k in (4, 5, 6, 7)] + [(f"skeleton {S}^3", lambda: skeleton_tree(ctx))]
for name, make in inputs:
    with limit(240, "building " + name):
        tree = make()
        if tree is None:
            continue
        xyz, radius, parent = tree
        depth = depth_of(parent)
    with limit(240, "timing " + name):
        want = pnr_amd.prune_tree_host(xyz, radius, parent, **OPTS)
        got = ctx.prune_tree(xyz, radius, parent, **OPTS)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:])), name
        kernels, gpu, host = [], [], []
        for _ in range(REPS):
            ctx.reset_kernel_ms()
            t0 = time.perf_counter()
            info = ctx.prune_tree(xyz, radius, parent, **OPTS)[0]
            t1 = time.perf_counter()
            pnr_amd.prune_tree_host(xyz, radius, parent, **OPTS)
            t2 = time.perf_counter()
            kernels.append(ctx.kernel_ms("prune"))
            gpu.append(1e3 * (t1 - t0))
            host.append(1e3 * (t2 - t1))
        g, h = float(np.median(gpu)), float(np.median(host))
        print(f"{name:<22} {len(parent):>9} {depth:>7} {info['n_removed']:>8} {info['rounds_up']:>3} {info['rounds_down']:>4} {kernels[0][1]:>8} "
              f"{float(np.median([k[0] for k in kernels])):>11.3f} {g:>12.3f} {h:>9.3f} {h / g:>10.2f}", flush=True)
ctx.close()
