"""Image classes the synthetic tubes of synth.py never produce (plain numpy, deterministic): inputs on which the analytic shortcuts
of hessian_tile, the survivor queue, the sparse J8 path of the seed extraction and the stable seed sort take other branches than on
a black stack with a few Gaussian tubes.  tests/test_image_classes_host.py shows on the oracle alone what
each class brings; tests/test_gpu_image_classes.py puts every class through the device path."""
import numpy as np
import synth

CLASSES = ("noise", "noisytubes", "inverted", "lowamp", "binary", "saturated", "ball", "blocks")


def make(name, w, h, l):
    """uint8 [l][h][w], contiguous"""
    if name == "noise":  # every wave of hessian_tile mixes all branches; a dense J8
        out = np.random.RandomState(1).randint(0, 256, (l, h, w))
    elif name == "noisytubes":
        out = synth.synth(w, h, l, seed=3, noise=120) if l > 1 else synth.synth(w, h, 3, seed=3, noise=120)[1:2]
    elif name == "ball":  # one wide blob: J8 > 0 over most of the stack, a tiny Jmax
        zz, yy, xx = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
        d2 = (xx - (w - 1) / 2) ** 2 + (yy - (h - 1) / 2) ** 2 + (2 * (zz - (l - 1) / 2)) ** 2
        out = np.floor(250 * np.exp(-d2 / (2 * 40.0 ** 2)))
    elif name == "blocks":  # saturated plateaus (an exactly zero Hessian), straight faces / edges / corners, ties of corr
        out = np.zeros((l, h, w), np.uint8)
        out[l // 8: l - l // 8, 2: h - 2, 10:60] = 255
        out[:, :, 70:72] = 255
    else:
        base = synth.synth(w, h, l, seed=3) if l > 1 else synth.synth(w, h, 3, seed=3)[1:2]
        if name == "inverted":  # a positive trace almost everywhere
            out = 255 - base.astype(np.int32)
        elif name == "lowamp":  # values 0..3: a Jmax near 1e-6
            out = base // 64
        elif name == "binary":
            out = np.where(base > 60, 255, 0)
        elif name == "saturated":  # flat-topped tubes
            out = np.clip(3 * base.astype(np.int32), 0, 255)
        else:
            raise ValueError(f"no image class {name!r}")
    return np.ascontiguousarray(out, np.uint8)
