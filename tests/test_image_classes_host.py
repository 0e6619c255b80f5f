"""What each image class of tests/imgclass.py brings, on the oracle alone (no GPU): the conditions below are what
tests/test_gpu_image_classes.py relies on, so that its byte-for-byte parity cannot pass on inputs that exercise nothing -- a dense
J8, many seeds, a filter that keeps none of them, saturated plateaus, ties of corr among the kept seeds, a tiny Jmax, every stop
reason.  They are conditions on the inputs, not tolerances: if one misses, the generator has changed."""
import numpy as np
import pytest
import orc
import imgclass

W, H, L_, SIGS, ZDIST, TOL, ZNCCTH, NP, NI = 83, 29, 41, [2.0, 3.0], 2.0, 5, 0.3, 50, 12


@pytest.fixture(scope="module")
def stages(oracle):
    """per class: the stack, the oracle's J8 / Jmax / seeds / scores and the stop reasons of its first three sorted seeds"""
    out = {}
    T = orc.Tracker(oracle, SIGS, 2, NP, NI, 3.0, ZNCCTH, zdist=ZDIST)
    for name in imgclass.CLASSES:
        img = imgclass.make(name, W, H, L_)
        assert img.dtype == np.uint8 and img.shape == (L_, H, W) and img.flags.c_contiguous
        J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, SIGS, ZDIST)
        J8 = orc.j8(oracle, J, jmin, jmax)
        so = orc.extract_seeds(oracle, TOL, J8, Vx, Vy, Vz)
        corr = T.zncc(img, so[:, :6])[0] if len(so) else np.zeros(0, np.float32)
        keep = corr >= np.float32(ZNCCTH)
        order = np.argsort(-corr[keep], kind="stable")
        stops = []
        for q in so[keep][order][:3, :6]:
            for sgn in (1, -1):
                q_ = q.copy(); q_[3:] *= sgn
                stops.append(T.trace(img, q_)[1])
        out[name] = dict(img=img, dense=float((J8 > 0).mean()), jmax=jmax, seeds=len(so), kept=corr[keep][order], stops=stops)
        print(f"\n[{name}] J8>0 {out[name]['dense']:.3f} jmax {jmax:.3g} seeds {len(so)} kept {int(keep.sum())} stops {stops}")
    return out


def _ties(kept):
    """kept seeds whose corr equals another kept seed's"""
    _, inv, cnt = np.unique(kept, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def test_generators_are_deterministic():
    for name in imgclass.CLASSES:
        for shape in ((83, 29, 41), (83, 29, 1)):
            a, b = imgclass.make(name, *shape), imgclass.make(name, *shape)
            assert a.shape == shape[::-1] and a.dtype == np.uint8 and np.array_equal(a, b), (name, shape)
    with pytest.raises(ValueError):
        imgclass.make("nothing", 8, 8, 8)


def test_noise_is_dense_and_keeps_no_seed(stages):
    s = stages["noise"]
    assert s["dense"] >= 0.20 and s["seeds"] >= 500 and len(s["kept"]) == 0, (s["dense"], s["seeds"], len(s["kept"]))


def test_ball_is_dense(stages):
    assert stages["ball"]["dense"] >= 0.40, stages["ball"]["dense"]


def test_blocks_are_saturated_and_tie(stages):
    s = stages["blocks"]
    assert (s["img"] == 255).mean() >= 0.30 and _ties(s["kept"]) >= 20, ((s["img"] == 255).mean(), _ties(s["kept"]))


def test_lowamp_has_a_tiny_jmax(stages):
    s = stages["lowamp"]
    assert 0 < s["jmax"] < 1e-5 and len(s["kept"]) >= 50, (s["jmax"], len(s["kept"]))


@pytest.mark.parametrize("name", ["inverted", "binary", "saturated", "noisytubes"])
def test_tube_variants_keep_seeds(stages, name):
    assert len(stages[name]["kept"]) >= 20, len(stages[name]["kept"])


def test_every_stop_reason_is_reached(stages):
    got = set(st for s in stages.values() for st in s["stops"])
    assert {0, 1, 2} <= got, got
