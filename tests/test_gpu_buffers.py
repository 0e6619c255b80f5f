"""Ownership of device and pinned memory (csrc/devbuf.h): every allocation of libpnr_hip.so goes through one owner type that counts
its bytes, so "close() returns everything", "a second run at the same size keeps nothing more" and "a failed allocation leaks
nothing" are differences of lib.live_bytes().  Differences, after gc.collect(): other contexts of the pytest process may be alive."""
import gc

import numpy as np
import pytest

import pnr_amd
from pnr_amd import lib
import synth

pytestmark = pytest.mark.gpu

SIGMAS = (2, 4)


def _params(somaradius=0):
    return pnr_amd.make_params(sigmas=SIGMAS, np_=20, ni=30, somaradius=somaradius)


def _live():
    gc.collect()
    return lib.live_bytes()


@pytest.fixture(scope="module")
def img48():
    """the 48^3 stack of every test here, with one cell body so that the soma path has voxels to compact"""
    img = synth.add_somas(synth.synth(48, 48, 48, seed=3), [(30, 14, 24, 5)])
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def fresh48(img48):
    """(Jmin, Jmax), J8 of the 48^3 stack on a context that has done nothing else"""
    c = pnr_amd.Context(_params(), 0)
    c.set_volume(img48)
    mm = c.frangi()
    j8 = c.get_frangi(J=False, V=False)["J8"]
    c.close()
    return mm, j8


def _touch_every_owner(c, img, driver):
    """one call of every stage that owns device or pinned memory, on context c"""
    c.set_volume(img)
    c.filter_volume(median=3, tophat=2)
    c.soma()
    c.frangi()
    g = c.get_frangi(J=True, V=True)
    assert g["J"].shape == img.shape and g["Vx"].shape == img.shape
    seeds = c.score_filter_sort(c.extract_seeds())
    assert len(seeds) >= 4
    nodes, links, ntr, _ = c.trace_replay(seeds)
    assert len(nodes) > 1
    T, _, _, dbg = c.trace_batch(seeds[:4], dbg_iters=3)
    assert len(T) == 8 and dbg["xfilt"].shape[1] == 3
    c.reconstruct(nodes, links)
    k, _ = c.measure_radii(np.stack([nodes["x"], nodes["y"], nodes["z"]], 1)[1:])
    assert len(k) == len(nodes) - 1
    k, _ = c.measure_radii(np.stack([nodes["x"], nodes["y"], nodes["z"]], 1)[1:], rmax=7)  # another shell table: the cached one is rebuilt
    assert len(k) == len(nodes) - 1
    c.gaussian(2.0)
    c.hessian(2.0)
    A = np.eye(3)[None].repeat(5, 0)
    c.eigen(A)
    c.eigen(A, vectors=False)
    c.expf(np.linspace(-3, 0, 17, dtype=np.float32))
    img16 = np.stack([img.astype(np.uint16) * 200, img.astype(np.uint16) * 7], -1)
    c.set_volume(img16, channel=1)
    assert c.window is not None
    if driver == "phased":  # a one-slice stack takes the 2-D tracker tables: the context reloads them (the persistent driver is 3-D only)
        c.set_volume(np.ascontiguousarray(img[24:25]))


@pytest.mark.parametrize("driver", ["phased", "persistent"])
def test_close_returns_everything(img48, driver):
    d0, p0 = _live()
    c = pnr_amd.Context(_params(somaradius=3), 0)
    c.set_smc_driver(driver)
    _touch_every_owner(c, img48, driver)
    d1, p1 = _live()
    print(f"{driver}: live while open: device {d1 - d0} B, pinned {p1 - p0} B")
    assert d1 > d0 and p1 > p0
    c.close()
    assert _live() == (d0, p0)


@pytest.mark.parametrize("driver", ["phased", "persistent"])
def test_second_run_keeps_nothing_more(img48, driver):
    d0, p0 = _live()
    c = pnr_amd.Context(_params(somaradius=3), 0)
    c.set_smc_driver(driver)
    _touch_every_owner(c, img48, driver)
    first = _live()
    _touch_every_owner(c, img48, driver)
    second = _live()
    print(f"{driver}: after run 1 {first[0] - d0} / {first[1] - p0} B, after run 2 {second[0] - d0} / {second[1] - p0} B (device / pinned)")
    assert second == first
    c.close()
    assert _live() == (d0, p0)


def test_failed_allocation_leaks_nothing(img48, fresh48):
    import torch
    d0, p0 = _live()
    c = pnr_amd.Context(_params(), 0)
    c.set_volume(img48)
    c.frangi()
    before = _live()
    t = torch.zeros(64, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    # a stack no device can hold: PNR_E_NOMEM before any sample is read
    rc = c.L.pnr_set_volume_u16_device(c.h, t.data_ptr(), 1 << 20, 1 << 10, 1 << 20, 1, 0, None, None, None)
    assert rc == -5, c.L.pnr_last_error()
    after = _live()
    assert after[0] <= before[0] and after[1] <= before[1]
    c.set_volume(img48)
    assert c.frangi() == fresh48[0]
    assert np.array_equal(c.get_frangi(J=False, V=False)["J8"], fresh48[1])
    c.close()
    assert _live() == (d0, p0)


def test_shrink_and_regrow():
    def run(c, img):
        c.set_volume(img)
        c.frangi()
        return c.get_frangi(J=False, V=False)["J8"], c.extract_seeds()

    small, large = synth.synth(32, 32, 32, seed=5), synth.synth(64, 64, 64, seed=6)
    d0, p0 = _live()
    ref = pnr_amd.Context(_params(), 0)
    j8_ref, seeds_ref = run(ref, small)
    ref.close()
    assert len(seeds_ref) > 0
    c = pnr_amd.Context(_params(), 0)
    run(c, small)
    run(c, large)
    j8, seeds = run(c, small)
    assert np.array_equal(j8, j8_ref)
    assert np.array_equal(seeds, seeds_ref)
    c.close()
    assert _live() == (d0, p0)


def test_exchange_returns_everything():
    d0, p0 = _live()
    x = lib.RcclExchange(lib.RcclExchange.unique_id(), 0, 1, 0, capacity=1 << 16)
    d1, p1 = _live()
    assert d1 - d0 == 2 << 16 and p1 - p0 == 2 << 16  # send + receive staging of one rank, device and pinned
    x.close()
    assert _live() == (d0, p0)
