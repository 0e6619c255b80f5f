"""The kernel timers of an SMC step.  A step of the phased driver is five launches -- ph_predict, ph_cube (option "cube_copy"), ph_sample,
ph_sums, ph_update -- timed as the groups smc_predict, smc_cube, smc, smc_sums, smc_update; bench.py's kernel table relies on them.  The
batch driver (trace_batch) and the streaming engine (trace_replay) both issue the step, so both must report all five groups, once per
step, and the timers must not change a result."""
import numpy as np
import pytest

import pnr_amd
import synth

pytestmark = pytest.mark.gpu

GROUPS = ("smc_predict", "smc_cube", "smc", "smc_sums", "smc_update")
NI = 30


@pytest.fixture(scope="module")
def traced():
    """a phased-driver context on the 48^3 stack of test_gpu_buffers.py, and its sorted seeds"""
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 4), np_=20, ni=NI), 0)
    c.set_smc_driver("phased")
    c.set_volume(synth.synth(48, 48, 48, seed=3))
    c.frangi()
    seeds = c.score_filter_sort(c.extract_seeds())
    assert len(seeds) >= 4
    yield c, seeds
    c.close()


def _launches(c):
    return {g: c.kernel_ms(g)[1] for g in GROUPS}


def _batch(c, seeds, cube_copy):
    c.set_option("cube_copy", cube_copy)
    c.reset_kernel_ms()
    T, stop, xc, _ = c.trace_batch(seeds[:4])
    return T, stop, xc, _launches(c)


def test_batch_driver_times_every_kernel_of_every_step(traced):
    c, seeds = traced
    c.set_profiling(True)
    try:
        T, stop, xc, n = _batch(c, seeds, 1)
        T0, stop0, xc0, n0 = _batch(c, seeds, 0)
    finally:
        c.set_option("cube_copy", 1)
        c.set_profiling(False)
    P = n["smc_predict"]
    print(f"batch driver: T = {T.tolist()}, launches {n}; without the cube copy {n0}")
    # the host stops issuing steps once the counter of running traces, read a few steps late, is zero: at least one step per
    # iteration any trace ran, at most iterations 0 .. ni
    assert min(int(T.max()) + 1, NI) <= P <= NI + 1
    assert all(n[g] == P for g in GROUPS)
    assert n0["smc_cube"] == 0
    assert n0["smc_predict"] > 0 and all(n0[g] == n0["smc_predict"] for g in GROUPS if g != "smc_cube")
    assert np.array_equal(T0, T) and np.array_equal(stop0, stop) and np.array_equal(xc0, xc)


PROFILED = [(1, 1), (1, 3), (2, 1), (2, 3)]  # (groups, profile_every)


@pytest.fixture(scope="module")
def replays(traced):
    """trace_replay of all seeds: profiled under every (groups, profile_every), and once without profiling"""
    c, seeds = traced
    c.set_option("cube_copy", 1)
    out = {}
    try:
        for groups, every in PROFILED:
            c.set_option("groups", groups)
            c.set_option("profile_every", every)
            c.set_profiling(True)
            c.reset_kernel_ms()
            nodes, links, _, _ = c.trace_replay(seeds)
            out[(groups, every)] = (nodes, links, _launches(c))
        c.set_profiling(False)
        c.reset_kernel_ms()
        nodes, links, _, _ = c.trace_replay(seeds)
        out[None] = (nodes, links, _launches(c))
    finally:
        c.set_profiling(False)
        c.set_option("groups", 0)
        c.set_option("profile_every", 1)
    return out


@pytest.mark.parametrize("groups,every", PROFILED)
def test_streaming_engine_times_every_kernel_of_a_profiled_step(replays, groups, every):
    n = replays[(groups, every)][2]
    print(f"streaming engine, groups = {groups}, profile_every = {every}: launches {n}")
    P = n["smc_predict"]
    assert P > 0 and P % every == 0
    assert all(n[g] == P for g in GROUPS)


def test_streaming_engine_results_do_not_depend_on_the_timers(replays):
    nodes, links, n = replays[None]
    assert len(nodes) > 1
    assert all(v == 0 for v in n.values())
    for key in PROFILED:
        assert np.array_equal(replays[key][0], nodes) and np.array_equal(replays[key][1], links), key
