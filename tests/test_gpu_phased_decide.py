"""GPU: the decision half of the phased SMC step (ph_update, then the drawing branch of the following step's ph_predict, of
pnr_amd/csrc/smc_phased.hip) on GIVEN correlations, regime by regime, through the test tap pnr_phased_decide -- the production
kernels with the launch parameters of a production step; the tap only decides what is in memory beforehand.

Every case compares every word the two kernels leave behind -- the particle block (weights, corr, sig), N_eff, the centroid, the
record of the pending iteration, T / stop, idxres, the flag words, the next step's list and its counter, then the next particles'
poses and priors and the chain numbering -- with the oracle's (orc_smc_draw / orc_smc_decide / orc_smc_pending) BIT FOR BIT, NaN
equal to NaN: the contract of DESIGN.md section 2, so there is no tolerance.  What a case reaches is computed on the CPU from the
inputs (tests/decide_ref.py) before the GPU result exists; tests/test_phased_decide_host.py asserts those coverage conditions alone.
Without a reference value, hence left out: the next particle of a parent whose direction is NaN (the reference indexes its table
with -1)."""
import numpy as np
import pytest
import decide_ref as D
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu


def _run(cases, n_p, S, ratio=0.8):
    """launches that share one context: [(tracker, traces, draws[, den])]"""
    c = D.make_context(n_p, S, ratio)
    try:
        return [D.run_case(case[0], case[1], case[2], den=case[3] if len(case) > 3 else None, ctx=c, lp=i & 1) for i, case in enumerate(cases)]
    finally:
        c.close()


def test_flag_words():
    assert (D.RES, D.STOP, D.T_, D.IT, D.DONE, D.NCH, D.PAUSE) == (lib.PHL_RES, lib.PHL_STOP, lib.PHL_T, lib.PHL_IT, lib.PHL_DONE, lib.PHL_NCH, lib.PHL_PAUSE)


@pytest.mark.parametrize("n_p,S", D.NP_SWEEP)
def test_np_sweep(oracle, n_p, S):
    """blocks of 8 with a scalar tail in the sums, the centroid, N_eff and the CDF: np below 8, 8k - 1, 8k, 8k + 1, one and two passes
    of the 256-thread loops, 500; iterations 0, 1 and 2, carry on and off, ties between scales, NaN scales, shared chains"""
    T = D.make_tracker(oracle, n_p, S)
    rng = np.random.RandomState(n_p * 10 + S)
    _run([(T, D.sweep_traces(T, rng), D.draws_for(rng, n_p))], n_p, S)


@pytest.mark.parametrize("n_p", [8, 37])
def test_weights(oracle, n_p):
    """uniform (exact CDF), one dominant weight, half the weights exactly 0, weights over 2^-120 .. 1 with denormal products; N_eff on
    either side of neff_ratio * np for each"""
    D.weight_family(oracle, n_p, gpu=True)


def test_resampling_draws(oracle):
    """the bisection against the reference's clamped forward walk: draws 0, 1, the largest below ratio 1, the first at ratio 1 and
    RAND_MAX, ties ui == csw[k], flat stretches of the CDF, csw[np - 1] < 1 with ui beyond it, all draws onto one index"""
    cases = D.resampling_cases(oracle)
    for n_p in sorted({c[0].np for c in cases}):
        _run([c for c in cases if c[0].np == n_p], n_p, 1, 2.0)


def test_draw_iteration0(oracle):
    """iter0New's draw (ph_predict alone, at iteration 0: no ph_update precedes it): np whose last ui passes w0cws[sz - 1], draws[0] =
    0 and RAND_MAX, seed directions with 0 .. 3 NaN components; beside them a paused trace, a stopped one and traces at iterations
    1 and 2, whose parents are read through the given idxres or without it"""
    cases = D.iter0_cases(oracle)
    for n_p in sorted({c[0].np for c in cases}):
        c = D.make_context(n_p, 1)
        try:
            for i, (T, specs, draws) in enumerate(x for x in cases if x[0].np == n_p):
                D.run_case(T, specs, draws, ctx=c, lp=i & 1, predict_only=True)
        finally:
            c.close()


def test_draw_later_iterations(oracle):
    """cdf_search_wide against the linear walk: every offset of the table for three directions, u1 == cws[sz - 1], parents on each
    direction, exactly between two, zero and NaN, read through idxres and without"""
    _run(D.iterI_cases(oracle), D.ITERI_NP, 1)


def test_stops(oracle):
    """roundf at exactly +-x.5 on the six faces, the DENSITY stop at nodepervol - 1 / nodepervol, the pending centroid below, at and
    above znccth from FL_STOP 0, 3 and 1, the tail at it == ni"""
    T, faces, dens, pend, den, draws = D.stop_cases(oracle)
    _run([(T, faces + dens + pend, draws, den), (T, faces + pend, draws)], 2, 3)


@pytest.mark.parametrize("nt", [1, 2, 70])
def test_launch_shape(oracle, nt):
    """1, 2 and 70 traces: both parities of the double buffers, paused traces untouched word for word, the next list exactly the
    traces still running"""
    T, specs, draws = D.launch_cases(oracle, nt)
    _run([(T, specs, draws), (T, specs[::-1], draws)], 20, 3)


def test_nonfinite_centroid(oracle):
    """wsum == 0 and a NaN prior sum: every weight, N_eff and the centroid NaN; the reference's build converts the rounded NaN to
    INT_MIN, hence stop 1 at T = it"""
    T, specs, draws = D.nonfinite_cases(oracle)
    _run([(T, specs, draws)], 9, 3)


def test_arguments(oracle):
    T = D.make_tracker(oracle, 4, 1)
    a = D.pack([D.base_trace(T, np.random.RandomState(0), 1)], 4, 1)
    p = pnr_amd.make_params(sigmas=[2.0], np_=4, ni=D.NI)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver("phased")
    try:
        with pytest.raises(pnr_amd.PnrError, match="no volume"):
            c.phased_decide(**a)
        c.set_volume(np.zeros((8, 16, 16), np.uint8))
        for key, j, bad, msg in (("flags", D.IT, D.NI + 1, "iteration"), ("flags", D.IT, -1, "iteration"), ("flags", D.NCH, 0, "chains"),
                                 ("flags", D.NCH, 6, "chains"), ("cmap", 1, 5, "on chain"), ("cmap", 1, -1, "on chain"),
                                 ("idxres", 2, 4, "resampling index"), ("idxres", 2, -1, "resampling index")):
            b = {k: v.copy() for k, v in a.items()}
            b[key][0, j] = bad
            with pytest.raises(pnr_amd.PnrError, match=msg):
                c.phased_decide(**b)
        with pytest.raises(pnr_amd.PnrError, match="step list"):
            c.phased_decide(lp=2, **a)
        with pytest.raises(pnr_amd.PnrError, match="number of traces"):
            c.phased_decide(**{k: v[:0] for k, v in a.items()})
        c.set_smc_driver("persistent")
        with pytest.raises(pnr_amd.PnrError, match="phased driver"):
            c.phased_decide(**a)
        c.set_smc_driver("phased")
        out = c.phased_decide(**a)
        assert out["cnt_next"][0] == 1 and out["flags_u"][0, D.IT] == 2
    finally:
        c.close()
