"""Ladder adaptation and per-pair swap diagnostics without a GPU: known answers of the float64 update (tests/ladder_ref.py),
its convergence on a synthetic acceptance model, ladder_stats_from_log on synthetic swap logs against an independent count, and
the refusals of ParallelTempering(adapt_ladder=...) that need no library."""
import numpy as np
import pytest

import ladder_ref as ref
from ptnn_amd import ladder
from ptnn_amd.parallel_tempering import ladder_stats_from_log


def _geo(R, tmax):
    return np.asarray(ladder.temperatures(R, tmax), np.float32)


# ------------------------------------------------------------------ the update
def test_equal_acceptances_leave_the_ladder_unchanged():
    T0 = _geo(8, 10)
    s = ref.initial_log_gaps(T0)
    for a in (0.0, 0.37, 1.0):
        s1, T = ref.update(s, np.full(7, a), 3, 0.5, 20.0, T0[-1])
        assert np.allclose(s1, s, rtol=0, atol=1e-15)              # the mean of equal values may be off by an ulp
        assert np.array_equal(T.astype(np.float32), T0)             # the float32 ladder: bit for bit


def test_weak_pair_gap_shrinks():
    T0 = _geo(8, 10)
    s = ref.initial_log_gaps(T0)
    a = np.full(7, 0.6)
    a[3] = 0.1
    _, T = ref.update(s, a, 0, 0.5, 20.0, T0[-1])
    g0, g1 = np.diff(T0.astype(np.float64)), np.diff(T)
    assert g1[3] / g0[3] < min(g1[k] / g0[k] for k in range(7) if k != 3)
    assert g1[3] < g0[3]


def test_endpoints_fixed_and_monotone():
    rng = np.random.default_rng(5)
    T0 = _geo(16, 1000)
    s = ref.initial_log_gaps(T0)
    for t in range(200):
        s, T = ref.update(s, rng.random(15), t, 2.0, 5.0, T0[-1])
        assert T[0] == 1.0 and T[-1] == float(T0[-1])
        assert np.all(np.diff(T) > 0)
        Tf = T.astype(np.float32)
        assert Tf[0] == 1.0 and Tf[-1] == T0[-1] and np.all(np.diff(Tf) > 0)


def test_kappa_schedule():
    assert ref.kappa(0, 0.5, 20.0) == 0.5
    assert ref.kappa(20, 0.5, 20.0) == 0.25
    assert ref.kappa(60, 2.0, 20.0) == 0.5
    assert np.isclose(ref.kappa(1, 1.0, 1000.0), 1000.0 / 1001.0)


def test_converges_on_a_synthetic_model():
    """a_k = exp(-c (delta beta_k)^2): the fixed point has equal delta beta; the spread of the acceptances falls below 1e-3."""
    T0 = _geo(12, 1000)
    c = 40.0
    s = ref.initial_log_gaps(T0)
    T = T0.astype(np.float64)

    def acc(T):
        return np.exp(-c * np.diff(1.0 / T) ** 2)
    spread0 = np.ptp(acc(T))
    for t in range(20000):
        s, T = ref.update(s, acc(T), t, 0.5, 1e9, T0[-1])      # t0 huge: constant kappa
        if np.ptp(acc(T)) < 1e-3:
            break
    assert np.ptp(acc(T)) < 1e-3 < spread0
    assert T[0] == 1.0 and T[-1] == float(T0[-1])


def test_replay_is_the_update_iterated():
    rng = np.random.default_rng(1)
    T0 = _geo(6, 50)
    rows = rng.random((5, 5))
    hist = ref.replay(T0, rows, 5, 0.5, 20.0)
    assert hist.shape == (6, 6) and np.array_equal(hist[0], T0)
    s = ref.initial_log_gaps(T0)
    for t in range(5):
        s, T = ref.update(s, rows[t], t, 0.5, 20.0, T0[-1])
        assert np.array_equal(hist[t + 1], T.astype(np.float32))


def test_pair_accept_reference():
    T = np.array([1.0, 2.0, 4.0])
    a = ref.pair_accept(T, [-10.0, -5.0, np.nan])
    assert a[0] == 1.0 and a[1] == 1.0
    a = ref.pair_accept(T, [-5.0, -10.0, -30.0])
    assert np.isclose(a[0], np.exp(-2.5)) and np.isclose(a[1], np.exp(-5.0))


# ------------------------------------------------------------------ ladder_stats_from_log
def _check_against_ref(log, rule, first, n_moves=None):
    st = ladder_stats_from_log(log, rule, first, n_moves=n_moves)
    acc, prop, trips = ref.stats_from_log(log, rule, first, n_moves)
    assert st["accepted"].tolist() == acc and st["proposed"].tolist() == prop
    assert st["round_trips"].tolist() == trips
    return st


def test_rule1_parity_counting():
    R = 4
    ident = list(range(R))
    log = [[1, 0, 2, 3], [0, 2, 1, 3], [0, 1, 3, 2], ident]     # round 0: pair 0; round 1: pair 1; round 2: pair 2; round 3: none
    st = _check_against_ref(log, 1, 0)
    assert st["proposed"].tolist() == [2, 2, 2]                 # even rounds propose pairs 0, 2; odd rounds pair 1
    assert st["accepted"].tolist() == [1, 1, 1]
    assert np.allclose(st["pair_accept"], [0.5, 0.5, 0.5])
    st = _check_against_ref(log, 1, 2)
    assert st["proposed"].tolist() == [1, 1, 1] and st["accepted"].tolist() == [0, 0, 1]


def test_rule0_counting_and_phantom_excluded():
    log = [[1, 2, 0], [0, 1, 2], [1, 0, 2]]                     # cascade: state 0 carried to the top in round 0
    st = _check_against_ref(log, 0, 0)
    assert st["proposed"].tolist() == [3, 3] and st["accepted"].tolist() == [2, 1]
    st = _check_against_ref(log, 0, 0, n_moves=2)               # the last row is the phantom round
    assert st["proposed"].tolist() == [2, 2] and st["accepted"].tolist() == [1, 1]


def test_exactly_two_round_trips():
    # R = 3, rule 1; walker 0 goes 0 -> 1 -> 2 -> 1 -> 0 twice
    up0, up1 = [1, 0, 2], [0, 2, 1]                              # swap pair 0 (even round), pair 1 (odd round)
    ident = [0, 1, 2]
    log = [up0, up1, ident, up1, up0, ident] * 2 + [up0]          # walker 0 after each round: 1, 2, 2, 1, 0, 0 | twice, then 1
    st = _check_against_ref(log, 1, 0)
    assert st["round_trips"][0] == 2
    assert st["mean_round_trip_rounds"] == 5.0                  # timed from the last visit of 0: rounds 0 -> 5 and 6 -> 11


def test_label_and_state_logs_random():
    rng = np.random.default_rng(9)
    R = 8
    for rule in (0, 1):
        log = []
        for r in range(60):
            src = np.arange(R)
            for k in range(r % 2 if rule == 1 else 0, R - 1, 2 if rule == 1 else 1):
                if rule == 1 and rng.random() < 0.6:
                    src[k], src[k + 1] = k + 1, k
            if rule == 0:
                src = rng.permutation(R)
            log.append(src.tolist())
        for first in (0, 17):
            _check_against_ref(log, rule, first)


def test_stats_refusals():
    with pytest.raises(ValueError):
        ladder_stats_from_log(np.zeros((3,), np.int32), 1, 0)
    with pytest.raises(ValueError):
        ladder_stats_from_log([[0, 1]], 2, 0)


# ------------------------------------------------------------------ refusals before the library loads
def _pt(tmp_path, **kw):
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    d = np.zeros((20, 5))
    args = dict(seed=1, write_files=False)
    args.update(kw)
    return ParallelTempering(False, 0.1, d, d, [4, 5, 1], 8, 10, 8 * 1001, 5, 0.5, str(tmp_path), **args)


def test_refuses_rule0(tmp_path):
    with pytest.raises(ValueError, match="swap_rule=1"):
        _pt(tmp_path, adapt_ladder=True)


def test_refuses_bad_dict(tmp_path):
    with pytest.raises(ValueError, match="dict"):
        _pt(tmp_path, swap_rule=1, adapt_ladder=dict(round=3))
    with pytest.raises(ValueError, match="kappa0"):
        _pt(tmp_path, swap_rule=1, adapt_ladder=dict(kappa0=-1.0))
    with pytest.raises(ValueError, match="t0"):
        _pt(tmp_path, swap_rule=1, adapt_ladder=dict(t0=float("inf")))


def test_refuses_too_few_rounds_in_burn_in(tmp_path):
    pt = _pt(tmp_path, swap_rule=1, adapt_ladder=True)
    with pytest.raises(ValueError, match="burn_in"):
        pt.initialize_chains(0.005)                              # step 5: one hand-off (step 5 itself is not before it)


def test_refuses_rounds_beyond_run_or_switch(tmp_path):
    pt = _pt(tmp_path, swap_rule=1, adapt_ladder=dict(rounds=10 ** 6))
    with pytest.raises(ValueError, match="swap rounds"):
        pt.initialize_chains(0.5)
    # S = 1000 -> switch at step 600: round 120 hands off at step 600, round 121 at 605
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    d = np.zeros((20, 5))
    pt = ParallelTempering(False, 0.1, d, d, [4, 5, 1], 8, 10, 8 * 1000, 5, 0.5, str(tmp_path), seed=1, write_files=False,
                           swap_rule=1, adapt_ladder=dict(rounds=121))
    with pytest.raises(ValueError, match="temperature switch"):
        pt.initialize_chains(0.5)


def test_adapt_spec_counts_burn_in_rounds(tmp_path):
    pt = _pt(tmp_path, swap_rule=1, adapt_ladder=True)
    pt.burn_in = 0.5                                            # S = 1001, no switch; hand-offs 5, 10, ..., 495 before step 500
    assert pt._ladder_adapt_spec()[0] == 99
    assert pt._freeze_step() == 496
    pt = _pt(tmp_path, swap_rule=1, adapt_ladder=dict(rounds=0))
    pt.burn_in = 0.5
    assert pt._ladder_adapt_spec()[0] == 0 and pt._freeze_step() == 0
