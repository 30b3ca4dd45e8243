"""The swap-round cases of tests/swap_cases.py mean what they say -- shown from the float64 oracle alone, without a GPU:
  * every scripted ladder drops the carried state exactly at its drop set, whatever the round's uniforms;
  * EVERY case the device test runs (scripted, ties, normal draws, specials; all sizes, all rounds) is at least 8 units of fp32
    spacing away from every decision boundary, so the device has no excuse to differ;
  * the NumPy restatement of the ballot scan passes every case, and each of its four mutants (the scan's corner cases, broken one at
    a time) fails at least one: the cases are strong enough to notice exactly the defects they were built for;
  * the replay helpers reproduce the oracle's own posted scalars and permutations from the oracle's own traces."""
import math

import numpy as np
import pytest

import parity
import swap_cases as sc
from parity import orc

TAPE = orc.PhiloxTape(sc.SEED)


@pytest.mark.parametrize("R", sc.SIZES)
def test_scripted_cases_drop_exactly_their_drop_set(R):
    for name, drops in sc.drop_sets(R).items():
        L = sc.scripted(R, drops)
        for rnd in sc.ROUNDS:
            src, nsw = orc.swap_cascade([float(v) for v in L], TAPE.swap_uniforms(rnd, R - 1))
            got = [k for k in range(R - 1) if src[k] != k + 1]
            assert got == list(drops), (R, name, rnd)
            assert nsw == R - 1 - len(drops)


def test_the_drop_sets_reach_the_corners():
    """Lane 63 and lane 0 of a later window, a partial last window and a full one are all among the cases."""
    assert {(R - 1) % sc.WAVE for R in sc.SIZES} >= {0, 1, 63}          # full last window, one live lane, one dead lane
    for R in sc.SIZES:
        s = sc.drop_sets(R)
        assert 63 in s["lane63"] and (R < 66 or 64 in s["lane0"]) and [63] in s.values()
        assert [R - 2] in s.values() and [R - 3] in s.values()
    assert any(name.startswith("nan-next-64") for name, _, _ in sc.cases(130, 0))


@pytest.mark.parametrize("R", sc.SIZES)
def test_every_case_clears_the_margin(R):
    worst = {}
    for rnd in sc.ROUNDS:
        u = TAPE.swap_uniforms(rnd, R - 1)
        for name, L, _ in sc.cases(R, rnd):
            m = sc.margin(L, u)
            kind = "scripted" if name.startswith("scripted") else name if name in ("ties", "normal") else "special"
            worst[kind] = min(worst.get(kind, math.inf), m)
            assert m >= sc.MARGIN_UNITS, (R, rnd, name, m)
    print(f"R = {R}: worst margins in units " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert worst["scripted"] > 2.5e6                         # |ln 2u - 1| >= 1 - ln 2 at a spacing of 2^-23 .. 2^-20


def test_margin_notices_a_near_tie():
    """A pair moved to within a few ulp of its boundary is reported as such."""
    R = 66
    u = TAPE.swap_uniforms(0, R - 1)
    L = sc.ties(R).astype(np.float64)
    c = 0
    src, _ = orc.swap_cascade(list(L), u)
    for k in range(40):
        if src[k] != k + 1:
            c = k + 1
    L[41] = L[c] + math.log(2.0 * u[40]) + 3 * np.spacing(np.float32(1.0))
    assert sc.margin(L, u) < 4.0
    assert sc.margin(L, u, dL=np.full(R, 1e-6)) < 0.0        # an uncertainty of the scalars comes off the distance


def _passes(mutant, R, rnd):
    u = TAPE.swap_uniforms(rnd, R - 1)
    for name, L, _ in sc.cases(R, rnd):
        want = orc.swap_cascade([float(v) for v in L], u)
        if sc.ballot_scan(L, u, mutant) != (want[0], want[1]):
            return name
    return None


@pytest.mark.parametrize("R", sc.SIZES)
def test_ballot_scan_restated_passes_every_case(R):
    for rnd in sc.ROUNDS:
        assert _passes(None, R, rnd) is None, (R, rnd)


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_each_mutant_of_the_scan_fails_a_case(mutant):
    failed = {R: _passes(mutant, R, 0) for R in (65, 66, 130)}
    print(mutant, failed)
    assert any(v is not None for v in failed.values()), mutant
    # R = 65 is one full window: only the lane-63 mask can go wrong there; the other three need a second, or a partial, window
    assert (failed[65] is not None) == (mutant == "no_j63_case"), failed
    assert failed[66] is not None and failed[130] is not None, failed


def _oracle_run(R, S, si, seed, swap_rule=0, use_lg=True, ntr=7, nte=3):
    d = parity.datasets()
    pt = orc.PTOracle(orc.TASK_REG, (4, 5, 1), d["sunspot_train"][:ntr], d["sunspot_test"][:nte], R, 2, S * R, si, use_lg=use_lg,
                      l_prob=0.5, lr=0.1, seed=seed, swap_rule=swap_rule)
    lik0 = [rep.likelihood for rep in pt.replicas]
    pt.run()
    likeh = np.stack([rep.likeh[:, 0] for rep in pt.replicas])
    accept = np.stack([rep.accept_list for rep in pt.replicas])
    nacc = [rep.num_accepted for rep in pt.replicas]
    return pt, likeh, accept, nacc, lik0


def test_replay_reproduces_the_oracles_own_rounds():
    """4-5-1, R = 8, S = 41, si = 8: four hand-off rounds and the phantom one, from the oracle's traces alone."""
    R, S, si = 8, 41, 8
    pt, likeh, accept, nacc, lik0 = _oracle_run(R, S, si, seed=11)
    rounds = sc.replay_rule0(orc.TASK_REG, pt.temperatures, likeh, accept, nacc, lik0, S, si, dtype=np.float64)
    assert len(rounds) == pt.rounds_done == 5 and [ph for _, _, ph in rounds] == [False] * 4 + [True]
    assert sum(int(a.sum()) for a in sc.accepted_steps(accept, nacc)) > R          # the chains moved: the scalars are not lik0
    for n, (L, dL, _) in enumerate(rounds):
        assert [float(v) for v in L] == pt.L_log[n] and not dL.any(), n
        assert orc.swap_cascade([float(v) for v in L], pt.tape.swap_uniforms(n, R - 1))[0] == pt.src_log[n]
    nsw, worst, skipped = sc.check_rounds(rounds, pt.src_log, pt.tape)
    assert nsw == pt.num_swap and not skipped and worst >= sc.MARGIN_UNITS


def test_rule1_replay_reproduces_the_oracles_own_rounds():
    """Even/odd rule at R = 131 (the device's second pass of the strided loop): the replayed untempered scalars give the oracle's
    own permutations, round for round, and every round clears the rule-1 margin."""
    R, S, si = 131, 41, 8
    pt, likeh, accept, nacc, lik0 = _oracle_run(R, S, si, seed=sc.EVENODD_SEED, swap_rule=1)
    T = pt.temperatures
    Lr = sc.replay_rule1(T, likeh, accept, nacc, lik0, S, si, pt.tape, dtype=np.float64)
    assert len(Lr) == pt.rounds_done == 4 and pt.num_swap > 0
    nsw = 0
    for n, L in enumerate(Lr):
        src, k = sc.rule1_round(L, T, pt.tape.swap_uniforms(n, R - 1), n)
        assert src == pt.src_log[n], n
        nsw += k
        assert sc.rule1_margin(L, np.float32(T), pt.tape.swap_uniforms(n, R - 1), n) >= sc.RULE1_MARGIN_UNITS, n
    assert nsw == pt.num_swap
