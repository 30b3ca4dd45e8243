"""Cases, decision margins and replay helpers for the swap round (cascade_lds_prefix in csrc/ptnn_dev_spec.hpp) past one wave of
pairs.  Host only: nothing here touches the library; the only import is the float64 oracle.  tests/test_swap_cases_cpu.py proves
from the oracle alone that the cases mean what they say, tests/test_gpu_swap_cascade.py runs them on the device.

THE DECISION MARGIN, rule 0 (the reference's cascade).  The oracle swaps pair k iff u_k < min(1, 0.5 exp(min(709, L[k+1] - L[c]))),
i.e. iff ln(2 u_k) < min(709, L[k+1] - L[c]) =: rhs.  The device forms both sides in fp32 from the SAME inputs (the fp32 scalars
L and the 23-bit uniform, exact in fp32) and differs from the float64 evaluation by
    * one fp32 subtraction d = L[k+1] - L[c]:                               1/2 ulp of d;
    * ln(2 u) = LN2 * v_log_f32(2 u) (logf_fast; 2 u is exact): 1 ulp for the instruction, 1/2 ulp for the product and
      1/2 ulp for the rounding of the constant LN2:                         at most 2 ulp of ln(2 u).
With the unit = the fp32 spacing at max(|rhs|, |ln 2u|, 1) (one unit is at least one ulp of either side) the two sides move by
less than 2.5 units together.  A case or a round is held to the oracle when every pair with a finite rhs is at least
MARGIN_UNITS = 8 units away from its decision boundary: more than three times the a-priori error.  A decision outside 8 units that
the device takes differently is a finding about logf_fast or the scan, not a reason to widen the bound.  (rhs = -inf, a carried
+inf or a -inf picked up, decides without arithmetic and has no margin; rhs = 709 from the clamp -- NaN, +inf, a difference above
709 -- is finite and counts: ln(2 u) >= -16 is hundreds of units away.)

THE DECISION MARGIN, rule 1 (even/odd Metropolis, not in the reference).  Pair k swaps iff u_k < p, p = min(1, exp(min(80, d))),
d = (1/T_k - 1/T_k+1) (Lr[k+1] - Lr[k]) on untempered log-likelihoods.  d >= 0 (or NaN) gives p = 1 on both sides: the signs of the
two fp32 differences are exact and u < 1 always.  For d < 0 the fp32 chain is
    * two reciprocals a = 1/T_k, b = 1/T_k+1:                               at most 1 ulp each;
    * the subtraction g = a - b:                                            1/2 ulp of g, plus the two reciprocal errors, which the
      cancellation amplifies: relative error e_g = (ulp(a) + ulp(b) + ulp(g)/2) / |g|  (4.5e-5 on a ladder of 131 rungs up to T = 2);
    * the subtraction Lr[k+1] - Lr[k] and the product with g:               2^-24 each, relative;
    * expf_fast(d) = v_exp_f32(LOG2E * d): the product and the rounding of LOG2E move the argument by 2^-23 |d| LOG2E, i.e. p by
      2^-23 |d| relative, and the instruction adds 1 ulp:                   2^-23 relative.
Relative error of p:  e_p = |d| (e_g + 2^-23 + 2^-23) + 2^-23.  The margin of a pair is |u - p| / p in units of e_p; a round is held
to the oracle when every pair with d < 0 is at least RULE1_MARGIN_UNITS = 3.2 units away (the same ratio as 8 : 2.5 above)."""
import math
import os
import sys

import numpy as np

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
if _ORACLE not in sys.path:
    sys.path.insert(0, _ORACLE)

import ptnn_oracle as orc  # noqa: E402

WAVE = 64
SEED = 4242
SIZES = (65, 66, 128, 129, 130, 193, 257, 512, 513, 1024)
ROUNDS = (0, 1, 7)
MARGIN_UNITS = 8.0
RULE1_MARGIN_UNITS = 3.2
EVENODD_SEED = 7          # seed of the even/odd runs (tests/test_gpu_swap_cascade.py part c and its CPU check)
MUTANTS = ("no_j63_case", "lc_not_carried", "stale_lc_at_lane0", "dead_lanes_counted")

# seeds of the N(-300, 2) draws by (R, round); an entry here replaces the default (R, round) seed of a draw whose margin fell below 8
NORMAL_SEEDS = {}


# ---- scripted ladders ---------------------------------------------------------------------------------------------------------
def scripted(R, drops):
    """float32 L[R] for which the carried state is dropped exactly at the pairs in `drops`, whatever the uniforms are:
    L[k+1] = L[c] + 1 where the state swaps (ln 2u < ln 2 < 1), L[k+1] = L[c] - 50 where it is dropped (ln 2u >= ln 2^-23 > -17).
    Every value is an integer below 2^24 in size: exact in fp32, and so is every difference."""
    drops = set(int(k) for k in drops)
    assert all(0 <= k < R - 1 for k in drops), (R, sorted(drops))
    L = np.zeros(R, dtype=np.float64)
    c = 0
    for k in range(R - 1):
        if k in drops:
            L[k + 1] = L[c] - 50.0
            c = k + 1
        else:
            L[k + 1] = L[c] + 1.0
    out = L.astype(np.float32)
    assert (out.astype(np.float64) == L).all()
    return out


def drop_sets(R):
    """name -> sorted list of pairs: the drop sets of the scripted cases at R rungs (equal sets under two names are kept once)."""
    pairs = range(R - 1)
    sets = {
        "none": [],
        "all": list(pairs),
        "odd": [k for k in pairs if k & 1],
        "lane63": [k for k in pairs if k % WAVE == 63],
        "lane0": [k for k in pairs if k % WAVE == 0],
        "lanes0-62-63": [k for k in pairs if k % WAVE in (0, 62, 63)],
    }
    for name, k in (("pair62", 62), ("pair63", 63), ("pair64", 64), ("pair65", 65), ("pairR-3", R - 3), ("pairR-2", R - 2)):
        if 0 <= k < R - 1:
            sets[name] = [k]
    out, seen = {}, set()
    for name, s in sets.items():
        if tuple(s) not in seen:
            seen.add(tuple(s))
            out[name] = s
    return out


# ---- uniform-decided ladders --------------------------------------------------------------------------------------------------
def ties(R):
    """All L equal: d = 0 exactly, the decision is u < 0.5."""
    return np.full(R, -312.5, dtype=np.float32)


def normal_draw(R, rnd):
    """L ~ N(-300, 2) rounded to float32, seeded per (R, round)."""
    seed = NORMAL_SEEDS.get((R, rnd), (SEED, R, rnd))
    return np.random.default_rng(seed).normal(-300.0, 2.0, R).astype(np.float32)


# ---- specials -----------------------------------------------------------------------------------------------------------------
SPECIALS = ("nan", "+inf", "-inf", "over709")


def special_positions(R):
    return sorted({p for p in (62, 63, 64, 65, R - 1) if 1 <= p <= R - 1})


def special_next(R, kind, p):
    """The special is L[p], the right-hand scalar L[k+1] of pair k = p - 1, on the ladder that otherwise drops every odd pair.
    over709: L[p] lies 1000 above its neighbours (the carried state is at most 100 below them), so d > 709 and the clamp binds."""
    L = scripted(R, [k for k in range(R - 1) if k & 1])
    L[p] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "over709": L[p] + np.float32(1000.0)}[kind]
    return L


def special_carried(R, kind, p):
    """The special is the carried L[c] when the scan reaches pair p - 1 and, where it is not dropped there, beyond it into the next
    window.  A pair whose right-hand scalar is NaN, +inf or far above always swaps, so such a state is never PICKED UP in the middle
    of the ladder; what can be carried there is
      -inf     picked up at slot p (pair p - 1 drops the carried state onto it): every later pair has d = +inf -> 709 and swaps;
      over709  a scalar 1000 below everything else, picked up at slot p the same way: every later d is above 709;
      +inf     carried from slot 0 over L[1 .. p-1] = +inf (d = NaN -> 709: swap) and dropped at pair p - 1, where L[p] is finite
               (d = -inf); behind it the ladder drops every odd pair;
      nan      carried from slot 0 to the end (every d is NaN -> 709), over a ladder that would otherwise drop every odd pair."""
    odd = [k for k in range(R - 1) if k & 1]
    if kind == "-inf":
        L = scripted(R, [p - 1])
        L[p] = -np.inf
    elif kind == "over709":
        L = scripted(R, [p - 1])
        L[p] = L[p] - np.float32(1000.0)
    elif kind == "+inf":
        L = scripted(R, odd)
        L[:p] = np.inf
    else:
        L = scripted(R, odd)
        L[0] = np.nan
    return L


def cases(R, rnd):
    """Every case of the kernel-alone test at (R, round): list of (name, L float32 [R], drops or None).  drops: the pairs where the
    carried state must be dropped whatever the uniforms (scripted cases); None: the oracle decides."""
    out = [("scripted-" + name, scripted(R, s), s) for name, s in drop_sets(R).items()]
    out.append(("ties", ties(R), None))
    out.append(("normal", normal_draw(R, rnd), None))
    for kind in SPECIALS:
        for p in special_positions(R):
            out.append((f"{kind}-next-{p}", special_next(R, kind, p), None))
            if kind != "nan":
                out.append((f"{kind}-carried-{p}", special_carried(R, kind, p), None))
        if kind == "nan":
            out.append(("nan-carried-0", special_carried(R, kind, 1), None))
    return out


# ---- margins ------------------------------------------------------------------------------------------------------------------
def _spacing32(x):
    return float(np.spacing(np.float32(x)))


def margin(L, u, dL=None):
    """The oracle's pass over (k, c) -> the smallest |ln(2 u_k) - min(709, L[k+1] - L[c])| over the pairs with a finite right-hand
    side, in units of the fp32 spacing at max(|rhs|, |ln 2u|, 1).  dL (optional, [R]): an absolute uncertainty of every scalar as
    handed in (a scalar reconstructed from a rounded product, not read); it is taken off the distance before the division."""
    L = [float(v) for v in L]
    src, _ = orc.swap_cascade(L, u)
    worst, c = math.inf, 0
    for k in range(len(L) - 1):
        d = L[k + 1] - L[c]
        rhs = 709.0 if not (d < 709.0) else d
        if math.isfinite(rhs):
            t = math.log(2.0 * float(u[k]))
            dist = abs(t - rhs) - (0.0 if dL is None else float(dL[k + 1]) + float(dL[c]))
            worst = min(worst, dist / _spacing32(max(abs(rhs), abs(t), 1.0)))
        if src[k] != k + 1:
            assert src[k] == c
            c = k + 1
    return worst


def rule1_round(Lraw, T, u, rnd):
    """The oracle's even/odd round (PTOracle.swap_round_even_odd) on given untempered log-likelihoods and temperatures:
    -> (src, accepted swaps)."""
    R = len(Lraw)
    src = list(range(R))
    nsw = 0
    for k in range(rnd & 1, R - 1, 2):
        d = (1.0 / float(T[k]) - 1.0 / float(T[k + 1])) * (float(Lraw[k + 1]) - float(Lraw[k]))
        p = 1.0 if d != d else min(1.0, math.exp(min(d, 80.0)))
        if u[k] < p:
            src[k], src[k + 1] = k + 1, k
            nsw += 1
    return src, nsw


def rule1_margin(Lraw, T, u, rnd):
    """Smallest |u_k - p| / p over the round's pairs with d < 0, in units of the a-priori relative fp32 error e_p of p (module
    docstring).  T: the temperatures the device holds (fp32 values)."""
    worst = math.inf
    e = 2.0 ** -23
    for k in range(rnd & 1, len(Lraw) - 1, 2):
        a, b = 1.0 / float(T[k]), 1.0 / float(T[k + 1])
        g = a - b
        d = g * (float(Lraw[k + 1]) - float(Lraw[k]))
        if not d < 0.0:
            continue
        e_g = (_spacing32(a) + _spacing32(b) + 0.5 * _spacing32(abs(g))) / abs(g)
        e_p = abs(d) * (e_g + 2.0 * e) + e
        p = math.exp(d)
        worst = min(worst, abs(float(u[k]) - p) / p / e_p)
    return worst


# ---- the ballot scan, restated ------------------------------------------------------------------------------------------------
_ALL = (1 << WAVE) - 1


def ballot_scan(L, u, mutant=None):
    """NumPy restatement of the rule-0 branch of cascade_lds_prefix: wave 0 takes the pairs 64 at a time, a ballot finds the first
    pair where the carried state is dropped, the next state's L is picked up from that lane, (c, Lc) are carried from one window
    into the next.  fp32 subtraction and compare; ln(2 u) is the float64 logarithm rounded to fp32.  -> (src[R], accepted swaps).
    mutant: one of MUTANTS, a defect the cases must notice (tests/test_swap_cases_cpu.py):
      no_j63_case         the mask update ~((1 << (j + 1)) - 1) without the j == 63 case, the shift count taken modulo 64 as the
                          hardware takes it: after a drop at lane 63 nothing is cleared (the scan gives up after 128 turns);
      lc_not_carried      Lc is set to L[0] again at the head of every window (c is kept);
      stale_lc_at_lane0   a drop at lane 63 ends the window before Lc is picked up: the next window's lanes meet the old Lc;
      dead_lanes_counted  the partial last window's dead lanes (L = 0, ln 2u = 0) take part in the ballots."""
    assert mutant is None or mutant in MUTANTS, mutant
    L = np.asarray(L, dtype=np.float32)
    R = len(L)
    with np.errstate(all="ignore"):
        lnu = np.log(2.0 * np.asarray(u, dtype=np.float64)).astype(np.float32)
    src = np.full(R + WAVE + 1, -1, dtype=np.int64)          # room for what a mutant writes past the ladder
    lanes = np.arange(WAVE)
    c, nsw, Lc = 0, 0, L[0]
    for k0 in range(0, R - 1, WAVE):
        k = k0 + lanes
        valid = k < R - 1
        Ln = np.where(valid, L[np.minimum(k + 1, R - 1)], np.float32(0.0)).astype(np.float32)
        tk = np.where(valid, lnu[np.minimum(k, R - 2)], np.float32(0.0)).astype(np.float32)
        if mutant == "lc_not_carried":
            Lc = L[0]
        todo = _ALL if mutant == "dead_lanes_counted" else int(sum(1 << int(j) for j in lanes[valid]))
        swapped, turns = 0, 0
        while todo:
            turns += 1
            if turns > 2 * WAVE:
                break
            with np.errstate(all="ignore"):
                d = (Ln - Lc).astype(np.float32)
            d = np.where(d < np.float32(709.0), d, np.float32(709.0))
            fail = int(sum(1 << int(j) for j in lanes[~(tk < d)])) & todo
            if not fail:
                swapped |= todo
                break
            j = (fail & -fail).bit_length() - 1
            swapped |= todo & ((1 << j) - 1)
            src[k0 + j] = c
            c = k0 + j + 1
            if mutant == "stale_lc_at_lane0" and j == WAVE - 1:
                todo = 0
                break
            Lc = Ln[j]
            if mutant == "no_j63_case":
                todo &= ~((1 << ((j + 1) % WAVE)) - 1) & _ALL
            else:
                todo &= 0 if j == WAVE - 1 else ~((2 << j) - 1) & _ALL
        for j in lanes[valid]:
            if (swapped >> int(j)) & 1:
                src[k0 + int(j)] = k0 + int(j) + 1
        nsw += bin(swapped).count("1")
    src[R - 1] = c
    return [int(v) for v in src[:R]], nsw


# ---- the rounds of a finished run, replayed from its traces -----------------------------------------------------------------------
def handoff_steps(task, S, si):
    """The MH steps after which a swap round runs (Q10)."""
    return [i for i in range(S - 1) if orc.swap_trigger(task, i, si)]


def accepted_steps(accept, num_accepted):
    """accept [R, S]: accept_list (row i + 1 = accepted steps BEFORE step i); num_accepted [R]: the final counters -> bool [R, S-1]."""
    acc = np.asarray(accept).astype(np.int64)
    R, S = acc.shape
    dec = np.empty((R, S - 1), dtype=np.int64)
    dec[:, :S - 2] = acc[:, 2:] - acc[:, 1:S - 1]
    dec[:, S - 2] = np.asarray(num_accepted, dtype=np.int64) - acc[:, S - 1]
    assert set(np.unique(dec).tolist()) <= {0, 1}, "the accept counters are no step function"
    return dec.astype(bool)


def _tempered(task, likeh_row, T, dtype):
    """The likelihood a slot holds after the accepted step that wrote likeh_row, and how well it is known.  REG records the
    tempered likelihood itself (REG:391); CLS records likelihood * T (CLS:404): it is divided out again, which leaves the two
    roundings of product (half an ulp of the record, up to one ulp of the quotient) and quotient (half an ulp): 1.5 ulp."""
    if task == orc.TASK_REG:
        return dtype(likeh_row), 0.0
    v = dtype(dtype(likeh_row) / dtype(T))
    return v, 1.5 * float(np.spacing(np.abs(v)))


def replay_rule0(task, T, likeh, accept, num_accepted, lik0, S, si, dtype=np.float32):
    """The scalars every rule-0 round of a finished run decided on, from the run's own traces (Q11, Q12, Q13).  A slot keeps the
    likelihood of the last proposal IT accepted (a swap moves (w, eta) only), from lik0 [R] (the start-up likelihood) on.
      hand-off rounds: REG posts likelihood * T, one product in `dtype`; CLS posts the tempered likelihood;
      phantom round (int(S / si) rounds are counted): the final tempered likelihood, from the state after step S - 2.
    T [R] temperatures as the run holds them, likeh / accept [R, S] the traces, num_accepted [R] the final counters.
    dtype float32 replays the device's arithmetic bit for bit (regression); float64 the oracle's.
    -> list of (L [R], dL [R] absolute uncertainty, phantom)."""
    dec = accepted_steps(accept, num_accepted)
    R = dec.shape[0]
    lik = [dtype(v) for v in lik0]
    unc = [0.0] * R
    out, done = [], 0

    def advance(upto):                                       # steps done .. upto inclusive
        for r in range(R):
            for i in range(done, upto + 1):
                if dec[r, i]:
                    lik[r], unc[r] = _tempered(task, likeh[r][i + 1], T[r], dtype)
    for i in handoff_steps(task, S, si):
        advance(i)
        done = i + 1
        if task == orc.TASK_REG:
            L = [dtype(lik[r] * dtype(T[r])) for r in range(R)]
            dL = [unc[r] * float(T[r]) for r in range(R)]
        else:
            L, dL = list(lik), list(unc)
        out.append((np.array(L, dtype=dtype), np.array(dL), False))
    if si > 0 and int(S / si) > len(out):
        advance(S - 2)
        out.append((np.array(lik, dtype=dtype), np.array(unc), True))
    return out


def replay_rule1(T, likeh, accept, num_accepted, lik0, S, si, tape, dtype=np.float32, src_log=None, final=None):
    """The even/odd rounds of a finished regression run that never reaches the temperature switch: per round the untempered
    log-likelihoods Lr = likelihood * T it decided on (post_raw in csrc/ptnn_dev_sweep_forward.hpp), in `dtype`.  A moved state brings
    its likelihood along, re-tempered for its new slot: likelihood = Lr[src] / T (swap_block).  The permutation applied after each
    round is src_log's (the device's own log) or, without one, the oracle's rule on these scalars.  final: a list that receives the
    likelihood every slot holds after the last step.  -> list of Lr [R]."""
    dec = accepted_steps(accept, num_accepted)
    R = dec.shape[0]
    lik = [dtype(v) for v in lik0]
    out, done = [], 0
    for n, i in enumerate(handoff_steps(orc.TASK_REG, S, si)):
        for r in range(R):
            for j in range(done, i + 1):
                if dec[r, j]:
                    lik[r] = dtype(likeh[r][j + 1])
        done = i + 1
        Lr = [dtype(lik[r] * dtype(T[r])) for r in range(R)]
        out.append(np.array(Lr, dtype=dtype))
        src = src_log[n] if src_log is not None else rule1_round(Lr, T, tape.swap_uniforms(n, R - 1), n)[0]
        for k in range(R):
            if int(src[k]) != k:
                lik[k] = dtype(Lr[int(src[k])] / dtype(T[k]))
    if final is not None:
        for r in range(R):
            for j in range(done, S - 1):
                if dec[r, j]:
                    lik[r] = dtype(likeh[r][j + 1])
        final.extend(lik)
    return out


def check_rounds(rounds, log, tape, label=""):
    """Every replayed rule-0 round against the device's swap log: log[n] must equal orc.swap_cascade on the round's scalars and
    uniforms wherever the round's margin is at least MARGIN_UNITS; a round below it is skipped, at most one in ten.
    -> (accepted swaps over all rounds: the oracle's where it was held, the log's own elsewhere; worst margin; skipped rounds)."""
    assert len(log) == len(rounds), (label, len(log), len(rounds))
    nsw_total, worst, skipped = 0, math.inf, []
    for n, (L, dL, _) in enumerate(rounds):
        R = len(L)
        u = tape.swap_uniforms(n, R - 1)
        m = margin(L, u, dL)
        got = [int(v) for v in log[n]]
        if m < MARGIN_UNITS:
            skipped.append(n)
            nsw_total += sum(1 for k in range(R - 1) if got[k] == k + 1)
            continue
        worst = min(worst, m)
        src, nsw = orc.swap_cascade([float(v) for v in L], u)
        assert got == src, f"{label}round {n} (margin {m:.3g} units): first difference at slot {next(k for k in range(R) if got[k] != src[k])}"
        nsw_total += nsw
    assert 10 * len(skipped) <= len(rounds), f"{label}rounds {skipped} of {len(rounds)} below the margin"
    return nsw_total, worst, skipped
