"""Host side of the drop-in: the public surface of the reference's `ParallelTempering` class.

Reference: REG = multicore-pt-regression/pt_timeseries_regression.py:487-875,
           CLS = multicore-pt-classification/pt_classification.py:497-897.

What `main()` touches (REG:995-1007, CLS:1080-1092) is kept: the constructor arguments, `make_directory`,
`initialize_chains(burn_in)`, `run_chains()` with its 11-tuple, the attributes `num_swap`,
`total_swap_proposals`, `temperatures`, `NumSamples`, `num_param`, and every file under `path`
(SURVEY.md section 8b).  What happens in between -- one forked process per replica, queues and events --
is replaced by libptnn.so: all replicas advance inside one HIP kernel -- one launch for the whole run with the
swap cascade inside it where every work-group is resident, else one launch per swap interval with the cascade
as a second kernel; this module only configures the run, fetches the traces and writes the files.
"""
import math
import os
import shutil
import tempfile
import time
import warnings
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, ladder, philox

TASK_REG, TASK_CLS = _lib.TASK_REG, _lib.TASK_CLS


def _text_round(a, fmt, threads=8):
    """Values as np.loadtxt would read them back from np.savetxt(..., fmt=fmt) (show_results re-reads the files)."""
    return _lib.text_round(a, fmt, threads)


def stitch_by_temperature(tr, swap_log, handoff_steps, S):
    """Label swapping: the device records trace rows per chain slot and a slot's temperature changes at the swap rounds.  Row
    i + 1 is written by MH step i, so the rows up to the hand-off step + 1 belong to the assignment before the round; round k
    hands temperature t to the chain that held temperature swap_log[k][t].  -> (traces keyed by temperature, final holder[t])."""
    R = next(v for v in tr.values() if v is not None).shape[0]
    holder = np.arange(R)                                    # holder[t] = slot whose chain holds temperature t
    out = {k: (None if v is None else np.empty_like(v)) for k, v in tr.items()}
    row0 = 0
    for k, i_k in enumerate(list(handoff_steps) + [None]):
        row1 = S if i_k is None else i_k + 2
        for key, v in tr.items():
            if v is not None:
                out[key][:, row0:row1] = v[holder, row0:row1]
        if i_k is None:
            break
        holder = holder[np.asarray(swap_log[k])]
        row0 = row1
    return out, holder


def ladder_stats_from_log(src_log, rule, first_round, n_moves=None):
    """Per-pair swap acceptance and round trips of the walkers from a swap log (Sampler.swap_log(): row r = src of round r, slot k
    received the state / label of slot src[k]), over rounds first_round .. n_moves - 1 (n_moves None = every row; a rule-0 run
    that ended with the phantom round passes the number of hand-off rounds, the phantom moves nothing).  Pair k is proposed in
    every round under rule 0 and in the rounds of its parity (k % 2 == r % 2) under rule 1, and accepted when src[k] == k + 1.
    A walker (a state under state moves, a chain under label swapping) at index j goes to the k with src[k] == j; a round trip
    is index 0 -> R-1 -> 0, timed from its last visit of 0 before it reached R-1.
    -> dict(pair_accept [R-1] (NaN where nothing was proposed), accepted [R-1], proposed [R-1], round_trips [R] (per walker,
    walker w starts at index w), mean_round_trip_rounds (NaN without a trip))."""
    log = np.asarray(src_log, dtype=np.int64)
    if log.ndim != 2 or log.shape[1] < 2:
        raise ValueError(f"src_log must be [rounds, R >= 2], got shape {log.shape}")
    if int(rule) not in (0, 1):
        raise ValueError(f"rule must be 0 or 1, got {rule}")
    n = log.shape[0] if n_moves is None else min(int(n_moves), log.shape[0])
    R = log.shape[1]
    k = np.arange(R - 1)
    acc = np.zeros(R - 1, np.int64)
    prop = np.zeros(R - 1, np.int64)
    pos = np.arange(R)                          # pos[w] = index of walker w
    state = np.zeros(R, np.int64)               # 0: not at 0 yet, 1: left 0 heading up, 2: reached R-1 heading down
    start = np.zeros(R, np.int64)
    trips = np.zeros(R, np.int64)
    durations = []
    first = int(first_round)

    def visit(r):
        for w in range(R):
            if pos[w] == 0:
                if state[w] == 2:
                    trips[w] += 1
                    durations.append(r - start[w])
                state[w], start[w] = 1, r
            elif pos[w] == R - 1 and state[w] == 1:
                state[w] = 2
    for r in range(n):
        src = log[r]
        if r >= first:
            if r == first:
                visit(r)                        # where the walkers stand when the counting starts
            on = np.ones(R - 1, bool) if int(rule) == 0 else (k % 2 == r % 2)
            prop += on
            acc += on & (src[:-1] == k + 1)
        inv = np.empty(R, np.int64)
        inv[src] = np.arange(R)                 # the walker at index j moves to the k with src[k] == j
        pos = inv[pos]
        if r >= first:
            visit(r + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pa = np.where(prop > 0, acc / np.maximum(prop, 1), np.nan)
    return dict(pair_accept=pa, accepted=acc, proposed=prop, round_trips=trips,
                mean_round_trip_rounds=float(np.mean(durations)) if durations else float("nan"))


LADDER_KAPPA0, LADDER_T0 = 0.05, 1000.0  # defaults of adapt_ladder=True (measured: DESIGN.md section 16, profiles/ladder_probe_effect.jsonl)


def overlap_cuts(S, swap_interval, chunks):
    """MH-step counts at which an overlapped run_chains() ends its launches: at most `chunks` launches of whole swap intervals
    (near-equal), strictly increasing, the last one at S - 1 (all steps; ptnn_run then also runs the phantom round if one is due)."""
    si = max(1, int(swap_interval))
    n_int = max(1, (S - 1) // si)
    K = max(1, min(int(chunks), n_int))
    return sorted({min(S - 1, si * max(1, round(n_int * (c + 1) / K))) for c in range(K - 1)} | {S - 1})


def percentile_ranks(n, percentiles):
    """np.percentile(..., method="linear") of n values reduced to ranks: for each percentile p the two 0-based ranks of the sorted
    values it interpolates between and its weight gamma, with numpy 2.x's arithmetic (q = p / 100, virtual index (n - 1) q, floor,
    clamped to [0, n - 1]).  -> list of (lo, hi, gamma)."""
    out = []
    for p in percentiles:
        q = np.true_divide(np.float64(p), np.float64(100))
        vi = np.float64(n - 1) * q
        lo = np.floor(vi)
        gamma = vi - lo
        if vi >= n - 1:
            lo_i = hi_i = n - 1
        elif vi < 0:
            lo_i = hi_i = 0
        else:
            lo_i, hi_i = int(lo), int(lo) + 1
        out.append((lo_i, hi_i, gamma))
    return out


def lerp_percentile(a, b, gamma):
    """numpy's _lerp of the order statistics a (rank lo) and b (rank hi), float64, including its t >= 0.5 branch."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    diff = np.subtract(b, a)
    res = np.add(a, diff * gamma)
    if gamma >= 0.5:
        res = np.subtract(b, diff * (1 - gamma))
    return res


# posterior_predictive's result: mean [n_rows, n_out] float64; percentiles {p: [n_rows, n_out] float64}; vote [n_rows, n_out] and
# pred_class [n_rows] (classification, else None); samples [n_samples, n_rows, n_out] float32 or None; n_samples; n_distinct
Predictive = namedtuple("Predictive", "mean percentiles vote pred_class samples n_samples n_distinct")


# input_sensitivity's result, g = d output / d input: grad_mean, percentiles {p: ...}, prob_positive, prob_negative [n_rows, n_out,
# n_in] float64; importance (mean over samples and rows of |g|), importance_rms, importance_percentiles {p: ...}, top_prob (the share
# of the samples in which the input is the output's most important one) [n_out, n_in] float64; samples [n_samples, n_rows, n_out,
# n_in] float32 or None; n_samples; n_distinct
Sensitivity = namedtuple("Sensitivity", "grad_mean percentiles prob_positive prob_negative importance importance_rms "
                         "importance_percentiles top_prob samples n_samples n_distinct")


def top_share(a, counts=None):
    """a [n, n_out, n_in]: per sample and output a non-negative score of every input; counts [n]: integer multiplicities (None = 1
    each).  -> [n_out, n_in] float64: the share of the expanded samples in which input i has the largest score of output o
    (np.argmax: the first index on a tie)."""
    a = np.asarray(a)
    n, O, I = a.shape
    c = np.ones(n, np.int64) if counts is None else np.asarray(counts, dtype=np.int64).reshape(n)
    best = np.argmax(a, axis=2)                                  # [n, n_out]
    hits = np.zeros((O, I), np.int64)
    for o in range(O):
        hits[o] = np.bincount(best[:, o], weights=None if counts is None else c, minlength=I).astype(np.int64)
    return hits / np.float64(c.sum())


# convergence_diagnostics' result: names [Q]; mean, sd, r_hat, ess, mcse_mean [Q] float64; ess_chain [n_chains, Q] or None; rho
# [n_lags, Q] or None; trunc_lag [Q] int32; n_chains, n_draws
Convergence = namedtuple("Convergence", "names mean sd r_hat ess mcse_mean ess_chain rho trunc_lag n_chains n_draws")

# predictive_accuracy's result: totals elpd_loo, se_elpd_loo, p_loo, elpd_waic, se_elpd_waic, p_waic, lppd, se_lppd (float);
# pointwise lppd_i, elpd_loo_i, p_waic_i, khat [n_rows] float64; good_k (the k-hat threshold for this S); n_high_k (rows above
# it); log_lik [n_samples, n_rows] float64 or None; n_samples; n_distinct
PredictiveAccuracy = namedtuple("PredictiveAccuracy", "elpd_loo se_elpd_loo p_loo elpd_waic se_elpd_waic p_waic lppd se_lppd "
                                "lppd_i elpd_loo_i p_waic_i khat good_k n_high_k log_lik n_samples n_distinct")


# forecast's result: mean [n_origins, horizon] float64; percentiles {p: [n_origins, horizon] float64}; samples [n_samples,
# n_origins, horizon] float32 or None; n_samples; n_trajectories (per origin)
Forecast = namedtuple("Forecast", "mean percentiles samples n_samples n_trajectories")

# log_evidence's result: the stepping-stone and thermodynamic-integration estimates of log Z with their standard errors
# (float); ti_discretisation (float); betas [K+1] ascending, 0 first (the prior); u_mean, u_mcse, ess [K+1] (entry 0: the prior's
# self-normalised mean of U, its MCSE and Kish ESS); log_stones [K] (stone k takes beta_k to beta_{k+1}, stone 0 from the prior);
# prior_kish_ess (of the first stone's weights); n_draws [K+1] (entry 0: prior draws); n_distinct; u_draws [K] arrays of every
# rung's U draws and u_prior_draws [n_prior] (return_draws) or None
Evidence = namedtuple("Evidence", "log_z_ss se_log_z_ss log_z_ti se_log_z_ti ti_discretisation betas u_mean u_mcse ess log_stones "
                      "prior_kish_ess n_draws n_distinct u_draws u_prior_draws")


def evidence_log_c(task, n_rows):
    """The constant of the evidence: 0 for a classification; for a regression, whose eta = log tau^2 is
    integrated out of the improper 1 / tau^2 prior, log 2 + lgamma(N / 2 + 1) - (N / 2) log pi over N training rows."""
    if task == TASK_CLS:
        return 0.0
    n = float(n_rows)
    return math.log(2.0) + math.lgamma(n / 2.0 + 1.0) - (n / 2.0) * math.log(math.pi)


def _trapezoid(b, u):
    """Trapezoid weights over the points b (ascending) and the integral sum w_k u_k."""
    w = np.zeros(b.size)
    d = np.diff(b)
    w[:-1] += d / 2.0
    w[1:] += d / 2.0
    return w, float(np.dot(w, u))


def evidence_from_rungs(betas, u_mean, u_var, ess, log_stones, stone_relvar, *, prior_log_mean_exp_b, prior_u_mean, prior_u_var,
                        prior_kish_ess_b, prior_log_mean_exp_first, prior_kish_ess_first, n_prior, log_c=0.0):
    """log Z from per-rung statistics; host arithmetic only.

    betas [K] ascending with betas[-1] == 1; per rung: u_mean, u_var (ddof 1), ess of its U draws; log_stones[k] = log mean
    exp((betas[k+1] - betas[k]) U) over rung k's draws and stone_relvar[k] the relative variance of those exp-terms (entry K-1
    unused).  The prior (beta = 0) from n_prior independent draws: prior_log_mean_exp_b = log E[e^b], prior_u_mean / prior_u_var
    the mean and variance of U weighted by e^b with Kish ESS prior_kish_ess_b; prior_log_mean_exp_first = log E[e^{b + betas[0]
    U}] with Kish ESS prior_kish_ess_first.  Returns dict(log_z_ti, se_log_z_ti, ti_discretisation, log_z_ss, se_log_z_ss,
    betas, u_mean, u_mcse, ess) with the prior prepended to the last four."""
    b = np.asarray(betas, np.float64).reshape(-1)
    K = b.size
    if K < 1 or b[-1] != 1.0 or b[0] <= 0.0 or np.any(np.diff(b) <= 0.0):
        raise ValueError(f"betas must rise strictly from above 0 to exactly 1, got {b}")
    um, uv, es = (np.asarray(v, np.float64).reshape(-1) for v in (u_mean, u_var, ess))
    ls, rv = np.asarray(log_stones, np.float64).reshape(-1), np.asarray(stone_relvar, np.float64).reshape(-1)
    n = float(n_prior)
    # the prior's point: a self-normalised mean of U, and log E[e^b] (independent draws: Kish ESS; var of a log-mean = 1/kish - 1/n)
    bb = np.concatenate([[0.0], b])
    uu = np.concatenate([[float(prior_u_mean)], um])
    # a rung whose draws are all equal has variance 0 and no ESS (NaN): its term is known exactly; a rung whose split halves are
    # each constant has no finite ESS either: it counts as one draw
    ed = np.where(np.isfinite(es) & (es > 0.0), es, 1.0)
    var_mean = np.concatenate([[float(prior_u_var) / float(prior_kish_ess_b)], np.where(uv > 0.0, uv / ed, 0.0)])
    var_stones = np.where(rv[:K - 1] > 0.0, rv[:K - 1] / ed[:K - 1], 0.0)
    w, integral = _trapezoid(bb, uu)
    var_lme_b = max(1.0 / float(prior_kish_ess_b) - 1.0 / n, 0.0)
    log_z_ti = float(log_c) + float(prior_log_mean_exp_b) + integral
    se_ti = math.sqrt(var_lme_b + float(np.dot(w * w, var_mean)))
    keep = np.zeros(K + 1, bool)                         # every other point, both ends kept
    keep[::2] = True
    keep[-1] = True
    _, integral_half = _trapezoid(bb[keep], uu[keep])
    disc = abs(integral - integral_half)
    # stepping stones: the first from the prior, stone k (k < K - 1) from rung k's draws
    var_first = max(1.0 / float(prior_kish_ess_first) - 1.0 / n, 0.0)
    log_z_ss = float(log_c) + float(prior_log_mean_exp_first) + float(np.sum(ls[:K - 1]))
    se_ss = math.sqrt(var_first + float(np.sum(var_stones)))
    return dict(log_z_ti=log_z_ti, se_log_z_ti=se_ti, ti_discretisation=disc, log_z_ss=log_z_ss, se_log_z_ss=se_ss, betas=bb,
                u_mean=uu, u_mcse=np.sqrt(var_mean), ess=np.concatenate([[float(prior_kish_ess_b)], es]))


def evidence_compare(a, b):
    """The log Bayes factor of two Evidence results, log Z_a - log Z_b, with SE sqrt(se_a^2 + se_b^2) (independent runs; for a
    regression both must be fitted to the same training rows).  -> dict(log_bf_ss, se_log_bf_ss, log_bf_ti, se_log_bf_ti)."""
    return dict(log_bf_ss=float(a.log_z_ss - b.log_z_ss), se_log_bf_ss=math.hypot(a.se_log_z_ss, b.se_log_z_ss),
                log_bf_ti=float(a.log_z_ti - b.log_z_ti), se_log_bf_ti=math.hypot(a.se_log_z_ti, b.se_log_z_ti))


def _se_total(x):
    """Standard error of a sum of pointwise values: sqrt(N var(x, ddof 1)) (Vehtari, Gelman & Gabry 2017, eq. 23)."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(x.size * np.var(x, ddof=1))) if x.size > 1 else float("nan")


def elpd_compare(a, b):
    """The elpd difference of two results on the same data, a - b, with the paired standard error sqrt(N var(a_i - b_i, ddof 1)).
    Two PredictiveAccuracy results over the same rows -> dict(elpd_loo_diff, se_loo_diff, elpd_waic_diff, se_waic_diff); two
    LeaveFutureOut results over equal origins and block -> dict(elpd_lfo_diff, se_lfo_diff).  A mix of the two is refused: a
    leave-one-out and a leave-future-out score answer different questions.  Host arithmetic only."""
    lfo_a, lfo_b = isinstance(a, LeaveFutureOut), isinstance(b, LeaveFutureOut)
    if lfo_a != lfo_b:
        raise ValueError("elpd_compare needs two results of one kind: a LeaveFutureOut cannot be compared with a PredictiveAccuracy")
    if lfo_a:
        if a.block != b.block:
            raise ValueError(f"the two results score different blocks: block = {a.block} vs {b.block}")
        if not np.array_equal(np.asarray(a.origins), np.asarray(b.origins)):
            raise ValueError(f"the two results cover different origins: {len(a.origins)} vs {len(b.origins)} (or other rows)")
        da = np.asarray(a.elpd_lfo_i, np.float64) - np.asarray(b.elpd_lfo_i, np.float64)
        return dict(elpd_lfo_diff=float(np.sum(a.elpd_lfo_i) - np.sum(b.elpd_lfo_i)), se_lfo_diff=_se_total(da))
    la, lb = np.asarray(a.elpd_loo_i, np.float64), np.asarray(b.elpd_loo_i, np.float64)
    if la.shape != lb.shape:
        raise ValueError(f"the two results cover different rows: {la.shape[0]} vs {lb.shape[0]}")
    wa = np.asarray(a.lppd_i, np.float64) - np.asarray(a.p_waic_i, np.float64)
    wb = np.asarray(b.lppd_i, np.float64) - np.asarray(b.p_waic_i, np.float64)
    return dict(elpd_loo_diff=float(np.sum(la) - np.sum(lb)), se_loo_diff=_se_total(la - lb),
                elpd_waic_diff=float(np.sum(wa) - np.sum(wb)), se_waic_diff=_se_total(wa - wb))


# leave_future_out's result: totals elpd_lfo, se_elpd_lfo (float; sqrt(n var(pointwise, ddof 1)) over the origins); per origin
# (ascending) elpd_lfo_i, khat [n] float64, tail_len [n] int64, origins [n], fit_origin [n] (the fit that scored it: the rows
# [0, fit_origin) it had seen), exact [n] bool (fit_origin == origin: no importance weights); refit_origins (in walk order);
# n_refits; k_threshold; n_samples (of the first fit); block
LeaveFutureOut = namedtuple("LeaveFutureOut", "elpd_lfo se_elpd_lfo elpd_lfo_i khat tail_len origins fit_origin exact refit_origins "
                            "n_refits k_threshold n_samples block")


def good_k(n_samples):
    """The k-hat threshold of DESIGN.md section 13 for S samples: min(1 - 1 / log10(S), 0.7)."""
    return min(1.0 - 1.0 / math.log10(n_samples), 0.7)


def lfo_refit_seed(seed, origin):
    """The seed of the sampler leave_future_out() refits on rows [0, origin): a function of the object's seed and the origin."""
    return (int(seed) + 0x9E3779B97F4A7C15 * (int(origin) + 1)) % (1 << 64)


def lfo_walk(origins, n_fit, first_fit, score, fit=None, *, k_threshold, max_refits=None):
    """The walk of approximate leave-future-out cross-validation (Buerkner, Gabry & Vehtari 2020, algorithm 1), in both
    directions.  `first_fit` has seen rows [0, n_fit).  Origins >= n_fit are walked forward (ascending) from it, origins < n_fit
    backward (descending); each walk begins again at `first_fit`.  score(fit_object, its n_fit, origins) -> dict(elpd_lfo, khat,
    tail_len) scores all remaining origins from the current fit; the origins before the first one (in walk order) whose khat
    exceeds k_threshold (+inf, the khat of a tail of <= 4 samples, does; the origin at the fit itself is exact) are kept.  With fit(origin) -> fit_object (None: never refit) a fit on rows [0, origin) replaces the
    current one, scores that origin exactly and the walk goes on from there; after `max_refits` refits (None = no bound) the
    remaining origins are kept as scored, high khat included.  Needs no GPU: the two callables do the work.
    -> dict(origins (ascending, repeats removed), elpd_lfo, khat, tail_len, fit_origin, exact, refit_origins, n_refits,
    max_refits_hit)."""
    og = sorted({int(i) for i in np.asarray(origins).reshape(-1)})
    if not og:
        raise ValueError("no origin to score")
    if max_refits is not None and max_refits < 0:
        raise ValueError(f"max_refits = {max_refits} must be >= 0 (or None)")
    res = {i: None for i in og}
    refit_origins = []
    hit = False
    for order in ([i for i in og if i >= n_fit], [i for i in reversed(og) if i < n_fit]):
        cur, cur_fit, rest = first_fit, int(n_fit), order
        while rest:
            out = score(cur, cur_fit, rest)
            kh = np.asarray(out["khat"], np.float64)
            # +inf (a tail of <= 4 samples: raw weights, nothing to diagnose them by) exceeds every threshold, as does NaN;
            # only the origin at the fit itself, whose weights are uniform, is exact whatever its khat says
            high = np.flatnonzero(~(kh <= k_threshold) & (np.asarray(rest) != cur_fit))
            stop = int(high[0]) if high.size else len(rest)
            can_refit = fit is not None and stop < len(rest) and (max_refits is None or len(refit_origins) < max_refits)
            if stop < len(rest) and fit is not None and not can_refit:
                hit = True
            keep = stop if can_refit else len(rest)
            for k in range(keep):
                res[rest[k]] = (float(out["elpd_lfo"][k]), float(kh[k]), int(out["tail_len"][k]), cur_fit)
            if not can_refit:
                break
            rest = rest[stop:]
            cur_fit = rest[0]
            cur = fit(cur_fit)
            refit_origins.append(cur_fit)
    fit_origin = np.array([res[i][3] for i in og], np.int64)
    oa = np.array(og, np.int64)
    return dict(origins=oa, elpd_lfo=np.array([res[i][0] for i in og]), khat=np.array([res[i][1] for i in og]),
                tail_len=np.array([res[i][2] for i in og], np.int64), fit_origin=fit_origin, exact=fit_origin == oa,
                refit_origins=refit_origins, n_refits=len(refit_origins), max_refits_hit=hit)


def lfo_origins(n_rows, n_fit, block, min_train=None):
    """The origins leave_future_out() scores: min_train .. n_rows - block.  min_train=None: n_fit when rows follow the fit
    (the sequential score of the rows after it), else n_rows // 2.  Refusals that need no GPU."""
    if block < 1:
        raise ValueError(f"block = {block} must be >= 1")
    if not 0 < n_fit <= n_rows:
        raise ValueError(f"n_fit = {n_fit} outside [1, {n_rows}]: the fit has seen rows [0, n_fit) of the {n_rows} rows")
    L = (n_fit if n_fit < n_rows else n_rows // 2) if min_train is None else int(min_train)
    if L < 1:
        raise ValueError(f"min_train = {L} must be >= 1: an origin predicts from the rows before it")
    if L + block > n_rows:
        raise ValueError(f"min_train = {L} with block = {block} leaves no origin: i + block must be <= {n_rows} rows")
    return np.arange(L, n_rows - block + 1, dtype=np.int64)


# predictive_calibration's result.  Regression: crps, se_crps (float; None with crps=False); crps_i, pit, pred_mean, pred_sd
# [n_rows] float64; pit_hist [bins] counts of the PIT in equal-width bins of (0, 1); coverage {level: share of rows inside the
# central interval of that level}; quantiles {p: [n_rows]}; intervals {(p_lo, p_hi): dict(level, width, score)} for every
# symmetric pair of quantiles.  Classification: brier, log_score (means), brier_i, log_score_i [n_rows]; p_mean [n_rows, n_out];
# confidence, correct [n_rows]; reliability dict(edges, count, confidence, accuracy) over `bins` confidence bins; ece, mce.
# What does not apply to the task is None.  n_samples; n_distinct
Calibration = namedtuple("Calibration", "crps se_crps crps_i pit pit_hist coverage quantiles intervals pred_mean pred_sd "
                         "brier log_score brier_i log_score_i p_mean confidence correct reliability ece mce n_samples n_distinct")


def check_probability_levels(name, values, limit=None):
    """Levels strictly inside (0, 1), at most `limit` of them -> list of float."""
    v = [float(x) for x in values]
    if limit is not None and len(v) > limit:
        raise ValueError(f"{len(v)} {name}: at most {limit} per call")
    if any(not (0.0 < x < 1.0) for x in v):
        raise ValueError(f"{name} must lie in (0, 1), got {v}")
    return v


def pit_coverage(pit, levels=(0.5, 0.8, 0.9, 0.95)):
    """Share of rows whose target lies inside the central predictive interval of each level q: (1 - q) / 2 <= pit <= (1 + q) / 2
    (exact: no quantile is needed).  -> {q: share}."""
    pit = np.asarray(pit, dtype=np.float64)
    return {q: float(np.mean((pit >= (1.0 - q) / 2.0) & (pit <= (1.0 + q) / 2.0))) for q in check_probability_levels("levels", levels)}


def pit_histogram(pit, bins=10):
    """Counts of the PIT values in `bins` equal-width bins of (0, 1) (np.histogram: uniform when the model is calibrated)."""
    return np.histogram(np.asarray(pit, dtype=np.float64), int(bins), (0.0, 1.0))[0]


def interval_scores(levels, quantiles, y):
    """For every symmetric pair (a / 2, 1 - a / 2) among the quantile `levels` (quantiles [len(levels), n_rows], targets y): the
    mean width u - l and the mean interval score (u - l) + (2 / a) (l - y)_+ + (2 / a) (y - u)_+ (Gneiting & Raftery 2007).
    -> {(p_lo, p_hi): dict(level = 1 - a, width, score)}."""
    lv = [float(p) for p in levels]
    q = np.asarray(quantiles, dtype=np.float64).reshape(len(lv), -1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    out = {}
    for i, lo in enumerate(lv):
        for j, hi in enumerate(lv):
            if lo < hi and abs(lo + hi - 1.0) <= 1e-12:
                a = 2.0 * lo
                l, u = q[i], q[j]
                score = (u - l) + (2.0 / a) * np.maximum(l - y, 0.0) + (2.0 / a) * np.maximum(y - u, 0.0)
                out[(lo, hi)] = dict(level=1.0 - a, width=float(np.mean(u - l)), score=float(np.mean(score)))
    return out


def crps_summary(crps_i):
    """-> (mean CRPS, its standard error sd(ddof 1) / sqrt(N))."""
    c = np.asarray(crps_i, dtype=np.float64)
    return float(np.mean(c)), (float(np.std(c, ddof=1) / math.sqrt(c.size)) if c.size > 1 else float("nan"))


def reliability_table(confidence, correct, bins=10):
    """Reliability of a classifier's confidence over `bins` equal-width bins of [0, 1] (a value on an edge goes to the upper bin,
    1.0 to the last) -> dict(edges [bins + 1], count [bins], confidence, accuracy [bins] (nan in an empty bin), ece = sum_b
    (count_b / N) |accuracy_b - confidence_b|, mce = the largest gap over the non-empty bins)."""
    bins = int(bins)
    if bins < 1:
        raise ValueError(f"bins = {bins} must be >= 1")
    conf = np.asarray(confidence, dtype=np.float64).reshape(-1)
    hit = np.asarray(correct, dtype=np.float64).reshape(-1)
    edges = np.arange(bins + 1) / bins
    idx = np.clip(np.searchsorted(edges, conf, side="right") - 1, 0, bins - 1)
    count = np.bincount(idx, minlength=bins)
    with np.errstate(invalid="ignore", divide="ignore"):
        mconf = np.bincount(idx, weights=conf, minlength=bins) / count
        acc = np.bincount(idx, weights=hit, minlength=bins) / count
    full = count > 0
    gap = np.abs(acc[full] - mconf[full])
    return dict(edges=edges, count=count, confidence=mconf, accuracy=acc,
                ece=float(np.sum(count[full] / conf.size * gap)), mce=float(np.max(gap)) if gap.size else float("nan"))


def classification_scores(p_mean, y, bins=10):
    """Proper scores and reliability of predictive class probabilities p_mean [n_rows, n_out] against labels y: brier_i = sum_k
    (p_k - 1[y = k])^2, log_score_i = -log p_y, confidence = max_k p_k, correct = (argmax == y) (first index on a tie), and
    reliability_table() of the last two.  -> dict(brier_i, log_score_i, confidence, correct, reliability, ece, mce)."""
    p = np.asarray(p_mean, dtype=np.float64)
    lab = np.asarray(y).reshape(-1).astype(np.int64)
    if p.ndim != 2 or p.shape[0] != lab.size:
        raise ValueError(f"p_mean {p.shape} and {lab.size} labels do not match")
    if lab.size and (lab.min() < 0 or lab.max() >= p.shape[1]):
        raise ValueError(f"labels must lie in [0, {p.shape[1]})")
    rows = np.arange(lab.size)
    onehot = np.zeros_like(p)
    onehot[rows, lab] = 1.0
    with np.errstate(divide="ignore"):
        log_score = -np.log(p[rows, lab])
    conf, correct = np.max(p, axis=1), np.argmax(p, axis=1) == lab
    rel = reliability_table(conf, correct, bins)
    return dict(brier_i=np.sum((p - onehot) ** 2, axis=1), log_score_i=log_score, confidence=conf, correct=correct,
                reliability={k: rel[k] for k in ("edges", "count", "confidence", "accuracy")}, ece=rel["ece"], mce=rel["mce"])


# What predictive_check() returns.  names: the statistics in the device's order; p_value, t_obs_mean, t_rep_mean, t_rep_sd,
# n_defined: dicts by name -- p = P(T(y_rep, theta) >= T(y, theta)) with ties counted half, the means of T on the data and on the
# replicates, the (population) sd of T on the replicates, and the occurrences where both T are finite (the others are left out of
# all of them; p is nan when none is left).  t_obs, t_rep [n_samples, len(names)] float64, chain-major (return_samples, else
# None).  n_samples: the occurrences, each with its own replicate; n_distinct
PredictiveCheck = namedtuple("PredictiveCheck", "names p_value t_obs_mean t_rep_mean t_rep_sd n_defined t_obs t_rep n_samples n_distinct")

PPC_REGRESSION_STATS = ("mean", "sd", "min", "max", "chi2", "max_abs_resid", "ljung_box")
PPC_CLASSIFICATION_STATS = ("deviance", "accuracy")
PPC_DEFAULT_LAGS = (1, 2, 3, 4, 5)         # predictive_check's lags when none are given (a classification: none)


def ppc_check_lags(lags, n_rows):
    """The residual autocorrelation lags of a check on n_rows rows: distinct integers in [1, n_rows - 1], at most 16 -> list."""
    lg = [int(k) for k in lags]
    if any(k != v for k, v in zip(lg, lags)):
        raise ValueError(f"lags must be integers, got {list(lags)}")
    if len(lg) > _lib.PPC_MAX_LAGS:
        raise ValueError(f"{len(lg)} lags: at most {_lib.PPC_MAX_LAGS} per call")
    if len(set(lg)) != len(lg):
        raise ValueError(f"lags must be distinct, got {lg}")
    if any(not (1 <= k <= n_rows - 1) for k in lg):
        raise ValueError(f"lags must lie in [1, n_rows - 1 = {n_rows - 1}], got {lg}")
    return lg


def ppc_stat_names(task, *, lags=(), n_out=1):
    """The statistics of a posterior predictive check in the device's order: a regression's (TASK_REG) with one resid_acf[k]
    per lag, a classification's with one class_count[k] per class."""
    if task == TASK_REG:
        return list(PPC_REGRESSION_STATS) + [f"resid_acf[{int(k)}]" for k in lags]
    return list(PPC_CLASSIFICATION_STATS) + [f"class_count[{k}]" for k in range(int(n_out))]


def ppc_p_values(n_greater, n_equal, n_defined):
    """p = (n_greater + n_equal / 2) / n_defined per statistic: ties count half (a discrete T, such as a class count, then has
    a p-value centred on 1/2 under the model); nan where no occurrence is defined."""
    g, e, d = (np.asarray(v, dtype=np.float64) for v in (n_greater, n_equal, n_defined))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, (g + 0.5 * e) / d, np.nan)


def ppc_flagged(check, alpha=0.05):
    """The names of the statistics whose posterior predictive p-value lies outside [alpha / 2, 1 - alpha / 2], in the order of
    check.names: the features of the data the fitted model does not reproduce.  An undefined p-value (nan) is not flagged."""
    a = float(alpha)
    if not (0.0 < a < 1.0):
        raise ValueError(f"alpha = {alpha} must lie in (0, 1)")
    return [n for n in check.names if check.p_value[n] < a / 2.0 or check.p_value[n] > 1.0 - a / 2.0]


# powerscale_sensitivity's result: names [Q]; prior, likelihood {name: D}; mean_shift, sd_ratio {(component, sign): {name: value}},
# component "prior" / "likelihood", sign "-" (alpha = 1 / (1 + delta)) / "+" (alpha = 1 + delta): (perturbed mean - base mean) /
# base sd and perturbed sd / base sd; khat {(component, sign): k-hat}; diagnosis {name: text}; delta; threshold; good_k
PowerScaling = namedtuple("PowerScaling", "names prior likelihood mean_shift sd_ratio khat diagnosis delta threshold good_k n_samples "
                          "n_distinct")
POWERSCALE_DEFAULT_QUANTITIES = ("weights", "eta", "predictions")     # quantities=None; a classification's default leaves eta out
POWERSCALE_COMPONENTS = ("likelihood", "prior")                        # the device's order
POWERSCALE_SIGNS = ("-", "+")


def powerscale_check_delta(delta):
    """The perturbation size of a power-scaling call: a finite number > 0 -> float."""
    d = float(delta)
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError(f"delta = {delta} must be a finite number > 0")
    return d


def powerscale_groups(quantities, task):
    """The quantity groups of a power-scaling call in the device's order (weights, eta, predictions, loglik) -> list."""
    if quantities is None:
        quantities = [g for g in POWERSCALE_DEFAULT_QUANTITIES if g != "eta" or task == TASK_REG]
    q = list(quantities)
    for g in q:
        if g not in _lib.POWERSCALE_GROUPS:
            raise ValueError(f"unknown quantity group {g!r}: choose among {list(_lib.POWERSCALE_GROUPS)}")
    if not q:
        raise ValueError("no quantity group chosen")
    if "eta" in q and task != TASK_REG:
        raise ValueError("eta: a classification has no eta")
    return [g for g in _lib.POWERSCALE_GROUPS if g in q]


def powerscale_names(groups, *, n_param, n_rows=0, n_out=1, task=TASK_REG):
    """The names of the quantities in the device's order: w[p]; eta; f[n] (regression) or p[n,k] (classification); loglik."""
    names = []
    for g in _lib.POWERSCALE_GROUPS:
        if g not in groups:
            continue
        if g == "weights":
            names += [f"w[{p}]" for p in range(int(n_param))]
        elif g == "predictions":
            names += ([f"f[{n}]" for n in range(int(n_rows))] if task == TASK_REG and int(n_out) == 1 else
                      [f"{'f' if task == TASK_REG else 'p'}[{n},{k}]" for n in range(int(n_rows)) for k in range(int(n_out))])
        else:
            names.append(g)
    return names


def powerscale_diagnosis(prior, likelihood, threshold=0.05):
    """The table of Kallioinen et al. (2023) for one quantity's two sensitivities at `threshold`."""
    if prior >= threshold:
        return "prior-data conflict" if likelihood >= threshold else "strong prior / weak likelihood"
    return "-"


def powerscale_flagged(result, threshold=0.05):
    """The names of the quantities whose prior sensitivity reaches `threshold`, with their diagnosis at that threshold, in the
    order of result.names -> list of (name, diagnosis)."""
    t = float(threshold)
    if not t > 0.0:
        raise ValueError(f"threshold = {threshold} must be > 0")
    out = [(n, powerscale_diagnosis(result.prior[n], result.likelihood[n], t)) for n in result.names]
    return [(n, d) for n, d in out if d != "-"]


# scalar trace columns convergence_diagnostics takes by name (a regression's acc_train slot holds eta = log tau^2)
_SCALAR_COLS = {"likelihood": _lib.TR_LIKEH, "rmse_train": _lib.TR_RMSE_TR, "rmse_test": _lib.TR_RMSE_TE, "acc_train": _lib.TR_ACC_TR,
                "eta": _lib.TR_ACC_TR, "acc_test": _lib.TR_ACC_TE}


class ParallelTemperingBase:
    task = None                       # set by the two drop-in subclasses
    rmse_fmt = None                   # REG '%1.8f' (REG:462-464), CLS '%1.2f' (CLS:473-475)

    def __init__(self, use_langevin_gradients, learn_rate, traindata, testdata, topology, num_chains, maxtemp,
                 NumSample, swap_interval, langevin_prob, path, *, seed=None, device=None, devices=None, exchange="auto",
                 transport=None, waves_per_replica=0, schedule=0, groups_per_replica=0, trace_capacity=0, swap_rule=0,
                 label_swap=False, shared_noise=True, write_files=True, io_threads=None, forward_bf16=0, overlap_chunks=8,
                 adapt_ladder=False):
        # what leave_future_out() builds its refits from: the keyword arguments as given, and NumSample
        self._ctor_kw = dict(device=device, devices=devices, exchange=exchange, transport=transport, waves_per_replica=waves_per_replica,
                             schedule=schedule, groups_per_replica=groups_per_replica, trace_capacity=trace_capacity,
                             swap_rule=swap_rule, label_swap=label_swap, shared_noise=shared_noise, io_threads=io_threads,
                             forward_bf16=forward_bf16, overlap_chunks=overlap_chunks, adapt_ladder=adapt_ladder)
        self._num_sample_arg = NumSample
        # FNN chain variables (REG:491-494)
        self.traindata = traindata
        self.testdata = testdata
        self.topology = topology
        self.num_param = (topology[0] * topology[1]) + (topology[1] * topology[2]) + topology[1] + topology[2]
        # parallel tempering variables (REG:496-507)
        self.swap_interval = swap_interval
        self.path = path
        self.maxtemp = maxtemp
        self.langevin_prob = langevin_prob
        self.num_swap = 0
        self.total_swap_proposals = 0
        self.num_chains = num_chains
        self.chains = []
        self.temperatures = []
        self.NumSamples = int(NumSample / self.num_chains)
        self.learn_rate = learn_rate
        self.use_langevin_gradients = use_langevin_gradients
        # build-specific knobs (keyword only; defaults reproduce the reference's behaviour)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")       # the reference never seeds its generators
        self.seed = int(seed)
        self.device = int(os.environ.get("PTNN_DEVICE", "0")) if device is None else int(device)
        # devices=[0, 1, ...]: the ladder is cut into len(devices) equal contiguous blocks, one per GPU; the swap rounds exchange
        # over RCCL inside libptnn (where the reference forks one process per chain and pipes every vector through the parent,
        # REG:694-771).  $PTNN_DEVICES="0,1,2,3" does the same for an unmodified driver script.  `exchange`: "auto", "gather"
        # or "boundary" (include/ptnn.h); `transport`: None = RCCL when the devices are distinct, host-staged otherwise;
        # "auto" = try RCCL whatever the list; both fall back to host-staged (with a warning) when the RCCL bring-up fails; "rccl" / "host" = that one or an error.
        if devices is None and os.environ.get("PTNN_DEVICES"):
            devices = [int(v) for v in os.environ["PTNN_DEVICES"].split(",")]
        self.devices = None if devices is None else [int(d) for d in devices]
        if self.devices is not None and self.num_chains % len(self.devices) != 0:
            raise ValueError(f"num_chains = {self.num_chains} cannot be cut into {len(self.devices)} equal blocks (one per device)")
        self.exchange = {"auto": _lib.XCHG_AUTO, "gather": _lib.XCHG_GATHER, "boundary": _lib.XCHG_BOUNDARY}[exchange]
        self.transport = transport
        self.waves_per_replica = int(waves_per_replica)
        self.schedule = int(schedule)            # 0 auto, 1 cooperative, 2 speculative, 3 packed, 4 prefetching tree (include/ptnn.h)
        self.groups_per_replica = int(groups_per_replica)
        self.swap_rule = int(swap_rule)          # 0 = the reference's cascade; 1 = even/odd Metropolis exchange (not in the reference)
        # forward pass on the matrix cores (nets of 24..64 or a multiple of 32 > 64 hidden units): 0 = fp32 accuracy on split bf16
        # operands (default), 2 = the exact fp32 instruction (bit-identical to the other schedules), 1 = operands rounded to bf16 (study)
        self.forward_bf16 = int(forward_bf16)
        # True (default): all chains read ONE noise tape -- what the reference's forked chains do, which all inherit the parent's
        # numpy / random state (REG:709-712); the only mode that meets every statistical parity bound against the
        # reference's own runs (tests: F9).  False: every (chain, step) has its own Philox counter, the statistically sounder
        # choice (within-slot posterior variance comes out 1.3 - 1.8 x the reference's on high-acceptance chains).
        self.shared_noise = bool(shared_noise)
        # True: swap rounds permute which chain holds which temperature instead of moving (w, eta) between the temperature slots
        # (zero payload between GPUs; not in the reference).  The files stay keyed by temperature: the rows a
        # temperature's files hold are those of the chain that held it at the time (_stitch_by_temperature).
        self.label_swap = bool(label_swap)
        self.trace_capacity = int(trace_capacity)   # rows per replica kept in HBM (0 = all); smaller = streamed to the host
        self.write_files = bool(write_files)
        self.io_threads = io_threads or min(16, os.cpu_count() or 1)
        # run_chains() cuts the run into this many launches and lets the trace rows of each leave for the host -- and into the
        # per-chain files -- while the next is being sampled (one GPU, every row resident); 0: download and write after the last step
        self.overlap_chunks = int(overlap_chunks)
        # adapt the ladder during burn-in (swap_rule 1): True = every swap round that hands off before
        # int(burn_in * NumSamples) and not past the temperature switch, kappa0 / t0 the defaults; dict(rounds=, kappa0=, t0=)
        # overrides them.  After run_chains() `temperatures` is the frozen ladder, `ladder_history` every adapted one.
        if adapt_ladder is not False and adapt_ladder is not None:
            if self.swap_rule != 1:
                raise ValueError("adapt_ladder needs swap_rule=1: the reference's cascade (swap_rule=0) has no per-pair Metropolis "
                                 "acceptance to equalise")
            if adapt_ladder is not True:
                if not isinstance(adapt_ladder, dict) or set(adapt_ladder) - {"rounds", "kappa0", "t0"}:
                    raise ValueError("adapt_ladder must be True, False or a dict with the keys rounds, kappa0, t0")
                for key in ("kappa0", "t0"):
                    v = adapt_ladder.get(key)
                    if v is not None and not (math.isfinite(float(v)) and float(v) > 0):
                        raise ValueError(f"adapt_ladder: {key} = {v} must be finite and > 0")
        self.adapt_ladder = adapt_ladder if adapt_ladder not in (False, None) else False
        self.ladder_history = None
        self._img = None
        self.timings = {}
        self._sampler = None
        self._w0 = None
        self._finished = False

    # ------------------------------------------------------------------ ladder (REG:529-636)
    def default_beta_ladder(self, ndim, ntemps, Tmax):
        return ladder.default_beta_ladder(ndim, ntemps=ntemps, Tmax=Tmax)

    def assign_temperatures(self):
        """T_i = 1 / beta_i of the geometric ladder (the only spacing main() can reach, REG:615-628)."""
        betas = self.default_beta_ladder(2, ntemps=self.num_chains, Tmax=self.maxtemp)
        self.temperatures.extend(np.inf if b == 0 else float(1.0 / b) for b in betas)

    # ------------------------------------------------------------------ initialize_chains (REG:639-650)
    def initialize_chains(self, burn_in):
        self.burn_in = burn_in
        self.assign_temperatures()
        # w0 per chain: the reference draws np.random.randn(num_param) in the parent (REG:649); here the
        # draws come from Philox stream 3 keyed by (seed, chain) so that a run is reproducible from `seed`
        self._w0 = np.stack([philox.initial_weights(self.seed, r, self.num_param) for r in range(self.num_chains)])
        self._configure()

    def set_initial_weights(self, w0):
        """Override the initial weights (tests / resuming from a known state); shape [num_chains, num_param]."""
        w0 = np.asarray(w0, dtype=np.float64)
        if w0.shape != (self.num_chains, self.num_param):
            raise ValueError("w0 must be [num_chains, num_param]")
        self._w0 = w0
        if self._sampler is not None:
            # a restart begins at the initial ladder again (ptnn_set_state restarts the adaptation from it)
            self._sampler.set_state(self._w0, self._ladder0 if self.ladder_history is not None else self.temperatures)

    def _pt_switch_step(self):
        # `i == pt_samples` with pt_samples = samples * 0.6 compares an int with a float (REG:301,320): it fires
        # only when the product is integral in double arithmetic
        pt_samples = self.NumSamples * 0.6
        return int(pt_samples) if pt_samples == int(pt_samples) else -1

    def _ladder_adapt_spec(self):
        """(rounds, kappa0, t0) of adapt_ladder, or None; the refusals that need no GPU."""
        if self.adapt_ladder is False:
            return None
        hand = self._handoff_steps()
        sw = self._pt_switch_step()
        spec = {} if self.adapt_ladder is True else dict(self.adapt_ladder)
        kappa0 = float(spec.get("kappa0", LADDER_KAPPA0))
        t0 = float(spec.get("t0", LADDER_T0))
        if spec.get("rounds") is None:
            step0 = int(self.burn_in * self.NumSamples)
            A = sum(1 for i in hand if i < step0 and (sw < 0 or i <= sw))
            if A < 2:
                raise ValueError(f"adapt_ladder: {A} swap round(s) hand off inside the burn-in (before step {step0}, "
                                 f"swap_interval {self.swap_interval}): at least 2 are needed (a longer burn_in or more samples)")
        else:
            A = int(spec["rounds"])
            if A < 0 or A > len(hand):
                raise ValueError(f"adapt_ladder: rounds = {A}: the run has {len(hand)} swap rounds")
            if A > 0 and sw >= 0 and hand[A - 1] > sw:
                raise ValueError(f"adapt_ladder: rounds = {A}: the last adapted round hands off after step {hand[A - 1]}, past "
                                 f"the temperature switch at step {sw}")
        return A, kappa0, t0

    def _freeze_step(self):
        """First MH step that runs on the frozen ladder (0 without adaptation)."""
        spec = self._ladder_adapt_spec()
        if spec is None or spec[0] == 0:
            return 0
        return self._handoff_steps()[spec[0] - 1] + 1

    def _configure(self):
        I, H, O = (int(v) for v in self.topology)
        S = self.NumSamples
        if self.swap_interval < 1:
            raise ZeroDivisionError("integer division or modulo by zero")      # `i % self.swap_interval` (REG:427)
        adapt = self._ladder_adapt_spec()
        train = np.asarray(self.traindata, dtype=np.float64)
        test = np.asarray(self.testdata, dtype=np.float64)
        if train.ndim != 2 or train.shape[1] <= I:
            raise IndexError(f"index {I} is out of bounds for axis 1 with size {train.shape[1] if train.ndim == 2 else 0}")
        lib = _lib.load_library()
        if not lib.ptnn_supports(self.task, I, H, O):
            raise _lib.PtnnError(f"no gfx950 kernel for task={self.task} topology={[I, H, O]} in {_lib.library_path()}: "
                                 f"add X({self.task}, {I}, {O}) to PTNN_SHAPES (csrc/ptnn_shapes.hpp) and rebuild; "
                                 f"n_hidden may be anything up to 512")
        config = dict(
            task=self.task, n_in=I, n_hidden=H, n_out=O, n_replicas_global=self.num_chains,
            n_samples=S, swap_interval=int(self.swap_interval), pt_switch_step=self._pt_switch_step(),
            use_langevin=1 if self.use_langevin_gradients is True else 0, waves_per_replica=self.waves_per_replica,
            schedule=self.schedule, groups_per_replica=self.groups_per_replica, trace_capacity=self.trace_capacity,
            swap_rule=self.swap_rule, shared_noise=int(self.shared_noise), label_swap=int(self.label_swap),
            forward_bf16=self.forward_bf16, l_prob=float(self.langevin_prob), learn_rate=float(self.learn_rate), step_w=0.025, step_eta=0.2,
            sigma_squared=25.0, nu_1=0.0, nu_2=0.0, seed=self.seed)
        if self.devices is not None and len(self.devices) > 1:
            from . import distributed
            self._sampler = distributed.LadderGroup(self.devices, exchange=self.exchange, transport=self.transport, **config)
        else:
            dev = self.device if self.devices is None else self.devices[0]
            self._sampler = _lib.Sampler(device_id=dev, n_replicas_local=self.num_chains, first_global_replica=0, **config)
        self._sampler.set_data(train, test)
        self._sampler.set_state(self._w0, self.temperatures)
        self._finished = False
        if self.swap_rule == 1 or self.label_swap:
            self._sampler.set_ladder(self.temperatures)
        if adapt is not None:
            self._sampler.set_ladder_adaptation(*adapt)
        self._ladder0 = list(self.temperatures)
        self.ladder_history = None
        self._img = None
        # (the images are pinned host memory the size of the device's trace arrays: taken up to 1 GiB, above that the resident path)
        image_bytes = self.num_chains * S * (self.num_param + 24) * 4
        if (self.overlap_chunks > 1 and isinstance(self._sampler, _lib.Sampler) and not self.label_swap and not (0 < self.trace_capacity < S)
                and image_bytes <= int(os.environ.get("PTNN_TRACE_IMAGE_MAX_BYTES", 1 << 30))):
            try:
                self._img = self._sampler.trace_image()      # pinned host images of the trace arrays, allocated here once
            except _lib.PtnnError:
                self._img = None                             # compact traces (wide nets): the resident path

    # ------------------------------------------------------------------ run_chains (REG:694-771)
    def run_chains(self, *, checkpoint_path=None, checkpoint_every=None, resume_from=None, max_steps=None):
        """The reference's run_chains().  Keyword-only extras (the reference has none): `checkpoint_path` +
        `checkpoint_every` (MH steps) write a resumable .npz (device state of the chains + the trace rows fetched so far)
        as the run proceeds; `resume_from` continues such a file bit for bit; `max_steps` stops after that many MH steps of
        this call (writing a checkpoint when a path is given) and returns None instead of the result tuple."""
        if self._sampler is None:
            raise RuntimeError("call initialize_chains(burn_in) before run_chains()")
        S = self.NumSamples
        open(self.path + '/num_exchange.txt', 'a').close()                      # REG:704: opened, never written
        t0 = time.perf_counter()
        cap = self.trace_capacity
        chunked = bool(cap and cap < S) or checkpoint_every or resume_from or max_steps
        if chunked:
            # the device keeps a ring of `cap` trace rows per replica (all S rows when cap == 0): drain it in windows
            parts, row, t_fetch = [], 0, 0.0
            if resume_from is not None:
                with np.load(resume_from) as z:
                    self._sampler.restore(z["blob"].tobytes())
                    parts.append({k[3:]: z[k] for k in z.files if k.startswith("tr_")})
                row = self._sampler.steps_done() + 1
                if parts[0]["accept"].shape[1] != row:
                    raise ValueError("checkpoint file is inconsistent: trace rows do not end at the saved step")
            window = (cap - 1) if (cap and cap < S) else S
            if checkpoint_every:
                window = min(window, int(checkpoint_every))
            budget = None if max_steps is None else int(max_steps)

            def save():
                tf = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
                tmp = checkpoint_path + ".tmp.npz"
                np.savez(tmp, blob=np.frombuffer(self._sampler.checkpoint(), np.uint8), **{"tr_" + k: v for k, v in tf.items()})
                os.replace(tmp, checkpoint_path)
            while self._sampler.steps_done() < S - 1 and (budget is None or budget > 0):
                n = min(window, S - 1 - self._sampler.steps_done())
                if budget is not None:
                    n = min(n, budget)
                    budget -= n
                self._sampler.run(n)
                self._sampler.sync()
                tf = time.perf_counter()
                hi = self._sampler.steps_done() + 1
                parts.append(self._sampler.traces(row, hi - row))
                row = hi
                if checkpoint_path is not None and (checkpoint_every or budget == 0):
                    save()
                t_fetch += time.perf_counter() - tf
            if self._sampler.steps_done() < S - 1:
                return None                                                     # max_steps reached: resume later
            self._sampler.run(-1)                                               # phantom round, if due
            self._sampler.sync()
            tr = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
            t1 = time.perf_counter() - t_fetch
            t2 = t1 + t_fetch
            self.num_swap, self.total_swap_proposals, self.rounds = self._sampler.swap_stats()
        elif self._img is not None:
            return self._run_overlapped(t0)
        else:
            self._sampler.run(-1)
            self._sampler.sync()
            t1 = time.perf_counter()
            self.num_swap, self.total_swap_proposals, self.rounds = self._sampler.swap_stats()
            tr = self._sampler.traces()
            t2 = time.perf_counter()
        if self.label_swap:
            tr = self._stitch_by_temperature(tr)
        # the per-chain files (REG:454-481) and what show_results derives from them (REG:775-871) are independent of each other
        # once the traces are on the host: one pool formats the 8 R + 3 files while this thread builds the return values
        with ThreadPoolExecutor(max_workers=self.io_threads) as ex:
            pending = self._write_chain_files(tr, ex) if self.write_files else []
            t3 = time.perf_counter()
            out = self.show_results(tr, _pool=ex, _pending=pending)
            t4 = time.perf_counter()
            for f in pending:
                f.result()                                   # an I/O error of any file surfaces here
        t5 = time.perf_counter()
        return self._finish_run(out, dict(sampling_s=t1 - t0, fetch_s=t2 - t1, chain_files_s=t3 - t2, show_results_s=t4 - t3, files_drain_s=t5 - t4,
                                          files_and_results_s=t5 - t2, overlapped=False))

    def _finish_run(self, out, timings):
        self._finished = True
        if self.adapt_ladder is not False:
            # the rows after the freeze were sampled at the frozen ladder (the files keep the names of the initial one)
            lad, _ = self._sampler.ladder_history()
            self.ladder_history = lad
            A = lad.shape[0] - 1
            frozen = lad[min(A, self.rounds)]
            if not np.all(np.diff(frozen) > 0):
                # float32 rounding of nearly collapsed gaps (a kappa0 far too large): the rungs are no longer distinct
                warnings.warn(f"the adapted ladder is not strictly increasing in float32: {frozen.tolist()}; use a smaller kappa0",
                              stacklevel=2)
            self.temperatures = [float(T) for T in frozen]
        nlaunch, kms = self._sampler.kernel_time()
        self.timings = dict(timings, segment_launches=nlaunch, segment_kernel_ms=kms,
                            samples_per_s=self.num_chains * (self.NumSamples - 1) / max(timings["sampling_s"], 1e-12))
        pos_w, fx_train, fx_test, rmse_train, rmse_test, acc_train, acc_test, likelihood_vec, accept_vec, accept = out
        swap_perc = self.num_swap * 100 / self.total_swap_proposals            # ZeroDivisionError when no round ran (REG:769)
        return (pos_w, fx_train, fx_test, rmse_train, rmse_test, acc_train, acc_test, likelihood_vec, swap_perc,
                accept_vec, accept)

    # ------------------------------------------------------------------ run_chains with the download and the files behind the sampling
    def _run_overlapped(self, t0):
        """The run in `overlap_chunks` launches (whole swap intervals each; the chain does not depend on the cut: ptnn_run); the
        trace rows of a launch are copied into the pinned images by a second stream as soon as it ends, and formatted into the
        per-chain files (append mode) by the pool, while the next launch samples.  Same bytes in every file as the resident path."""
        s, S, si = self._sampler, self.NumSamples, max(1, int(self.swap_interval))
        pos_img, rows_img = self._img
        ends = overlap_cuts(S, si, self.overlap_chunks)
        tickets, done, row = [], 0, 0
        for b in ends:
            s.run(-1 if b == S - 1 else b - done)           # queued, not waited for
            done = b
            tickets.append((s.trace_fetch(row, b + 1 - row), row, b + 1))       # rows 0 .. b exist once step b - 1 has run
            row = b + 1
        # one writer thread takes the windows in order (a file's pieces must follow each other); each window is one call into the C
        # library, which spreads its 7 R files over the I/O threads
        with ThreadPoolExecutor(max_workers=self.io_threads) as ex, ThreadPoolExecutor(max_workers=1) as writer:
            pending, landed = [], []
            for tk, lo, hi in tickets:
                s.trace_wait(tk)
                landed.append(round(time.perf_counter() - t0, 6))
                if self.write_files:
                    pending.append(writer.submit(self._write_chain_rows, pos_img, rows_img, lo, hi))
            s.sync()                                         # a failed run surfaces here
            t1 = time.perf_counter()
            self.num_swap, self.total_swap_proposals, self.rounds = s.swap_stats()
            zeros = np.zeros((self.num_chains, S), np.float32)
            tr = {"pos_w": pos_img, "likeh": rows_img[:, :, 0], "rmse_train": rows_img[:, :, 1], "rmse_test": rows_img[:, :, 2],
                  "acc_train": zeros if self.task == TASK_REG else rows_img[:, :, 3],      # REG:403 (the slot carries eta, ptnn.h)
                  "acc_test": rows_img[:, :, 4], "accept": rows_img[:, :, 5].view(np.int32)}
            if self.write_files:
                self._final_accepted = s.state()["num_accepted"]
                for r, T in enumerate(self.temperatures):
                    acc_ratio = int(self._final_accepted[r]) / (S * 1.0) * 100     # REG:447
                    pending.append(ex.submit(_lib.savetxt, f'{self.path}/posterior/accept_list/chain_{T}_accept.txt', np.array([acc_ratio]), '%1.4f'))
            t3 = time.perf_counter()
            out = self.show_results(tr, _pool=ex, _pending=pending)
            t4 = time.perf_counter()
            for f in pending:
                f.result()                                   # an I/O error of any file surfaces here
        t5 = time.perf_counter()
        return self._finish_run(out, dict(sampling_s=t1 - t0, fetch_s=0.0, chain_files_s=t3 - t1, show_results_s=t4 - t3, files_drain_s=t5 - t4,
                                          files_and_results_s=t5 - t1, overlapped=True, launches_per_run=len(ends), rows_landed_s=landed))

    def _write_chain_rows(self, pos_img, rows_img, lo, hi):
        """Rows [lo, hi) of every per-chain trace file (REG:454-481): one call into the C library, which spreads the 7 R files over
        the I/O threads (pieces of a file are written in order: the caller runs these calls one after the other)."""
        n, R = hi - lo, self.num_chains
        rows = rows_img[:, lo:hi]                                                 # [R, n, 8] view of the image
        likeh = np.zeros((R, n, 2), dtype=np.float32)
        likeh[:, :, 0] = rows[:, :, 0]
        if lo == 0:
            likeh[:, 0, 1] = -100.0                                               # row 0 = [-100, -100] (REG:293)
        # accept_list[i+1] holds the count BEFORE step i (REG:380): small integers, exact in float32
        accept = rows[:, :, 5].view(np.int32).astype(np.float32)
        acc_tr = np.zeros((R, n, 1), np.float32) if self.task == TASK_REG else rows[:, :, 3:4]
        big, small = [], []
        for r, T in enumerate(self.temperatures):
            tn = str(T)
            big.append((f'{self.path}/posterior/pos_w/chain_{tn}.txt', pos_img[r, lo:hi], '%.18e'))
            small += [
                (f'{self.path}/predictions/rmse_test_chain_{tn}.txt', rows[r, :, 2:3], self.rmse_fmt),
                (f'{self.path}/predictions/rmse_train_chain_{tn}.txt', rows[r, :, 1:2], self.rmse_fmt),
                (f'{self.path}/predictions/acc_test_chain_{tn}.txt', rows[r, :, 4:5], '%1.2f'),
                (f'{self.path}/predictions/acc_train_chain_{tn}.txt', acc_tr[r], '%1.2f'),
                (f'{self.path}/posterior/pos_likelihood/chain_{tn}.txt', likeh[r], '%1.4f'),
                (f'{self.path}/posterior/accept_list/chain_{tn}.txt', accept[r], '%1.4f'),
            ]
        _lib.savetxt_batch(big + small, append=lo > 0, threads=self.io_threads)   # the big files first

    # ------------------------------------------------------------------ label swapping: rows per chain slot -> rows per temperature
    def _handoff_steps(self):
        """MH steps after which a swap round moved something: REG i % si == 0, i != 0 (REG:427); CLS (i + 1) % si == 0 (CLS:438)."""
        si, S = int(self.swap_interval), self.NumSamples
        if self.task == TASK_REG:
            return [i for i in range(1, S - 1) if i % si == 0]
        return [i for i in range(S - 1) if (i + 1) % si == 0]

    def _stitch_by_temperature(self, tr):
        out, self._final_holder = stitch_by_temperature(tr, self._sampler.swap_log(), self._handoff_steps(), self.NumSamples)
        return out

    # ------------------------------------------------------------------ per-chain files (REG:454-481)
    def _chain_file_jobs(self, tr):
        S = self.NumSamples
        jobs = []
        for r, T in enumerate(self.temperatures):
            tn = str(T)
            likeh = np.zeros((S, 2), dtype=np.float32)
            likeh[:, 0] = tr["likeh"][r]
            likeh[0, 1] = -100.0                                                 # row 0 = [-100, -100] (REG:293)
            acc_ratio = int(self._final_accepted[r]) / (S * 1.0) * 100                 # REG:447
            # float32 arrays go to the C writer as they are (every value printed as the double it converts to, like np.savetxt);
            # the biggest file first so that the pool's last job is a small one
            jobs += [
                (f'{self.path}/posterior/pos_w/chain_{tn}.txt', tr["pos_w"][r], '%.18e'),
                (f'{self.path}/predictions/rmse_test_chain_{tn}.txt', tr["rmse_test"][r], self.rmse_fmt),
                (f'{self.path}/predictions/rmse_train_chain_{tn}.txt', tr["rmse_train"][r], self.rmse_fmt),
                (f'{self.path}/predictions/acc_test_chain_{tn}.txt', tr["acc_test"][r], '%1.2f'),
                (f'{self.path}/predictions/acc_train_chain_{tn}.txt', tr["acc_train"][r], '%1.2f'),
                (f'{self.path}/posterior/pos_likelihood/chain_{tn}.txt', likeh, '%1.4f'),
                (f'{self.path}/posterior/accept_list/chain_{tn}_accept.txt', np.array([acc_ratio]), '%1.4f'),
                (f'{self.path}/posterior/accept_list/chain_{tn}.txt', tr["accept"][r], '%1.4f'),
            ]
        return jobs

    def _write_chain_files(self, tr, pool):
        """Queues every per-chain file on `pool`; returns the futures."""
        # accept_list[i+1] holds the count BEFORE step i (REG:380); the percentage file uses the final count
        self._final_accepted = self._sampler.state()["num_accepted"]
        if self.label_swap:                                  # per temperature: the count of the chain that holds it at the end
            self._final_accepted = self._final_accepted[self._final_holder]
        jobs = self._chain_file_jobs(tr)
        jobs.sort(key=lambda j: -np.asarray(j[1]).size)
        return [pool.submit(_lib.savetxt, *j) for j in jobs]

    # ------------------------------------------------------------------ show_results (REG:775-871 / CLS:780-893)
    def _likelihood_rows(self, burnin):
        raise NotImplementedError

    def show_results(self, tr=None, _pool=None, _pending=None):
        if tr is None:
            tr = self._sampler.traces()
            if self.label_swap:
                tr = self._stitch_by_temperature(tr)
        S, R = self.NumSamples, self.num_chains
        burnin = int(S * self.burn_in)
        th = self.io_threads
        # the reference re-reads the per-chain text files, so every value below has been through their format
        # ('%.18e' round-trips a float32 exactly: the posterior matrix is the traces themselves, cut, widened and transposed)
        posterior = _lib.posterior_matrix(tr["pos_w"], burnin, th)              # (P, R (S - burnin)) float64
        rmse_train = _text_round(tr["rmse_train"][:, burnin:], self.rmse_fmt, th)
        rmse_test = _text_round(tr["rmse_test"][:, burnin:], self.rmse_fmt, th)
        acc_train = _text_round(tr["acc_train"][:, burnin:], '%1.2f', th)
        acc_test = _text_round(tr["acc_test"][:, burnin:], '%1.2f', th)
        accept_list = tr["accept"].astype(np.float64)
        lo = self._likelihood_rows(burnin)
        likelihood_vec = np.zeros((R * (S - lo), 2))                             # rows: chain after chain
        likelihood_vec[:, 0] = _text_round(tr["likeh"][:, lo:], '%1.4f', th).reshape(-1)
        if lo == 0:
            likelihood_vec[::S, 1] = -100.0
        accept_percent = np.zeros((R, 1))                                        # never filled (REG:780,860)

        fx_train_all = np.zeros((R, S - burnin, np.asarray(self.traindata).shape[0]))
        fx_test_all = np.zeros((R, S - burnin, np.asarray(self.testdata).shape[0]))
        rmse_train = rmse_train.reshape(R * (S - burnin), 1)
        acc_train = acc_train.reshape(R * (S - burnin), 1)
        rmse_test = rmse_test.reshape(R * (S - burnin), 1)
        acc_test = acc_test.reshape(R * (S - burnin), 1)
        accept_vec = accept_list
        accept = np.sum(accept_percent) / R
        if self.write_files:
            jobs = [(self.path + '/likelihood.txt', likelihood_vec, '%1.5f'), (self.path + '/accept_list.txt', accept_list, '%1.2f'),
                    (self.path + '/acceptpercent.txt', np.array([accept]), '%1.2f')]
            if _pool is not None:
                _pending.extend(_pool.submit(_lib.savetxt, *j) for j in jobs)
            else:
                for j in jobs:
                    _lib.savetxt(*j)
        return (posterior, fx_train_all, fx_test_all, rmse_train, rmse_test, acc_train, acc_test, likelihood_vec,
                accept_vec, accept)

    # ------------------------------------------------------------------ posterior predictive (not in the reference's run_chains)
    # ------------------------------------------------------------------ what the posterior analysis calls share
    def ladder_diagnostics(self, burn_in=None):
        """How the ladder works, over the swap rounds that hand off at or after int(NumSamples * burn_in) (None = the object's
        burn_in): dict(temperatures = the (frozen) ladder, pair_accept [R-1] = accepted / proposed per adjacent pair,
        pair_accept_rb [R-1] = mean Rao-Blackwellised acceptance a_k of those rounds (None without adapt_ladder), round_trips [R]
        per walker (index 0 -> R-1 -> 0), mean_round_trip_rounds, history = the ladder history (None without adapt_ladder))."""
        if self._sampler is None or not self._finished:
            raise ValueError("ladder_diagnostics needs a finished run: call initialize_chains() and run_chains() first")
        b = self.burn_in if burn_in is None else burn_in
        step0 = int(self.NumSamples * b)
        hand = self._handoff_steps()
        first = sum(1 for i in hand if i < step0)
        st = ladder_stats_from_log(self._sampler.swap_log(), self.swap_rule, first, n_moves=len(hand))
        rb = None
        if self.adapt_ladder is not False:
            _, acc = self._sampler.ladder_history()
            rows = acc[first:len(hand)]
            rb = rows.astype(np.float64).mean(axis=0) if rows.shape[0] else np.full(self.num_chains - 1, np.nan)
        return dict(temperatures=np.asarray(self.temperatures, np.float64), pair_accept=st["pair_accept"], pair_accept_rb=rb,
                    round_trips=st["round_trips"], mean_round_trip_rounds=st["mean_round_trip_rounds"], history=self.ladder_history)

    def _need_sampler(self, name):
        if self._sampler is None:
            raise ValueError(f"{name} needs the chains' device handle: call initialize_chains() and run_chains() first")
        if not isinstance(self._sampler, _lib.Sampler):
            raise ValueError(f"{name} runs on one GPU: a ladder sharded over several devices is not supported")

    def _check_trace(self, alt):
        """The trace of a finished run is on the device, one chain per temperature; `alt` names the host-data argument."""
        S = self.NumSamples
        if self.label_swap:
            raise ValueError(f"label_swap=True: trace rows are kept per chain slot, not per temperature; pass {alt}=")
        if 0 < self.trace_capacity < S:
            raise ValueError(f"trace_capacity = {self.trace_capacity} < NumSamples = {S}: the rows have been streamed off "
                             f"the device; pass {alt}=")
        if not self._finished:
            raise ValueError(f"no finished run_chains() on this object: the trace is incomplete; pass {alt}=")

    def _trace_selection(self, burn_in, chains, thin, alt="weights"):
        """Every selected chain's trace rows from int(NumSamples * burn_in) on, every thin-th -> (Sampler source keywords,
        sample count)."""
        self._check_trace(alt)
        S = self.NumSamples
        b = self.burn_in if burn_in is None else burn_in
        step0 = int(S * b)
        if chains == "all":
            reps = None
        elif chains == "cold":
            reps = [int(np.argmin(self.temperatures))]
        else:
            reps = [int(c) for c in chains]
            if not reps or min(reps) < 0 or max(reps) >= self.num_chains:
                raise ValueError(f"chains {chains!r}: indices must lie in [0, {self.num_chains})")
        nrep = self.num_chains if reps is None else len(reps)
        return dict(replicas=reps, step0=step0, nsteps=S - step0, thin=int(thin)), nrep * max(0, -(-(S - step0) // max(1, int(thin))))

    def _weights(self, weights):
        """weights=: vectors [n, num_param] (or their transpose), or a pair (vectors, integer multiplicities) -> (w, mult)."""
        mult = None
        if isinstance(weights, tuple):
            weights, mult = weights
        w = np.asarray(weights)
        P = self.num_param
        if w.ndim != 2 or P not in w.shape:
            raise ValueError(f"weights must be [n, {P}] vectors (or their transpose), got shape {w.shape}")
        return (w if w.shape[1] == P else w.T), mult

    @staticmethod
    def _band_ranks(M, pcts):
        """The order statistics np.percentile's linear interpolation needs for `pcts` of M samples -> (spots, ranks)."""
        if M < 1:
            raise ValueError("the selection holds no sample")
        spots = percentile_ranks(M, pcts)
        ranks = sorted({r for lo, hi, _ in spots for r in (lo, hi)})
        if len(ranks) > _lib.PREDICT_MAX_RANKS:
            raise ValueError(f"{len(pcts)} percentiles need {len(ranks)} order statistics: at most {_lib.PREDICT_MAX_RANKS} per call")
        return spots, ranks

    @staticmethod
    def _bands(order_stats, pcts, spots, ranks):
        pos = {r: k for k, r in enumerate(ranks)}
        return {p: lerp_percentile(order_stats[pos[lo]], order_stats[pos[hi]], g) for p, (lo, hi, g) in zip(pcts, spots)}

    def posterior_predictive(self, x="test", *, burn_in=None, chains="all", thin=1, percentiles=(5, 95), weights=None,
                             return_samples=False):
        """Predictions with uncertainty from the sampled chains, computed on the GPU: what the reference's drafts derive from
        fx_train_all / fx_test_all (fx_mu = fx.mean(axis=0), np.percentile bands; Misc_code/ldpt_classifier_multi.py:788-794).

        The sample set is by default the columns of the posterior matrix run_chains() returns: every chain's trace rows from
        int(NumSamples * burn_in) on.  `chains`: "all", "cold" (the temperature-1 chain) or a list of chain indices; `thin`: every
        thin-th row.  `weights`: weight vectors instead of the trace -- [n, num_param] (e.g. run_chains()[0].T), or a pair
        (vectors, integer multiplicities); works whenever the handle exists.  `x`: "train", "test" or an array whose first n_in
        columns are the inputs.  Percentiles follow np.percentile(method="linear") exactly: the device returns the exact order
        statistics, the interpolation is numpy's arithmetic.  -> Predictive(mean, percentiles, vote, pred_class, samples,
        n_samples, n_distinct); outputs are [n_rows, n_out], samples [n_samples, n_rows, n_out] in chain-major order."""
        self._need_sampler("posterior_predictive")
        I = int(self.topology[0])
        if isinstance(x, str):
            if x not in ("train", "test"):
                raise ValueError(f"x must be 'train', 'test' or an array, not {x!r}")
            xs = x
        else:
            xa = np.asarray(x)
            if xa.ndim != 2 or xa.shape[1] < I:
                raise ValueError(f"x must be 2-D with at least n_in = {I} columns, got shape {xa.shape}")
            xs = np.ascontiguousarray(xa[:, :I], dtype=np.float32)
        pcts = list(percentiles)
        if any(not (0 <= p <= 100) for p in pcts):
            raise ValueError(f"percentiles must lie in [0, 100], got {pcts}")
        if weights is not None:
            w, mult = self._weights(weights)
            kw = dict(w=w, multiplicity=mult)
            M = int(np.sum(np.asarray(mult, dtype=np.int64))) if mult is not None else w.shape[0]
        else:
            kw, M = self._trace_selection(burn_in, chains, thin)
        spots, ranks = self._band_ranks(M, pcts)
        cls = self.task == TASK_CLS
        out = self._sampler.predict(xs, ranks=ranks, vote=cls, samples=bool(return_samples), **kw)
        bands = self._bands(out["order_stats"], pcts, spots, ranks)
        mean = out["mean"]
        return Predictive(mean=mean, percentiles=bands, vote=out["vote"] if cls else None,
                          pred_class=np.argmax(mean, axis=1) if cls else None, samples=out["samples"],
                          n_samples=out["n_samples"], n_distinct=out["n_distinct"])

    # ------------------------------------------------------------------ input sensitivity (not in the reference)
    def input_sensitivity(self, x="test", *, burn_in=None, chains="all", thin=1, weights=None, percentiles=(5, 95), return_samples=False):
        """Which inputs the sampled nets respond to, and how sure the posterior is about it, computed on the GPU: the gradient
        g[n, o, i] = d output_o / d input_i of every selected sample on every row of `x` (the outputs posterior_predictive returns:
        the sigmoid output of a regression, the class probabilities of a classification), reduced over the
        samples.  For the time-series nets the inputs are lags.

        Sample set, `chains`, `thin`, `weights` and `x` as in posterior_predictive; percentiles follow np.percentile(method="linear")
        exactly.  -> Sensitivity: per row, output and input the posterior grad_mean, percentiles[q], prob_positive and
        prob_negative (the shares of the samples with g > 0 and g < 0); per output and input the global relevance -- with
        a_s = the mean over the rows of |g| in sample s: importance = the mean of a_s, importance_percentiles[q] of a_s,
        importance_rms = sqrt of the mean of g^2 over rows and samples, top_prob = the share of the samples in which this input
        has the largest a_s of the output (first index on a tie); samples [n_samples, n_rows, n_out, n_in] (chain-major) on
        request; n_samples, n_distinct."""
        self._need_sampler("input_sensitivity")
        I = int(self.topology[0])
        if isinstance(x, str):
            if x not in ("train", "test"):
                raise ValueError(f"x must be 'train', 'test' or an array, not {x!r}")
            xs = x
        else:
            xa = np.asarray(x)
            if xa.ndim != 2 or xa.shape[1] < I:
                raise ValueError(f"x must be 2-D with at least n_in = {I} columns, got shape {xa.shape}")
            xs = np.ascontiguousarray(xa[:, :I], dtype=np.float32)
        pcts = list(percentiles)
        if any(not (0 <= p <= 100) for p in pcts):
            raise ValueError(f"percentiles must lie in [0, 100], got {pcts}")
        if weights is not None:
            w, mult = self._weights(weights)
            kw = dict(w=w, multiplicity=mult)
            M = int(np.sum(np.asarray(mult, dtype=np.int64))) if mult is not None else w.shape[0]
        else:
            kw, M = self._trace_selection(burn_in, chains, thin)
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.sensitivity(xs, ranks=ranks, ranks2=ranks, sample_abs=True, samples=bool(return_samples), **kw)
        # top_prob from the distinct samples: runs of equal consecutive rows of sample_abs with their lengths
        sa = out["sample_abs"]
        new = np.ones(sa.shape[0], bool)
        new[1:] = np.any(sa[1:] != sa[:-1], axis=(1, 2))
        starts = np.flatnonzero(new)
        top = top_share(sa[starts], np.diff(np.append(starts, sa.shape[0])))
        has = bool(ranks)
        return Sensitivity(grad_mean=out["grad_mean"], percentiles=self._bands(out["order_stats"], pcts, spots, ranks) if has else {},
                           prob_positive=out["pos_count"] / np.float64(M), prob_negative=out["neg_count"] / np.float64(M),
                           importance=out["abs_mean"], importance_rms=np.sqrt(out["sq_mean"]),
                           importance_percentiles=self._bands(out["abs_order_stats"], pcts, spots, ranks) if has else {},
                           top_prob=top, samples=out["samples"], n_samples=out["n_samples"], n_distinct=out["n_distinct"])

    # ------------------------------------------------------------------ convergence diagnostics (not in the reference)
    def convergence_diagnostics(self, *, burn_in=None, chains="all", thin=1, params=None, scalars=("likelihood",), per_chain=False,
                                n_lags=0, draws=None):
        """Split-R-hat, split-ESS and the Monte Carlo standard error of the mean of weights and scalar traces, computed on the GPU
        from the traces it already holds (classic split-R-hat / split-ESS with Geyer's initial monotone sequence, BDA3 11.4-11.5,
        not rank-normalised).

        The draws are by default those of the posterior matrix run_chains() returns: every chain's trace rows from
        int(NumSamples * burn_in) on.  `chains`: "all", "cold" (the temperature-1 chain) or a list of chain indices; `thin`: every
        thin-th row.  The default chains="all" pools every temperature, as the reference's pos_w does, so R-hat over a ladder also
        measures the spread between temperatures; chains="cold" with per_chain=True gives the posterior's own figure (a single
        chain's split-R-hat compares its two halves).  `params`: weight indices (None = all, [] = none); `scalars`: names among
        likelihood, rmse_train, rmse_test, acc_train, acc_test (regression: eta, the log tau^2 trace, instead of acc_train).
        `per_chain`: also the ESS of each chain alone; `n_lags`: also the raw combined autocorrelation rho_t, t < n_lags.
        `draws`: host draws [n_chains, n_draws, Q] instead of the trace (names q0 ..); works whenever the handle exists.
        -> Convergence(names, mean, sd, r_hat, ess, mcse_mean = sd / sqrt(ess), ess_chain, rho, trunc_lag, n_chains, n_draws)."""
        self._need_sampler("convergence_diagnostics")
        if draws is not None:
            d = np.asarray(draws)
            if d.ndim != 3:
                raise ValueError(f"draws must be [n_chains, n_draws, n_quantities], got shape {d.shape}")
            names = [f"q{k}" for k in range(d.shape[2])]
            out = self._sampler.convergence(draws=d, per_chain=per_chain, n_lags=n_lags)
        else:
            kw, _ = self._trace_selection(burn_in, chains, thin, alt="draws")
            P = self.num_param
            pidx = None if params is None else [int(p) for p in params]
            if pidx is not None and any(not (0 <= p < P) for p in pidx):
                raise ValueError(f"params: weight indices must lie in [0, {P})")
            reg = self.task != TASK_CLS
            cols = {}
            for nm in scalars:
                if nm not in _SCALAR_COLS or (nm == "eta" and not reg) or (nm == "acc_train" and reg):
                    allowed = ["likelihood", "rmse_train", "rmse_test", "eta" if reg else "acc_train", "acc_test"]
                    raise ValueError(f"scalar {nm!r}: one of {allowed}")
                cols[_SCALAR_COLS[nm]] = nm
            names = [f"w{p}" for p in (range(P) if pidx is None else pidx)] + [cols[c] for c in sorted(cols)]
            if not names:
                raise ValueError("no quantity selected: give params and/or scalars")
            out = self._sampler.convergence(params=pidx, scalars=sorted(cols), per_chain=per_chain, n_lags=n_lags, **kw)
        sd = np.sqrt(out["var"])
        with np.errstate(invalid="ignore", divide="ignore"):
            mcse = sd / np.sqrt(out["ess"])
        return Convergence(names=names, mean=out["mean"], sd=sd, r_hat=out["r_hat"], ess=out["ess"], mcse_mean=mcse,
                           ess_chain=out["ess_chain"], rho=out["rho"], trunc_lag=out["trunc_lag"], n_chains=out["n_chains"],
                           n_draws=out["n_draws"])

    # ------------------------------------------------------------------ predictive accuracy (not in the reference)
    def predictive_accuracy(self, data="train", *, burn_in=None, chains="all", thin=1, weights=None, eta=None, loglik=None,
                            r_eff=1.0, return_pointwise=False):
        """How well the sampled model predicts, as the expected log pointwise predictive density (elpd), computed on the GPU from
        the traces it already holds: the figure to compare two models by -- e.g. 5 vs 10 hidden units, or
        Langevin vs random-walk proposals -- with elpd_compare().

        data="train": elpd_loo is the PSIS-LOO estimate of the elpd of a new data point from the training rows (Pareto smoothed
        importance sampling leave-one-out; khat is the Pareto shape per row, rows with khat > good_k make the estimate unreliable,
        and a warning says so), elpd_waic the WAIC estimate, lppd the in-sample fit they correct by p_loo / p_waic.  data="test"
        (or rows [n_rows, >= n_in + 1], the column after the inputs the target): lppd is itself the held-out log predictive
        density of those rows -- the direct measure; elpd_loo / elpd_waic then estimate how each row would fare had it been left
        out of a fit it was never in.  The log-likelihood is untempered (regression: Gaussian with tau^2 = exp(eta) of each
        sample; classification: log of the softmax probability of the true class).

        The sample set is by default the columns of the posterior matrix run_chains() returns: every chain's trace rows from
        int(NumSamples * burn_in) on.  `chains`: "all", "cold" (the temperature-1 chain) or a list of chain indices; `thin`: every
        thin-th row.  As in pos_w, rows before the temperature switch (the reference's pt_samples = 0.6 NumSamples) are draws of
        the tempered chains; chains="all" pools every temperature.  A regression needs each row's eta, which the trace records
        only from a chain's first accepted step on: a selection that reaches earlier rows is refused (use a larger burn_in).
        `weights`: weight vectors instead of the trace -- [n, num_param] or a pair (vectors, integer multiplicities), with `eta`
        [n] (regression); `loglik`: a pointwise log-likelihood [n_samples, n_rows] (or a pair with multiplicities) instead of
        both.  r_eff: relative efficiency of the draws for the PSIS tail length.  return_pointwise: also log_lik [S, n_rows].
        -> PredictiveAccuracy; totals are sums over rows, se_* = sqrt(N var(pointwise, ddof 1))."""
        self._need_sampler("predictive_accuracy")
        I = int(self.topology[0])
        kw = {}
        if loglik is not None:
            mult = None
            if isinstance(loglik, tuple):
                loglik, mult = loglik
            kw = dict(loglik=np.asarray(loglik, dtype=np.float64), multiplicity=mult)
            ds = "test"
        else:
            if isinstance(data, str):
                if data not in ("train", "test"):
                    raise ValueError(f"data must be 'train', 'test' or an array, not {data!r}")
                ds = data
            else:
                xa = np.asarray(data)
                if xa.ndim != 2 or xa.shape[1] < I + 1:
                    raise ValueError(f"data must be 2-D with at least n_in + 1 = {I + 1} columns (inputs, target), got shape {xa.shape}")
                ds = np.ascontiguousarray(xa[:, :I + 1], dtype=np.float32)
            if weights is not None:
                w, mult = self._weights(weights)
                if self.task != TASK_CLS and eta is None:
                    raise ValueError("a regression's weights need eta = log tau^2, one per vector (Sampler.eta_trace())")
                kw = dict(w=w, eta=None if self.task == TASK_CLS else eta, multiplicity=mult)
        if not kw:
            kw, _ = self._trace_selection(burn_in, chains, thin)
        out = self._sampler.elpd(ds, r_eff=r_eff, loglik_out=bool(return_pointwise) and loglik is None, **kw)
        lppd_i, p_waic_i, loo_i, khat = out["lppd"], out["p_waic"], out["elpd_loo"], out["khat"]
        waic_i = lppd_i - p_waic_i
        n_s = out["n_samples"]
        good_k = min(1.0 - 1.0 / math.log10(n_s), 0.7)
        high = np.isfinite(khat) & (khat > good_k)
        n_high = int(np.count_nonzero(high))
        if n_high:
            warnings.warn(f"{n_high} of {khat.size} rows have a Pareto k-hat above {good_k:.2f}: the PSIS-LOO estimate is "
                          f"unreliable for them", stacklevel=2)
        elpd_loo = float(np.sum(loo_i))
        return PredictiveAccuracy(elpd_loo=elpd_loo, se_elpd_loo=_se_total(loo_i), p_loo=float(np.sum(lppd_i)) - elpd_loo,
                                  elpd_waic=float(np.sum(waic_i)), se_elpd_waic=_se_total(waic_i), p_waic=float(np.sum(p_waic_i)),
                                  lppd=float(np.sum(lppd_i)), se_lppd=_se_total(lppd_i), lppd_i=lppd_i, elpd_loo_i=loo_i,
                                  p_waic_i=p_waic_i, khat=khat, good_k=good_k, n_high_k=n_high,
                                  log_lik=(loglik if loglik is not None else out["loglik"]) if return_pointwise else None,
                                  n_samples=n_s, n_distinct=out["n_distinct"])

    # ------------------------------------------------------------------ leave-future-out cross-validation (not in the reference)
    def _lfo_refit(self, rows, origin):
        """A fresh sampler of this class and these constructor arguments fitted on rows [0, origin): no files, its own scratch
        directory (removed after the run), seed lfo_refit_seed(seed, origin)."""
        path = tempfile.mkdtemp(prefix="ptnn_lfo_")
        try:
            args = [self.use_langevin_gradients, self.learn_rate, rows[:origin], self.testdata, self.topology, self.num_chains,
                    self.maxtemp, self._num_sample_arg, self.swap_interval]
            if self.task != TASK_CLS:
                args.append(self.langevin_prob)
            pt = type(self)(*args, path, seed=lfo_refit_seed(self.seed, origin), write_files=False, **self._ctor_kw)
            pt.initialize_chains(self.burn_in)
            pt.run_chains()
        finally:
            shutil.rmtree(path, ignore_errors=True)
        return pt

    def leave_future_out(self, min_train=None, block=1, data="train", *, n_fit=None, refit=True, k_threshold=None, max_refits=None,
                         burn_in=None, chains="all", thin=1, r_eff=1.0):
        """Leave-future-out cross-validation of ordered rows on the GPU (Buerkner, Gabry & Vehtari 2020):
        for every origin i, the log predictive density of rows i .. i + block - 1 from a posterior that has seen rows 0 .. i - 1
        only -- the question to ask of a time series, where PSIS-LOO (predictive_accuracy) lets a row's neighbours, its future
        included, inform its prediction.  `block` > 1 scores the next `block` rows jointly, each from its own observed inputs:
        `block` one-step predictions, not a recursive `block`-step forecast (forecast() does those).

        data="train": the training rows, which this object's chains have seen (n_fit = their count); origins min_train ..
        N - block (min_train=None: N // 2), walked backward from the fit.  data="test": the training rows followed by the test
        rows, n_fit = the training count, origins n_fit .. N - block walked forward: the sequential score of the test rows, row n
        predicted by the posterior updated with the test rows before it -- what a deployed one-step forecaster does, and lppd
        does not measure.  data=rows [N, >= n_in + 1] with n_fit= for anything else: the chains must have been fitted to
        rows[:n_fit].  The sample set: burn_in, chains, thin, r_eff as in predictive_accuracy.

        One device call scores every remaining origin from the current fit by Pareto-smoothed importance weights; the origins up
        to the first (in walk order) whose k-hat exceeds k_threshold (default: good_k of the sample count) are kept.  refit=True:
        a fresh sampler of this class and constructor arguments (no files, seed lfo_refit_seed(seed, origin): the result is
        reproducible from `seed`) is fitted on rows [0, i), scores that origin exactly, and the walk goes on from it;
        refit=callable(rows) -> a fitted ParallelTempering does the fit instead; refit=False never refits.  After max_refits
        refits the remaining origins are returned with their high k-hat, and a warning says so.  -> LeaveFutureOut."""
        self._need_sampler("leave_future_out")
        I = int(self.topology[0])
        if isinstance(data, str):
            if data not in ("train", "test"):
                raise ValueError(f"data must be 'train', 'test' or an array, not {data!r}")
            if n_fit is not None:
                raise ValueError("n_fit= goes with an array of rows: 'train' and 'test' fix it at the training count")
            full = np.asarray(self.traindata) if data == "train" else np.vstack([np.asarray(self.traindata), np.asarray(self.testdata)])
            n_fit = len(self.traindata)
        else:
            full = np.asarray(data)
            if full.ndim != 2 or full.shape[1] < I + 1:
                raise ValueError(f"data must be 2-D with at least n_in + 1 = {I + 1} columns (inputs, target), got shape {full.shape}")
            if n_fit is None:
                raise ValueError("an array of rows needs n_fit=: the chains have seen rows[:n_fit]")
        rows = np.ascontiguousarray(full[:, :I + 1], dtype=np.float32)
        block, n_fit = int(block), int(n_fit)
        origins = lfo_origins(rows.shape[0], n_fit, block, min_train)
        if refit is not True and refit is not False and not callable(refit):
            raise ValueError("refit must be True, False or a callable(rows) -> a fitted ParallelTempering")
        sel, n_s = self._trace_selection(burn_in, chains, thin)
        if n_s < 2:
            raise ValueError(f"the selection holds {n_s} samples: importance weights need at least 2")
        if k_threshold is None:
            k_threshold = good_k(n_s)

        def score(pt, fit_rows, og):
            kw, _ = pt._trace_selection(burn_in, chains, thin)
            return pt._sampler.lfo(rows, n_fit=fit_rows, origins=og, block=block, r_eff=r_eff, **kw)

        def fit(origin):
            if refit is True:
                return self._lfo_refit(full, origin)
            pt = refit(full[:origin])
            pt._need_sampler("leave_future_out (the refit)")
            return pt

        out = lfo_walk(origins, n_fit, self, score, fit if refit is not False else None, k_threshold=float(k_threshold),
                       max_refits=max_refits)
        high = ~(out["khat"] <= k_threshold) & ~out["exact"]
        if np.any(high):
            why = f"max_refits = {max_refits} was reached" if out["max_refits_hit"] else "refit=False"
            warnings.warn(f"{int(np.count_nonzero(high))} of {high.size} origins have a Pareto k-hat above {k_threshold:.2f} "
                          f"({why}): the PSIS-LFO estimate is unreliable for them", stacklevel=2)
        return LeaveFutureOut(elpd_lfo=float(np.sum(out["elpd_lfo"])), se_elpd_lfo=_se_total(out["elpd_lfo"]), elpd_lfo_i=out["elpd_lfo"],
                              khat=out["khat"], tail_len=out["tail_len"], origins=out["origins"], fit_origin=out["fit_origin"],
                              exact=out["exact"], refit_origins=out["refit_origins"], n_refits=out["n_refits"],
                              k_threshold=float(k_threshold), n_samples=n_s, block=block)

    # ------------------------------------------------------------------ calibration (not in the reference)
    def predictive_calibration(self, data="test", *, burn_in=None, chains="all", thin=1, weights=None, eta=None,
                               quantiles=(0.05, 0.95), levels=(0.5, 0.8, 0.9, 0.95), bins=10, crps=True):
        """Is the predictive band right?  Calibration and proper scores of the predictive distribution of the targets, computed
        on the GPU from the sampled chains.

        Regression: the predictive distribution of y on a row is the mixture (1/S) sum_s N(f_s(x), tau_s^2) with each sample's
        own observation noise tau_s^2 = exp(eta_s) -- not the band of the mean function that posterior_predictive() returns.
        Per row: pit = F(y) (uniform on (0, 1) when the model is calibrated; pit_hist), pred_mean, pred_sd, the quantiles of y
        at the levels `quantiles` (at most 16, in (0, 1)), and crps_i, the continuous ranked probability score (closed form of a
        Gaussian mixture; a sum over all pairs of distinct samples, refused above 65536 of them: thin=, chains= or crps=False).
        coverage[q]: the share of rows inside the central interval of level q, from the PIT; intervals: the mean width and
        interval score of every symmetric pair of quantiles.  Classification: p_mean, the Brier and log scores, and the
        reliability table of the confidence max_k p_mean over `bins` bins with its expected / maximum calibration error.

        Samples, `chains`, `thin`, `weights` (with `eta` for a regression) and `data` as predictive_accuracy().
        -> Calibration."""
        I = int(self.topology[0])
        cls = self.task == TASK_CLS
        qs = check_probability_levels("quantiles", quantiles, _lib.CALIB_MAX_LEVELS)
        lv = check_probability_levels("levels", levels)
        if int(bins) < 1:
            raise ValueError(f"bins = {bins} must be >= 1")
        if isinstance(data, str):
            if data not in ("train", "test"):
                raise ValueError(f"data must be 'train', 'test' or an array, not {data!r}")
            ds = data
            y = np.asarray(self.traindata if data == "train" else self.testdata)[:, I]
        else:
            xa = np.asarray(data)
            if xa.ndim != 2 or xa.shape[1] < I + 1:
                raise ValueError(f"data must be 2-D with at least n_in + 1 = {I + 1} columns (inputs, target), got shape {xa.shape}")
            ds = np.ascontiguousarray(xa[:, :I + 1], dtype=np.float32)
            y = ds[:, I]
        if weights is not None:
            w, mult = self._weights(weights)
            if not cls and eta is None:
                raise ValueError("a regression's weights need eta = log tau^2, one per vector (Sampler.eta_trace())")
            kw = dict(w=w, eta=None if cls else eta, multiplicity=mult)
        self._need_sampler("predictive_calibration")
        if weights is None:
            kw, _ = self._trace_selection(burn_in, chains, thin)
        out = self._sampler.calibration(ds, quantiles=() if cls else qs, crps=bool(crps) and not cls, **kw)
        none = dict.fromkeys(Calibration._fields)
        none.update(n_samples=out["n_samples"], n_distinct=out["n_distinct"])
        if cls:
            sc = classification_scores(out["p_mean"], y, bins)
            none.update(sc, p_mean=out["p_mean"], brier=float(np.mean(sc["brier_i"])), log_score=float(np.mean(sc["log_score_i"])))
            return Calibration(**none)
        y32 = np.asarray(y, dtype=np.float32).astype(np.float64)              # the targets as the device reads them
        q = out["quantiles"]
        none.update(crps_i=out["crps"], pit=out["pit"], pit_hist=pit_histogram(out["pit"], bins), coverage=pit_coverage(out["pit"], lv),
                    quantiles={p: q[k] for k, p in enumerate(qs)}, intervals=interval_scores(qs, q, y32) if qs else {},
                    pred_mean=out["pred_mean"], pred_sd=out["pred_sd"])
        if out["crps"] is not None:
            none["crps"], none["se_crps"] = crps_summary(out["crps"])
        return Calibration(**none)

    # ------------------------------------------------------------------ posterior predictive checks (not in the reference)
    def predictive_check(self, data="train", *, burn_in=None, chains="all", thin=1, weights=None, eta=None, lags=PPC_DEFAULT_LAGS,
                         seed=None, return_samples=False):
        """Does data simulated from the fitted model look like the data?  Posterior predictive checks (BDA3 ch. 6), computed on the
        GPU from the sampled chains.  Every selected sample draws one replicated data set y_rep on the rows
        of `data`; a test quantity T is evaluated on y_rep and on the targets y; p_value = P(T(y_rep, theta) >= T(y, theta)) over
        the samples.  A p-value near 0 or 1 (ppc_flagged) names a feature of the data the model does not reproduce.

        Regression (one output): y_rep = f + tau z with the sample's own tau^2 = exp(eta).  mean, sd, min, max of the series;
        chi2 = sum e^2 and max_abs_resid = max |e| of the standardised residuals e = (y - f) / tau (the replicate's are z);
        resid_acf[k], their autocorrelation at every lag of `lags` (at most 16, in [1, n_rows - 1]; default 1 .. 5), and ljung_box over those
        lags: the Gaussian likelihood assumes independent residuals, which a flat PIT histogram (predictive_calibration) does not
        test.  The rows are taken in the order given -- for the time-series nets that is time.  Classification: y_rep is drawn
        from the sample's class probabilities; deviance = -2 sum log p_label, accuracy against argmax p, class_count[k].

        Samples, `chains`, `thin`, `weights` (with `eta` for a regression) and `data` as predictive_accuracy(); every occurrence
        of a repeated sample (a rejected MH step) draws its own replicate.  `seed`: the Philox key of the draws (stream
        STREAM_PPC; None = the object's seed).  -> PredictiveCheck; t_obs / t_rep with return_samples."""
        I = int(self.topology[0])
        cls = self.task == TASK_CLS
        if isinstance(data, str):
            if data not in ("train", "test"):
                raise ValueError(f"data must be 'train', 'test' or an array, not {data!r}")
            ds = data
            n_rows = len(self.traindata if data == "train" else self.testdata)
        else:
            xa = np.asarray(data)
            if xa.ndim != 2 or xa.shape[1] < I + 1:
                raise ValueError(f"data must be 2-D with at least n_in + 1 = {I + 1} columns (inputs, target), got shape {xa.shape}")
            ds = np.ascontiguousarray(xa[:, :I + 1], dtype=np.float32)
            n_rows = ds.shape[0]
        if n_rows < 2:
            raise ValueError(f"{n_rows} data rows: a posterior predictive check needs at least 2")
        if cls:
            if lags is not PPC_DEFAULT_LAGS and lags is not None and len(lags):
                raise ValueError("lags: a classification has no residual autocorrelation")
            lg = []
        else:
            if int(self.topology[2]) != 1:
                raise ValueError("predictive_check needs a regression net with one output, or a classification")
            if lags is PPC_DEFAULT_LAGS:
                lags = [k for k in PPC_DEFAULT_LAGS if k <= n_rows - 1]
            lg = ppc_check_lags(() if lags is None else lags, n_rows)
        if weights is not None:
            w, mult = self._weights(weights)
            if not cls and eta is None:
                raise ValueError("a regression's weights need eta = log tau^2, one per vector (Sampler.eta_trace())")
            kw = dict(w=w, eta=None if cls else eta, multiplicity=mult)
        self._need_sampler("predictive_check")
        if weights is None:
            kw, _ = self._trace_selection(burn_in, chains, thin)
        out = self._sampler.ppc(ds, lags=lg, seed=self.seed if seed is None else int(seed), samples=bool(return_samples), **kw)
        names = ppc_stat_names(self.task, lags=lg, n_out=int(self.topology[2]))
        p = ppc_p_values(out["n_greater"], out["n_equal"], out["n_defined"])
        by = lambda v: dict(zip(names, (x.item() for x in np.asarray(v))))       # noqa: E731
        return PredictiveCheck(names=names, p_value=by(p), t_obs_mean=by(out["mean_obs"]), t_rep_mean=by(out["mean_rep"]),
                               t_rep_sd=by(np.sqrt(out["var_rep"])), n_defined=by(out["n_defined"]), t_obs=out["t_obs"],
                               t_rep=out["t_rep"], n_samples=out["n_samples"], n_distinct=out["n_distinct"])

    # ------------------------------------------------------------------ power-scaling sensitivity (not in the reference)
    def powerscale_sensitivity(self, data="test", *, quantities=None, delta=0.01, burn_in=None, chains="all",
                               thin=1, weights=None, eta=None, r_eff=None, threshold=0.05):
        """How much do the conclusions depend on the prior, and do prior and data pull against each other?  Power-scaling
        sensitivity (Kallioinen, Paananen, Buerkner & Vehtari 2023), computed on the GPU from one fit.
        The prior (sigma_squared, nu_1, nu_2 of this object) and the likelihood of the training rows are each raised to the powers
        1 / (1 + delta) and 1 + delta by importance-reweighting the samples; the weights are Pareto smoothed as
        predictive_accuracy()'s; D = the distance the marginal of a quantity moves (a symmetrised, cumulative Jensen-Shannon
        distance), per unit of log2 alpha.  diagnosis, at `threshold`: prior and likelihood both >= threshold: "prior-data
        conflict"; prior only: "strong prior / weak likelihood"; else "-" (powerscale_flagged lists the others).

        quantities: None = "weights", "eta" (regression) and "predictions"; else any of "weights" (every w[p]), "eta"
        (regression), "predictions" (f[n], or p[n,k] of a classification, on
        the rows of `data`: "train", "test" or rows with at least n_in columns) and "loglik" (the training log-likelihood).
        Samples, `chains`, `thin`, `weights` (with `eta` for a regression) as predictive_accuracy(); r_eff as there (None: 1).
        A k-hat above good_k(n_samples) means the reweighting is unreliable for that perturbation, and a warning says so.  With
        Langevin proposals the chain is not an exact sampler of the stated posterior (section 15): the diagnostic describes the
        samples it is given.  -> PowerScaling."""
        delta = powerscale_check_delta(delta)
        groups = powerscale_groups(quantities, self.task)
        I, O = int(self.topology[0]), int(self.topology[2])
        n_rows = 0
        ds = "test"
        if "predictions" in groups:
            if isinstance(data, str):
                if data not in ("train", "test"):
                    raise ValueError(f"data must be 'train', 'test' or an array, not {data!r}")
                ds = data
                n_rows = len(self.traindata if data == "train" else self.testdata)
            else:
                xa = np.asarray(data)
                if xa.ndim != 2 or xa.shape[1] < I:
                    raise ValueError(f"data must be 2-D with at least n_in = {I} columns, got shape {xa.shape}")
                ds = np.ascontiguousarray(xa[:, :I], dtype=np.float32)
                n_rows = ds.shape[0]
        cls = self.task == TASK_CLS
        if weights is not None:
            w, mult = self._weights(weights)
            if not cls and eta is None:
                raise ValueError("a regression's weights need eta = log tau^2, one per vector (Sampler.eta_trace())")
            kw = dict(w=w, eta=None if cls else eta, multiplicity=mult)
        self._need_sampler("powerscale_sensitivity")
        if weights is None:
            kw, _ = self._trace_selection(burn_in, chains, thin)
        out = self._sampler.powerscale(ds, groups=groups, delta=float(delta), r_eff=1.0 if r_eff is None else float(r_eff), **kw)
        names = powerscale_names(groups, n_param=self.num_param, n_rows=n_rows, n_out=O, task=self.task)
        by = lambda v: dict(zip(names, (float(x) for x in v)))       # noqa: E731
        lik, pri = by(out["sens"][0]), by(out["sens"][1])
        bsd = out["base_sd"]
        shift, ratio, khat = {}, {}, {}
        with np.errstate(invalid="ignore", divide="ignore"):
            for c, comp in enumerate(POWERSCALE_COMPONENTS):
                for g, sign in enumerate(POWERSCALE_SIGNS):
                    shift[comp, sign] = by((out["mean"][c, g] - out["base_mean"]) / bsd)
                    ratio[comp, sign] = by(out["sd"][c, g] / bsd)
                    khat[comp, sign] = float(out["khat"][c, g])
        gk = good_k(out["n_samples"])
        high = [f"{c} {g}" for (c, g), k in khat.items() if math.isfinite(k) and k > gk]
        if high:
            warnings.warn(f"the Pareto k-hat of the perturbations {high} is above {gk:.2f}: the power-scaled weights are "
                          f"unreliable for them", stacklevel=2)
        return PowerScaling(names=names, prior=pri, likelihood=lik, mean_shift=shift, sd_ratio=ratio, khat=khat,
                            diagnosis={n: powerscale_diagnosis(pri[n], lik[n], threshold) for n in names}, delta=float(delta),
                            threshold=float(threshold), good_k=gk, n_samples=out["n_samples"], n_distinct=out["n_distinct"])

    # ------------------------------------------------------------------ recursive forecasts (not in the reference)
    def forecast(self, horizon, origin="end", *, burn_in=None, chains="all", thin=1, percentiles=(5, 95), noise=False, seed=None,
                 weights=None, eta=None, return_samples=False):
        """Multi-step forecasts past the data with their uncertainty, computed on the GPU from the sampled chains (DESIGN.md
        section 14).  The fitted net is a one-step map x[t+1] = f(x[t-n_in+1 .. t]); each of `horizon` steps feeds its output back
        as the newest input, for every posterior sample, and the spread across samples gives the bands.

        `origin`: "end" -- the window right after the data, testdata[-1, 1:n_in+1]; this assumes the rows are consecutive windows
        of one series with delay 1 (each row's inputs are the previous row's shifted by one, its target the next value), as the
        shipped Data_OneStepAhead series and drivers.takens_embedding build them; "test" / "train" -- every row's inputs, one
        forecast per row (rolling origins); or an array whose first n_in columns are the origin windows.  noise=False: each sample
        runs the deterministic map; noise=True: each step also adds the sample's observation noise exp(eta / 2) z (tau^2 =
        exp(eta), the likelihood's variance), fed back with it, drawn from the Philox stream STREAM_FORECAST of `seed` (None = the
        object's seed).  The sample set is by default the columns of the posterior matrix run_chains() returns: every chain's
        trace rows from int(NumSamples * burn_in) on.  `chains`: "all", "cold" (the temperature-1 chain) or a list of chain
        indices; `thin`: every thin-th row.  With noise the trace's eta is recorded only from a chain's first accepted step on: a
        selection that reaches earlier rows is refused.  `weights`: weight vectors instead of the trace -- [n, num_param] or a
        pair (vectors, integer multiplicities), with `eta` [n] when noise is on.  Percentiles follow np.percentile(method="linear")
        exactly.  -> Forecast(mean, percentiles, samples, n_samples, n_trajectories); outputs are [n_origins, horizon] (one origin
        for "end"), samples [n_samples, n_origins, horizon] in chain-major order.  Regression nets with one output only."""
        self._need_sampler("forecast")
        if self.task == TASK_CLS or int(self.topology[2]) != 1:
            raise ValueError("forecast needs a regression net with one output (a one-step map of one series)")
        I = int(self.topology[0])
        if isinstance(origin, str):
            if origin == "end":
                last = np.asarray(self.testdata)[-1]
                org = np.ascontiguousarray(np.asarray(last[1:I + 1], dtype=np.float32).reshape(1, I))
            elif origin in ("train", "test"):
                org = origin
            else:
                raise ValueError(f"origin must be 'end', 'train', 'test' or an array, not {origin!r}")
        else:
            oa = np.asarray(origin)
            if oa.ndim != 2 or oa.shape[1] < I:
                raise ValueError(f"origin must be 2-D with at least n_in = {I} columns, got shape {oa.shape}")
            org = np.ascontiguousarray(oa[:, :I], dtype=np.float32)
        pcts = list(percentiles)
        if any(not (0 <= p <= 100) for p in pcts):
            raise ValueError(f"percentiles must lie in [0, 100], got {pcts}")
        if weights is not None:
            w, mult = self._weights(weights)
            if noise and eta is None:
                raise ValueError("noise=True with weights= needs eta = log tau^2, one per vector (Sampler.eta_trace())")
            kw = dict(w=w, multiplicity=mult, eta=eta if noise else None)
            M = int(np.sum(np.asarray(mult, dtype=np.int64))) if mult is not None else w.shape[0]
        else:
            kw, M = self._trace_selection(burn_in, chains, thin)
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.forecast(int(horizon), org, noise=bool(noise), seed=self.seed if seed is None else int(seed),
                                     ranks=ranks, samples=bool(return_samples), **kw)
        return Forecast(mean=out["mean"], percentiles=self._bands(out["order_stats"], pcts, spots, ranks), samples=out["samples"], n_samples=out["n_samples"],
                        n_trajectories=out["n_trajectories"])

    # ------------------------------------------------------------------ log evidence (not in the reference)
    def log_evidence(self, *, burn_in=None, thin=1, prior_draws=1 << 20, seed=None, weights=None, return_draws=False):
        """The marginal likelihood log Z of the model, for Bayes factors between topologies (evidence_compare), computed on the GPU
        from every rung of the ladder.  Rung k samples the power posterior pi(w) L(w)^beta_k, beta_k =
        1 / float32(T_k); with U(w) the untempered full-data log-likelihood (a regression's tau^2 integrated out), log Z is
        estimated by thermodynamic integration over the rungs (trapezoid rule, the prior as beta = 0; ti_discretisation the
        ptemcee estimate |TI - TI over every other rung|) and by stepping stones (Xie et al. 2011).  A regression's evidence is
        relative to the improper 1 / tau^2 prior: it cancels in Bayes factors between models fitted to the same training rows.

        The draws of rung k are its trace rows from int(NumSamples * burn_in) up to the temperature switch (the reference's
        pt_samples = 0.6 NumSamples, after which every chain runs at T = 1) or to NumSamples; `thin`: every thin-th row.  The
        prior's point and first stone come from `prior_draws` draws of N(0, sigma^2 I) (Philox stream STREAM_PRIOR of `seed`,
        None = the object's seed).  `weights`: (betas [K], vectors [K, n, num_param]) instead of the trace.  Standard errors
        take each rung's split-ESS of U; they assume independent rungs.  return_draws: also every draw's U.  -> Evidence.

        The estimate is exact only when the tempered chains sample the power posterior: random-walk proposals, swap_rule=1,
        shared_noise=False and a large integer maxtemp (so that the hottest rung is close to the prior); a warning names the
        settings that break this."""
        self._need_sampler("log_evidence")
        S = self.NumSamples
        n_prior = int(prior_draws)
        if n_prior < 2:
            raise ValueError(f"prior_draws = {n_prior}: the prior's point needs at least 2 draws")
        if weights is not None:
            if not isinstance(weights, tuple) or len(weights) != 2:
                raise ValueError("weights must be a pair (betas [K], vectors [K, n, num_param])")
            bw, w = weights
            betas = np.asarray(bw, np.float64).reshape(-1)
            w = np.asarray(w)
            if w.ndim != 3 or w.shape[0] != betas.size or w.shape[2] != self.num_param:
                raise ValueError(f"weights: vectors must be [K = {betas.size}, n, {self.num_param}], got shape {w.shape}")
            if w.shape[1] < 4:
                raise ValueError(f"weights: {w.shape[1]} draws per rung: the split ESS needs at least 4")
            order = np.argsort(betas, kind="stable")
            kw = dict(w=w[order])
        else:
            self._check_trace("weights")
            betas = np.array([1.0 / float(np.float32(T)) for T in self.temperatures])
            order = np.argsort(betas, kind="stable")
            b = self.burn_in if burn_in is None else burn_in
            step0 = int(S * b)
            if step0 < self._freeze_step():
                raise ValueError(f"the window starts at step {step0} (burn_in = {b}), before the adapted ladder froze at step "
                                 f"{self._freeze_step()}: the rungs moved inside it (a larger burn_in)")
            sw = self._pt_switch_step()
            end = sw if sw >= 0 else S
            per = max(0, -(-(end - step0) // max(1, int(thin))))
            if per < 4:
                raise ValueError(f"the window [{step0}, {end}) of every rung (burn_in = {b}, up to the temperature switch) holds "
                                 f"{per} draws at thin = {int(thin)}: at least 4 are needed (a smaller burn_in or more samples)")
            kw = dict(replicas=[int(r) for r in order], step0=step0, nsteps=end - step0, thin=int(thin))
        bs = betas[order]
        if np.any(np.diff(bs) == 0.0):
            raise ValueError(f"duplicate temperatures in the ladder: {sorted(set(bs[np.flatnonzero(np.diff(bs) == 0.0)].tolist()))} "
                             f"(as betas): the rungs must be distinct")
        if bs[-1] != 1.0:
            raise ValueError(f"the coldest rung has beta = {bs[-1]!r}: log Z needs a rung at temperature 1")
        causes = []
        if self.use_langevin_gradients is True and self.langevin_prob > 0:
            causes.append("Langevin proposals at T != 1 (the Hastings term is divided by T)")
        if self.swap_rule == 0:
            causes.append("swap_rule=0 (the reference's cascade uses stale likelihoods)")
        if self.shared_noise:
            causes.append("shared_noise=True (the rungs are correlated, so the standard errors are not valid)")
        if causes:
            warnings.warn("log_evidence: the tempered chains do not sample the power posterior exactly: " + "; ".join(causes)
                          + ". An exact estimate needs random-walk proposals, swap_rule=1, shared_noise=False and a large "
                          "integer maxtemp", stacklevel=2)
        d = np.append(np.diff(bs), 0.0)
        out = self._sampler.evidence(d=d, n_prior=n_prior, seed=self.seed if seed is None else int(seed), a=[0.0, float(bs[0])],
                                     u_out=bool(return_draws), u_prior_out=bool(return_draws), **kw)
        N = int(np.asarray(self.traindata).shape[0])
        r = evidence_from_rungs(bs, out["u_mean"], out["u_var"], out["u_ess"], out["log_stone"], out["stone_relvar"],
                                prior_log_mean_exp_b=out["prior_log_mean_exp"][0], prior_u_mean=out["prior_u_mean"][0],
                                prior_u_var=out["prior_u_var"][0], prior_kish_ess_b=out["prior_kish_ess"][0],
                                prior_log_mean_exp_first=out["prior_log_mean_exp"][1], prior_kish_ess_first=out["prior_kish_ess"][1],
                                n_prior=n_prior, log_c=evidence_log_c(self.task, N))
        kish = float(out["prior_kish_ess"][1])
        if kish < 0.01 * n_prior:
            warnings.warn(f"log_evidence: the first stepping stone's prior draws have a Kish ESS of {kish:.1f} of {n_prior} "
                          f"(below 1 %): the hottest rung (beta = {bs[0]:.4g}) is far from the prior; raise maxtemp", stacklevel=2)
        gap = abs(r["log_z_ti"] - r["log_z_ss"])
        if gap > 3.0 * math.hypot(r["se_log_z_ti"], r["se_log_z_ss"]) + r["ti_discretisation"]:
            warnings.warn(f"log_evidence: thermodynamic integration ({r['log_z_ti']:.4f}) and stepping stones ({r['log_z_ss']:.4f}) "
                          f"disagree by more than their errors: more rungs, more samples or a hotter ladder", stacklevel=2)
        u_draws = None
        if return_draws:
            u_draws = np.split(out["u"], np.cumsum(out["n_draws"])[:-1])
        return Evidence(log_z_ss=r["log_z_ss"], se_log_z_ss=r["se_log_z_ss"], log_z_ti=r["log_z_ti"], se_log_z_ti=r["se_log_z_ti"],
                        ti_discretisation=r["ti_discretisation"], betas=r["betas"], u_mean=r["u_mean"], u_mcse=r["u_mcse"],
                        ess=r["ess"], log_stones=np.concatenate([[out["prior_log_mean_exp"][1]], out["log_stone"][:-1]]),
                        prior_kish_ess=kish, n_draws=np.concatenate([[n_prior], out["n_draws"]]), n_distinct=out["n_distinct"],
                        u_draws=u_draws, u_prior_draws=out["u_prior"] if return_draws else None)

    def make_directory(self, directory):
        if not os.path.exists(directory):
            os.makedirs(directory)
