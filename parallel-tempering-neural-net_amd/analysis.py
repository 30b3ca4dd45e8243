"""The posterior analysis calls of the drop-in (none is in the reference): their host-only helpers and result tuples, and the
class that holds the eleven public methods.  Every method checks its arguments here, makes one low-level call of `_lib.Sampler`
(the device does the work) and finishes the result with host arithmetic.
"""
import math
import shutil
import tempfile
import warnings
from collections import namedtuple

import numpy as np

from . import _lib

TASK_REG, TASK_CLS = _lib.TASK_REG, _lib.TASK_CLS

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


def check_percentiles(percentiles):
    """Percentiles inside [0, 100] -> list."""
    pcts = list(percentiles)
    if any(not (0 <= p <= 100) for p in pcts):
        raise ValueError(f"percentiles must lie in [0, 100], got {pcts}")
    return pcts


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

# rank_diagnostics' result: names [Q]; r_hat = max(r_hat_bulk, r_hat_tail), r_hat_bulk, r_hat_tail, ess_bulk, ess_tail, ess_median
# [Q] float64; ess_quantile {p: [Q]} for the probs asked for; ess_bulk_chain, ess_tail_chain [n_chains, Q] or None; rank_hist
# [n_chains, bins, Q] int64; z [n_chains, 2 (n_draws // 2), Q] float64 or None; n_chains, n_draws
RankConvergence = namedtuple("RankConvergence", "names r_hat r_hat_bulk r_hat_tail ess_bulk ess_tail ess_median ess_quantile "
                             "ess_bulk_chain ess_tail_chain rank_hist z n_chains n_draws")


def rank_check_bins(bins):
    """The bins of a rank histogram: an integer in [2, 64] -> int."""
    b = int(bins)
    if b != bins or not 2 <= b <= _lib.RANK_MAX_BINS:
        raise ValueError(f"bins = {bins!r} must be an integer in [2, {_lib.RANK_MAX_BINS}]")
    return b


def rank_uniformity(result):
    """Chi-square statistics [n_chains, Q] of each chain's rank histogram against the uniform one: sum over the bins of
    (count - e)^2 / e with e = the chain's kept draws / bins.  Under mixing, and without ties, a chain's statistic is roughly
    chi-square with bins - 1 degrees of freedom; autocorrelation inflates it and ties (every rejected step repeats a row, and tied
    draws share one average rank, hence one bin) make the reference distribution approximate, so read it as a ranking of chains
    and quantities, not as a test.  nan where a quantity has no counts (a draw that is not finite)."""
    hist = np.asarray(result.rank_hist, dtype=np.float64)
    expect = hist.sum(axis=1, keepdims=True) / hist.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(expect[:, 0] > 0, ((hist - expect) ** 2 / expect).sum(axis=1), np.nan)


def rank_flagged(result, r_hat=1.01, ess_per_chain=100):
    """The names whose r_hat exceeds `r_hat`, or whose ess_bulk or ess_tail lies below ess_per_chain * n_chains (the thresholds of
    Vehtari et al. 2021); a figure that is nan is flagged."""
    need = ess_per_chain * result.n_chains
    with np.errstate(invalid="ignore"):
        ok = (result.r_hat <= r_hat) & (result.ess_bulk >= need) & (result.ess_tail >= need)
    return [nm for nm, good in zip(result.names, ok) if not good]


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

# what weights= without eta= is refused with where a regression's likelihood needs it (forecast has a wording of its own)
_ETA_REFUSAL = "a regression's weights need eta = log tau^2, one per vector (Sampler.eta_trace())"


class PosteriorAnalysis:
    """The eleven posterior analysis methods, for `ParallelTemperingBase` to inherit.  They use the constructor's attributes
    (`task`, `topology`, `num_param`, `num_chains`, `NumSamples`, `traindata`, `testdata`, `temperatures`, `burn_in`, `seed`,
    `label_swap`, `trace_capacity`, `swap_rule`, `shared_noise`, `use_langevin_gradients`, `langevin_prob`, `_sampler`,
    `_finished`; leave_future_out's refit also the constructor arguments it kept) and, for log_evidence, the driver's
    `_freeze_step()` and `_pt_switch_step()`."""

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

    def _rows(self, name, value, target=False):
        """A rows argument as `Sampler` takes it: 'train' or 'test' as they are, an array cut to its first n_in columns (with
        `target` n_in + 1: the inputs and the target) as contiguous float32."""
        if isinstance(value, str):
            if value not in ("train", "test"):
                raise ValueError(f"{name} must be 'train', 'test' or an array, not {value!r}")
            return value
        cols = int(self.topology[0]) + bool(target)
        a = np.asarray(value)
        if a.ndim != 2 or a.shape[1] < cols:
            what = f"n_in + 1 = {cols} columns (inputs, target)" if target else f"n_in = {cols} columns"
            raise ValueError(f"{name} must be 2-D with at least {what}, got shape {a.shape}")
        return np.ascontiguousarray(a[:, :cols], dtype=np.float32)

    def _host_rows(self, rows):
        """What _rows() returned, on the host: the object's own rows for 'train' / 'test'."""
        return np.asarray(self.traindata if rows == "train" else self.testdata) if isinstance(rows, str) else rows

    def _sample_source(self, weights, burn_in, chains, thin, *, eta=None, need_eta=None, eta_refusal=_ETA_REFUSAL, count=False,
                       late_handle=None):
        """The samples of a call: `weights` (see _weights) or else the trace selection -> (Sampler source keywords, sample count;
        of weights only with `count`).  need_eta: None = the call takes no eta, False = it has no use for the one given, True =
        weights must come with it, else `eta_refusal`.  late_handle: the method's name where the handle is looked at only here,
        after the weights' checks and before the trace's (predictive_calibration, predictive_check, powerscale_sensitivity)."""
        if weights is not None:
            w, mult = self._weights(weights)
            if need_eta and eta is None:
                raise ValueError(eta_refusal)
            kw = dict(w=w, multiplicity=mult)
            if need_eta is not None:
                kw["eta"] = eta if need_eta else None
            M = None
            if count:
                M = int(np.sum(np.asarray(mult, dtype=np.int64))) if mult is not None else w.shape[0]
        if late_handle is not None:
            self._need_sampler(late_handle)
        if weights is None:
            kw, M = self._trace_selection(burn_in, chains, thin)
        return kw, M

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
        xs = self._rows("x", x)
        pcts = check_percentiles(percentiles)
        kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
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
        xs = self._rows("x", x)
        pcts = check_percentiles(percentiles)
        kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
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
    def _convergence_quantities(self, method, burn_in, chains, thin, params, scalars, draws):
        """The quantities of convergence_diagnostics and rank_diagnostics: host draws (names q0 ..), else the selected trace rows
        with the weights `params` and the scalar traces `scalars` -> (names, Sampler source keywords)."""
        self._need_sampler(method)
        if draws is not None:
            d = np.asarray(draws)
            if d.ndim != 3:
                raise ValueError(f"draws must be [n_chains, n_draws, n_quantities], got shape {d.shape}")
            return [f"q{k}" for k in range(d.shape[2])], dict(draws=d)
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
        return names, dict(params=pidx, scalars=sorted(cols), **kw)

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
        names, source = self._convergence_quantities("convergence_diagnostics", burn_in, chains, thin, params, scalars, draws)
        out = self._sampler.convergence(per_chain=per_chain, n_lags=n_lags, **source)
        sd = np.sqrt(out["var"])
        with np.errstate(invalid="ignore", divide="ignore"):
            mcse = sd / np.sqrt(out["ess"])
        return Convergence(names=names, mean=out["mean"], sd=sd, r_hat=out["r_hat"], ess=out["ess"], mcse_mean=mcse,
                           ess_chain=out["ess_chain"], rho=out["rho"], trunc_lag=out["trunc_lag"], n_chains=out["n_chains"],
                           n_draws=out["n_draws"])

    def rank_diagnostics(self, *, burn_in=None, chains="all", thin=1, params=None, scalars=("likelihood",), per_chain=False, probs=(),
                         bins=20, draws=None, return_z=False):
        """The rank-normalised split-R-hat, the bulk and tail effective sample sizes and the per-chain rank histograms of weights
        and scalar traces (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021), computed on the GPU from the
        traces it already holds: the figures Stan, `posterior` and ArviZ report, beside the classic ones of convergence_diagnostics.

        The pooled kept draws of a quantity (each chain's first and last half) are replaced by the normal scores z of their average
        ranks, ties sharing a rank.  r_hat_bulk and ess_bulk are the split-R-hat and split-ESS of z; r_hat_tail is that R-hat of the
        scores of |x - median|, which sees chains that agree in location but not in scale; r_hat is the larger.  ess_tail is the
        smaller split-ESS of the indicators of the 5 % and 95 % quantiles, ess_median that of the median, `probs` asks for further
        quantiles (at most 16, in (0, 1)).  None of them needs a finite variance.  rank_hist counts every chain's draws per `bins`
        equal rank ranges (2 .. 64): under mixing each chain's histogram is flat (rank_uniformity); rank_flagged applies the
        thresholds r_hat <= 1.01 and ESS >= 100 per chain.  A constant quantity has nan figures; one with a draw that is not
        finite has nan figures and an empty histogram.

        Selection (`burn_in`, `chains`, `thin`, `params`, `scalars`, `draws`), names and refusals are those of
        convergence_diagnostics; chains="all" over a ladder also measures the spread between temperatures, chains="cold" with
        per_chain=True gives the posterior's own figures: ess_bulk_chain and ess_tail_chain rank each chain's draws on their own.
        `return_z`: also the bulk scores z [n_chains, 2 (n_draws // 2), Q] in the order of the kept draws, for rank plots.
        -> RankConvergence(names, r_hat, r_hat_bulk, r_hat_tail, ess_bulk, ess_tail, ess_median, ess_quantile {p: [Q]},
        ess_bulk_chain, ess_tail_chain, rank_hist, z, n_chains, n_draws)."""
        names, source = self._convergence_quantities("rank_diagnostics", burn_in, chains, thin, params, scalars, draws)
        pr = check_probability_levels("probs", probs, _lib.RANK_MAX_PROBS)
        out = self._sampler.rank_convergence(probs=pr, n_bins=rank_check_bins(bins), per_chain=per_chain, z=return_z, **source)
        with np.errstate(invalid="ignore"):
            r_hat = np.where(np.isnan(out["r_hat_bulk"]) | np.isnan(out["r_hat_tail"]), np.nan, np.maximum(out["r_hat_bulk"], out["r_hat_tail"]))
        return RankConvergence(names=names, r_hat=r_hat, r_hat_bulk=out["r_hat_bulk"], r_hat_tail=out["r_hat_tail"],
                               ess_bulk=out["ess_bulk"], ess_tail=out["ess_tail"], ess_median=out["ess_median"],
                               ess_quantile={p: out["ess_quantile"][k] for k, p in enumerate(pr)},
                               ess_bulk_chain=out["ess_bulk_chain"], ess_tail_chain=out["ess_tail_chain"], rank_hist=out["rank_hist"],
                               z=out["z"], n_chains=out["n_chains"], n_draws=out["n_draws"])

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
        if loglik is not None:
            mult = None
            if isinstance(loglik, tuple):
                loglik, mult = loglik
            kw = dict(loglik=np.asarray(loglik, dtype=np.float64), multiplicity=mult)
            ds = "test"
        else:
            ds = self._rows("data", data, target=True)
            kw, _ = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=self.task != TASK_CLS)
        out = self._sampler.elpd(ds, r_eff=r_eff, loglik_out=bool(return_pointwise) and loglik is None, **kw)
        lppd_i, p_waic_i, loo_i, khat = out["lppd"], out["p_waic"], out["elpd_loo"], out["khat"]
        waic_i = lppd_i - p_waic_i
        n_s = out["n_samples"]
        gk = good_k(n_s)
        high = np.isfinite(khat) & (khat > gk)
        n_high = int(np.count_nonzero(high))
        if n_high:
            warnings.warn(f"{n_high} of {khat.size} rows have a Pareto k-hat above {gk:.2f}: the PSIS-LOO estimate is "
                          f"unreliable for them", stacklevel=2)
        elpd_loo = float(np.sum(loo_i))
        return PredictiveAccuracy(elpd_loo=elpd_loo, se_elpd_loo=_se_total(loo_i), p_loo=float(np.sum(lppd_i)) - elpd_loo,
                                  elpd_waic=float(np.sum(waic_i)), se_elpd_waic=_se_total(waic_i), p_waic=float(np.sum(p_waic_i)),
                                  lppd=float(np.sum(lppd_i)), se_lppd=_se_total(lppd_i), lppd_i=lppd_i, elpd_loo_i=loo_i,
                                  p_waic_i=p_waic_i, khat=khat, good_k=gk, n_high_k=n_high,
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
        rows = self._rows("data", data, target=True)
        if isinstance(rows, str):
            if n_fit is not None:
                raise ValueError("n_fit= goes with an array of rows: 'train' and 'test' fix it at the training count")
            full = np.asarray(self.traindata) if data == "train" else np.vstack([np.asarray(self.traindata), np.asarray(self.testdata)])
            n_fit = len(self.traindata)
            rows = np.ascontiguousarray(full[:, :int(self.topology[0]) + 1], dtype=np.float32)
        else:
            full = np.asarray(data)                           # what a refit is given: every column, as it came
            if n_fit is None:
                raise ValueError("an array of rows needs n_fit=: the chains have seen rows[:n_fit]")
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
        ds = self._rows("data", data, target=True)
        y = self._host_rows(ds)[:, I]
        kw, _ = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=not cls, late_handle="predictive_calibration")
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
        cls = self.task == TASK_CLS
        ds = self._rows("data", data, target=True)
        n_rows = len(self._host_rows(ds))
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
        kw, _ = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=not cls, late_handle="predictive_check")
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
        O = int(self.topology[2])
        n_rows = 0
        ds = "test"
        if "predictions" in groups:
            ds = self._rows("data", data)
            n_rows = len(self._host_rows(ds))
        cls = self.task == TASK_CLS
        kw, _ = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=not cls, late_handle="powerscale_sensitivity")
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
        if isinstance(origin, str) and origin == "end":
            last = np.asarray(self.testdata)[-1]
            org = np.ascontiguousarray(np.asarray(last[1:I + 1], dtype=np.float32).reshape(1, I))
        elif isinstance(origin, str) and origin not in ("train", "test"):
            raise ValueError(f"origin must be 'end', 'train', 'test' or an array, not {origin!r}")
        else:
            org = self._rows("origin", origin)
        pcts = check_percentiles(percentiles)
        kw, M = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=bool(noise), count=True, eta_refusal=(
            "noise=True with weights= needs eta = log tau^2, one per vector (Sampler.eta_trace())"))
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.forecast(int(horizon), org, noise=bool(noise), seed=self.seed if seed is None else int(seed),
                                     ranks=ranks, samples=bool(return_samples), **kw)
        return Forecast(mean=out["mean"], percentiles=self._bands(out["order_stats"], pcts, spots, ranks), samples=out["samples"], n_samples=out["n_samples"],
                        n_trajectories=out["n_trajectories"])

    def _rung_source(self, name, burn_in, thin, weights):
        """The rungs of log_evidence and rung_reweighting: every chain's trace rows from int(NumSamples * burn_in) up to the
        temperature switch, every thin-th, or `weights` = (betas [K], vectors [K, n, num_param]); the refusals, and the warning
        (under `name`) about settings under which the chains do not sample the power posterior.  -> (betas ascending, Sampler
        source keywords, the rungs' order: the chain or the row of `weights` of every beta)."""
        S = self.NumSamples
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
            warnings.warn(f"{name}: the tempered chains do not sample the power posterior exactly: " + "; ".join(causes)
                          + ". An exact estimate needs random-walk proposals, swap_rule=1, shared_noise=False and a large "
                          "integer maxtemp", stacklevel=3)
        return bs, kw, order

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
        n_prior = int(prior_draws)
        if n_prior < 2:
            raise ValueError(f"prior_draws = {n_prior}: the prior's point needs at least 2 draws")
        bs, kw, _ = self._rung_source("log_evidence", burn_in, thin, weights)
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
