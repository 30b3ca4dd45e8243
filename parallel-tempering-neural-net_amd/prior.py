"""Prior predictive checks of the drop-in (not in the reference): what the prior implies before any data is looked at.  The
host-only helpers, the result tuple, and the mixin that holds the public method.  The method checks its arguments here, makes one
low-level call of `_lib.Sampler` (the device does the work) and finishes the result with host arithmetic.
"""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import TASK_CLS, TASK_REG, check_percentiles, lerp_percentile, percentile_ranks, ppc_p_values

# prior_predictive's result, S = len(sigma_squared) scales.  Per scale, row and output over the draws: mean, saturated (the share
# of draws with f < eps or f > 1 - eps) [S, n_rows, n_out] float64, percentiles {p: [S, n_rows, n_out]}, vote [S, n_rows, n_out]
# (classification, else None).  Per scale and statistic of the drawn function, over the draws: names; stat_mean, stat_sd, p_value,
# n_greater, n_equal, n_defined {name: [S]}, stat_percentiles {p: {name: [S]}}; t_obs {name: float}, T of the data (nan where it
# has no counterpart, and p_value with it).  t_draw [S, n_draws, len(names)] float64, samples [S, n_draws, n_rows, n_out] float32,
# weights [S, n_draws, num_param] float32: None unless asked for.  n_draws, eps, seed: as used
PriorPredictive = namedtuple("PriorPredictive", "sigma_squared mean percentiles vote saturated names stat_mean stat_sd stat_percentiles "
                                                "p_value n_greater n_equal n_defined t_obs t_draw samples weights n_draws eps seed")

PRIOR_REGRESSION_STATS = ("mean", "sd", "min", "max", "acf1", "rmse", "saturated")
PRIOR_CLASSIFICATION_STATS = ("accuracy", "log_score", "confidence", "saturated")


def prior_stat_names(task, n_out=1):
    """The statistics of a drawn function in the device's order: a regression's (TASK_REG), or a classification's with one
    class_share[k] per class."""
    if task == TASK_REG:
        return list(PRIOR_REGRESSION_STATS)
    return list(PRIOR_CLASSIFICATION_STATS) + [f"class_share[{k}]" for k in range(int(n_out))]


def check_prior_scale(name, value):
    """A prior variance: finite and greater than 0 -> float."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} = {value!r} must be a finite number > 0") from None
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} = {value!r} must be a finite number > 0")
    return v


def prior_scales(sigma_squared, own):
    """sigma_squared= of prior_predictive: None (the object's own), one value or up to 8 -> tuple of floats."""
    if sigma_squared is None:
        return (float(own),)
    values = list(np.atleast_1d(np.asarray(sigma_squared, dtype=object)).reshape(-1))
    if not 1 <= len(values) <= _lib.PRIOR_MAX_SCALES:
        raise ValueError(f"{len(values)} prior scales: between 1 and {_lib.PRIOR_MAX_SCALES} per call")
    return tuple(check_prior_scale(f"sigma_squared[{k}]", v) for k, v in enumerate(values))


def prior_p_values(n_greater, n_equal, n_defined, t_obs):
    """ppc_p_values of the counts of T(f_i) against T(y); nan where the data has no counterpart (t_obs nan)."""
    p = ppc_p_values(n_greater, n_equal, n_defined)
    return np.where(np.isnan(np.asarray(t_obs, dtype=np.float64)), np.nan, p)


def prior_flagged(result, alpha=0.05):
    """For each scale of result.sigma_squared, in their order: the names of the statistics whose prior predictive p-value lies
    outside [alpha / 2, 1 - alpha / 2] -- the features of the data that the prior at that scale all but rules out.  An
    undefined p-value (nan) is not flagged.  -> list of lists."""
    a = float(alpha)
    if not (0.0 < a < 1.0):
        raise ValueError(f"alpha = {alpha} must lie in (0, 1)")
    return [[n for n in result.names if result.p_value[n][s] < a / 2.0 or result.p_value[n][s] > 1.0 - a / 2.0]
            for s in range(len(result.sigma_squared))]


class PriorAnalysis:
    """prior_predictive(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row helper it uses.  It reads
    the constructor's attributes `task`, `topology`, `seed`, `sigma_squared` and `_sampler`."""

    def prior_predictive(self, x="train", *, n_draws=1000, sigma_squared=None, percentiles=(5, 50, 95), eps=0.01, seed=None, draw0=0,
                         target=False, return_draws=False, return_samples=False, return_weights=False):
        """What the prior implies, before any data is looked at, computed on the GPU (Gabry et al. 2019):
        n_draws weight vectors w ~ N(0, sigma_squared I) are drawn, the network is evaluated on the rows `x`, and the drawn
        functions are summarised.  Works as soon as initialize_chains() has made the handle; needs no trace and no run.

        Everything is about f, the output posterior_predictive() returns (a regression's sigmoid output, a classification's class
        probabilities).  tau^2 has an improper prior (nu_1 = nu_2 = 0), so replicated data y is not defined under the prior and
        is not drawn.

        `sigma_squared`: None (the object's own prior variance), one value, or up to 8 for a scan.  All scales use the same
        normal deviates (w = float32(sqrt(s)) z), so curves over the scale are smooth; every result has a leading scale axis.
        `x`: "train", "test" (with their targets) or an array whose first n_in columns are the inputs; with target=True column
        n_in is the target (a classification's: an integer class).  `seed`: None = the object's seed; draw i has the counter
        draw0 + i, so a call with draw0=m continues one that ended at m.  `eps` in (0, 0.5): an output below eps or above 1 - eps
        counts as saturated.  Percentiles follow np.percentile(method="linear") exactly (at most 16 order statistics).

        Per scale, row and output over the draws: mean, percentiles, vote (classification), saturated.  Per scale and draw, the
        statistics `names` of the drawn function over the rows -- a regression's mean, sd, min, max, acf1 (lag-1 autocorrelation),
        rmse, saturated (share of rows); a classification's accuracy, log_score, confidence, saturated (share of rows with max p >
        1 - eps), class_share[k] -- and over the draws their stat_mean, stat_sd, stat_percentiles.  Where the data has a
        counterpart T(y) (t_obs: mean, sd, min, max, acf1 of the target series; the label shares), the counts n_greater, n_equal
        of T(f_i) against it and p_value = (n_greater + n_equal / 2) / n_defined; nan elsewhere.  A draw whose statistic is
        undefined (nan: acf1 of a constant function) is left out of that statistic and of n_defined.  rmse, accuracy and
        log_score need a target and are nan without one.  -> PriorPredictive; prior_flagged() lists the extreme p-values."""
        if self._sampler is None:
            raise ValueError("prior_predictive needs the chains' device handle: call initialize_chains() first")
        if not isinstance(self._sampler, _lib.Sampler):
            raise ValueError("prior_predictive runs on one GPU: a ladder sharded over several devices is not supported")
        xs = self._rows("x", x, target=bool(target))
        n = int(n_draws)
        if n != n_draws or n < 1:
            raise ValueError(f"n_draws = {n_draws!r} must be an integer >= 1")
        d0 = int(draw0)
        if d0 != draw0 or d0 < 0 or d0 + n > 1 << 32:
            raise ValueError(f"draw0 = {draw0!r} with n_draws = {n}: the draws' Philox counters must lie in [0, 2^32)")
        scales = prior_scales(sigma_squared, self.sigma_squared)
        e = float(eps)
        if not (0.0 < e < 0.5):
            raise ValueError(f"eps = {eps!r} must lie in (0, 0.5)")
        pcts = check_percentiles(percentiles)
        spots = percentile_ranks(n, pcts)
        ranks = sorted({r for lo, hi, _ in spots for r in (lo, hi)})
        if len(ranks) > _lib.PREDICT_MAX_RANKS:
            raise ValueError(f"{len(pcts)} percentiles need {len(ranks)} order statistics: at most {_lib.PREDICT_MAX_RANKS} per call")
        key = self.seed if seed is None else int(seed)
        out = self._sampler.prior_predictive(xs, n_draws=n, sigma_squared=scales, draw0=d0, seed=key, ranks=ranks, eps=e,
                                             target=bool(target) and not isinstance(xs, str), t_draw=bool(return_draws),
                                             samples=bool(return_samples), weights=bool(return_weights))
        names = prior_stat_names(self.task, self.topology[2])
        pos = {r: k for k, r in enumerate(ranks)}

        def bands(order_stats):              # [S, n_ranks, ...] -> {p: [S, ...]}
            return {p: lerp_percentile(order_stats[:, pos[lo]], order_stats[:, pos[hi]], g) for p, (lo, hi, g) in zip(pcts, spots)}

        def by_name(a):                      # [S, n_stats] -> {name: [S]}
            return {nm: np.array(a[:, j]) for j, nm in enumerate(names)}
        stat_bands = bands(out["stat_order_stats"]) if ranks else {}
        p = prior_p_values(out["n_greater"], out["n_equal"], out["n_defined"], out["t_obs"][None, :])
        return PriorPredictive(
            sigma_squared=scales, mean=out["mean"], percentiles=bands(out["order_stats"]) if ranks else {},
            vote=out["vote"] if self.task == TASK_CLS else None, saturated=out["sat_count"] / float(n), names=names,
            stat_mean=by_name(out["stat_mean"]), stat_sd=by_name(out["stat_sd"]),
            stat_percentiles={q: by_name(v) for q, v in stat_bands.items()}, p_value=by_name(p),
            n_greater=by_name(out["n_greater"]), n_equal=by_name(out["n_equal"]), n_defined=by_name(out["n_defined"]),
            t_obs={nm: float(out["t_obs"][j]) for j, nm in enumerate(names)}, t_draw=out["t_draw"], samples=out["samples"],
            weights=out["weights"], n_draws=n, eps=e, seed=key)
