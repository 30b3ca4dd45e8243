"""Forecast verification of the drop-in (not in the reference, which scores one-step predictions of the test rows only): how far
ahead can the recursive forecasts of forecast() be trusted?  Proper scores of the k-step predictive distribution per lead time,
the energy score of the whole path, and skill against persistence and climatology.  The host-only
helpers, the result tuple, and the mixin that holds the public method.  The method checks its arguments here, makes one
low-level call of `_lib.Sampler` (the device scores every (origin, step) column) and finishes the per-horizon summary with host
arithmetic in float64.
"""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import check_probability_levels, interval_scores, pit_coverage, pit_histogram

TASK_CLS = _lib.TASK_CLS

# forecast_accuracy's result, R origins, h = horizon steps.  Per horizon [h] (over the origins with truth at that step): n int64,
# rmse, mae, bias of pred_mean, crps, se_crps, log_score, se_log_score, rmse_persistence, mae_persistence, rmse_climatology,
# crps_climatology, rmse_skill, crps_skill float64; coverage {q: [h]}; pit_hist [h, bins] int64; intervals {(p_lo, p_hi):
# dict(level, width [h], score [h])}; skill_horizon int.  Pointwise [R, h] float64, NaN without truth: crps_i, log_score_i, pit,
# pred_mean, pred_sd; quantiles {p: [R, h]}; truth [R, h] float32; origins [R, n_in] float32.  Per origin: energy_score [R] with
# energy_mean, se_energy (floats over the origins scored).  n_samples, n_trajectories.  What was not asked for is None.
ForecastAccuracy = namedtuple("ForecastAccuracy", "horizon n rmse mae bias crps se_crps log_score se_log_score coverage pit_hist "
                                                  "intervals rmse_persistence mae_persistence rmse_climatology crps_climatology "
                                                  "rmse_skill crps_skill skill_horizon crps_i log_score_i pit pred_mean pred_sd "
                                                  "quantiles energy_score energy_mean se_energy truth origins n_samples n_trajectories")


def series_from_windows(rows, n_in):
    """The series that overlapping windows were cut from.  rows [n, >= n_in + 1] (n_in inputs, then the target): stride = the
    smallest s in 1 .. n_in with rows[k + 1, :n_in + 1 - s] == rows[k, s:n_in + 1] for every k, bit for bit; series = the first
    row followed by the last s values of every later one, so that rows[k] == series[k s : k s + n_in + 1].  -> (series, stride).
    Rows that are no such windows (shuffled, or cut with a delay above 1) raise: pass series= instead."""
    a = np.ascontiguousarray(np.asarray(rows)[:, :n_in + 1])
    if a.ndim != 2 or a.shape[1] != n_in + 1 or a.shape[0] < 1:
        raise ValueError(f"rows must be [n, n_in + 1 = {n_in + 1}] windows, got shape {np.asarray(rows).shape}")
    W = n_in + 1
    for s in range(1, n_in + 1):
        if np.ascontiguousarray(a[1:, :W - s]).tobytes() == np.ascontiguousarray(a[:-1, s:]).tobytes():
            return np.concatenate([a[0], a[1:, W - s:].reshape(-1)]), s
    raise ValueError(f"the rows are not overlapping windows of one series (no stride in 1 .. {n_in} makes each row continue the one "
                     f"before it): pass series= (and stride=) instead")


def windows_and_truth(series, n_in, horizon, stride=1, n_origins=None):
    """Origin windows series[t : t + n_in] at t = 0, stride, ... (as many as have a value after them, or n_origins) and the values
    that follow them: truth[r, k - 1] = series[r stride + n_in - 1 + k], k = 1 .. horizon, NaN past the end of the series.
    -> (origins [R, n_in] float32, truth [R, horizon] float32)."""
    x = np.asarray(series, dtype=np.float32).reshape(-1)
    s, h = int(stride), int(horizon)
    if s < 1:
        raise ValueError(f"stride = {stride} must be >= 1")
    if h < 1:
        raise ValueError(f"horizon = {horizon} must be >= 1")
    R = (x.size - n_in - 1) // s + 1 if x.size > n_in else 0
    if n_origins is not None:
        R = min(R, int(n_origins))
    if R < 1:
        raise ValueError(f"a series of {x.size} values holds no window of n_in = {n_in} inputs with a value after it")
    t0 = np.arange(R) * s
    origins = np.ascontiguousarray(x[t0[:, None] + np.arange(n_in)[None, :]])
    idx = t0[:, None] + n_in + np.arange(h)[None, :]
    truth = np.full((R, h), np.nan, dtype=np.float32)
    ok = idx < x.size
    truth[ok] = x[idx[ok]]
    return origins, truth


def crps_gaussian(y, mu, sigma):
    """The CRPS of N(mu, sigma^2) at y (Gneiting & Raftery 2007, eq. 21), elementwise in float64."""
    y = np.asarray(y, dtype=np.float64)
    z = (y - mu) / sigma
    erf = np.vectorize(math.erf, otypes=[np.float64])
    cdf = 0.5 * (1.0 + erf(z / math.sqrt(2.0)))
    pdf = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return sigma * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - 1.0 / math.sqrt(math.pi))


def _mean_se(x):
    """-> (mean, sd(ddof 1) / sqrt(n)) of a 1-D array; NaN where undefined."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return float("nan"), float("nan")
    return float(np.mean(x)), (float(np.std(x, ddof=1) / math.sqrt(x.size)) if x.size > 1 else float("nan"))


def energy_score_ensemble(paths, y, weights=None):
    """The energy score of an ensemble of paths [M, d] against y [d] (Gneiting et al. 2008): (1/M) sum_i c_i |Y_i - y| -
    (1 / (2 M^2)) sum_i sum_j c_i c_j |Y_i - Y_j|, i = j included, M = sum c; the O(M^2) float64 sum.  With d = 1 it is the CRPS
    of the ensemble."""
    Y = np.asarray(paths, dtype=np.float64).reshape(len(paths), -1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    c = np.ones(Y.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    M = float(np.sum(c))
    first = float(np.sum(c * np.sqrt(np.sum((Y - y[None, :]) ** 2, axis=1)))) / M
    pair = np.sqrt(np.sum((Y[:, None, :] - Y[None, :, :]) ** 2, axis=2))
    return first - float(c @ pair @ c) / (2.0 * M * M)


def horizon_summary(truth, pred_mean, *, crps=None, log_score=None, pit=None, levels=(0.5, 0.8, 0.9, 0.95), bins=10,
                    quantile_levels=(), quantiles=None):
    """The per-horizon summary of pointwise [R, h] results, over the origins with (finite) truth at each step: n, rmse / mae / bias
    of pred_mean, the means of crps and log_score with their standard errors sd(ddof 1) / sqrt(n), coverage {q: [h]} and pit_hist
    [h, bins] from the PIT, intervals {(p_lo, p_hi): dict(level, width [h], score [h])} from the quantiles (interval_scores per
    step).  A step without truth gives NaN.  The origins of a rolling forecast overlap: the standard errors ignore the
    autocorrelation this causes and are optimistic.  Host arithmetic only.  -> dict."""
    y = np.asarray(truth, dtype=np.float32).astype(np.float64)
    R, h = y.shape
    lv = check_probability_levels("levels", levels)
    qs = [float(p) for p in quantile_levels]
    nan = lambda: np.full(h, np.nan)                    # noqa: E731
    out = dict(n=np.zeros(h, np.int64), rmse=nan(), mae=nan(), bias=nan(), crps=None, se_crps=None, log_score=None,
               se_log_score=None, coverage=None, pit_hist=None, intervals=None)
    for name, src in (("crps", crps), ("log_score", log_score)):
        if src is not None:
            out[name], out["se_" + name] = nan(), nan()
    if pit is not None:
        out["coverage"] = {q: nan() for q in lv}
        out["pit_hist"] = np.zeros((h, int(bins)), np.int64)
    iv = {}
    for k in range(h):
        ok = np.isfinite(y[:, k])
        n = int(np.sum(ok))
        out["n"][k] = n
        if n == 0:
            continue
        e = np.asarray(pred_mean, np.float64)[ok, k] - y[ok, k]
        out["rmse"][k], out["mae"][k], out["bias"][k] = math.sqrt(float(np.mean(e * e))), float(np.mean(np.abs(e))), float(np.mean(e))
        for name, src in (("crps", crps), ("log_score", log_score)):
            if src is not None:
                out[name][k], out["se_" + name][k] = _mean_se(np.asarray(src, np.float64)[ok, k])
        if pit is not None:
            pk = np.asarray(pit, np.float64)[ok, k]
            for q, share in pit_coverage(pk, lv).items():
                out["coverage"][q][k] = share
            out["pit_hist"][k] = pit_histogram(pk, bins)
        if qs and quantiles is not None:
            for pair, d in interval_scores(qs, np.asarray(quantiles, np.float64)[:, ok, k], y[ok, k]).items():
                slot = iv.setdefault(pair, dict(level=d["level"], width=nan(), score=nan()))
                slot["width"][k], slot["score"][k] = d["width"], d["score"]
    if qs and quantiles is not None:
        out["intervals"] = iv
    return out


def forecast_baselines(last_value, truth, train_targets, crps=True):
    """The two reference forecasts per horizon.  Persistence: the origin window's last value at every step (rmse_persistence,
    mae_persistence).  Climatology: N(m, s^2) with m, s the mean and sd (ddof 1) of the training targets (rmse_climatology,
    crps_climatology by the closed-form Gaussian CRPS).  -> dict of [h] arrays over the origins with truth at each step."""
    y = np.asarray(truth, dtype=np.float32).astype(np.float64)
    last = np.asarray(last_value, dtype=np.float32).astype(np.float64).reshape(-1)
    t = np.asarray(train_targets, dtype=np.float64).reshape(-1)
    m, s = float(np.mean(t)), (float(np.std(t, ddof=1)) if t.size > 1 else float("nan"))
    h = y.shape[1]
    out = {k: np.full(h, np.nan) for k in ("rmse_persistence", "mae_persistence", "rmse_climatology", "crps_climatology")}
    for k in range(h):
        ok = np.isfinite(y[:, k])
        if not np.any(ok):
            continue
        e = last[ok] - y[ok, k]
        out["rmse_persistence"][k], out["mae_persistence"][k] = math.sqrt(float(np.mean(e * e))), float(np.mean(np.abs(e)))
        out["rmse_climatology"][k] = math.sqrt(float(np.mean((m - y[ok, k]) ** 2)))
        if crps and s > 0.0:
            out["crps_climatology"][k] = float(np.mean(crps_gaussian(y[ok, k], m, s)))
    return out


def forecast_skill(rmse, rmse_persistence, crps=None, crps_climatology=None):
    """rmse_skill = 1 - rmse / rmse_persistence, crps_skill = 1 - crps / crps_climatology (positive = better than the baseline),
    skill_horizon = the number of leading steps with crps_skill > 0.  -> (rmse_skill [h], crps_skill [h] or None, skill_horizon or
    None)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = 1.0 - np.asarray(rmse, np.float64) / np.asarray(rmse_persistence, np.float64)
        if crps is None:
            return rs, None, None
        cs = 1.0 - np.asarray(crps, np.float64) / np.asarray(crps_climatology, np.float64)
    lead = 0
    while lead < cs.size and cs[lead] > 0.0:
        lead += 1
    return rs, cs, lead


def forecast_compare(a, b):
    """Two ForecastAccuracy results on the same origins and truth, a - b: per horizon the paired mean difference and its standard
    error sd(ddof 1) / sqrt(n) of crps and of log_score over the columns both scored, and the same of the energy score over the
    origins both scored.  Refused unless both were scored on bitwise-equal truth.  (Smaller is better for crps and the energy
    score, larger for log_score; the standard errors ignore the overlap of rolling origins.)
    -> dict(crps_diff, se_crps_diff, log_score_diff, se_log_score_diff [h]; energy_diff, se_energy_diff floats; None where a
    result lacks the score)."""
    ta, tb = np.asarray(a.truth, np.float32), np.asarray(b.truth, np.float32)
    if ta.shape != tb.shape or ta.tobytes() != tb.tobytes():
        raise ValueError(f"the two results were scored on different truth ({ta.shape} vs {tb.shape}, or other values): "
                         f"forecast_compare needs the same origins and horizon")
    h = ta.shape[1]
    out = dict(crps_diff=None, se_crps_diff=None, log_score_diff=None, se_log_score_diff=None, energy_diff=None, se_energy_diff=None)
    for name, xa, xb in (("crps", a.crps_i, b.crps_i), ("log_score", a.log_score_i, b.log_score_i)):
        if xa is None or xb is None:
            continue
        d = np.asarray(xa, np.float64) - np.asarray(xb, np.float64)
        m, se = np.full(h, np.nan), np.full(h, np.nan)
        for k in range(h):
            m[k], se[k] = _mean_se(d[np.isfinite(d[:, k]), k])
        out[name + "_diff"], out["se_" + name + "_diff"] = m, se
    if a.energy_score is not None and b.energy_score is not None:
        d = np.asarray(a.energy_score, np.float64) - np.asarray(b.energy_score, np.float64)
        out["energy_diff"], out["se_energy_diff"] = _mean_se(d[np.isfinite(d)])
    return out


class VerificationAnalysis:
    """forecast_accuracy(), for `ParallelTemperingBase` to inherit beside `PosteriorAnalysis`, whose helpers (`_need_sampler`,
    `_rows`, `_host_rows`, `_sample_source`) and attributes it uses."""

    def forecast_accuracy(self, horizon, data="test", *, series=None, stride=None, burn_in=None, chains="all", thin=1, weights=None,
                          eta=None, noise=True, seed=None, quantiles=(0.05, 0.95), levels=(0.5, 0.8, 0.9, 0.95), bins=10, crps=True,
                          energy=True):
        """How far ahead can the forecast be trusted?  The recursive forecasts of forecast() from rolling origins, scored against
        the values that followed, per lead time k = 1 .. horizon, on the GPU.

        The k-step predictive distribution is the mixture (1/M) sum_i N(mu_{i,k}, tau_i^2) over the trajectories of forecast():
        mu the net's output at step k before that step's noise is added, tau_i^2 = exp(eta_i).  noise=True (the honest
        predictive): every sample's observation noise is fed back, step by step (seed: the Philox seed of forecast(), None = the
        object's); noise=False: the deterministic maps only, which shows how much of the spread at step k comes from fed-back
        noise.  Per (origin, step): pit, pred_mean, pred_sd, quantiles, crps_i (crps=True; all pairs of trajectories, refused
        above 65536 of them: thin=, chains=, crps=False) and log_score_i, defined as predictive_calibration() defines them.  Per
        origin: energy_score (energy=True; same cap), the energy score of the whole path over the steps with truth -- it also
        sees whether the dependence between steps is right, which no per-step score does.

        Origins and truth: `data` ("test", "train" or rows [n, n_in + 1]) must be overlapping windows of one series
        (series_from_windows finds the stride; origin r = row r's inputs, step 1's truth the row's own target, later steps the
        values that followed, missing past the end of the rows); or `series` (1-D) with `stride` (default 1): windows series[t : t +
        n_in] at t = 0, stride, ... and the values after them.

        Per horizon over the origins with truth: n, rmse / mae / bias of pred_mean, crps +- se_crps, log_score +- se_log_score,
        coverage[q] of the central intervals `levels` (from the PIT), pit_hist [horizon, bins], intervals (mean width and interval
        score of every symmetric pair of `quantiles`); the baselines rmse_persistence, mae_persistence (the origin's last value)
        and rmse_climatology, crps_climatology (N(m, s^2) of the training targets); rmse_skill = 1 - rmse / rmse_persistence,
        crps_skill = 1 - crps / crps_climatology and skill_horizon, the number of leading steps with crps_skill > 0.  Rolling
        origins overlap, so their scores are autocorrelated: every se here ignores that and is optimistic.

        Samples, `chains`, `thin`, `weights` (with `eta`) as predictive_calibration().  -> ForecastAccuracy."""
        I = int(self.topology[0])
        hz = int(horizon)
        if hz < 1:
            raise ValueError(f"horizon = {horizon} must be >= 1")
        if self.task == TASK_CLS or int(self.topology[2]) != 1:
            raise ValueError("forecast_accuracy needs a regression net with one output (a one-step map of one series)")
        qs = check_probability_levels("quantiles", quantiles, _lib.CALIB_MAX_LEVELS)
        lv = check_probability_levels("levels", levels)
        if int(bins) < 1:
            raise ValueError(f"bins = {bins} must be >= 1")
        if series is not None:
            org, truth = windows_and_truth(series, I, hz, 1 if stride is None else stride)
        else:
            rows = self._host_rows(self._rows("data", data, target=True))
            ser, s = series_from_windows(np.asarray(rows, dtype=np.float32), I)
            if stride is not None and int(stride) != s:
                raise ValueError(f"stride = {stride} but the rows overlap with stride {s}; pass series= for another spacing")
            org, truth = windows_and_truth(ser, I, hz, s, n_origins=np.asarray(rows).shape[0])
        kw, _ = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=True, late_handle="forecast_accuracy")
        out = self._sampler.forecast_score(hz, org, truth, noise=bool(noise), seed=self.seed if seed is None else int(seed),
                                           quantiles=qs, crps=bool(crps), energy=bool(energy), **kw)
        q = out["quantiles"]
        sm = horizon_summary(truth, out["pred_mean"], crps=out["crps"], log_score=out["log_score"], pit=out["pit"], levels=lv,
                             bins=bins, quantile_levels=qs, quantiles=q)
        base = forecast_baselines(org[:, I - 1], truth, np.asarray(self.traindata)[:, I], crps=bool(crps))
        rs, cs, lead = forecast_skill(sm["rmse"], base["rmse_persistence"], sm["crps"], base["crps_climatology"])
        es = out["energy_score"]
        e_mean, e_se = _mean_se(es[np.isfinite(es)]) if es is not None else (None, None)
        return ForecastAccuracy(horizon=hz, rmse_skill=rs, crps_skill=cs, skill_horizon=lead, crps_i=out["crps"],
                                log_score_i=out["log_score"], pit=out["pit"], pred_mean=out["pred_mean"], pred_sd=out["pred_sd"],
                                quantiles={p: q[k] for k, p in enumerate(qs)} if qs else {}, energy_score=es, energy_mean=e_mean,
                                se_energy=e_se, truth=truth, origins=org, n_samples=out["n_samples"],
                                n_trajectories=out["n_trajectories"], **sm, **base)
