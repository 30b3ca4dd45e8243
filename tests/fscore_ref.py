"""Float64 restatement of ptnn_forecast_score: the trajectories of forecast_ref with their pre-noise means,
the per-column scores of the mixture (1/M) sum_i c_i N(mu_i, tau_i^2) through calibration_ref, the log score as a plain
logsumexp, and the energy score of the path as the O(M^2) numpy double sum."""
import math

import numpy as np

import calibration_ref as cref
import forecast_ref as fref
from parity import orc

LOG_2PI = math.log(2.0 * math.pi)


def trajectories(w, origins, horizon, topo, eta=None, seed=0, traj_index=None):
    """forecast_ref.trajectories, also returning the means: (paths, mu) [n, n_origins, horizon] float64, mu the map's output at
    every step before that step's noise exp(eta / 2) z_k is added (eta None: mu = paths)."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    win0 = np.atleast_2d(np.asarray(origins, dtype=np.float64))[:, :topo[0]]
    n, R = w.shape[0], win0.shape[0]
    idx = np.arange(n) if traj_index is None else np.asarray(traj_index)
    paths, mu = np.empty((n, R, horizon)), np.empty((n, R, horizon))
    for v in range(n):
        win = win0.copy()
        z = None
        if eta is not None:
            sd = np.exp(0.5 * np.float64(np.float32(eta[v])))
            z = np.stack([fref.noise_draws(horizon, int(idx[v]), r, seed) for r in range(R)])
        for k in range(horizon):
            m = orc.forward(win, w[v], topo)[1][:, 0]
            y = m if z is None else m + sd * z[:, k]
            mu[v, :, k], paths[v, :, k] = m, y
            win = np.concatenate([win[:, 1:], y[:, None]], axis=1)
    return paths, mu


def log_score(y, mu, eta, multiplicity=None):
    """log (1/S) sum c N(y; mu, exp(eta)): a plain logsumexp in float64."""
    mu = np.asarray(mu, np.float32).astype(np.float64).reshape(-1)
    e = np.asarray(eta, np.float32).astype(np.float64).reshape(-1)
    c = np.ones(mu.size) if multiplicity is None else np.asarray(multiplicity, np.float64).reshape(-1)
    keep = c > 0
    ll = (-0.5 * (LOG_2PI + e) - 0.5 * (float(y) - mu) ** 2 * np.exp(-e))[keep]
    mx = float(np.max(ll))
    return mx + math.log(float(np.sum(c[keep] * np.exp(ll - mx))) / float(np.sum(c)))


def energy_score(paths, y, multiplicity=None):
    """(1/S) sum c |Y_i - y| - (1 / (2 S^2)) sum_i sum_j c_i c_j |Y_i - Y_j| over the steps with finite y; NaN without any."""
    y = np.asarray(y, np.float32).astype(np.float64).reshape(-1)
    K = np.isfinite(y)
    if not np.any(K):
        return float("nan")
    Y = np.asarray(paths, np.float32).astype(np.float64)[:, K]
    c = np.ones(Y.shape[0]) if multiplicity is None else np.asarray(multiplicity, np.float64).reshape(-1)
    S = float(np.sum(c))
    first = float(np.sum(c * np.sqrt(np.sum((Y - y[K][None, :]) ** 2, axis=1)))) / S
    pair = 0.0
    for i0 in range(0, Y.shape[0], 512):                 # blocks of rows: [512, M, |K|] at a time
        d = np.sqrt(np.sum((Y[i0:i0 + 512, None, :] - Y[None, :, :]) ** 2, axis=2))
        pair += float(c[i0:i0 + 512] @ d @ c)
    return first - pair / (2.0 * S * S)


def scores(means, samples, eta, truth, multiplicity=None, levels=(), crps=True, energy=True):
    """Every output of ptnn_forecast_score from the device's own fp32 means / samples [U, n_origins, h], eta [U], multiplicities
    [U] and truth [n_origins, h] (NaN = none): dict(pit, pred_mean, pred_sd, crps, log_score [n_origins, h], quantiles
    [len(levels), n_origins, h], energy_score [n_origins]); NaN where there is no truth."""
    means, samples = np.asarray(means, np.float32), np.asarray(samples, np.float32)
    truth = np.asarray(truth, np.float32)
    R, h = truth.shape
    nan = lambda *s: np.full(s, np.nan)                  # noqa: E731
    out = dict(pit=nan(R, h), pred_mean=nan(R, h), pred_sd=nan(R, h), crps=nan(R, h), log_score=nan(R, h),
               quantiles=nan(len(levels), R, h), energy_score=nan(R))
    for r in range(R):
        for k in range(h):
            y = float(truth[r, k])
            if not math.isfinite(y):
                continue
            f = means[:, r, k]
            out["pit"][r, k] = cref.pit(y, f, eta, multiplicity)
            out["pred_mean"][r, k], out["pred_sd"][r, k] = cref.moments(f, eta, multiplicity)
            if crps:
                out["crps"][r, k] = cref.crps(y, f, eta, multiplicity)
            out["log_score"][r, k] = log_score(y, f, eta, multiplicity)
            for j, p in enumerate(levels):
                out["quantiles"][j, r, k] = cref.quantile(p, f, eta, multiplicity)
        if energy:
            out["energy_score"][r] = energy_score(samples[:, r, :], truth[r], multiplicity)
    return out
