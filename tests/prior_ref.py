"""Float64 numpy restatement of the reductions of the prior predictive check (ptnn_prior_predictive, include/ptnn.h): the
statistics of every drawn function over the rows, their summaries over the draws and the counts against the data's.  The inputs
are the device's own fp32 outputs `samples` [n_draws, n_rows, n_out] and the targets; nothing here runs a network, except
outputs(), the oracle's forward pass of drawn vectors, which the CPU test uses to look at a seed without a device."""
import numpy as np

REG_STATS = ("mean", "sd", "min", "max", "acf1", "rmse", "saturated")
CLS_FIXED = ("accuracy", "log_score", "confidence", "saturated")


def _mean_in_row_order(x):
    """The mean over the last axis, added up in row order (np.cumsum adds sequentially) as one lane of the device does: the
    centred sums below then start from the same mean, bit for bit."""
    return np.cumsum(x, axis=-1)[..., -1] / x.shape[-1]


def series(x):
    """mean, sd (population), min, max, acf1 (centred lag-1 autocorrelation) over the last axis of x (float64) -> [..., 5];
    acf1 of a constant series is 0 / 0 = nan."""
    x = np.asarray(x, dtype=np.float64)
    m = _mean_in_row_order(x)
    d = x - m[..., None]
    c0 = np.sum(d * d, axis=-1)
    c1 = np.sum(d[..., 1:] * d[..., :-1], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        acf1 = c1 / c0
    return np.stack([m, np.sqrt(c0 / x.shape[-1]), x.min(axis=-1), x.max(axis=-1), acf1], axis=-1)


def regression(samples, y, eps):
    """samples [n_draws, n_rows, 1] fp32, y [n_rows] or None -> (t_draw [n_draws, 7], t_obs [7])."""
    f = np.asarray(samples)[:, :, 0].astype(np.float64)
    n, N = f.shape
    t = np.full((n, len(REG_STATS)), np.nan)
    t[:, :5] = series(f)
    t[:, 6] = np.sum((f < eps) | (f > 1.0 - eps), axis=1) / N
    t_obs = np.full(len(REG_STATS), np.nan)
    if y is not None:
        y = np.asarray(y, dtype=np.float64)
        t[:, 5] = np.sqrt(np.sum((y[None, :] - f) ** 2, axis=1) / N)
        t_obs[:5] = series(y)
    return t, t_obs


def classification(samples, y, eps):
    """samples [n_draws, n_rows, O] fp32 class probabilities, y [n_rows] integer labels or None -> (t_draw [n_draws, 4 + O],
    t_obs [4 + O]).  argmax: the first index on a tie."""
    p = np.asarray(samples)
    n, N, O = p.shape
    arg = np.argmax(p, axis=2)
    best = p.max(axis=2).astype(np.float64)
    t = np.full((n, len(CLS_FIXED) + O), np.nan)
    t[:, 2] = np.sum(best, axis=1) / N
    t[:, 3] = np.sum(best > 1.0 - eps, axis=1) / N
    for k in range(O):
        t[:, 4 + k] = np.sum(arg == k, axis=1) / N
    t_obs = np.full(len(CLS_FIXED) + O, np.nan)
    if y is not None:
        y = np.asarray(y).astype(np.int64)
        t[:, 0] = np.sum(arg == y[None, :], axis=1) / N
        py = np.take_along_axis(p, np.broadcast_to(y[None, :, None], (n, N, 1)), axis=2)[:, :, 0].astype(np.float64)
        with np.errstate(divide="ignore"):
            t[:, 1] = np.sum(-np.log(py), axis=1) / N
        t_obs[4:] = np.bincount(y, minlength=O) / N
    return t, t_obs


def summarise(t_draw, t_obs):
    """Per statistic over the draws, nan draws left out: dict(mean, sd (population), n_greater, n_equal, n_defined, p_value);
    p = (n_greater + n_equal / 2) / n_defined, nan where nothing is defined or the data has no counterpart."""
    t = np.asarray(t_draw, dtype=np.float64)
    ok = ~np.isnan(t)
    nd = ok.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ok, t, 0.0).sum(axis=0) / nd
        sd = np.sqrt(np.where(ok, (t - mean[None, :]) ** 2, 0.0).sum(axis=0) / nd)
        ng = (ok & (t > t_obs[None, :])).sum(axis=0)
        ne = (ok & (t == t_obs[None, :])).sum(axis=0)
        p = np.where((nd > 0) & ~np.isnan(t_obs), (ng + 0.5 * ne) / nd, np.nan)
    return dict(mean=mean, sd=sd, n_greater=ng.astype(np.int64), n_equal=ne.astype(np.int64), n_defined=nd.astype(np.int64), p_value=p)


def close_draws(t_draw, t_obs, rtol, atol):
    """[n_draws, n_stats] bool: the draws whose T(f_i) lies within the tolerance of T(y): a comparison of the two that rounding
    may turn."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(t_draw) - t_obs[None, :]) <= atol + rtol * np.abs(t_obs[None, :])


def outputs(orc, task, X, W, topo):
    """The oracle's outputs of the vectors W [n, P] on rows X, rounded to fp32 as the device returns them: [n, n_rows, O]; a
    classification's: the softmax."""
    out = np.stack([orc.forward(X, w.astype(np.float64), topo)[1] for w in W])
    if task == orc.TASK_CLS:
        e = np.exp(out)
        out = e / e.sum(axis=2, keepdims=True)
    return out.astype(np.float32)
