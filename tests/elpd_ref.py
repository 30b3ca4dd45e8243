"""Float64 oracle of ptnn_elpd: lppd, p_waic, PSIS-LOO elpd and the Pareto k-hat per data row, over the
expanded multiset of samples.  Written from the definitions (Vehtari, Gelman & Gabry 2017; Zhang & Stephens 2009 with the weakly
informative prior of Vehtari et al. 2024) in plain numpy, one row at a time."""
import math

import numpy as np

DBL_EPS = np.finfo(np.float64).eps
LOG_DBL_MIN = math.log(np.finfo(np.float64).tiny)


def pointwise_loglik(task, f, y, eta=None):
    """ll [S, n_rows] from the fp32 network outputs f: regression f [S, n_rows] (one output) with eta [S]; classification the
    softmax probabilities f [S, n_rows, O] and integer labels y [n_rows]."""
    if task == 0:
        tau2 = np.exp(np.asarray(eta, np.float32).astype(np.float64))[:, None]
        d = np.asarray(y, np.float64)[None, :] - np.asarray(f, np.float32).astype(np.float64)
        return -0.5 * np.log(2.0 * math.pi * tau2) - 0.5 * d * d / tau2
    p = np.asarray(f, np.float32)
    yi = np.asarray(y).astype(np.int64)
    return np.log(p[:, np.arange(p.shape[1]), yi].astype(np.float64))


def _logsumexp(a):
    m = np.max(a)
    return m + math.log(np.sum(np.exp(a - m)))


def gpdfit(x):
    """(k, sigma) of a generalized Pareto fit to the ascending sample x (Zhang & Stephens 2009, prior of Vehtari et al.)."""
    n = x.size
    m = 30 + int(math.floor(math.sqrt(n)))
    b = 1.0 - np.sqrt(m / (np.arange(m) + 0.5))
    b = b / (3.0 * x[int(math.floor(n / 4.0 + 0.5)) - 1]) + 1.0 / x[n - 1]
    k = np.array([np.mean(np.log1p(-bi * x)) for bi in b])
    L = n * (np.log(-b / k) - k - 1.0)
    wt = np.array([1.0 / np.sum(np.exp(L - Li)) for Li in L])
    keep = ~(wt < 10.0 * DBL_EPS)
    wt = wt[keep] / np.sum(wt[keep])
    b_post = np.sum(b[keep] * wt)
    k_post = np.mean(np.log1p(-b_post * x))
    sigma = -k_post / b_post
    khat = (n * k_post + 10.0 * 0.5) / (n + 10.0)
    return khat, sigma


def gpinv(p, k, sigma):
    if not sigma > 0:
        return np.full_like(p, np.nan)
    if abs(k) < DBL_EPS:
        return -sigma * np.log1p(-p)
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def psis(lr, r_eff=1.0):
    """Pareto-smoothed log weights of the log ratios lr [S] -> (lw normalised, khat, T)."""
    S = lr.size
    lw = lr - np.max(lr)
    M = int(math.ceil(min(0.2 * S, 3.0 * math.sqrt(S / r_eff))))
    srt = np.sort(lw)
    cut = max(srt[S - M - 1], LOG_DBL_MIN) if S - M - 1 >= 0 else LOG_DBL_MIN
    tail = np.flatnonzero(lw > cut)
    T = tail.size
    khat = math.inf
    if T > 4:
        order = tail[np.argsort(lw[tail], kind="stable")]
        x = np.exp(lw[order]) - math.exp(cut)
        khat, sigma = gpdfit(x)
        if np.isfinite(khat):
            sm = np.log(gpinv((np.arange(T) + 0.5) / T, khat, sigma) + math.exp(cut))
            lw = lw.copy()
            lw[order] = sm
            lw = np.minimum(lw, 0.0)
    return lw - _logsumexp(lw), khat, T


def elpd_rows(ll, multiplicity=None, r_eff=1.0):
    """Per data row of ll [n_samples, n_rows] (sample s counted multiplicity[s] times): dict(lppd, p_waic, elpd_loo, khat, tail_len)."""
    ll = np.asarray(ll, np.float64)
    if multiplicity is not None:
        ll = np.repeat(ll, np.asarray(multiplicity, np.int64), axis=0)
    S, N = ll.shape
    out = {k: np.empty(N) for k in ("lppd", "p_waic", "elpd_loo", "khat")}
    out["tail_len"] = np.empty(N, np.int64)
    for n in range(N):
        col = ll[:, n]
        out["lppd"][n] = _logsumexp(col) - math.log(S)
        mean = np.sum(col) / S
        out["p_waic"][n] = np.sum((col - mean) ** 2) / (S - 1)
        lw, khat, T = psis(-col, r_eff)
        out["elpd_loo"][n] = _logsumexp(lw + col)
        out["khat"][n] = khat
        out["tail_len"][n] = T
    return out


def totals(r):
    """Totals and standard errors of elpd_rows' output (host arithmetic of predictive_accuracy)."""
    N = r["lppd"].size
    se = lambda x: math.sqrt(N * np.var(x, ddof=1))  # noqa: E731
    waic_i = r["lppd"] - r["p_waic"]
    return dict(elpd_loo=np.sum(r["elpd_loo"]), se_elpd_loo=se(r["elpd_loo"]), p_loo=np.sum(r["lppd"]) - np.sum(r["elpd_loo"]),
                elpd_waic=np.sum(waic_i), se_elpd_waic=se(waic_i), p_waic=np.sum(r["p_waic"]), lppd=np.sum(r["lppd"]),
                se_lppd=se(r["lppd"]))
