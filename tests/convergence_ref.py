"""Float64 numpy restatement of the convergence estimator of DESIGN.md section 12 (classic split-R-hat and split-ESS, BDA3
11.4-11.5, Geyer's initial monotone sequence), branch for branch, for the tests of ptnn_convergence / convergence_diagnostics."""
import math

import numpy as np


def split_chains(x):
    """x [C, n] -> [2C, h]: each chain's first and last h = n // 2 draws (an odd n drops the middle draw)."""
    x = np.asarray(x, dtype=np.float64)
    C, n = x.shape
    h = n // 2
    out = np.empty((2 * C, h))
    out[0::2] = x[:, :h]
    out[1::2] = x[:, n - h:]
    return out


def autocov(s):
    """Biased autocovariance of each row of s [M, h] about its own mean: gamma [M, h], gamma_t = (1/h) sum_{i < h - t} d_i d_{i+t}."""
    M, h = s.shape
    d = s - s.mean(axis=1, keepdims=True)
    if h <= 64:
        g = np.empty((M, h))
        for t in range(h):
            g[:, t] = np.einsum("ji,ji->j", d[:, :h - t], d[:, t:]) / h
        return g
    f = np.fft.rfft(d, n=2 * h, axis=1)                     # zero-padded: the circular products are the linear ones
    return np.fft.irfft(f * np.conj(f), n=2 * h, axis=1)[:, :h] / h


def moments(s):
    """-> (W, var_plus, gamma [M, h]) of split chains s [M, h]."""
    M, h = s.shape
    g = autocov(s)
    s2 = g[:, 0] * h / (h - 1)
    W = s2.mean()
    var_plus = W * (h - 1) / h + np.var(s.mean(axis=1), ddof=1)
    return W, var_plus, g


def rho_raw(s):
    """The combined rho_t, t = 0 .. h - 1, before the positivity and monotone edits (nan where var+ = 0)."""
    W, var_plus, g = moments(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - (W - g.mean(axis=0)) / var_plus


def ess_from_rho(r, M, h):
    """The pair loop, the initial monotone sequence and tau exactly as DESIGN.md section 12 writes them.
    -> (ess, max_t, deciding) where deciding is the pair sum even + odd that ended the pair loop."""
    rho = np.zeros(h + 2)
    rho[0] = 1.0
    even, odd = 1.0, r[1]
    rho[1] = odd
    t = 1
    while t < h - 3 and even + odd > 0:
        even, odd = r[t + 1], r[t + 2]
        if even + odd >= 0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t + 1])) + rho[max_t + 1]
    tau = max(tau, 1.0 / math.log10(M * h))
    return M * h / tau, max_t, even + odd


def diagnose(x):
    """One quantity, draws x [C, n] (n >= 4) -> dict(mean, var, r_hat, ess, trunc_lag, ess_chain [C], rho [h], deciding)."""
    x = np.asarray(x, dtype=np.float64)
    C, n = x.shape
    s = split_chains(x)
    M, h = s.shape
    W, var_plus, _ = moments(s)
    r = rho_raw(s)
    if var_plus == 0:
        r_hat, ess, max_t, dec = math.nan, math.nan, ess_from_rho(r, M, h)[1], math.nan
    else:
        r_hat = math.inf if W == 0 else math.sqrt(var_plus / W)
        ess, max_t, dec = ess_from_rho(r, M, h)
    ess_chain, dec_chain = np.empty(C), np.empty(C)
    for c in range(C):
        sc = s[2 * c:2 * c + 2]
        _, vp, _ = moments(sc)
        ess_chain[c], _, dec_chain[c] = (math.nan, 0, math.nan) if vp == 0 else ess_from_rho(rho_raw(sc), 2, h)
    return dict(mean=x.mean(), var=x.var(ddof=1), r_hat=r_hat, ess=ess, trunc_lag=max_t, ess_chain=ess_chain, rho=r, deciding=dec,
                deciding_chain=dec_chain)


def diagnose_all(draws):
    """draws [C, n, Q] -> dict of arrays over the Q quantities (ess_chain [C, Q], rho [h, Q])."""
    draws = np.asarray(draws)
    res = [diagnose(draws[:, :, q]) for q in range(draws.shape[2])]
    out = {k: np.array([r[k] for r in res]) for k in ("mean", "var", "r_hat", "ess", "trunc_lag", "deciding")}
    out["ess_chain"] = np.stack([r["ess_chain"] for r in res], axis=1)
    out["deciding_chain"] = np.stack([r["deciding_chain"] for r in res], axis=1)
    out["rho"] = np.stack([r["rho"] for r in res], axis=1)
    return out
