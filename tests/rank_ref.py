"""Float64 numpy restatement of the rank-normalised convergence diagnostics of DESIGN.md section 23 (Vehtari, Gelman, Simpson,
Carpenter & Buerkner 2021), branch for branch, for the tests of ptnn_rank_convergence / rank_diagnostics.  Average ranks come
from a stable sort plus run detection, the normal quantile is the standard library's NormalDist().inv_cdf (Wichura's AS241,
PPND16, as on the device), and split-R-hat / split-ESS are those of tests/convergence_ref.py."""
import math
from statistics import NormalDist

import numpy as np

import convergence_ref as cr

_INV_CDF = NormalDist().inv_cdf
TAIL_PROBS = (0.05, 0.95)


def keep(x):
    """x [C, n] -> [C, 2h]: each chain's first and last h = n // 2 draws (an odd n drops the middle draw)."""
    x = np.asarray(x)
    n = x.shape[1]
    h = n // 2
    return np.concatenate([x[:, :h], x[:, n - h:]], axis=1)


def average_ranks(v):
    """1-based ranks of the values v [S] (any float dtype), ties sharing the mean of the ranks they cover; -0 equals +0."""
    v = np.asarray(v).reshape(-1)
    S = v.size
    order = np.argsort(v, kind="stable")
    s = v[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))           # the first sorted position of every run of ties
    end = np.concatenate([start[1:], [S]])
    run = np.repeat(np.arange(start.size), end - start)
    r = np.empty(S)
    r[order] = (start[run] + 1 + end[run]) / 2.0                                  # mean of the ranks start + 1 .. end
    return r


def z_scores(r, S):
    """z = Phi^-1((r - 3/8) / (S + 1/4)) of ranks r among S draws."""
    p = (np.asarray(r, dtype=np.float64) - 0.375) / (S + 0.25)
    return np.array([_INV_CDF(float(v)) for v in p.reshape(-1)]).reshape(p.shape)


def folded(xk):
    """|x - med| in double of the pooled kept draws xk, med = (x_(S/2-1) + x_(S/2)) / 2 of their order statistics."""
    v = np.asarray(xk, dtype=np.float64)
    s = np.sort(v.reshape(-1), kind="stable")
    S = s.size
    med = (s[S // 2 - 1] + s[S // 2]) / 2.0
    return np.abs(v - med)


def indicator(xk, p):
    """I = [x <= x_(lo)], lo = floor((S - 1) p), of the pooled kept draws xk -> float64 0 / 1."""
    v = np.asarray(xk)
    s = np.sort(v.reshape(-1), kind="stable")
    lo = int(math.floor((s.size - 1) * p))
    return (v <= s[lo]).astype(np.float64)


def histogram(r, C, bins):
    """The rank histogram [C, bins] of average ranks r [C, 2h] among S = r.size draws: bin ((2r - 2) bins) // (2S), integers."""
    S = r.size
    r2 = np.rint(2.0 * np.asarray(r)).astype(np.int64)
    b = ((r2 - 2) * bins) // (2 * S)
    out = np.zeros((C, bins), np.int64)
    for c in range(C):
        out[c] = np.bincount(b[c], minlength=bins)
    return out


def _series(xk):
    """The bulk z-scores of kept draws xk [C, 2h], ranked over all of them -> (z [C, 2h], ranks [C, 2h])."""
    r = average_ranks(xk).reshape(xk.shape)
    return z_scores(r, xk.size), r


def _rhat_ess(series):
    """Split-R-hat, split-ESS and the deciding pair sum of a series [C, 2h]: the combined figures of cr.diagnose, from its parts
    (without the per-chain loop it also runs)."""
    s = cr.split_chains(series)
    M, h = s.shape
    W, var_plus, _ = cr.moments(s)
    if var_plus == 0:
        return math.nan, math.nan, math.nan
    ess, _, dec = cr.ess_from_rho(cr.rho_raw(s), M, h)
    return (math.inf if W == 0 else math.sqrt(var_plus / W)), ess, dec


def _ess(series):
    return _rhat_ess(series)[1:]


def trunc_lag(series):
    """The lag at which the pair loop of the split-ESS of a series [C, 2h] stopped (-1 where var+ = 0 and there is no ESS)."""
    s = cr.split_chains(series)
    if cr.moments(s)[1] == 0:
        return -1
    return cr.ess_from_rho(cr.rho_raw(s), *s.shape)[1]


def diagnose(x, probs=(), bins=20, per_chain=False):
    """One quantity, fp32 draws x [C, n] (n >= 4) -> dict(r_hat_bulk, r_hat_tail, r_hat, ess_bulk, ess_tail, ess_median,
    ess_quantile [len(probs)], rank_hist [C, bins], z [C, 2h], ranks [C, 2h], deciding: the pair sums that ended the pair loops of
    ess_bulk, the 0.05, 0.95 and 0.5 indicators and those of probs; with per_chain ess_bulk_chain, ess_tail_chain [C],
    deciding_chain [C, 3] and z_chain [C, 2h], each chain's z-scores among its own kept draws)."""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[0]
    xk = keep(x)
    nan = math.nan
    all_p = list(TAIL_PROBS) + [0.5] + [float(p) for p in probs]
    if not np.all(np.isfinite(x)):                                                # the one explicit rule
        out = dict(r_hat_bulk=nan, r_hat_tail=nan, r_hat=nan, ess_bulk=nan, ess_tail=nan, ess_median=nan,
                   ess_quantile=np.full(len(probs), nan), rank_hist=np.zeros((C, bins), np.int64), z=np.full(xk.shape, nan),
                   ranks=np.full(xk.shape, nan), deciding=np.full(1 + len(all_p), nan))
        if per_chain:
            out.update(ess_bulk_chain=np.full(C, nan), ess_tail_chain=np.full(C, nan), deciding_chain=np.full((C, 3), nan),
                       z_chain=np.full(xk.shape, nan))
        return out
    z, r = _series(xk)
    bulk = dict(zip(("r_hat", "ess", "deciding"), _rhat_ess(z)))
    zf, _ = _series(folded(xk))
    r_hat_tail = _rhat_ess(zf)[0]
    ess_p, dec_p = zip(*[_ess(indicator(xk, p)) for p in all_p])
    either = math.isnan(bulk["r_hat"]) or math.isnan(r_hat_tail)
    tail_nan = math.isnan(ess_p[0]) or math.isnan(ess_p[1])
    out = dict(r_hat_bulk=bulk["r_hat"], r_hat_tail=r_hat_tail, r_hat=nan if either else max(bulk["r_hat"], r_hat_tail),
               ess_bulk=bulk["ess"], ess_tail=nan if tail_nan else min(ess_p[0], ess_p[1]), ess_median=ess_p[2],
               ess_quantile=np.array(ess_p[3:], dtype=np.float64), rank_hist=histogram(r, C, bins), z=z, ranks=r,
               deciding=np.array([bulk["deciding"], *dec_p]))
    if per_chain:
        eb, et, dc, zc = np.empty(C), np.empty(C), np.empty((C, 3)), np.empty(xk.shape)
        for c in range(C):
            xc = xk[c:c + 1]
            zc[c] = _series(xc)[0][0]
            eb[c], dc[c, 0] = _ess(zc[c:c + 1])
            (lo, dc[c, 1]), (hi, dc[c, 2]) = _ess(indicator(xc, TAIL_PROBS[0])), _ess(indicator(xc, TAIL_PROBS[1]))
            et[c] = nan if math.isnan(lo) or math.isnan(hi) else min(lo, hi)
        out.update(ess_bulk_chain=eb, ess_tail_chain=et, deciding_chain=dc, z_chain=zc)
    return out


def diagnose_all(draws, probs=(), bins=20, per_chain=False):
    """draws [C, n, Q] -> dict of arrays over the Q quantities, quantity last: r_hat_bulk .. ess_median [Q], ess_quantile
    [len(probs), Q], rank_hist [C, bins, Q], z, ranks [C, 2h, Q], deciding [1 + 3 + len(probs), Q], ess_bulk_chain,
    ess_tail_chain [C, Q], deciding_chain [C, 3, Q], z_chain [C, 2h, Q]."""
    draws = np.asarray(draws)
    res = [diagnose(draws[:, :, q], probs, bins, per_chain) for q in range(draws.shape[2])]
    return {k: np.stack([np.asarray(r[k]) for r in res], axis=-1) for k in res[0]}
