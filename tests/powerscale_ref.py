"""Float64 oracle of ptnn_powerscale: the two components, the Pareto-smoothed power-scaled weights, the
cumulative Jensen-Shannon distance on the CDF and the survival side, the sensitivity and the moments, written from the
definitions of include/ptnn.h in plain numpy, one quantity at a time.  The smoothing is elpd_ref.psis on the expanded log ratios."""
import math

import numpy as np

import elpd_ref

COMPONENTS = ("likelihood", "prior")
QUADRATURE_D = 0.04463          # D of N(0, s^2) against N(0, s^2 / alpha) at delta = 0.01, by quadrature of the definition


def prior_component(task, w, eta, topo, sigma_squared=25.0, nu_1=0.0, nu_2=0.0):
    """pi [n] of the fp32 vectors w [n, P] (and eta [n], regression): prior_likelihood in float64."""
    I, H, O = topo
    w = np.asarray(w, np.float32).astype(np.float64)
    cnt = I * H + H + 2 if task == 0 else I * H + H + O + H * O
    pr = -1.0 * (cnt / 2.0) * math.log(sigma_squared) - np.sum(w * w, axis=1) / (2.0 * sigma_squared)
    if task == 0:
        e = np.asarray(eta, np.float32).astype(np.float64)
        pr = pr - (1.0 + nu_1) * e - nu_2 * np.exp(-e)
    return pr


def alphas(delta):
    return 1.0 / (1.0 + delta), 1.0 + delta


def smoothed_weights(comp, counts, alpha, r_eff=1.0):
    """q [U] (sum 1), khat, T: the Pareto smoothing of lr = (alpha - 1) comp over the expanded samples (vector u counts[u]
    times, consecutively, so a stable sort orders ties by distinct index), summed back per distinct vector."""
    counts = np.asarray(counts, np.int64)
    owner = np.repeat(np.arange(counts.size), counts)
    lr = (alpha - 1.0) * np.asarray(comp, np.float64)[owner]
    lw, khat, T = elpd_ref.psis(lr, r_eff)
    q = np.zeros(counts.size)
    np.add.at(q, owner, np.exp(lw - np.max(lw)))         # from the largest log weight, as the device forms them
    return q / np.sum(q), khat, T


def _h(a, m):
    out = np.zeros_like(a)
    k = a > 0
    out[k] = a[k] * (np.log2(a[k]) - np.log2(m[k]))
    return out


def _side(x, p, q):
    """d^2 of one side: x ascending, p and q the weights in that order."""
    b = np.diff(x)
    P, Q = np.cumsum(p)[:-1], np.cumsum(q)[:-1]
    m = 0.5 * (P + Q)
    return np.sum(b * (_h(P, m) + _h(Q, m))) / np.sum(b * (P + Q))


def distance(x, base, q):
    """d of one quantity: x [U] fp32 values, base and q [U] weights (each sum 1); vectors of base weight 0 take no part."""
    x = np.asarray(x, np.float32)
    live = np.asarray(base) > 0
    x, base, q = x[live], np.asarray(base, np.float64)[live], np.asarray(q, np.float64)[live]
    # ascending, -0 before +0, ties by distinct index: the order of the device's (key, index) words
    order = np.lexsort((np.arange(x.size), np.signbit(x) == 0, x))
    xs = x[order].astype(np.float64)
    if xs.size < 2 or xs[0] == xs[-1]:
        return 0.0
    d2 = max(_side(xs, base[order], q[order]), _side(-xs[::-1], base[order][::-1], q[order][::-1]))
    return math.sqrt(d2) if d2 > 0 else 0.0


def moments(x, wts):
    x = np.asarray(x, np.float32).astype(np.float64)
    m = np.sum(wts * x)
    return m, math.sqrt(np.sum(wts * (x - m) ** 2))


def powerscale(values, logp, counts, delta=0.01, r_eff=1.0):
    """values [Q, U] fp32 quantities, logp [2, U] (likelihood, prior), counts [U] -> dict with the device's outputs: sens [2, Q],
    dist, mean, sd [2, 2, Q], base_mean, base_sd [Q], khat, tail_len [2, 2], q [2, 2, U]."""
    values = np.asarray(values, np.float32)
    counts = np.asarray(counts, np.int64)
    Q, U = values.shape
    base = counts / counts.sum()
    out = dict(sens=np.empty((2, Q)), dist=np.empty((2, 2, Q)), mean=np.empty((2, 2, Q)), sd=np.empty((2, 2, Q)),
               base_mean=np.empty(Q), base_sd=np.empty(Q), khat=np.empty((2, 2)), tail_len=np.empty((2, 2), np.int64),
               q=np.empty((2, 2, U)))
    for c in range(2):
        for g, a in enumerate(alphas(delta)):
            out["q"][c, g], out["khat"][c, g], out["tail_len"][c, g] = smoothed_weights(logp[c], counts, a, r_eff)
    for j in range(Q):
        out["base_mean"][j], out["base_sd"][j] = moments(values[j], base)
        for c in range(2):
            for g in range(2):
                out["dist"][c, g, j] = distance(values[j], base, out["q"][c, g])
                out["mean"][c, g, j], out["sd"][c, g, j] = moments(values[j], out["q"][c, g])
    out["sens"] = (out["dist"][:, 0] + out["dist"][:, 1]) / (2.0 * math.log2(1.0 + delta))
    return out


def _cdf_side(x, P, Q):
    """d^2 of one side from the two CDFs on the ascending grid x (the definition's sum with P_j, Q_j given)."""
    b = np.diff(x)
    P, Q = P[:-1], Q[:-1]
    m = 0.5 * (P + Q)
    return np.sum(b * (_h(P, m) + _h(Q, m))) / np.sum(b * (P + Q))


def quadrature_sensitivity(lo, hi, sigma=5.0, delta=0.01, n=100001):
    """D of N(0, sigma^2) whose precision is scaled by alpha (the prior component of quadrature_case), by quadrature of the
    definition on n grid points over [lo, hi]: the normaliser sum b (P + Q) grows with the range while the divergence does not,
    so D is a function of the range and is taken over the range the sample covers."""
    g = np.linspace(lo, hi, n)
    phi = np.vectorize(lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0))))
    P = phi(g / sigma)
    d = 0.0
    for a in alphas(delta):
        Q = phi(g * math.sqrt(a) / sigma)
        d2 = max(_cdf_side(g, P, Q), _cdf_side(-g[::-1], 1.0 - P[::-1], 1.0 - Q[::-1]))
        d += math.sqrt(max(d2, 0.0))
    return d / (2.0 * math.log2(1.0 + delta))


def quadrature_case(seed, n_w, P, eta=-2.0):
    """n_w vectors from N(0, 25 I) in fp32 with one eta: the prior component scales every weight's precision by alpha."""
    w = np.random.default_rng(seed).normal(0.0, 5.0, (n_w, P)).astype(np.float32)
    return w, np.full(n_w, eta, np.float32)
