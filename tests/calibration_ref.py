"""Float64 oracle of ptnn_calibration: PIT, predictive mean and sd, quantiles and the CRPS of the Gaussian
mixture (1/S) sum_s c_s N(f_s, tau_s^2) per data row, over the expanded multiset of samples, evaluated on the distinct ones.
Written from the definitions in numpy, with torch on the CPU for a vectorised float64 erf; tau_s^2 = exp(eta_s) with the fp32
eta widened to double, f the fp32 network outputs widened to double."""
import math
from statistics import NormalDist

import numpy as np
import torch

SQRT2 = math.sqrt(2.0)


def _erf(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def _erfc(x):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def Phi(x):
    """Standard normal cdf (through erfc: full relative accuracy in the lower tail)."""
    return 0.5 * _erfc(-np.asarray(x, np.float64) / SQRT2)


def A(m, v):
    """A(m, v) = m (2 Phi(m / sqrt v) - 1) + 2 sqrt(v) phi(m / sqrt v): E|X| of X ~ N(m, v) (Grimit et al. 2006)."""
    m, v = np.broadcast_arrays(np.asarray(m, np.float64), np.asarray(v, np.float64))
    mt, vt = torch.from_numpy(np.ascontiguousarray(m)), torch.from_numpy(np.ascontiguousarray(v))
    sd = torch.sqrt(vt)
    x = mt / sd
    return (mt * torch.special.erf(x / SQRT2) + 2.0 * sd * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)).numpy()


def _setup(f, eta, multiplicity):
    f = np.asarray(f, np.float32).astype(np.float64).reshape(-1)
    tau2 = np.exp(np.asarray(eta, np.float32).astype(np.float64).reshape(-1))
    c = np.ones(f.size) if multiplicity is None else np.asarray(multiplicity, np.float64).reshape(-1)
    return f, tau2, c, float(np.sum(c))


def mixture_cdf(z, f, eta, multiplicity=None):
    f, tau2, c, S = _setup(f, eta, multiplicity)
    return float(np.sum(c * Phi((z - f) / np.sqrt(tau2))) / S)


def pit(y, f, eta, multiplicity=None):
    return mixture_cdf(float(y), f, eta, multiplicity)


def moments(f, eta, multiplicity=None):
    """(pred_mean, pred_sd); the variance is centred on the mean."""
    f, tau2, c, S = _setup(f, eta, multiplicity)
    mean = float(np.sum(c * f) / S)
    return mean, math.sqrt(float(np.sum(c * (tau2 + (f - mean) ** 2)) / S))


def crps(y, f, eta, multiplicity=None):
    """(1/S) sum c A(y - f, tau^2) - (1 / (2 S^2)) sum_s sum_t c_s c_t A(f_s - f_t, tau_s^2 + tau_t^2), s = t included."""
    f, tau2, c, S = _setup(f, eta, multiplicity)
    first = float(np.sum(c * A(float(y) - f, tau2)) / S)
    pair = A(f[:, None] - f[None, :], tau2[:, None] + tau2[None, :])
    return first - float(c @ pair @ c) / (2.0 * S * S)


def crps_gaussian(y, mu, sigma):
    """The CRPS of one Gaussian (Gneiting & Raftery 2007, eq. 21)."""
    z = (y - mu) / sigma
    nd = NormalDist()
    return sigma * (z * (2.0 * nd.cdf(z) - 1.0) + 2.0 * nd.pdf(z) - 1.0 / math.sqrt(math.pi))


def quantile(p, f, eta, multiplicity=None):
    """A root of F(z) = p by bisection in double from [min (f + tau z_p), max (f + tau z_p)], until the midpoint is an end."""
    f, tau2, c, S = _setup(f, eta, multiplicity)
    tau = np.sqrt(tau2)
    zp = NormalDist().inv_cdf(float(p))
    keep = c > 0
    lo, hi = float(np.min((f + tau * zp)[keep])), float(np.max((f + tau * zp)[keep]))
    mid = lo
    for _ in range(1200):
        mid = 0.5 * lo + 0.5 * hi
        if not (lo < mid < hi):
            break
        if float(np.sum(c * Phi((mid - f) / tau)) / S) < p:
            lo = mid
        else:
            hi = mid
    return mid


def rows(fx, y, eta, multiplicity=None, crps_term=True):
    """Per data row from fx [U, n_rows]: dict(pit, pred_mean, pred_sd, crps) [n_rows]."""
    fx = np.asarray(fx, np.float32)
    n = fx.shape[1]
    out = dict(pit=np.empty(n), pred_mean=np.empty(n), pred_sd=np.empty(n), crps=np.full(n, np.nan))
    for r in range(n):
        out["pit"][r] = pit(y[r], fx[:, r], eta, multiplicity)
        out["pred_mean"][r], out["pred_sd"][r] = moments(fx[:, r], eta, multiplicity)
        if crps_term:
            out["crps"][r] = crps(y[r], fx[:, r], eta, multiplicity)
    return out


def crps_quadrature(y, f, eta, multiplicity=None, n=200001, width=12.0):
    """int (F(z) - 1{z >= y})^2 dz by composite Simpson on each side of y (the integrand jumps there), over every component's
    +- `width` sd; n points per side."""
    f, tau2, c, S = _setup(f, eta, multiplicity)
    tau = np.sqrt(tau2)
    lo, hi = min(float(np.min(f - width * tau)), y - 1.0), max(float(np.max(f + width * tau)), y + 1.0)

    def side(a, b, upper):
        z = np.linspace(a, b, n)
        F = np.zeros(n)
        for k in range(f.size):
            F += c[k] * Phi((z - f[k]) / tau[k])
        g = (F / S - (1.0 if upper else 0.0)) ** 2
        h = (b - a) / (n - 1)
        return h / 3.0 * (g[0] + g[-1] + 4.0 * np.sum(g[1:-1:2]) + 2.0 * np.sum(g[2:-1:2]))

    return side(lo, y, False) + side(y, hi, True)
