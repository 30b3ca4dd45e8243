"""float64 numpy reference of the multistate Bennett acceptance ratio (Shirts & Chodera 2008): the fixed
point over weighted items, the weight matrix, the covariance Theta in its K x K and N x N forms, weighted moments and systematic
resampling.  States k have the reduced log density l_k(n) = g_k b_n + beta_k U_n (g_k = 0 for a prior state of beta = 0)."""
import numpy as np


def lse(a, axis, w=None):
    """log sum w exp(a) along `axis`, relative to the exact maximum over the entries with w > 0."""
    a = np.asarray(a, np.float64)
    if w is None:
        w = np.ones_like(a)
    w = np.broadcast_to(np.asarray(w, np.float64), a.shape)
    m = np.max(np.where(w > 0, a, -np.inf), axis=axis, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.sum(np.where(w > 0, w * np.exp(a - m), 0.0), axis=axis, keepdims=True)
    return np.squeeze(m + np.log(s), axis=axis)


def reduced(u, b, betas, g):
    """l [n, K]."""
    u, b = np.asarray(u, np.float64), np.asarray(b, np.float64)
    return np.asarray(g, np.float64)[None, :] * b[:, None] + np.asarray(betas, np.float64)[None, :] * u[:, None]


def solve(u, b, c, betas, g, n_k, tol=1e-10, max_iter=10000, batch=8):
    """The plain self-consistent iteration from f = 0, f_0 pinned to 0 after every sweep; sweeps run in batches of `batch` and
    stop when max |f - previous f| <= tol.  -> (f [K], D [n], n_iter, residual)."""
    l = reduced(u, b, betas, g)
    c = np.asarray(c, np.float64)
    ln_n = np.log(np.asarray(n_k, np.float64))
    f = np.zeros(l.shape[1])
    n_iter, resid = 0, np.inf
    while n_iter < max_iter and not resid <= tol:
        for _ in range(batch):
            D = lse(ln_n[None, :] + f[None, :] + l, axis=1)
            raw = -lse(l - D[:, None], axis=0, w=c[:, None])
            new = raw - raw[0]
            resid = float(np.max(np.abs(new - f)))
            f = new
        n_iter += batch
    D = lse(ln_n[None, :] + f[None, :] + l, axis=1)
    return f, D, n_iter, resid


def weight_matrix(u, b, betas, g, f, D):
    """W [n, K] = exp(f_k + l_k(n) - D_n)."""
    return np.exp(np.asarray(f)[None, :] + reduced(u, b, betas, g) - np.asarray(D)[:, None])


def gram(W, c):
    return W.T @ (np.asarray(c, np.float64)[:, None] * W)


def theta_kk(M, n_k):
    """Theta = M pinv(I - diag(N) M), the K x K form."""
    M = np.asarray(M, np.float64)
    return M @ np.linalg.pinv(np.eye(M.shape[0]) - np.diag(np.asarray(n_k, np.float64)) @ M, rcond=1e-12)


def theta_nn(W, n_k):
    """Theta = W^T (I - W N W^T)^+ W, the N x N form (unit item weights; small n only)."""
    W = np.asarray(W, np.float64)
    return W.T @ np.linalg.pinv(np.eye(W.shape[0]) - W @ np.diag(np.asarray(n_k, np.float64)) @ W.T, rcond=1e-12) @ W


def target_log_weights(u, b, c, D, beta):
    """log(c_n W_n) at `beta` (g = 1), its free energy formed like a state's; -inf where c_n = 0."""
    u, b, c, D = (np.asarray(a, np.float64) for a in (u, b, c, D))
    a = b + beta * u - D
    ft = -lse(a, axis=0, w=c)
    with np.errstate(divide="ignore"):
        return np.where(c > 0, np.log(c) + a + ft, -np.inf)


def weight_stats(lw, c):
    """(sum w, Kish ESS (sum w)^2 / sum (w^2 / c), largest share) of w = exp(lw) = c W."""
    w, c = np.exp(np.asarray(lw, np.float64)), np.asarray(c, np.float64)
    s = w.sum()
    return float(s), float(s * s / np.sum(w[c > 0] ** 2 / c[c > 0])), float(w.max() / s)


def weighted_moments(values, lw):
    """Weighted mean and population variance of values [n, ...] under w = exp(lw), two passes."""
    w = np.exp(np.asarray(lw, np.float64))
    w = w / w.sum()
    v = np.asarray(values, np.float64)
    mean = np.tensordot(w, v, axes=(0, 0))
    return mean, np.tensordot(w, (v - mean) ** 2, axes=(0, 0))


def systematic_resample(cum, u, m):
    """Draw i of m takes the first item whose running sum `cum` exceeds ((u + i) / m) cum[-1]; past the end: the last item of
    positive weight.  -> int64 [m]."""
    cum = np.asarray(cum, np.float64)
    t = (u + np.arange(m, dtype=np.float64)) / float(m) * cum[-1]
    idx = np.searchsorted(cum, t, side="right")
    last = int(np.flatnonzero(np.diff(np.concatenate([[0.0], cum])) > 0)[-1])
    return np.minimum(idx, last).astype(np.int64)


def gaussian_ladder(K, n, seed):
    """The analytic ladder: states beta_k = k / (K - 1), the first one the prior state (beta 0, l = 0); draws x ~ N(0, 1 / (1 +
    beta)), U = -x^2 / 2, b = 0; log Z = log(Z_1 / Z_0) = -log(2) / 2.  -> (u [K, n], betas [K], true log Z)."""
    rng = np.random.default_rng(seed)
    betas = np.linspace(0.0, 1.0, K)
    x = rng.standard_normal((K, n)) / np.sqrt(1.0 + betas)[:, None]
    return -0.5 * x * x, betas, -0.5 * np.log(2.0)
