"""Float64 restatement of the log evidence (ptnn_evidence / log_evidence): U and b of weight vectors on the
training rows through the oracle's forward pass, the per-rung and prior reductions, the regression constant log c, and a naive
prior Monte Carlo estimate of log Z for small problems."""
import math

import numpy as np

from ptnn_oracle import TASK_CLS, forward


def log_c(task, n_rows):
    if task == TASK_CLS:
        return 0.0
    n = float(n_rows)
    return math.log(2.0) + math.lgamma(n / 2.0 + 1.0) - (n / 2.0) * math.log(math.pi)


def log_c_quadrature(n_rows, sse, beta=1.0):
    """log of the integral over eta of e^{-eta} L(tau^2 = e^eta)^beta for a Gaussian likelihood with residual sum of squares sse
    over n_rows rows, by the trapezoid rule on a fine eta grid, minus the closed-form w-dependent part b + beta U."""
    eta = np.linspace(-60.0, 60.0, 400001)
    ll = -0.5 * n_rows * (np.log(2 * math.pi) + eta) - 0.5 * sse * np.exp(-eta)
    f = -eta + beta * ll
    m = f.max()
    val = m + math.log(np.trapezoid(np.exp(f - m), eta))
    u = -0.5 * n_rows * math.log(sse)
    b = -math.log(sse)
    return val - b - beta * u


def u_and_b(task, rows, W, topo):
    """U [M] and b [M] of the weight vectors W [M, P] on rows [N, n_in + 1] (last column the target), float64 throughout."""
    I = topo[0]
    X, y = rows[:, :I].astype(np.float64), rows[:, I].astype(np.float64)
    W = np.atleast_2d(np.asarray(W, np.float64))
    U, B = np.empty(W.shape[0]), np.empty(W.shape[0])
    for j in range(W.shape[0]):
        out = forward(X, W[j], topo)[1]
        if task == TASK_CLS:
            e = np.exp(out)
            p = e / e.sum(axis=1, keepdims=True)
            U[j] = float(np.sum(np.log(p[np.arange(X.shape[0]), y.astype(np.int64)])))
            B[j] = 0.0
        else:
            sse = float(np.sum((y - out[:, 0]) ** 2))
            U[j] = -0.5 * X.shape[0] * math.log(sse)
            B[j] = -math.log(sse)
    return U, B


def u_and_b_batched(task, rows, W, topo):
    """u_and_b for many vectors at once (numpy broadcasting; the naive Monte Carlo reference)."""
    I, H, O = topo
    X, y = rows[:, :I].astype(np.float64), rows[:, I].astype(np.float64)
    W = np.asarray(W, np.float64)
    W1 = W[:, :I * H].reshape(-1, I, H)
    W2 = W[:, I * H:I * H + H * O].reshape(-1, H, O)
    B1 = W[:, I * H + H * O:I * H + H * O + H]
    B2 = W[:, I * H + H * O + H:]
    hid = 1.0 / (1.0 + np.exp(-(np.einsum("ni,mih->mnh", X, W1) - B1[:, None, :])))
    out = 1.0 / (1.0 + np.exp(-(np.einsum("mnh,mho->mno", hid, W2) - B2[:, None, :])))
    if task == TASK_CLS:
        lse = np.log(np.sum(np.exp(out), axis=2))
        U = np.sum(out[:, np.arange(X.shape[0]), y.astype(np.int64)] - lse, axis=1)
        return U, np.zeros_like(U)
    sse = np.sum((y[None, :] - out[:, :, 0]) ** 2, axis=1)
    return -0.5 * X.shape[0] * np.log(sse), -np.log(sse)


def rung_stats(u, d=0.0):
    u = np.asarray(u, np.float64)
    t = d * u
    m = t.max()
    e = np.exp(t - m)
    me = e.mean()
    return dict(mean=u.mean(), var=u.var(ddof=1), log_stone=m + math.log(me), relvar=e.var(ddof=1) / me ** 2)


def prior_stats(u, b, a):
    u, b = np.asarray(u, np.float64), np.asarray(b, np.float64)
    t = b + a * u
    m = t.max()
    w = np.exp(t - m)
    s0 = w.sum()
    mu = float(np.dot(w, u) / s0)
    return dict(log_mean_exp=m + math.log(s0 / u.size), kish=s0 * s0 / float(np.dot(w, w)), u_mean=mu,
                u_var=float(np.dot(w, (u - mu) ** 2) / s0))


def naive_log_z(task, rows, topo, n_draws, sigma, seed, chunk=1 << 16):
    """log c + log mean e^{b + U} over n_draws independent prior draws, with its standard error (delta method)."""
    rng = np.random.default_rng(seed)
    P = topo[0] * topo[1] + topo[1] * topo[2] + topo[1] + topo[2]
    ts = []
    for k in range(0, n_draws, chunk):
        W = rng.standard_normal((min(chunk, n_draws - k), P)) * sigma
        U, B = u_and_b_batched(task, rows, W, topo)
        ts.append(B + U)
    t = np.concatenate(ts)
    m = t.max()
    e = np.exp(t - m)
    me = e.mean()
    return log_c(task, rows.shape[0]) + m + math.log(me), math.sqrt(e.var(ddof=1) / me ** 2 / t.size)
