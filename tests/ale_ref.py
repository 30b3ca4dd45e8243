"""Accumulated local effects in float64 numpy (no GPU): the definitions of include/ptnn.h written twice over
-- for an arbitrary callable f(X) -> [n, O], and for a net through the oracle's forward pass on substituted rows --, the
first-order error bound of the device's fp32 local effects, and the reductions ptnn_accumulated_effects makes of them, every sum
in the stated ascending order so that the device's reduced outputs are reproduced bit for bit from its own local effects."""
import numpy as np

import pd_ref
from parity import orc

U32 = pd_ref.U32


# ---- bins
def last_bin(z):
    """K*: the first position of the last (largest) edge; the edges from there on are padding."""
    z = np.asarray(z)
    return int(np.argmax(z == z[-1]))


def bins(x, z):
    """x [n], edges z [E] (increasing, then constant) -> b [n] in 1 .. K*: the smallest k >= 1 with x <= z_k, K* when there is none."""
    z = np.asarray(z, np.float64)
    ks = last_bin(z)
    b = np.full(len(x), ks, np.int64)
    for n, v in enumerate(np.asarray(x, np.float64)):
        for k in range(1, ks + 1):
            if v <= z[k]:
                b[n] = k
                break
    return b


def counts(b, K):
    """b [n] in 1 .. K -> n_k [K]."""
    return np.bincount(np.asarray(b) - 1, minlength=K).astype(np.int64)


def cell_counts(bk, bm, K2):
    N = np.zeros((K2, K2), np.int64)
    for k, m in zip(bk, bm):
        N[k - 1, m - 1] += 1
    return N


# ---- the curve of one input: d [..., n, O] local effects (any leading axes), b [n] -> ALE [..., K + 1, O] float64
def bin_means(d, b, K):
    """m [..., K, O]: the sum of d over the rows of each bin in ascending row order, in double, divided by the count; 0 when empty."""
    d = np.asarray(d).astype(np.float64)
    s = np.zeros(d.shape[:-2] + (K, d.shape[-1]))
    for n in range(d.shape[-2]):
        s[..., b[n] - 1, :] += d[..., n, :]
    nk = counts(b, K)
    m = np.zeros_like(s)
    for k in range(K):
        if nk[k]:
            m[..., k, :] = s[..., k, :] / np.float64(nk[k])
    return m


def curve(d, b, K):
    """ALE [..., K + 1, O] float64: g_0 = 0, g_k = g_{k-1} + m_k, c = (sum_k n_k g_k) / N in ascending k, ALE = g - c."""
    m = bin_means(d, b, K)
    nk = counts(b, K)
    g = np.zeros(m.shape[:-2] + (K + 1, m.shape[-1]))
    c = np.zeros(m.shape[:-2] + (m.shape[-1],))
    for k in range(1, K + 1):
        g[..., k, :] = g[..., k - 1, :] + m[..., k - 1, :]
        c = c + np.float64(nk[k - 1]) * g[..., k, :]
    c = c / np.float64(len(b))
    return g - c[..., None, :]


def ranges(ale32):
    """ale32 [..., E, O] float32 -> [..., O] float32: max_k - min_k, the difference formed in double and rounded once."""
    p = np.asarray(ale32, np.float32).astype(np.float64)
    return (p.max(axis=-2) - p.min(axis=-2)).astype(np.float32)


# ---- the surface of one pair: D2 [..., n, O], (bk, bm) [n] -> ALE2 [..., K2 + 1, K2 + 1, O] float64
def surface(D2, bk, bm, K2):
    D2 = np.asarray(D2).astype(np.float64)
    lead, O = D2.shape[:-2], D2.shape[-1]
    N = cell_counts(bk, bm, K2)
    s = np.zeros(lead + (K2, K2, O))
    for n in range(D2.shape[-2]):
        s[..., bk[n] - 1, bm[n] - 1, :] += D2[..., n, :]
    h = np.zeros(lead + (K2 + 1, K2 + 1, O))
    for k in range(1, K2 + 1):
        run = np.zeros(lead + (O,))
        for m in range(1, K2 + 1):
            if N[k - 1, m - 1]:
                run = run + s[..., k - 1, m - 1, :] / np.float64(N[k - 1, m - 1])
            h[..., k, m, :] = h[..., k - 1, m, :] + run
    A = np.zeros(lead + (K2 + 1, O))
    B = np.zeros(lead + (K2 + 1, O))
    for k in range(1, K2 + 1):
        t = np.zeros(lead + (O,))
        for m in range(1, K2 + 1):
            t = t + np.float64(N[k - 1, m - 1]) * (h[..., k, m, :] - h[..., k - 1, m, :])
        nk = N[k - 1].sum()
        A[..., k, :] = A[..., k - 1, :] + (t / np.float64(nk) if nk else 0.0)
    for m in range(1, K2 + 1):
        t = np.zeros(lead + (O,))
        for k in range(1, K2 + 1):
            t = t + np.float64(N[k - 1, m - 1]) * (h[..., k, m, :] - h[..., k, m - 1, :])
        nm = N[:, m - 1].sum()
        B[..., m, :] = B[..., m - 1, :] + (t / np.float64(nm) if nm else 0.0)
    g2 = (h - A[..., :, None, :]) - B[..., None, :, :]
    c = np.zeros(lead + (O,))
    for k in range(1, K2 + 1):
        for m in range(1, K2 + 1):
            c = c + np.float64(N[k - 1, m - 1]) * g2[..., k, m, :]
    c = c / np.float64(len(bk))
    return g2 - c[..., None, None, :]


def interaction(ale2_32, bk, bm, K2):
    """ale2_32 [..., K2 + 1, K2 + 1, O] float32 -> [..., O] float32: sqrt((sum_{k, m >= 1} N(k, m) ALE2_32^2) / N), k-major."""
    a = np.asarray(ale2_32, np.float32).astype(np.float64)
    N = cell_counts(bk, bm, K2)
    s = np.zeros(a.shape[:-3] + (a.shape[-1],))
    for k in range(1, K2 + 1):
        for m in range(1, K2 + 1):
            s = s + np.float64(N[k - 1, m - 1]) * (a[..., k, m, :] * a[..., k, m, :])
    return np.sqrt(s / np.float64(len(bk))).astype(np.float32)


# ---- local effects of an arbitrary callable f(X) -> [n, O]
def _sub(X, cols, vals):
    Xs = np.array(X, dtype=np.float64)
    for j, v in zip(cols, vals):
        Xs[:, j] = v
    return Xs


def local1_f(f, X, j, z):
    """(d [n, O], b [n]): f on the rows with x_j at the upper edge of the row's bin minus f with x_j at the lower edge."""
    z = np.asarray(z, np.float64)
    b = bins(np.asarray(X)[:, j], z)
    return np.asarray(f(_sub(X, [j], [z[b]])), np.float64) - np.asarray(f(_sub(X, [j], [z[b - 1]])), np.float64), b


def local2_f(f, X, j, l, u, v):
    """(D2 [n, O], bk, bm): the second difference of f over the row's cell, in the order of include/ptnn.h."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    bk, bm = bins(np.asarray(X)[:, j], u), bins(np.asarray(X)[:, l], v)
    F = lambda a, c: np.asarray(f(_sub(X, [j, l], [a, c])), np.float64)      # noqa: E731
    return (F(u[bk], v[bm]) - F(u[bk - 1], v[bm])) - (F(u[bk], v[bm - 1]) - F(u[bk - 1], v[bm - 1])), bk, bm


def ale_f(f, X, j, z):
    """(ALE [K + 1, O], n_k [K]) of input j of the callable."""
    K = len(z) - 1
    d, b = local1_f(f, X, j, z)
    return curve(d, b, K), counts(b, K)


def ale2_f(f, X, j, l, u, v):
    """(ALE2 [K2 + 1, K2 + 1, O], N [K2, K2]) of the pair (j, l) of the callable."""
    K2 = len(u) - 1
    D2, bk, bm = local2_f(f, X, j, l, u, v)
    return surface(D2, bk, bm, K2), cell_counts(bk, bm, K2)


# ---- a net: the oracle's forward pass on the substituted rows
def net(w, topo, task):
    """f(X) -> [n, O] of the weight vector w: the output ptnn_predict returns (a classification's p = softmax(s))."""
    w = np.asarray(w, np.float64)

    def f(X):
        out = orc.forward(np.asarray(X, np.float64), w, topo)[1]
        return pd_ref._softmax(out) if task == orc.TASK_CLS else out
    return f


def local1(X, w, topo, task, j, z):
    return local1_f(net(w, topo, task), X, j, z)


def local2(X, w, topo, task, j, l, u, v):
    return local2_f(net(w, topo, task), X, j, l, u, v)


# ---- the error bounds of the device's fp32 local effects: |dev - ref| <= K u T to first order
def bound1(X, w, topo, task, j, z):
    """T1 [n, O] = pd_ref.error_bound at the upper edge + at the lower edge + |d_ref| (the one rounding of the difference)."""
    z = np.asarray(z, np.float64)
    d, b = local1(X, w, topo, task, j, z)
    return pd_ref.error_bound(X, w, topo, task, j, z[b]) + pd_ref.error_bound(X, w, topo, task, j, z[b - 1]) + np.abs(d)


def error_bound2(X, w, topo, task, j, vj, l, vl):
    """pd_ref.error_bound generalised to two substitutions, the device's zb_h = z_h + (vl - x_l) W1[l,h], then zb_h + (vj - x_j)
    W1[j,h]: Z_h gains (|x_l| + |vl - x_l|) |W1[l,h]| and the count I + 3 one more operation."""
    I, H, O = topo
    W1, W2, B1, B2 = orc.decode(np.asarray(w, np.float64), topo)
    X = np.asarray(X, np.float64)
    Xs = _sub(X, [j, l], [vj, vl])
    hid = orc.sigmoid(Xs @ W1 - B1)
    d = hid * (1.0 - hid)
    s = orc.sigmoid(hid @ W2 - B2)
    ds = s * (1.0 - s)
    Z = (np.abs(X) @ np.abs(W1) + np.abs(B1) + (np.abs(X[:, j]) + np.abs(vj - X[:, j]))[:, None] * np.abs(W1[j])[None, :]
         + (np.abs(X[:, l]) + np.abs(vl - X[:, l]))[:, None] * np.abs(W1[l])[None, :])
    A = hid @ np.abs(W2) + np.abs(B2)
    T = ds * ((d * ((I + 4) * Z + 4)) @ np.abs(W2) + (H + 2) * A) + 4 * s
    if task != orc.TASK_CLS:
        return T
    p = pd_ref._softmax(s)
    return p * (T + np.sum(p * T, axis=1, keepdims=True)) + (O + 8) * p


def bound2(X, w, topo, task, j, l, u, v):
    """T2 [n, O] = error_bound2 at the four corners of the row's cell + |D2_ref|."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    D2, bk, bm = local2(X, w, topo, task, j, l, u, v)
    T = np.abs(D2)
    for a in (u[bk], u[bk - 1]):
        for c in (v[bm], v[bm - 1]):
            T = T + error_bound2(X, w, topo, task, j, a, l, c)
    return T


# ---- the device's arithmetic in numpy float32 (the delta form, every fused multiply-add as fl32(a b + c) from float64)
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sig32(z):
    e = np.exp(-np.abs(z)).astype(np.float32)
    return (np.where(z >= 0, np.float32(1), e) / (np.float32(1) + e)).astype(np.float32)


def emulate(X32, w32, topo, task, j, vj, l=None, vl=None):
    """f [n, O] float32 as ale_forward_kernel forms it: z_h over the row as it is, zb = fma(vl - x_l, W1[l], z) (dl = 0 without
    l), fma(vj - x_j, W1[j], zb), the input with the larger index first; the hidden sums in ascending h."""
    I, H, O = topo
    if l is not None and l < j:
        j, vj, l, vl = l, vl, j, vj
    X32 = np.asarray(X32, np.float32)
    W1, W2, B1, B2 = (np.asarray(a, np.float32) for a in orc.decode(np.asarray(w32, np.float32), topo))
    n = X32.shape[0]
    acc = np.zeros((n, O), np.float32)
    dj = (np.asarray(vj, np.float32) - X32[:, j]).astype(np.float32)
    dl = np.zeros(n, np.float32) if l is None else (np.asarray(vl, np.float32) - X32[:, l]).astype(np.float32)
    for h in range(H):
        z = np.zeros(n, np.float32)
        for i in range(I):
            z = _fma(X32[:, i], np.full(n, W1[i, h], np.float32), z)
        z = (z - B1[h]).astype(np.float32)
        zb = _fma(dl, np.full(n, W1[0 if l is None else l, h], np.float32), z)
        hid = _sig32(_fma(dj, np.full(n, W1[j, h], np.float32), zb))
        for o in range(O):
            acc[:, o] = _fma(hid, np.full(n, W2[h, o], np.float32), acc[:, o])
    f = _sig32((acc - B2[None, :]).astype(np.float32))
    if task == orc.TASK_CLS:
        e = np.exp(f).astype(np.float32)
        s = np.zeros(n, np.float32)
        for o in range(O):
            s = (s + e[:, o]).astype(np.float32)
        f = (e / s[:, None]).astype(np.float32)
    return f
