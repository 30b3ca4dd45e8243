"""Partial dependence and ICE curves in float64 numpy (no GPU): the outputs of the oracle's forward pass on rows with one input
substituted, the first-order error bound of the device's fp32 evaluation, and the reductions
ptnn_partial_dependence makes of its ICE values."""
import numpy as np

from parity import orc

U32 = 2.0 ** -24                          # unit round-off of fp32


def _softmax(s):
    e = np.exp(s)
    return e / e.sum(axis=1, keepdims=True)


def ice(X, w, topo, task, j, v):
    """f [n_rows, O] of vector w on the rows X with column j set to v: the oracle's forward pass on the substituted rows; a
    classification's p = softmax(s)."""
    Xs = np.array(X, dtype=np.float64)
    Xs[:, j] = v
    out = orc.forward(Xs, np.asarray(w, np.float64), topo)[1]
    return _softmax(out) if task == orc.TASK_CLS else out


def ice_all(X, w, topo, task, inputs, grid):
    """[n_rows, A, G, O]: ice() for every selected input and grid value, in the device's column order."""
    return np.stack([np.stack([ice(X, w, topo, task, int(j), float(v)) for v in grid[a]], axis=1) for a, j in enumerate(inputs)], axis=1)


def error_bound(X, w, topo, task, j, v):
    """T [n_rows, O]: |f_fp32 - f| <= K u T to first order, for the device's delta form z_h + (v - x_j) W1[j,h].  With the
    float64 intermediates at the substituted row, Z_h = sum_i |x_i W1[i,h]| + |B1[h]| + (|x_j| + |v - x_j|) |W1[j,h]| (the I FMAs
    and the bias over the row as it is, the difference and its FMA) and A_o = sum_h hid_h |W2[h,o]| + |B2[o]|:
        T_o = ds_o (sum_h |W2[h,o]| d_h ((I + 3) Z_h + 4) + (H + 2) A_o) + 4 s_o
    (the slope of hid in z is d_h; 4 for the exp, the sum 1 + e and the division; the length-H sum and the bias; the output
    sigmoid).  Classification: T_c' = p_c (T_c + sum_o p_o T_o) + (O + 8) p_c for the softmax's exps, sum and division."""
    I, H, O = topo
    W1, W2, B1, B2 = orc.decode(np.asarray(w, np.float64), topo)
    X = np.asarray(X, np.float64)
    Xs = X.copy()
    Xs[:, j] = v
    hid = orc.sigmoid(Xs @ W1 - B1)
    d = hid * (1.0 - hid)
    s = orc.sigmoid(hid @ W2 - B2)
    ds = s * (1.0 - s)
    Z = np.abs(X) @ np.abs(W1) + np.abs(B1) + (np.abs(X[:, j]) + np.abs(v - X[:, j]))[:, None] * np.abs(W1[j])[None, :]
    A = hid @ np.abs(W2) + np.abs(B2)
    T = ds * ((d * ((I + 3) * Z + 4)) @ np.abs(W2) + (H + 2) * A) + 4 * s
    if task != orc.TASK_CLS:
        return T
    p = _softmax(s)
    return p * (T + np.sum(p * T, axis=1, keepdims=True)) + (O + 8) * p


def error_bound_all(X, w, topo, task, inputs, grid):
    return np.stack([np.stack([error_bound(X, w, topo, task, int(j), float(v)) for v in grid[a]], axis=1) for a, j in enumerate(inputs)],
                    axis=1)


def row_means(ice32):
    """ice32 [M, n_rows, A, G, O] float32 -> PD [M, A, G, O] float64: the means over the rows, summed in ascending row order in
    double, as pd_rows_kernel sums them."""
    f = np.asarray(ice32, np.float32).astype(np.float64)
    s = np.zeros((f.shape[0],) + f.shape[2:])
    for n in range(f.shape[1]):
        s += f[:, n]
    return s / np.float64(f.shape[1])


def ranges(pd32):
    """pd32 [M, A, G, O] float32 -> range_s [M, A, O] float32: max_k - min_k, the difference formed in double and rounded once."""
    p = np.asarray(pd32, np.float32).astype(np.float64)
    return (p.max(axis=2) - p.min(axis=2)).astype(np.float32)
