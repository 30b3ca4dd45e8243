"""Input sensitivity in float64 numpy (no GPU): the gradient of the network outputs with respect to the inputs (DESIGN.md section
19), the first-order error bound of its fp32 evaluation, and the reductions ptnn_sensitivity makes of it."""
import numpy as np

from parity import orc

U32 = 2.0 ** -24                          # unit round-off of fp32


def _sigmoid_slope(z):
    """sigmoid(z) and sigmoid'(z) without the cancellation 1 - sigmoid(z)."""
    e = np.exp(-np.abs(z))
    q = 1.0 + e
    return np.where(z >= 0, 1.0, e) / q, e / (q * q)


def _parts(X, w, topo):
    W1, W2, B1, B2 = orc.decode(np.asarray(w, np.float64), topo)
    X = np.asarray(X, np.float64)
    z = X @ W1 - B1
    hid, d = _sigmoid_slope(z)
    a = hid @ W2 - B2
    s, ds = _sigmoid_slope(a)
    return X, W1, W2, B1, B2, hid, d, s, ds


def _softmax(s):
    e = np.exp(s)
    return e / e.sum(axis=1, keepdims=True)


def jacobian(X, w, topo, task):
    """g [n_rows, O, I]: J[o,i] = ds_o sum_h W2[h,o] d_h W1[i,h]; classification: the gradient of p = softmax(s),
    g[c,i] = p_c (J[c,i] - sum_o p_o J[o,i])."""
    _, W1, W2, _, _, _, d, s, ds = _parts(X, w, topo)
    J = ds[:, :, None] * np.einsum("nh,ho,ih->noi", d, W2, W1)
    if task != orc.TASK_CLS:
        return J
    p = _softmax(s)
    return p[:, :, None] * (J - np.einsum("no,noi->ni", p, J)[:, None, :])


def error_bound(X, w, topo, task):
    """T [n_rows, O, I]: |g_fp32 - g| <= K u T to first order.  Each term ds_o |W2[h,o]| d_h |W1[i,h]| of |J| carries the relative
    error (I + 2) Z_h + (H + 2) + 8 from z_h (Z_h = sum_i |x_i W1[i,h]| + |B1[h]|: the slope of d in z is at most d itself), the
    length-H sum and the exp, divisions and products; likewise (H + 2) A_o + 8 from a_o (A_o = sum_h hid_h |W2[h,o]| + |B2[o]|).
    Classification: those through g's linear form, plus (O + 8) p_c (|J|[c,i] + sum_o p_o |J|[o,i]) for the softmax and the sum."""
    I, H, O = topo
    X, W1, W2, B1, B2, hid, d, s, ds = _parts(X, w, topo)
    Z = np.abs(X) @ np.abs(W1) + np.abs(B1)
    A = hid @ np.abs(W2) + np.abs(B2)
    aJ = ds[:, :, None] * np.einsum("nh,ho,ih->noi", d, np.abs(W2), np.abs(W1))
    T = ds[:, :, None] * np.einsum("nh,ho,ih->noi", d * ((I + 2) * Z + (H + 2) + 8), np.abs(W2), np.abs(W1))
    T = T + aJ * ((H + 2) * A + 8)[:, :, None]
    if task != orc.TASK_CLS:
        return T
    p = _softmax(s)
    mix = lambda V: p[:, :, None] * (V + np.einsum("no,noi->ni", p, V)[:, None, :])   # noqa: E731
    return mix(T) + (O + 8) * mix(aJ)


def row_means(g32):
    """g32 [M, n_rows, O, I] float32 -> (a, q) [M, O, I] float64: the means over the rows of |g| and g^2, summed in ascending
    row order in double, as sensitivity_rows_kernel sums them."""
    g = np.asarray(g32, np.float32).astype(np.float64)
    sa = np.zeros((g.shape[0],) + g.shape[2:])
    sq = np.zeros_like(sa)
    for n in range(g.shape[1]):
        sa += np.abs(g[:, n])
        sq += g[:, n] * g[:, n]
    return sa / np.float64(g.shape[1]), sq / np.float64(g.shape[1])
