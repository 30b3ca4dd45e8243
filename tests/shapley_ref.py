"""Coalition values and Shapley attributions in float64 numpy (no GPU): the oracle's forward pass on hybrid rows (DESIGN.md section
29), Shapley values by the subset formula and by walking orders, the coalition tables shapley_table must build, and the error bound
of the device's evaluation.

The bound of one output out[n, o, t] = sum_c coef[c, t] v[n, S_c, o], v = (1/B) sum_b f_o(w; h(x_n, b, S_c)):

    |out_dev - out_ref| <= K u sum_c |coef[c, t]| (1/B) sum_b T_o(h(x_n, b, S_c)) + u |out_ref| + C 2^-52 sum_c |coef[c, t]| |v_c| + 1e-30

with u = 2^-24 and K = 1.  First term: the device evaluates f in fp32 on the hybrid row h, whose entries are exact fp32 values (a
select), by I FMAs per hidden unit in ascending input order and the bias, z_h, with |dz_h| <= (I + 1) u Z_h to first order, Z_h =
sum_i |h_i W1[i,h]| + |B1[h]|; the sigmoid (exp, 1 + e, the division: 4 u, slope d_h); H FMAs in ascending hidden order and the
bias, |da_o| <= sum_h |W2[h,o]| |dhid_h| + (H + 2) u A_o; the output sigmoid (slope ds_o, 4 u s_o); a classification's softmax.
That is pd_ref.error_bound's T_o with its delta form's two extra operations unused -- it charges (I + 3) Z_h with Z_h enlarged by
(|x_j| + |v - x_j|) |W1[j,h]| -- evaluated at the hybrid row with no substitution (v = x_j, taken at j = 0), so it covers this
kernel with room.  The mean over b and the sum over c are linear, so the forward errors add with the weights |coef| / B.  Second
term: the one fp32 store.  Third term: the double arithmetic -- per coalition the sum over b (six butterfly levels, at most three
further chunk additions, one division: at most 10 roundings of 2^-53 |v_c|, the summands being positive) and then C fmas, each
rounding a partial sum that is at most sum_c |coef| |v_c|: together under (C + 10) 2^-53 <= C 2^-52 times that sum for C >= 10,
and for the smaller identity tables of the tests (C = 5, one non-zero coefficient per term, every fma exact) the 10 roundings of
the sum over b are C 2^-52.  Both are some 2^-26 of the second term."""
import itertools
import math

import numpy as np

import pd_ref
from parity import orc

U32 = 2.0 ** -24                          # unit round-off of fp32
U64 = 2.0 ** -52


def _softmax(s):
    e = np.exp(s)
    return e / e.sum(axis=1, keepdims=True)


def hybrid(X, bg, mask):
    """[n_rows, B, I]: input i from the explained row where bit i of mask is set, else from the background row."""
    X, bg = np.asarray(X, np.float64), np.asarray(bg, np.float64)
    take = np.array([(int(mask) >> i) & 1 for i in range(X.shape[1])], bool)
    return np.where(take[None, None, :], X[:, None, :], bg[None, :, :])


def _f(rows, w, topo, task):
    out = orc.forward(rows, np.asarray(w, np.float64), topo)[1]
    return _softmax(out) if task == orc.TASK_CLS else out


def coalition_values(X, bg, w, topo, task, masks):
    """v [n_rows, C, O]: the mean over the background rows, summed in ascending order, of f on the hybrid rows."""
    n, B, O = np.shape(X)[0], np.shape(bg)[0], topo[2]
    v = np.zeros((n, len(masks), O))
    for c, m in enumerate(masks):
        f = _f(hybrid(X, bg, m).reshape(n * B, -1), w, topo, task).reshape(n, B, O)
        s = np.zeros((n, O))
        for b in range(B):
            s += f[:, b]
        v[:, c] = s / np.float64(B)
    return v


def functionals(v, coef):
    """out [n_rows, O, T] = sum_c coef[c, t] v[n, c, o], the coalitions added in table order."""
    out = np.zeros((v.shape[0], v.shape[2], coef.shape[1]))
    for c in range(coef.shape[0]):
        out += v[:, c, :, None] * coef[c][None, None, :]
    return out


def shapley_exact(X, bg, w, topo, task):
    """phi [n_rows, O, I] by the subset formula: sum over S without j of |S|! (I - |S| - 1)! / I! (v(S + j) - v(S))."""
    I = topo[0]
    v = coalition_values(X, bg, w, topo, task, list(range(1 << I)))
    phi = np.zeros((v.shape[0], topo[2], I))
    for j in range(I):
        for S in range(1 << I):
            if not (S >> j) & 1:
                k = bin(S).count("1")
                phi[:, :, j] += math.factorial(k) * math.factorial(I - k - 1) / math.factorial(I) * (v[:, S | (1 << j)] - v[:, S])
    return phi


def shapley_permutation(X, bg, w, topo, task, orders):
    """phi [n_rows, O, I]: the mean over the orders of the marginal contribution of each input as it joins its predecessors."""
    I = topo[0]
    orders = np.asarray(orders)
    phi = np.zeros((np.shape(X)[0], topo[2], I))
    cache = {}

    def v(mask):
        if mask not in cache:
            cache[mask] = coalition_values(X, bg, w, topo, task, [mask])[:, 0]
        return cache[mask]
    for order in orders:
        mask = 0
        for j in (int(t) for t in order):
            phi[:, :, j] += (v(mask | (1 << j)) - v(mask)) / orders.shape[0]
            mask |= 1 << j
    return phi


def shapley_brute_force(X, bg, w, topo, task):
    """All I! orders."""
    return shapley_permutation(X, bg, w, topo, task, list(itertools.permutations(range(topo[0]))))


def table_exact(I):
    """What shapley_table(I, 'exact') must return: masks 0 .. 2^I - 1, the Shapley weights, v(empty) and v(all) in terms I, I + 1."""
    coef = np.zeros((1 << I, I + 2))
    for S in range(1 << I):
        k = bin(S).count("1")
        for j in range(I):
            if (S >> j) & 1:          # S = S' + j with |S'| = k - 1
                coef[S, j] += math.factorial(k - 1) * math.factorial(I - k) / math.factorial(I)
            else:
                coef[S, j] -= math.factorial(k) * math.factorial(I - k - 1) / math.factorial(I)
    coef[0, I] = 1.0
    coef[(1 << I) - 1, I + 1] = 1.0
    return np.arange(1 << I, dtype=np.uint64), coef


def table_permutation(I, orders):
    """What shapley_table(I, permutations=orders) must return: the prefixes of every order merged by mask, first appearance first."""
    orders = np.asarray(orders)
    n = orders.shape[0]
    table = {0: np.zeros(I + 2)}
    for order in orders:
        prefix = [0]
        for j in order:
            prefix.append(prefix[-1] | (1 << int(j)))
        for k, j in enumerate(order):
            table.setdefault(prefix[k], np.zeros(I + 2))[int(j)] -= 1.0 / n
            table.setdefault(prefix[k + 1], np.zeros(I + 2))[int(j)] += 1.0 / n
    table[0][I] = 1.0
    table[(1 << I) - 1][I + 1] = 1.0
    return np.array(list(table), np.uint64), np.stack(list(table.values()))


def error_bound(X, bg, w, topo, task, masks, coef, K=1.0):
    """-> (bound, out_ref), each [n_rows, O, T]: the module docstring's bound of the device's out around the float64 out_ref."""
    n, B, O = np.shape(X)[0], np.shape(bg)[0], topo[2]
    coef = np.asarray(coef, np.float64)
    C = coef.shape[0]
    v = coalition_values(X, bg, w, topo, task, masks)
    out = functionals(v, coef)
    fwd = np.zeros_like(out)
    acc = np.zeros_like(out)
    for c, m in enumerate(masks):
        h = hybrid(X, bg, m).reshape(n * B, -1)
        T = pd_ref.error_bound(h, w, topo, task, 0, h[:, 0]).reshape(n, B, O).mean(axis=1)        # (1/B) sum_b T_o
        fwd += T[:, :, None] * np.abs(coef[c])[None, None, :]
        acc += np.abs(v[:, c])[:, :, None] * np.abs(coef[c])[None, None, :]
    return K * U32 * fwd + U32 * np.abs(out) + C * U64 * acc + 1e-30, out
