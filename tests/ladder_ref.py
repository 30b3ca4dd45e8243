"""Float64 restatement of the ladder adaptation (ptnn_dev_ladder.hpp) and an independent count of the
per-pair swap acceptances and round trips of a swap log (ladder_stats_from_log's reference)."""
import numpy as np


def kappa(t, kappa0, t0):
    return kappa0 * t0 / (t + t0)


def initial_log_gaps(T):
    T = np.asarray(T, np.float32).astype(np.float64)
    return np.log(np.diff(T))


def update(s, a, t, kappa0, t0, tmax):
    """One adapted round: log-gaps s [R-1] and acceptances a [R-1] -> (new s, new float64 ladder [R]) with T_0 = 1 and
    T_R-1 = tmax exactly."""
    s = np.asarray(s, np.float64)
    a = np.asarray(a, np.float64)
    s_new = s + kappa(t, kappa0, t0) * (a - a.mean())
    g = np.exp(s_new)
    scale = (float(tmax) - 1.0) / g.sum()
    T = np.empty(s.size + 1)
    T[0] = 1.0
    T[1:] = 1.0 + scale * np.cumsum(g)
    T[-1] = float(tmax)
    return s_new, T


def replay(T0, accept_rows, A, kappa0, t0):
    """The ladder history [A+1, R] (float32) the device should write, fed its own recorded a_k(t) rows."""
    T0 = np.asarray(T0, np.float32)
    s = initial_log_gaps(T0)
    out = [T0.copy()]
    for t in range(A):
        s, T = update(s, accept_rows[t], t, kappa0, t0, T0[-1])
        out.append(T.astype(np.float32))
    return np.stack(out)


def pair_accept(T, L_raw):
    """a_k of every adjacent pair, float64: min(1, exp(min((1/T_k - 1/T_k+1)(L_k+1 - L_k), 80))), NaN -> 1."""
    T = np.asarray(T, np.float64)
    L = np.asarray(L_raw, np.float64)
    d = (1.0 / T[:-1] - 1.0 / T[1:]) * (L[1:] - L[:-1])
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.minimum(1.0, np.exp(np.minimum(d, 80.0)))
    return np.where(np.isnan(d), 1.0, a)


def stats_from_log(log, rule, first_round, n_moves=None):
    """Walk the log round by round with plain Python lists: per-pair accepted / proposed counts and completed 0 -> R-1 -> 0
    round trips of every walker."""
    log = [list(map(int, row)) for row in log]
    n = len(log) if n_moves is None else min(n_moves, len(log))
    R = len(log[0])
    acc, prop = [0] * (R - 1), [0] * (R - 1)
    where = list(range(R))                   # where[w] = index of walker w
    seek = [None] * R                        # None: not seen at 0 yet, "up", "down"
    trips = [0] * R
    for r in range(n):
        src = log[r]
        if r == first_round:
            for w in range(R):
                if where[w] == 0:
                    seek[w] = "up"
        if r >= first_round:
            for k in range(R - 1):
                if rule == 0 or k % 2 == r % 2:
                    prop[k] += 1
                    acc[k] += src[k] == k + 1
        where = [src.index(j) for j in where]
        if r >= first_round:
            for w in range(R):
                if where[w] == R - 1 and seek[w] == "up":
                    seek[w] = "down"
                elif where[w] == 0:
                    if seek[w] == "down":
                        trips[w] += 1
                    seek[w] = "up"
    return acc, prop, trips
