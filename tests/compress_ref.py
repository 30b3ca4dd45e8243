"""Posterior compression restated in numpy (include/ptnn.h: ptnn_compress), in the device's own orders, one
rounding per operation: the strided-256 partials (thread t adds the terms t, t + 256, ... in ascending order), the LDS tree of
wg_sum (pairs i, i + N / 2; ...; 0, 1), the rows in ascending order.  With dtype=np.float64 a result is the device's bit for bit;
with dtype=np.longdouble the same walk is the reference the bounds are taken against."""
import itertools

import numpy as np

THREADS = 256


def wg_sum(parts):
    """The LDS tree of ptnn_dev_wg.hpp over len(parts) = a power of two values."""
    a = np.array(parts)
    d = len(a) // 2
    while d > 0:
        a[:d] = a[:d] + a[d:2 * d]
        d //= 2
    return a[0]


def strided_sum(terms, dtype=np.float64, threads=THREADS):
    """Thread t adds terms[t], terms[t + threads], ... in ascending order; the partials go down the tree."""
    terms = np.asarray(terms, dtype=dtype).reshape(-1)
    pad = (-len(terms)) % threads
    rows = np.concatenate([terms, np.zeros(pad, dtype)]).reshape(-1, threads)      # + 0.0 changes no bit of a non-negative sum
    part = np.zeros(threads, dtype)
    for row in rows:
        part = part + row
    return wg_sum(part)


def distances(sq, dtype=np.float64):
    return np.sqrt(np.asarray(sq, dtype=np.float64).astype(dtype))


def mean_distances(sq, count, dtype=np.float64):
    """-> (mu [U], D0): mu of an absent sample is 0."""
    count = np.asarray(count, dtype=np.int64)
    d = distances(sq, dtype)
    U, M = len(count), dtype(int(count.sum()))
    c = count.astype(dtype)
    mu = np.zeros(U, dtype)
    for u in range(U):
        if count[u] > 0:
            mu[u] = strided_sum(np.where(count > 0, c * np.where(count > 0, d[u], 0), 0), dtype) / M
    s = dtype(0)
    for u in range(U):
        s = s + c[u] * mu[u]
    return mu, s / M


def energy_of(musum, pair, n, d0, dtype=np.float64):
    n = dtype(n)
    return ((dtype(2) * musum) / n - pair / (n * n)) - d0


def key_of(score):
    """The order-preserving bit map of a signed float64 (the device compares these words, then the index)."""
    b = np.asarray(score, dtype=np.float64).view(np.int64)
    return np.where(b < 0, ~b, b | np.int64(-2 ** 63)).view(np.uint64)


def herd(sq, count, m, dtype=np.float64, follow=None):
    """The herding walk -> dict(picks, energy, pick_score, mu, d0, gap): m picks without replacement among the present samples,
    the lowest index on a tie.  follow: picks to take instead of the walk's own (the device's), with gap[j] = the score of the
    followed pick less the smallest score of step j."""
    count = np.asarray(count, dtype=np.int64)
    d = distances(sq, dtype)
    mu, d0 = mean_distances(sq, count, dtype)
    live = count > 0
    r = np.zeros(len(count), dtype)
    musum = pair = dtype(0)
    picks, energy, scores, gaps = [], [], [], []
    for j in range(m):
        score = mu - r / dtype(j + 1)
        cand = np.flatnonzero(live)
        if dtype is np.float64:
            best = int(cand[np.argmin(key_of(score[cand]))])
        else:
            best = int(cand[np.argmin(score[cand])])
        x = best if follow is None else int(follow[j])
        assert live[x]
        gaps.append(score[x] - score[best])
        musum = musum + mu[x]
        pair = pair + dtype(2) * r[x]
        picks.append(x)
        scores.append(score[x])
        energy.append(energy_of(musum, pair, j + 1, d0, dtype))
        live[x] = False
        r = r + d[x]
    return dict(picks=np.asarray(picks, dtype=np.int64), energy=np.asarray(energy, dtype=dtype), pick_score=np.asarray(scores, dtype=dtype),
                mu=mu, d0=d0, gap=np.asarray(gaps, dtype=dtype))


def subset_energy(sq, count, samples, dtype=np.float64, mu=None, d0=None):
    """The energy of the measure (1 / k) sum delta(samples[i]) against the full weighted sample, in the device's order: the ordered
    pairs p -> (p // k, p % k), ascending."""
    if mu is None:
        mu, d0 = mean_distances(sq, count, dtype)
    s = np.asarray(samples, dtype=np.int64)
    d = distances(sq, dtype)
    k = len(s)
    return energy_of(strided_sum(mu[s], dtype), strided_sum(d[np.ix_(s, s)].reshape(-1), dtype), k, d0, dtype)


def energy_plain(points, count, subset):
    """The energy distance by its definition, float64, no particular order: points [U, n], the measure of the subset (sample
    indices, equal weights) against the count-weighted full sample.  2 E d(X, Y) - E d(Y, Y') - E d(X, X')."""
    P = np.asarray(points, dtype=np.float64)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2))
    w = np.asarray(count, dtype=np.float64)
    w = w / w.sum()
    q = np.bincount(np.asarray(subset, dtype=np.int64), minlength=len(w)) / float(len(subset))
    return float(2 * q @ d @ w - q @ d @ q - w @ d @ w)


def mean_energy_of_draws(points, count, k):
    """The mean energy of k draws WITH replacement from the count-weighted sample, by enumeration of the U^k ordered tuples."""
    w = np.asarray(count, dtype=np.float64)
    w = w / w.sum()
    total = 0.0
    for tup in itertools.product(range(len(w)), repeat=k):
        p = float(np.prod(w[list(tup)]))
        if p > 0:
            total += p * energy_plain(points, count, tup)
    return total


def sq_of(points):
    P = np.asarray(points, dtype=np.float64)
    return ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
