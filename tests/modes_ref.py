"""A numpy restatement of posterior modes (ptnn_modes / posterior_modes), written from the definitions and
sharing no code with ptnn_amd/modes.py: the squared function-space distance in np.longdouble, the density-peaks stage on any given
matrix, and the host finishing from scratch -- labels, numbering, occupancy and hops from expanded per-row labels.  No device."""
import math

import numpy as np


def sq_longdouble(F):
    """F [U, n] -> sq [U, U] = sum_j (F[u, j] - F[v, j])^2 in np.longdouble."""
    F = np.asarray(F).astype(np.longdouble)
    out = np.zeros((F.shape[0], F.shape[0]), np.longdouble)
    for u in range(F.shape[0]):
        d = F - F[u]
        out[u] = (d * d).sum(axis=1)
    return out


def bound(n, ref):
    """|got - ref| <= 2 (n + 4) 2^-53 ref: every term is non-negative; one rounding in the widened difference, hence two relative
    to its square, and one per accumulation; (n + 2) u covers any order, and the factor leaves 2 x."""
    return 2.0 * (n + 4) * 2.0 ** -53 * np.asarray(ref, dtype=np.float64)


def density_peaks(sq, count, near_sq):
    """The density-peaks stage on a given matrix sq [U, U] with integer counts -> (rho [U] int64, delta_sq [U], parent [U] int64).
    Plain loops: v precedes u iff rho_v > rho_u, or rho_v = rho_u and v < u; absent samples (count 0) count nowhere."""
    sq, count = np.asarray(sq), [int(c) for c in count]
    U = len(count)
    rho = [0] * U
    for u in range(U):
        if count[u]:
            rho[u] = sum(count[v] for v in range(U) if count[v] and sq[u, v] <= near_sq)
    delta, parent = [0.0] * U, [-1] * U
    for u in range(U):
        if not count[u]:
            continue
        best = None
        for v in range(U):
            if count[v] and (rho[v] > rho[u] or (rho[v] == rho[u] and v < u)):
                if best is None or sq[u, v] < sq[u, best]:
                    best = v
        if best is None:
            delta[u] = max(sq[u, v] for v in range(U) if count[v])
        else:
            delta[u], parent[u] = sq[u, best], best
    return np.asarray(rho, np.int64), np.asarray(delta, np.float64), np.asarray(parent, np.int64)


def sq_float64(F):
    """The same matrix in float64, a row at a time: what a host would compute (the timing probe's comparison)."""
    F = np.asarray(F, dtype=np.float64)
    out = np.empty((F.shape[0], F.shape[0]))
    for u in range(F.shape[0]):
        d = F - F[u]
        out[u] = np.einsum("ij,ij->i", d, d)
    return out


def density_peaks_rows(sq, count, near_sq):
    """density_peaks with numpy over every row (the timing probe's comparison; tests/test_modes_cpu.py holds it to the loops)."""
    sq, count = np.asarray(sq, dtype=np.float64), np.asarray(count, dtype=np.int64)
    U = len(count)
    here = count > 0
    rho = np.where(here, ((sq <= near_sq) * count[None, :]).sum(axis=1), 0).astype(np.int64)
    delta, parent = np.zeros(U), np.full(U, -1, np.int64)
    idx = np.arange(U)
    for u in np.flatnonzero(here):
        before = here & ((rho > rho[u]) | ((rho == rho[u]) & (idx < u)))
        if before.any():
            cand = np.where(before, sq[u], np.inf)
            parent[u] = int(np.argmin(cand))                                # the first of equals: the lowest index
            delta[u] = cand[parent[u]]
        else:
            delta[u] = sq[u][here].max()
    return rho, delta, parent


def spread_sq(sq, count):
    """sum_u sum_v c_u c_v sq[u, v] / M^2 in np.longdouble."""
    c = np.asarray(count).astype(np.longdouble)
    return (c[:, None] * c[None, :] * np.asarray(sq).astype(np.longdouble)).sum() / (c.sum() * c.sum())


def labels_of(rho, delta_sq, parent, count, sep_sq_sum, min_count):
    """Centres, labels and numbering from the decision graph -> (sample_labels [U], centres [K], mass counts [K]).  Recursive on
    the parents instead of a walk in precedence order; numbering by a sort of (-mass, centre)."""
    U = len(rho)
    centre = [count[u] > 0 and (parent[u] < 0 or (delta_sq[u] > sep_sq_sum and rho[u] >= min_count)) for u in range(U)]

    def head(u):
        while not centre[u]:
            u = int(parent[u])
        return u
    heads = [head(u) if count[u] > 0 else -1 for u in range(U)]
    mass = {}
    for u, hd in enumerate(heads):
        if hd >= 0:
            mass[hd] = mass.get(hd, 0) + int(count[u])
    ranked = sorted(mass, key=lambda hd: (-mass[hd], hd))
    number = {hd: k for k, hd in enumerate(ranked)}
    return (np.asarray([number.get(hd, -1) for hd in heads], np.int64), np.asarray(ranked, np.int64),
            np.asarray([mass[hd] for hd in ranked], np.int64))


def chain_figures(labels, K):
    """Expanded labels [n_chains, m] -> (occupancy [n_chains, K], hops [n_chains], hop_matrix [K, K]), by plain loops."""
    C, m = np.shape(labels)
    occ, hops, hm = np.zeros((C, K)), np.zeros(C, np.int64), np.zeros((K, K), np.int64)
    for c in range(C):
        for t in range(m):
            occ[c, labels[c][t]] += 1
            if t and labels[c][t] != labels[c][t - 1]:
                hops[c] += 1
                hm[labels[c][t - 1], labels[c][t]] += 1
    return occ / m, hops, hm


def modes(F, count, separation, radius, min_mass):
    """The whole analysis on outputs F [U, n] with counts, sq in longdouble rounded to double -> dict."""
    F = np.asarray(F, dtype=np.float64)
    n = F.shape[1]
    sq = sq_longdouble(F).astype(np.float64)
    M = int(np.sum(count))
    rho, delta, parent = density_peaks(sq, count, radius * radius * n)
    lab, centres, mass = labels_of(rho, delta, parent, count, separation * separation * n, math.ceil(min_mass * M))
    return dict(sq=sq, rho=rho, delta_sq=delta, parent=parent, sample_labels=lab, centres=centres, mass=mass / M, n_modes=len(centres))
