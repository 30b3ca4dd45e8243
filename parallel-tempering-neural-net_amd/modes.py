"""Posterior modes of the drop-in (not in the reference, which never asks whether its tempered chains found more than one mode):
function-space clusters of the sampled nets and the chains' hops between them.  The host-only helpers, the result tuple, and the
mixin that holds the public method.  The method checks its arguments here, makes one low-level call of `_lib.Sampler` (the device
forms the all-pairs squared distance of the distinct samples' outputs and the density-peaks stage on it) and finishes the result
with host arithmetic in float64 and integers.
"""
import math
from collections import namedtuple

import numpy as np

# posterior_modes' result: U distinct samples, M selected samples, K modes, n = n_rows * n_out output columns.  n_modes = K;
# sample_labels [U] int64, the mode of every distinct sample (-1: absent, count 0); labels, the mode of every selected item
# ([n_chains, m] for the trace, [n] for weights= and values=); centres [K] int64, distinct-sample indices; centre_rows [K, 2] int64
# (chain, selected-row index) of the centre's first item (-1 where there is no chain or no row); mass [K], shares of M; mode_mean,
# mode_sd [K, n_rows, n_out] ([K, n_a] for values=), count-weighted over the members' outputs, ddof 0; between [K, K], the distance
# d of the centres; within [K], the count-weighted RMS d of the members to their centre; occupancy [n_chains, K], the share of each
# chain's selected rows per mode, hops [n_chains] int64, the label changes between consecutive selected rows, hop_matrix [K, K]
# int64, those transitions pooled, from-mode by to-mode (all three None without chains); rho [U] int64, delta [U] (a distance),
# parent [U] int64: the decision graph; spread = sqrt(spread_sq / n); n_samples; n_distinct; distances [U, U] on request (d).
PosteriorModes = namedtuple("PosteriorModes", "n_modes sample_labels labels centres centre_rows mass mode_mean mode_sd between within "
                                              "occupancy hops hop_matrix rho delta parent spread n_samples n_distinct distances")


def precedence_order(rho, count):
    """The present samples (count > 0) in precedence order: descending rho, lower index first on a tie -> int64 indices."""
    rho, count = np.asarray(rho, dtype=np.int64), np.asarray(count, dtype=np.int64)
    present = np.nonzero(count > 0)[0]
    return present[np.argsort(-rho[present], kind="stable")].astype(np.int64)


def mode_labels(rho, delta_sq, parent, count, sep_sq_sum, min_count):
    """Centres and labels of the density-peaks decision graph.  u is a centre iff parent_u = -1, or (delta_sq_u > sep_sq_sum and
    rho_u >= min_count).  Walking the samples in precedence order, a centre opens a mode and every other sample takes its parent's;
    modes are numbered by descending mass (the members' counts), lower centre index first on a tie; absent samples get -1.
    -> (sample_labels [U] int64, centres [K] int64, mode counts [K] int64)."""
    rho, parent, count = (np.asarray(a, dtype=np.int64) for a in (rho, parent, count))
    delta_sq = np.asarray(delta_sq, dtype=np.float64)
    raw = np.full(rho.shape[0], -1, np.int64)
    opened = []
    for u in precedence_order(rho, count):
        if parent[u] < 0 or (delta_sq[u] > sep_sq_sum and rho[u] >= min_count):
            raw[u] = len(opened)
            opened.append(int(u))
        else:
            raw[u] = raw[parent[u]]
    opened = np.asarray(opened, dtype=np.int64)
    counts = np.asarray([int(count[raw == k].sum()) for k in range(len(opened))], dtype=np.int64)
    order = np.lexsort((opened, -counts))
    number = np.empty(len(opened), np.int64)
    number[order] = np.arange(len(opened))
    labels = np.where(raw >= 0, number[np.maximum(raw, 0)], -1) if len(opened) else raw
    return labels.astype(np.int64), opened[order], counts[order]


def chain_hops(labels, n_modes):
    """labels [n_chains, m] of the selected rows -> (occupancy [n_chains, K], hops [n_chains] int64, hop_matrix [K, K] int64)."""
    labels = np.asarray(labels, dtype=np.int64)
    C, m = labels.shape
    occ = np.stack([np.bincount(row, minlength=n_modes)[:n_modes] for row in labels]).astype(np.float64) / max(m, 1)
    a, b = labels[:, :-1], labels[:, 1:]
    change = a != b
    hm = np.zeros((n_modes, n_modes), np.int64)
    np.add.at(hm, (a[change], b[change]), 1)
    return occ, change.sum(axis=1).astype(np.int64), hm


def finish_modes(out, shape, n, sep_sq_sum, min_mass, n_chains=None, with_rows=True):
    """The host arithmetic of posterior_modes: the device's decision graph, item map and outputs [U, n] -> PosteriorModes with the
    output axes `shape`.  n_chains: the trace's chains (the items are chain-major), None for weights= and values=."""
    rho, count = np.asarray(out["rho"], dtype=np.int64), np.asarray(out["count"], dtype=np.int64)
    parent, item = np.asarray(out["parent"], dtype=np.int64), np.asarray(out["item_sample"], dtype=np.int64)
    delta_sq = np.asarray(out["delta_sq"], dtype=np.float64)
    M, U = int(out["n_samples"]), int(out["n_distinct"])
    sample_labels, centres, counts = mode_labels(rho, delta_sq, parent, count, sep_sq_sum, math.ceil(min_mass * M))
    K = len(centres)
    F = np.asarray(out["outputs"], dtype=np.float64).reshape(U, n)
    w = count.astype(np.float64)
    mean, sd, within = np.zeros((K, n)), np.zeros((K, n)), np.zeros(K)
    for k in range(K):
        mem = sample_labels == k
        wk = w[mem] / w[mem].sum()
        mean[k] = wk @ F[mem]
        sd[k] = np.sqrt(wk @ (F[mem] - mean[k]) ** 2)
        within[k] = math.sqrt(float(wk @ ((F[mem] - F[centres[k]]) ** 2).sum(axis=1)) / n)
    Fc = F[centres]
    between = np.sqrt(((Fc[:, None, :] - Fc[None, :, :]) ** 2).sum(axis=2) / n)
    labels = sample_labels[item]
    first = np.full(U, -1, np.int64)
    first[item[::-1]] = np.arange(len(item))[::-1]
    rows = np.full((K, 2), -1, np.int64)
    occupancy = hops = hop_matrix = None
    if n_chains is not None:
        m = len(item) // n_chains
        labels = labels.reshape(n_chains, m)
        rows = np.stack([first[centres] // m, first[centres] % m], axis=1)
        occupancy, hops, hop_matrix = chain_hops(labels, K)
    elif with_rows:
        rows[:, 1] = first[centres]
    dist = None if out.get("sq_dist") is None else np.sqrt(np.asarray(out["sq_dist"], dtype=np.float64) / n)
    return PosteriorModes(n_modes=K, sample_labels=sample_labels, labels=labels, centres=centres, centre_rows=rows, mass=counts / float(M),
                          mode_mean=mean.reshape((K,) + tuple(shape)), mode_sd=sd.reshape((K,) + tuple(shape)), between=between,
                          within=within, occupancy=occupancy, hops=hops, hop_matrix=hop_matrix, rho=rho, delta=np.sqrt(delta_sq / n),
                          parent=parent, spread=math.sqrt(out["spread_sq"] / n), n_samples=M, n_distinct=U, distances=dist)


def modes_stuck(result, min_mass=0.1):
    """The (chain, mode) pairs of a PosteriorModes where a mode of at least `min_mass` of the samples was never visited by the
    chain: -> int64 [n, 2], row-major.  A result without chains (weights= or values=) has none to report and is refused."""
    if not 0 <= min_mass <= 1:
        raise ValueError(f"min_mass = {min_mass!r} must lie in [0, 1]")
    if result.occupancy is None:
        raise ValueError("this result has no chains (weights= or values=): nothing to report")
    big = np.asarray(result.mass) >= min_mass
    return np.argwhere((np.asarray(result.occupancy) == 0) & big[None, :]).astype(np.int64)


class ModesAnalysis:
    """posterior_modes(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row and sample-source helpers it
    uses.  It reads the constructor's attributes `topology`, `num_chains` and `_sampler`."""

    def posterior_modes(self, x="train", *, separation=0.05, radius=None, min_mass=0.02, burn_in=None, chains="all", thin=1,
                        weights=None, values=None, return_distances=False):
        """Did the chains find more than one mode, which rungs sit in which, and how often does a chain cross?  Computed on the GPU
        from the sampled chains.

        Sampled nets are compared by what they compute, not by where their weights lie: a one-hidden-layer net has H! x (sign)
        equivalent labelings of its hidden units, so R-hat on the weights is blind to this.  The distance of two sampled nets is
        d = the RMS difference of their outputs on the rows `x` ("train", "test" or rows of n_in columns), in output units (both
        tasks put out values in [0, 1]).  The modes are those of density-peaks clustering (Rodriguez & Laio 2014) on d: rho counts
        the samples within `radius` (None = separation / 2) of a sample; a sample heads a mode iff no denser sample lies within
        `separation` of it and its rho is at least ceil(min_mass x n_samples); every other sample joins the mode of its nearest
        denser sample.  The defaults are conventions in output units (separation = 5 % of the output range), not tuned values; a
        cloud wider than the separation merges planted groups into one mode rather than splitting into spurious ones.

        Samples, `chains`, `thin` and `weights` as posterior_predictive().  chains="cold" is the posterior's own figure; the default
        chains="all" pools the tempered rungs, and `occupancy` then says which rungs sit in which mode.  `values` [n, n_a] (or a
        pair with integer multiplicities [n]) takes the place of the samples and the forward pass: every row is a sample's output
        vector.  With weights= or values= there are no chains: occupancy, hops and hop_matrix are None.
        -> PosteriorModes."""
        self._need_sampler("posterior_modes")
        sep = float(separation)
        if not (math.isfinite(sep) and sep > 0):
            raise ValueError(f"separation = {separation!r} must be a finite number > 0")
        rad = sep / 2 if radius is None else float(radius)
        if not (math.isfinite(rad) and rad >= 0):
            raise ValueError(f"radius = {radius!r} must be a finite number >= 0")
        if not 0 <= min_mass <= 1:
            raise ValueError(f"min_mass = {min_mass!r} must lie in [0, 1]")
        if values is not None:
            if weights is not None:
                raise ValueError("values= takes the place of the samples: no weights= with it")
            mult = None
            if isinstance(values, tuple):
                values, mult = values
            va = np.asarray(values, dtype=np.float32)
            if va.ndim != 2 or va.shape[0] < 1 or va.shape[1] < 1:
                raise ValueError(f"values must be [n_samples, n_a], got shape {va.shape}")
            M = va.shape[0] if mult is None else int(np.sum(np.maximum(np.asarray(mult, dtype=np.int64), 0)))
            if M < 1:
                raise ValueError("the selection holds no sample")
            n, shape, n_chains = va.shape[1], (va.shape[1],), None
            out = self._sampler.modes(radius_sq_sum=rad * rad * n, values=va, multiplicity=mult, sq_dist=bool(return_distances), outputs=True)
        else:
            xs = self._rows("x", x)
            kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
            if M < 1:
                raise ValueError("the selection holds no sample")
            n_x, O = len(self._host_rows(xs)), int(self.topology[2])
            n, shape = n_x * O, (n_x, O)
            n_chains = None if weights is not None else (self.num_chains if kw["replicas"] is None else len(kw["replicas"]))
            out = self._sampler.modes(xs, radius_sq_sum=rad * rad * n, sq_dist=bool(return_distances), outputs=True, **kw)
        return finish_modes(out, shape, n, sep * sep * n, min_mass, n_chains, with_rows=values is None)
