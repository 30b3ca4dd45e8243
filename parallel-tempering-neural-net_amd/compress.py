"""Posterior compression of the drop-in (not in the reference, which hands every sampled net to whoever wants to use the fit): a
few dozen of the sampled nets, chosen so that together they stand for all of them.  The host-only helpers, the result tuple, and
the mixin that holds the public method.  The method checks its arguments here, makes one low-level call of `_lib.Sampler` (the
device forms the all-pairs function-space distance of the distinct samples as posterior_modes does, and walks the herding
sequence on it) and finishes the result with host arithmetic in float64 and integers.
"""
import math
from collections import namedtuple

import numpy as np

from ._lib import TASK_REG

# posterior_compress' result: U distinct samples, M selected samples, m picks, n = n_rows * n_out output columns.  picks [m] int64,
# distinct-sample indices in herding order: any prefix is the herded set of that size; items [m] int64, the first selected item of
# each pick (evaluate= takes them back); rows [m, 2] int64 (chain, selected-row index) of that item (-1 where there is no chain or
# no row); vectors [m, num_param] float32 (None for values=); eta [m] float32, the eta recorded with that trace row or given with
# that vector (None for a classification, for values= and for weights= without eta=): carried along, not matched; energy [m], the
# energy distance between the first k picks with equal weights and the full weighted sample, in the units of the summed distance
# sqrt(sq), and spread = D0 = E d(X, X') of the full sample in the same units; energy_rms, spread_rms: both divided by sqrt(n), the
# RMS output difference posterior_modes reports; equivalent_draws [m] = D0 / energy_k: the independent draws the first k picks are
# worth (inf where the energy is not positive); pick_score [m]; evaluated [B], the energies of the evaluate= subsets (None without);
# energy_thinned, the energy of the evenly spaced m-subset of the selected samples (None for m = 0); mean_gap, the largest
# |difference| over the output columns between the predictive mean of the full sample and of the picks, and sd_ratio, the median
# over the columns of sd(picks) / sd(full) (both None for m = 0); mu [U], every distinct sample's mean distance to the full sample;
# n_samples; n_distinct; distances [U, U] on request (d / sqrt(n)).
PosteriorCompression = namedtuple("PosteriorCompression", "picks items rows vectors eta energy spread energy_rms spread_rms equivalent_draws "
                                                          "pick_score evaluated energy_thinned mean_gap sd_ratio mu n_samples n_distinct distances")


def thinned_items(m, n_items, multiplicity=None):
    """The evenly spaced m-subset of a selection: positions k * M // m, k < m, of the M samples in the selection's order (an item of
    multiplicity c holds c consecutive positions, one of multiplicity 0 none) -> int64 item indices [m]."""
    if multiplicity is None:
        return (np.arange(m, dtype=np.int64) * n_items) // max(m, 1)
    ends = np.cumsum(np.maximum(np.asarray(multiplicity, dtype=np.int64), 0))
    pos = (np.arange(m, dtype=np.int64) * int(ends[-1])) // max(m, 1)
    return np.searchsorted(ends, pos, side="right").astype(np.int64)


def first_items(item_sample, n_distinct):
    """The first selected item of every distinct sample -> int64 [U] (-1: no item)."""
    item = np.asarray(item_sample, dtype=np.int64)
    first = np.full(n_distinct, -1, np.int64)
    first[item[::-1]] = np.arange(len(item))[::-1]
    return first


def moment_match(outputs, count, picks):
    """How well the picks with equal weights reproduce the first two moments of the full weighted sample, per output column, in
    float64: -> (the largest |difference| of the means, the median of sd(picks) / sd(full) over the columns where sd(full) > 0,
    nan where there is none)."""
    F = np.asarray(outputs, dtype=np.float64)
    w = np.asarray(count, dtype=np.float64)
    w = w / w.sum()
    mean = w @ F
    sd = np.sqrt(w @ (F - mean) ** 2)
    Fp = F[np.asarray(picks, dtype=np.int64)]
    ok = sd > 0
    ratio = float(np.median(Fp.std(axis=0)[ok] / sd[ok])) if ok.any() else float("nan")
    return float(np.max(np.abs(Fp.mean(axis=0) - mean))), ratio


def finish_compress(out, n, n_chains=None, with_rows=True, vectors=None, eta=None, evaluated=None, energy_thinned=None):
    """The host arithmetic of posterior_compress: the device's picks, curve, item map and outputs [U, n] -> PosteriorCompression.
    n_chains: the trace's chains (the items are chain-major), None for weights= and values=."""
    picks = np.asarray(out["picks"], dtype=np.int64)
    item = np.asarray(out["item_sample"], dtype=np.int64)
    U, m = int(out["n_distinct"]), len(picks)
    energy, d0 = np.asarray(out["energy"], dtype=np.float64), float(out["d0"])
    items = first_items(item, U)[picks]
    rows = np.full((m, 2), -1, np.int64)
    if n_chains is not None:
        per = len(item) // n_chains
        rows = np.stack([items // per, items % per], axis=1) if m else rows
    elif with_rows:
        rows[:, 1] = items
    with np.errstate(divide="ignore"):
        draws = np.where(energy > 0, d0 / np.where(energy > 0, energy, 1.0), np.inf)
    gap, ratio = moment_match(out["outputs"], out["count"], picks) if m else (None, None)
    root = math.sqrt(n)
    dist = None if out.get("sq_dist") is None else np.sqrt(np.asarray(out["sq_dist"], dtype=np.float64) / n)
    return PosteriorCompression(picks=picks, items=items, rows=rows, vectors=vectors, eta=eta, energy=energy, spread=d0, energy_rms=energy / root,
                                spread_rms=d0 / root, equivalent_draws=draws, pick_score=np.asarray(out["pick_score"], dtype=np.float64),
                                evaluated=evaluated, energy_thinned=energy_thinned, mean_gap=gap, sd_ratio=ratio,
                                mu=np.asarray(out["mu"], dtype=np.float64), n_samples=int(out["n_samples"]), n_distinct=U, distances=dist)


class CompressAnalysis:
    """posterior_compress(), for `ParallelTemperingBase` to inherit next to `ModesAnalysis`; it uses the row and sample-source helpers
    of `PosteriorAnalysis` and reads the constructor's attributes `task`, `topology`, `num_chains`, `num_param` and `_sampler`."""

    def posterior_compress(self, m, x="train", *, burn_in=None, chains="all", thin=1, weights=None, eta=None, values=None, evaluate=None,
                           return_distances=False):
        """`m` of the sampled nets that together stand for all of them, chosen on the GPU to match the posterior (DESIGN.md section
        34): every analysis call takes them as weights=result.vectors (and eta=result.eta), as it takes the vectors of
        rung_reweighting.

        Sampled nets are compared by what they compute, as in posterior_modes: d = the distance of two nets' outputs on the rows
        `x`.  The picks are the kernel-herding sequence of the energy-distance kernel ("support points"): pick k + 1 is the sample
        whose mean distance to the full sample, less its mean distance to the k picks so far, is smallest.  `energy[k - 1]` is the
        energy distance between the first k picks (equal weights) and the full sample; any prefix of the picks is the herded set of
        that size.  The curve is NOT monotone in k: one more pick can raise it.  A random k-subset drawn with replacement has
        expected energy exactly spread / k, so `equivalent_draws` = spread / energy says how many independent draws the picks are
        worth; thin= and rung_reweighting(resample=) pick blindly and are worth about as many draws as they keep
        (`energy_thinned`).  eta is carried with each pick, not matched.

        Samples, `chains`, `thin`, `weights` and `values` as posterior_modes(); `eta` [n] comes with weights= and is handed back for
        the picks.  m: an integer from 0 to the number of present distinct samples.  `evaluate`: one list of item indices of this
        selection, or an array [B, k] of them (repeats allowed): the energy of each subset against the full sample on these rows --
        with m = 0 and another `x`, the picks of an earlier call judged on rows they were not chosen on.
        -> PosteriorCompression."""
        self._need_sampler("posterior_compress")
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 0:
            raise ValueError(f"m = {m!r} must be an integer in [0, the present distinct samples]")
        m = int(m)
        if eta is not None and weights is None:
            raise ValueError("eta= comes with weights=: the trace carries its own, values= has none")
        mult = w = None
        if values is not None:
            if weights is not None:
                raise ValueError("values= takes the place of the samples: no weights= with it")
            if isinstance(values, tuple):
                values, mult = values
            va = np.asarray(values, dtype=np.float32)
            if va.ndim != 2 or va.shape[0] < 1 or va.shape[1] < 1:
                raise ValueError(f"values must be [n_samples, n_a], got shape {va.shape}")
            n_items, n, n_chains = va.shape[0], va.shape[1], None
            args, kw = (), dict(values=va, multiplicity=mult)
        else:
            xs = self._rows("x", x)
            kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
            if weights is not None:
                w, mult = kw["w"], kw["multiplicity"]
                n_items, n_chains = w.shape[0], None
                if eta is not None:
                    eta = np.asarray(eta, dtype=np.float32).reshape(-1)
                    if eta.shape != (n_items,):
                        raise ValueError(f"eta must have one entry per vector: {n_items}, got shape {eta.shape}")
            else:
                n_items, n_chains = M, (self.num_chains if kw["replicas"] is None else len(kw["replicas"]))
            n = len(self._host_rows(xs)) * int(self.topology[2])
            args = (xs,)
        positive = n_items if mult is None else int(np.count_nonzero(np.asarray(mult, dtype=np.int64) > 0))
        if positive < 1:
            raise ValueError("the selection holds no sample")
        if m > positive:
            raise ValueError(f"m = {m} picks but the selection holds {positive} items with a positive count")
        subsets = None
        if evaluate is not None:
            subsets = np.asarray(evaluate)
            if subsets.ndim == 1:
                subsets = subsets[None, :]
            if subsets.ndim != 2 or subsets.shape[1] < 1 or not np.issubdtype(subsets.dtype, np.integer):
                raise ValueError(f"evaluate must be one list of item indices or an array [B, k] of them, got shape {np.shape(evaluate)}")
            if subsets.size and (subsets.min() < 0 or subsets.max() >= n_items):
                bad = subsets[(subsets < 0) | (subsets >= n_items)][0]
                raise ValueError(f"evaluate holds item {int(bad)} outside [0, {n_items})")
            if mult is not None and subsets.size and (np.asarray(mult, dtype=np.int64)[subsets] <= 0).any():
                bad = subsets[np.asarray(mult, dtype=np.int64)[subsets] <= 0][0]
                raise ValueError(f"evaluate holds item {int(bad)}, whose multiplicity is 0: it is absent from the selection")
            subsets = np.ascontiguousarray(subsets, dtype=np.int32)
        thinned = thinned_items(m, n_items, mult).astype(np.int32)[None, :] if m else None
        # one low-level call: the thinned subset rides with evaluate= when they have one size, else it is judged by a call of its own
        together = thinned is not None and (subsets is None or subsets.shape[1] == m)
        sub = thinned if subsets is None else (np.concatenate([subsets, thinned]) if together else subsets)
        out = self._sampler.compress(*args, m=m, subsets=sub, sq_dist=bool(return_distances), outputs=True, **kw)
        energies = out["subset_energy"]
        energy_thinned = evaluated = None
        if thinned is not None:
            energy_thinned = float(energies[-1]) if together else float(
                self._sampler.compress(*args, m=0, subsets=thinned, **kw)["subset_energy"][0])
        if subsets is not None:
            evaluated = np.asarray(energies[:len(subsets)], dtype=np.float64)
        res = finish_compress(out, n, n_chains, with_rows=values is None, evaluated=evaluated, energy_thinned=energy_thinned)
        if values is not None or m == 0:
            return res
        if w is not None:
            return res._replace(vectors=np.ascontiguousarray(w[res.items], dtype=np.float32), eta=None if eta is None else eta[res.items])
        # the trace: pick k is row step0 + thin * rows[k, 1] of chain replicas[rows[k, 0]]
        reps = list(range(self.num_chains)) if kw["replicas"] is None else kw["replicas"]
        reg = self.task == TASK_REG
        vectors, etas = np.empty((m, self.num_param), np.float32), np.empty(m, np.float32)
        for k, (c, r) in enumerate(res.rows):
            step = kw["step0"] + kw["thin"] * int(r)
            vectors[k] = self._sampler.traces(step, 1)["pos_w"][reps[int(c)], 0]
            if reg:
                etas[k] = self._sampler.trace_rows(step, 1)[reps[int(c)], 0, 3]
        return res._replace(vectors=vectors, eta=etas if reg else None)
