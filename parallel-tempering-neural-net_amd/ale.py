"""Accumulated local effects of the drop-in (not in the reference): what the sampled nets do as an input moves across the bin each
data row already lies in, averaged per bin, accumulated and centred (Apley & Zhu 2020), first order and for pairs of inputs, once
per sampled net, so that curve, surface and interaction strength get a posterior band.  The host-only edge helpers, the result
tuple, and the body of `EffectAnalysis.accumulated_effects` (effects.py), which checks its arguments here, makes one low-level call
of `_lib.Sampler` (the device does the work) and finishes the result with host arithmetic.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import check_percentiles, top_share

# accumulated_effects' result, A selected inputs, Q pairs, O outputs.  inputs [A] int64; edges: A float64 arrays, the bin edges of
# each input with the padding stripped (E_a = len(edges[a]) <= E, the common padded width of the arrays below: positions from E_a
# on repeat position E_a - 1); bin_count [A, E - 1] int64.  The curve ALE_s[a, k, o] at the edges, per sample s: ale_mean [A, E, O]
# float64, ale_percentiles {p: [A, E, O]}; range_s[a, o] = max_k - min_k: effect_range (its mean), effect_range_percentiles {p:
# ...}, top_prob (the share of the samples in which the input has the largest range of the output) [A, O]; sample_ale [n_samples,
# A, E, O] float32.  Pairs (None / {} without any): pairs [Q, 2] int64; pair_edges: Q pairs of float64 arrays; cell_count [Q, E2 -
# 1, E2 - 1]; the surface at the edge pairs ale2_mean [Q, E2, E2, O], ale2_percentiles; its count-weighted RMS interaction [Q, O]
# (the mean), interaction_percentiles; sample_ale2, sample_interaction.  Per row (local=True, else None / {}): local_mean [n_rows, A
# + Q, O], local_percentiles: the local effects, first-order slots then pairs; samples [n_samples, n_rows, A + Q, O] or None.
AccumulatedEffects = namedtuple("AccumulatedEffects", "inputs edges bin_count ale_mean ale_percentiles effect_range effect_range_percentiles "
                                                      "top_prob sample_ale pairs pair_edges cell_count ale2_mean ale2_percentiles interaction "
                                                      "interaction_percentiles sample_ale2 sample_interaction local_mean local_percentiles "
                                                      "samples n_samples n_distinct")


def _input_indices(inputs, n_in):
    """None (all n_in) or distinct integer indices in [0, n_in) -> [A] int32."""
    idx = np.arange(n_in, dtype=np.int32) if inputs is None else np.atleast_1d(np.asarray(inputs))
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= n_in:
        raise ValueError(f"inputs {inputs!r}: one or more integer indices in [0, {n_in})")
    if np.unique(idx).size != idx.size:
        raise ValueError(f"inputs {inputs!r}: an index is given twice")
    return idx.astype(np.int32)


def _pad_edges(lists, max_edges, what):
    """Per input one array of edges -> [len(lists), E] float32, each row strictly increasing and then padded with its last edge."""
    rows = []
    for a, e in enumerate(lists):
        with np.errstate(over="ignore"):
            e32 = np.asarray(e, dtype=np.float64).reshape(-1).astype(np.float32)
        if not np.all(np.isfinite(e32)):
            raise ValueError(f"{what}[{a}]: an edge is not a finite float32")
        if e32.size < 2 or np.any(np.diff(e32) <= 0):
            raise ValueError(f"{what}[{a}]: at least two edges, strictly increasing as float32")
        if e32.size > max_edges:
            raise ValueError(f"{what}[{a}] = {e32.size} edges: at most {max_edges} per input")
        rows.append(e32)
    E = max(r.size for r in rows)
    return np.ascontiguousarray([np.concatenate([r, np.full(E - r.size, r[-1], np.float32)]) for r in rows], dtype=np.float32)


def ale_edges(rows, inputs, bins, max_edges=_lib.ALE_MAX_EDGES):
    """The bin edges of accumulated local effects.  rows [n, >= n_in]: the data rows; inputs: indices of columns; bins: an integer
    K, 1 <= K < max_edges.  Input j gets np.percentile(rows[:, j], np.linspace(0, 100, K + 1)) as float32 with the duplicates
    removed (a column with ties has fewer, wider bins), at least two distinct edges, padded at the end by repeating the last
    edge so that every input has K + 1.  -> edges [A, K + 1] float32."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) < max_edges:
        raise ValueError(f"bins = {bins!r}: an integer between 1 and {max_edges - 1}")
    K = int(bins)
    cols = np.asarray(rows, dtype=np.float64)
    out = np.empty((len(inputs), K + 1), np.float32)
    for a, j in enumerate(inputs):
        z = np.unique(np.percentile(cols[:, int(j)], np.linspace(0, 100, K + 1)).astype(np.float32))
        if z.size < 2 or not np.all(np.isfinite(z)):
            raise ValueError(f"input {int(j)}: its column needs two distinct finite values to have a bin")
        out[a, :z.size] = z
        out[a, z.size:] = z[-1]
    return out


def _strip(row):
    """A padded row of edges -> float64 without the padding."""
    return row[:int(np.argmax(row)) + 1].astype(np.float64)


def accumulated_effects(self, x="train", *, inputs=None, bins=16, edges=None, pairs=None, pair_bins=6, pair_edges=None,
                        percentiles=(5, 95), local=False, burn_in=None, chains="all", thin=1, weights=None, return_samples=False):
    """Accumulated local effects (Apley & Zhu 2020) of the sampled nets, first order and of input pairs, with posterior
    bands, computed on the GPU.  partial_dependence() sets an input to a grid value on every row; for
    correlated inputs -- the lags of one series -- that evaluates the nets where no data lies.  Here an input is moved only
    across the bin its row already lies in; the local differences are averaged per bin, accumulated and centred.  The
    second-order effect of a pair is what two inputs do together beyond their main effects.

    `inputs`: None (all) or a list of input indices.  `bins`: an integer K -- input j gets the edges ale_edges() makes of the
    rows' column (its 0, 100 / K, ... percentiles, duplicates removed) --, or `edges`: one strictly increasing array per
    selected input, at most 64 edges, used as float32.  A row's bin is the first whose upper edge is >= its value; rows
    outside the edges fall in the first or last bin.  `pairs`: None, "all" (every pair of the selected inputs, at most 16)
    or a list of (j, l); each input of a pair gets `pair_bins` quantile bins of its own, or `pair_edges`: per pair two arrays,
    at most 16 edges.  An empty cell contributes a zero second difference (ALEPlot borrows from the nearest non-empty cell
    instead); cell_count says how much of a surface rests on data.  Sample set, `chains`, `thin`, `weights` and `x` as in
    posterior_predictive; percentiles follow np.percentile(method="linear") exactly.

    -> AccumulatedEffects: inputs, edges (padding stripped), bin_count; over the samples ale_mean and ale_percentiles[q] [A,
    E, O] at the edges (positions past an input's last edge repeat it), effect_range, effect_range_percentiles[q] and
    top_prob [A, O], sample_ale; with pairs: pairs, pair_edges, cell_count, ale2_mean and ale2_percentiles[q] [Q, E2, E2, O],
    interaction (the count-weighted RMS of the surface) and interaction_percentiles[q] [Q, O], sample_ale2,
    sample_interaction; with local=True the per-row local effects' local_mean and local_percentiles[q] [n_rows, A + Q, O];
    samples [n_samples, n_rows, A + Q, O] (chain-major) on request; n_samples, n_distinct."""
    self._need_sampler("accumulated_effects")
    xs = self._rows("x", x)
    n_in = int(self.topology[0])
    host = np.asarray(self._host_rows(xs)[:, :n_in], dtype=np.float32)      # the rows as the device compares them with the edges
    idx = _input_indices(inputs, n_in)
    if edges is None:
        e32 = ale_edges(host, idx, bins)
    else:
        if len(edges) != idx.size:
            raise ValueError(f"edges must hold one array per selected input ({idx.size}), got {len(edges)}")
        e32 = _pad_edges(edges, _lib.ALE_MAX_EDGES, "edges")
    if pairs is None:
        pr = np.zeros((0, 2), np.int32)
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"pairs must be None, 'all' or a list of (j, l), not {pairs!r}")
        pr = np.array([(int(j), int(l)) for a, j in enumerate(idx) for l in idx[a + 1:]], np.int32).reshape(-1, 2)
    else:
        pr = np.asarray(pairs)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu" or pr.size == 0 or pr.min() < 0 or pr.max() >= n_in:
            raise ValueError(f"pairs {pairs!r}: a list of pairs (j, l) of integer indices in [0, {n_in})")
        pr = pr.astype(np.int32)
    Q = pr.shape[0]
    if Q > _lib.ALE_MAX_PAIRS:
        raise ValueError(f"{Q} pairs: at most {_lib.ALE_MAX_PAIRS} per call")
    if np.any(pr[:, 0] == pr[:, 1]) or len({frozenset(p) for p in pr.tolist()}) != Q:
        raise ValueError(f"pairs {pr.tolist()}: two different inputs per pair, and no pair twice")
    e2 = None
    if Q:
        if pair_edges is None:
            e2 = ale_edges(host, pr.reshape(-1), pair_bins, _lib.ALE_MAX_EDGES2).reshape(Q, 2, -1)
        else:
            if len(pair_edges) != Q or any(len(p) != 2 for p in pair_edges):
                raise ValueError(f"pair_edges must hold two arrays per pair ({Q} pairs)")
            e2 = _pad_edges([e for p in pair_edges for e in p], _lib.ALE_MAX_EDGES2, "pair_edges").reshape(Q, 2, -1)
    pcts = check_percentiles(percentiles)
    kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
    spots, ranks = self._band_ranks(M, pcts)
    out = self._sampler.accumulated_effects(xs, inputs=idx, edges=e32, pairs=pr if Q else None, edges2=e2, ranks=ranks if local else [],
                                            ranks2=ranks, local_mean=bool(local), sample_ale=True, sample_range=True,
                                            sample_ale2=bool(Q), sample_inter=bool(Q), samples=bool(return_samples), **kw)
    has = bool(ranks)
    bands = lambda key: self._bands(out[key], pcts, spots, ranks) if has and out[key] is not None else {}     # noqa: E731
    return AccumulatedEffects(
        inputs=idx.astype(np.int64), edges=[_strip(r) for r in e32], bin_count=out["bin_count"], ale_mean=out["ale_mean"],
        ale_percentiles=bands("ale_order_stats"), effect_range=out["range_mean"],
        effect_range_percentiles=bands("range_order_stats"),
        top_prob=top_share(np.moveaxis(out["sample_range"], 1, 2)).T, sample_ale=out["sample_ale"],
        pairs=pr.astype(np.int64) if Q else None, pair_edges=[(_strip(p[0]), _strip(p[1])) for p in e2] if Q else None,
        cell_count=out["cell_count"], ale2_mean=out["ale2_mean"], ale2_percentiles=bands("ale2_order_stats"),
        interaction=out["inter_mean"], interaction_percentiles=bands("inter_order_stats"), sample_ale2=out["sample_ale2"],
        sample_interaction=out["sample_inter"], local_mean=out["local_mean"], local_percentiles=bands("local_order_stats"),
        samples=out["samples"], n_samples=out["n_samples"], n_distinct=out["n_distinct"])
