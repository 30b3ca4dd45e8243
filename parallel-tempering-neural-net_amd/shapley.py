"""Shapley attributions of the drop-in (not in the reference): how much of one prediction each input accounts for against a
background sample (Shapley 1953; Strumbelj & Kononenko 2014; Lundberg & Lee 2017: the interventional value function), once per
sampled net, so that the split gets a posterior band.  The host-only coalition-table helper, the result tuple, and the body of
`EffectAnalysis.shapley_values` (effects.py), which checks its arguments here, makes one low-level call of `_lib.Sampler` (the
device evaluates the coalitions) and finishes the result with host arithmetic.
"""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import check_percentiles, top_share

# shapley_values' result, O outputs, I = n_in inputs.  method "exact" or "permutation", n_coalitions (distinct coalitions evaluated
# per sample, row and background row), background [B, n_in] float32 (the rows used).  base [O] float64 and base_percentiles {p:
# [O]}: v(empty) = the mean output over the background, over the samples; fx_mean [n_rows, O]: the mean of v(all) = the output on
# the row.  Per row, output and input: phi_mean, phi_percentiles {p: ...}, prob_positive [n_rows, O, n_in] float64.  Per output and
# input, with a_s = the mean over the rows of |phi| in sample s: importance (its mean), importance_percentiles {p: ...}, top_prob
# (the share of the samples in which the input has the largest a_s of the output) [O, n_in] float64.  efficiency_gap: the largest
# |sum_j phi_mean - (fx_mean - base)|.  sample_importance [n_samples, O, n_in] float32; samples [n_samples, n_rows, O, n_in + 2]
# float32 (chain-major; the last axis holds phi_0 .. phi_{I-1}, v(empty), v(all)) or None; n_samples; n_distinct
ShapleyValues = namedtuple("ShapleyValues", "method n_coalitions background base base_percentiles fx_mean phi_mean phi_percentiles "
                                            "prob_positive importance importance_percentiles top_prob efficiency_gap "
                                            "sample_importance samples n_samples n_distinct")

SHAP_EXACT_DEFAULT, SHAP_EXACT_MAX = 6, 12      # exact enumeration: the default up to 6 inputs, allowed up to 12 (2^12 coalitions)


def shapley_method(n_in, method, permutations=None):
    """'auto' resolved: 'exact' up to 6 inputs when no orders are given, else 'permutation'."""
    if method not in ("auto", "exact", "permutation"):
        raise ValueError(f"method = {method!r} must be 'auto', 'exact' or 'permutation'")
    if method != "auto":
        return method
    return "exact" if permutations is None and n_in <= SHAP_EXACT_DEFAULT else "permutation"


def shapley_table(n_in, method="auto", n_permutations=32, seed=None, permutations=None):
    """The coalition table of Shapley values for `n_in` inputs -> (masks [C] uint64, coef [C, n_in + 2] float64): the device
    evaluates v(S) for every mask (bit i set: input i from the explained row) and returns sum_c coef[c, t] v(S_c) per term t.
    Terms 0 .. n_in - 1 are the inputs' Shapley values, term n_in is v(empty) (the base value), term n_in + 1 is v(all).

    method "exact" (the "auto" choice for n_in <= 6, allowed up to 12): all 2^n_in masks in ascending order, for every S without j
    coef[S + {j}, j] += w and coef[S, j] -= w with w = |S|! (n_in - |S| - 1)! / n_in!.  method "permutation" (the "auto" choice
    otherwise): `n_permutations` orders (an even number) drawn from np.random.default_rng(seed) in antithetic pairs, an order and
    its reverse, or the explicit orders `permutations` [n, n_in]; prefix k of an order adds +1/n to the input it just added and
    -1/n to the next.  Equal masks are merged (their rows summed) in the order of their first appearance, so each distinct
    coalition is evaluated once; the empty mask comes first."""
    I = int(n_in)
    if I != n_in or not 1 <= I <= _lib.SHAP_MAX_TERMS - 2:
        raise ValueError(f"n_in = {n_in!r} must be an integer in [1, {_lib.SHAP_MAX_TERMS - 2}]")
    method = shapley_method(I, method, permutations)
    T, full = I + 2, (1 << I) - 1
    if method == "exact":
        if permutations is not None:
            raise ValueError("method = 'exact' enumerates every coalition: it takes no permutations")
        if I > SHAP_EXACT_MAX:
            raise ValueError(f"method = 'exact' with n_in = {I} needs 2^{I} coalitions: at most n_in = {SHAP_EXACT_MAX}; use 'permutation'")
        masks = np.arange(1 << I, dtype=np.uint64)
        coef = np.zeros((1 << I, T), np.float64)
        wt = [math.factorial(k) * math.factorial(I - k - 1) / math.factorial(I) for k in range(I)]
        for S in range(1 << I):
            w = wt[bin(S).count("1")] if S != full else 0.0
            for j in range(I):
                if not (S >> j) & 1:
                    coef[S | (1 << j), j] += w
                    coef[S, j] -= w
    else:
        if permutations is None:
            n = int(n_permutations)
            if n != n_permutations or n < 2 or n % 2:
                raise ValueError(f"n_permutations = {n_permutations!r} must be an even integer >= 2 (antithetic pairs)")
            rng = np.random.default_rng(seed)
            orders = np.empty((n, I), np.int64)
            for k in range(0, n, 2):
                orders[k] = rng.permutation(I)
                orders[k + 1] = orders[k][::-1]
        else:
            orders = np.asarray(permutations)
            if orders.ndim != 2 or orders.shape[0] < 1 or orders.shape[1] != I or orders.dtype.kind not in "iu":
                raise ValueError(f"permutations must be [n, {I}] integer orders, got shape {np.shape(permutations)}")
            if not np.array_equal(np.sort(orders, axis=1), np.broadcast_to(np.arange(I), orders.shape)):
                raise ValueError(f"permutations: every row must hold each of 0 .. {I - 1} once")
        n = orders.shape[0]
        index, rows = {}, []

        def row(mask):
            if mask not in index:
                index[mask] = len(rows)
                rows.append(np.zeros(T, np.float64))
            return rows[index[mask]]
        row(0)
        for order in orders:
            mask = 0
            for j in (int(v) for v in order):
                row(mask)[j] -= 1.0 / n
                mask |= 1 << j
                row(mask)[j] += 1.0 / n
        masks = np.array(list(index), dtype=np.uint64)
        coef = np.stack(rows)
        if masks.size > _lib.SHAP_MAX_COALITIONS:
            raise ValueError(f"{n} permutations of {I} inputs give {masks.size} distinct coalitions: at most {_lib.SHAP_MAX_COALITIONS} per call")
    coef[int(np.flatnonzero(masks == 0)[0]), I] = 1.0
    coef[int(np.flatnonzero(masks == np.uint64(full))[0]), I + 1] = 1.0
    return masks, coef


def shapley_values(self, x="test", background="train", *, max_background=64, method="auto", n_permutations=32, seed=None,
                   permutations=None, percentiles=(5, 95), burn_in=None, chains="all", thin=1, weights=None, return_samples=False):
    """How much of one prediction each input accounts for, and how sure the posterior is of that split, computed on the GPU
    (DESIGN.md section 29): Shapley values (Shapley 1953; Strumbelj & Kononenko 2014) of the output posterior_predictive()
    returns, against a background sample, with the interventional value function (Lundberg & Lee 2017): v(S) is the mean over
    the background rows b of the output on the row that takes the inputs in S from the explained row and the others from b.
    For every selected sample, row of `x` and output, phi_j sums to v(all) - v(empty) = the row's output minus the mean output
    over the background.  input_sensitivity() gives the slope at the rows and partial_dependence() one input's curve averaged
    over the rows; this splits a single prediction among the inputs, once per sample, so the split gets a band.

    For the time-series nets the inputs are lags of one series and depend on each other: the interventional value function
    evaluates the net on lag combinations the series never produced, as partial_dependence() does.  With method
    "permutation" the values are a Monte-Carlo estimate whose own error is not reported: the same orders serve every sample,
    row and background row, so the band over the samples shows the posterior and not that error.

    `background`: "train", "test" or an array of rows (its first n_in columns); with more than `max_background` (at most
    256) rows, the rows at np.rint(np.linspace(0, n - 1, max_background)) are taken.  `method`, `n_permutations`, `seed`,
    `permutations`: the coalition table, see shapley_table(); "auto" is exact up to 6 inputs.  Sample set, `chains`, `thin`,
    `weights` and `x` as in posterior_predictive; percentiles follow np.percentile(method="linear") exactly.

    -> ShapleyValues: method, n_coalitions, background (the rows used); base [O] and base_percentiles[q] (v(empty) over the
    samples); fx_mean [n_rows, O]; phi_mean, phi_percentiles[q] and prob_positive [n_rows, O, n_in] (the layout of
    input_sensitivity); with a_s = the mean over the rows of |phi| in sample s: importance (the mean of a_s),
    importance_percentiles[q] and top_prob (the share of the samples in which this input has the largest a_s of the output,
    first index on a tie) [O, n_in]; efficiency_gap = the largest |sum_j phi_mean - (fx_mean - base)|; sample_importance
    [n_samples, O, n_in]; samples [n_samples, n_rows, O, n_in + 2] (chain-major; phi, then v(empty) and v(all)) on request;
    n_samples, n_distinct."""
    self._need_sampler("shapley_values")
    xs = self._rows("x", x)
    I = int(self.topology[0])
    bg = self._host_rows(self._rows("background", background))
    bg = np.ascontiguousarray(np.asarray(bg)[:, :I], dtype=np.float32)
    nb = int(max_background)
    if nb != max_background or not 1 <= nb <= _lib.SHAP_MAX_BACKGROUND:
        raise ValueError(f"max_background = {max_background!r} must be an integer in [1, {_lib.SHAP_MAX_BACKGROUND}]")
    if bg.shape[0] < 1:
        raise ValueError("background holds no row")
    if bg.shape[0] > nb:
        bg = np.ascontiguousarray(bg[np.rint(np.linspace(0, bg.shape[0] - 1, nb)).astype(np.int64)])
    if not np.all(np.isfinite(bg)):
        b, i = (int(v[0]) for v in np.nonzero(~np.isfinite(bg)))
        raise ValueError(f"background[{b}, {i}] = {bg[b, i]} is not a finite float32")
    masks, coef = shapley_table(I, method, n_permutations, seed, permutations)
    pcts = check_percentiles(percentiles)
    kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
    spots, ranks = self._band_ranks(M, pcts)
    out = self._sampler.coalition_values(xs, background=bg, masks=masks, coef=coef, ranks=ranks, ranks2=ranks, counts=True,
                                         sample_abs=True, samples=bool(return_samples), **kw)
    mean, sa = out["mean"], out["sample_abs"][:, :, :I]
    has = bool(ranks)
    bands = self._bands(out["order_stats"], pcts, spots, ranks) if has else {}
    abs_bands = self._bands(out["abs_order_stats"], pcts, spots, ranks) if has else {}
    phi, base, fx = mean[:, :, :I], mean[:, :, I], mean[:, :, I + 1]
    return ShapleyValues(
        method=shapley_method(I, method, permutations), n_coalitions=int(masks.size), background=bg,
        base=base[0].copy(), base_percentiles={p: v[0, :, I].copy() for p, v in bands.items()}, fx_mean=fx.copy(),
        phi_mean=phi.copy(), phi_percentiles={p: v[:, :, :I].copy() for p, v in bands.items()},
        prob_positive=out["pos_count"][:, :, :I] / np.float64(M),
        importance=out["abs_mean"][:, :I].copy(), importance_percentiles={p: v[:, :I].copy() for p, v in abs_bands.items()},
        top_prob=top_share(sa), efficiency_gap=float(np.max(np.abs(phi.sum(axis=2) - (fx - base)))),
        sample_importance=np.ascontiguousarray(sa), samples=out["samples"], n_samples=out["n_samples"], n_distinct=out["n_distinct"])
