"""Partial dependence and ICE curves of the drop-in (not in the reference): what the sampled nets do as one input goes over a grid
of values, the other inputs held at the data rows (Friedman 2001; Goldstein et al. 2015); and Shapley attributions: how much of
one prediction each input accounts for against a background sample (Shapley 1953; Strumbelj & Kononenko 2014; Lundberg & Lee
2017; the helpers, the result tuple and the method's body live in shapley.py; accumulated local effects likewise in ale.py).  The host-only grid helper, the result tuple, and
the mixin that holds the public methods.  A method checks its arguments, makes one low-level call of `_lib.Sampler` (the device
does the work) and finishes the result with host arithmetic.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from . import ale as _ale
from . import shapley as _shapley
from .ale import AccumulatedEffects, ale_edges  # noqa: F401
from .analysis import check_percentiles, top_share
from .shapley import ShapleyValues, shapley_table  # noqa: F401

# partial_dependence's result, A selected inputs, G grid values, O outputs.  inputs [A] int64; grid [A, G] float64 (the float32
# values the device used).  The curve PD_s[a, k, o] = the mean over the rows of the output with input a set to grid[a, k], per
# sample s: pd_mean [A, G, O] float64 and pd_percentiles {p: [A, G, O]} over the samples.  How far a sample's curve moves,
# range_s[a, o] = max_k - min_k: effect_range (its mean), effect_range_percentiles {p: ...}, top_prob (the share of the samples in
# which the input has the largest range of the output) [A, O] float64.  Per row (ice=True, else None / {}): ice_mean [n_rows, A, G,
# O] float64, ice_percentiles {p: ...}.  sample_pd [n_samples, A, G, O] float32 and samples [n_samples, n_rows, A, G, O] float32
# (chain-major) or None; n_samples; n_distinct
PartialDependence = namedtuple("PartialDependence", "inputs grid pd_mean pd_percentiles effect_range effect_range_percentiles top_prob "
                                                    "ice_mean ice_percentiles sample_pd samples n_samples n_distinct")


def pd_grid(rows, inputs, grid, grid_range=(5, 95)):
    """The selected inputs and their grids.  rows [n, >= n_in]: the data rows (only an integer `grid` reads them); inputs: None (all
    n_in = rows.shape[1]) or distinct indices in [0, n_in); grid: an integer G -- input j gets np.percentile(rows[:, j],
    np.linspace(lo, hi, G)) with grid_range = (lo, hi) --, an array [G] for every selected input, or an array [A, G].  1 <= G <=
    64, every value finite.  -> (inputs [A] int32, grid [A, G] float32)."""
    n_in = int(np.shape(rows)[1])
    idx = np.arange(n_in, dtype=np.int32) if inputs is None else np.atleast_1d(np.asarray(inputs))
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= n_in:
        raise ValueError(f"inputs {inputs!r}: one or more integer indices in [0, {n_in})")
    if np.unique(idx).size != idx.size:
        raise ValueError(f"inputs {inputs!r}: an index is given twice")
    idx = idx.astype(np.int32)
    A = idx.size
    if isinstance(grid, (int, np.integer)) and not isinstance(grid, bool):
        G = int(grid)
        if not 1 <= G <= _lib.PD_MAX_GRID:
            raise ValueError(f"grid = {G} values: between 1 and {_lib.PD_MAX_GRID} per input")
        try:
            lo, hi = (float(v) for v in grid_range)
        except (TypeError, ValueError):
            raise ValueError(f"grid_range = {grid_range!r} must be a pair (lo, hi) of percentiles") from None
        if not 0.0 <= lo <= hi <= 100.0:
            raise ValueError(f"grid_range = {grid_range!r} must satisfy 0 <= lo <= hi <= 100")
        cols = np.asarray(rows, dtype=np.float64)[:, idx]
        g = np.percentile(cols, np.linspace(lo, hi, G), axis=0).T
    else:
        g = np.asarray(grid, dtype=np.float64)
        if g.ndim == 1:
            g = np.broadcast_to(g, (A, g.size))
        if g.ndim != 2 or g.shape[0] != A:
            raise ValueError(f"grid must be an integer, [G] values or [{A}, G] (one row per selected input), got shape {np.shape(grid)}")
        if not 1 <= g.shape[1] <= _lib.PD_MAX_GRID:
            raise ValueError(f"grid = {g.shape[1]} values: between 1 and {_lib.PD_MAX_GRID} per input")
    with np.errstate(over="ignore"):
        g32 = np.ascontiguousarray(g, dtype=np.float32)
    if not np.all(np.isfinite(g32)):
        a, k = (int(v[0]) for v in np.nonzero(~np.isfinite(g32)))
        raise ValueError(f"grid[{a}, {k}] = {g32[a, k]} (input {int(idx[a])}) is not a finite float32")
    return idx, g32


class EffectAnalysis:
    """partial_dependence(), accumulated_effects() and shapley_values(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row, sample-source and
    percentile helpers it uses.  It reads the constructor's attributes `task`, `topology` and `_sampler`."""

    def partial_dependence(self, x="train", *, inputs=None, grid=16, grid_range=(5, 95), percentiles=(5, 95), ice=False, burn_in=None,
                           chains="all", thin=1, weights=None, return_samples=False):
        """What the sampled nets do as one input goes from its low values to its high ones, and how sure the posterior is of
        that shape, computed on the GPU: partial dependence (Friedman 2001) and individual conditional
        expectation curves (Goldstein et al. 2015) of the output posterior_predictive() returns -- a regression's sigmoid output,
        a classification's class probabilities.  For the time-series nets the inputs are lags.  input_sensitivity() gives the
        slope at the rows; this gives the curve, which a saturated unit with slope 0 at every row can still bend.

        For every selected sample s, row n of `x`, selected input a and grid value v = grid[a, k], ICE_s[n, a, k, o] is the
        output of the net on row n with input a set to v; the curve PD_s[a, k, o] is its mean over the rows, and range_s[a, o] =
        max_k PD_s - min_k PD_s is how far the curve moves.  `inputs`: None (all) or a list of input indices.  `grid`: an
        integer G (input j gets np.percentile(column j of the rows, np.linspace(lo, hi, G)) with grid_range = (lo, hi)), [G]
        values for every selected input, or [A, G]; at most 64 values per input, used as float32.  Sample set, `chains`, `thin`,
        `weights` and `x` as in posterior_predictive; percentiles follow np.percentile(method="linear") exactly.

        -> PartialDependence: inputs, grid; over the samples pd_mean and pd_percentiles[q] [A, G, O], effect_range (the mean of
        range_s), effect_range_percentiles[q] and top_prob (the share of the samples in which this input has the largest range
        of the output, first index on a tie) [A, O]; with ice=True the per-row ice_mean and ice_percentiles[q] [n_rows, A, G, O];
        sample_pd [n_samples, A, G, O]; samples [n_samples, n_rows, A, G, O] (chain-major) on request; n_samples, n_distinct."""
        self._need_sampler("partial_dependence")
        xs = self._rows("x", x)
        idx, g32 = pd_grid(self._host_rows(xs)[:, :int(self.topology[0])], inputs, grid, grid_range)
        pcts = check_percentiles(percentiles)
        kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.partial_dependence(xs, inputs=idx, grid=g32, ranks=ranks if ice else [], ranks2=ranks, ice_mean=bool(ice),
                                               sample_pd=True, sample_range=True, samples=bool(return_samples), **kw)
        sp, sr = out["sample_pd"], out["sample_range"]
        top = top_share(np.moveaxis(sr, 1, 2)).T                       # [M, A, O] -> top_share's [M, O, A] -> [A, O]
        has = bool(ranks)
        return PartialDependence(
            inputs=idx.astype(np.int64), grid=g32.astype(np.float64), pd_mean=out["pd_mean"],
            pd_percentiles=self._bands(out["pd_order_stats"], pcts, spots, ranks) if has else {},
            effect_range=out["range_mean"],
            effect_range_percentiles=self._bands(out["range_order_stats"], pcts, spots, ranks) if has else {}, top_prob=top,
            ice_mean=out["ice_mean"] if ice else None,
            ice_percentiles=self._bands(out["ice_order_stats"], pcts, spots, ranks) if ice and has else {},
            sample_pd=sp, samples=out["samples"], n_samples=out["n_samples"], n_distinct=out["n_distinct"])

    # accumulated local effects, first order and of input pairs, with their posterior bands (ale.py holds the body and the docstring)
    accumulated_effects = _ale.accumulated_effects

    # Shapley attributions of single predictions with their posterior bands (shapley.py holds the body and the docstring)
    shapley_values = _shapley.shapley_values
