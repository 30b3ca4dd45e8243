"""Predictive uncertainty of the drop-in (not in the reference, which publishes a mean and a band): how uncertain the sampled nets
are on a row, split into the part the data's noise explains (aleatoric) and the part the nets' disagreement explains (epistemic),
and whether abstaining on the most uncertain rows lowers the error.  The host-only helpers, the result tuple, and the mixin
that holds the public method.  The method checks its arguments here, makes one low-level call of `_lib.Sampler` (the device
does the work per sample) and finishes the result with host arithmetic in float64.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import check_percentiles
from .report import auc_pairs

TASK_CLS = _lib.TASK_CLS

# predictive_uncertainty's result, N rows, S samples.  Classification (K classes): p_mean, vote [N, K] float64
# (posterior_predictive's mean and vote); total = H(p_mean) (at most log K), aleatoric = the mean over the samples of H(p_s),
# epistemic = max(total - aleatoric, 0) (the mutual information between the prediction and the weights), confidence = max_k p_mean,
# variation_ratio = 1 - max_k vote, disagreement = 1 - sum_k vote^2, each [N] float64, entropies in nats; entropy_percentiles
# {q: [N] float64} of the samples' H(p_s); sample_entropy [S, N] float32 (chain-major) or None.  Regression: pred_mean,
# epistemic_var (the variance of the mean function over the samples), total_var = epistemic_var + aleatoric_var, epistemic_share =
# epistemic_var / total_var, each [N, n_out] float64; aleatoric_var = the mean of the samples' tau^2 = exp(eta), a float.  Both:
# selective {score: risk_coverage()} when the rows carry targets, else None; n_samples; n_distinct.  What belongs to the other
# task is None.
Uncertainty = namedtuple("Uncertainty", "p_mean vote total aleatoric epistemic confidence variation_ratio disagreement "
                                        "entropy_percentiles sample_entropy pred_mean epistemic_var aleatoric_var total_var "
                                        "epistemic_share selective n_samples n_distinct")

CLASSIFICATION_SCORES = ("total", "epistemic", "aleatoric", "confidence", "variation_ratio")      # "confidence": 1 - confidence
REGRESSION_SCORES = ("epistemic",)


def entropy(p):
    """H = -sum_k p_k log p_k over the last axis, natural log, 0 log 0 = 0 -> float64."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0.0, p * np.log(p), 0.0)
    return 0.0 - np.sum(t, axis=-1)


def risk_coverage(score, loss):
    """The risk-coverage curve of abstaining on the most uncertain rows (El-Yaniv & Wiener 2010; Geifman et al. 2019): the rows
    sorted by ascending `score` (stable: ties keep the row order), risk[j] = the mean `loss` of the j + 1 most certain rows,
    coverage[j] = (j + 1) / N, aurc = the mean of risk; aurc_optimal = the same with the rows sorted by the loss itself (no
    score does better); e_aurc = aurc - aurc_optimal.  Host arithmetic in float64.
    -> dict(coverage, risk, aurc, aurc_optimal, e_aurc)."""
    s = np.asarray(score, dtype=np.float64).reshape(-1)
    ls = np.asarray(loss, dtype=np.float64).reshape(-1)
    if s.size != ls.size or s.size < 1:
        raise ValueError(f"risk_coverage needs one score and one loss per row, and at least one row: got {s.size} and {ls.size}")
    count = np.arange(1, s.size + 1, dtype=np.float64)
    risk = np.cumsum(ls[np.argsort(s, kind="stable")]) / count
    best = np.cumsum(np.sort(ls, kind="stable")) / count
    aurc, optimal = float(np.mean(risk)), float(np.mean(best))
    return dict(coverage=count / s.size, risk=risk, aurc=aurc, aurc_optimal=optimal, e_aurc=aurc - optimal)


def uncertainty_scores(result):
    """The row scores of an Uncertainty result, larger = less certain -> {name: [N] float64}: a classification's total, epistemic,
    aleatoric, confidence (as 1 - confidence) and variation_ratio; a regression's epistemic (epistemic_var summed over the
    outputs; total_var orders the rows the same way)."""
    if result.total is not None:
        return dict(total=result.total, epistemic=result.epistemic, aleatoric=result.aleatoric, confidence=1.0 - result.confidence,
                    variation_ratio=result.variation_ratio)
    return dict(epistemic=np.sum(result.epistemic_var, axis=1))


def uncertainty_compare(a, b):
    """Per score both Uncertainty results hold: the probability that a row of `b` is ranked more uncertain than a row of `a`,
    ties counted half (the ROC-AUC of the score as a detector of b's rows) -- the usual out-of-distribution check between two
    row sets: 0.5 says the score does not tell them apart.  -> {name: float}."""
    sa, sb = uncertainty_scores(a), uncertainty_scores(b)
    out = {}
    for name in sa:
        if name in sb:
            x, y = np.asarray(sa[name], np.float64), np.asarray(sb[name], np.float64)
            both = np.concatenate([x, y])
            out[name] = auc_pairs(both, np.arange(both.size) >= x.size) / (2.0 * x.size * y.size)
    return out


class UncertaintyAnalysis:
    """predictive_uncertainty(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row, sample-source and
    percentile helpers it uses.  It reads the constructor's attributes `task`, `topology` and `_sampler`."""

    def predictive_uncertainty(self, data="test", *, percentiles=(5, 95), burn_in=None, chains="all", thin=1, weights=None, eta=None,
                               return_samples=False):
        """How uncertain is the model on each row, and is that noise in the data or disagreement among the sampled nets?
        Computed on the GPU from the sampled chains.

        Classification: total = H(p_mean), the entropy of the pooled prediction; aleatoric = the mean over the samples of
        H(p_s), what stays uncertain when the weights are known; epistemic = total - aleatoric >= 0, the mutual information
        between the prediction and the weights, which more data would remove.  Also confidence = max_k p_mean, variation_ratio
        = 1 - max_k vote, disagreement = 1 - sum_k vote^2, and entropy_percentiles[q] of the samples' H(p_s)
        (np.percentile(method="linear"), exactly).  Regression: epistemic_var = the variance of the mean function over the
        samples, aleatoric_var = the mean of the samples' noise variance tau^2 = exp(eta), total_var their sum (the variance of
        predictive_calibration's mixture), epistemic_share = epistemic_var / total_var.

        `data`: "train", "test" or rows.  Rows with more than n_in columns carry the target from column n_in on (a class label;
        a regression's n_out targets); with exactly n_in columns they carry none.  With targets, selective[score] =
        risk_coverage(score, loss): does abstaining on the rows the score calls uncertain lower the error?  A classification's
        scores are total, epistemic, aleatoric, confidence (1 - confidence) and variation_ratio, its loss the 0/1 error of argmax
        p_mean (first index on a tie); a regression's score is epistemic, its loss the squared error of pred_mean summed over
        the outputs.  Samples, `chains`, `thin` and `weights` (with `eta` for a regression) as predictive_calibration().
        -> Uncertainty; sample_entropy [n_samples, n_rows] (chain-major) with return_samples=True."""
        self._need_sampler("predictive_uncertainty")
        cls = self.task == TASK_CLS
        I, O = int(self.topology[0]), int(self.topology[2])
        n_target = 1 if cls else O
        rows = self._rows("data", data)
        pcts = check_percentiles(percentiles)
        full = np.asarray(self._host_rows(data) if isinstance(data, str) else data)
        has_target = full.shape[1] >= I + n_target
        y = np.asarray(full[:, I:I + n_target], dtype=np.float64) if has_target else None
        if cls and has_target:
            labels = y[:, 0]
            bad = np.flatnonzero(~((labels >= 0) & (labels < O) & (labels == np.floor(labels))))
            if bad.size:
                raise ValueError(f"class label {labels[bad[0]]} in row {int(bad[0])} is not an integer in [0, {O})")
        kw, M = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=not cls, count=True)
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.uncertainty(rows, ranks=ranks if cls else (), samples=bool(return_samples) and cls, **kw)
        res = dict.fromkeys(Uncertainty._fields)
        res.update(n_samples=out["n_samples"], n_distinct=out["n_distinct"])
        mean = out["mean"]
        if cls:
            vote = out["vote"]
            # held to log K as the device holds a sample's entropy: fp32 probabilities may sum to a little over 1
            total, alea = np.minimum(entropy(mean), np.log(float(O))), out["entropy_mean"]
            res.update(p_mean=mean, vote=vote, total=total, aleatoric=alea, epistemic=np.maximum(total - alea, 0.0),
                       confidence=np.max(mean, axis=1), variation_ratio=1.0 - np.max(vote, axis=1),
                       disagreement=1.0 - np.sum(vote * vote, axis=1),
                       entropy_percentiles=self._bands(out["entropy_order_stats"], pcts, spots, ranks) if ranks else {},
                       sample_entropy=out["sample_entropy"])
        else:
            ev, av = out["epistemic_var"], out["aleatoric_var"]
            res.update(pred_mean=mean, epistemic_var=ev, aleatoric_var=av, total_var=ev + av, epistemic_share=ev / (ev + av))
        result = Uncertainty(**res)
        if has_target:
            loss = (np.argmax(mean, axis=1) != y[:, 0].astype(np.int64)).astype(np.float64) if cls else np.sum((mean - y) ** 2, axis=1)
            result = result._replace(selective={k: risk_coverage(v, loss) for k, v in uncertainty_scores(result).items()})
        return result
