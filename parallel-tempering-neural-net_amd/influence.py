"""Case influence of the drop-in (not in the reference, which never asks what a data row does to a prediction): which training
rows drive a prediction, a forecast or a held-out score, to first order, from the samples the device already holds.  The
host-only helpers, the result tuple, and the mixin that holds the public method.  The method checks its arguments here, makes
one low-level call of `_lib.Sampler` (the device forms the covariance matrix over the samples) and finishes the result with
host arithmetic in float64.
"""
from collections import namedtuple

import numpy as np

from . import _lib

TASK_CLS = _lib.TASK_CLS

# case_influence's result: n_x target rows, n_cases case rows, M samples.  `...` stands for the target axes: [n_x, n_out] with
# of="prediction", [n_x] with of="loglik".  cov [..., n_cases] = Cov over the samples of the target with the case's
# log-likelihood (ddof 1), the first-order effect of giving the case more weight; corr = cov / (sd_target sd_case), NaN where
# either sd is 0; deletion_shift = -cov, the first-order change of the target's posterior mean when the case is deleted;
# deletion_z = deletion_shift / target_sd; target_mean, target_sd [...]; case_loglik_mean, case_loglik_var [n_cases] (the
# variance is the case's WAIC penalty); top_cases [..., top] int64, the cases with the largest |cov| of each target column (lowest
# index first on a tie), and top_shift [..., top], their deletion_shift; case_importance [n_cases] = the mean over the target
# columns of |corr|, NaN ignored (NaN where every column is); n_samples; n_distinct.  All float64 but top_cases.
CaseInfluence = namedtuple("CaseInfluence", "cov corr deletion_shift deletion_z target_mean target_sd case_loglik_mean "
                                            "case_loglik_var top_cases top_shift case_importance n_samples n_distinct")


def top_cases(cov, top):
    """The `top` (clipped to n_cases) case indices of every target column by descending |cov|, lowest index first on a tie
    -> (indices [..., top] int64, -cov at them)."""
    cov = np.asarray(cov, dtype=np.float64)
    k = min(int(top), cov.shape[-1])
    order = np.argsort(-np.abs(cov), axis=-1, kind="stable")[..., :k]
    return order.astype(np.int64), 0.0 - np.take_along_axis(cov, order, axis=-1)


def case_importance(corr):
    """The mean over the target columns (every axis but the last) of |corr|, NaN ignored; NaN for a case whose every entry is."""
    a = np.abs(np.asarray(corr, dtype=np.float64)).reshape(-1, np.shape(corr)[-1])
    ok = ~np.isnan(a)
    n = ok.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, np.where(ok, a, 0.0).sum(axis=0) / n, np.nan)


def finish_influence(cov, target_mean, target_var, case_mean, case_var, shape, top, n_samples, n_distinct):
    """The host arithmetic of case_influence: the device's covariance [n_a, n_cases] and moments -> CaseInfluence with the target
    axes `shape`."""
    n_b = cov.shape[1]
    cov = cov.reshape(tuple(shape) + (n_b,))
    t_sd, c_sd = np.sqrt(target_var).reshape(shape), np.sqrt(case_var)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = t_sd[..., None] * c_sd
        corr = np.where(scale > 0.0, cov / scale, np.nan)
        z = np.where(t_sd[..., None] > 0.0, (0.0 - cov) / t_sd[..., None], np.nan)
    idx, shift = top_cases(cov, top)
    return CaseInfluence(cov=cov, corr=corr, deletion_shift=0.0 - cov, deletion_z=z, target_mean=target_mean.reshape(shape), target_sd=t_sd,
                         case_loglik_mean=case_mean, case_loglik_var=case_var, top_cases=idx, top_shift=shift,
                         case_importance=case_importance(corr), n_samples=n_samples, n_distinct=n_distinct)


def influence_flagged(result, z=0.5):
    """The (target column, case) pairs of a CaseInfluence whose deletion would move the target's posterior mean by at least `z`
    of its posterior sd, to first order: -> int64 [n, result.cov.ndim], one row of indices per pair (the target axes, then the
    case), in row-major order."""
    if not z > 0:
        raise ValueError(f"z = {z!r} must be > 0")
    with np.errstate(invalid="ignore"):
        return np.argwhere(np.abs(result.deletion_z) >= z).astype(np.int64)


class InfluenceAnalysis:
    """case_influence(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row and sample-source helpers it
    uses.  It reads the constructor's attributes `task`, `topology` and `_sampler`."""

    def case_influence(self, x="test", cases="train", *, of="prediction", top=5, burn_in=None, chains="all", thin=1, weights=None,
                       eta=None, values=None, loglik=None):
        """Which data rows drive a prediction?  Computed on the GPU from the sampled chains.

        For a posterior p(theta) ~ prior x prod_i p(y_i | theta)^{w_i}, the derivative of a posterior mean E[g] by the weight w_i
        of case i, at w = 1, is Cov(g, l_i) over the posterior, l_i = log p(y_i | x_i, theta).  cov[j, i] is that covariance over
        the selected samples of target j with case i; deletion_shift = -cov says what deleting the case would do to the
        target's posterior mean, deletion_z the same in posterior sds of the target, corr the correlation.  This is first-order:
        exact only in the limit of small changes of a case's weight.  Deleting a case outright adds a second-order term that grows
        with the case's leverage, so a large deletion_z ranks and flags a case; it is not the refitted value.

        `of`: "prediction" -- the targets are the network outputs on the rows `x` ("train", "test" or rows of n_in columns);
        "loglik" -- the targets are the log-likelihoods of the rows `x` (n_in inputs and the target), so cov says which cases
        help (positive) or hurt a held-out row's log score; with x = cases the diagonal is case_loglik_var, the WAIC penalty
        predictive_accuracy() reports.  `cases`: "train", "test" or rows of n_in inputs and the target.  `top`: how many cases to
        list per target column (clipped to the number of cases).

        Samples, `chains`, `thin` and `weights` (with `eta` for a regression) as predictive_calibration().  chains="cold" is the
        posterior's own figure; the default chains="all" pools the tempered rungs, like every other call.  `values` [n, n_a] with
        `loglik` [n, n_cases] (or a pair with integer multiplicities [n]) take the place of the samples and the forward pass:
        the covariance of given columns, cov [n_a, n_cases].
        -> CaseInfluence."""
        self._need_sampler("case_influence")
        if of not in ("prediction", "loglik"):
            raise ValueError(f"of = {of!r} must be 'prediction' or 'loglik'")
        k = int(top)
        if k != top or k < 1:
            raise ValueError(f"top = {top!r} must be an integer >= 1")
        cls = self.task == TASK_CLS
        if values is not None or loglik is not None:
            if values is None or loglik is None:
                raise ValueError("values= and loglik= come together: the target columns and the cases' log-likelihoods of the same samples")
            if weights is not None:
                raise ValueError("values= and loglik= take the place of the samples: no weights= with them")
            mult = None
            if isinstance(loglik, tuple):
                loglik, mult = loglik
            va, la = np.asarray(values, dtype=np.float32), np.asarray(loglik, dtype=np.float64)
            if va.ndim != 2 or la.ndim != 2 or va.shape[0] != la.shape[0] or va.shape[1] < 1 or la.shape[1] < 1:
                raise ValueError(f"values must be [n_samples, n_a] and loglik [n_samples, n_cases], got shapes {va.shape} and {la.shape}")
            M = va.shape[0] if mult is None else int(np.sum(np.maximum(np.asarray(mult, dtype=np.int64), 0)))
            if M < 2:
                raise ValueError(f"the selection holds {M} samples: a covariance needs at least 2")
            if not np.all(np.isfinite(la)):
                s, i = (int(v[0]) for v in np.nonzero(~np.isfinite(la)))
                raise ValueError(f"loglik[{s}, {i}] = {la[s, i]} is not finite")
            shape = (va.shape[1],)
            out = self._sampler.influence(values=va, loglik=la, multiplicity=mult)
        else:
            xs = self._rows("x", x, target=of == "loglik")
            cs = self._rows("cases", cases, target=True)
            kw, M = self._sample_source(weights, burn_in, chains, thin, eta=eta, need_eta=not cls, count=True)
            if M < 2:
                raise ValueError(f"the selection holds {M} samples: a covariance needs at least 2")
            n_x = len(self._host_rows(xs))
            shape = (n_x, int(self.topology[2])) if of == "prediction" else (n_x,)
            out = self._sampler.influence(xs, cs, of=of, **kw)
        return finish_influence(out["cov"], out["target_mean"], out["target_var"], out["case_mean"], out["case_var"], shape, k,
                                out["n_samples"], out["n_distinct"])
