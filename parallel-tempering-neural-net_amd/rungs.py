"""Every rung of the ladder at once (not in the reference, which discards the tempered chains' draws): the multistate Bennett
acceptance ratio (MBAR; Shirts & Chodera 2008) over the rungs and the prior gives the log evidence with the smallest variance
among estimators that combine the rungs, and a weight for every draw of every rung that turns the pooled tempered sample into a
weighted posterior sample.  The host-only helpers, the result tuple, and the mixin that holds the public method.  The method
checks its arguments here, makes one low-level call of `_lib.Sampler` (the device runs the fixed point, the Gram matrix of the
weights and the resampling) and finishes the result with host arithmetic in float64.
"""
import math
import warnings
from collections import namedtuple

import numpy as np

from .analysis import TASK_REG, evidence_log_c

# rung_reweighting's result.  K' states: the prior first (include_prior), then the K rungs by ascending beta.  log_z_mbar,
# se_log_z_mbar (float; NaN without the prior state); free_energy [K'] (f_k - f_0), betas [K'], theta [K', K'] the covariance of f,
# n_eff [K'] the N_k of the fixed point; n_iter, residual; log_weights [K, n] the log posterior weight of every draw of every rung
# (rungs by ascending beta, draws in trace order; all draws' weights and the prior draws' sum to 1), prior_log_weights [n_prior] or
# None; kish_ess, cold_draws (draws of the rung at T = 1), ess_gain = kish_ess / the ESS of that rung, max_weight_share; with
# resample = m: vectors [m, num_param] float32, eta [m] float32 (regression) or None, index [m, 2] int64 (chain or rung row, step or
# draw; (-1, i) for prior draw i), else None; mean, sd [n_rows, n_out] of the network outputs on the rows x under the weights (x
# given), else None; n_distinct.  ess_gain is NaN where n_eff of the cold rung is no ESS (effective=False, or the fallback 1).
RungWeights = namedtuple("RungWeights", "log_z_mbar se_log_z_mbar free_energy betas theta n_eff n_iter residual log_weights "
                                        "prior_log_weights kish_ess cold_draws ess_gain max_weight_share vectors eta index mean sd n_distinct")


def mbar_covariance(gram, n_eff):
    """The asymptotic covariance of the MBAR free energies (Shirts & Chodera 2008, eq. D8 in its K x K form): Theta = M pinv(I -
    diag(N) M) from the Gram matrix M = W^T diag(c) W [K, K] and the states' draw counts N [K]; var(f_i - f_j) = Theta_ii +
    Theta_jj - 2 Theta_ij.  Host arithmetic only."""
    M, N = np.asarray(gram, np.float64), np.asarray(n_eff, np.float64).reshape(-1)
    if M.ndim != 2 or M.shape != (N.size, N.size):
        raise ValueError(f"gram must be [K, K] with K = {N.size} entries of n_eff, got shape {M.shape}")
    if not (np.all(np.isfinite(M)) and np.all(np.isfinite(N)) and np.all(N > 0)):
        raise ValueError("gram must be finite and n_eff finite and > 0")
    return M @ np.linalg.pinv(np.eye(N.size) - N[:, None] * M, rcond=1e-12)


def mbar_compare(a, b):
    """The log Bayes factor of two RungWeights results, log Z_a - log Z_b, with SE sqrt(se_a^2 + se_b^2) (independent runs; for a
    regression both must be fitted to the same training rows).  -> dict(log_bf_mbar, se_log_bf_mbar)."""
    return dict(log_bf_mbar=float(a.log_z_mbar - b.log_z_mbar), se_log_bf_mbar=math.hypot(a.se_log_z_mbar, b.se_log_z_mbar))


def redraw_eta(sse, n_rows, seed):
    """eta = log tau^2 of weight vectors with sums of squared errors `sse` [m] over n_rows training rows, drawn from its exact
    conditional at beta = 1 under the target of DESIGN.md section 15: with t = exp(-eta), t ~ Gamma(shape n_rows / 2 + 1, rate
    sse / 2).  numpy.random.Generator(Philox(seed)) -> float64 [m]."""
    sse = np.asarray(sse, np.float64).reshape(-1)
    if not np.all(sse > 0):
        raise ValueError("sse must be > 0")
    rng = np.random.Generator(np.random.Philox(int(seed) & 0xFFFFFFFFFFFFFFFF))
    return -np.log(rng.gamma(float(n_rows) / 2.0 + 1.0, 2.0 / sse))


class RungAnalysis:
    """rung_reweighting(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose rung selection (log_evidence's)
    it uses.  It reads the constructor's attributes `seed`, `task`, `traindata` and `_sampler`."""

    def rung_reweighting(self, x=None, *, burn_in=None, thin=1, prior_draws=1 << 20, include_prior=True, effective=True, target_beta=1.0,
                         resample=0, seed=None, weights=None, tol=1e-10, max_iter=10000):
        """Use every rung: the log evidence and a posterior weight for every draw of every rung, by the multistate Bennett
        acceptance ratio (MBAR, binless WHAM) on the GPU.  Rung k samples pi(w) L(w)^beta_k; with U and b of
        log_evidence() the reduced log density of a draw under rung k is b + beta_k U, and 0 under the prior.  One fixed point
        over all draws gives the free energy f_k of every state, log Z = log c - (f_K - f_prior), and the weight of every draw
        under any beta of the ladder.

        The rungs, `burn_in`, `thin` and `weights` = (betas [K], vectors [K, n, num_param]) are log_evidence()'s, with its refusals
        and its warning.  include_prior: `prior_draws` draws of N(0, sigma^2 I) (the same stream as log_evidence) form a state of
        their own; without it only free-energy differences among the rungs are reported and log_z_mbar is NaN.  effective: a
        rung's draws count as its split-ESS of U, not as their number (prior draws are independent).  target_beta in [beta of
        the hottest rung, 1]: the weights' target.  The fixed point stops at `tol` or after `max_iter` sweeps (a warning).

        The weights are weights of w, the network's weight vector; a regression's eta = log tau^2 of a tempered rung is no
        posterior draw given w.  resample = m: m draws by systematic resampling from the weights (Philox stream 7 of `seed`) ->
        vectors [m, num_param], index [m, 2], and for a regression eta [m] redrawn on the host from its exact conditional at
        beta = 1 (redraw_eta).  vectors and eta go into the weights= / eta= arguments of posterior_predictive() and the other
        analysis calls, which then use every rung.  A resampled prior draw's vector is the one the device formed and weighted.

        x ("train", "test" or rows of n_in columns): also mean and sd [n_rows, n_out], the weighted mean and the square root of
        the weighted population variance of the network outputs on those rows over every draw of every rung, without resampling
        noise.  ess_gain = kish_ess / the cold rung's ESS; NaN with effective=False or where that ESS fell back to 1.
        -> RungWeights."""
        self._need_sampler("rung_reweighting")
        xs = None if x is None else self._rows("x", x)
        m = int(resample)
        if m < 0:
            raise ValueError(f"resample = {resample!r} must be >= 0")
        n_prior = int(prior_draws) if include_prior else 0
        if include_prior and n_prior < 2:
            raise ValueError(f"prior_draws = {n_prior}: the prior state needs at least 2 draws")
        if not (float(tol) > 0 and math.isfinite(float(tol))):
            raise ValueError(f"tol = {tol!r} must be a finite number > 0")
        if int(max_iter) < 1:
            raise ValueError(f"max_iter = {max_iter!r} must be >= 1")
        bs, kw, order = self._rung_source("rung_reweighting", burn_in, thin, weights)
        tb = float(target_beta)
        if not (math.isfinite(tb) and bs[0] <= tb <= 1.0):
            raise ValueError(f"target_beta = {target_beta!r} outside [{float(bs[0])!r}, 1]: the ladder covers only these")
        sd = self.seed if seed is None else int(seed)
        out = self._sampler.mbar(bs, n_prior=n_prior, seed=sd, effective=bool(effective), target_beta=tb, tol=float(tol),
                                 max_iter=int(max_iter), n_resample=m, resample_seed=sd, x=xs, resample_w=m > 0, item_map=m > 0,
                                 sse=m > 0 and self.task == TASK_REG, **kw)
        K = bs.size
        k0 = 1 if n_prior > 0 else 0
        f, n_eff = out["f"], out["n_eff"]
        theta = mbar_covariance(out["gram"], n_eff)
        N = int(np.asarray(self.traindata).shape[0])
        log_z = se = float("nan")
        if k0:
            log_z = evidence_log_c(self.task, N) - float(f[-1] - f[0])
            se = math.sqrt(max(float(theta[0, 0] + theta[-1, -1] - 2.0 * theta[0, -1]), 0.0))
        lw = out["log_weight"]
        per = (lw.size - n_prior) // K
        if out["n_iter"] >= int(max_iter) and not out["residual"] <= float(tol):
            warnings.warn(f"rung_reweighting: the fixed point stopped after {out['n_iter']} sweeps with a residual of "
                          f"{out['residual']:.3g} > tol = {float(tol):.3g}: the free energies are not converged (a larger max_iter)",
                          stacklevel=2)
        if out["max_weight_share"] > 0.5 or out["kish_ess"] < 5:
            warnings.warn(f"rung_reweighting: the weighted sample is degenerate (largest share {out['max_weight_share']:.3f}, Kish ESS "
                          f"{out['kish_ess']:.1f}): the rungs' draws hardly cover the target", stacklevel=2)
        vectors = eta = index = None
        if m > 0:
            vectors, eta, index = self._resampled(out, kw, order, sd, N)
        cold = float(n_eff[-1])                              # an ESS only with `effective`, and not where it fell back to 1
        gain = out["kish_ess"] / cold if effective and cold > 1.0 else float("nan")
        mean = sdev = None
        if xs is not None:
            mean, sdev = out["mean"], np.sqrt(out["var"])
        return RungWeights(log_z_mbar=log_z, se_log_z_mbar=se, free_energy=f - f[0], betas=np.concatenate([[0.0], bs]) if k0 else bs,
                           theta=theta, n_eff=n_eff, n_iter=out["n_iter"], residual=out["residual"],
                           log_weights=lw[n_prior:].reshape(K, per), prior_log_weights=lw[:n_prior] if k0 else None,
                           kish_ess=out["kish_ess"], cold_draws=per, ess_gain=gain, max_weight_share=out["max_weight_share"],
                           vectors=vectors, eta=eta, index=index, mean=mean, sd=sdev, n_distinct=out["n_distinct"])

    def _resampled(self, out, kw, order, seed, n_rows):
        """The resampled items of a Sampler.mbar result -> (vectors [m, P] float32 as the device gathered them, eta [m] float32 or
        None, index [m, 2])."""
        item = out["resample_item"]
        index = np.stack([out["item_chain"][item], out["item_step"][item]], axis=1).astype(np.int64)
        if "w" in kw:                                        # the rung's row in `weights` as the caller gave them
            rungs = index[:, 0] >= 0
            index[rungs, 0] = np.asarray(order)[index[rungs, 0]]
        eta = None
        if self.task == TASK_REG:
            eta = redraw_eta(out["sse"][item], n_rows, seed).astype(np.float32)
        return out["resample_w"], eta, index
