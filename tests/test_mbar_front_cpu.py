"""The Python front of rung_reweighting (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its recording
stand-in for `_lib.Sampler`, taught the one call more (it answers with tests/mbar_ref.py on canned U): the keywords the sampler
receives, what comes back, the warnings, every refusal before the device is asked for anything, and the object states."""
import math
import warnings

import numpy as np
import pytest

import mbar_ref as ref
import test_analysis_front_cpu as front
from test_analysis_front_cpu import BETAS, STATES, WK, fill

from ptnn_amd import philox, rungs  # noqa: E402


class MbarStandIn(front.StandIn):
    def traces(self, step0=0, nsteps=None):
        n = self.S - step0 if nsteps is None else nsteps
        return dict(pos_w=fill((self.R, self.S, self.P), 31, -1, 1, np.float32)[:, step0:step0 + n])

    def mbar(self, *args, **kw):
        self._log("mbar", args, kw)
        betas = np.asarray(args[0], np.float64)
        K, n_prior = betas.size, kw["n_prior"]
        per = np.asarray(kw["w"]).shape[1] if kw.get("w") is not None else self._count(kw) // K
        u = np.concatenate([fill(n_prior, 1, -9, -5) * 2.0, (fill((K, per), 2, -3, -1) * 2.0).reshape(-1)])
        b = u / 15.0 if self.task == front._lib.TASK_REG else np.zeros(u.size)
        c = np.concatenate([np.ones(n_prior), np.full(K * per, 0.5 if kw["effective"] else 1.0)])
        k0 = 1 if n_prior else 0
        bs, g = np.concatenate([np.zeros(k0), betas]), np.concatenate([np.zeros(k0), np.ones(K)])
        n_k = np.concatenate([np.full(k0, float(n_prior)), np.full(K, per * (0.5 if kw["effective"] else 1.0))])
        f, D, n_iter, resid = ref.solve(u, b, c, bs, g, n_k, tol=kw["tol"], max_iter=kw["max_iter"])
        lw = ref.target_log_weights(u, b, c, D, kw["target_beta"])
        s, kish, share = (1.0, 1.2, 0.9) if self.mode == "degenerate" else ref.weight_stats(lw, c)   # degenerate: one draw outweighs the rest
        m = kw["n_resample"]
        cum = np.cumsum(np.exp(lw))
        uu = philox.resample_uniform(kw["resample_seed"])
        item = ref.systematic_resample(cum, uu, m) if m else None
        vec = None
        if kw["resample_w"]:                                            # the vectors a device would gather
            vec = np.empty((m, self.P), np.float32)
            for i, it in enumerate(item):
                if it < n_prior:
                    vec[i] = philox.normals(self.P, int(it), 0, philox.STREAM_PRIOR, kw["seed"]).astype(np.float32) * np.float32(5.0)
                elif kw.get("w") is not None:
                    vec[i] = np.asarray(kw["w"], np.float32)[(it - n_prior) // per, (it - n_prior) % per]
                else:
                    vec[i] = self.traces()["pos_w"][kw["replicas"][(it - n_prior) // per], kw["step0"] + (it - n_prior) % per * kw["thin"]]
        chain = step = None
        if kw["item_map"]:
            rows = np.arange(K * per)
            host = kw.get("w") is not None
            chain = np.concatenate([np.full(n_prior, -1), rows // per if host else np.asarray(kw["replicas"])[rows // per]]).astype(np.int32)
            step = np.concatenate([np.arange(n_prior), rows % per if host else kw["step0"] + rows % per * kw["thin"]]).astype(np.int64)
        mean = var = None
        if kw["x"] is not None:
            mean, var = ref.weighted_moments(outputs(u.size, self._n_rows(kw["x"]), self.O), lw)
        return dict(f=f, gram=ref.gram(ref.weight_matrix(u, b, bs, g, f, D), c), n_eff=n_k, log_weight=lw, item_chain=chain,
                    item_step=step, sse=np.exp(-b) if kw["sse"] else None, cum_weight=cum if m else None, resample_item=item, resample_w=vec, mean=mean, var=var,
                    residual=resid, weight_sum=s, kish_ess=kish, max_weight_share=share, resample_u=uu if m else 0.0, n_iter=n_iter,
                    n_items=u.size, n_distinct=K * per)


def outputs(n_items, n_rows, O):
    """The network outputs the stand-in ascribes to the items on the rows x."""
    return fill((n_items, n_rows, O), 41, 0.1, 0.9)


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(MbarStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.rung_reweighting(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=text):
            make(key, calls).rung_reweighting(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def test_trace_source_and_result():
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # exact settings: no warning
        pt, calls, rw = run("reg_exact", prior_draws=64, resample=10, seed=5)
    (tag, fn, args, got), = calls
    bs = np.sort(1.0 / np.asarray(pt.temperatures, np.float32).astype(np.float64))
    assert fn == "mbar" and args == front.enc([bs])
    # temperatures [2, 1, 4, 1.5]: chains by ascending beta; rows 10 .. 23 (the switch at 0.6 NumSamples)
    assert got == front.enc(dict(n_prior=64, seed=5, effective=True, target_beta=1.0, tol=1e-10, max_iter=10000, n_resample=10,
                                 resample_seed=5, x=None, resample_w=True, item_map=True, sse=True, replicas=[2, 0, 3, 1], step0=10, nsteps=14, thin=1))
    assert rw.betas.tolist() == [0.0] + bs.tolist() and rw.free_energy[0] == 0.0 and rw.free_energy.shape == (5,)
    N = len(pt.traindata)
    log_c = math.log(2.0) + math.lgamma(N / 2 + 1) - N / 2 * math.log(math.pi)
    assert rw.log_z_mbar == pytest.approx(log_c - rw.free_energy[-1], rel=1e-14)
    assert np.array_equal(rw.theta, rungs.mbar_covariance(ref.gram(*_w_and_c(pt, calls)), rw.n_eff))
    assert rw.se_log_z_mbar == math.sqrt(rw.theta[0, 0] + rw.theta[-1, -1] - 2 * rw.theta[0, -1]) > 0
    assert rw.log_weights.shape == (4, 14) and rw.prior_log_weights.shape == (64,) and rw.cold_draws == 14
    assert np.exp(rw.log_weights).sum() + np.exp(rw.prior_log_weights).sum() == pytest.approx(1.0, abs=1e-12)
    assert rw.ess_gain == rw.kish_ess / rw.n_eff[-1] > 0 and rw.n_iter % 8 == 0 and rw.residual <= 1e-10
    # the resampled draws: rows of the trace by (chain, step), a prior draw by (-1, draw); eta from the Gamma conditional of its SSE
    assert rw.vectors.shape == (10, pt.num_param) and rw.vectors.dtype == np.float32 and rw.index.shape == (10, 2)
    pos = pt._sampler.traces()["pos_w"]
    for v, (chain, step) in zip(rw.vectors, rw.index):
        want = pos[chain, step] if chain >= 0 else philox.normals(pt.num_param, step, 0, philox.STREAM_PRIOR, 5).astype(np.float32) * np.float32(5.0)
        assert np.array_equal(v, want)
    assert rw.eta.shape == (10,) and rw.eta.dtype == np.float32 and np.all(np.isfinite(rw.eta))
    assert rw.mean is None and rw.sd is None
    # rows x: the weighted mean and sd of the outputs over every item, the rows as posterior_predictive passes them
    pt, calls, rx = run("reg_exact", "test", prior_draws=64)
    assert calls[0][3] == front.enc(dict(n_prior=64, seed=11, effective=True, target_beta=1.0, tol=1e-10, max_iter=10000, n_resample=0,
                                         resample_seed=11, x="test", resample_w=False, item_map=False, sse=False, replicas=[2, 0, 3, 1], step0=10, nsteps=14,
                                         thin=1))
    lw = np.concatenate([rx.prior_log_weights, rx.log_weights.reshape(-1)])
    mean, var = ref.weighted_moments(outputs(lw.size, len(pt.testdata), 1), lw)
    assert np.array_equal(rx.mean, mean) and np.array_equal(rx.sd, np.sqrt(var)) and rx.mean.shape == (len(pt.testdata), 1)
    _, calls, rx = run("reg_exact", front.REG_ROWS, prior_draws=64)
    assert calls[0][3]["d"][-1] == ["'x'", front.enc(np.ascontiguousarray(front.REG_ROWS[:, :4], dtype=np.float32))] and rx.mean.shape == (12, 1)
    # ess_gain has a meaning only against an ESS
    assert math.isnan(run("reg_exact", prior_draws=64, effective=False)[2].ess_gain)


def _w_and_c(pt, calls):
    """W and c of the stand-in's answer to the one recorded call, rebuilt."""
    K, per, n_prior = 4, 14, 64
    u = np.concatenate([fill(n_prior, 1, -9, -5) * 2.0, (fill((K, per), 2, -3, -1) * 2.0).reshape(-1)])
    b, c = u / 15.0, np.concatenate([np.ones(n_prior), np.full(K * per, 0.5)])
    bs = np.concatenate([[0.0], np.sort(1.0 / np.asarray(pt.temperatures, np.float32).astype(np.float64))])
    g, n_k = np.concatenate([[0.0], np.ones(K)]), np.concatenate([[64.0], np.full(K, 7.0)])
    f, D, _, _ = ref.solve(u, b, c, bs, g, n_k)
    return ref.weight_matrix(u, b, bs, g, f, D), c


@pytest.mark.filterwarnings("ignore:rung_reweighting. the tempered chains:UserWarning")     # cls_exact keeps its Langevin proposals
def test_weights_source_options_and_warnings():
    pt, calls, rw = run("cls_exact", weights=(BETAS, WK[:, :, :1].repeat(51, axis=2)), include_prior=False, effective=False,
                        target_beta=0.5, tol=1e-6, max_iter=64)
    (_, fn, args, got), = calls
    assert args == front.enc([np.array([0.25, 0.5, 1.0])])
    assert got == front.enc(dict(n_prior=0, seed=11, effective=False, target_beta=0.5, tol=1e-6, max_iter=64, n_resample=0, resample_seed=11,
                                 x=None, resample_w=False, item_map=False, sse=False, w=np.asarray(WK[:, :, :1].repeat(51, axis=2))[[0, 2, 1]]))
    assert math.isnan(rw.log_z_mbar) and math.isnan(rw.se_log_z_mbar) and rw.prior_log_weights is None
    assert rw.betas.tolist() == [0.25, 0.5, 1.0] and rw.log_weights.shape == (3, 6) and rw.vectors is None and rw.eta is None and rw.index is None
    # the index of a resample from weights= names (row of weights, draw)
    pt, calls, rw = run("cls_exact", weights=(BETAS, WK[:, :, :1].repeat(51, axis=2)), include_prior=False, resample=5)
    assert set(rw.index[:, 0].tolist()) <= {0, 1, 2} and rw.eta is None
    for v, (row, draw) in zip(rw.vectors, rw.index):
        assert np.array_equal(v, WK[row, draw, :1].repeat(51).astype(np.float32))
    # the drop-in's defaults: log_evidence's warning under this method's name
    with pytest.warns(UserWarning, match="rung_reweighting: the tempered chains do not sample the power posterior exactly"):
        run("reg", prior_draws=16)
    with pytest.warns(UserWarning, match="stopped after 8 sweeps"):
        run("reg_exact", prior_draws=16, max_iter=1, tol=1e-300)
    with pytest.warns(UserWarning, match="the weighted sample is degenerate"):
        run("reg_degenerate", prior_draws=16)


FAULTS = [
    ("x_unknown_name", dict(x="valid"), "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_too_few_columns", dict(x=front.BAD_ROWS), "at least n_in = 4 columns"),
    ("x_and_resample_negative", dict(x="valid", resample=-1), "x must be"),
    ("resample_negative", dict(resample=-1), "resample = -1 must be >= 0"),
    ("prior_draws_one", dict(prior_draws=1), "prior_draws = 1: the prior state needs at least 2 draws"),
    ("tol_zero", dict(tol=0), "tol = 0 must be a finite number > 0"),
    ("max_iter_zero", dict(max_iter=0), "max_iter = 0 must be >= 1"),
    ("target_beta_above_one", dict(target_beta=1.5), r"target_beta = 1.5 outside \[0.25, 1\]"),
    ("target_beta_below_the_ladder", dict(target_beta=0.1), "target_beta = 0.1 outside"),
    ("target_beta_nan", dict(target_beta=float("nan")), "target_beta = nan outside"),
    ("too_few_draws", dict(burn_in=0.55), "at least 4 are needed"),
    ("weights_not_a_pair", dict(weights=WK), "weights must be a pair"),
    ("weights_wrong_shape", dict(weights=(BETAS, WK[:, :, :5])), "vectors must be"),
    ("weights_too_few_draws", dict(weights=(BETAS, WK[:, :3])), "the split ESS needs at least 4"),
    ("weights_duplicate", dict(weights=([0.5, 1.0, 0.5], WK)), "duplicate temperatures"),
    ("weights_no_cold_rung", dict(weights=([0.25, 0.5, 0.75], WK)), "needs a rung at temperature 1"),
    # the order of the checks
    ("resample_negative_and_tol", dict(resample=-1, tol=0), "resample = -1"),
    ("tol_and_too_few_draws", dict(tol=0, burn_in=0.55), "tol = 0"),
    ("too_few_draws_and_target", dict(burn_in=0.55, target_beta=2), "at least 4 are needed"),
]


@pytest.mark.parametrize("name, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, kw, text):
    refused("reg", text, **kw)


def test_ladder_refusals():
    refused("reg_dup", "duplicate temperatures")
    refused("reg_hot", "needs a rung at temperature 1")


STATE_TEXT = {"none": "rung_reweighting needs the chains' device handle", "sharded": "rung_reweighting runs on one GPU",
              "label": "label_swap=True", "cap": "trace_capacity = 5 < NumSamples = 40", "unfinished": "no finished run_chains"}


@pytest.mark.parametrize("state", STATES)
def test_object_states(state):
    refused(f"reg_{state}", STATE_TEXT[state])
    # the handle comes first, before the arguments; the trace's state after them
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "resample = -1", resample=-1)
    if state in ("none", "sharded"):
        refused(f"reg_{state}", STATE_TEXT[state], weights=(BETAS, WK))
    else:                                                               # weights= needs no finished trace
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, calls, rw = run(f"reg_{state}", weights=(BETAS, WK), prior_draws=16)
        assert len(calls) == 1 and rw.log_weights.shape == (3, 6)
