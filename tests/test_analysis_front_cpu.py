"""The Python front of the ten posterior analysis calls, characterised (no GPU): what each public method refuses and in which
order, which low-level `Sampler` call it makes with which arguments, what it warns about and from which frame, and what it
returns.  The two drop-in classes are built on small arrays (their constructor does not touch the device) and given a stand-in
for `_lib.Sampler` that records every call -- arrays as dtype, shape, C-contiguity and SHA-256 -- and answers with canned
outputs of the right shapes.  CASES names, per method, valid calls over every sample source and rows argument, every single
fault the method refuses, pairs of simultaneous faults for every adjacent pair of checks (the order of the checks decides which
one is reported), and the object states (no handle, a sharded ladder, label_swap, a streamed trace, an unfinished run).

The expected values are tests/golden/analysis_front.json, with the SHA-256 of the ten docstrings.  The file is recorded from the
commit BEFORE a change to these methods, never from the code under test:

    python tests/test_analysis_front_cpu.py --record

test_every_refusal_site_is_reached counts the `raise` and `warnings.warn` statements of the class that holds the methods and
asserts that the cases reach every one of them.
"""
import ast
import hashlib
import inspect
import json
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "analysis_front.json")
sys.path.insert(0, ROOT)
import ptnn_amd  # noqa: E402,F401
from ptnn_amd import _lib, parallel_tempering as pt_module  # noqa: E402
from ptnn_amd import pt_classification, pt_timeseries_regression  # noqa: E402

METHODS = ("posterior_predictive", "input_sensitivity", "convergence_diagnostics", "predictive_accuracy", "leave_future_out",
           "predictive_calibration", "predictive_check", "powerscale_sensitivity", "forecast", "log_evidence")
# methods of the sampler driver with refusals of their own: they count only while the driver and the analysis methods share a class
DRIVER_FUNCS = ("__init__", "set_initial_weights", "_ladder_adapt_spec", "_configure", "run_chains", "_finish_run",
                "_likelihood_rows", "ladder_diagnostics")
UNREACHED_ON_CPU = {}                                    # {"function: text of the line": reason}; none


def fill(shape, salt=0, lo=0.0, hi=1.0, dtype=np.float64):
    """A fixed array of `shape` with values in [lo, hi): integer arithmetic and one division, the same on every machine."""
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    v = ((np.arange(int(np.prod(shape)), dtype=np.int64) * 7919 + salt * 104729) % 1013) / 1013.0
    return (lo + (hi - lo) * v).reshape(shape).astype(dtype)


def table(n, salt, labels=0, extra=0):
    a = fill((n, 5 + extra), salt)
    if labels:
        a[:, 4] = (np.arange(n) * 5 + salt) % labels
    return a


REG_TOPO, CLS_TOPO, REG_P, CLS_P = [4, 5, 1], [4, 6, 3], 31, 51
REG_ROWS, CLS_ROWS = table(12, 5, extra=2), table(12, 6, labels=3, extra=2)       # an array with extra columns
W, WC = fill((6, REG_P), 7, -1, 1), fill((6, CLS_P), 8, -1, 1)
MULT, ETA = [1, 2, 0, 3, 1, 1], fill(6, 9, -3, -1)
LOGLIK = fill((8, 12), 10, -4, -1)
BETAS = [0.25, 1.0, 0.5]
WK = fill((3, 6, REG_P), 11, -1, 1)


# ---- the stand-in for _lib.Sampler: records its calls, returns canned outputs ----
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def enc(v):
    """A value as JSON: an array as dtype, shape, C-contiguity and SHA-256; a float by its repr (nan compares equal)."""
    if isinstance(v, np.ndarray):
        return {"nd": [str(v.dtype), list(v.shape), bool(v.flags.c_contiguous), sha(v)]}
    if isinstance(v, np.generic):
        return {"np": [str(v.dtype), repr(v.item())]}
    if v is None or isinstance(v, (bool, str, int)):
        return v
    if isinstance(v, float):
        return {"f": repr(v)}
    if isinstance(v, tuple):
        return {"t": [enc(x) for x in v]}
    if isinstance(v, (list, range)):
        return [enc(x) for x in v]
    if isinstance(v, dict):
        return {"d": sorted([repr(k), enc(x)] for k, x in v.items())}
    raise TypeError(f"cannot record a {type(v).__name__}")


def digest(v):
    return hashlib.sha256(json.dumps(enc(v), sort_keys=True).encode()).hexdigest()[:16]


class StandIn(_lib.Sampler):
    """A `_lib.Sampler` with no handle and no library: made with object.__new__, see stand_in()."""

    def close(self):
        pass

    def _log(self, name, args, kw):
        self.calls.append([self.tag, name, enc(list(args)), enc(kw)])

    def _count(self, kw):
        if kw.get("w") is not None:
            m = kw.get("multiplicity")
            return np.asarray(kw["w"]).shape[0] if m is None else int(np.maximum(np.asarray(m), 0).sum())
        reps, step0 = kw.get("replicas"), kw.get("step0", 0)
        nsteps = self.S - step0 if kw.get("nsteps") is None else kw["nsteps"]
        return (self.R if reps is None else len(reps)) * max(0, -(-nsteps // max(1, kw.get("thin", 1))))

    def _n_rows(self, x):
        return {"train": self.ntr, "test": self.nte}[x] if isinstance(x, str) else np.asarray(x).shape[0]

    def predict(self, *args, **kw):
        self._log("predict", args, kw)
        n, O, M, k = self._n_rows(args[0]), self.O, self._count(kw), len(kw["ranks"])
        return dict(mean=fill((n, O), 1), order_stats=fill((k, n, O), 2, dtype=np.float32) if k else None,
                    vote=fill((n, O), 3) if kw["vote"] else None, samples=fill((M, n, O), 4, dtype=np.float32) if kw["samples"] else None,
                    n_samples=M, n_distinct=max(M - 1, 0))

    def sensitivity(self, *args, **kw):
        self._log("sensitivity", args, kw)
        n, O, I, M, k = self._n_rows(args[0]), self.O, self.I, self._count(kw), len(kw["ranks"])
        sa = np.repeat(fill((-(-M // 2), O, I), 5, dtype=np.float32), 2, axis=0)[:M]      # runs of equal rows: repeated samples
        return dict(grad_mean=fill((n, O, I), 1, -1, 1), order_stats=fill((k, n, O, I), 2, dtype=np.float32) if k else None,
                    pos_count=fill((n, O, I), 3, 0, M, np.int64), neg_count=fill((n, O, I), 4, 0, M, np.int64),
                    abs_mean=fill((O, I), 6), sq_mean=fill((O, I), 7), abs_order_stats=fill((k, O, I), 8, dtype=np.float32) if k else None,
                    sample_abs=sa, samples=fill((M, n, O, I), 9, dtype=np.float32) if kw["samples"] else None, n_samples=M,
                    n_distinct=-(-M // 2))

    def convergence(self, *args, **kw):
        self._log("convergence", args, kw)
        if kw.get("draws") is not None:
            nc, nd, Q = np.asarray(kw["draws"]).shape
        else:
            nc = self.R if kw["replicas"] is None else len(kw["replicas"])
            nd = self._count(kw) // nc
            Q = (self.P if kw["params"] is None else len(kw["params"])) + len(kw["scalars"])
        ess = fill(Q, 3, 1, 50)
        ess[::4] = np.nan                                                            # a constant quantity has no ESS
        return dict(mean=fill(Q, 1), var=fill(Q, 2), r_hat=fill(Q, 4, 1, 1.2), ess=ess, trunc_lag=fill(Q, 5, 0, 9, np.int32),
                    ess_chain=fill((nc, Q), 6, 1, 50) if kw["per_chain"] else None,
                    rho=fill((kw["n_lags"], Q), 7, -1, 1) if kw["n_lags"] else None, n_chains=int(nc), n_draws=int(nd))

    def elpd(self, *args, **kw):
        self._log("elpd", args, kw)
        if kw.get("loglik") is not None:
            M, n = kw["loglik"].shape
            if kw.get("multiplicity") is not None:
                M = int(np.sum(kw["multiplicity"]))
        else:
            M, n = self._count(kw), self._n_rows(args[0])
        khat = fill(n, 4, -0.2, 1.0 if self.mode != "calm" else 0.3)
        khat[0] = np.inf
        return dict(lppd=fill(n, 1, -2, 0), p_waic=fill(n, 2, 0, 0.3), elpd_loo=fill(n, 3, -2.5, 0), khat=khat,
                    tail_len=fill(n, 5, 5, 20, np.int64), loglik=fill((M, n), 6, -4, -1) if kw["loglik_out"] else None, n_samples=M,
                    n_distinct=max(M - 2, 1))

    def lfo(self, *args, **kw):
        self._log("lfo", args, kw)
        n, M = len(kw["origins"]), self._count(kw)
        return dict(elpd_lfo=fill(n, 1 + kw["n_fit"], -2, 0), khat=fill(n, 2 + kw["n_fit"], 0.0, 1.2 if self.mode != "calm" else 0.3),
                    tail_len=fill(n, 3, 5, 20, np.int64), loglik=None, n_samples=M, n_distinct=M)

    def calibration(self, *args, **kw):
        self._log("calibration", args, kw)
        n, M, q = self._n_rows(args[0]), self._count(kw), len(kw["quantiles"])
        out = dict(pit=None, crps=None, pred_mean=None, pred_sd=None, quantiles=None, p_mean=None, n_samples=M, n_distinct=M)
        if self.task == _lib.TASK_REG:
            out.update(pit=fill(n, 1), pred_mean=fill(n, 2), pred_sd=fill(n, 3, 0.1, 0.5), crps=fill(n, 4) if kw["crps"] else None,
                       quantiles=np.sort(fill((q, n), 5), axis=0) if q else None)
        else:
            p = fill((n, self.O), 6, 0.1, 1.0)
            out.update(p_mean=p / p.sum(axis=1, keepdims=True))
        return out

    def ppc(self, *args, **kw):
        self._log("ppc", args, kw)
        M = self._count(kw)
        ns = 7 + len(kw["lags"]) if self.task == _lib.TASK_REG else 2 + self.O
        nd = fill(ns, 1, 0, M + 1, np.int64)
        nd[-1] = 0                                                                   # a statistic that is nowhere defined: p = nan
        ng = nd // 2
        return dict(n_defined=nd, n_greater=ng, n_equal=(nd - ng) // 3, mean_obs=fill(ns, 2), mean_rep=fill(ns, 3), var_rep=fill(ns, 4),
                    t_obs=fill((M, ns), 5) if kw["samples"] else None, t_rep=fill((M, ns), 6) if kw["samples"] else None, n_samples=M,
                    n_distinct=M)

    def powerscale(self, *args, **kw):
        self._log("powerscale", args, kw)
        g, M = kw["groups"], self._count(kw)
        Q = ((self.P if "weights" in g else 0) + ("eta" in g) + (self._n_rows(args[0]) * self.O if "predictions" in g else 0)
             + ("loglik" in g))
        bsd = fill(Q, 5, 0.1, 1)
        bsd[0] = 0.0                                                                 # a constant quantity: the ratios are inf / nan
        return dict(sens=fill((2, Q), 1, 0, 0.1), mean=fill((2, 2, Q), 2), sd=fill((2, 2, Q), 3, 0.1, 1), base_mean=fill(Q, 4),
                    base_sd=bsd, khat=fill((2, 2), 6, 0.3, 1.1 if self.mode != "calm" else 0.5), n_samples=M, n_distinct=M)

    def forecast(self, *args, **kw):
        self._log("forecast", args, kw)
        hz, n, M, k = args[0], self._n_rows(args[1]), self._count(kw), len(kw["ranks"])
        return dict(mean=fill((n, hz), 1), order_stats=fill((k, n, hz), 2, dtype=np.float32) if k else None,
                    samples=fill((M, n, hz), 3, dtype=np.float32) if kw["samples"] else None, n_samples=M, n_trajectories=M)

    def evidence(self, *args, **kw):
        self._log("evidence", args, kw)
        K, n_prior, b0 = len(kw["d"]), kw["n_prior"], kw["a"][1]
        per = np.asarray(kw["w"]).shape[1] if kw.get("w") is not None else self._count(kw) // K
        out = dict(u_mean=np.sort(fill(K, 1, -40, -20)), u_var=fill(K, 2, 1, 4), u_ess=fill(K, 3, 2, per), log_stone=fill(K, 4, -9, -3),
                   stone_relvar=fill(K, 5, 0, 2), n_draws=np.full(K, per, np.int64), prior_log_mean_exp=fill(2, 6, -50, -40),
                   prior_kish_ess=np.array([0.5, 0.001 if self.mode == "low_kish" else 0.4]) * n_prior, prior_u_mean=fill(2, 7, -60, -50),
                   prior_u_var=fill(2, 8, 1, 9), u=fill(K * per, 9, -60, -20) if kw["u_out"] else None,
                   u_prior=fill(n_prior, 10, -90, -50) if kw["u_prior_out"] else None, n_distinct=K * per)
        if self.mode == "agree":                                                     # U = -3 everywhere: both estimates are -3
            out.update(u_mean=np.full(K, -3.0), u_var=np.zeros(K), log_stone=-3.0 * np.asarray(kw["d"]), stone_relvar=np.zeros(K),
                       prior_log_mean_exp=np.array([0.0, -3.0 * b0]), prior_u_mean=np.full(2, -3.0), prior_u_var=np.zeros(2))
        return out


def stand_in(pt, calls, tag, mode):
    s = object.__new__(StandIn)
    s.calls, s.tag, s.mode, s.task = calls, tag, mode, pt.task
    s.I, _, s.O = (int(v) for v in pt.topology)
    s.P, s.R, s.S, s.ntr, s.nte = pt.num_param, pt.num_chains, pt.NumSamples, len(pt.traindata), len(pt.testdata)
    return s


# ---- the objects: "<task>[_<state or mode>]" ----
def make(key, calls, tag="self", train=None):
    """The object of a case: reg / cls (a finished run with a stand-in sampler), or one of those in another state."""
    task, _, state = key.partition("_")
    kw = dict(seed=11, write_files=False)
    if state == "label":
        kw.update(label_swap=True)
    elif state.startswith("cap"):                                                    # cap_unfinished: two states at once
        kw.update(trace_capacity=5)
    elif state in ("exact", "adapt"):
        kw.update(swap_rule=1, shared_noise=False, adapt_ladder=state == "adapt")
    if task == "cls":
        pt = pt_classification.ParallelTempering(True, 0.01, table(30, 3, labels=3) if train is None else train, table(20, 4, labels=3),
                                                 CLS_TOPO, 4, 4.0, 160, 5, "unused", **kw)
    else:
        pt = pt_timeseries_regression.ParallelTempering(state != "exact", 0.01, table(30, 1) if train is None else train, table(20, 2),
                                                        [4, 5, 2] if state == "twoout" else REG_TOPO, 4, 4.0, 160, 5, 0.5, "unused", **kw)
    assert pt.NumSamples == 40
    pt.burn_in = 0.5 if state == "adapt" else 0.25
    pt.temperatures = {"dup": [1.0, 2.0, 2.0, 4.0], "hot": [1.5, 2.0, 3.0, 4.0]}.get(state, [2.0, 1.0, 4.0, 1.5])
    pt._finished = "unfinished" not in state
    pt._sampler = None if state == "none" else object() if state == "sharded" else stand_in(pt, calls, tag, state)
    return pt


class Refit:
    """leave_future_out's refit=callable: a second object with a stand-in of its own, fitted to the rows it is given."""

    def __init__(self, key):
        self.key = key

    def bind(self, calls):
        return lambda rows: (calls.append(["refit", "rows", enc(rows)]), make(self.key, calls, f"refit{len(rows)}", train=rows))[1]


STATES = ("none", "sharded", "label", "cap", "unfinished")
BAD_ROWS = fill((5, 3), 1)                                                           # too few columns for every rows argument
TRACE_FAULTS = [("chains_out_of_range", dict(chains=[0, 4])), ("chains_negative", dict(chains=[-1])), ("chains_empty", dict(chains=[]))]
BAD_W = [("weights_wrong_width", dict(weights=fill((6, 30), 1))), ("weights_1d", dict(weights=fill(REG_P, 1)))]
MANY_PCTS = [3 + 5.5 * k for k in range(17)]                                         # more order statistics than one call takes


def c(name, obj, *args, **kw):
    return (name, obj, args, kw)


def sources(obj, w, *args, eta=None, **kw):
    """Valid calls over every sample source: the trace selections and the three forms of weights= (a classification: one each)."""
    e = {} if eta is None else dict(eta=eta)
    if obj == "cls":
        return [c("cls_trace_list_burn_in", obj, *args, chains=[2, 0], burn_in=0.5, thin=2, **kw),
                c("cls_weights_multiplicities", obj, *args, weights=(w, MULT), **e, **kw)]
    return [c("trace_all", obj, *args, **kw), c("trace_cold_thin", obj, *args, chains="cold", thin=3, **kw),
            c("trace_list_burn_in", obj, *args, chains=[2, 0], burn_in=0.5, thin=2, **kw),
            c("trace_burn_in_zero", obj, *args, burn_in=0, **kw),
            c("weights_vectors", obj, *args, weights=w, **e, **kw), c("weights_transposed", obj, *args, weights=w.T, **e, **kw),
            c("weights_multiplicities", obj, *args, weights=(w, MULT), **e, **kw)]


def states(obj_task, *args, **kw):
    return [c(f"state_{s}", f"{obj_task}_{s}", *args, **kw) for s in STATES]


def late(method_kw, fault_name, fault):
    """The three methods that look at the handle late: every state alone, with weights, and paired with a data fault."""
    return (states("reg") + [c(f"state_{s}_with_weights", f"reg_{s}", weights=W, eta=ETA, **method_kw) for s in STATES]
            + [c(f"state_{s}_and_{fault_name}", f"reg_{s}", **fault) for s in STATES]
            + [c(f"state_{s}_and_weights_without_eta", f"reg_{s}", weights=W) for s in ("none", "sharded")])


CASES = {
    "posterior_predictive": [
        *sources("reg", W), *sources("cls", WC, "train"),
        c("train", "reg", "train"), c("rows_with_extra_columns", "reg", REG_ROWS), c("rows_float32_exact_width", "reg", fill((7, 4), 3, dtype=np.float32)),
        c("return_samples", "cls", return_samples=True), c("percentiles_none", "reg", percentiles=()),
        c("percentiles_ends", "reg", percentiles=[0, 50, 100, 12.5]),
        *states("reg"), c("state_label_with_weights", "reg_label", weights=W), c("state_unfinished_with_weights", "reg_unfinished", weights=W),
        c("x_unknown_name", "reg", "valid"), c("x_1d", "reg", fill(4, 1)), c("x_too_few_columns", "reg", BAD_ROWS),
        c("percentile_above_100", "reg", percentiles=[5, 101]), c("percentile_negative", "reg", percentiles=[-1]),
        *[c(n, "reg", **k) for n, k in BAD_W + TRACE_FAULTS],
        c("no_sample_trace", "reg", burn_in=1.0), c("no_sample_multiplicities", "reg", weights=(W, [0] * 6)),
        c("too_many_percentiles", "reg", percentiles=MANY_PCTS),
        c("state_none_and_x_unknown_name", "reg_none", "valid"), c("x_unknown_name_and_percentile_above_100", "reg", "valid", percentiles=[101]),
        c("x_too_few_columns_and_weights_1d", "reg", BAD_ROWS, weights=fill(REG_P, 1)),
        c("percentile_above_100_and_weights_1d", "reg", percentiles=[101], weights=fill(REG_P, 1)),
        c("percentile_above_100_and_state_label", "reg_label", percentiles=[101]),
        c("state_label_and_chains_empty", "reg_label", chains=[]), c("state_cap_and_state_unfinished", "reg_cap_unfinished"),
        c("chains_empty_and_too_many_percentiles", "reg", chains=[], percentiles=MANY_PCTS),
        c("weights_1d_and_too_many_percentiles", "reg", weights=fill(REG_P, 1), percentiles=MANY_PCTS),
        c("no_sample_and_too_many_percentiles", "reg", burn_in=1.0, percentiles=MANY_PCTS),
    ],
    "input_sensitivity": [
        *sources("reg", W), *sources("cls", WC, "train"),
        c("rows_with_extra_columns", "cls", CLS_ROWS), c("return_samples", "reg", return_samples=True),
        c("percentiles_none", "reg", percentiles=()), *states("reg"), c("state_cap_with_weights", "reg_cap", weights=W),
        c("x_unknown_name", "reg", "end"), c("x_too_few_columns", "reg", BAD_ROWS), c("percentile_above_100", "reg", percentiles=[100.5]),
        *[c(n, "reg", **k) for n, k in BAD_W + TRACE_FAULTS], c("no_sample_trace", "reg", burn_in=1.0),
        c("too_many_percentiles", "reg", percentiles=MANY_PCTS),
        c("state_sharded_and_x_unknown_name", "reg_sharded", "end"), c("x_unknown_name_and_percentile_above_100", "reg", "end", percentiles=[101]),
        c("percentile_above_100_and_weights_1d", "reg", percentiles=[101], weights=fill(REG_P, 1)),
        c("percentile_above_100_and_state_unfinished", "reg_unfinished", percentiles=[101]),
        c("chains_empty_and_too_many_percentiles", "reg", chains=[], percentiles=MANY_PCTS),
    ],
    "convergence_diagnostics": [
        c("trace_all", "reg"), c("trace_cold_thin", "reg", chains="cold", thin=3, per_chain=True, n_lags=4),
        c("trace_list_burn_in", "cls", chains=[2, 0], burn_in=0.5, thin=2), c("params_some", "reg", params=[3, 0, 30], scalars=()),
        c("params_none_scalars_all", "reg", params=[], scalars=("rmse_test", "eta", "likelihood", "acc_test", "rmse_train")),
        c("cls_acc_train", "cls", params=[1], scalars=("acc_train", "likelihood", "likelihood")),
        c("draws", "reg", draws=fill((3, 8, 2), 1)), c("draws_with_options", "cls", draws=fill((2, 9, 4), 2, dtype=np.float32), per_chain=True, n_lags=2),
        *states("reg"), c("state_label_with_draws", "reg_label", draws=fill((3, 8, 2), 1)),
        c("draws_2d", "reg", draws=fill((3, 8), 1)), *[c(n, "reg", **k) for n, k in TRACE_FAULTS],
        c("param_out_of_range", "reg", params=[0, 31]), c("param_negative", "reg", params=[-1]), c("scalar_unknown", "reg", scalars=("loss",)),
        c("scalar_eta_of_a_classification", "cls", scalars=("eta",)), c("scalar_acc_train_of_a_regression", "reg", scalars=("acc_train",)),
        c("no_quantity", "reg", params=[], scalars=()),
        c("state_none_and_draws_2d", "reg_none", draws=fill((3, 8), 1)), c("state_label_and_param_out_of_range", "reg_label", params=[31]),
        c("chains_empty_and_param_out_of_range", "reg", chains=[], params=[31]),
        c("param_out_of_range_and_scalar_unknown", "reg", params=[31], scalars=("loss",)),
        c("draws_2d_and_scalar_unknown", "reg", draws=fill((3, 8), 1), scalars=("loss",)),
        c("draws_and_scalar_unknown", "reg", draws=fill((3, 8, 2), 1), scalars=("loss",), params=[99]),
    ],
    "predictive_accuracy": [
        *sources("reg", W, eta=ETA), *sources("cls", WC, "test"),
        c("calm", "reg_calm"), c("rows_with_extra_columns", "reg", REG_ROWS), c("rows_with_extra_columns_cls", "cls", CLS_ROWS, r_eff=0.7),
        c("cls_eta_not_needed", "cls", weights=WC, eta=ETA), c("return_pointwise", "reg", return_pointwise=True),
        c("loglik_array", "reg", loglik=LOGLIK), c("loglik_with_multiplicities", "reg", loglik=(LOGLIK, [1, 2, 0, 3, 1, 1, 1, 4]), return_pointwise=True),
        c("loglik_wins_over_data_and_weights", "reg", "valid", loglik=LOGLIK, weights=fill(REG_P, 1)),
        *states("reg"), c("state_unfinished_with_weights", "reg_unfinished", weights=W, eta=ETA), c("state_label_with_loglik", "reg_label", loglik=LOGLIK),
        c("data_unknown_name", "reg", "valid"), c("data_too_few_columns", "reg", fill((5, 4), 1)), c("data_1d", "reg", fill(5, 1)),
        *[c(n, "reg", eta=ETA, **k) for n, k in BAD_W], c("weights_without_eta", "reg", weights=W), *[c(n, "reg", **k) for n, k in TRACE_FAULTS],
        c("state_none_and_data_unknown_name", "reg_none", "valid"), c("data_unknown_name_and_weights_1d", "reg", "valid", weights=fill(REG_P, 1)),
        c("data_too_few_columns_and_weights_without_eta", "reg", fill((5, 4), 1), weights=W),
        c("weights_1d_and_without_eta", "reg", weights=fill(REG_P, 1)), c("weights_without_eta_and_state_label", "reg_label", weights=W),
        c("data_unknown_name_and_state_label", "reg_label", "valid"), c("state_label_and_chains_empty", "reg_label", chains=[]),
    ],
    "leave_future_out": [
        c("train_no_refit", "reg", refit=False), c("test_no_refit", "reg", None, 2, "test", refit=False, k_threshold=0.6),
        c("calm", "reg_calm", refit=False), c("cls_rows", "cls", 4, 1, CLS_ROWS, n_fit=8, refit=False, r_eff=0.8),
        c("rows_backward_and_forward", "reg", 3, 1, REG_ROWS, n_fit=7, refit=False, chains="cold", thin=3),
        c("trace_list_burn_in", "reg", refit=False, chains=[2, 0], burn_in=0.5, thin=2),
        c("refit_callable", "reg", 20, refit=Refit("reg"), k_threshold=0.7), c("refit_callable_forward_cls", "cls", None, 1, "test", refit=Refit("cls")),
        c("refit_callable_max_refits", "reg", 20, refit=Refit("reg"), k_threshold=0.5, max_refits=1),
        c("refit_callable_max_refits_zero", "reg", 24, 2, refit=Refit("reg"), k_threshold=0.5, max_refits=0),
        *states("reg", refit=False), c("refit_without_a_handle", "reg", 20, refit=Refit("reg_none"), k_threshold=0.0),
        c("refit_on_a_sharded_ladder", "reg", 20, refit=Refit("reg_sharded"), k_threshold=0.0),
        c("refit_unfinished", "reg", 20, refit=Refit("reg_unfinished"), k_threshold=0.0),
        c("data_unknown_name", "reg", data="valid", refit=False), c("n_fit_with_a_name", "reg", data="test", n_fit=30, refit=False),
        c("data_too_few_columns", "reg", data=fill((9, 4), 1), n_fit=4, refit=False), c("rows_without_n_fit", "reg", data=REG_ROWS, refit=False),
        c("block_zero", "reg", block=0, refit=False), c("n_fit_zero", "reg", data=REG_ROWS, n_fit=0, refit=False),
        c("n_fit_above_the_rows", "reg", data=REG_ROWS, n_fit=13, refit=False), c("min_train_zero", "reg", 0, refit=False),
        c("no_origin_left", "reg", 28, 3, refit=False), c("refit_not_callable", "reg", refit="yes"),
        *[c(n, "reg", refit=False, **k) for n, k in TRACE_FAULTS], c("one_sample", "reg", refit=False, chains="cold", thin=100),
        c("max_refits_negative", "reg", refit=False, max_refits=-1),
        c("state_none_and_data_unknown_name", "reg_none", data="valid"), c("data_unknown_name_and_n_fit", "reg", data="valid", n_fit=3),
        c("data_too_few_columns_and_no_n_fit", "reg", data=fill((9, 4), 1)), c("n_fit_with_a_name_and_block_zero", "reg", n_fit=3, block=0),
        c("rows_without_n_fit_and_block_zero", "reg", data=REG_ROWS, block=0), c("block_zero_and_n_fit_zero", "reg", data=REG_ROWS, n_fit=0, block=0),
        c("n_fit_zero_and_min_train_zero", "reg", 0, data=REG_ROWS, n_fit=0), c("min_train_zero_and_no_origin_left", "reg", 0, 31),
        c("no_origin_left_and_refit_not_callable", "reg", 28, 3, refit=1), c("refit_not_callable_and_state_label", "reg_label", refit=1),
        c("block_zero_and_state_label", "reg_label", block=0), c("state_label_and_chains_empty", "reg_label", chains=[], refit=False),
        c("chains_empty_and_one_sample", "reg", chains=[], thin=100, refit=False),
        c("one_sample_and_max_refits_negative", "reg", refit=False, chains="cold", thin=100, max_refits=-1),
    ],
    "predictive_calibration": [
        *sources("reg", W, eta=ETA), *sources("cls", WC, "train"),
        c("rows_with_extra_columns", "reg", REG_ROWS, quantiles=(0.1, 0.25, 0.5, 0.75, 0.9), levels=(0.5,), bins=4),
        c("rows_with_extra_columns_cls", "cls", CLS_ROWS, bins=3), c("no_crps_no_quantiles", "reg", "train", quantiles=(), crps=False),
        c("cls_eta_not_needed", "cls", weights=WC, eta=ETA),
        *late({}, "data_unknown_name", dict(data="valid")),
        c("too_many_quantiles", "reg", quantiles=[(k + 1) / 20 for k in range(17)]), c("quantile_one", "reg", quantiles=(0.5, 1.0)),
        c("level_zero", "reg", levels=(0.0, 0.5)), c("bins_zero", "reg", bins=0), c("data_unknown_name", "reg", "valid"),
        c("data_too_few_columns", "reg", fill((5, 4), 1)), *[c(n, "reg", eta=ETA, **k) for n, k in BAD_W], c("weights_without_eta", "reg", weights=W),
        *[c(n, "reg", **k) for n, k in TRACE_FAULTS], c("labels_out_of_range", "cls", fill((6, 5), 1, 3, 9)),
        c("too_many_quantiles_and_quantile_one", "reg", quantiles=[(k + 1) / 17 for k in range(17)]),
        c("quantile_one_and_level_zero", "reg", quantiles=(1.0,), levels=(0.0,)), c("level_zero_and_bins_zero", "reg", levels=(0.0,), bins=0),
        c("bins_zero_and_data_unknown_name", "reg", "valid", bins=0), c("data_unknown_name_and_weights_1d", "reg", "valid", weights=fill(REG_P, 1)),
        c("data_too_few_columns_and_weights_without_eta", "reg", fill((5, 4), 1), weights=W), c("weights_1d_and_without_eta", "reg", weights=fill(REG_P, 1)),
        c("state_none_and_chains_empty", "reg_none", chains=[]), c("state_label_and_chains_empty", "reg_label", chains=[]),
        c("state_none_and_bins_zero", "reg_none", bins=0),
    ],
    "predictive_check": [
        *sources("reg", W, eta=ETA), *sources("cls", WC, "test"),
        c("rows_with_extra_columns", "reg", REG_ROWS, lags=[2, 1, 7], seed=5, return_samples=True), c("rows_with_extra_columns_cls", "cls", CLS_ROWS, lags=None),
        c("lags_none", "reg", lags=None), c("lags_empty_cls", "cls", lags=()), c("default_lags_cut_to_the_rows", "reg", fill((4, 5), 2)),
        c("cls_eta_not_needed", "cls", weights=WC, eta=ETA),
        *late({}, "data_unknown_name", dict(data="valid")),
        c("data_unknown_name", "reg", "valid"), c("data_too_few_columns", "reg", fill((5, 4), 1)), c("one_row", "reg", fill((1, 5), 1)),
        c("lags_of_a_classification", "cls", lags=[1]), c("two_outputs", "reg_twoout"), c("lag_not_an_integer", "reg", lags=[1.5]),
        c("too_many_lags", "reg", lags=list(range(1, 18))), c("lag_twice", "reg", lags=[1, 2, 1]), c("lag_at_the_row_count", "reg", lags=[30]),
        *[c(n, "reg", eta=ETA, **k) for n, k in BAD_W], c("weights_without_eta", "reg", weights=W), *[c(n, "reg", **k) for n, k in TRACE_FAULTS],
        c("data_unknown_name_and_lag_twice", "reg", "valid", lags=[1, 1]), c("one_row_and_lags_of_a_classification", "cls", CLS_ROWS[:1], lags=[1]),
        c("one_row_and_two_outputs", "reg_twoout", fill((1, 5), 1)), c("two_outputs_and_lag_twice", "reg_twoout", lags=[1, 1]),
        c("lag_twice_and_weights_1d", "reg", lags=[1, 1], weights=fill(REG_P, 1)), c("lags_of_a_classification_and_weights_1d", "cls", lags=[1], weights=fill(CLS_P, 1)),
        c("weights_1d_and_without_eta", "reg", weights=fill(REG_P, 1)), c("state_none_and_chains_empty", "reg_none", chains=[]),
        c("state_none_and_lag_twice", "reg_none", lags=[1, 1]), c("state_label_and_chains_empty", "reg_label", chains=[]),
    ],
    "powerscale_sensitivity": [
        *sources("reg", W, eta=ETA), *sources("cls", WC, "train"),
        c("calm", "reg_calm"), c("rows_with_extra_columns", "reg", REG_ROWS, quantities=("predictions", "loglik"), delta=0.1, r_eff=0.5, threshold=0.02),
        c("rows_two_outputs", "reg_twoout", fill((3, 4), 2), quantities=["predictions"]),
        c("no_predictions_ignores_data", "reg", "valid", quantities=("loglik", "eta", "weights")), c("cls_eta_not_needed", "cls", weights=WC, eta=ETA),
        *late({}, "data_unknown_name", dict(data="valid")),
        c("delta_zero", "reg", delta=0), c("delta_nan", "reg", delta=float("nan")), c("quantity_unknown", "reg", quantities=["weights", "bias"]),
        c("quantities_empty", "reg", quantities=[]), c("eta_of_a_classification", "cls", quantities=["eta"]), c("data_unknown_name", "reg", "valid"),
        c("data_too_few_columns", "reg", BAD_ROWS), *[c(n, "reg", eta=ETA, **k) for n, k in BAD_W], c("weights_without_eta", "reg", weights=W),
        *[c(n, "reg", **k) for n, k in TRACE_FAULTS],
        c("delta_zero_and_quantity_unknown", "reg", delta=0, quantities=["bias"]), c("quantity_unknown_and_quantities_eta_cls", "cls", quantities=["eta", "bias"]),
        c("quantities_empty_and_data_unknown_name", "reg", "valid", quantities=[]), c("data_unknown_name_and_weights_1d", "reg", "valid", weights=fill(REG_P, 1)),
        c("data_too_few_columns_and_weights_without_eta", "reg", BAD_ROWS, weights=W), c("weights_1d_and_without_eta", "reg", weights=fill(REG_P, 1)),
        c("state_none_and_chains_empty", "reg_none", chains=[]), c("state_none_and_delta_zero", "reg_none", delta=0),
        c("state_label_and_chains_empty", "reg_label", chains=[]),
    ],
    "forecast": [
        *sources("reg", W, 3), c("noise_trace", "reg", 2, noise=True, seed=9), c("noise_weights", "reg", 2, "test", noise=True, weights=(W, MULT), eta=ETA),
        c("eta_not_needed", "reg", 2, weights=W, eta=ETA), c("origin_train", "reg", 2, "train", return_samples=True),
        c("origin_rows_with_extra_columns", "reg", 4, REG_ROWS, percentiles=[50]), c("percentiles_none", "reg", 1, percentiles=()),
        *states("reg", 2), c("state_label_with_weights", "reg_label", 2, weights=W),
        c("classification", "cls", 2), c("two_outputs", "reg_twoout", 2), c("origin_unknown_name", "reg", 2, "start"), c("origin_1d", "reg", 2, fill(4, 1)),
        c("origin_too_few_columns", "reg", 2, BAD_ROWS), c("percentile_above_100", "reg", 2, percentiles=[101]),
        *[c(n, "reg", 2, **k) for n, k in BAD_W + TRACE_FAULTS], c("noise_weights_without_eta", "reg", 2, noise=True, weights=W),
        c("no_sample_trace", "reg", 2, burn_in=1.0), c("too_many_percentiles", "reg", 2, percentiles=MANY_PCTS),
        c("state_none_and_classification", "cls_none", 2), c("classification_and_origin_unknown_name", "cls", 2, "start"),
        c("origin_unknown_name_and_percentile_above_100", "reg", 2, "start", percentiles=[101]),
        c("origin_too_few_columns_and_percentile_above_100", "reg", 2, BAD_ROWS, percentiles=[101]),
        c("percentile_above_100_and_weights_1d", "reg", 2, percentiles=[101], weights=fill(REG_P, 1)),
        c("weights_1d_and_noise_without_eta", "reg", 2, noise=True, weights=fill(REG_P, 1)),
        c("noise_weights_without_eta_and_too_many_percentiles", "reg", 2, noise=True, weights=W, percentiles=MANY_PCTS),
        c("percentile_above_100_and_state_label", "reg_label", 2, percentiles=[101]),
        c("chains_empty_and_too_many_percentiles", "reg", 2, chains=[], percentiles=MANY_PCTS),
    ],
    "log_evidence": [
        c("trace", "reg", prior_draws=64), c("trace_thin_burn_in", "reg", burn_in=0.1, thin=3, prior_draws=50, seed=3, return_draws=True),
        c("trace_cls", "cls", prior_draws=64), c("exact_settings", "reg_exact", prior_draws=64), c("agree", "reg_agree", prior_draws=64),
        c("low_kish", "reg_low_kish", prior_draws=64), c("adapted_ladder", "reg_adapt", prior_draws=64),
        c("weights", "reg", weights=(BETAS, WK), prior_draws=64), c("weights_return_draws", "reg_label", weights=(np.array(BETAS), WK), prior_draws=8, return_draws=True),
        *states("reg", prior_draws=64), c("state_unfinished_with_weights", "reg_unfinished", weights=(BETAS, WK), prior_draws=64),
        c("one_prior_draw", "reg", prior_draws=1), c("weights_not_a_pair", "reg", weights=WK), c("weights_a_triple", "reg", weights=(BETAS, WK, MULT)),
        c("weights_wrong_width", "reg", weights=(BETAS, WK[:, :, :30])), c("weights_other_rung_count", "reg", weights=(BETAS[:2], WK)),
        c("weights_three_draws", "reg", weights=(BETAS, WK[:, :3])), c("window_before_the_freeze", "reg_adapt", burn_in=0.25),
        c("window_too_short", "reg", burn_in=0.55), c("window_too_short_thinned", "reg", thin=5), c("duplicate_temperatures", "reg_dup"),
        c("duplicate_betas", "reg", weights=([0.5, 1.0, 0.5], WK)), c("no_rung_at_one", "reg_hot"), c("no_beta_at_one", "reg", weights=([0.2, 0.4, 0.8], WK)),
        c("state_none_and_one_prior_draw", "reg_none", prior_draws=1), c("one_prior_draw_and_weights_not_a_pair", "reg", prior_draws=1, weights=WK),
        c("one_prior_draw_and_state_label", "reg_label", prior_draws=1), c("weights_wrong_width_and_three_draws", "reg", weights=(BETAS, WK[:, :3, :30])),
        c("weights_three_draws_and_duplicate_betas", "reg", weights=([0.5, 1.0, 0.5], WK[:, :3])),
        c("state_label_and_window_too_short", "reg_label", burn_in=0.55), c("window_before_the_freeze_and_too_short", "reg_adapt", burn_in=0.3, thin=9),
        c("window_too_short_and_duplicate_temperatures", "reg_dup", burn_in=0.55), c("duplicate_betas_and_no_beta_at_one", "reg", weights=([0.5, 0.5, 0.8], WK)),
    ],
}
def case_ids():
    return [(m, name) for m in METHODS for name, _, _, _ in CASES[m]]


def run_case(method, name):
    """One case -> {"raises": [type, text]} or {"calls", "warnings", "result"}."""
    (obj, args, kw), = [(o, a, k) for n, o, a, k in CASES[method] if n == name]
    calls = []
    pt = make(obj, calls)
    kw = {k: v.bind(calls) if isinstance(v, Refit) else v for k, v in kw.items()}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out = getattr(pt, method)(*args, **kw)                                   # the frame a stacklevel=2 warning reports
        except Exception as e:                                                       # noqa: BLE001
            return {"raises": [type(e).__name__, str(e)]}
    assert type(out).__name__ in dir(pt_module) and out._fields
    return {"calls": calls, "warnings": [[w.category.__name__, str(w.message), os.path.relpath(w.filename, ROOT)] for w in caught],
            "result": {f: digest(getattr(out, f)) for f in out._fields}}


def analysis_class():
    """The class that defines the ten methods."""
    return next(k for k in pt_module.ParallelTemperingBase.__mro__ if "posterior_predictive" in vars(k))


def doc_digests():
    return {m: hashlib.sha256(getattr(pt_module.ParallelTemperingBase, m).__doc__.encode()).hexdigest() for m in METHODS}


def refusal_sites():
    """(source file, {line: "function: source line"}) of every raise and warnings.warn statement of the analysis class."""
    cls = analysis_class()
    path = inspect.getsourcefile(cls)
    text = open(path).read()
    lines = text.splitlines()
    node, = [n for n in ast.walk(ast.parse(text)) if isinstance(n, ast.ClassDef) and n.name == cls.__name__]
    same_class_as_the_driver = "run_chains" in vars(cls)
    sites = {}
    for fn in node.body:
        if isinstance(fn, ast.FunctionDef) and not (same_class_as_the_driver and fn.name in DRIVER_FUNCS):
            for n in ast.walk(fn):
                warn = isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "warn"
                if isinstance(n, ast.Raise) or warn:
                    sites[n.lineno] = f"{fn.name}: {lines[n.lineno - 1].strip()}"
    return path, sites


@pytest.fixture(scope="module")
def observed():
    """Every case run once, with the lines of the analysis class's file that were executed."""
    path, _ = refusal_sites()
    hit = set()

    def local(frame, event, arg):
        if event == "line":
            hit.add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_filename == path else None
    before = sys.gettrace()
    sys.settrace(tracer)
    try:
        got = {(m, n): run_case(m, n) for m, n in case_ids()}
    finally:
        sys.settrace(before)
    return got, hit


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_case_table_is_the_recorded_one(golden):
    assert all(len({n for n, _, _, _ in CASES[m]}) == len(CASES[m]) for m in METHODS)
    assert sorted(CASES) == sorted(METHODS)
    assert {m: sorted(golden["cases"][m]) for m in golden["cases"]} == {m: sorted(n for n, _, _, _ in CASES[m]) for m in METHODS}


@pytest.mark.parametrize("method, name", case_ids(), ids=lambda v: v)
def test_case_is_the_recorded_one(observed, golden, method, name):
    got = observed[0][method, name]
    assert got == golden["cases"][method][name]
    if "warnings" in got:
        assert all(w[2] == os.path.join("tests", "test_analysis_front_cpu.py") for w in got["warnings"])      # the caller's frame


def test_docstrings_are_the_recorded_ones(golden):
    assert doc_digests() == golden["docstrings"]


def test_every_refusal_site_is_reached(observed):
    _, sites = refusal_sites()
    missed = {text for line, text in sites.items() if line not in observed[1]}
    print(f"{len(sites)} raise / warn sites in {analysis_class().__name__}, {len(sites) - len(missed)} reached")
    assert missed == set(UNREACHED_ON_CPU)


def test_old_pickles_resolve():
    """A result pickled when the tuples lived in parallel_tempering names them there."""
    import pickle
    for name in ("Predictive", "Sensitivity", "Convergence", "PredictiveAccuracy", "LeaveFutureOut", "Calibration", "PredictiveCheck",
                 "PowerScaling", "Forecast", "Evidence"):
        cls = getattr(pt_module, name)
        blob = pickle.dumps(cls(*range(len(cls._fields))), protocol=2).replace(cls.__module__.encode(), b"ptnn_amd.parallel_tempering")
        assert pickle.loads(blob) == cls(*range(len(cls._fields)))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage (from the commit before the change): python tests/test_analysis_front_cpu.py --record")
    doc = dict(cases={m: {} for m in METHODS}, docstrings=doc_digests())
    for m_, n_ in case_ids():
        doc["cases"][m_][n_] = run_case(m_, n_)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: {{\n' + ",\n".join(f'  {json.dumps(a)}: ' + (
            "{\n" + ",\n".join(f'   {json.dumps(b)}: {json.dumps(w, sort_keys=True)}' for b, w in sorted(v.items())) + "\n  }"
            if k == "cases" else json.dumps(v)) for a, v in sorted(d.items())) + "\n }" for k, d in sorted(doc.items())) + "\n}\n")
    n_raise = sum("raises" in v for d in doc["cases"].values() for v in d.values())
    print(f"{len(case_ids())} cases recorded in {GOLDEN}: {n_raise} refusals, {len(case_ids()) - n_raise} calls")
