"""The argument checks of seventeen posterior analysis calls, characterised (no GPU): every call checks its spec before it looks
at the handle, so a NULL handle shows which fault a spec is refused for, with which return code and which ptnn_last_error()
text.  CASES names, per call, faulty specs for every refusal that precedes the handle check -- pairs of simultaneous faults
included, where the order of the checks decides which one is reported -- and valid specs, which reach the handle check.  One
refusal is left out: ptnn_evidence's "more than 2^31 - 1 expanded draws" needs 8 GiB of host multiplicities to provoke.

The expected values are tests/golden/analysis_errors.json, with the size and the (offset, size) of every field of their spec
structures.  The file is recorded once, from a library built from the commit BEFORE a change to the analysis calls, never from the
code under test:

    PTNN_LIBRARY=<parent checkout>/parallel-tempering-neural-net_amd/libptnn.so python tests/test_analysis_errors_cpu.py --record
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "analysis_errors.json")

HOST, TRAIN = 0, 1                                       # PTNN_PREDICT_X_* / PTNN_FORECAST_ORIGIN_*
f32 = lambda *shape: np.zeros(shape, np.float32)         # noqa: E731
f64 = lambda *shape: np.full(shape, -1.0)                # noqa: E731
i32 = lambda *v: np.array(v, np.int32)                   # noqa: E731
i64 = lambda *v: np.array(v, np.int64)                   # noqa: E731


def _nan_at(a, *idx):
    a[idx] = math.nan
    return a


# ---- valid specs: the fields of a spec that passes every argument check (struct_bytes is set by the test) ----
TRACE = dict(nsteps=8, thin=1)                                                     # trace rows of all chains
ROWS = dict(x_source=TRAIN, n_rows=5)
PREDICT = dict(TRACE, **ROWS)
PREDICT_HOST = dict(w=f32(3, 4), n_w=3, x_source=HOST, x=f32(5, 4), n_rows=5)
CONV = dict(TRACE)
CONV_HOST = dict(draws=f32(2, 8, 3), n_chains=2, n_draws=8, n_quantities=3)
ELPD = dict(TRACE, r_eff=1.0, **ROWS)
ELPD_W = dict(w=f32(3, 4), n_w=3, r_eff=1.0, **ROWS)
ELPD_LL = dict(loglik=f64(4, 6), n_w=4, n_rows=6, r_eff=1.0)
LFO_ARGS = dict(n_fit=6, block=1, origins=i32(2, 4), n_origins=2)
LFO = dict(TRACE, r_eff=1.0, x_source=TRAIN, n_rows=6, **LFO_ARGS)
LFO_LL = dict(ELPD_LL, **LFO_ARGS)
FORECAST = dict(TRACE, origin_source=TRAIN, n_origins=3, horizon=2)
EVID = dict(TRACE)
EVID_U = dict(u=f64(2, 4), n_rungs=2, n_per_rung=4)
EVID_W = dict(w=f32(2, 4, 3), n_rungs=2, n_per_rung=4)
PRIOR = dict(n_prior=10, a=np.array([0.5, 1.0]), n_a=2)
CALIB = dict(TRACE, **ROWS)
CALIB_W = dict(w=f32(3, 4), n_w=3, **ROWS)
LEVELS = dict(n_levels=2, levels_p=np.array([0.1, 0.9]), levels_z=np.array([-1.28, 1.28]), quantiles=f64(2, 5))
PPC = dict(TRACE, **ROWS)
PPC_W = dict(w=f32(3, 4), n_w=3, **ROWS)
PS = dict(TRACE, groups=1 | 4, delta=0.01, r_eff=1.0, **ROWS)
PS_W = dict(w=f32(3, 4), n_w=3, groups=1 | 4, delta=0.01, r_eff=1.0, **ROWS)
PD_ARGS = dict(n_grid=3, grid=f32(2, 3), inputs=i32(0, 2), n_inputs=2)
PD = dict(PREDICT, **PD_ARGS)
PD_HOST = dict(PREDICT_HOST, **PD_ARGS)
SHAP_ARGS = dict(n_background=2, background=f32(2, 4), n_coalitions=3, masks=np.array([0, 1, 3], np.uint64), n_terms=2, coef=f64(3, 2))
SHAP = dict(PREDICT, **SHAP_ARGS)
SHAP_HOST = dict(PREDICT_HOST, **SHAP_ARGS)
REPORT = dict(PREDICT, auc=1)
REPORT_HOST = dict(PREDICT_HOST, x=f32(5, 5), auc=1)
UNC = dict(TRACE, **ROWS)
UNC_W = dict(w=f32(3, 4), n_w=3, **ROWS)
INFL_ROWS = dict(case_source=TRAIN, n_cases=5, target_source=TRAIN, n_targets=4)
INFL = dict(TRACE, **INFL_ROWS)
INFL_W = dict(w=f32(3, 4), n_w=3, **INFL_ROWS)
INFL_MAT = dict(target_values=f32(4, 3), loglik=f64(4, 6), n_w=4, n_a=3, n_b=6)
FSCORE = dict(TRACE, origin_source=TRAIN, n_origins=3, horizon=2, truth=f32(3, 2))
FSCORE_W = dict(FSCORE, w=f32(3, 4), n_w=3, eta=f32(3), origin_source=HOST, origins=f32(3, 4))
FSCORE_LEVELS = dict(n_levels=2, levels_p=np.array([0.1, 0.9]), levels_z=np.array([-1.28, 1.28]), quantiles=f64(2, 6))
MBAR_ARGS = dict(n_rungs=2, betas=np.array([0.5, 1.0]), target_beta=1.0, tol=1e-8, max_iter=100)
MBAR = dict(TRACE, **MBAR_ARGS)
MBAR_U = dict(MBAR_ARGS, u=f64(2, 4), n_per_rung=4)
MBAR_W = dict(MBAR_ARGS, w=f32(2, 4, 3), n_per_rung=4)
MBAR_PRIOR = dict(n_prior=3, u_prior=f64(3))
MBAR_MULT_NEGATIVE = dict(multiplicity=np.array([[1, 1, 1, 1], [1, -3, 1, 1]], np.int32))

RANK_FAULTS = [
    ("n_ranks_negative", dict(n_ranks=-1)),
    ("n_ranks_above_max", dict(n_ranks=17)),
    ("ranks_null", dict(n_ranks=2)),
    ("order_stats_without_ranks", dict(order_stats=f32(5))),
]
TRACE_FAULTS = [
    ("thin_zero", dict(thin=0)),
    ("replica_list_empty", dict(replicas=i32(0), n_replicas=0)),
]
ROW_FAULTS = [
    ("x_source_unknown", dict(x_source=7)),
    ("x_host_null", dict(x_source=HOST)),
]
MULT_NEGATIVE = dict(multiplicity=i32(1, -2, 1))

# (structure, entry point, [(case name, base fields, overriding fields)])
CASES = {
    "predict": ("PredictSpec", "ptnn_predict", [
        ("valid_trace", PREDICT, {}),
        ("valid_host", PREDICT_HOST, {}),
        *[(n, PREDICT, f) for n, f in TRACE_FAULTS + ROW_FAULTS + RANK_FAULTS],
        ("n_w_zero", PREDICT_HOST, dict(n_w=0)),
        ("n_rows_zero", PREDICT, dict(n_rows=0)),
        ("thin_zero_and_n_rows_zero", PREDICT, dict(thin=0, n_rows=0)),
        ("x_source_unknown_and_n_rows_zero", PREDICT, dict(x_source=7, n_rows=0)),
        ("n_rows_zero_and_n_ranks_negative", PREDICT, dict(n_rows=0, n_ranks=-1)),
    ]),
    "sensitivity": ("SensitivitySpec", "ptnn_sensitivity", [
        ("valid_trace", PREDICT, {}),
        ("valid_host", PREDICT_HOST, dict(ranks=i64(0, 2), n_ranks=2, ranks2=i64(1), n_ranks2=1)),
        *[(n, PREDICT, f) for n, f in TRACE_FAULTS + ROW_FAULTS + RANK_FAULTS],
        ("n_w_zero", PREDICT_HOST, dict(n_w=0)),
        ("n_rows_zero", PREDICT, dict(n_rows=0)),
        ("n_ranks2_negative", PREDICT, dict(n_ranks2=-1)),
        ("n_ranks2_above_max", PREDICT, dict(n_ranks2=17)),
        ("ranks2_null", PREDICT, dict(n_ranks2=2)),
        ("abs_order_stats_without_ranks2", PREDICT, dict(abs_order_stats=f32(5))),
        ("ranks_null_and_n_ranks2_negative", PREDICT, dict(n_ranks=3, n_ranks2=-1)),
        ("thin_zero_and_x_source_unknown", PREDICT, dict(thin=0, x_source=7)),
    ]),
    "convergence": ("ConvergenceSpec", "ptnn_convergence", [
        ("valid_trace", CONV, dict(scalars=1 | 2, n_lags=2, rho=f64(2, 6))),
        ("valid_host", CONV_HOST, {}),
        ("n_chains_zero", CONV_HOST, dict(n_chains=0)),
        ("n_draws_three", CONV_HOST, dict(n_draws=3)),
        ("n_quantities_zero", CONV_HOST, dict(n_quantities=0)),
        ("n_chains_zero_and_n_draws_three", CONV_HOST, dict(n_chains=0, n_draws=3)),
        *[(n, CONV, f) for n, f in TRACE_FAULTS],
        ("n_params_negative", CONV, dict(params=i32(0), n_params=-1)),
        ("scalars_not_a_quantity", CONV, dict(scalars=1 << 5)),
        ("n_lags_negative", CONV, dict(n_lags=-1)),
        ("rho_null", CONV, dict(n_lags=2)),
        ("rho_without_lags", CONV, dict(rho=f64(4))),
        ("thin_zero_and_n_lags_negative", CONV, dict(thin=0, n_lags=-1)),
        ("n_quantities_zero_and_rho_null", CONV_HOST, dict(n_quantities=0, n_lags=1)),
    ]),
    "elpd": ("ElpdSpec", "ptnn_elpd", [
        ("valid_trace", ELPD, {}),
        ("valid_host", ELPD_W, dict(multiplicity=i32(1, 0, 2))),
        ("valid_loglik", ELPD_LL, dict(x_source=7)),
        ("w_and_loglik", ELPD_LL, dict(w=f32(4, 3))),
        ("r_eff_zero", ELPD, dict(r_eff=0.0)),
        ("r_eff_nan", ELPD, dict(r_eff=math.nan)),
        ("r_eff_inf", ELPD, dict(r_eff=math.inf)),
        ("no_source", ELPD, dict(nsteps=0)),
        *[(n, ELPD, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", ELPD_W, dict(n_w=0)),
        ("n_w_zero_loglik", ELPD_LL, dict(n_w=0)),
        ("n_rows_zero", ELPD, dict(n_rows=0)),
        ("loglik_out_with_loglik", ELPD_LL, dict(loglik_out=f64(4, 6))),
        ("multiplicity_negative", ELPD_W, MULT_NEGATIVE),
        ("loglik_not_finite", ELPD_LL, dict(loglik=_nan_at(f64(4, 6), 2, 5))),
        ("loglik_infinite_first_entry", ELPD_LL, dict(loglik=np.full((4, 6), -math.inf))),
        ("w_and_loglik_and_r_eff_zero", ELPD_LL, dict(w=f32(4, 3), r_eff=0.0)),
        ("r_eff_zero_and_no_source", ELPD, dict(r_eff=0.0, nsteps=0)),
        ("no_source_and_thin_zero", ELPD, dict(nsteps=0, thin=0)),
        ("thin_zero_and_n_rows_zero", ELPD, dict(thin=0, n_rows=0)),
        ("n_rows_zero_and_x_source_unknown", ELPD, dict(n_rows=0, x_source=7)),
        ("loglik_out_and_loglik_not_finite", ELPD_LL, dict(loglik_out=f64(4, 6), loglik=_nan_at(f64(4, 6), 0, 0))),
        ("multiplicity_negative_and_loglik_not_finite", ELPD_LL, dict(multiplicity=i32(1, 1, -1, 1), loglik=_nan_at(f64(4, 6), 0, 0))),
    ]),
    "lfo": ("LfoSpec", "ptnn_lfo", [
        ("valid_trace", LFO, {}),
        ("valid_host", LFO, dict(w=f32(3, 4), n_w=3, nsteps=0)),
        ("valid_loglik", LFO_LL, {}),
        ("w_and_loglik", LFO_LL, dict(w=f32(4, 3))),
        ("r_eff_zero", LFO, dict(r_eff=0.0)),
        ("no_source", LFO, dict(nsteps=0)),
        *[(n, LFO, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", LFO_LL, dict(n_w=0)),
        ("n_rows_zero", LFO, dict(n_rows=0)),
        ("block_zero", LFO, dict(block=0)),
        ("n_fit_zero", LFO, dict(n_fit=0)),
        ("n_fit_above_n_rows", LFO, dict(n_fit=7)),
        ("n_origins_zero", LFO, dict(n_origins=0)),
        ("origins_null", LFO, dict(origins=None)),
        ("origin_zero", LFO, dict(origins=i32(2, 0))),
        ("origin_at_n_rows", LFO, dict(origins=i32(6, 2))),
        ("origin_block_past_the_rows", LFO, dict(block=3)),
        ("loglik_out_with_loglik", LFO_LL, dict(loglik_out=f64(4, 6))),
        ("multiplicity_negative", LFO_LL, dict(multiplicity=i32(-1, 1, 1, 1))),
        ("loglik_not_finite", LFO_LL, dict(loglik=_nan_at(f64(4, 6), 3, 1))),
        ("r_eff_zero_and_block_zero", LFO, dict(r_eff=0.0, block=0)),
        ("n_rows_zero_and_block_zero", LFO, dict(n_rows=0, block=0)),
        ("block_zero_and_n_fit_zero", LFO, dict(block=0, n_fit=0)),
        ("n_fit_zero_and_n_origins_zero", LFO, dict(n_fit=0, n_origins=0)),
        ("origin_zero_and_x_source_unknown", LFO, dict(origins=i32(0, 2), x_source=7)),
        ("x_host_null_and_multiplicity_negative", LFO, dict(w=f32(3, 4), n_w=3, x_source=HOST, **MULT_NEGATIVE)),
    ]),
    "forecast": ("ForecastSpec", "ptnn_forecast", [
        ("valid_trace", FORECAST, dict(noise=1)),
        ("valid_host", FORECAST, dict(w=f32(3, 4), n_w=3, eta=f32(3), noise=1, origin_source=HOST, origins=f32(3, 4))),
        *[(n, FORECAST, f) for n, f in TRACE_FAULTS + RANK_FAULTS],
        ("n_w_zero", FORECAST, dict(w=f32(3, 4), n_w=0)),
        ("origin_source_unknown", FORECAST, dict(origin_source=-1)),
        ("origins_host_null", FORECAST, dict(origin_source=HOST)),
        ("n_origins_zero", FORECAST, dict(n_origins=0)),
        ("horizon_zero", FORECAST, dict(horizon=0)),
        ("too_many_columns", FORECAST, dict(n_origins=70000, horizon=70000)),
        ("noise_without_eta", FORECAST, dict(w=f32(3, 4), n_w=3, noise=1)),
        ("n_origins_zero_and_horizon_zero", FORECAST, dict(n_origins=0, horizon=0)),
        ("horizon_zero_and_n_ranks_negative", FORECAST, dict(horizon=0, n_ranks=-1)),
        ("ranks_null_and_noise_without_eta", FORECAST, dict(w=f32(3, 4), n_w=3, noise=1, n_ranks=1)),
    ]),
    "evidence": ("EvidenceSpec", "ptnn_evidence", [
        ("valid_trace", EVID, PRIOR),
        ("valid_host", EVID_W, dict(multiplicity=np.array([[1, 0, 2, 1], [4, 0, 0, 0]], np.int32))),
        ("valid_u", EVID_U, dict(multiplicity=np.array([[1, 0, 2, 1], [4, 0, 0, 0]], np.int32), u=_nan_at(f64(2, 4), 1, 2))),
        ("w_and_u", EVID_U, dict(w=f32(2, 4, 3))),
        ("n_rungs_zero", EVID_U, dict(n_rungs=0)),
        ("n_per_rung_zero", EVID_W, dict(n_per_rung=0)),
        ("no_source", EVID, dict(nsteps=0)),
        *[(n, EVID, f) for n, f in TRACE_FAULTS],
        ("n_prior_negative", EVID, dict(n_prior=-1)),
        ("n_prior_above_int32", EVID, dict(PRIOR, n_prior=1 << 31)),
        ("n_a_zero", EVID, dict(PRIOR, n_a=0)),
        ("n_a_above_max", EVID, dict(PRIOR, n_a=5)),
        ("a_null", EVID, dict(n_prior=10, n_a=2)),
        ("a_not_finite", EVID, dict(PRIOR, a=np.array([0.5, math.inf]))),
        ("u_prior_out_without_prior", EVID, dict(u_prior_out=f64(4))),
        ("u_out_with_u", EVID_U, dict(u_out=f64(8))),
        ("too_many_host_rows", EVID_W, dict(n_rungs=2, n_per_rung=1 << 30)),
        ("multiplicity_negative", EVID_U, dict(multiplicity=np.array([[1, 1, 1, 1], [1, -3, 1, 1]], np.int32))),
        ("u_not_finite", EVID_U, dict(u=_nan_at(f64(2, 4), 1, 2))),
        ("w_and_u_and_n_rungs_zero", EVID_U, dict(w=f32(2, 4, 3), n_rungs=0)),
        ("n_rungs_zero_and_n_prior_negative", EVID_U, dict(n_rungs=0, n_prior=-1)),
        ("no_source_and_thin_zero", EVID, dict(nsteps=0, thin=0)),
        ("thin_zero_and_n_prior_negative", EVID, dict(thin=0, n_prior=-1)),
        ("u_out_and_u_not_finite", EVID_U, dict(u_out=f64(8), u=_nan_at(f64(2, 4), 0, 0))),
    ]),
    "calibration": ("CalibrationSpec", "ptnn_calibration", [
        ("valid_trace", CALIB, dict(LEVELS, pair_term=1, crps=f64(5))),
        ("valid_host", CALIB_W, dict(multiplicity=i32(2, 0, 1))),
        ("no_source", CALIB, dict(nsteps=0)),
        *[(n, CALIB, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", CALIB_W, dict(n_w=0)),
        ("n_rows_zero", CALIB, dict(n_rows=0)),
        ("n_levels_negative", CALIB, dict(n_levels=-1)),
        ("n_levels_above_max", CALIB, dict(LEVELS, n_levels=17)),
        ("levels_z_null", CALIB, dict(LEVELS, levels_z=None)),
        ("quantiles_null", CALIB, dict(LEVELS, quantiles=None)),
        ("quantiles_without_levels", CALIB, dict(quantiles=f64(5))),
        ("level_one", CALIB, dict(LEVELS, levels_p=np.array([0.1, 1.0]))),
        ("level_z_infinite", CALIB, dict(LEVELS, levels_z=np.array([-math.inf, 1.28]))),
        ("crps_without_pair_term", CALIB, dict(crps=f64(5))),
        ("multiplicity_negative", CALIB_W, MULT_NEGATIVE),
        ("no_source_and_n_rows_zero", CALIB, dict(nsteps=0, n_rows=0)),
        ("n_rows_zero_and_x_source_unknown", CALIB, dict(n_rows=0, x_source=7)),
        ("x_host_null_and_n_levels_negative", CALIB, dict(x_source=HOST, n_levels=-1)),
        ("crps_without_pair_term_and_multiplicity_negative", CALIB_W, dict(MULT_NEGATIVE, crps=f64(5))),
    ]),
    "ppc": ("PpcSpec", "ptnn_ppc", [
        ("valid_trace", PPC, dict(lags=i32(1, 4, 2), n_lags=3)),
        ("valid_host", PPC_W, dict(multiplicity=i32(2, 0, 1))),
        ("no_source", PPC, dict(nsteps=0)),
        *[(n, PPC, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", PPC_W, dict(n_w=0)),
        ("n_rows_one", PPC, dict(n_rows=1)),
        ("n_lags_negative", PPC, dict(n_lags=-1)),
        ("n_lags_above_max", PPC, dict(n_lags=17, lags=i32(*range(1, 18)))),
        ("lags_null", PPC, dict(n_lags=2)),
        ("lag_zero", PPC, dict(lags=i32(1, 0), n_lags=2)),
        ("lag_at_n_rows", PPC, dict(lags=i32(5, 1), n_lags=2)),
        ("lag_listed_twice", PPC, dict(lags=i32(1, 2, 1), n_lags=3)),
        ("multiplicity_negative", PPC_W, MULT_NEGATIVE),
        ("n_rows_one_and_x_source_unknown", PPC, dict(n_rows=1, x_source=7)),
        ("lag_listed_twice_and_lag_zero", PPC, dict(lags=i32(2, 2, 0), n_lags=3)),
        ("lags_null_and_multiplicity_negative", PPC_W, dict(MULT_NEGATIVE, n_lags=1)),
    ]),
    "powerscale": ("PowerscaleSpec", "ptnn_powerscale", [
        ("valid_trace", PS, {}),
        ("valid_host", PS_W, dict(multiplicity=i32(2, 0, 1))),
        ("valid_without_predictions", PS, dict(groups=1 | 2 | 8, n_rows=0, x_source=7)),
        ("delta_zero", PS, dict(delta=0.0)),
        ("delta_nan", PS, dict(delta=math.nan)),
        ("r_eff_zero", PS, dict(r_eff=0.0)),
        ("r_eff_inf", PS, dict(r_eff=math.inf)),
        ("groups_zero", PS, dict(groups=0)),
        ("groups_unknown", PS, dict(groups=16)),
        ("no_source", PS, dict(nsteps=0)),
        *[(n, PS, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", PS_W, dict(n_w=0)),
        ("n_rows_zero", PS, dict(n_rows=0)),
        ("multiplicity_negative", PS_W, MULT_NEGATIVE),
        ("delta_zero_and_r_eff_zero", PS, dict(delta=0.0, r_eff=0.0)),
        ("r_eff_zero_and_groups_zero", PS, dict(r_eff=0.0, groups=0)),
        ("groups_zero_and_no_source", PS, dict(groups=0, nsteps=0)),
        ("thin_zero_and_n_rows_zero", PS, dict(thin=0, n_rows=0)),
        ("x_source_unknown_and_multiplicity_negative", PS_W, dict(MULT_NEGATIVE, x_source=7)),
    ]),
    "partial_dependence": ("PdSpec", "ptnn_partial_dependence", [
        ("valid_trace", PD, {}),
        ("valid_host", PD_HOST, dict(ranks=i64(0, 2), n_ranks=2, ranks2=i64(1), n_ranks2=1)),
        ("valid_all_inputs", PD, dict(inputs=None, n_inputs=0, grid=_nan_at(f32(2, 3), 0, 0))),     # that grid is checked with the handle
        *[(n, PD, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", PD_HOST, dict(n_w=0)),
        ("n_rows_zero", PD, dict(n_rows=0)),
        ("n_ranks_negative", PD, dict(n_ranks=-1)),
        ("n_ranks_above_max", PD, dict(n_ranks=17)),
        ("ranks_null", PD, dict(n_ranks=2)),
        ("ice_order_stats_without_ranks", PD, dict(ice_order_stats=f32(5))),
        ("n_ranks2_negative", PD, dict(n_ranks2=-1)),
        ("ranks2_null", PD, dict(n_ranks2=2)),
        ("pd_order_stats_without_ranks2", PD, dict(pd_order_stats=f32(5))),
        ("range_order_stats_without_ranks2", PD, dict(range_order_stats=f32(5))),
        ("n_grid_zero", PD, dict(n_grid=0)),
        ("n_grid_above_max", PD, dict(n_grid=65)),
        ("grid_null", PD, dict(grid=None)),
        ("input_list_empty", PD, dict(n_inputs=0)),
        ("grid_not_finite", PD, dict(grid=_nan_at(f32(2, 3), 1, 2))),
        ("x_source_unknown_and_n_rows_zero", PD, dict(x_source=7, n_rows=0)),
        ("thin_zero_and_x_source_unknown", PD, dict(thin=0, x_source=7)),
        ("n_rows_zero_and_n_ranks_negative", PD, dict(n_rows=0, n_ranks=-1)),
        ("ranks_null_and_n_ranks2_negative", PD, dict(n_ranks=3, n_ranks2=-1)),
        ("n_ranks_above_max_and_n_grid_zero", PD, dict(n_ranks=17, n_grid=0)),
        ("n_ranks2_negative_and_grid_null", PD, dict(n_ranks2=-1, grid=None)),
        ("n_grid_zero_and_grid_null", PD, dict(n_grid=0, grid=None)),
        ("grid_null_and_input_list_empty", PD, dict(grid=None, n_inputs=0)),
        ("input_list_empty_and_grid_not_finite", PD, dict(n_inputs=0, grid=_nan_at(f32(2, 3), 0, 0))),
    ]),
    "coalition_values": ("ShapSpec", "ptnn_coalition_values", [
        ("valid_trace", SHAP, {}),
        ("valid_host", SHAP_HOST, dict(ranks=i64(0, 2), n_ranks=2, ranks2=i64(1), n_ranks2=1)),
        ("valid_mask_bit_above_n_in", SHAP, dict(masks=np.array([0, 1, 1 << 40], np.uint64))),      # a mask's bits are checked with the handle
        *[(n, SHAP, f) for n, f in TRACE_FAULTS + ROW_FAULTS + RANK_FAULTS],
        ("n_w_zero", SHAP_HOST, dict(n_w=0)),
        ("n_rows_zero", SHAP, dict(n_rows=0)),
        ("n_ranks2_negative", SHAP, dict(n_ranks2=-1)),
        ("ranks2_null", SHAP, dict(n_ranks2=2)),
        ("abs_order_stats_without_ranks2", SHAP, dict(abs_order_stats=f32(5))),
        ("n_background_zero", SHAP, dict(n_background=0)),
        ("n_background_above_max", SHAP, dict(n_background=257)),
        ("n_coalitions_zero", SHAP, dict(n_coalitions=0)),
        ("n_coalitions_above_max", SHAP, dict(n_coalitions=4097)),
        ("n_terms_zero", SHAP, dict(n_terms=0)),
        ("n_terms_above_max", SHAP, dict(n_terms=65)),
        ("background_null", SHAP, dict(background=None)),
        ("masks_null", SHAP, dict(masks=None)),
        ("coef_null", SHAP, dict(coef=None)),
        ("coef_not_finite", SHAP, dict(coef=_nan_at(f64(3, 2), 2, 1))),
        ("x_source_unknown_and_n_rows_zero", SHAP, dict(x_source=7, n_rows=0)),
        ("n_rows_zero_and_n_ranks_negative", SHAP, dict(n_rows=0, n_ranks=-1)),
        ("ranks_null_and_n_ranks2_negative", SHAP, dict(n_ranks=3, n_ranks2=-1)),
        ("n_ranks2_negative_and_n_background_zero", SHAP, dict(n_ranks2=-1, n_background=0)),
        ("n_background_zero_and_n_coalitions_zero", SHAP, dict(n_background=0, n_coalitions=0)),
        ("n_coalitions_zero_and_n_terms_zero", SHAP, dict(n_coalitions=0, n_terms=0)),
        ("n_terms_zero_and_background_null", SHAP, dict(n_terms=0, background=None)),
        ("background_null_and_masks_null", SHAP, dict(background=None, masks=None)),
        ("masks_null_and_coef_null", SHAP, dict(masks=None, coef=None)),
        ("masks_null_and_coef_not_finite", SHAP, dict(masks=None, coef=_nan_at(f64(3, 2), 0, 0))),
    ]),
    "class_report": ("ClassReportSpec", "ptnn_class_report", [
        ("valid_trace", REPORT, {}),
        ("valid_host", REPORT_HOST, dict(ranks=i64(0, 2), n_ranks=2)),
        ("valid_without_auc_above_its_cap", REPORT, dict(auc=0, n_rows=16385)),
        *[(n, REPORT, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", REPORT_HOST, dict(n_w=0)),
        ("n_rows_zero", REPORT, dict(n_rows=0)),
        ("n_rows_above_the_grid", REPORT, dict(auc=0, n_rows=65535 * 64 + 1)),
        ("n_ranks_negative", REPORT, dict(n_ranks=-1)),
        ("n_ranks_above_max", REPORT, dict(n_ranks=17)),
        ("ranks_null", REPORT, dict(n_ranks=2)),
        ("metric_order_stats_without_ranks", REPORT, dict(metric_order_stats=f32(5))),
        ("auc_rows_above_cap", REPORT, dict(n_rows=16385)),
        ("x_source_unknown_and_n_rows_zero", REPORT, dict(x_source=7, n_rows=0)),
        ("thin_zero_and_x_source_unknown", REPORT, dict(thin=0, x_source=7)),
        ("n_rows_above_the_grid_and_n_ranks_negative", REPORT, dict(n_rows=65535 * 64 + 1, n_ranks=-1)),
        ("n_ranks_negative_and_auc_rows_above_cap", REPORT, dict(n_ranks=-1, n_rows=16385)),
    ]),
    "uncertainty": ("UncertaintySpec", "ptnn_uncertainty", [
        ("valid_trace", UNC, {}),
        ("valid_host", UNC_W, dict(multiplicity=i32(2, 0, 1), ranks=i64(0, 2), n_ranks=2)),
        ("no_source", UNC, dict(nsteps=0)),
        *[(n, UNC, f) for n, f in TRACE_FAULTS + ROW_FAULTS],
        ("n_w_zero", UNC_W, dict(n_w=0)),
        ("n_rows_zero", UNC, dict(n_rows=0)),
        ("n_ranks_negative", UNC, dict(n_ranks=-1)),
        ("n_ranks_above_max", UNC, dict(n_ranks=17)),
        ("ranks_null", UNC, dict(n_ranks=2)),
        ("entropy_order_stats_without_ranks", UNC, dict(entropy_order_stats=f32(5))),
        ("multiplicity_negative", UNC_W, MULT_NEGATIVE),
        ("no_source_and_thin_zero", UNC, dict(nsteps=0, thin=0)),
        ("thin_zero_and_x_source_unknown", UNC, dict(thin=0, x_source=7)),
        ("x_source_unknown_and_n_rows_zero", UNC, dict(x_source=7, n_rows=0)),
        ("n_rows_zero_and_n_ranks_negative", UNC, dict(n_rows=0, n_ranks=-1)),
        ("ranks_null_and_multiplicity_negative", UNC_W, dict(MULT_NEGATIVE, n_ranks=2)),
    ]),
    "influence": ("InfluenceSpec", "ptnn_influence", [
        ("valid_trace", INFL, {}),
        ("valid_host", INFL_W, dict(multiplicity=i32(2, 0, 1), target_kind=1)),
        ("valid_matrices", INFL_MAT, dict(multiplicity=i32(1, 0, 2, 1), case_source=7, target_kind=9)),
        ("target_values_without_loglik", INFL_MAT, dict(loglik=None)),
        ("loglik_without_target_values", INFL_MAT, dict(target_values=None)),
        ("w_and_matrices", INFL_MAT, dict(w=f32(4, 3))),
        ("no_source", INFL, dict(nsteps=0)),
        *[(n, INFL, f) for n, f in TRACE_FAULTS],
        ("n_w_zero", INFL_W, dict(n_w=0)),
        ("n_w_zero_matrices", INFL_MAT, dict(n_w=0)),
        ("n_a_zero", INFL_MAT, dict(n_a=0)),
        ("n_b_zero", INFL_MAT, dict(n_b=0)),
        ("matrices_too_many_elements", INFL_MAT, dict(n_a=1 << 14, n_b=(1 << 13) + 1)),
        ("target_kind_unknown", INFL, dict(target_kind=2)),
        ("case_source_unknown", INFL, dict(case_source=7)),
        ("case_x_null", INFL, dict(case_source=HOST)),
        ("target_source_unknown", INFL, dict(target_source=-1)),
        ("target_x_null", INFL, dict(target_source=HOST)),
        ("n_cases_zero", INFL, dict(n_cases=0)),
        ("n_targets_zero", INFL, dict(n_targets=0)),
        ("multiplicity_negative", INFL_W, MULT_NEGATIVE),
        ("loglik_not_finite", INFL_MAT, dict(loglik=_nan_at(f64(4, 6), 2, 5))),
        ("target_values_without_loglik_and_w", INFL_MAT, dict(loglik=None, w=f32(4, 3))),
        ("w_and_matrices_and_n_w_zero", INFL_MAT, dict(w=f32(4, 3), n_w=0)),
        ("no_source_and_target_kind_unknown", INFL, dict(nsteps=0, target_kind=2)),
        ("thin_zero_and_case_source_unknown", INFL, dict(thin=0, case_source=7)),
        ("n_w_zero_and_n_a_zero", INFL_MAT, dict(n_w=0, n_a=0)),
        ("target_kind_unknown_and_case_source_unknown", INFL, dict(target_kind=2, case_source=7)),
        ("case_x_null_and_target_source_unknown", INFL, dict(case_source=HOST, target_source=-1)),
        ("target_x_null_and_n_cases_zero", INFL, dict(target_source=HOST, n_cases=0)),
        ("n_targets_zero_and_multiplicity_negative", INFL_W, dict(MULT_NEGATIVE, n_targets=0)),
        ("multiplicity_negative_and_loglik_not_finite", INFL_MAT, dict(multiplicity=i32(1, 1, -1, 1), loglik=_nan_at(f64(4, 6), 0, 0))),
    ]),
    "forecast_score": ("ForecastScoreSpec", "ptnn_forecast_score", [
        ("valid_trace", FSCORE, dict(FSCORE_LEVELS, pair_term=1, crps=f64(6), energy=1, energy_score=f64(3), noise=1)),
        ("valid_host", FSCORE_W, dict(multiplicity=i32(2, 0, 1), noise=1, truth=_nan_at(f32(3, 2), 1, 0))),
        ("valid_trace_without_rows", FSCORE, dict(nsteps=0)),                      # an empty selection is refused with the handle
        *[(n, FSCORE, f) for n, f in TRACE_FAULTS],
        ("n_w_zero", FSCORE_W, dict(n_w=0)),
        ("origin_source_unknown", FSCORE, dict(origin_source=-1)),
        ("origins_host_null", FSCORE, dict(origin_source=HOST)),
        ("n_origins_zero", FSCORE, dict(n_origins=0)),
        ("horizon_zero", FSCORE, dict(horizon=0)),
        ("too_many_columns", FSCORE, dict(n_origins=70000, horizon=70000)),
        ("truth_null", FSCORE, dict(truth=None)),
        ("truth_infinite", FSCORE, dict(truth=np.array([[0, 0], [0, -math.inf], [0, 0]], np.float32))),
        ("truth_all_nan", FSCORE, dict(truth=np.full((3, 2), math.nan, np.float32))),
        ("n_levels_negative", FSCORE, dict(n_levels=-1)),
        ("n_levels_above_max", FSCORE, dict(FSCORE_LEVELS, n_levels=17)),
        ("levels_z_null", FSCORE, dict(FSCORE_LEVELS, levels_z=None)),
        ("quantiles_null", FSCORE, dict(FSCORE_LEVELS, quantiles=None)),
        ("quantiles_without_levels", FSCORE, dict(quantiles=f64(6))),
        ("level_one", FSCORE, dict(FSCORE_LEVELS, levels_p=np.array([0.1, 1.0]))),
        ("level_z_infinite", FSCORE, dict(FSCORE_LEVELS, levels_z=np.array([-math.inf, 1.28]))),
        ("crps_without_pair_term", FSCORE, dict(crps=f64(6))),
        ("energy_score_without_energy", FSCORE, dict(energy_score=f64(3))),
        ("energy_horizon_above_max", FSCORE, dict(energy=1, n_origins=1, horizon=2049, truth=f32(1, 2049))),
        ("noise_without_eta", FSCORE_W, dict(eta=None, noise=1)),
        ("multiplicity_negative", FSCORE_W, MULT_NEGATIVE),
        ("thin_zero_and_origin_source_unknown", FSCORE, dict(thin=0, origin_source=-1)),
        ("origins_host_null_and_n_origins_zero", FSCORE, dict(origin_source=HOST, n_origins=0)),
        ("n_origins_zero_and_horizon_zero", FSCORE, dict(n_origins=0, horizon=0)),
        ("horizon_zero_and_truth_null", FSCORE, dict(horizon=0, truth=None)),
        ("horizon_zero_and_n_levels_negative", FSCORE, dict(horizon=0, n_levels=-1)),
        ("truth_null_and_n_levels_negative", FSCORE, dict(truth=None, n_levels=-1)),
        ("truth_infinite_and_level_one", FSCORE, dict(FSCORE_LEVELS, truth=np.full((3, 2), math.inf, np.float32), levels_p=np.array([0.1, 1.0]))),
        ("truth_all_nan_and_quantiles_without_levels", FSCORE, dict(truth=np.full((3, 2), math.nan, np.float32), quantiles=f64(6))),
        ("level_one_and_crps_without_pair_term", FSCORE, dict(FSCORE_LEVELS, levels_p=np.array([0.1, 1.0]), crps=f64(6))),
        ("crps_without_pair_term_and_energy_score_without_energy", FSCORE, dict(crps=f64(6), energy_score=f64(3))),
        ("energy_score_without_energy_and_noise_without_eta", FSCORE_W, dict(energy_score=f64(3), eta=None, noise=1)),
        ("noise_without_eta_and_multiplicity_negative", FSCORE_W, dict(MULT_NEGATIVE, eta=None, noise=1)),
    ]),
    "mbar": ("MbarSpec", "ptnn_mbar", [
        ("valid_trace", MBAR, dict(n_prior=10, replicas=i32(0, 1), n_replicas=2)),
        ("valid_host", MBAR_W, dict(multiplicity=np.array([[1, 0, 2, 1], [4, 0, 0, 0]], np.int32), x_source=TRAIN, n_rows=5, mean=f64(5),
                                    n_resample=4, resample_item=i64(0, 0, 0, 0), resample_w=f32(4, 3), n_prior=3, effective=1)),
        ("valid_u", MBAR_U, dict(MBAR_PRIOR, b=f64(2, 4), b_prior=f64(3), multiplicity=np.array([[1, 0, 2, 1], [4, 0, 0, 0]], np.int32),
                                 u=_nan_at(f64(2, 4), 1, 2), x_source=7)),
        ("w_and_u", MBAR_U, dict(w=f32(2, 4, 3))),
        ("b_without_u", MBAR_W, dict(b=f64(2, 4))),
        ("n_rungs_zero", MBAR_U, dict(n_rungs=0)),
        ("betas_null", MBAR_U, dict(betas=None)),
        ("n_per_rung_zero", MBAR_W, dict(n_per_rung=0)),
        ("no_source", MBAR, dict(nsteps=0)),
        *[(n, MBAR, f) for n, f in TRACE_FAULTS],
        ("n_replicas_not_n_rungs", MBAR, dict(replicas=i32(0, 1, 2), n_replicas=3)),
        ("beta_zero", MBAR_U, dict(betas=np.array([0.0, 1.0]))),
        ("beta_not_finite", MBAR_U, dict(betas=np.array([0.5, math.inf]))),
        ("betas_not_rising", MBAR_U, dict(betas=np.array([0.5, 0.5]))),
        ("n_prior_negative", MBAR, dict(n_prior=-1)),
        ("n_prior_above_int32", MBAR, dict(n_prior=1 << 31)),
        ("b_prior_without_u_prior", MBAR_U, dict(n_prior=3, b_prior=f64(3))),
        ("u_prior_without_n_prior", MBAR_U, dict(u_prior=f64(3))),
        ("too_many_states", MBAR_U, dict(n_prior=1, n_rungs=512, betas=np.arange(1, 513) / 512.0, u=f64(512, 4))),
        ("target_beta_below_the_ladder", MBAR_U, dict(target_beta=0.25)),
        ("target_beta_nan", MBAR_U, dict(target_beta=math.nan)),
        ("tol_zero", MBAR_U, dict(tol=0.0)),
        ("tol_inf", MBAR_U, dict(tol=math.inf)),
        ("max_iter_zero", MBAR_U, dict(max_iter=0)),
        ("n_resample_negative", MBAR_U, dict(n_resample=-1)),
        ("resample_item_without_n_resample", MBAR_U, dict(resample_item=i64(0, 0))),
        ("cum_weight_without_n_resample", MBAR_U, dict(cum_weight=f64(8))),
        ("mean_with_u", MBAR_U, dict(mean=f64(5), x_source=TRAIN, n_rows=5)),
        ("var_with_u_prior", MBAR_W, dict(MBAR_PRIOR, var=f64(5), x_source=TRAIN, n_rows=5)),
        ("resample_w_with_u", MBAR_U, dict(n_resample=2, resample_w=f32(2, 3))),
        ("resample_w_without_n_resample", MBAR_W, dict(resample_w=f32(2, 3))),
        ("mean_n_rows_zero", MBAR_W, dict(mean=f64(5), x_source=TRAIN)),
        ("mean_x_source_unknown", MBAR_W, dict(mean=f64(5), x_source=7, n_rows=5)),
        ("mean_x_host_null", MBAR_W, dict(mean=f64(5), x_source=HOST, n_rows=5)),
        ("u_prior_not_finite", MBAR_U, dict(MBAR_PRIOR, u_prior=_nan_at(f64(3), 1))),
        ("b_prior_not_finite", MBAR_U, dict(MBAR_PRIOR, b_prior=_nan_at(f64(3), 2))),
        ("too_many_host_rows", MBAR_W, dict(n_per_rung=1 << 30)),
        ("multiplicity_negative", MBAR_U, MBAR_MULT_NEGATIVE),
        ("u_not_finite", MBAR_U, dict(u=_nan_at(f64(2, 4), 1, 2))),
        ("b_not_finite", MBAR_U, dict(b=_nan_at(f64(2, 4), 0, 3))),
        ("w_and_u_and_b_without_u", MBAR_U, dict(w=f32(2, 4, 3), b=f64(2, 4))),
        ("n_rungs_zero_and_betas_null", MBAR_U, dict(n_rungs=0, betas=None)),
        ("betas_null_and_n_per_rung_zero", MBAR_U, dict(betas=None, n_per_rung=0)),
        ("n_per_rung_zero_and_betas_not_rising", MBAR_U, dict(n_per_rung=0, betas=np.array([0.5, 0.5]))),
        ("no_source_and_beta_zero", MBAR, dict(nsteps=0, betas=np.array([0.0, 1.0]))),
        ("betas_not_rising_and_multiplicity_negative", MBAR_U, dict(MBAR_MULT_NEGATIVE, betas=np.array([0.5, 0.5]))),
        ("betas_not_rising_and_u_prior_not_finite", MBAR_U, dict(MBAR_PRIOR, betas=np.array([1.0, 0.5]), u_prior=_nan_at(f64(3), 0))),
        ("beta_zero_and_n_prior_negative", MBAR_U, dict(betas=np.array([0.0, 1.0]), n_prior=-1)),
        ("n_per_rung_zero_and_u_prior_without_n_prior", MBAR_U, dict(n_per_rung=0, u_prior=f64(3))),
        ("u_prior_without_n_prior_and_target_beta_nan", MBAR_U, dict(u_prior=f64(3), target_beta=math.nan)),
        ("mean_with_u_and_u_prior_not_finite", MBAR_U, dict(MBAR_PRIOR, mean=f64(5), x_source=TRAIN, n_rows=5, u_prior=_nan_at(f64(3), 0))),
        ("u_prior_not_finite_and_multiplicity_negative", MBAR_U, dict(MBAR_PRIOR, **MBAR_MULT_NEGATIVE, u_prior=_nan_at(f64(3), 1))),
        ("u_prior_not_finite_and_n_per_rung_above_int32", MBAR_U, dict(MBAR_PRIOR, u_prior=_nan_at(f64(3), 1), n_per_rung=1 << 30)),
        ("multiplicity_negative_and_u_not_finite", MBAR_U, dict(MBAR_MULT_NEGATIVE, u=_nan_at(f64(2, 4), 0, 0))),
    ]),
}
SPEC_FAULTS = ("null_spec", "struct_bytes_zero", "struct_bytes_off_by_one")       # the first check of every call
POINTER_OF = {np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32,
              np.dtype(np.int64): C.c_int64, np.dtype(np.uint64): C.c_uint64}


def _lib():
    sys.path.insert(0, ROOT)
    import ptnn_amd  # noqa: F401
    from ptnn_amd import _lib
    return _lib


def _build(cls, base, over):
    """The structure with struct_bytes and the fields of `base` overridden by `over` -> (spec, the arrays it points to)."""
    spec, keep, types = cls(), [], dict(cls._fields_)
    spec.struct_bytes = C.sizeof(cls)
    for name, v in {**base, **over}.items():
        if isinstance(v, np.ndarray):
            assert types[name] == C.POINTER(POINTER_OF[v.dtype]), (name, v.dtype)
            keep.append(np.ascontiguousarray(v))
            v = keep[-1].ctypes.data_as(types[name])
        setattr(spec, name, v)
    return spec, keep


def _refusal(binding, lib, call, case):
    """(return code, ptnn_last_error() text) of one case with a NULL handle."""
    cls_name, fn, cases = CASES[call]
    cls = getattr(binding, cls_name)
    if case in SPEC_FAULTS:
        spec, keep = _build(cls, {}, {})
        spec.struct_bytes = dict(struct_bytes_zero=0, struct_bytes_off_by_one=C.sizeof(cls) + 1).get(case, 0)
        arg = None if case == "null_spec" else C.byref(spec)
    else:
        (base, over), = [(b, o) for n, b, o in cases if n == case]
        spec, keep = _build(cls, base, over)
        arg = C.byref(spec)
    rc = getattr(lib, fn)(None, arg)
    return [rc, lib.ptnn_last_error().decode()]


def _layout(binding):
    return {cls_name: dict(sizeof=C.sizeof(getattr(binding, cls_name)),
                           fields={n: [getattr(getattr(binding, cls_name), n).offset, getattr(getattr(binding, cls_name), n).size]
                                   for n, _ in getattr(binding, cls_name)._fields_})
            for cls_name, _, _ in CASES.values()}


def _case_ids():
    return [(call, case) for call, (_, _, cases) in CASES.items() for case in SPEC_FAULTS + tuple(n for n, _, _ in cases)]


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__
    __graft_entry__.build()
    return _lib()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_case_table_is_the_recorded_one(golden):
    assert all(len({n for n, _, _ in CASES[call][2]}) == len(CASES[call][2]) for call in CASES)
    assert {call: sorted(golden["errors"][call]) for call in golden["errors"]} == \
        {call: sorted(case for c, case in _case_ids() if c == call) for call in CASES}


@pytest.mark.parametrize("call, case", _case_ids(), ids=lambda v: v)
def test_refusal_is_the_recorded_one(binding, golden, call, case):
    got = _refusal(binding, binding.load_library(), call, case)
    assert got == golden["errors"][call][case]
    if case.startswith("valid"):
        assert got[0] < 0 and "handle" in got[1].lower()                          # every argument check passed: the handle is next


def test_structure_layouts_are_the_recorded_ones(binding, golden):
    assert _layout(binding) == golden["layout"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: PTNN_LIBRARY=<the parent commit's libptnn.so> python tests/test_analysis_errors_cpu.py --record")
    if not os.environ.get("PTNN_LIBRARY"):
        sys.exit("--record reads the library of the parent commit: set PTNN_LIBRARY to it")
    b = _lib()
    lb = b.load_library()
    doc = dict(errors={call: {} for call in CASES}, layout=_layout(b))
    for call_, case_ in _case_ids():
        doc["errors"][call_][case_] = _refusal(b, lb, call_, case_)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in doc['errors'].values())} cases recorded in {GOLDEN}")
