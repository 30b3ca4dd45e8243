"""ctypes binding of libptnn.so (include/ptnn.h).  No fallback: a missing library or device raises PtnnError."""
import ctypes as C
import math
import os
from statistics import NormalDist

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 4
TASK_REG, TASK_CLS = 0, 1


class PtnnError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_int32), ("device_id", C.c_int32), ("task", C.c_int32),
        ("n_in", C.c_int32), ("n_hidden", C.c_int32), ("n_out", C.c_int32),
        ("n_replicas_local", C.c_int32), ("n_replicas_global", C.c_int32), ("first_global_replica", C.c_int32),
        ("n_samples", C.c_int32), ("swap_interval", C.c_int32), ("pt_switch_step", C.c_int32),
        ("use_langevin", C.c_int32), ("waves_per_replica", C.c_int32), ("schedule", C.c_int32), ("groups_per_replica", C.c_int32), ("trace_capacity", C.c_int32), ("forward_bf16", C.c_int32), ("swap_rule", C.c_int32), ("shared_noise", C.c_int32), ("label_swap", C.c_int32), ("shared_device", C.c_int32), ("reserved_", C.c_int32),
        ("l_prob", C.c_float), ("learn_rate", C.c_float), ("step_w", C.c_float), ("step_eta", C.c_float),
        ("sigma_squared", C.c_float), ("nu_1", C.c_float), ("nu_2", C.c_float),
        ("seed", C.c_uint64),
    ]


PREDICT_X_HOST, PREDICT_X_TRAIN, PREDICT_X_TEST = 0, 1, 2
PREDICT_MAX_RANKS = 16

# the six leading fields of every analysis spec: its size, then the trace selection
_SELECTION = [("struct_bytes", C.c_int32), ("replicas", C.POINTER(C.c_int32)), ("n_replicas", C.c_int32), ("step0", C.c_int32),
              ("nsteps", C.c_int32), ("thin", C.c_int32)]


class PredictSpec(C.Structure):
    """ptnn_predict_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("reserved_", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("order_stats", C.POINTER(C.c_float)), ("vote", C.POINTER(C.c_double)),
        ("samples", C.POINTER(C.c_float)), ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


# scalar trace columns (PTNN_TR_* of include/ptnn.h) that ptnn_convergence takes as quantities
TR_LIKEH, TR_RMSE_TR, TR_RMSE_TE, TR_ACC_TR, TR_ACC_TE, TR_ACCEPT, TR_LOGALPHA, TR_SRC = range(8)


class ConvergenceSpec(C.Structure):
    """ptnn_convergence_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("params", C.POINTER(C.c_int32)), ("n_params", C.c_int32), ("scalars", C.c_int32),
        ("draws", C.POINTER(C.c_float)), ("n_chains", C.c_int32), ("n_draws", C.c_int32), ("n_quantities", C.c_int32),
        ("n_lags", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("var", C.POINTER(C.c_double)), ("r_hat", C.POINTER(C.c_double)), ("ess", C.POINTER(C.c_double)),
        ("trunc_lag", C.POINTER(C.c_int32)), ("ess_chain", C.POINTER(C.c_double)), ("rho", C.POINTER(C.c_double)),
    ]


RANK_MAX_PROBS, RANK_MAX_BINS = 16, 64


class RankConvergenceSpec(C.Structure):
    """ptnn_rank_convergence_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("params", C.POINTER(C.c_int32)), ("n_params", C.c_int32), ("scalars", C.c_int32),
        ("draws", C.POINTER(C.c_float)), ("n_chains", C.c_int32), ("n_draws", C.c_int32), ("n_quantities", C.c_int32),
        ("n_probs", C.c_int32), ("probs", C.POINTER(C.c_double)), ("n_bins", C.c_int32), ("reserved_", C.c_int32),
        ("r_hat_bulk", C.POINTER(C.c_double)), ("r_hat_tail", C.POINTER(C.c_double)), ("ess_bulk", C.POINTER(C.c_double)),
        ("ess_tail", C.POINTER(C.c_double)), ("ess_median", C.POINTER(C.c_double)), ("ess_quantile", C.POINTER(C.c_double)),
        ("ess_bulk_chain", C.POINTER(C.c_double)), ("ess_tail_chain", C.POINTER(C.c_double)), ("rank_hist", C.POINTER(C.c_int64)),
        ("z", C.POINTER(C.c_double)),
    ]


class ElpdSpec(C.Structure):
    """ptnn_elpd_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("loglik", C.POINTER(C.c_double)),
        ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("r_eff", C.c_double),
        ("lppd", C.POINTER(C.c_double)), ("p_waic", C.POINTER(C.c_double)), ("elpd_loo", C.POINTER(C.c_double)),
        ("khat", C.POINTER(C.c_double)), ("tail_len", C.POINTER(C.c_int64)), ("loglik_out", C.POINTER(C.c_double)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


ELPD_TAIL_CAP = 4096


class LfoSpec(C.Structure):
    """ptnn_lfo_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("loglik", C.POINTER(C.c_double)),
        ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("n_fit", C.c_int32), ("block", C.c_int32), ("origins", C.POINTER(C.c_int32)), ("n_origins", C.c_int32),
        ("r_eff", C.c_double),
        ("elpd_lfo", C.POINTER(C.c_double)), ("khat", C.POINTER(C.c_double)), ("tail_len", C.POINTER(C.c_int64)),
        ("loglik_out", C.POINTER(C.c_double)), ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]

FORECAST_ORIGIN_HOST, FORECAST_ORIGIN_TRAIN, FORECAST_ORIGIN_TEST = 0, 1, 2


class ForecastSpec(C.Structure):
    """ptnn_forecast_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("eta", C.POINTER(C.c_float)), ("n_w", C.c_int64),
        ("origin_source", C.c_int32), ("n_origins", C.c_int32), ("origins", C.POINTER(C.c_float)),
        ("horizon", C.c_int32), ("noise", C.c_int32), ("seed", C.c_uint64),
        ("ranks", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("reserved_", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("order_stats", C.POINTER(C.c_float)), ("samples", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_trajectories", C.POINTER(C.c_int64)),
    ]


class EvidenceSpec(C.Structure):
    """ptnn_evidence_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_double)), ("multiplicity", C.POINTER(C.c_int32)),
        ("n_rungs", C.c_int32), ("reserved_", C.c_int32), ("n_per_rung", C.c_int64), ("d", C.POINTER(C.c_double)),
        ("n_prior", C.c_int64), ("seed", C.c_uint64), ("a", C.POINTER(C.c_double)), ("n_a", C.c_int32), ("reserved2_", C.c_int32),
        ("u_mean", C.POINTER(C.c_double)), ("u_var", C.POINTER(C.c_double)), ("u_ess", C.POINTER(C.c_double)),
        ("log_stone", C.POINTER(C.c_double)), ("stone_relvar", C.POINTER(C.c_double)), ("n_draws", C.POINTER(C.c_int64)),
        ("prior_log_mean_exp", C.POINTER(C.c_double)), ("prior_kish_ess", C.POINTER(C.c_double)),
        ("prior_u_mean", C.POINTER(C.c_double)), ("prior_u_var", C.POINTER(C.c_double)),
        ("u_out", C.POINTER(C.c_double)), ("u_prior_out", C.POINTER(C.c_double)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


EVIDENCE_MAX_A = 4


class MbarSpec(C.Structure):
    """ptnn_mbar_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)), ("multiplicity", C.POINTER(C.c_int32)),
        ("n_rungs", C.c_int32), ("effective", C.c_int32), ("n_per_rung", C.c_int64), ("betas", C.POINTER(C.c_double)),
        ("n_prior", C.c_int64), ("seed", C.c_uint64), ("u_prior", C.POINTER(C.c_double)), ("b_prior", C.POINTER(C.c_double)),
        ("target_beta", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int32), ("reserved_", C.c_int32),
        ("n_resample", C.c_int64), ("resample_seed", C.c_uint64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("f", C.POINTER(C.c_double)), ("gram", C.POINTER(C.c_double)), ("n_eff", C.POINTER(C.c_double)),
        ("n_iter", C.POINTER(C.c_int64)), ("residual", C.POINTER(C.c_double)),
        ("u_out", C.POINTER(C.c_double)), ("b_out", C.POINTER(C.c_double)), ("log_weight", C.POINTER(C.c_double)),
        ("cum_weight", C.POINTER(C.c_double)),
        ("weight_sum", C.POINTER(C.c_double)), ("kish_ess", C.POINTER(C.c_double)), ("max_weight_share", C.POINTER(C.c_double)),
        ("resample_u", C.POINTER(C.c_double)), ("resample_item", C.POINTER(C.c_int64)), ("resample_w", C.POINTER(C.c_float)),
        ("mean", C.POINTER(C.c_double)), ("var", C.POINTER(C.c_double)),
        ("item_chain", C.POINTER(C.c_int32)), ("item_multiplicity", C.POINTER(C.c_int32)), ("item_step", C.POINTER(C.c_int64)),
        ("sse", C.POINTER(C.c_double)),
        ("n_items", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


MBAR_MAX_STATES = 512


class CalibrationSpec(C.Structure):
    """ptnn_calibration_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("levels_p", C.POINTER(C.c_double)), ("levels_z", C.POINTER(C.c_double)), ("n_levels", C.c_int32), ("pair_term", C.c_int32),
        ("pit", C.POINTER(C.c_double)), ("crps", C.POINTER(C.c_double)), ("pred_mean", C.POINTER(C.c_double)),
        ("pred_sd", C.POINTER(C.c_double)), ("quantiles", C.POINTER(C.c_double)), ("p_mean", C.POINTER(C.c_double)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


CALIB_MAX_LEVELS = 16
CALIB_MAX_DISTINCT = 65536


class ForecastScoreSpec(C.Structure):
    """ptnn_forecast_score_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("eta", C.POINTER(C.c_float)), ("n_w", C.c_int64),
        ("origin_source", C.c_int32), ("n_origins", C.c_int32), ("origins", C.POINTER(C.c_float)), ("truth", C.POINTER(C.c_float)),
        ("horizon", C.c_int32), ("noise", C.c_int32), ("seed", C.c_uint64),
        ("levels_p", C.POINTER(C.c_double)), ("levels_z", C.POINTER(C.c_double)), ("n_levels", C.c_int32), ("pair_term", C.c_int32),
        ("energy", C.c_int32), ("reserved_", C.c_int32),
        ("pit", C.POINTER(C.c_double)), ("crps", C.POINTER(C.c_double)), ("log_score", C.POINTER(C.c_double)),
        ("pred_mean", C.POINTER(C.c_double)), ("pred_sd", C.POINTER(C.c_double)), ("quantiles", C.POINTER(C.c_double)),
        ("energy_score", C.POINTER(C.c_double)), ("samples", C.POINTER(C.c_float)), ("means", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_trajectories", C.POINTER(C.c_int64)),
    ]


FSCORE_MAX_ENERGY_HORIZON = 2048


class SensitivitySpec(C.Structure):
    """ptnn_sensitivity_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("ranks2", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("n_ranks2", C.c_int32),
        ("grad_mean", C.POINTER(C.c_double)), ("order_stats", C.POINTER(C.c_float)),
        ("pos_count", C.POINTER(C.c_int64)), ("neg_count", C.POINTER(C.c_int64)),
        ("abs_mean", C.POINTER(C.c_double)), ("sq_mean", C.POINTER(C.c_double)), ("abs_order_stats", C.POINTER(C.c_float)),
        ("sample_abs", C.POINTER(C.c_float)), ("samples", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


class PdSpec(C.Structure):
    """ptnn_pd_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("inputs", C.POINTER(C.c_int32)), ("n_inputs", C.c_int32), ("n_grid", C.c_int32), ("grid", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("ranks2", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("n_ranks2", C.c_int32),
        ("ice_mean", C.POINTER(C.c_double)), ("ice_order_stats", C.POINTER(C.c_float)),
        ("pd_mean", C.POINTER(C.c_double)), ("pd_order_stats", C.POINTER(C.c_float)),
        ("range_mean", C.POINTER(C.c_double)), ("range_order_stats", C.POINTER(C.c_float)),
        ("sample_pd", C.POINTER(C.c_float)), ("sample_range", C.POINTER(C.c_float)), ("samples", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


PD_MAX_GRID = 64


class AleSpec(C.Structure):
    """ptnn_ale_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("inputs", C.POINTER(C.c_int32)), ("n_inputs", C.c_int32), ("n_edges", C.c_int32), ("edges", C.POINTER(C.c_float)),
        ("pairs", C.POINTER(C.c_int32)), ("n_pairs", C.c_int32), ("n_edges2", C.c_int32), ("edges2", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("ranks2", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("n_ranks2", C.c_int32),
        ("bin_count", C.POINTER(C.c_int64)), ("cell_count", C.POINTER(C.c_int64)),
        ("ale_mean", C.POINTER(C.c_double)), ("ale_order_stats", C.POINTER(C.c_float)),
        ("range_mean", C.POINTER(C.c_double)), ("range_order_stats", C.POINTER(C.c_float)),
        ("sample_ale", C.POINTER(C.c_float)), ("sample_range", C.POINTER(C.c_float)),
        ("ale2_mean", C.POINTER(C.c_double)), ("ale2_order_stats", C.POINTER(C.c_float)),
        ("inter_mean", C.POINTER(C.c_double)), ("inter_order_stats", C.POINTER(C.c_float)),
        ("sample_ale2", C.POINTER(C.c_float)), ("sample_inter", C.POINTER(C.c_float)),
        ("local_mean", C.POINTER(C.c_double)), ("local_order_stats", C.POINTER(C.c_float)), ("samples", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


ALE_MAX_EDGES, ALE_MAX_EDGES2, ALE_MAX_PAIRS = 64, 16, 16


class ShapSpec(C.Structure):
    """ptnn_shapley_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("background", C.POINTER(C.c_float)), ("masks", C.POINTER(C.c_uint64)), ("coef", C.POINTER(C.c_double)),
        ("n_background", C.c_int32), ("n_coalitions", C.c_int32), ("n_terms", C.c_int32), ("reserved_", C.c_int32),
        ("ranks", C.POINTER(C.c_int64)), ("ranks2", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("n_ranks2", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("order_stats", C.POINTER(C.c_float)),
        ("pos_count", C.POINTER(C.c_int64)), ("neg_count", C.POINTER(C.c_int64)),
        ("abs_mean", C.POINTER(C.c_double)), ("abs_order_stats", C.POINTER(C.c_float)),
        ("sample_abs", C.POINTER(C.c_float)), ("samples", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


SHAP_MAX_COALITIONS, SHAP_MAX_BACKGROUND, SHAP_MAX_TERMS, SHAP_MAX_ACC = 4096, 256, 64, 256


class PpcSpec(C.Structure):
    """ptnn_ppc_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("lags", C.POINTER(C.c_int32)), ("n_lags", C.c_int32), ("reserved_", C.c_int32), ("seed", C.c_uint64),
        ("n_defined", C.POINTER(C.c_int64)), ("n_greater", C.POINTER(C.c_int64)), ("n_equal", C.POINTER(C.c_int64)),
        ("mean_obs", C.POINTER(C.c_double)), ("mean_rep", C.POINTER(C.c_double)), ("var_rep", C.POINTER(C.c_double)),
        ("t_obs", C.POINTER(C.c_double)), ("t_rep", C.POINTER(C.c_double)),
        ("z", C.POINTER(C.c_float)), ("y_rep", C.POINTER(C.c_int32)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


PPC_MAX_LAGS = 16


class PowerscaleSpec(C.Structure):
    """ptnn_powerscale_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("groups", C.c_int32), ("reserved_", C.c_int32), ("delta", C.c_double), ("r_eff", C.c_double),
        ("sens", C.POINTER(C.c_double)), ("dist", C.POINTER(C.c_double)), ("mean", C.POINTER(C.c_double)), ("sd", C.POINTER(C.c_double)),
        ("base_mean", C.POINTER(C.c_double)), ("base_sd", C.POINTER(C.c_double)), ("khat", C.POINTER(C.c_double)),
        ("tail_len", C.POINTER(C.c_int64)), ("logp", C.POINTER(C.c_double)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)), ("n_quantities", C.POINTER(C.c_int64)),
    ]


POWERSCALE_GROUPS = {"weights": 1, "eta": 2, "predictions": 4, "loglik": 8}      # PTNN_POWERSCALE_*, in the order of the quantities
POWERSCALE_MAX_DISTINCT = 65536


class PriorSpec(C.Structure):
    """ptnn_prior_spec (include/ptnn.h)."""
    _fields_ = [
        ("struct_bytes", C.c_int32), ("n_scales", C.c_int32), ("sigma_squared", C.POINTER(C.c_double)),
        ("n_draws", C.c_int64), ("draw0", C.c_int64), ("seed", C.c_uint64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("has_target", C.c_int32), ("n_ranks", C.c_int32), ("ranks", C.POINTER(C.c_int64)), ("eps", C.c_double),
        ("mean", C.POINTER(C.c_double)), ("order_stats", C.POINTER(C.c_float)), ("vote", C.POINTER(C.c_double)),
        ("sat_count", C.POINTER(C.c_int64)),
        ("t_obs", C.POINTER(C.c_double)), ("stat_mean", C.POINTER(C.c_double)), ("stat_sd", C.POINTER(C.c_double)),
        ("stat_order_stats", C.POINTER(C.c_float)),
        ("n_greater", C.POINTER(C.c_int64)), ("n_equal", C.POINTER(C.c_int64)), ("n_defined", C.POINTER(C.c_int64)),
        ("t_draw", C.POINTER(C.c_double)), ("samples", C.POINTER(C.c_float)), ("weights", C.POINTER(C.c_float)),
        ("n_stats", C.POINTER(C.c_int64)), ("n_blocks", C.POINTER(C.c_int64)),
    ]


PRIOR_MAX_SCALES = 8
PRIOR_REG_STATS, PRIOR_CLS_FIXED = 7, 4       # statistics of a drawn function: a regression's; a classification's before class_share


class ClassReportSpec(C.Structure):
    """ptnn_class_report_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("auc", C.c_int32),
        ("p_mean", C.POINTER(C.c_double)), ("vote", C.POINTER(C.c_double)), ("p_correct", C.POINTER(C.c_double)),
        ("metric_mean", C.POINTER(C.c_double)), ("metric_order_stats", C.POINTER(C.c_float)), ("confusion_sum", C.POINTER(C.c_int64)),
        ("sample_metrics", C.POINTER(C.c_float)), ("sample_confusion", C.POINTER(C.c_int32)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


REPORT_MAX_AUC_ROWS = 16384


class UncertaintySpec(C.Structure):
    """ptnn_uncertainty_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("ranks", C.POINTER(C.c_int64)), ("n_ranks", C.c_int32), ("reserved_", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("vote", C.POINTER(C.c_double)), ("entropy_mean", C.POINTER(C.c_double)),
        ("entropy_order_stats", C.POINTER(C.c_float)), ("sample_entropy", C.POINTER(C.c_float)),
        ("epistemic_var", C.POINTER(C.c_double)), ("aleatoric_var", C.POINTER(C.c_double)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


class InfluenceSpec(C.Structure):
    """ptnn_influence_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("eta", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("target_values", C.POINTER(C.c_float)), ("loglik", C.POINTER(C.c_double)), ("n_a", C.c_int32), ("n_b", C.c_int32),
        ("case_source", C.c_int32), ("n_cases", C.c_int32), ("case_x", C.POINTER(C.c_float)),
        ("target_kind", C.c_int32), ("target_source", C.c_int32), ("n_targets", C.c_int32), ("reserved_", C.c_int32),
        ("target_x", C.POINTER(C.c_float)),
        ("cov", C.POINTER(C.c_double)), ("target_mean", C.POINTER(C.c_double)), ("target_var", C.POINTER(C.c_double)),
        ("case_mean", C.POINTER(C.c_double)), ("case_var", C.POINTER(C.c_double)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


INFLUENCE_OUTPUT, INFLUENCE_LOGLIK = 0, 1
INFLUENCE_MAX_ELEMENTS = 1 << 27
INFLUENCE_KCHUNK = 512                   # distinct samples per partial sum (csrc/ptnn_dev_influence.hpp: INFL_KCHUNK)


class ModesSpec(C.Structure):
    """ptnn_modes_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("values", C.POINTER(C.c_float)), ("n_a", C.c_int32), ("reserved_", C.c_int32), ("near_sq", C.c_double),
        ("room", C.c_int64), ("rho", C.POINTER(C.c_int64)), ("delta_sq", C.POINTER(C.c_double)), ("parent", C.POINTER(C.c_int32)),
        ("count", C.POINTER(C.c_int32)), ("item_sample", C.POINTER(C.c_int32)), ("spread_sq", C.POINTER(C.c_double)),
        ("sq_dist", C.POINTER(C.c_double)), ("outputs", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


MODES_MAX_ELEMENTS = 1 << 27
MODES_MAX_DISTINCT = math.isqrt(MODES_MAX_ELEMENTS)      # 11585: the largest U with U * U <= MODES_MAX_ELEMENTS


class CompressSpec(C.Structure):
    """ptnn_compress_spec (include/ptnn.h)."""
    _fields_ = _SELECTION + [
        ("w", C.POINTER(C.c_float)), ("multiplicity", C.POINTER(C.c_int32)), ("n_w", C.c_int64),
        ("x_source", C.c_int32), ("n_rows", C.c_int32), ("x", C.POINTER(C.c_float)),
        ("values", C.POINTER(C.c_float)), ("n_a", C.c_int32), ("m", C.c_int32),
        ("subset_items", C.POINTER(C.c_int32)), ("n_subsets", C.c_int32), ("subset_size", C.c_int32),
        ("room", C.c_int64), ("picks", C.POINTER(C.c_int32)), ("energy", C.POINTER(C.c_double)), ("pick_score", C.POINTER(C.c_double)),
        ("mu", C.POINTER(C.c_double)), ("d0", C.POINTER(C.c_double)), ("subset_energy", C.POINTER(C.c_double)),
        ("count", C.POINTER(C.c_int32)), ("item_sample", C.POINTER(C.c_int32)),
        ("sq_dist", C.POINTER(C.c_double)), ("outputs", C.POINTER(C.c_float)),
        ("n_samples", C.POINTER(C.c_int64)), ("n_distinct", C.POINTER(C.c_int64)),
    ]


COMPRESS_MAX_SUBSET = 65536              # entries of one evaluated subset (include/ptnn.h: subset_size)


class LadderAdaptSpec(C.Structure):
    """ptnn_ladder_adapt_spec (include/ptnn.h)."""
    _fields_ = [("struct_bytes", C.c_int32), ("rounds", C.c_int32), ("kappa0", C.c_double), ("t0", C.c_double)]


def library_path():
    return os.environ.get("PTNN_LIBRARY", os.path.join(_HERE, "libptnn.so"))


_lib = None

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_vpp = C.POINTER(C.c_void_p)

# callbacks of the host-staged transport (ptnn_all_gather_fn / ptnn_send_recv_fn of include/ptnn.h)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
SEND_RECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _ip, _ip, _vpp, C.c_int64)
XCHG_AUTO, XCHG_GATHER, XCHG_BOUNDARY = 0, 1, 2
UNIQUE_ID_BYTES = 128

# every symbol include/ptnn.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ptnn_abi_version": (C.c_int, []),
    "ptnn_last_error": (C.c_char_p, []),
    "ptnn_supports": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ptnn_create": (C.c_int, [C.POINTER(Config), _vpp]),
    "ptnn_destroy": (C.c_int, [C.c_void_p]),
    "ptnn_set_data": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, C.c_int, C.c_int]),
    "ptnn_set_state": (C.c_int, [C.c_void_p, _fp, _fp]),
    "ptnn_set_ladder": (C.c_int, [C.c_void_p, _fp]),
    "ptnn_set_ladder_adaptation": (C.c_int, [C.c_void_p, C.POINTER(LadderAdaptSpec)]),
    "ptnn_get_ladder_history": (C.c_int, [C.c_void_p, _fp, _fp, _ip]),
    "ptnn_get_ladder_adaptation": (C.c_int, [C.c_void_p, C.POINTER(LadderAdaptSpec)]),
    "ptnn_run": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_sync": (C.c_int, [C.c_void_p]),
    "ptnn_steps_done": (C.c_int, [C.c_void_p]),
    "ptnn_comm_unique_id": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "ptnn_comm_probe": (C.c_int, [_ip, C.c_int, C.POINTER(C.c_double)]),
    "ptnn_comm_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip]),
    "ptnn_comm_last_stage": (C.c_int, [C.c_char_p, C.c_int]),
    "ptnn_comm_init_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptnn_comm_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_comm_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    "ptnn_comm_finalize": (C.c_int, [C.c_void_p]),
    "ptnn_route": (C.c_int, [_ip, C.c_int, C.c_int, C.c_int, _ip, C.c_int]),
    "ptnn_run_segment": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "ptnn_swap_L_ptr": (C.c_int, [C.c_void_p, C.c_int, _vpp]),
    "ptnn_swap_set_L": (C.c_int, [C.c_void_p, C.c_int, _fp]),
    "ptnn_swap_cascade": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "ptnn_swap_row_ptr": (C.c_int, [C.c_void_p, C.c_int, _vpp, _vpp]),
    "ptnn_state_row_floats": (C.c_int, [C.c_void_p]),
    "ptnn_stream": (C.c_int, [C.c_void_p, _vpp]),
    "ptnn_swap_apply": (C.c_int, [C.c_void_p, _ip, C.c_int]),
    "ptnn_xchg_ptr": (C.c_int, [C.c_void_p, _vpp, _ip]),
    "ptnn_swap_pack": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_swap_apply_gathered": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_get_traces": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _ip]),
    "ptnn_get_trace_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp]),
    "ptnn_get_swap_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    "ptnn_get_swap_log": (C.c_int, [C.c_void_p, _ip, C.c_int]),
    "ptnn_get_state": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, _ip, _ip, _ip]),
    "ptnn_get_labels": (C.c_int, [C.c_void_p, _ip]),
    "ptnn_checkpoint_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ptnn_checkpoint_save": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "ptnn_checkpoint_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "ptnn_evaluate": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp]),
    "ptnn_langevin_gradient": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp]),
    "ptnn_time_sgd_epoch": (C.c_int, [C.c_void_p, _fp, C.c_int, C.POINTER(C.c_double)]),
    "ptnn_time_tree_round": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "ptnn_tape": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp, _fp]),
    "ptnn_describe": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "ptnn_kernel_time": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "ptnn_debug_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptnn_text_round": (C.c_int, [C.POINTER(C.c_double), C.c_int64, C.c_char_p]),
    "ptnn_savetxt": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.c_int64, C.c_int64, C.c_char_p]),
    "ptnn_savetxt_f32": (C.c_int, [C.c_char_p, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int]),
    "ptnn_text_round_f32": (C.c_int, [_fp, C.POINTER(C.c_double), C.c_int64, C.c_char_p]),
    "ptnn_posterior_matrix": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_int]),
    "ptnn_savetxt_f32_batch": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(_fp), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_char_p), C.c_int, C.c_int]),
    "ptnn_trace_image": (C.c_int, [C.c_void_p, C.POINTER(_fp), _ip, C.POINTER(_fp)]),
    "ptnn_trace_image_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ptnn_trace_image_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "ptnn_predict": (C.c_int, [C.c_void_p, C.POINTER(PredictSpec)]),
    "ptnn_convergence": (C.c_int, [C.c_void_p, C.POINTER(ConvergenceSpec)]),
    "ptnn_rank_convergence": (C.c_int, [C.c_void_p, C.POINTER(RankConvergenceSpec)]),
    "ptnn_elpd": (C.c_int, [C.c_void_p, C.POINTER(ElpdSpec)]),
    "ptnn_lfo": (C.c_int, [C.c_void_p, C.POINTER(LfoSpec)]),
    "ptnn_forecast": (C.c_int, [C.c_void_p, C.POINTER(ForecastSpec)]),
    "ptnn_evidence": (C.c_int, [C.c_void_p, C.POINTER(EvidenceSpec)]),
    "ptnn_mbar": (C.c_int, [C.c_void_p, C.POINTER(MbarSpec)]),
    "ptnn_calibration": (C.c_int, [C.c_void_p, C.POINTER(CalibrationSpec)]),
    "ptnn_forecast_score": (C.c_int, [C.c_void_p, C.POINTER(ForecastScoreSpec)]),
    "ptnn_sensitivity": (C.c_int, [C.c_void_p, C.POINTER(SensitivitySpec)]),
    "ptnn_partial_dependence": (C.c_int, [C.c_void_p, C.POINTER(PdSpec)]),
    "ptnn_accumulated_effects": (C.c_int, [C.c_void_p, C.POINTER(AleSpec)]),
    "ptnn_coalition_values": (C.c_int, [C.c_void_p, C.POINTER(ShapSpec)]),
    "ptnn_ppc": (C.c_int, [C.c_void_p, C.POINTER(PpcSpec)]),
    "ptnn_powerscale": (C.c_int, [C.c_void_p, C.POINTER(PowerscaleSpec)]),
    "ptnn_prior_predictive": (C.c_int, [C.c_void_p, C.POINTER(PriorSpec)]),
    "ptnn_class_report": (C.c_int, [C.c_void_p, C.POINTER(ClassReportSpec)]),
    "ptnn_uncertainty": (C.c_int, [C.c_void_p, C.POINTER(UncertaintySpec)]),
    "ptnn_influence": (C.c_int, [C.c_void_p, C.POINTER(InfluenceSpec)]),
    "ptnn_modes": (C.c_int, [C.c_void_p, C.POINTER(ModesSpec)]),
    "ptnn_compress": (C.c_int, [C.c_void_p, C.POINTER(CompressSpec)]),
}


def load_library():
    """dlopen libptnn.so and declare every prototype.  Loading does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise PtnnError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError here = header and library out of step
        fn.restype, fn.argtypes = res, args
    if lib.ptnn_abi_version() != ABI_VERSION:
        raise PtnnError(f"libptnn ABI {lib.ptnn_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, typ=_fp):
    return None if a is None else a.ctypes.data_as(typ)


def _spec(cls):
    """A zeroed spec structure of an analysis call, its struct_bytes set."""
    spec = cls()
    spec.struct_bytes = C.sizeof(cls)
    return spec


def _ranks(spec, keep, ranks, fields=("ranks", "n_ranks")):
    """0-based ranks of order statistics -> the spec's pointer and count fields (named by `fields`); returns the count."""
    rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    keep.append(rk)
    setattr(spec, fields[0], _ptr(rk, C.POINTER(C.c_int64)) if rk.size else None)
    setattr(spec, fields[1], rk.size)
    return rk.size


_POINTER_OF = {np.dtype(np.float64): C.POINTER(C.c_double), np.dtype(np.float32): _fp, np.dtype(np.int64): C.POINTER(C.c_int64),
               np.dtype(np.int32): _ip}


def _bind(spec, out, **fields):
    """The output arrays of `out` -> the spec's pointer fields of the same names (`fields`: the field of a key named otherwise),
    each typed by its array's dtype; None stays NULL."""
    for k, v in out.items():
        setattr(spec, fields.get(k, k), None if v is None else _ptr(v, _POINTER_OF[v.dtype]))


def comm_unique_id():
    """ncclGetUniqueId through libptnn (loads librccl.so): 128 bytes rank 0 hands to every rank."""
    lib = load_library()
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    if lib.ptnn_comm_unique_id(buf, UNIQUE_ID_BYTES) < 0:
        raise PtnnError(lib.ptnn_last_error().decode())
    return buf.raw


def comm_probe(devices):
    """ptnn_comm_probe: one bounded RCCL round trip among `devices` IN THIS PROCESS -> seconds it took; raises PtnnError with the
    stage that failed.  Callers want distributed.rccl_probe(), which runs this in a fresh child process."""
    lib = load_library()
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    sec = C.c_double()
    if lib.ptnn_comm_probe(_ptr(dev, _ip), int(dev.size), C.byref(sec)) < 0:
        raise PtnnError(lib.ptnn_last_error().decode())
    return sec.value


def comm_last_stage():
    """The last stage a communicator bring-up / exchange entered in this process (text), for error reports."""
    lib = load_library()
    buf = C.create_string_buffer(256)
    lib.ptnn_comm_last_stage(buf, 256)
    return buf.value.decode()


def route(src, n_local, rank):
    """ptnn_route: the rows `rank` receives / sends for the permutation src -> (recvs, sends), each a list of
    (local row, peer rank, global destination slot) in ascending global destination slot.  Pure host function."""
    lib = load_library()
    src = np.ascontiguousarray(src, dtype=np.int32)
    msg = np.empty((src.size + 1, 4), np.int32)
    n = lib.ptnn_route(_ptr(src, _ip), src.size, int(n_local), int(rank), _ptr(msg, _ip), msg.shape[0])
    if n < 0:
        raise PtnnError(lib.ptnn_last_error().decode())
    recvs = [(int(m[2]), int(m[1]), int(m[3])) for m in msg[:n] if m[0] == 0]
    sends = [(int(m[2]), int(m[1]), int(m[3])) for m in msg[:n] if m[0] == 1]
    return recvs, sends


class Sampler:
    """Thin object wrapper over a ptnn_handle (one GPU, one contiguous block of the ladder)."""

    def __init__(self, **kw):
        self.lib = load_library()
        cfg = Config()
        cfg.struct_bytes = C.sizeof(Config)
        for k, v in kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.P = cfg.n_in * cfg.n_hidden + cfg.n_hidden * cfg.n_out + cfg.n_hidden + cfg.n_out
        self.R = cfg.n_replicas_local
        self.S = cfg.n_samples
        h = C.c_void_p()
        self._check(self.lib.ptnn_create(C.byref(cfg), C.byref(h)))
        self.h = h

    def _check(self, rc):
        if rc < 0:
            raise PtnnError(self.lib.ptnn_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.ptnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, train, test):
        tr, te = _f32(train), _f32(test)
        if tr.ndim != 2 or te.ndim != 2 or tr.shape[1] != te.shape[1]:
            raise ValueError("train/test must be 2-D with the same number of columns")
        self._check(self.lib.ptnn_set_data(self.h, _ptr(tr), tr.shape[0], _ptr(te), te.shape[0], tr.shape[1]))
        self.ntr, self.nte = tr.shape[0], te.shape[0]

    def set_state(self, w0, temperatures):
        w0, t = _f32(w0), _f32(temperatures)
        if w0.shape != (self.R, self.P) or t.shape != (self.R,):
            raise ValueError(f"w0 must be [{self.R},{self.P}], temperatures [{self.R}]")
        self._check(self.lib.ptnn_set_state(self.h, _ptr(w0), _ptr(t)))

    def set_ladder(self, temperatures_global):
        t = _f32(temperatures_global)
        if t.shape != (self.cfg.n_replicas_global,):
            raise ValueError("temperatures_global must have n_replicas_global entries")
        self._check(self.lib.ptnn_set_ladder(self.h, _ptr(t)))

    def set_ladder_adaptation(self, rounds, kappa0, t0):
        """Adapt the ladder over the first `rounds` swap rounds (swap_rule 1; ptnn_set_ladder_adaptation); rounds = 0 records the
        per-pair acceptances only."""
        spec = LadderAdaptSpec(C.sizeof(LadderAdaptSpec), int(rounds), float(kappa0), float(t0))
        self._check(self.lib.ptnn_set_ladder_adaptation(self.h, C.byref(spec)))

    def ladder_adaptation(self):
        """(rounds, kappa0, t0) of the adaptation the handle runs (a restored checkpoint's), or None."""
        spec = LadderAdaptSpec()
        if self._check(self.lib.ptnn_get_ladder_adaptation(self.h, C.byref(spec))) == 0:
            return None
        return spec.rounds, spec.kappa0, spec.t0

    def ladder_history(self):
        """(ladders [A+1, R_global] float32, accept [rounds run, R_global-1] float32): the ladder of every adapted round (row A =
        the frozen one) and a_k(t) of every round."""
        Rg = self.cfg.n_replicas_global
        spec = self.ladder_adaptation()              # the handle's own A: the buffer is sized from what the library will copy
        if spec is None:
            raise PtnnError("no ladder adaptation on this handle (set_ladder_adaptation)")
        A = spec[0]
        lad = np.empty((A + 1, Rg), np.float32)
        acc = np.empty((self.S // self.cfg.swap_interval + 2, Rg - 1), np.float32)
        n = C.c_int32()
        self._check(self.lib.ptnn_get_ladder_history(self.h, _ptr(lad), _ptr(acc), C.byref(n)))
        return lad, acc[:n.value].copy()

    def run(self, n_steps=-1):
        self._check(self.lib.ptnn_run(self.h, int(n_steps)))

    def sync(self):
        self._check(self.lib.ptnn_sync(self.h))

    def steps_done(self):
        return self.lib.ptnn_steps_done(self.h)

    # ---- sharded ladder: communicators ----
    def comm_init(self, unique_id, rank, nranks):
        """RCCL communicator over the ranks that own the blocks of this ladder (collective: every rank calls it)."""
        self._check(self.lib.ptnn_comm_init(self.h, unique_id, len(unique_id), int(rank), int(nranks)))

    def comm_init_host(self, rank, nranks, all_gather, send_recv):
        """Host-staged transport: all_gather(buf: uint8 array [nranks, bytes_per_rank]) fills the other ranks' blocks in place;
        send_recv(msgs: list of (peer, is_send, uint8 array)) completes all messages.  Exceptions become an error return."""
        def _ag(ctx, buf, nbytes):
            try:
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(int(nranks), int(nbytes)))
                all_gather(arr)
                return 0
            except Exception:                                   # noqa: BLE001 -- must not unwind through C
                import traceback
                traceback.print_exc()
                return -1

        def _sr(ctx, n, peer, is_send, bufs, nbytes):
            try:
                msgs = [(int(peer[k]), bool(is_send[k]),
                         np.ctypeslib.as_array(C.cast(bufs[k], C.POINTER(C.c_uint8)), shape=(int(nbytes),))) for k in range(n)]
                send_recv(msgs)
                return 0
            except Exception:                                   # noqa: BLE001
                import traceback
                traceback.print_exc()
                return -1
        self._callbacks = (ALL_GATHER_FN(_ag), SEND_RECV_FN(_sr))      # keep them alive as long as the handle
        self._check(self.lib.ptnn_comm_init_host(self.h, int(rank), int(nranks), C.cast(self._callbacks[0], C.c_void_p),
                                                 C.cast(self._callbacks[1], C.c_void_p), None))

    def comm_set_mode(self, mode):
        self._check(self.lib.ptnn_comm_set_mode(self.h, int(mode)))

    def comm_stats(self):
        a, b, r, m = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.ptnn_comm_stats(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(m)))
        return dict(bytes_sent=a.value, bytes_received=b.value, rounds=r.value, mode={0: "none", 1: "gather", 2: "boundary"}[m.value])

    def comm_info(self):
        """What is attached to the handle: transport, rank, ranks as the communicator reports them, device (ptnn_comm_info)."""
        t, r, n, d = (C.c_int32() for _ in range(4))
        self._check(self.lib.ptnn_comm_info(self.h, C.byref(t), C.byref(r), C.byref(n), C.byref(d)))
        return dict(transport={0: "none", 1: "rccl", 2: "host"}[t.value], rank=r.value, nranks=n.value, device=d.value)

    def comm_finalize(self):
        self._check(self.lib.ptnn_comm_finalize(self.h))

    def run_segment(self):
        ho = C.c_int(0)
        self._check(self.lib.ptnn_run_segment(self.h, C.byref(ho)))
        return ho.value

    def swap_L_ptr(self, phantom):
        p = C.c_void_p()
        self._check(self.lib.ptnn_swap_L_ptr(self.h, int(phantom), C.byref(p)))
        return p.value

    def swap_set_L(self, L, phantom=0):
        L = _f32(L)
        if L.shape != (self.cfg.n_replicas_global,):
            raise ValueError("L must have n_replicas_global entries")
        self._check(self.lib.ptnn_swap_set_L(self.h, int(phantom), _ptr(L)))

    def swap_cascade(self, phantom):
        src = np.empty(self.cfg.n_replicas_global, dtype=np.int32)
        self._check(self.lib.ptnn_swap_cascade(self.h, int(phantom), _ptr(src, _ip)))
        return src

    def swap_row_ptr(self, local_replica):
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.lib.ptnn_swap_row_ptr(self.h, int(local_replica), C.byref(a), C.byref(b)))
        return a.value, b.value

    def stream_ptr(self):
        p = C.c_void_p()
        self._check(self.lib.ptnn_stream(self.h, C.byref(p)))
        return p.value

    def state_row_floats(self):
        return self.lib.ptnn_state_row_floats(self.h)

    def swap_apply(self, src, phantom):
        src = np.ascontiguousarray(src, dtype=np.int32)
        self._check(self.lib.ptnn_swap_apply(self.h, _ptr(src, _ip), int(phantom)))

    def xchg_ptr(self):
        base, n = C.c_void_p(), C.c_int32()
        self._check(self.lib.ptnn_xchg_ptr(self.h, C.byref(base), C.byref(n)))
        return base.value, n.value

    def swap_pack(self, phantom):
        self._check(self.lib.ptnn_swap_pack(self.h, int(phantom)))

    def swap_apply_gathered(self, phantom):
        self._check(self.lib.ptnn_swap_apply_gathered(self.h, int(phantom)))

    def traces(self, step0=0, nsteps=None, pos_w=True):
        n = self.S - step0 if nsteps is None else nsteps
        out = {
            "pos_w": np.empty((self.R, n, self.P), np.float32) if pos_w else None,
            "likeh": np.empty((self.R, n), np.float32),
            "rmse_train": np.empty((self.R, n), np.float32), "rmse_test": np.empty((self.R, n), np.float32),
            "acc_train": np.empty((self.R, n), np.float32), "acc_test": np.empty((self.R, n), np.float32),
            "accept": np.empty((self.R, n), np.int32),
        }
        self._check(self.lib.ptnn_get_traces(self.h, step0, n, _ptr(out["pos_w"]), _ptr(out["likeh"]),
                                             _ptr(out["rmse_train"]), _ptr(out["rmse_test"]), _ptr(out["acc_train"]),
                                             _ptr(out["acc_test"]), _ptr(out["accept"], _ip)))
        return out

    # ---- trace images: the download overlapped with sampling (ptnn_trace_image*) ----
    def trace_image(self):
        """(pos_w, rows): numpy views of the handle's pinned host images -- pos_w [R, S, P] float32 (rows strided by the device's
        padded row), rows [R, S, 8] as trace_rows() describes them.  Valid until close(); filled by trace_fetch()."""
        pw, rw, rf = _fp(), _fp(), C.c_int32()
        self._check(self.lib.ptnn_trace_image(self.h, C.byref(pw), C.byref(rf), C.byref(rw)))
        pos = np.ctypeslib.as_array(pw, shape=(self.R, self.S, rf.value))[:, :, :self.P]
        rows = np.ctypeslib.as_array(rw, shape=(self.R, self.S, 8))
        return pos, rows

    def trace_fetch(self, row0, nrows):
        """Queues the copy of trace rows [row0, row0 + nrows) into the images behind the steps queued so far; returns a ticket."""
        return self._check(self.lib.ptnn_trace_image_fetch(self.h, int(row0), int(nrows)))

    def trace_wait(self, ticket):
        self._check(self.lib.ptnn_trace_image_wait(self.h, int(ticket)))

    def trace_rows(self, row0=0, nrows=None):
        """The scalar trace rows as the device keeps them (ptnn_get_trace_rows), [R, nrows, 8] float32."""
        n = self.S - row0 if nrows is None else nrows
        rows = np.empty((self.R, n, 8), np.float32)
        self._check(self.lib.ptnn_get_trace_rows(self.h, int(row0), int(n), _ptr(rows)))
        return rows

    def eta_trace(self):
        """Regression: eta = log tau^2 of the state recorded in every trace row, [R, S] (row i + 1 after MH step i; 0 before the
        first accepted step); classification has no eta: None."""
        if self.cfg.task != TASK_REG:
            return None
        return self.trace_rows()[:, :, 3].copy()

    def log_alpha(self, step0=0, nsteps=None):
        """log alpha of MH steps step0 .. step0+nsteps-1 as the kernel computed it, [R, nsteps] (row i + 1 belongs to step i)."""
        n = self.S - 1 - step0 if nsteps is None else nsteps
        rows = np.empty((self.R, n, 8), np.float32)
        self._check(self.lib.ptnn_get_trace_rows(self.h, step0 + 1, n, _ptr(rows)))
        return rows[:, :, 6].copy()

    def swap_stats(self):
        a, b, r = C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.ptnn_get_swap_stats(self.h, C.byref(a), C.byref(b), C.byref(r)))
        return a.value, b.value, r.value

    def swap_log(self, max_rounds=None):
        Rg = self.cfg.n_replicas_global
        cap = max_rounds or (self.S // self.cfg.swap_interval + 2)
        buf = np.empty((cap, Rg), np.int32)
        n = self._check(self.lib.ptnn_get_swap_log(self.h, _ptr(buf, _ip), cap))
        return buf[:n]

    def labels(self):
        lab = np.empty(self.cfg.n_replicas_global, np.int32)
        self._check(self.lib.ptnn_get_labels(self.h, _ptr(lab, _ip)))
        return lab

    def state(self):
        w = np.empty((self.R, self.P), np.float32)
        eta, lik, pri = (np.empty(self.R, np.float32) for _ in range(3))
        nacc, lg, lga = (np.zeros(self.R, np.int32) for _ in range(3))
        self._check(self.lib.ptnn_get_state(self.h, _ptr(w), _ptr(eta), _ptr(lik), _ptr(pri), _ptr(nacc, _ip), _ptr(lg, _ip),
                                            _ptr(lga, _ip)))
        return dict(w=w, eta=eta, likelihood=lik, prior=pri, num_accepted=nacc, langevin_count=lg, langevin_accepted=lga)

    def checkpoint(self):
        """State of the chains as bytes (ptnn_checkpoint_save); traces are not included."""
        n = C.c_int64()
        self._check(self.lib.ptnn_checkpoint_size(self.h, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        self._check(self.lib.ptnn_checkpoint_save(self.h, buf.ctypes.data_as(C.c_void_p), n.value))
        return buf.tobytes()

    def restore(self, blob):
        """Continue chains saved by checkpoint() (call after set_data, instead of set_state)."""
        buf = np.frombuffer(blob, np.uint8)
        self._check(self.lib.ptnn_checkpoint_load(self.h, buf.ctypes.data_as(C.c_void_p), buf.size))

    def evaluate(self, w, tau_sq=None):
        w = _f32(np.atleast_2d(w))
        n = w.shape[0]
        tau = None if tau_sq is None else _f32(np.broadcast_to(np.asarray(tau_sq, dtype=np.float32), (n,)))
        out = np.empty((n, 8), np.float32)
        self._check(self.lib.ptnn_evaluate(self.h, _ptr(w), _ptr(tau), n, _ptr(out)))
        return out

    def _rows(self, spec, keep, x, name, cols, fields=("x_source", "n_rows", "x")):
        """A rows argument of an analysis call: "train", "test" or an array [n, cols[0]] (cols[1] says what the columns are)
        -> the spec's source, count and pointer fields (named by `fields`)."""
        src_f, n_f, ptr_f = fields
        if isinstance(x, str):
            src = {"train": PREDICT_X_TRAIN, "test": PREDICT_X_TEST}.get(x)
            if src is None:
                raise ValueError(f"{name} must be 'train', 'test' or an array, not {x!r}")
            setattr(spec, src_f, src)
            setattr(spec, n_f, self.ntr if src == PREDICT_X_TRAIN else self.nte)
        else:
            xa = _f32(x)
            if xa.ndim != 2 or xa.shape[1] != cols[0]:
                raise ValueError(f"{name} must be [{n_f}, {cols[0]}] ({cols[1]}), got shape {xa.shape}")
            keep.append(xa)
            setattr(spec, src_f, PREDICT_X_HOST)
            setattr(spec, n_f, xa.shape[0])
            setattr(spec, ptr_f, _ptr(xa))

    def _trace_source(self, spec, keep, replicas, step0, nsteps, thin):
        """The trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all) -> (chains, rows per chain)."""
        nrep = self.R
        if replicas is not None:
            ra = np.ascontiguousarray(replicas, dtype=np.int32).reshape(-1)
            keep.append(ra)
            spec.replicas, spec.n_replicas = _ptr(ra, _ip), ra.size
            nrep = ra.size
        spec.step0 = int(step0)
        spec.nsteps = int(self.S - step0 if nsteps is None else nsteps)
        spec.thin = int(thin)
        return nrep, max(0, -(-spec.nsteps // max(1, spec.thin)))

    def _host_vectors(self, spec, keep, w, eta=None):
        """Host vectors w [n, P] and their eta [n] (optional) -> n."""
        wa = _f32(w)
        if wa.ndim != 2 or wa.shape[1] != self.P:
            raise ValueError(f"w must be [n, {self.P}], got shape {wa.shape}")
        keep.append(wa)
        spec.w, spec.n_w = _ptr(wa), wa.shape[0]
        if eta is not None:
            ea = _f32(np.reshape(eta, -1))
            if ea.shape != (wa.shape[0],):
                raise ValueError("eta must have one entry per vector")
            keep.append(ea)
            spec.eta = _ptr(ea)
        return wa.shape[0]

    @staticmethod
    def _multiplicity(spec, keep, multiplicity, shape, message):
        """Integer multiplicities of the host items (None = 1 each) -> the sample count; `message` may name {want} and {got}."""
        if multiplicity is None:
            return int(np.prod(shape))
        mu = np.ascontiguousarray(multiplicity, dtype=np.int32)
        if mu.shape != tuple(shape):
            raise ValueError(message.format(want=tuple(shape), got=mu.shape))
        keep.append(mu)
        spec.multiplicity = _ptr(mu, _ip)
        return int(np.maximum(mu, 0).astype(np.int64).sum())

    def _samples(self, spec, keep, *, w, eta=None, multiplicity, replicas, step0, nsteps, thin, unit):
        """The sample source of an analysis call: host vectors w [n, P] (eta [n] optional) with integer multiplicities (one
        entry per `unit`), else the trace rows -> the sample count."""
        if w is not None:
            n = self._host_vectors(spec, keep, w, eta)
            return self._multiplicity(spec, keep, multiplicity, (n,), f"multiplicity must have one entry per {unit}")
        return math.prod(self._trace_source(spec, keep, replicas, step0, nsteps, thin))

    def _pointwise_source(self, spec, keep, data, *, loglik, multiplicity, **source):
        """The sources of elpd() and lfo(): a host loglik [n, n_rows], else data rows with host vectors or trace rows -> the
        sample count."""
        if loglik is None:
            self._rows(spec, keep, data, "data", (self.cfg.n_in + 1, "n_in inputs and the target"))
            return self._samples(spec, keep, multiplicity=multiplicity, unit="sample", **source)
        la = np.ascontiguousarray(loglik, dtype=np.float64)
        if la.ndim != 2:
            raise ValueError(f"loglik must be [n_samples, n_rows], got shape {la.shape}")
        keep.append(la)
        spec.loglik, spec.n_w, spec.n_rows = _ptr(la, C.POINTER(C.c_double)), la.shape[0], la.shape[1]
        spec.x_source = PREDICT_X_HOST
        return self._multiplicity(spec, keep, multiplicity, (la.shape[0],), "multiplicity must have one entry per sample")

    def _call(self, fn, spec, out, counters=("n_samples", "n_distinct")):
        """One analysis call: the int64 counters the library reports attached, the return code checked -> `out` with their values."""
        values = {name: C.c_int64(0) for name in counters}
        for name, v in values.items():
            setattr(spec, name, C.pointer(v))
        self._check(fn(self.h, C.byref(spec)))
        out.update((name, v.value) for name, v in values.items())
        return out

    def predict(self, x="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None, ranks=(), mean=True,
                vote=False, samples=False):
        """ptnn_predict: network outputs of the selected weight vectors on input rows, reduced on the device.  Source: the trace rows
        step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with optional integer
        `multiplicity` [n].  x: "train", "test" or rows [n_rows, n_in].  -> dict(mean [n_rows, O] float64, order_stats
        [len(ranks), n_rows, O] float32 (exact values of those 0-based ranks), vote [n_rows, O] float64 (classification), samples
        [M, n_rows, O] float32, n_samples, n_distinct); what was not asked for is None."""
        spec, keep = _spec(PredictSpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O = spec.n_rows, self.cfg.n_out
        M = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        n_rk = _ranks(spec, keep, ranks)
        out = dict(mean=np.empty((n_rows, O), np.float64) if mean else None,
                   order_stats=np.empty((n_rk, n_rows, O), np.float32) if n_rk else None,
                   vote=np.empty((n_rows, O), np.float64) if vote else None,
                   samples=np.empty((max(M, 0), n_rows, O), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_predict, spec, out)

    def _quantities(self, spec, keep, replicas, step0, nsteps, thin, params, scalars, draws):
        """The quantities of convergence() and rank_convergence(): host draws [C, n, Q], else the trace rows with the weights `params`
        (None = all P) and the scalar columns `scalars` -> (chains, draws per chain, quantities)."""
        if draws is not None:
            da = _f32(draws)
            if da.ndim != 3:
                raise ValueError(f"draws must be [n_chains, n_draws, n_quantities], got shape {da.shape}")
            keep.append(da)
            spec.draws = _ptr(da)
            nc, nd, Q = da.shape
            spec.n_chains, spec.n_draws, spec.n_quantities = nc, nd, Q
        else:
            nc, nd = self._trace_source(spec, keep, replicas, step0, nsteps, thin)
            if params is not None:
                pa = np.ascontiguousarray(params, dtype=np.int32).reshape(-1)
                keep.append(pa)
                spec.params = pa.ctypes.data_as(_ip)              # a list, even an empty one (= no weight)
                spec.n_params = pa.size
                n_par = pa.size
            else:
                n_par = self.P
            mask = 0
            for col in scalars:
                mask |= 1 << int(col)
            spec.scalars = mask
            Q = n_par + sum(1 for c in range(8) if mask >> c & 1)
        return nc, nd, max(int(Q), 0)

    def convergence(self, *, replicas=None, step0=0, nsteps=None, thin=1, params=None, scalars=(), draws=None, per_chain=False,
                    n_lags=0):
        """ptnn_convergence: split-R-hat and split-ESS on the device.  Source: the trace rows step0, step0 + thin, ... < step0 + nsteps
        of `replicas` (None = all) -- quantities: the weights `params` (None = all P), then the scalar columns `scalars` (TR_LIKEH ..
        TR_ACC_TE) in TR_ order -- or host draws [C, n, Q].  -> dict(mean, var, r_hat, ess [Q] float64, trunc_lag [Q] int32,
        ess_chain [C, Q] float64 (per_chain), rho [n_lags, Q] float64 (n_lags > 0), n_chains, n_draws); what was not asked for is None."""
        spec, keep = _spec(ConvergenceSpec), []
        nc, nd, Q = self._quantities(spec, keep, replicas, step0, nsteps, thin, params, scalars, draws)
        out = dict(mean=np.empty(Q), var=np.empty(Q), r_hat=np.empty(Q), ess=np.empty(Q), trunc_lag=np.empty(Q, np.int32),
                   ess_chain=np.empty((max(nc, 0), Q)) if per_chain else None,
                   rho=np.empty((int(n_lags), Q)) if n_lags else None)
        _bind(spec, out)
        spec.n_lags = int(n_lags)
        self._call(self.lib.ptnn_convergence, spec, out, counters=())
        out["n_chains"], out["n_draws"] = int(nc), int(nd)
        return out

    def rank_convergence(self, *, replicas=None, step0=0, nsteps=None, thin=1, params=None, scalars=(), draws=None, probs=(), n_bins=20,
                         per_chain=False, z=False):
        """ptnn_rank_convergence: the rank-normalised split-R-hat, bulk / tail / quantile ESS and rank histograms on the device.  Sources
        and quantities as convergence().  probs: further quantile probabilities in (0, 1), at most 16.  -> dict(r_hat_bulk, r_hat_tail,
        ess_bulk, ess_tail, ess_median [Q], ess_quantile [len(probs), Q], ess_bulk_chain, ess_tail_chain [C, Q] (per_chain), all
        float64; rank_hist [C, n_bins, Q] int64; z [C, 2 (n // 2), Q] float64, the bulk z-scores of the kept draws (z); n_chains,
        n_draws); what was not asked for is None."""
        spec, keep = _spec(RankConvergenceSpec), []
        nc, nd, Q = self._quantities(spec, keep, replicas, step0, nsteps, thin, params, scalars, draws)
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        keep.append(pr)
        spec.probs, spec.n_probs, spec.n_bins = _ptr(pr, C.POINTER(C.c_double)) if pr.size else None, pr.size, int(n_bins)
        nc0, B = max(int(nc), 0), max(int(n_bins), 0)
        out = dict(r_hat_bulk=np.empty(Q), r_hat_tail=np.empty(Q), ess_bulk=np.empty(Q), ess_tail=np.empty(Q), ess_median=np.empty(Q),
                   ess_quantile=np.empty((pr.size, Q)) if pr.size else None,
                   ess_bulk_chain=np.empty((nc0, Q)) if per_chain else None, ess_tail_chain=np.empty((nc0, Q)) if per_chain else None,
                   rank_hist=np.empty((nc0, B, Q), np.int64), z=np.empty((nc0, 2 * (max(int(nd), 0) // 2), Q)) if z else None)
        _bind(spec, out)
        self._call(self.lib.ptnn_rank_convergence, spec, out, counters=())
        out["n_chains"], out["n_draws"] = int(nc), int(nd)
        return out

    def elpd(self, data="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None, loglik=None, multiplicity=None,
             r_eff=1.0, loglik_out=False):
        """ptnn_elpd: per data row lppd, p_waic, PSIS-LOO elpd and its Pareto k-hat, on the device.  Source: the trace rows step0,
        step0 + thin, ... < step0 + nsteps of `replicas` (None = all), host vectors w [n, P] with eta [n] (regression), or a host
        pointwise log-likelihood loglik [n, n_rows] float64; sources 2 and 3 take optional integer `multiplicity` [n].  data:
        "train", "test" or rows [n_rows, n_in + 1] (last column the target; ignored with loglik).  -> dict(lppd, p_waic, elpd_loo,
        khat [n_rows] float64, tail_len [n_rows] int64, loglik [S, n_rows] float64 (loglik_out), n_samples, n_distinct)."""
        spec, keep = _spec(ElpdSpec), []
        S = self._pointwise_source(spec, keep, data, loglik=loglik, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas,
                                   step0=step0, nsteps=nsteps, thin=thin)
        spec.r_eff = float(r_eff)
        n_rows = spec.n_rows
        out = dict(lppd=np.empty(n_rows), p_waic=np.empty(n_rows), elpd_loo=np.empty(n_rows), khat=np.empty(n_rows),
                   tail_len=np.empty(n_rows, np.int64), loglik=np.empty((max(S, 0), n_rows)) if loglik_out else None)
        _bind(spec, out, loglik="loglik_out")
        return self._call(self.lib.ptnn_elpd, spec, out)

    def lfo(self, data="train", *, n_fit, origins, block=1, replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None,
            loglik=None, multiplicity=None, r_eff=1.0, loglik_out=False):
        """ptnn_lfo: leave-future-out scores of ordered data rows, on the device.  The samples (the three sources of elpd()) are
        conditioned on rows [0, n_fit); origin i scores rows [i, i + block) -- `block` one-step predictions, each from its own
        observed inputs, scored jointly; not a recursive forecast -- from rows [0, i) by Pareto-smoothed importance weights.
        data: "train", "test" or rows [n_rows, n_in + 1] in time order (ignored with loglik).  -> dict(elpd_lfo, khat [n_origins]
        float64, tail_len [n_origins] int64, loglik [S, n_rows] float64 (loglik_out), n_samples, n_distinct)."""
        spec, keep = _spec(LfoSpec), []
        S = self._pointwise_source(spec, keep, data, loglik=loglik, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas,
                                   step0=step0, nsteps=nsteps, thin=thin)
        og = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1)
        keep.append(og)
        spec.origins, spec.n_origins = (_ptr(og, _ip) if og.size else None), og.size
        spec.n_fit, spec.block, spec.r_eff = int(n_fit), int(block), float(r_eff)
        n_rows = spec.n_rows
        out = dict(elpd_lfo=np.empty(og.size), khat=np.empty(og.size), tail_len=np.empty(og.size, np.int64),
                   loglik=np.empty((max(S, 0), n_rows)) if loglik_out else None)
        _bind(spec, out, loglik="loglik_out")
        return self._call(self.lib.ptnn_lfo, spec, out)

    def calibration(self, data="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None, multiplicity=None,
                    quantiles=(), crps=True):
        """ptnn_calibration: the predictive distribution of the targets, scored per data row on the device.  Source: the trace rows
        step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with eta [n] (regression)
        and optional integer `multiplicity` [n].  data: "train", "test" or rows [n_rows, n_in + 1] (last column the target).
        Regression -> dict(pit, pred_mean, pred_sd [n_rows] float64, crps [n_rows] (crps=True: the all-pairs term), quantiles
        [len(quantiles), n_rows] of the levels `quantiles` in (0, 1)); classification -> dict(p_mean [n_rows, n_out]); both
        n_samples, n_distinct; what does not apply is None."""
        spec, keep = _spec(CalibrationSpec), []
        dp = C.POINTER(C.c_double)
        self._rows(spec, keep, data, "data", (self.cfg.n_in + 1, "n_in inputs and the target"))
        self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                      unit="sample")
        n_rows, reg = spec.n_rows, self.cfg.task == TASK_REG
        lp = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        if lp.size > CALIB_MAX_LEVELS:
            raise ValueError(f"{lp.size} quantile levels: at most {CALIB_MAX_LEVELS} per call")
        if lp.size and not (np.all(lp > 0.0) and np.all(lp < 1.0)):
            raise ValueError(f"quantile levels must lie in (0, 1), got {lp.tolist()}")
        if lp.size and not reg:
            raise ValueError("quantiles: a classification has no predictive quantiles")
        lz = np.array([NormalDist().inv_cdf(float(p)) for p in lp], dtype=np.float64)
        keep += [lp, lz]
        out = dict(pit=None, crps=None, pred_mean=None, pred_sd=None, quantiles=None, p_mean=None)
        if reg:
            out.update(pit=np.empty(n_rows), pred_mean=np.empty(n_rows), pred_sd=np.empty(n_rows),
                       crps=np.empty(n_rows) if crps else None, quantiles=np.empty((lp.size, n_rows)) if lp.size else None)
            spec.pair_term = 1 if crps else 0
            if lp.size:
                spec.levels_p, spec.levels_z, spec.n_levels = lp.ctypes.data_as(dp), lz.ctypes.data_as(dp), lp.size
        else:
            out.update(p_mean=np.empty((n_rows, self.cfg.n_out)))
        _bind(spec, out)
        return self._call(self.lib.ptnn_calibration, spec, out)

    def class_report(self, data="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None, ranks=(), auc=True,
                     sample_confusion=False):
        """ptnn_class_report: confusion counts, per-class precision / recall / F1 and one-vs-rest ROC-AUC of every selected sample
        and of the pooled classifier, on the device (classification only).  Source: the trace rows step0, step0 + thin, ... <
        step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with optional integer `multiplicity` [n].  data:
        "train", "test" or rows [n_rows, n_in + 1] (last column the label).  With K = n_out and Q = 4 + 4 K metric columns (3 + 3 K
        with auc=False; their order: include/ptnn.h) -> dict(p_mean, vote [n_rows, K] float64, p_correct [n_rows] float64,
        metric_mean [Q] float64, metric_order_stats [len(ranks), Q] float32 (exact values of those 0-based ranks), confusion_sum
        [K, K] int64, sample_metrics [S, Q] float32, sample_confusion [S, K, K] int32 or None, n_samples, n_distinct)."""
        spec, keep = _spec(ClassReportSpec), []
        self._rows(spec, keep, data, "data", (self.cfg.n_in + 1, "n_in inputs and the label"))
        n_rows, K = spec.n_rows, self.cfg.n_out
        S = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        n_rk = _ranks(spec, keep, ranks)
        spec.auc = 1 if auc else 0
        Q = (4 + 4 * K) if auc else (3 + 3 * K)
        out = dict(p_mean=np.empty((n_rows, K), np.float64), vote=np.empty((n_rows, K), np.float64), p_correct=np.empty(n_rows, np.float64),
                   metric_mean=np.empty(Q, np.float64), metric_order_stats=np.empty((n_rk, Q), np.float32) if n_rk else None,
                   confusion_sum=np.empty((K, K), np.int64), sample_metrics=np.empty((max(S, 0), Q), np.float32),
                   sample_confusion=np.empty((max(S, 0), K, K), np.int32) if sample_confusion else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_class_report, spec, out)

    def uncertainty(self, x="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None, multiplicity=None, ranks=(),
                    samples=False):
        """ptnn_uncertainty: the predictive uncertainty of every row split into its aleatoric and epistemic part, on the device.
        Source: the trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P]
        with eta [n] (regression) and optional integer `multiplicity` [n].  x: "train", "test" or rows [n_rows, n_in].
        Classification -> dict(mean, vote [n_rows, K] float64 (ptnn_predict's), entropy_mean [n_rows] float64 (the expected
        entropy of a sample's class probabilities), entropy_order_stats [len(ranks), n_rows] float32 (exact values of those
        0-based ranks of the per-sample entropies), sample_entropy [S, n_rows] float32 (samples=True)); regression ->
        dict(mean, epistemic_var [n_rows, n_out] float64, aleatoric_var float); both n_samples, n_distinct; what does not
        apply or was not asked for is None."""
        spec, keep = _spec(UncertaintySpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O = spec.n_rows, self.cfg.n_out
        S = self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="sample")
        out = dict(mean=np.empty((n_rows, O), np.float64), vote=None, entropy_mean=None, entropy_order_stats=None, sample_entropy=None,
                   epistemic_var=None, aleatoric_var=None)
        if self.cfg.task == TASK_REG:
            out.update(epistemic_var=np.empty((n_rows, O), np.float64), aleatoric_var=np.empty(1, np.float64))
        else:
            n_rk = _ranks(spec, keep, ranks)
            out.update(vote=np.empty((n_rows, O), np.float64), entropy_mean=np.empty(n_rows, np.float64),
                       entropy_order_stats=np.empty((n_rk, n_rows), np.float32) if n_rk else None,
                       sample_entropy=np.empty((max(S, 0), n_rows), np.float32) if samples else None)
        _bind(spec, out)
        self._call(self.lib.ptnn_uncertainty, spec, out)
        if out["aleatoric_var"] is not None:
            out["aleatoric_var"] = float(out["aleatoric_var"][0])
        return out

    def influence(self, x="test", cases="train", *, of="prediction", replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None,
                  multiplicity=None, values=None, loglik=None, cov=True):
        """ptnn_influence: the covariance over the samples of every target column with every case row's log-likelihood, on the
        device.  Source: the trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), host vectors w
        [n, P] with eta [n] (regression), or host matrices values [n, n_a] float32 and loglik [n, n_b] float64 (no forward pass;
        x, cases and of are ignored); sources 2 and 3 take optional integer `multiplicity` [n].  cases: "train", "test" or rows
        [n_cases, n_in + 1] (last column the target).  of "prediction": x = "train", "test" or rows [n_x, n_in], the target
        columns are the outputs, n_a = n_x * n_out (row-major); of "loglik": x rows have n_in + 1 columns, the target columns are
        their log-likelihoods, n_a = n_x.  -> dict(cov [n_a, n_b] (cov=True), target_mean, target_var [n_a], case_mean, case_var
        [n_b], all float64, variances with ddof 1 over the expanded samples; n_samples, n_distinct)."""
        spec, keep = _spec(InfluenceSpec), []
        if values is not None or loglik is not None:
            if values is None or loglik is None:
                raise ValueError("values and loglik come together")
            va, la = _f32(values), np.ascontiguousarray(loglik, dtype=np.float64)
            if va.ndim != 2 or la.ndim != 2 or va.shape[0] != la.shape[0]:
                raise ValueError(f"values must be [n_samples, n_a] and loglik [n_samples, n_b], got shapes {va.shape} and {la.shape}")
            keep += [va, la]
            spec.target_values, spec.loglik, spec.n_w = _ptr(va), _ptr(la, C.POINTER(C.c_double)), va.shape[0]
            n_a, n_b = spec.n_a, spec.n_b = va.shape[1], la.shape[1]
            self._multiplicity(spec, keep, multiplicity, (va.shape[0],), "multiplicity must have one entry per sample")
        else:
            kind = {"prediction": INFLUENCE_OUTPUT, "loglik": INFLUENCE_LOGLIK}.get(of)
            if kind is None:
                raise ValueError(f"of must be 'prediction' or 'loglik', not {of!r}")
            spec.target_kind = kind
            width = (self.cfg.n_in, "n_in columns") if kind == INFLUENCE_OUTPUT else (self.cfg.n_in + 1, "n_in inputs and the target")
            self._rows(spec, keep, x, "x", width, fields=("target_source", "n_targets", "target_x"))
            self._rows(spec, keep, cases, "cases", (self.cfg.n_in + 1, "n_in inputs and the target"), fields=("case_source", "n_cases", "case_x"))
            self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="sample")
            n_a, n_b = spec.n_targets * (self.cfg.n_out if kind == INFLUENCE_OUTPUT else 1), spec.n_cases
        if n_a * n_b > INFLUENCE_MAX_ELEMENTS:
            raise ValueError(f"{n_a} target columns x {n_b} cases: at most 2^27 elements per call")
        out = dict(cov=np.empty((n_a, n_b), np.float64) if cov else None, target_mean=np.empty(n_a), target_var=np.empty(n_a),
                   case_mean=np.empty(n_b), case_var=np.empty(n_b))
        _bind(spec, out)
        return self._call(self.lib.ptnn_influence, spec, out)

    def modes(self, x=None, *, radius_sq_sum, values=None, multiplicity=None, sq_dist=False, outputs=False, **source):
        """ptnn_modes: the squared function-space distance sq[u, v] = sum_j (F[u, j] - F[v, j])^2 (double) between the U distinct
        selected samples, and the density-peaks stage on it, on the device.  Source (`source`: replicas, step0, nsteps, thin, or
        w): the trace rows or host vectors w [n, P] as predict() takes them, F the fp32 network outputs on x ("train", "test" or
        rows [n_rows, n_in]), n = n_rows * n_out; or a host matrix values [n, n_a] float32 (no forward pass, x is ignored; every
        row is a sample, n = n_a).  `multiplicity` [n]: integer counts of the host items.  radius_sq_sum = radius^2 * n: rho_u
        counts the samples with sq[u, v] <= it.  -> dict(rho [U] int64, delta_sq [U] float64, parent [U] int32, count [U] int32,
        item_sample [n_items] int32 (the distinct sample of every selected item, chain-major for the trace), spread_sq,
        sq_dist [U, U] float64 and outputs [U, n] float32 on request, n_samples, n_distinct)."""
        spec, keep = _spec(ModesSpec), []
        if values is not None:
            if source.get("w") is not None:
                raise ValueError("values takes the place of the samples: no w with it")
            va = _f32(values)
            if va.ndim != 2 or va.shape[1] < 1:
                raise ValueError(f"values must be [n_samples, n_a], got shape {va.shape}")
            keep.append(va)
            spec.values, spec.n_w, spec.n_a = _ptr(va), va.shape[0], va.shape[1]
            n_items, n = va.shape[0], va.shape[1]
            self._multiplicity(spec, keep, multiplicity, (n_items,), "multiplicity must have one entry per sample")
        else:
            self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
            n = spec.n_rows * self.cfg.n_out
            src = dict(dict(w=None, replicas=None, step0=0, nsteps=None, thin=1), **source)
            self._samples(spec, keep, multiplicity=multiplicity, unit="vector", **src)
            if src["w"] is not None:
                n_items = int(spec.n_w)
            else:
                chains = self.R if src["replicas"] is None else int(spec.n_replicas)
                n_items = max(0, chains * -(-spec.nsteps // max(1, spec.thin)))
        spec.near_sq = float(radius_sq_sum)
        room = spec.room = max(1, n_items)
        big = min(room, MODES_MAX_DISTINCT)                 # sq_dist and outputs come back packed [U, U], [U, n]: U is known after the call
        out = dict(rho=np.zeros(room, np.int64), delta_sq=np.zeros(room, np.float64), parent=np.full(room, -1, np.int32),
                   count=np.zeros(room, np.int32), item_sample=np.zeros(room, np.int32), spread_sq=np.zeros(1, np.float64),
                   sq_dist=np.empty(big * big, np.float64) if sq_dist else None, outputs=np.empty(big * n, np.float32) if outputs else None)
        _bind(spec, out)
        out = self._call(self.lib.ptnn_modes, spec, out)
        U = out["n_distinct"]
        for k in ("rho", "delta_sq", "parent", "count"):
            out[k] = out[k][:U].copy()
        out["item_sample"] = out["item_sample"][:n_items]
        out["spread_sq"] = float(out["spread_sq"][0])
        if sq_dist:
            out["sq_dist"] = out["sq_dist"][:U * U].reshape(U, U).copy()
        if outputs:
            out["outputs"] = out["outputs"][:U * n].reshape(U, n).copy()
        return out

    def compress(self, x=None, *, m, subsets=None, values=None, multiplicity=None, sq_dist=False, outputs=False, **source):
        """ptnn_compress: kernel herding with the energy-distance kernel on ptnn_modes' squared function-space distance of the U
        distinct selected samples, on the device.  Source, x, values and multiplicity as modes().  m: the picks, 0 <= m <= the
        present samples (count > 0).  subsets [B, k] int32: item indices (repeats allowed) of B subsets whose energy distance to
        the full weighted sample is evaluated.  -> dict(picks [m] int32 (distinct-sample indices in herding order), energy [m],
        pick_score [m], mu [U], d0, subset_energy [B] (None without subsets), all float64 in the units of sqrt(sq); count [U]
        int32, item_sample [n_items] int32, sq_dist [U, U] float64 and outputs [U, n] float32 on request, n_samples,
        n_distinct)."""
        spec, keep = _spec(CompressSpec), []
        if values is not None:
            if source.get("w") is not None:
                raise ValueError("values takes the place of the samples: no w with it")
            va = _f32(values)
            if va.ndim != 2 or va.shape[1] < 1:
                raise ValueError(f"values must be [n_samples, n_a], got shape {va.shape}")
            keep.append(va)
            spec.values, spec.n_w, spec.n_a = _ptr(va), va.shape[0], va.shape[1]
            n_items, n = va.shape[0], va.shape[1]
            self._multiplicity(spec, keep, multiplicity, (n_items,), "multiplicity must have one entry per sample")
        else:
            self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
            n = spec.n_rows * self.cfg.n_out
            src = dict(dict(w=None, replicas=None, step0=0, nsteps=None, thin=1), **source)
            self._samples(spec, keep, multiplicity=multiplicity, unit="vector", **src)
            if src["w"] is not None:
                n_items = int(spec.n_w)
            else:
                chains = self.R if src["replicas"] is None else int(spec.n_replicas)
                n_items = max(0, chains * -(-spec.nsteps // max(1, spec.thin)))
        m = int(m)
        if m < 0:
            raise ValueError(f"m = {m} picks: must be >= 0")
        spec.m = m
        B = 0
        if subsets is not None:
            sub = np.ascontiguousarray(subsets, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[1] < 1 or sub.shape[1] > COMPRESS_MAX_SUBSET:
                raise ValueError(f"subsets must be [n_subsets, k] item indices with 1 <= k <= {COMPRESS_MAX_SUBSET}, got shape {sub.shape}")
            keep.append(sub)
            B = sub.shape[0]
            spec.subset_items, spec.n_subsets, spec.subset_size = (_ptr(sub, _ip) if B else None), B, sub.shape[1]
        room = spec.room = max(1, n_items)
        big = min(room, MODES_MAX_DISTINCT)                 # sq_dist and outputs come back packed [U, U], [U, n]: U is known after the call
        out = dict(picks=np.zeros(max(1, m), np.int32), energy=np.zeros(max(1, m), np.float64), pick_score=np.zeros(max(1, m), np.float64),
                   mu=np.zeros(room, np.float64), d0=np.zeros(1, np.float64), subset_energy=np.zeros(B, np.float64) if B else None,
                   count=np.zeros(room, np.int32), item_sample=np.zeros(room, np.int32),
                   sq_dist=np.empty(big * big, np.float64) if sq_dist else None, outputs=np.empty(big * n, np.float32) if outputs else None)
        _bind(spec, out)
        out = self._call(self.lib.ptnn_compress, spec, out)
        U = out["n_distinct"]
        for k in ("picks", "energy", "pick_score"):
            out[k] = out[k][:m].copy()
        for k in ("mu", "count"):
            out[k] = out[k][:U].copy()
        out["item_sample"] = out["item_sample"][:n_items]
        out["d0"] = float(out["d0"][0])
        if sq_dist:
            out["sq_dist"] = out["sq_dist"][:U * U].reshape(U, U).copy()
        if outputs:
            out["outputs"] = out["outputs"][:U * n].reshape(U, n).copy()
        return out

    def sensitivity(self, x="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None, ranks=(), ranks2=(),
                    sample_abs=False, samples=False):
        """ptnn_sensitivity: the gradient g of the network outputs with respect to the inputs, for the selected weight vectors on
        input rows, reduced on the device.  Source and x as predict().  -> dict(grad_mean [n_rows, O, I] float64, order_stats
        [len(ranks), n_rows, O, I] float32 (exact values of those 0-based ranks of g), pos_count, neg_count [n_rows, O, I] int64
        (samples with g > 0, g < 0), abs_mean, sq_mean [O, I] float64 (means over samples of the row means of |g| and g^2),
        abs_order_stats [len(ranks2), O, I] float32 (exact ranks of the per-sample row mean of |g|), sample_abs [M, O, I] float32,
        samples [M, n_rows, O, I] float32, n_samples, n_distinct); what was not asked for is None."""
        spec, keep = _spec(SensitivitySpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O, I = spec.n_rows, self.cfg.n_out, self.cfg.n_in
        M = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        n_rk, n_rk2 = _ranks(spec, keep, ranks), _ranks(spec, keep, ranks2, ("ranks2", "n_ranks2"))
        out = dict(grad_mean=np.empty((n_rows, O, I), np.float64),
                   order_stats=np.empty((n_rk, n_rows, O, I), np.float32) if n_rk else None,
                   pos_count=np.empty((n_rows, O, I), np.int64), neg_count=np.empty((n_rows, O, I), np.int64),
                   abs_mean=np.empty((O, I), np.float64), sq_mean=np.empty((O, I), np.float64),
                   abs_order_stats=np.empty((n_rk2, O, I), np.float32) if n_rk2 else None,
                   sample_abs=np.empty((max(M, 0), O, I), np.float32) if sample_abs else None,
                   samples=np.empty((max(M, 0), n_rows, O, I), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_sensitivity, spec, out)

    def partial_dependence(self, x="train", *, inputs=None, grid, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None,
                           ranks=(), ranks2=(), ice_mean=False, sample_pd=False, sample_range=False, samples=False):
        """ptnn_partial_dependence: the outputs of the selected weight vectors on the rows `x` with input inputs[a] set to
        grid[a, k], reduced on the device.  Source and x as predict().  inputs: the selected input indices (None = all n_in);
        grid [A, G] float32, one row per selected input.  ranks apply to ICE (its mean and order statistics are computed only with
        ice_mean or ranks), ranks2 to the per-sample curve and its range.  -> dict(ice_mean [n_rows, A, G, O] float64,
        ice_order_stats [len(ranks), n_rows, A, G, O] float32, pd_mean [A, G, O] float64, pd_order_stats [len(ranks2), A, G, O]
        float32, range_mean [A, O] float64, range_order_stats [len(ranks2), A, O] float32, sample_pd [M, A, G, O], sample_range
        [M, A, O], samples [M, n_rows, A, G, O] float32, n_samples, n_distinct); what was not asked for is None."""
        spec, keep = _spec(PdSpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O = spec.n_rows, self.cfg.n_out
        M = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        A = self.cfg.n_in
        if inputs is not None:
            ia = np.ascontiguousarray(inputs, dtype=np.int32).reshape(-1)
            keep.append(ia)
            spec.inputs, spec.n_inputs = _ptr(ia, _ip), ia.size
            A = ia.size
        ga = _f32(grid)
        if ga.ndim != 2 or ga.shape[0] != A:
            raise ValueError(f"grid must be [{A}, n_grid] (one row per selected input), got shape {ga.shape}")
        keep.append(ga)
        spec.grid, spec.n_grid = _ptr(ga), ga.shape[1]
        G = ga.shape[1]
        n_rk, n_rk2 = _ranks(spec, keep, ranks), _ranks(spec, keep, ranks2, ("ranks2", "n_ranks2"))
        out = dict(ice_mean=np.empty((n_rows, A, G, O), np.float64) if ice_mean else None,
                   ice_order_stats=np.empty((n_rk, n_rows, A, G, O), np.float32) if n_rk else None,
                   pd_mean=np.empty((A, G, O), np.float64),
                   pd_order_stats=np.empty((n_rk2, A, G, O), np.float32) if n_rk2 else None,
                   range_mean=np.empty((A, O), np.float64),
                   range_order_stats=np.empty((n_rk2, A, O), np.float32) if n_rk2 else None,
                   sample_pd=np.empty((max(M, 0), A, G, O), np.float32) if sample_pd else None,
                   sample_range=np.empty((max(M, 0), A, O), np.float32) if sample_range else None,
                   samples=np.empty((max(M, 0), n_rows, A, G, O), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_partial_dependence, spec, out)

    def accumulated_effects(self, x="train", *, inputs=None, edges=None, pairs=None, edges2=None, replicas=None, step0=0, nsteps=None,
                            thin=1, w=None, multiplicity=None, ranks=(), ranks2=(), local_mean=False, sample_ale=False, sample_range=False,
                            sample_ale2=False, sample_inter=False, samples=False):
        """ptnn_accumulated_effects: the accumulated local effects of the selected weight vectors on the rows `x`, reduced on the
        device.  Source and x as predict().  edges [A, E] float32, one row of bin edges per first-order input (increasing, the
        tail may repeat the last edge), None = no first-order term; inputs: their indices (None = all n_in).  pairs [Q, 2] with
        edges2 [Q, 2, E2].  ranks apply to the local effects (their mean and order statistics are computed only with local_mean
        or ranks), ranks2 to the curves, surfaces, ranges and interactions.  With T = A + Q -> dict(bin_count [A, E - 1],
        cell_count [Q, E2 - 1, E2 - 1] int64, ale_mean [A, E, O] float64, ale_order_stats [len(ranks2), A, E, O] float32,
        range_mean [A, O], range_order_stats, ale2_mean [Q, E2, E2, O], ale2_order_stats, inter_mean [Q, O], inter_order_stats,
        sample_ale [M, A, E, O], sample_range [M, A, O], sample_ale2 [M, Q, E2, E2, O], sample_inter [M, Q, O], local_mean
        [n_rows, T, O], local_order_stats [len(ranks), n_rows, T, O], samples [M, n_rows, T, O] float32, n_samples, n_distinct);
        what was not asked for, or has no term, is None."""
        spec, keep = _spec(AleSpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O = spec.n_rows, self.cfg.n_out
        M = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        A = E = Q = E2 = 0
        if edges is not None:
            A = self.cfg.n_in
            if inputs is not None:
                ia = np.ascontiguousarray(inputs, dtype=np.int32).reshape(-1)
                keep.append(ia)
                spec.inputs, spec.n_inputs = _ptr(ia, _ip), ia.size
                A = ia.size
            ea = _f32(edges)
            if ea.ndim != 2 or ea.shape[0] != A:
                raise ValueError(f"edges must be [{A}, n_edges] (one row per selected input), got shape {ea.shape}")
            keep.append(ea)
            spec.edges, spec.n_edges = _ptr(ea), ea.shape[1]
            E = ea.shape[1]
        if pairs is not None and np.size(pairs):
            pa = np.ascontiguousarray(pairs, dtype=np.int32)
            if pa.ndim != 2 or pa.shape[1] != 2:
                raise ValueError(f"pairs must be [n_pairs, 2], got shape {pa.shape}")
            Q = pa.shape[0]
            ea2 = _f32(edges2) if edges2 is not None else np.zeros((0,), np.float32)
            if ea2.ndim != 3 or ea2.shape[:2] != (Q, 2):
                raise ValueError(f"edges2 must be [{Q}, 2, n_edges2] (the edges of each pair's two inputs), got shape {ea2.shape}")
            keep += [pa, ea2]
            spec.pairs, spec.n_pairs, spec.edges2, spec.n_edges2 = _ptr(pa, _ip), Q, _ptr(ea2), ea2.shape[2]
            E2 = ea2.shape[2]
        T, Mx = A + Q, max(M, 0)
        n_rk, n_rk2 = _ranks(spec, keep, ranks), _ranks(spec, keep, ranks2, ("ranks2", "n_ranks2"))
        out = dict(bin_count=np.empty((A, E - 1), np.int64) if A else None,
                   cell_count=np.empty((Q, E2 - 1, E2 - 1), np.int64) if Q else None,
                   ale_mean=np.empty((A, E, O), np.float64) if A else None,
                   ale_order_stats=np.empty((n_rk2, A, E, O), np.float32) if A and n_rk2 else None,
                   range_mean=np.empty((A, O), np.float64) if A else None,
                   range_order_stats=np.empty((n_rk2, A, O), np.float32) if A and n_rk2 else None,
                   sample_ale=np.empty((Mx, A, E, O), np.float32) if A and sample_ale else None,
                   sample_range=np.empty((Mx, A, O), np.float32) if A and sample_range else None,
                   ale2_mean=np.empty((Q, E2, E2, O), np.float64) if Q else None,
                   ale2_order_stats=np.empty((n_rk2, Q, E2, E2, O), np.float32) if Q and n_rk2 else None,
                   inter_mean=np.empty((Q, O), np.float64) if Q else None,
                   inter_order_stats=np.empty((n_rk2, Q, O), np.float32) if Q and n_rk2 else None,
                   sample_ale2=np.empty((Mx, Q, E2, E2, O), np.float32) if Q and sample_ale2 else None,
                   sample_inter=np.empty((Mx, Q, O), np.float32) if Q and sample_inter else None,
                   local_mean=np.empty((n_rows, T, O), np.float64) if local_mean else None,
                   local_order_stats=np.empty((n_rk, n_rows, T, O), np.float32) if n_rk else None,
                   samples=np.empty((Mx, n_rows, T, O), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_accumulated_effects, spec, out)

    def coalition_values(self, x="test", *, background, masks, coef, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None,
                         ranks=(), ranks2=(), mean=True, counts=False, abs_mean=True, sample_abs=False, samples=False):
        """ptnn_coalition_values: for the selected weight vectors and the rows `x`, the value v(S) of every coalition of the table
        -- the mean over the `background` rows [B, n_in] of the output on the hybrid row (input i from the explained row where bit
        i of masks[c] is set, else from the background row) -- and out = sum_c coef[c, t] v(S_c), reduced on the device.  Source
        and x as predict().  masks [C] uint64, coef [C, T] float64.  ranks apply to out, ranks2 to the per-sample row mean of
        |out|.  -> dict(mean [n_rows, O, T] float64, order_stats [len(ranks), n_rows, O, T] float32, pos_count, neg_count [n_rows,
        O, T] int64 (counts), abs_mean [O, T] float64, abs_order_stats [len(ranks2), O, T] float32, sample_abs [M, O, T] float32,
        samples [M, n_rows, O, T] float32, n_samples, n_distinct); what was not asked for is None."""
        spec, keep = _spec(ShapSpec), []
        self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        n_rows, O, I = spec.n_rows, self.cfg.n_out, self.cfg.n_in
        M = self._samples(spec, keep, w=w, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        ba = _f32(background)
        if ba.ndim != 2 or ba.shape[1] != I:
            raise ValueError(f"background must be [n_background, {I}] (n_in columns), got shape {ba.shape}")
        ma = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1)
        ca = np.ascontiguousarray(coef, dtype=np.float64)
        if ca.ndim != 2 or ca.shape[0] != ma.size:
            raise ValueError(f"coef must be [{ma.size}, n_terms] (one row per coalition), got shape {ca.shape}")
        keep += [ba, ma, ca]
        spec.background, spec.n_background = _ptr(ba), ba.shape[0]
        spec.masks, spec.coef = _ptr(ma, C.POINTER(C.c_uint64)), _ptr(ca, C.POINTER(C.c_double))
        spec.n_coalitions, spec.n_terms = ca.shape
        T = ca.shape[1]
        n_rk, n_rk2 = _ranks(spec, keep, ranks), _ranks(spec, keep, ranks2, ("ranks2", "n_ranks2"))
        out = dict(mean=np.empty((n_rows, O, T), np.float64) if mean else None,
                   order_stats=np.empty((n_rk, n_rows, O, T), np.float32) if n_rk else None,
                   pos_count=np.empty((n_rows, O, T), np.int64) if counts else None,
                   neg_count=np.empty((n_rows, O, T), np.int64) if counts else None,
                   abs_mean=np.empty((O, T), np.float64) if abs_mean else None,
                   abs_order_stats=np.empty((n_rk2, O, T), np.float32) if n_rk2 else None,
                   sample_abs=np.empty((max(M, 0), O, T), np.float32) if sample_abs else None,
                   samples=np.empty((max(M, 0), n_rows, O, T), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_coalition_values, spec, out)

    def ppc(self, data="train", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, eta=None, multiplicity=None, lags=(), seed=0,
            samples=True, draws=False):
        """ptnn_ppc: posterior predictive checks on the device -- every selected occurrence draws one replicated data set (Philox
        stream STREAM_PPC of `seed`), test quantities T are evaluated on it and on the data.  Source: the trace rows step0, step0 +
        thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with eta [n] (regression) and optional
        integer `multiplicity` [n].  data: "train", "test" or rows [n_rows, n_in + 1] in their order (last column the target).
        lags: the residual autocorrelation lags of a regression.  -> dict(n_defined, n_greater, n_equal [n_stats] int64, mean_obs,
        mean_rep, var_rep [n_stats] float64, t_obs, t_rep [M, n_stats] float64 (samples), z [M, n_rows] float32 (draws, regression),
        y_rep [M, n_rows] int32 (draws, classification), n_samples, n_distinct); what was not asked for is None."""
        spec, keep = _spec(PpcSpec), []
        self._rows(spec, keep, data, "data", (self.cfg.n_in + 1, "n_in inputs and the target"))
        M = self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="sample")
        lg = np.ascontiguousarray(lags, dtype=np.int32).reshape(-1)
        keep.append(lg)
        spec.lags, spec.n_lags = (_ptr(lg, _ip) if lg.size else None), lg.size
        spec.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        reg = self.cfg.task == TASK_REG
        n_stats = 7 + lg.size if reg else 2 + self.cfg.n_out
        n_rows, M = spec.n_rows, max(M, 0)
        out = dict(n_defined=np.zeros(n_stats, np.int64), n_greater=np.zeros(n_stats, np.int64), n_equal=np.zeros(n_stats, np.int64),
                   mean_obs=np.empty(n_stats), mean_rep=np.empty(n_stats), var_rep=np.empty(n_stats),
                   t_obs=np.empty((M, n_stats)) if samples else None, t_rep=np.empty((M, n_stats)) if samples else None,
                   z=np.empty((M, n_rows), np.float32) if draws and reg else None,
                   y_rep=np.empty((M, n_rows), np.int32) if draws and not reg else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_ppc, spec, out)

    def powerscale(self, x="test", *, groups=("weights", "eta", "predictions"), delta=0.01, r_eff=1.0, replicas=None, step0=0,
                   nsteps=None, thin=1, w=None, eta=None, multiplicity=None):
        """ptnn_powerscale: power-scaling sensitivity on the device -- the prior and the likelihood are raised to 1 / (1 + delta)
        and 1 + delta by Pareto-smoothed importance weights, and the distance every quantity's marginal moves is measured.
        Source: the trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with
        eta [n] (regression) and optional integer `multiplicity` [n].  groups: names of POWERSCALE_GROUPS; x: the rows of the
        predictions, "train", "test" or rows [n_rows, n_in].  Axis 0 of sens is the component (likelihood, prior), axes 0, 1 of
        dist / mean / sd / khat / tail_len the component and the sign (alpha_minus, alpha_plus).  -> dict(sens [2, Q], dist, mean,
        sd [2, 2, Q], base_mean, base_sd [Q] float64, khat [2, 2] float64, tail_len [2, 2] int64, logp [2, U] float64 (the
        components per distinct sample), n_samples, n_distinct, n_quantities)."""
        spec, keep = _spec(PowerscaleSpec), []
        mask = 0
        for g in groups:
            if g not in POWERSCALE_GROUPS:
                raise ValueError(f"unknown group {g!r}: choose among {list(POWERSCALE_GROUPS)}")
            mask |= POWERSCALE_GROUPS[g]
        spec.groups = mask
        O = self.cfg.n_out
        if mask & POWERSCALE_GROUPS["predictions"]:
            self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        M = self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="sample")
        n_items = M if w is None else spec.n_w              # an item of multiplicity 0 is still a distinct sample
        spec.delta, spec.r_eff = float(delta), float(r_eff)
        Q = ((self.P if mask & 1 else 0) + (1 if mask & 2 else 0) + (spec.n_rows * O if mask & 4 else 0) + (1 if mask & 8 else 0))
        out = dict(sens=np.empty((2, Q)), dist=np.empty((2, 2, Q)), mean=np.empty((2, 2, Q)), sd=np.empty((2, 2, Q)),
                   base_mean=np.empty(Q), base_sd=np.empty(Q), khat=np.empty((2, 2)), tail_len=np.empty((2, 2), np.int64),
                   logp=np.empty(2 * max(n_items, 1)))
        _bind(spec, out)
        self._call(self.lib.ptnn_powerscale, spec, out, counters=("n_samples", "n_distinct", "n_quantities"))
        out["logp"] = out["logp"][:2 * out["n_distinct"]].reshape(2, out["n_distinct"]).copy()
        return out

    def prior_predictive(self, x="train", *, n_draws, sigma_squared=None, draw0=0, seed=0, target=False, ranks=(), eps=0.01,
                         t_draw=False, samples=False, weights=False):
        """ptnn_prior_predictive: the network outputs of n_draws weight vectors drawn from the prior N(0, sigma_squared I), at
        every scale of `sigma_squared` (None = the handle's, else up to 8 values) with the same normal deviates, reduced on the
        device.  x: "train", "test" or rows [n_rows, n_in] (`target`: [n_rows, n_in + 1], the last column the target).  Draw i has
        the Philox counter draw0 + i.  -> dict, S = the scales: mean, vote (classification) [S, n_rows, O] float64, order_stats
        [S, len(ranks), n_rows, O] float32, sat_count [S, n_rows, O] int64 (draws with f < eps or f > 1 - eps); t_obs [n_stats];
        stat_mean, stat_sd [S, n_stats] float64, stat_order_stats [S, len(ranks), n_stats] float32, n_greater, n_equal, n_defined
        [S, n_stats] int64; t_draw [S, n_draws, n_stats] float64, samples [S, n_draws, n_rows, O] float32, weights [S, n_draws, P]
        float32 (each on request, else None); n_stats, n_blocks."""
        spec, keep = _spec(PriorSpec), []
        I, O = self.cfg.n_in, self.cfg.n_out
        self._rows(spec, keep, x, "x", (I + 1, "n_in inputs and the target") if target else (I, "n_in columns"))
        spec.has_target = 1 if target else 0
        if sigma_squared is not None:
            sa = np.ascontiguousarray(sigma_squared, dtype=np.float64).reshape(-1)
            keep.append(sa)
            spec.sigma_squared, spec.n_scales = _ptr(sa, C.POINTER(C.c_double)), sa.size
        S = max(1, spec.n_scales)
        spec.n_draws, spec.draw0, spec.seed, spec.eps = int(n_draws), int(draw0), int(seed), float(eps)
        n_rk = _ranks(spec, keep, ranks)
        n_rows, n, cls = spec.n_rows, max(int(n_draws), 0), self.cfg.task == TASK_CLS
        n_stats = PRIOR_CLS_FIXED + O if cls else PRIOR_REG_STATS
        out = dict(mean=np.empty((S, n_rows, O), np.float64), order_stats=np.empty((S, n_rk, n_rows, O), np.float32) if n_rk else None,
                   vote=np.empty((S, n_rows, O), np.float64) if cls else None, sat_count=np.empty((S, n_rows, O), np.int64),
                   t_obs=np.empty(n_stats, np.float64), stat_mean=np.empty((S, n_stats), np.float64),
                   stat_sd=np.empty((S, n_stats), np.float64),
                   stat_order_stats=np.empty((S, n_rk, n_stats), np.float32) if n_rk else None,
                   n_greater=np.empty((S, n_stats), np.int64), n_equal=np.empty((S, n_stats), np.int64),
                   n_defined=np.empty((S, n_stats), np.int64),
                   t_draw=np.empty((S, n, n_stats), np.float64) if t_draw else None,
                   samples=np.empty((S, n, n_rows, O), np.float32) if samples else None,
                   weights=np.empty((S, n, self.P), np.float32) if weights else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_prior_predictive, spec, out, counters=("n_stats", "n_blocks"))

    def forecast(self, horizon, origins="test", *, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None, eta=None,
                 noise=False, seed=0, ranks=(), mean=True, samples=False):
        """ptnn_forecast: recursive multi-step forecasts of the one-step map f_w from origin windows, on the device.  Source: the
        trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all), or host vectors w [n, P] with optional
        integer `multiplicity` [n] and eta [n] (noise on).  origins: "train", "test" or windows [n_origins, n_in].  noise: add
        exp(eta / 2) z_k to every step (Philox stream STREAM_FORECAST of `seed`).  -> dict(mean [n_origins, horizon] float64,
        order_stats [len(ranks), n_origins, horizon] float32, samples [M, n_origins, horizon] float32, n_samples, n_trajectories);
        what was not asked for is None."""
        spec, keep = _spec(ForecastSpec), []
        self._rows(spec, keep, origins, "origins", (self.cfg.n_in, "n_in columns"), ("origin_source", "n_origins", "origins"))
        spec.horizon, spec.noise, spec.seed = int(horizon), 1 if noise else 0, int(seed) & 0xFFFFFFFFFFFFFFFF
        n_org, hz = spec.n_origins, max(int(horizon), 0)
        M = self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        n_rk = _ranks(spec, keep, ranks)
        out = dict(mean=np.empty((n_org, hz), np.float64) if mean else None,
                   order_stats=np.empty((n_rk, n_org, hz), np.float32) if n_rk else None,
                   samples=np.empty((max(M, 0), n_org, hz), np.float32) if samples else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_forecast, spec, out, counters=("n_samples", "n_trajectories"))

    def forecast_score(self, horizon, origins, truth, *, replicas=None, step0=0, nsteps=None, thin=1, w=None, multiplicity=None,
                       eta=None, noise=True, seed=0, quantiles=(), crps=True, energy=True, samples=False, means=False):
        """ptnn_forecast_score: the recursive forecasts of ptnn_forecast scored against `truth` [n_origins, horizon] (NaN = no
        observation) on the device.  Source, origins, noise and seed as forecast(); eta [n] always comes with host vectors.
        -> dict(pit, pred_mean, pred_sd, log_score [n_origins, horizon] float64, crps [n_origins, horizon] (crps=True: the
        all-pairs term), quantiles [len(quantiles), n_origins, horizon], energy_score [n_origins] (energy=True), samples and
        means [M, n_origins, horizon] float32, n_samples, n_trajectories); what was not asked for is None."""
        spec, keep = _spec(ForecastScoreSpec), []
        dp = C.POINTER(C.c_double)
        self._rows(spec, keep, origins, "origins", (self.cfg.n_in, "n_in columns"), ("origin_source", "n_origins", "origins"))
        spec.horizon, spec.noise, spec.seed = int(horizon), 1 if noise else 0, int(seed) & 0xFFFFFFFFFFFFFFFF
        n_org, hz = spec.n_origins, max(int(horizon), 0)
        ta = _f32(truth)
        if ta.shape != (n_org, hz):
            raise ValueError(f"truth must be [n_origins, horizon] = ({n_org}, {hz}), got shape {ta.shape}")
        keep.append(ta)
        spec.truth = _ptr(ta)
        M = self._samples(spec, keep, w=w, eta=eta, multiplicity=multiplicity, replicas=replicas, step0=step0, nsteps=nsteps, thin=thin,
                          unit="vector")
        lp = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        if lp.size > CALIB_MAX_LEVELS:
            raise ValueError(f"{lp.size} quantile levels: at most {CALIB_MAX_LEVELS} per call")
        if lp.size and not (np.all(lp > 0.0) and np.all(lp < 1.0)):
            raise ValueError(f"quantile levels must lie in (0, 1), got {lp.tolist()}")
        lz = np.array([NormalDist().inv_cdf(float(p)) for p in lp], dtype=np.float64)
        keep += [lp, lz]
        if lp.size:
            spec.levels_p, spec.levels_z, spec.n_levels = lp.ctypes.data_as(dp), lz.ctypes.data_as(dp), lp.size
        spec.pair_term, spec.energy = 1 if crps else 0, 1 if energy else 0
        col = lambda: np.empty((n_org, hz), np.float64)       # noqa: E731
        out = dict(pit=col(), pred_mean=col(), pred_sd=col(), log_score=col(), crps=col() if crps else None,
                   quantiles=np.empty((lp.size, n_org, hz), np.float64) if lp.size else None,
                   energy_score=np.empty(n_org, np.float64) if energy else None,
                   samples=np.empty((max(M, 0), n_org, hz), np.float32) if samples else None,
                   means=np.empty((max(M, 0), n_org, hz), np.float32) if means else None)
        _bind(spec, out)
        return self._call(self.lib.ptnn_forecast_score, spec, out, counters=("n_samples", "n_trajectories"))

    def evidence(self, *, replicas=None, step0=0, nsteps=None, thin=1, w=None, u=None, multiplicity=None, d=None, n_prior=0, seed=0,
                 a=(), u_out=False, u_prior_out=False):
        """ptnn_evidence: per-rung statistics of the full-data log-likelihood U and of prior draws, on the device.  Source: the
        trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None = all; one rung each), host vectors w
        [K, n, P], or a host U [K, n] float64; sources 2 and 3 take optional integer `multiplicity` [K, n].  d [K]: stone
        exponents; n_prior draws of the prior (Philox stream STREAM_PRIOR of `seed`) with exponents a (at most 4).
        -> dict(u_mean, u_var, u_ess, log_stone, stone_relvar [K] float64, n_draws [K] int64, prior_log_mean_exp,
        prior_kish_ess, prior_u_mean, prior_u_var [n_a] float64, u [sum n_draws] float64 (u_out), u_prior [n_prior] float64
        (u_prior_out), n_distinct)."""
        spec, keep = _spec(EvidenceSpec), []
        dp = C.POINTER(C.c_double)
        if u is not None:
            ua = np.ascontiguousarray(u, dtype=np.float64)
            if ua.ndim != 2:
                raise ValueError(f"u must be [n_rungs, n_per_rung], got shape {ua.shape}")
            keep.append(ua)
            spec.u, spec.n_rungs, spec.n_per_rung = ua.ctypes.data_as(dp), ua.shape[0], ua.shape[1]
            host = ua.shape
        elif w is not None:
            wa = _f32(w)
            if wa.ndim != 3 or wa.shape[2] != self.P:
                raise ValueError(f"w must be [n_rungs, n_per_rung, {self.P}], got shape {wa.shape}")
            keep.append(wa)
            spec.w, spec.n_rungs, spec.n_per_rung = _ptr(wa), wa.shape[0], wa.shape[1]
            host = wa.shape[:2]
        else:
            host = None
            K, per = self._trace_source(spec, keep, replicas, step0, nsteps, thin)
            total = K * per
        if host is not None:
            K = host[0]
            total = self._multiplicity(spec, keep, multiplicity, tuple(host),
                                       "multiplicity must be [n_rungs, n_per_rung] = {want}, got shape {got}")
        if d is not None:
            da = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
            if da.size != K:
                raise ValueError(f"d must have one exponent per rung ({K}), got {da.size}")
            keep.append(da)
            spec.d = da.ctypes.data_as(dp)
        aa = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        keep.append(aa)
        spec.n_prior, spec.seed, spec.n_a = int(n_prior), int(seed) & 0xFFFFFFFFFFFFFFFF, aa.size
        spec.a = aa.ctypes.data_as(dp) if aa.size else None
        out = {k: np.full(K, np.nan) for k in ("u_mean", "u_var", "u_ess", "log_stone", "stone_relvar")}
        out["n_draws"] = np.zeros(K, np.int64)
        for k in ("prior_log_mean_exp", "prior_kish_ess", "prior_u_mean", "prior_u_var"):
            out[k] = np.full(aa.size, np.nan)
        out["u"] = np.empty(max(total, 0)) if u_out else None
        out["u_prior"] = np.empty(max(int(n_prior), 0)) if u_prior_out else None
        _bind(spec, out, u="u_out", u_prior="u_prior_out")
        if d is None:
            spec.log_stone = spec.stone_relvar = None                   # no stones without exponents: they stay NaN
        return self._call(self.lib.ptnn_evidence, spec, out, counters=("n_distinct",))

    def mbar(self, betas, *, replicas=None, step0=0, nsteps=None, thin=1, w=None, u=None, b=None, multiplicity=None, n_prior=0, seed=0,
             u_prior=None, b_prior=None, effective=True, target_beta=1.0, tol=1e-10, max_iter=10000, n_resample=0, resample_seed=0,
             gram=True, draws=False, x=None, resample_w=False, item_map=False, sse=False):
        """ptnn_mbar: the multistate Bennett acceptance ratio over the rungs `betas` [K] (strictly ascending) and an optional prior
        state, on the device.  Source of the rungs: the trace rows step0, step0 + thin, ... < step0 + nsteps of `replicas` (None =
        all; one rung each, in the order of betas), host vectors w [K, n, P], or a host U [K, n] float64 with optional b [K, n];
        sources 2 and 3 take optional integer `multiplicity` [K, n].  The prior state: n_prior draws of the prior (Philox stream
        STREAM_PRIOR of `seed`), or host u_prior (and b_prior) [n_prior].  The items are the prior draws, then the rungs' rows.
        -> dict(f, n_eff [K'] float64 and gram [K', K'] (K' = K plus the prior state), n_iter, residual, log_weight [n_items]
        float64 at target_beta, weight_sum, kish_ess, max_weight_share, u and b [n_items] (draws), cum_weight [n_items], resample_u
        and resample_item [n_resample] int64 (n_resample > 0), resample_w [n_resample, P] float32 the drawn weight vectors
        (resample_w), mean and var [n_rows, O] float64 of the network outputs on the rows x ("train", "test" or [n_rows, n_in])
        under the weights (x given; like resample_w not with u or u_prior), item_chain, item_multiplicity int32 and item_step
        int64 [n_items] (item_map: chain or rung, step or row, -1 and the draw's number for a prior draw), sse [n_items] float64
        (sse; a regression), n_items, n_distinct); what was not asked for is None."""
        spec, keep = _spec(MbarSpec), []
        if x is not None:
            self._rows(spec, keep, x, "x", (self.cfg.n_in, "n_in columns"))
        dp = C.POINTER(C.c_double)
        ba = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        keep.append(ba)
        spec.betas, spec.n_rungs = ba.ctypes.data_as(dp), ba.size
        if b is not None and u is None:
            raise ValueError("b comes with a host U")
        if u is not None:
            ua = np.ascontiguousarray(u, dtype=np.float64)
            if ua.ndim != 2 or ua.shape[0] != ba.size:
                raise ValueError(f"u must be [n_rungs = {ba.size}, n_per_rung], got shape {ua.shape}")
            keep.append(ua)
            spec.u, spec.n_per_rung = ua.ctypes.data_as(dp), ua.shape[1]
            if b is not None:
                bb = np.ascontiguousarray(b, dtype=np.float64)
                if bb.shape != ua.shape:
                    raise ValueError(f"b must have the shape of u {ua.shape}, got {bb.shape}")
                keep.append(bb)
                spec.b = bb.ctypes.data_as(dp)
            host = ua.shape
        elif w is not None:
            wa = _f32(w)
            if wa.ndim != 3 or wa.shape[0] != ba.size or wa.shape[2] != self.P:
                raise ValueError(f"w must be [n_rungs = {ba.size}, n_per_rung, {self.P}], got shape {wa.shape}")
            keep.append(wa)
            spec.w, spec.n_per_rung = _ptr(wa), wa.shape[1]
            host = wa.shape[:2]
        else:
            host = None
            K, per = self._trace_source(spec, keep, replicas, step0, nsteps, thin)
            if K != ba.size:
                raise ValueError(f"{K} chains selected for {ba.size} betas")
            rows = K * per
        if host is not None:
            rows = int(np.prod(host))
            self._multiplicity(spec, keep, multiplicity, tuple(host), "multiplicity must be [n_rungs, n_per_rung] = {want}, got shape {got}")
        n_prior = int(n_prior)
        if u_prior is not None:
            up = np.ascontiguousarray(u_prior, dtype=np.float64).reshape(-1)
            keep.append(up)
            spec.u_prior, n_prior = up.ctypes.data_as(dp), up.size
            if b_prior is not None:
                bp = np.ascontiguousarray(b_prior, dtype=np.float64).reshape(-1)
                if bp.size != up.size:
                    raise ValueError(f"b_prior must have one entry per prior draw ({up.size}), got {bp.size}")
                keep.append(bp)
                spec.b_prior = bp.ctypes.data_as(dp)
        elif b_prior is not None:
            raise ValueError("b_prior comes with u_prior")
        spec.n_prior, spec.seed, spec.effective = n_prior, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if effective else 0
        spec.target_beta, spec.tol, spec.max_iter = float(target_beta), float(tol), int(max_iter)
        m = int(n_resample)
        spec.n_resample, spec.resample_seed = m, int(resample_seed) & 0xFFFFFFFFFFFFFFFF
        K1, nt = ba.size + (1 if n_prior > 0 else 0), max(n_prior, 0) + max(rows, 0)
        out = dict(f=np.full(K1, np.nan), gram=np.full((K1, K1), np.nan) if gram else None, n_eff=np.full(K1, np.nan),
                   log_weight=np.empty(nt), u=np.empty(nt) if draws else None, b=np.empty(nt) if draws else None,
                   cum_weight=np.empty(nt) if m > 0 else None, resample_item=np.empty(m, np.int64) if m > 0 else None,
                   resample_w=np.empty((m, self.P), np.float32) if resample_w else None,
                   mean=np.empty((spec.n_rows, self.cfg.n_out)) if x is not None else None,
                   var=np.empty((spec.n_rows, self.cfg.n_out)) if x is not None else None,
                   item_chain=np.empty(nt, np.int32) if item_map else None, item_multiplicity=np.empty(nt, np.int32) if item_map else None,
                   item_step=np.empty(nt, np.int64) if item_map else None, sse=np.empty(nt) if sse else None)
        _bind(spec, out, u="u_out", b="b_out")
        scal = {k: C.c_double(float("nan")) for k in ("residual", "weight_sum", "kish_ess", "max_weight_share", "resample_u")}
        for k, v in scal.items():
            setattr(spec, k, C.pointer(v))
        self._call(self.lib.ptnn_mbar, spec, out, counters=("n_iter", "n_items", "n_distinct"))
        out.update((k, v.value) for k, v in scal.items())
        return out

    def langevin_gradient(self, w):
        w = _f32(np.atleast_2d(w))
        out = np.empty_like(w)
        self._check(self.lib.ptnn_langevin_gradient(self.h, _ptr(w), w.shape[0], _ptr(out)))
        return out

    def time_sgd_epoch(self, w, reps=200, pair=False):
        """Milliseconds one sequential SGD epoch of one chain takes on the device (in-kernel constant-rate counter); pair=True
        (wide nets): (one epoch, a pair of epochs through one row loop)."""
        w = _f32(w).reshape(-1)
        ms = (C.c_double * 2)()
        self._check(self.lib.ptnn_time_sgd_epoch(self.h, _ptr(w), int(reps), ms))
        return (ms[0], ms[1]) if pair else ms[0]

    def time_tree_round(self, w, reps=200, xcd_local=True):
        """(forward pass ms, one granule one way ms, went through the XCD's L2?) -- ptnn_time_tree_round."""
        w = _f32(w).reshape(-1)
        ms = (C.c_double * 3)()
        self._check(self.lib.ptnn_time_tree_round(self.h, _ptr(w), int(reps), int(bool(xcd_local)), ms))
        return ms[0], ms[1], bool(ms[2])

    def tape(self, replica, step):
        noise, scal = np.empty(self.P, np.float32), np.empty(3, np.float32)
        self._check(self.lib.ptnn_tape(self.h, int(replica), int(step), _ptr(noise), _ptr(scal)))
        return noise, scal

    def debug_stamps(self):
        buf = (C.c_uint64 * 160)()
        self._check(self.lib.ptnn_debug_stamps(self.h, buf))
        return list(buf)

    def describe(self):
        """What the handle launches (kernel, grid, LDS, occupancy) as a dict; see ptnn_describe.  "swap_rounds" says how a swap round
        runs -- "pipelined (ring 4)" (replica k waits for replicas 0 .. k+1 only), "grid barrier", "in-kernel exchange" (tree, packed
        over several CUs) or "between launches" -- and "swap_ring_depth" the rounds the pipelined path buffers (0 elsewhere)."""
        import json
        buf = C.create_string_buffer(2048)
        self._check(self.lib.ptnn_describe(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def kernel_time(self, reset=False):
        n, ms = C.c_int64(), C.c_double()
        self._check(self.lib.ptnn_kernel_time(self.h, int(reset), C.byref(n), C.byref(ms)))
        return n.value, ms.value


def savetxt(path, array, fmt, append=False):
    """np.savetxt(path, array, fmt=fmt) for 1-D / 2-D arrays, byte for byte, formatted by the C library (GIL released).  float32
    arrays (the device's traces, also row-strided views of them) are written as they are; anything else goes through float64."""
    lib = load_library()
    a = np.asarray(array)
    if a.ndim not in (1, 2):
        raise ValueError("savetxt handles 1-D and 2-D arrays")
    if a.dtype == np.float32 and a.size and a.strides[-1] == 4 and (a.ndim == 1 or (a.strides[0] % 4 == 0 and a.strides[0] >= 4 * a.shape[1])):
        rows, cols, stride = (a.shape[0], 1, 1) if a.ndim == 1 else (a.shape[0], a.shape[1], a.strides[0] // 4)
        rc = lib.ptnn_savetxt_f32(os.fsencode(path), a.ctypes.data_as(_fp), rows, cols, stride, fmt.encode(), int(bool(append)))
    else:
        if append:
            raise ValueError("append mode takes float32 data")
        a = np.ascontiguousarray(a, dtype=np.float64)
        rows, cols = (a.shape[0], 1) if a.ndim == 1 else a.shape
        rc = lib.ptnn_savetxt(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_double)), rows, cols, fmt.encode())
    if rc < 0:
        raise PtnnError(lib.ptnn_last_error().decode())


def savetxt_batch(jobs, append=False, threads=8):
    """savetxt(path, array, fmt) for every (path, array, fmt) of `jobs` in ONE call into the C library, which spreads the files over
    `threads` host threads in the order given.  float32 arrays (1-D, or 2-D with unit column stride) only: the per-chain files of a
    window of trace rows."""
    lib = load_library()
    n = len(jobs)
    if n == 0:
        return
    paths, data, fmts = (C.c_char_p * n)(), (_fp * n)(), (C.c_char_p * n)()
    rows, cols, strides = (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
    keep = []
    for k, (path, array, fmt) in enumerate(jobs):
        a = np.asarray(array)
        if a.dtype != np.float32 or a.ndim not in (1, 2) or a.strides[-1] != 4 or (a.ndim == 2 and (a.strides[0] % 4 or a.strides[0] < 4 * a.shape[1])):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim not in (1, 2):
                raise ValueError("savetxt handles 1-D and 2-D arrays")
        keep.append(a)
        paths[k], fmts[k] = os.fsencode(path), fmt.encode()
        data[k] = a.ctypes.data_as(_fp)
        rows[k], cols[k], strides[k] = (a.shape[0], 1, 1) if a.ndim == 1 else (a.shape[0], a.shape[1], a.strides[0] // 4)
    if lib.ptnn_savetxt_f32_batch(n, paths, data, rows, cols, strides, fmts, int(bool(append)), int(threads)) < 0:
        raise PtnnError(lib.ptnn_last_error().decode())


def _chunks(n, threads, grain=65536):
    k = max(1, min(int(threads), n // grain + 1))
    b = np.linspace(0, n, k + 1).astype(np.int64)
    return [(int(b[i]), int(b[i + 1])) for i in range(k) if b[i + 1] > b[i]]


def text_round(array, fmt, threads=8):
    """Values as np.loadtxt reads them back after np.savetxt(..., fmt=fmt), float64, in the C library (exact integer arithmetic
    for the '%1.Nf' formats, no strings), chunked over a few threads (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    lib = load_library()
    src = np.asarray(array)
    f32 = src.dtype == np.float32
    src = np.ascontiguousarray(src, dtype=np.float32 if f32 else np.float64)
    out = np.empty(src.shape, dtype=np.float64) if f32 else np.array(src, copy=True)
    n = out.size
    if n == 0:
        return out
    flat_in, flat = src.reshape(-1), out.reshape(-1)
    dp = C.POINTER(C.c_double)

    def work(rng):
        lo, hi = rng
        if f32:
            rc = lib.ptnn_text_round_f32(flat_in[lo:hi].ctypes.data_as(_fp), flat[lo:hi].ctypes.data_as(dp), hi - lo, fmt.encode())
        else:
            rc = lib.ptnn_text_round(flat[lo:hi].ctypes.data_as(dp), hi - lo, fmt.encode())
        if rc < 0:
            raise PtnnError(lib.ptnn_last_error().decode())
    parts = _chunks(n, threads)
    if len(parts) == 1:
        work(parts[0])
    else:
        with ThreadPoolExecutor(max_workers=len(parts)) as ex:
            list(ex.map(work, parts))
    return out


def posterior_matrix(pos_w, first_row, threads=8):
    """pos_w float32 [R, S, P] -> float64 [P, R * (S - first_row)]: rows from first_row on, chains side by side, transposed
    (what show_results returns as pos_w, REG:795-797, 848)."""
    lib = load_library()
    a = np.asarray(pos_w)
    R, S, P = a.shape
    # the padded rows of a trace image are read in place; anything else is made dense first
    if not (a.dtype == np.float32 and a.strides[2] == 4 and a.strides[1] % 4 == 0 and a.strides[1] >= 4 * P and a.strides[0] == S * a.strides[1]):
        a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty((P, R * (S - first_row)), dtype=np.float64)
    if lib.ptnn_posterior_matrix(a.ctypes.data_as(_fp), R, S, P, a.strides[1] // 4, int(first_row), out.ctypes.data_as(C.POINTER(C.c_double)),
                                 int(threads)) < 0:
        raise PtnnError(lib.ptnn_last_error().decode())
    return out
