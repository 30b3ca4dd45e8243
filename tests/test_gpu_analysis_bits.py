"""The work-group reductions and scans of the posterior-analysis kernels (csrc/ptnn_dev_wg.hpp) held BIT FOR BIT to the outputs
recorded before they were gathered into one header (tests/golden/analysis_bits_parent.npz, written by
profiles/tools/record_analysis_bits.py on the commit before that change): the helpers may change how the source reads, never an
operation, its order or a barrier.

One call each of predict, sensitivity, elpd, lfo, evidence, calibration, ppc, powerscale and prior_predictive on a regression
net (4-5-1) and a classification net (4-12-3) with 24 data rows, from host-given samples: U distinct vectors with multiplicities
2 .. 4, U = 100 (threads of the 256-wide trees hold the identity), 256 (one item per thread) and 300 (the strided second pass;
the ragged last chunk of powerscale's prefix sums).  Every output of every call is compared as bits, a NaN with a NaN.  One
headline output per call is also held to the float64 reference of that analysis's own GPU test at that test's tolerance, so a
golden recorded from a broken build fails here on its own account.

A second list of calls -- partial_dependence, coalition_values, class_report, uncertainty, influence (of the predictions and of
the log-likelihoods), forecast, sensitivity with sample_abs and predict with samples -- is held in the same way to
tests/golden/analysis_bits_parent2.npz, recorded on the commit before the host code of these calls was folded onto shared paths
(the rows-by-vectors frame, the summary of signed columns, the pooled votes, the log-likelihood of rows): the same cases, every
output as bits.  Each case runs a second time with every call's scratch budget at five rows' worth, so 24 rows take five blocks
with a ragged last one, and is held to the same recorded bits: the shared helpers' `last` flag and row offsets live on that path,
and no output depends on the blocking.

A third list is held to tests/golden/analysis_bits_parent3.npz, recorded on the commit before the scored calls (elpd, lfo,
calibration, forecast_score, ppc, powerscale, uncertainty, influence) were given the rows-by-vectors frame, calibration and
forecast_score one body for the predictive-mixture columns, and evidence and mbar one rung layout.  forecast_score (regression
net) in four runs: noise off with the pair term, the energy score, three levels, samples and means; noise on; noise off with the
scratch at five origins' worth; and with the scratch below one origin's horizon and the energy score off, which splits the
horizon.  mbar from host vectors [2, U / 2, P] with multiplicities, U prior draws, effective sample sizes, mean and var on the
train rows and resampling, and from a host u / b.  And elpd (with loglik_out), lfo, calibration, ppc, powerscale and evidence of
the first list again with their scratch at five rows' worth (ppc: 64 vectors' worth, so U = 100 takes two blocks, the second
ragged): where the blocking changes the order of a sum (powerscale's l_u, evidence's U) these bits need not be the unblocked
ones, so they are recorded as arrays of their own.  The outputs in the selection's order (elpd's loglik, forecast_score's samples
and means) are asked for in every case and recorded at U = 100 only, samples and means not with the noise on (every occurrence is
a trajectory of its own there: two incompressible [M, 24, 6] arrays), to keep the file within the size of the second golden; the
per-row and per-column outputs beside them are functions of every one of their entries."""
import hashlib
import tempfile

import numpy as np
import pytest

import calibration_ref
import elpd_ref
import evidence_ref
import lfo_ref
import parity
import prior_ref
from parity import orc
from test_gpu_analysis_shapes import _data, _vectors
from test_gpu_calibration import _check_oracle_forward
from test_gpu_elpd import ATOL, _oracle_ll
from test_gpu_fscore import _check_against_ref as fscore_check_against_ref
from test_gpu_mbar import TOL as MBAR_TOL, _dev as mbar_dev, _reference as mbar_reference
from test_gpu_powerscale import check_oracle as powerscale_check_oracle
from test_gpu_ppc import check_occurrences
from test_gpu_predict import _outputs, _pt
from test_gpu_sensitivity import _worst_ratio
from test_prior_cpu import ATOL as PRIOR_ATOL, RTOL as PRIOR_RTOL

pytestmark = pytest.mark.gpu

GOLDEN_FILE = "analysis_bits_parent.npz"
REG, CLS = orc.TASK_REG, orc.TASK_CLS
NETS = {"reg": (REG, (4, 5, 1)), "cls": (CLS, (4, 12, 3))}
US = (100, 256, 300)
N_ROWS = 24
CASES = [(net, U) for net in NETS for U in US]
CALLS = ("predict", "sensitivity", "elpd", "lfo", "evidence", "calibration", "ppc", "powerscale", "prior_predictive")
N_FIT, ORIGINS, BLOCK = 16, (8, 12, 16, 20), 2
LAGS = (1, 2, 3)
QUANTILES = (0.05, 0.5, 0.95)
STONES = (0.3, 0.0)                   # evidence: two rungs of U / 2 vectors each
PRIOR_A = (0.0, 0.5)
SEED = 0x5EED_0000_0B17
EPS = 0.01
# the second list
GOLDEN_FILE2 = "analysis_bits_parent2.npz"
CALLS2 = ("partial_dependence", "coalition_values", "class_report", "uncertainty", "influence_prediction", "influence_loglik",
          "forecast", "sensitivity_sample_abs", "predict_samples")
CALLS2_OF = {"reg": tuple(c for c in CALLS2 if c != "class_report"), "cls": tuple(c for c in CALLS2 if c != "forecast")}
N_GRID, N_BACKGROUND, N_TERMS, HORIZON = 5, 8, 4, 6
BLOCK_ROWS = 5                        # rows per block of the blocked run: 24 rows in blocks of 5, 5, 5, 5 and 4
# the third list
GOLDEN_FILE3 = "analysis_bits_parent3.npz"
FSCORE_RUNS = ("fscore_noise_off", "fscore_noise_on", "fscore_origin_blocks", "fscore_split_horizon")
MBAR_RUNS = ("mbar_vectors", "mbar_host_u")
BLOCKED = ("elpd", "lfo", "calibration", "ppc", "powerscale", "evidence")
CALLS3_OF = {"reg": FSCORE_RUNS + MBAR_RUNS + tuple(c + "_blocked" for c in BLOCKED),
             "cls": MBAR_RUNS + tuple(c + "_blocked" for c in BLOCKED)}
BETAS = (0.5, 1.0)                    # mbar: two rungs of U / 2 vectors each
N_RESAMPLE = 64
PPC_BLOCK_VECTORS = 64
U_WITH_SAMPLES = 100                  # the outputs in the selection's order are recorded at this U only

_HANDLES = {}


def handle(net):
    """(ParallelTempering object, its training rows): one per net for the whole module, 24 rows, no run (every sample is
    host-given)."""
    if net not in _HANDLES:
        task, topo = NETS[net]
        train, test = _data(task, topo, 11 + task, n_tr=N_ROWS, n_te=N_ROWS)
        kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
        tmp = tempfile.TemporaryDirectory()                           # (nothing is written: write_files=False)
        _HANDLES[net] = (_pt(task, topo, train, test, 4, 20, tmp.name, **kw), train, tmp)
    return _HANDLES[net][:2]


def samples(net, U):
    """(distinct vectors [U, P] fp32, eta [U] fp32 or None, multiplicities [U] in 2 .. 4)."""
    task, topo = NETS[net]
    w = _vectors(topo, U, 1000 * task + U, spread=0.2)
    rng = np.random.default_rng(7 * U + task)
    mult = rng.integers(2, 5, U).astype(np.int32)
    eta = rng.normal(-3.0, 0.3, U).astype(np.float32) if task == REG else None
    return w, eta, mult


def run_calls(pt, net, U):
    """{call: the binding's whole result} of the nine calls of one case."""
    task, topo = NETS[net]
    s = pt._sampler
    w, eta, mult = samples(net, U)
    M = int(mult.sum())
    ranks = (0, M // 2, M - 1)
    groups = [g for g in ("weights", "eta", "predictions", "loglik") if g != "eta" or task == REG]
    out = {}
    out["predict"] = s.predict("train", w=w, multiplicity=mult, ranks=ranks, vote=task == CLS)
    out["sensitivity"] = s.sensitivity("train", w=w, multiplicity=mult, ranks=ranks, ranks2=ranks)
    out["elpd"] = s.elpd("train", w=w, eta=eta, multiplicity=mult)
    out["lfo"] = s.lfo("train", n_fit=N_FIT, origins=ORIGINS, block=BLOCK, w=w, eta=eta, multiplicity=mult)
    out["evidence"] = s.evidence(w=w.reshape(2, U // 2, -1), multiplicity=mult.reshape(2, U // 2), d=STONES, n_prior=U, seed=SEED,
                                 a=PRIOR_A, u_out=True, u_prior_out=True)
    out["calibration"] = s.calibration("train", w=w, eta=eta, multiplicity=mult, quantiles=QUANTILES if task == REG else ())
    out["ppc"] = s.ppc("train", w=w, eta=eta, multiplicity=mult, lags=LAGS if task == REG else (), seed=SEED, samples=False)
    out["powerscale"] = s.powerscale("train", groups=groups, w=w, eta=eta, multiplicity=mult)
    out["prior_predictive"] = s.prior_predictive("train", n_draws=U, seed=SEED, ranks=(0, U // 2, U - 1), eps=EPS, t_draw=True)
    assert tuple(out) == CALLS
    # the sort and the exclusive scan of psis_reduce run only with more than 4 tail entries
    assert out["elpd"]["tail_len"].min() > 4 and out["lfo"]["tail_len"].max() > 4, (out["elpd"]["tail_len"], out["lfo"]["tail_len"])
    return out


def scratch_budgets(net, U):
    """{call of the second list: (its scratch variable, the bytes that hold BLOCK_ROWS rows of its block at U distinct vectors)}:
    the row sizes are those of the calls' own budget arithmetic (fp32 columns per row and distinct vector; ptnn_influence gives a
    quarter of its budget to the block of targets, whose rows carry their double columns beside the forward image)."""
    task, (I, _, O) = NETS[net]
    row = 4 * U
    return {
        "partial_dependence": ("PTNN_PD_SCRATCH_BYTES", BLOCK_ROWS * row * I * N_GRID * O),
        "coalition_values": ("PTNN_SHAP_SCRATCH_BYTES", BLOCK_ROWS * row * O * N_TERMS),
        "class_report": ("PTNN_REPORT_SCRATCH_BYTES", BLOCK_ROWS * row * O),
        "uncertainty": ("PTNN_UNC_SCRATCH_BYTES", BLOCK_ROWS * row * (O + (task == CLS))),
        "influence_prediction": ("PTNN_INFLUENCE_SCRATCH_BYTES", 4 * BLOCK_ROWS * (row * O + 8 * U * O)),
        "influence_loglik": ("PTNN_INFLUENCE_SCRATCH_BYTES", 4 * BLOCK_ROWS * (row * O + 8 * U)),
        "forecast": ("PTNN_FORECAST_SCRATCH_BYTES", BLOCK_ROWS * row * HORIZON),
        "sensitivity_sample_abs": ("PTNN_SENSITIVITY_SCRATCH_BYTES", BLOCK_ROWS * row * O * I),
        "predict_samples": ("PTNN_PREDICT_SCRATCH_BYTES", BLOCK_ROWS * row * O),
    }


def run_calls2(pt, net, U, setenv=None):
    """{call: the binding's whole result} of the second list of one case; with `setenv` (monkeypatch.setenv) every call runs with
    its scratch budget at BLOCK_ROWS rows."""
    task, (I, _, O) = NETS[net]
    s = pt._sampler
    _, train = handle(net)
    w, eta, mult = samples(net, U)
    M = int(mult.sum())
    ranks = (0, M // 2, M - 1)
    src = dict(w=w, multiplicity=mult)
    X = np.asarray(train, np.float32)[:, :I]
    grid = np.percentile(X, np.linspace(5, 95, N_GRID), axis=0).T.astype(np.float32)                     # [I, N_GRID]
    rng = np.random.default_rng(31 * U + task)
    coef = rng.normal(0.0, 1.0, (1 << I, N_TERMS))
    calls = {
        "partial_dependence": lambda: s.partial_dependence("train", grid=grid, ranks=ranks, ranks2=ranks, ice_mean=True, sample_pd=True,
                                                           sample_range=True, **src),
        "coalition_values": lambda: s.coalition_values("train", background=X[:N_BACKGROUND], masks=np.arange(1 << I, dtype=np.uint64),
                                                       coef=coef, ranks=ranks, ranks2=ranks, counts=True, sample_abs=True, **src),
        "class_report": lambda: s.class_report("train", ranks=ranks, auc=True, sample_confusion=True, **src),
        "uncertainty": lambda: s.uncertainty("train", eta=eta, ranks=ranks, samples=True, **src),
        "influence_prediction": lambda: s.influence("test", "train", of="prediction", eta=eta, **src),
        "influence_loglik": lambda: s.influence("test", "train", of="loglik", eta=eta, **src),
        "forecast": lambda: s.forecast(HORIZON, "train", eta=eta, ranks=ranks, **src),
        "sensitivity_sample_abs": lambda: s.sensitivity("train", ranks=ranks, ranks2=ranks, sample_abs=True, **src),
        "predict_samples": lambda: s.predict("train", ranks=ranks, vote=task == CLS, samples=True, **src),
    }
    budgets = scratch_budgets(net, U)
    out = {}
    for call in CALLS2_OF[net]:
        if setenv:
            setenv(budgets[call][0], str(budgets[call][1]))
        out[call] = calls[call]()
    return out


def truth_of(U):
    """forecast_score's observations [N_ROWS, HORIZON] fp32: one in seven missing, the last origin with its first step only."""
    rng = np.random.default_rng(97 * U)
    truth = rng.normal(0.5, 0.2, (N_ROWS, HORIZON)).astype(np.float32)
    truth[rng.random((N_ROWS, HORIZON)) < 1.0 / 7.0] = np.nan
    truth[-1, 0], truth[-1, 1:] = 0.5, np.nan
    return truth


def host_u_of(U):
    """mbar's host source: (u, b [2, U / 2], u_prior, b_prior [U]) float64."""
    rng = np.random.default_rng(53 * U)
    return (rng.normal(-30.0, 2.0, (2, U // 2)), rng.normal(1.0, 0.3, (2, U // 2)), rng.normal(-60.0, 8.0, U), rng.normal(0.0, 0.5, U))


def scratch_budgets3(net, U):
    """{call of the third list that runs blocked: (its scratch variable, the bytes of its blocks)}, by the calls' own budget
    arithmetic: BLOCK_ROWS rows of fp32 outputs per distinct vector (elpd with loglik_out and powerscale: and a double beside
    them; lfo gives half of its budget to the rows), ppc PPC_BLOCK_VECTORS vectors with all rows, forecast_score BLOCK_ROWS
    origins of HORIZON steps, or one step less than a vector's window and one step hold (the horizon splits into single steps)."""
    task, (I, _, O) = NETS[net]
    row = 4 * U
    return {
        "elpd_blocked": ("PTNN_ELPD_SCRATCH_BYTES", BLOCK_ROWS * U * (4 * O + 8)),
        "lfo_blocked": ("PTNN_LFO_SCRATCH_BYTES", 2 * BLOCK_ROWS * row * O),
        "calibration_blocked": ("PTNN_CALIB_SCRATCH_BYTES", BLOCK_ROWS * row * O),
        "ppc_blocked": ("PTNN_PPC_SCRATCH_BYTES", PPC_BLOCK_VECTORS * N_ROWS * O * 4),
        "powerscale_blocked": ("PTNN_POWERSCALE_SCRATCH_BYTES", BLOCK_ROWS * U * (4 * O + 8)),
        "evidence_blocked": ("PTNN_EVIDENCE_SCRATCH_BYTES", BLOCK_ROWS * row * O),
        "fscore_origin_blocks": ("PTNN_FSCORE_SCRATCH_BYTES", BLOCK_ROWS * row * HORIZON),
        "fscore_split_horizon": ("PTNN_FSCORE_SCRATCH_BYTES", row * (I + 1)),
    }


def run_calls3(pt, net, U, setenv, delenv):
    """{call: the binding's whole result} of the third list of one case; every scratch variable is set for its call alone."""
    task, (I, _, O) = NETS[net]
    s = pt._sampler
    w, eta, mult = samples(net, U)
    src = dict(w=w, eta=eta, multiplicity=mult)
    groups = [g for g in ("weights", "eta", "predictions", "loglik") if g != "eta" or task == REG]
    truth = truth_of(U)
    fscore = dict(quantiles=QUANTILES, seed=SEED, samples=True, means=True, **src)
    u, b, u_prior, b_prior = host_u_of(U)
    mult2 = mult.reshape(2, U // 2)
    calls = {
        "fscore_noise_off": lambda: s.forecast_score(HORIZON, "train", truth, noise=False, **fscore),
        "fscore_noise_on": lambda: s.forecast_score(HORIZON, "train", truth, noise=True, **fscore),
        "fscore_origin_blocks": lambda: s.forecast_score(HORIZON, "train", truth, noise=False, **fscore),
        "fscore_split_horizon": lambda: s.forecast_score(HORIZON, "train", truth, noise=False, energy=False, **fscore),
        "mbar_vectors": lambda: s.mbar(BETAS, w=w.reshape(2, U // 2, -1), multiplicity=mult2, n_prior=U, seed=SEED, effective=True, x="train",
                                       n_resample=N_RESAMPLE, resample_seed=SEED + 1, resample_w=True, draws=True, item_map=True,
                                       sse=task == REG),
        "mbar_host_u": lambda: s.mbar(BETAS, u=u, b=b, multiplicity=mult2, u_prior=u_prior, b_prior=b_prior, effective=True,
                                      n_resample=N_RESAMPLE, resample_seed=SEED + 1, draws=True, item_map=True),
        "elpd_blocked": lambda: s.elpd("train", loglik_out=True, **src),
        "lfo_blocked": lambda: s.lfo("train", n_fit=N_FIT, origins=ORIGINS, block=BLOCK, **src),
        "calibration_blocked": lambda: s.calibration("train", quantiles=QUANTILES if task == REG else (), **src),
        "ppc_blocked": lambda: s.ppc("train", lags=LAGS if task == REG else (), seed=SEED, samples=False, **src),
        "powerscale_blocked": lambda: s.powerscale("train", groups=groups, **src),
        "evidence_blocked": lambda: s.evidence(w=w.reshape(2, U // 2, -1), multiplicity=mult2, d=STONES, n_prior=U, seed=SEED, a=PRIOR_A,
                                               u_out=True, u_prior_out=True),
    }
    budgets = scratch_budgets3(net, U)
    out = {}
    for call in CALLS3_OF[net]:
        if call in budgets:
            setenv(budgets[call][0], str(budgets[call][1]))
        out[call] = calls[call]()
        if call in budgets:
            delenv(budgets[call][0])
    return out


def recorded3(out, U):
    """`out` as the third golden file holds it: the outputs in the selection's order at U_WITH_SAMPLES only -- elpd's loglik, and
    forecast_score's samples and means: never with the noise on, and of the blocked runs the samples alone."""
    out = {call: dict(res) for call, res in out.items()}
    for call in FSCORE_RUNS:
        if call in out:
            keep = () if U != U_WITH_SAMPLES or call == "fscore_noise_on" else ("samples", "means") if call == "fscore_noise_off" else ("samples",)
            out[call].update((k, None) for k in ("samples", "means") if k not in keep)
    if U != U_WITH_SAMPLES:
        out["elpd_blocked"]["loglik"] = None
    return out


def key(net, U, call, name):
    return f"{net}_U{U}_{call}_{name}"


def digest(net, U, train):
    """The inputs of a case, as 32 bytes."""
    h = hashlib.sha256()
    for a in samples(net, U) + (np.asarray(train, np.float64),):
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def record():
    """Everything the golden file holds: per case the digest of its inputs and every output of every call as it is (npz keeps the
    bits of a float array); a count the binding returns as an int becomes an int64 array."""
    rec = {}
    for net, U in CASES:
        pt, train = handle(net)
        rec[key(net, U, "inputs", "sha256")] = digest(net, U, train)
        for call, res in run_calls(pt, net, U).items():
            for name, v in res.items():
                if v is not None:
                    rec[key(net, U, call, name)] = np.asarray(v)
    return rec


def record2():
    """The second golden file: the digests again, and every output of the second list."""
    rec = {}
    for net, U in CASES:
        pt, train = handle(net)
        rec[key(net, U, "inputs", "sha256")] = digest(net, U, train)
        for call, res in run_calls2(pt, net, U).items():
            for name, v in res.items():
                if v is not None:
                    rec[key(net, U, call, name)] = np.asarray(v)
    return rec


def record3():
    """The third golden file: the digests again, and every output of the third list."""
    import os
    rec = {}
    for net, U in CASES:
        pt, train = handle(net)
        rec[key(net, U, "inputs", "sha256")] = digest(net, U, train)
        for call, res in recorded3(run_calls3(pt, net, U, os.environ.__setitem__, os.environ.__delitem__), U).items():
            for name, v in res.items():
                if v is not None:
                    rec[key(net, U, call, name)] = np.asarray(v)
    return rec


def same_bits(got, want):
    """Element-wise: the same bits, or both NaN (a commuted fmax or add may pick the other payload)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return np.zeros(1, bool)
    if got.dtype.kind != "f":
        return got == want
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


_GOLDEN = {}


def golden(file=GOLDEN_FILE):
    if file not in _GOLDEN:
        _GOLDEN[file] = parity.golden(file)
    return _GOLDEN[file]


def check_references(pt, net, U, train, out):
    """One headline output per call against the float64 reference of that analysis's own GPU test, at its tolerance."""
    task, topo = NETS[net]
    I = topo[0]
    s = pt._sampler
    w, eta, mult = samples(net, U)
    M = int(mult.sum())
    c = mult.astype(np.float64)
    X = train[:, :I]
    y = train[:, I].astype(np.float32).astype(np.float64)
    f_or = _outputs(task, X, w.T.astype(np.float64), topo)                               # [U, n_rows, O]
    # predict (test_gpu_predict.py: the outputs within 1e-5 of the oracle's) -- the weighted mean of values within 1e-5
    assert np.max(np.abs(out["predict"]["mean"] - np.tensordot(c, f_or, 1) / M)) <= 1e-5
    # sensitivity (test_gpu_sensitivity.py: _worst_ratio's bound on every gradient, the mean against numpy) on a second call's samples
    sens = s.sensitivity("train", w=w, multiplicity=mult, samples=True)
    for k in ("grad_mean", "pos_count", "neg_count", "abs_mean", "sq_mean"):
        assert same_bits(sens[k], out["sensitivity"][k]).all(), k
    at = np.cumsum(mult) - mult
    _worst_ratio(sens["samples"][at], X, w, topo, task)
    np.testing.assert_allclose(out["sensitivity"]["grad_mean"], sens["samples"].astype(np.float64).mean(axis=0), rtol=1e-12, atol=0)
    # elpd (test_gpu_elpd.py: _check_oracle)
    ll = _oracle_ll(task, train, w.T, topo, eta)
    r = elpd_ref.elpd_rows(ll, mult)
    np.testing.assert_allclose(out["elpd"]["lppd"], r["lppd"], rtol=1e-5, atol=ATOL)
    np.testing.assert_allclose(out["elpd"]["elpd_loo"], r["elpd_loo"], rtol=1e-5, atol=ATOL)
    # lfo (test_gpu_lfo.py: _check_oracle)
    r = lfo_ref.lfo_rows(ll, N_FIT, ORIGINS, BLOCK, multiplicity=mult)
    K = np.abs(np.asarray(ORIGINS) - N_FIT) + BLOCK
    assert np.all(np.abs(out["lfo"]["elpd_lfo"] - r["elpd_lfo"]) <= 1e-5 * np.abs(r["elpd_lfo"]) + ATOL * K)
    # evidence (test_gpu_evidence.py: test_u_against_the_oracle)
    ev = out["evidence"]
    u = ev["u"]
    np.testing.assert_allclose(u, np.repeat(evidence_ref.u_and_b_batched(task, train, w, topo)[0], mult), rtol=1e-5, atol=1e-4)
    off = np.concatenate([[0], np.cumsum(mult.reshape(2, -1).sum(axis=1))])
    for k in range(2):
        st = evidence_ref.rung_stats(u[off[k]:off[k + 1]], STONES[k])
        assert ev["n_draws"][k] == off[k + 1] - off[k]
        assert ev["u_mean"][k] == pytest.approx(st["mean"], rel=1e-12)
        assert ev["log_stone"][k] == pytest.approx(st["log_stone"], rel=1e-12, abs=1e-12)
    up = ev["u_prior"]
    bp = np.zeros(up.size) if task == CLS else 2.0 * up / N_ROWS
    for j, a in enumerate(PRIOR_A):
        p = evidence_ref.prior_stats(up, bp, a)
        assert ev["prior_u_mean"][j] == pytest.approx(p["u_mean"], rel=1e-9)
        assert ev["prior_kish_ess"][j] == pytest.approx(p["kish"], rel=1e-9)
    # calibration (test_gpu_calibration.py: the CRPS against the oracle's forward pass; a classification's p_mean is predict's mean)
    cal = out["calibration"]
    if task == REG:
        _, crps_or, _ = _check_oracle_forward(None, train, w.T, topo, eta, mult)
        np.testing.assert_allclose(cal["crps"], crps_or, rtol=1e-5, atol=ATOL)
        np.testing.assert_allclose(cal["pred_mean"], out["predict"]["mean"][:, 0], rtol=1e-12)
        fx = s.predict("train", w=w, samples=True, mean=False)["samples"][:, :, 0]          # the device's own outputs [U, n_rows]
        for k, p in enumerate(QUANTILES):
            for n in range(N_ROWS):
                assert abs(calibration_ref.mixture_cdf(cal["quantiles"][k][n], fx[:, n], eta, mult) - p) <= 1e-12, (p, n)
    else:
        assert np.array_equal(cal["p_mean"], out["predict"]["mean"])
    # ppc (test_gpu_ppc.py: check_occurrences on the samples of a second call)
    ppc = s.ppc("train", w=w, eta=eta, multiplicity=mult, lags=LAGS if task == REG else (), seed=SEED, samples=True)
    for k in ("n_defined", "n_greater", "n_equal", "mean_obs", "mean_rep", "var_rep"):
        assert same_bits(ppc[k], out["ppc"][k]).all(), k
    check_occurrences(ppc)
    assert ppc["n_defined"].max() == M
    # powerscale (test_gpu_powerscale.py: check_oracle)
    powerscale_check_oracle(pt, "train", w, eta, mult, out["powerscale"], groups=("weights", "eta", "predictions", "loglik"))
    # prior_predictive (test_gpu_prior.py: check_statistics on the samples of a second call)
    pr = s.prior_predictive("train", n_draws=U, seed=SEED, eps=EPS, t_draw=True, samples=True)
    got = out["prior_predictive"]
    assert same_bits(pr["t_draw"], got["t_draw"]).all()
    t, _ = (prior_ref.regression if task == REG else prior_ref.classification)(pr["samples"][0], y, EPS)
    np.testing.assert_allclose(got["t_draw"][0], t, rtol=PRIOR_RTOL, atol=PRIOR_ATOL)
    want = prior_ref.summarise(got["t_draw"][0], got["t_obs"])
    np.testing.assert_allclose(got["stat_mean"][0], want["mean"], rtol=PRIOR_RTOL, atol=PRIOR_ATOL)
    np.testing.assert_allclose(got["stat_sd"][0], want["sd"], rtol=PRIOR_RTOL, atol=PRIOR_ATOL)
    assert np.array_equal(got["n_defined"][0], want["n_defined"])
    f32 = pr["samples"][0].astype(np.float64)
    assert np.array_equal(got["sat_count"][0], np.sum((f32 < EPS) | (f32 > 1.0 - EPS), axis=0))


def assert_recorded(g, net, U, train, out):
    """Every output of `out` has the recorded bits, and nothing recorded for the case is missing."""
    assert np.array_equal(digest(net, U, train), g[key(net, U, "inputs", "sha256")]), "the inputs are not the recorded ones"
    seen = set()
    for call, res in out.items():
        for name, v in res.items():
            k = key(net, U, call, name)
            if v is None:
                assert k not in g, k
                continue
            seen.add(k)
            got, want = np.asarray(v), g[k]
            same = same_bits(got, want)
            assert same.all(), f"{k}: {int((~same).sum())} of {same.size} values differ, first at {np.argwhere(~same)[0]}"
    assert seen == {k for k in g if k.startswith(f"{net}_U{U}_") and "_inputs_" not in k}, "an output of the recording is missing"


@pytest.mark.parametrize("net,U", CASES, ids=[f"{n}-U{u}" for n, u in CASES])
def test_outputs_equal_the_parent_commit(net, U):
    pt, train = handle(net)
    out = run_calls(pt, net, U)
    assert_recorded(golden(), net, U, train, out)
    check_references(pt, net, U, train, out)


def check_references2(net, U, out):
    """The second list against itself and against numpy: the three calls that pool the classifier agree on its mean and votes, a
    mean is the mean of the samples beside it, the curve is the row mean of ICE."""
    _, _, mult = samples(net, U)
    M = int(mult.sum())
    pred, unc = out["predict_samples"], out["uncertainty"]
    assert pred["n_samples"] == M and pred["n_distinct"] == U
    np.testing.assert_allclose(pred["mean"], pred["samples"].astype(np.float64).mean(axis=0), rtol=1e-12, atol=0)
    assert same_bits(unc["mean"], pred["mean"]).all()
    if NETS[net][0] == CLS:
        rep = out["class_report"]
        assert same_bits(rep["p_mean"], pred["mean"]).all()
        assert np.array_equal(unc["vote"], pred["vote"]) and np.array_equal(rep["vote"], pred["vote"])
        np.testing.assert_allclose(pred["vote"].sum(axis=1), 1.0, rtol=1e-12)
        assert np.array_equal(rep["confusion_sum"], rep["sample_confusion"].astype(np.int64).sum(axis=0))
    pd = out["partial_dependence"]
    np.testing.assert_allclose(pd["pd_mean"], pd["ice_mean"].mean(axis=0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(pd["range_mean"], pd["sample_range"].astype(np.float64).mean(axis=0), rtol=1e-12, atol=0)
    for name in ("coalition_values", "sensitivity_sample_abs"):
        r = out[name]
        np.testing.assert_allclose(r["abs_mean"], r["sample_abs"].astype(np.float64).mean(axis=0), rtol=1e-6, atol=0)    # fp32 a_s


@pytest.mark.parametrize("net,U", CASES, ids=[f"{n}-U{u}" for n, u in CASES])
def test_second_list_equals_the_parent_commit(net, U):
    pt, train = handle(net)
    out = run_calls2(pt, net, U)
    assert_recorded(golden(GOLDEN_FILE2), net, U, train, out)
    check_references2(net, U, out)


@pytest.mark.parametrize("net,U", CASES, ids=[f"{n}-U{u}" for n, u in CASES])
def test_second_list_in_five_blocks_of_rows_equals_the_parent_commit(net, U, monkeypatch):
    pt, train = handle(net)
    assert_recorded(golden(GOLDEN_FILE2), net, U, train, run_calls2(pt, net, U, setenv=monkeypatch.setenv))


def check_references3(net, U, train, out):
    """One headline output per call of the third list against the float64 reference of that call's own GPU test, at its tolerance
    (test_gpu_fscore.py: _check_against_ref on the device's own means and samples; test_gpu_mbar.py: _reference on the device's own
    N_k and sweep count, f within TOL; the U of the vectors as test_gpu_evidence.py holds them)."""
    task, topo = NETS[net]
    w, eta, mult = samples(net, U)
    at = np.cumsum(mult) - mult                                              # the first occurrence of every distinct vector
    if task == REG:
        off = out["fscore_noise_off"]
        assert off["n_samples"] == int(mult.sum()) and off["n_trajectories"] == U
        assert np.array_equal(off["samples"], off["means"])
        one_each = dict(off, samples=off["samples"][at], means=off["means"][at])
        fscore_check_against_ref(one_each, eta, truth_of(U), mult, f"{net} U={U} noise off", levels=QUANTILES)
    u, b, u_prior, b_prior = host_u_of(U)
    mult2 = mult.reshape(2, U // 2)
    hu = out["mbar_host_u"]
    r = mbar_reference(dict(betas=np.asarray(BETAS), u=u, b=b, multiplicity=mult2, u_prior=u_prior, b_prior=b_prior), hu, 1.0)
    mv = out["mbar_vectors"]
    assert mv["n_items"] == 2 * U and mv["n_distinct"] == U
    np.testing.assert_allclose(mv["u"][U:], evidence_ref.u_and_b_batched(task, train, w, topo)[0], rtol=1e-5, atol=1e-4)
    rv = mbar_reference(dict(betas=np.asarray(BETAS), u=mv["u"][U:].reshape(2, -1), b=mv["b"][U:].reshape(2, -1), multiplicity=mult2,
                             u_prior=mv["u"][:U], b_prior=mv["b"][:U]), mv, 1.0)
    dev = dict(host_u_f=mbar_dev(hu["f"], r["f"]), host_u_log_weight=mbar_dev(hu["log_weight"], r["lw"]),
               vectors_f=mbar_dev(mv["f"], rv["f"]), vectors_log_weight=mbar_dev(mv["log_weight"], rv["lw"]))
    print(f"{net} U={U} mbar: sweeps {hu['n_iter']} / {mv['n_iter']}, deviations " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= MBAR_TOL, (k, v)


@pytest.mark.parametrize("net,U", CASES, ids=[f"{n}-U{u}" for n, u in CASES])
def test_third_list_equals_the_parent_commit(net, U, monkeypatch):
    pt, train = handle(net)
    out = run_calls3(pt, net, U, monkeypatch.setenv, monkeypatch.delenv)
    assert_recorded(golden(GOLDEN_FILE3), net, U, train, recorded3(out, U))
    check_references3(net, U, train, out)
