"""The Python front of case_influence (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its recording
stand-in for `_lib.Sampler`, taught the one call more: valid calls over every sample source and `of` kind, the arguments the
sampler receives, what comes back, every refusal and the order of the checks, and the object states (no handle, a sharded
ladder, label_swap, a streamed trace, an unfinished run).  The last test asserts that the cases here reach every `raise` of
influence.py."""
import ast
import inspect
import sys

import numpy as np
import pytest

import influence_ref as ref
import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, BAD_W, CLS_ROWS, ETA, MULT, REG_P, REG_ROWS, STATES, TRACE_FAULTS, W, WC, fill

from ptnn_amd import influence, parallel_tempering as pt_module  # noqa: E402

VALUES, LOGLIK = fill((8, 3), 21, -2, 2, np.float32), fill((8, 12), 10, -4, -1)


class InfluenceStandIn(front.StandIn):
    def influence(self, *args, **kw):
        self._log("influence", args, kw)
        if kw.get("values") is not None:
            n_a, n_b = kw["values"].shape[1], kw["loglik"].shape[1]
            m = kw.get("multiplicity")
            M = kw["values"].shape[0] if m is None else int(np.sum(m))
        else:
            n_a = self._n_rows(args[0]) * (self.O if kw["of"] == "prediction" else 1)
            n_b, M = self._n_rows(args[1]), self._count(kw)
        t_var = fill(n_a, 3, 0.5, 2)
        t_var[0] = 0.0                                                   # a constant target column: corr and deletion_z are nan
        return dict(cov=fill((n_a, n_b), 1, -1, 1), target_mean=fill(n_a, 2, -1, 1), target_var=t_var, case_mean=fill(n_b, 4, -3, -1),
                    case_var=fill(n_b, 5, 0.1, 1), n_samples=M, n_distinct=-(-M // 2))


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(InfluenceStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.case_influence(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).case_influence(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def _check(ci, n_a_shape, n_b, M, top=5):
    """The result against the stand-in's canned outputs, finished by the plain restatement."""
    n_a = int(np.prod(n_a_shape))
    cov = fill((n_a, n_b), 1, -1, 1).reshape(n_a_shape + (n_b,))
    t_var = fill(n_a, 3, 0.5, 2)
    t_var[0] = 0.0
    t_sd, c_sd = np.sqrt(t_var).reshape(n_a_shape), np.sqrt(fill(n_b, 5, 0.1, 1))
    assert np.array_equal(ci.cov, cov) and np.array_equal(ci.deletion_shift, 0.0 - cov)
    assert np.array_equal(ci.target_mean, fill(n_a, 2, -1, 1).reshape(n_a_shape)) and np.array_equal(ci.target_sd, t_sd)
    assert np.array_equal(ci.case_loglik_mean, fill(n_b, 4, -3, -1)) and np.array_equal(ci.case_loglik_var, fill(n_b, 5, 0.1, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = cov / (t_sd[..., None] * c_sd)
        z = (0.0 - cov) / t_sd[..., None]
    first = (0,) * len(n_a_shape)
    corr[first], z[first] = np.nan, np.nan
    assert np.array_equal(ci.corr, corr, equal_nan=True) and np.array_equal(ci.deletion_z, z, equal_nan=True)
    assert np.isnan(ci.corr[first]).all() and np.isfinite(ci.corr.reshape(n_a, n_b)[1:]).all()
    k = min(top, n_b)
    assert ci.top_cases.shape == n_a_shape + (k,) and np.array_equal(ci.top_cases, ref.top_cases(cov, top))
    assert np.array_equal(ci.top_shift, 0.0 - np.take_along_axis(cov, ci.top_cases, axis=-1))
    assert np.allclose(ci.case_importance, np.nanmean(np.abs(corr).reshape(n_a, n_b), axis=0), rtol=1e-14, atol=0)
    assert ci.n_samples == M and ci.n_distinct == -(-M // 2)


# ---- valid calls
TRACE = [("all", {}, dict(replicas=None, step0=10, nsteps=30, thin=1), 120),
         ("cold_thin", dict(chains="cold", thin=3), dict(replicas=[1], step0=10, nsteps=30, thin=3), 10),
         ("list_burn_in", dict(chains=[2, 0], burn_in=0.5, thin=2), dict(replicas=[2, 0], step0=20, nsteps=20, thin=2), 20),
         ("burn_in_zero", dict(burn_in=0), dict(replicas=None, step0=0, nsteps=40, thin=1), 160)]


@pytest.mark.parametrize("of", ["prediction", "loglik"])
@pytest.mark.parametrize("name, kw, source, M", TRACE, ids=[t[0] for t in TRACE])
def test_trace_sources(name, kw, source, M, of):
    pt, calls, ci = run("reg", of=of, **kw)
    (tag, fn, args, got), = calls
    assert (tag, fn, args) == ("self", "influence", ["test", "train"])
    assert got == front.enc(dict(source, of=of))
    n_x, n_b = len(pt.testdata), len(pt.traindata)
    _check(ci, (n_x, 1) if of == "prediction" else (n_x,), n_b, M)


@pytest.mark.parametrize("key, w, eta", [("reg", W, ETA), ("cls", WC, None)], ids=["reg", "cls"])
def test_weight_sources(key, w, eta):
    O = 1 if key == "reg" else 3
    for weights, M, mult in ((w, 6, None), (w.T, 6, None), ((w, MULT), 8, MULT)):
        for of in ("prediction", "loglik"):
            pt, calls, ci = run(key, "train", "test", of=of, weights=weights, eta=eta, top=2)
            (_, fn, args, got), = calls
            assert args == ["train", "test"]
            assert got == front.enc(dict(w=np.asarray(w), multiplicity=mult, eta=eta, of=of))
            n_x = len(pt.traindata)
            _check(ci, (n_x, O) if of == "prediction" else (n_x,), len(pt.testdata), M, top=2)


def test_rows_and_options():
    # rows with extra columns: x cut to n_in (prediction) or n_in + 1 (loglik), cases to n_in + 1, float32
    for key, rows in (("reg", REG_ROWS), ("cls", CLS_ROWS)):
        for of, cols in (("prediction", 4), ("loglik", 5)):
            pt, calls, ci = run(key, rows, rows[:7], of=of, chains="cold", top=100)
            assert calls[0][2] == front.enc([np.ascontiguousarray(rows[:, :cols], dtype=np.float32),
                                             np.ascontiguousarray(rows[:7, :5], dtype=np.float32)])
            assert ci.top_cases.shape[-1] == 7                           # top is clipped to the number of cases
    # host matrices: no rows, no samples; a pair carries the multiplicities
    pt, calls, ci = run("reg", values=VALUES, loglik=LOGLIK)
    (_, fn, args, got), = calls
    assert fn == "influence" and args == [] and got == front.enc(dict(values=VALUES, loglik=LOGLIK, multiplicity=None))
    _check(ci, (3,), 12, 8)
    mult = [1, 0, 2, 1, 1, 3, 0, 1]
    pt, calls, ci = run("cls", values=VALUES.astype(np.float64), loglik=(LOGLIK.tolist(), mult), of="loglik", top=1)
    assert calls[0][3] == front.enc(dict(values=VALUES, loglik=LOGLIK, multiplicity=mult))
    _check(ci, (3,), 12, 9, top=1)
    assert type(ci).__name__ in dir(pt_module) and pt_module.CaseInfluence is influence.CaseInfluence
    assert pt_module.influence_flagged is influence.influence_flagged
    doc = " ".join(pt_module.ParallelTemperingBase.case_influence.__doc__.split())
    assert "first-order" in doc and "exact only in the limit of small changes" in doc
    assert 'chains="cold" is the posterior\'s own figure' in doc and 'chains="all" pools the tempered rungs' in doc


# ---- refusals, and the order of the checks
INF_LL = LOGLIK.copy()
INF_LL[5, 2] = -np.inf
FAULTS = [
    ("of_unknown", (), dict(of="output"), "of = 'output' must be 'prediction' or 'loglik'"),
    ("top_zero", (), dict(top=0), "top = 0 must be an integer >= 1"), ("top_fraction", (), dict(top=2.5), "top = 2.5"),
    ("x_unknown_name", ("valid",), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_1d", (fill(4, 1),), {}, "x must be 2-D"), ("x_too_few_columns", (BAD_ROWS,), {}, "at least n_in = 4 columns"),
    ("x_without_target", (fill((5, 4), 1),), dict(of="loglik"), r"x must be 2-D with at least n_in \+ 1 = 5 columns"),
    ("cases_unknown_name", ("test", "valid"), {}, "cases must be 'train', 'test' or an array, not 'valid'"),
    ("cases_without_target", ("test", fill((5, 4), 1)), {}, r"cases must be 2-D with at least n_in \+ 1 = 5 columns"),
    *[(n, (), k, "weights must be" if "weights" in k else "chains") for n, k in BAD_W + TRACE_FAULTS],
    ("weights_without_eta", (), dict(weights=W), "a regression's weights need eta"),
    ("no_sample_trace", (), dict(burn_in=1.0), "holds 0 samples: a covariance needs at least 2"),
    ("one_sample", (), dict(weights=(W, [0, 1, 0, 0, 0, 0]), eta=ETA), "holds 1 samples: a covariance needs at least 2"),
    ("values_alone", (), dict(values=VALUES), "values= and loglik= come together"),
    ("loglik_alone", (), dict(loglik=LOGLIK), "values= and loglik= come together"),
    ("values_with_weights", (), dict(values=VALUES, loglik=LOGLIK, weights=W), "no weights= with them"),
    ("values_1d", (), dict(values=VALUES[:, 0], loglik=LOGLIK), r"values must be \[n_samples, n_a\] and loglik \[n_samples, n_cases\]"),
    ("values_other_length", (), dict(values=VALUES[:7], loglik=LOGLIK), r"got shapes \(7, 3\) and \(8, 12\)"),
    ("values_no_column", (), dict(values=VALUES[:, :0], loglik=LOGLIK), "values must be"),
    ("matrices_one_sample", (), dict(values=VALUES, loglik=(LOGLIK, [0, 0, 1, 0, 0, 0, 0, 0])), "holds 1 samples"),
    ("loglik_not_finite", (), dict(values=VALUES, loglik=INF_LL), r"loglik\[5, 2\] = -inf is not finite"),
    # pairs: the order of the checks
    ("of_unknown_and_top_zero", (), dict(of="output", top=0), "of = 'output'"),
    ("top_zero_and_x_unknown_name", ("valid",), dict(top=0), "top = 0"),
    ("x_unknown_name_and_cases_unknown_name", ("valid", "valid"), {}, "x must be"),
    ("cases_unknown_name_and_weights_1d", ("test", "valid"), dict(weights=fill(REG_P, 1)), "cases must be"),
    ("weights_1d_and_without_eta", (), dict(weights=fill(REG_P, 1)), "weights must be"),
    ("top_zero_and_values_alone", (), dict(top=0, values=VALUES), "top = 0"),
    ("values_with_weights_and_1d", (), dict(values=VALUES[:, 0], loglik=LOGLIK, weights=W), "no weights= with them"),
    ("matrices_one_sample_and_not_finite", (), dict(values=VALUES, loglik=(INF_LL, [0, 0, 1, 0, 0, 0, 0, 0])), "holds 1 samples"),
]


@pytest.mark.parametrize("name, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, args, kw, text):
    refused("reg", text, *args, **kw)


def test_a_classification_takes_no_eta():
    _, calls, ci = run("cls", weights=WC)
    assert len(calls) == 1 and ci.n_samples == 6


STATE_TEXT = {"none": "case_influence needs the chains' device handle", "sharded": "case_influence runs on one GPU",
              "label": "label_swap=True", "cap": "trace_capacity = 5 < NumSamples = 40", "unfinished": "no finished run_chains"}


@pytest.mark.parametrize("state", STATES)
def test_object_states(state):
    refused(f"reg_{state}", STATE_TEXT[state])
    # the handle comes first, before the arguments; the trace's state last, after the rows
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "of = 'output'", of="output")
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "cases must be", "test", "valid")
    if state in ("none", "sharded"):
        refused(f"reg_{state}", STATE_TEXT[state], weights=W, eta=ETA)
        refused(f"reg_{state}", STATE_TEXT[state], values=VALUES, loglik=LOGLIK)
    else:                                                               # weights= and the host matrices need no finished trace
        _, calls, ci = run(f"reg_{state}", weights=W, eta=ETA)
        assert len(calls) == 1 and ci.n_samples == 6
        _, calls, ci = run(f"reg_{state}", values=VALUES, loglik=LOGLIK)
        assert len(calls) == 1 and ci.n_samples == 8
    if state == "cap":
        refused("reg_cap_unfinished", STATE_TEXT["cap"])


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(influence)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) >= 8
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
        for _, args, kw, text in FAULTS:
            refused("reg", text, *args, **kw)
        with pytest.raises(ValueError, match="z = 0 must be > 0"):
            influence.influence_flagged(None, z=0)
    finally:
        sys.settrace(before)
    missed = {t for ln, t in sites.items() if ln not in hit}
    print(f"{len(sites)} raise sites in influence.py, {len(sites) - len(missed)} reached")
    assert missed == set()
