"""Predictive uncertainty, host side (no GPU): the host helpers of uncertainty.py against brute force and the entropy identities,
the front on the drop-in classes of tests/test_analysis_front_cpu.py with a stand-in for `_lib.Sampler` that answers from
tests/uncertainty_ref.py (fields, bands, selective risk, every refusal and the order of adjacent checks), the binding, and the
conditions the GPU tests' case grid has to satisfy."""
import ast
import ctypes as C
import inspect
import math
import pickle
import sys

import numpy as np
import pytest

import test_analysis_front_cpu as front
import uncertainty_cases as cases
import uncertainty_ref as ref
from test_analysis_front_cpu import BAD_ROWS, CLS_ROWS, ETA, MANY_PCTS, MULT, REG_ROWS, W, WC, fill
from test_report_cpu import _softmax_outputs

from ptnn_amd import _lib, uncertainty, parallel_tempering as pt_module  # noqa: E402

PCTS = (0, 5, 50, 95, 100, 37.5)


# ---- the host helpers
def test_risk_coverage_against_brute_force_on_tied_and_untied_scores():
    rng = np.random.default_rng(3)
    for n, levels in ((1, 2), (7, 3), (40, 4), (200, 10 ** 6), (64, 1)):
        score = rng.integers(0, levels, n) / levels
        for loss in ((rng.uniform(size=n) < 0.3).astype(np.float64), rng.uniform(size=n) ** 2):
            got, want = uncertainty.risk_coverage(score, loss), ref.risk_coverage(score, loss)
            assert got["risk"].dtype == np.float64 and got["coverage"].tolist() == want["coverage"]
            np.testing.assert_allclose(got["risk"], want["risk"], rtol=1e-13, atol=0)
            for k in ("aurc", "aurc_optimal", "e_aurc"):
                assert abs(got[k] - want[k]) <= 1e-13, k
            assert got["e_aurc"] >= -1e-15 and got["risk"][-1] == pytest.approx(loss.mean(), rel=1e-13)
    # ties keep the row order: all scores equal, the curve follows the rows as given
    got = uncertainty.risk_coverage([0.5] * 4, [1, 0, 0, 1])
    assert got["risk"].tolist() == [1.0, 0.5, 1 / 3, 0.5] and got["coverage"].tolist() == [0.25, 0.5, 0.75, 1.0]
    assert got["aurc_optimal"] == (0 + 0 + 1 / 3 + 0.5) / 4
    with pytest.raises(ValueError, match="one score and one loss per row"):
        uncertainty.risk_coverage([0.1, 0.2], [1.0])
    with pytest.raises(ValueError, match="at least one row"):
        uncertainty.risk_coverage([], [])


def test_e_aurc_is_zero_when_the_score_is_the_loss():
    rng = np.random.default_rng(4)
    for loss in (rng.uniform(size=50), (rng.uniform(size=50) < 0.5).astype(np.float64)):
        got = uncertainty.risk_coverage(loss, loss)
        assert got["e_aurc"] == 0.0 and np.array_equal(got["risk"], np.cumsum(np.sort(loss)) / np.arange(1, 51))


def test_entropy_identities():
    for K in (2, 3, 10, 18):
        assert np.array_equal(uncertainty.entropy(np.eye(K)), np.zeros(K)) and np.array_equal(ref.entropy(np.eye(K)), np.zeros(K))
        assert not np.signbit(uncertainty.entropy(np.eye(K))).any()
        for f in (uncertainty.entropy, ref.entropy):
            assert abs(float(f(np.full(K, 1.0 / K))) - math.log(K)) <= 1e-14
    rng = np.random.default_rng(5)
    for S, N, K in ((1, 5, 3), (9, 20, 2), (30, 11, 18)):
        p = rng.dirichlet(np.full(K, 0.7), size=(S, N))
        p[0, 0] = np.eye(K)[0]                                           # an exact 0 among the probabilities
        r = ref.classification(p)
        assert np.max(np.abs((r["total"] - r["aleatoric"]) - ref.mean_kl(p))) <= 1e-12
        assert (r["total"] - r["aleatoric"] >= -1e-15).all() and np.max(np.abs(uncertainty.entropy(p) - r["H"])) <= 1e-14
        assert np.max(np.abs(uncertainty.entropy(p.mean(axis=0)) - r["total"])) <= 1e-14


# ---- the front, with a stand-in sampler that answers from the reference
class UncStandIn(front.StandIn):
    fx_override = None

    def uncertainty(self, *args, **kw):
        self._log("uncertainty", args, kw)
        rows = np.asarray(self.rows[args[0]] if isinstance(args[0], str) else args[0])
        I, O = self.I, self.O
        if kw.get("w") is not None:
            Wv = np.asarray(kw["w"])
            mult = np.ones(len(Wv), np.int64) if kw.get("multiplicity") is None else np.asarray(kw["multiplicity"])
            eta = kw.get("eta")
        else:
            M = self._count(kw)
            Wv, mult, eta = np.repeat(fill((-(-M // 2), self.P), 21, -1, 1), 2, axis=0)[:M], np.ones(M, np.int64), fill(M, 22, -6, -3)
        S = int(mult.sum())
        out = dict(mean=None, vote=None, entropy_mean=None, entropy_order_stats=None, sample_entropy=None, epistemic_var=None,
                   aleatoric_var=None, n_samples=S, n_distinct=len(Wv))
        if self.task == _lib.TASK_CLS:
            fx = _softmax_outputs(rows, Wv, I, O) if self.fx_override is None else self.fx_override
            p = np.repeat(fx.astype(np.float64), mult, axis=0)
            r = ref.classification(p)
            h32 = r["H"].astype(np.float32)
            self.last = dict(p=p, ref=r)
            out.update(mean=r["p_mean"], vote=r["vote"], entropy_mean=r["aleatoric"],
                       entropy_order_stats=np.sort(h32, axis=0)[list(kw["ranks"])] if len(kw["ranks"]) else None,
                       sample_entropy=h32 if kw["samples"] else None)
        else:
            z = np.einsum("ni,uio->uno", rows[:, :I].astype(np.float64), Wv[:, :I * O].reshape(-1, I, O).astype(np.float64))
            f = np.repeat((1.0 / (1.0 + np.exp(-z))).astype(np.float32).astype(np.float64), mult, axis=0)
            r = ref.regression(f, np.repeat(np.asarray(eta), mult))
            self.last = dict(f=f, ref=r)
            out.update(mean=r["pred_mean"], epistemic_var=r["epistemic_var"], aleatoric_var=r["aleatoric_var"])
        return out


def make(key, calls, fx=None):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(UncStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        s.rows = {"train": np.asarray(pt.traindata), "test": np.asarray(pt.testdata)}
        s.fx_override = fx
        pt._sampler = s
    return pt


def run(key, *args, fx=None, **kw):
    calls = []
    pt = make(key, calls, fx)
    return pt, calls, pt.predictive_uncertainty(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).predictive_uncertainty(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def _selective_matches(sel, scores, loss):
    assert sorted(sel) == sorted(scores)
    for name, score in scores.items():
        want = ref.risk_coverage(score, loss)
        np.testing.assert_allclose(sel[name]["risk"], want["risk"], rtol=1e-13, atol=0)
        assert abs(sel[name]["e_aurc"] - want["e_aurc"]) <= 1e-13 and sel[name]["coverage"].tolist() == want["coverage"]


def test_classification_front_against_the_reference():
    pt, calls, u = run("cls", "test", percentiles=PCTS, weights=(WC, MULT), return_samples=True)
    (_, fn, args, got), = calls
    spots, ranks = pt._band_ranks(8, list(PCTS))
    assert fn == "uncertainty" and args == ["test"]
    assert got == front.enc(dict(w=np.asarray(WC), multiplicity=MULT, eta=None, ranks=ranks, samples=True))
    r = pt._sampler.last["ref"]
    assert u.n_samples == 8 and u.n_distinct == 6
    for name in ("p_mean", "vote", "aleatoric", "confidence", "variation_ratio", "disagreement"):
        assert np.array_equal(getattr(u, name), r[name]), name
    assert np.max(np.abs(u.total - r["total"])) <= 1e-14 and np.max(np.abs(u.epistemic - r["epistemic"])) <= 1e-14
    assert (u.epistemic >= 0).all() and u.total.dtype == u.aleatoric.dtype == np.float64 and u.total.shape == (20,)
    assert u.sample_entropy.dtype == np.float32 and u.sample_entropy.shape == (8, 20)
    assert sorted(u.entropy_percentiles) == sorted(PCTS)
    for q in PCTS:                                                      # the bands are np.percentile of the expanded entropies
        assert np.array_equal(u.entropy_percentiles[q], np.percentile(u.sample_entropy.astype(np.float64), q, axis=0)), q
    for name in ("pred_mean", "epistemic_var", "aleatoric_var", "total_var", "epistemic_share"):
        assert getattr(u, name) is None, name
    y = np.asarray(pt.testdata)[:, 4].astype(np.int64)
    loss = (np.argmax(u.p_mean, axis=1) != y).astype(np.float64)
    _selective_matches(u.selective, dict(total=u.total, epistemic=u.epistemic, aleatoric=u.aleatoric, confidence=1 - u.confidence,
                                         variation_ratio=u.variation_ratio), loss)
    assert tuple(u.selective) == uncertainty.CLASSIFICATION_SCORES
    back = pickle.loads(pickle.dumps(u))                                # the tuple pickles
    assert type(back) is uncertainty.Uncertainty and np.array_equal(back.total, u.total)
    assert pt_module.Uncertainty is uncertainty.Uncertainty and pt_module.risk_coverage is uncertainty.risk_coverage
    assert pt_module.uncertainty_compare is uncertainty.uncertainty_compare
    mro = [k.__name__ for k in pt_module.ParallelTemperingBase.__mro__]
    assert "UncertaintyAnalysis" in mro and mro.index("UncertaintyAnalysis") == mro.index("ReportAnalysis") + 1
    assert "predictive_uncertainty" not in vars(front.analysis_class())


def test_trace_source_rows_without_targets_and_no_percentiles():
    pt, calls, u = run("cls", chains="cold", thin=3)
    (_, fn, args, got), = calls
    spots, ranks = pt._band_ranks(10, [5, 95])
    assert args == ["test"] and got == front.enc(dict(replicas=[1], step0=10, nsteps=30, thin=3, ranks=ranks, samples=False))
    assert u.n_samples == 10 and u.sample_entropy is None and sorted(u.entropy_percentiles) == [5, 95] and u.selective is not None
    # rows with extra columns: the device gets the n_in inputs as float32, the label is read from column n_in
    pt, calls, u = run("cls", CLS_ROWS, percentiles=())
    assert calls[0][2] == front.enc([np.ascontiguousarray(CLS_ROWS[:, :4], dtype=np.float32)])
    assert u.entropy_percentiles == {} and u.p_mean.shape == (12, 3) and dict(calls[0][3]["d"])["'ranks'"] == []
    assert u.selective["total"]["risk"].shape == (12,)
    # rows of exactly n_in columns carry no target
    pt, calls, u = run("cls", CLS_ROWS[:, :4])
    assert u.selective is None and u.total.shape == (12,)
    pt, calls, u = run("cls", np.full((3, 4), 0.25), percentiles=(50,), weights=WC[:1])
    assert u.n_samples == 1 and (u.epistemic == 0).all() and np.array_equal(u.total, u.aleatoric) and (u.variation_ratio == 0).all()


def test_regression_front_against_the_reference():
    pt, calls, u = run("reg", REG_ROWS, weights=(W, MULT), eta=ETA)
    (_, fn, args, got), = calls
    assert fn == "uncertainty" and args == front.enc([np.ascontiguousarray(REG_ROWS[:, :4], dtype=np.float32)])
    assert got == front.enc(dict(w=np.asarray(W), multiplicity=MULT, eta=ETA, ranks=(), samples=False))
    r = pt._sampler.last["ref"]
    assert np.array_equal(u.pred_mean, r["pred_mean"]) and np.array_equal(u.epistemic_var, r["epistemic_var"])
    assert isinstance(u.aleatoric_var, float) and u.aleatoric_var == r["aleatoric_var"] and u.pred_mean.shape == (12, 1)
    assert np.array_equal(u.total_var, r["total_var"]) and np.array_equal(u.epistemic_share, r["epistemic_share"])
    assert ((u.epistemic_share > 0) & (u.epistemic_share < 1)).all()
    for name in ("p_mean", "vote", "total", "aleatoric", "epistemic", "confidence", "variation_ratio", "disagreement",
                 "entropy_percentiles", "sample_entropy"):
        assert getattr(u, name) is None, name
    loss = ((u.pred_mean - REG_ROWS[:, 4:5]) ** 2).sum(axis=1)
    _selective_matches(u.selective, dict(epistemic=u.epistemic_var.sum(axis=1)), loss)
    assert tuple(u.selective) == uncertainty.REGRESSION_SCORES
    # the trace: no eta is passed on; "train" carries its targets; rows without a target column have no selective risk
    pt, calls, u = run("reg", "train", chains=[2, 0], burn_in=0.5, thin=2, return_samples=True)
    assert calls[0][3] == front.enc(dict(replicas=[2, 0], step0=20, nsteps=20, thin=2, ranks=(), samples=False))
    assert u.n_samples == 20 and u.selective["epistemic"]["risk"].shape == (30,)
    pt, calls, u = run("reg", REG_ROWS[:, :4], weights=W, eta=ETA)
    assert u.selective is None
    # two outputs: the targets are columns n_in and n_in + 1; one target column short of that is no target
    pt, calls, u = run("reg_twoout", REG_ROWS)
    assert u.pred_mean.shape == (12, 2) and u.epistemic_var.shape == (12, 2)
    loss = ((u.pred_mean - REG_ROWS[:, 4:6]) ** 2).sum(axis=1)
    _selective_matches(u.selective, dict(epistemic=u.epistemic_var.sum(axis=1)), loss)
    pt, calls, u = run("reg_twoout", REG_ROWS[:, :5])
    assert u.selective is None


def test_selective_risk_where_one_net_of_three_errs():
    """Net A puts 0.9 on the label of every row; net B agrees on the first 8 rows and puts 0.9 on the next class on the last 4.  B
    counts twice, so the pooled classifier errs exactly where the nets disagree: the epistemic score orders the rows as the loss
    does, the aleatoric one cannot tell them apart."""
    y = CLS_ROWS[:, 4].astype(np.int64)
    onto = lambda lab: np.where(np.arange(3)[None, :] == lab[:, None], 0.9, 0.05)
    shifted = np.where(np.arange(12) >= 8, (y + 1) % 3, y)
    fx = np.stack([onto(y), onto(shifted)]).astype(np.float32)
    pt, calls, u = run("cls", CLS_ROWS, fx=fx, weights=(WC[:2], [1, 2]))
    assert u.n_samples == 3
    loss = (np.argmax(u.p_mean, axis=1) != y).astype(np.float64)
    assert loss.tolist() == [0.0] * 8 + [1.0] * 4
    assert (u.epistemic[:8] <= 1e-14).all() and (u.epistemic[8:] > 0.3).all() and np.ptp(u.aleatoric) <= 1e-14
    sel = u.selective["epistemic"]
    assert sel["e_aurc"] == 0.0 and (sel["risk"][:8] == 0).all() and sel["risk"][-1] == 4 / 12
    assert sel["aurc"] == sel["aurc_optimal"] and u.selective["aleatoric"]["e_aurc"] >= 0.0
    assert np.array_equal(u.variation_ratio, np.where(np.arange(12) >= 8, 1 - 2 / 3, 0.0))
    assert np.allclose(u.disagreement[8:], 1 - (4 / 9 + 1 / 9), rtol=1e-12)


def test_uncertainty_compare():
    pt, calls, a = run("cls", "test", weights=WC)
    pt, calls, b = run("cls", "train", weights=WC)
    same = uncertainty.uncertainty_compare(a, a)
    assert sorted(same) == sorted(uncertainty.CLASSIFICATION_SCORES) and all(v == 0.5 for v in same.values())
    ab, ba = uncertainty.uncertainty_compare(a, b), uncertainty.uncertainty_compare(b, a)
    sa, sb = uncertainty.uncertainty_scores(a), uncertainty.uncertainty_scores(b)
    for name in ab:
        assert abs(ab[name] - ref.more_uncertain(sa[name], sb[name])) <= 1e-15 and abs(ab[name] + ba[name] - 1.0) <= 1e-15
    # rows every score calls more uncertain: probability 1
    far = a._replace(total=a.total + 10, epistemic=a.epistemic + 10, aleatoric=a.aleatoric + 10, confidence=a.confidence - 10,
                     variation_ratio=a.variation_ratio + 10)
    assert set(uncertainty.uncertainty_compare(a, far).values()) == {1.0}
    pt, calls, r = run("reg", REG_ROWS, weights=W, eta=ETA)
    assert uncertainty.uncertainty_compare(r, r) == {"epistemic": 0.5}
    assert uncertainty.uncertainty_compare(a, r) == {"epistemic": ref.more_uncertain(a.epistemic, r.epistemic_var.sum(axis=1))}


FAULTS = [
    ("no_handle", "cls_none", (), {}, "predictive_uncertainty needs the chains' device handle"),
    ("sharded", "cls_sharded", (), {}, "predictive_uncertainty runs on one GPU"),
    ("sharded_with_weights", "reg_sharded", (), dict(weights=W, eta=ETA), "predictive_uncertainty runs on one GPU"),
    ("data_unknown_name", "cls", ("valid",), {}, "data must be 'train', 'test' or an array, not 'valid'"),
    ("data_1d", "cls", (fill(5, 1),), {}, "data must be 2-D"),
    ("data_too_few_columns", "cls", (BAD_ROWS,), {}, r"at least n_in = 4 columns"),
    ("percentile_above_100", "cls", (), dict(percentiles=[5, 101]), "percentiles must lie in"),
    ("percentile_above_100_regression", "reg", (), dict(percentiles=[5, 101]), "percentiles must lie in"),
    ("label_too_large", "cls", (np.array([[0, 0, 0, 0, 1], [0, 0, 0, 0, 3.0]]),), {}, r"class label 3.0 in row 1 is not an integer in \[0, 3\)"),
    ("label_fraction", "cls", (np.array([[0, 0, 0, 0, 0.5], [0, 0, 0, 0, 3.0]]),), {}, "class label 0.5 in row 0"),
    ("label_negative", "cls", (np.array([[0, 0, 0, 0, -1.0]]),), {}, "class label -1.0 in row 0"),
    ("label_nan", "cls", (np.array([[0, 0, 0, 0, 2.0], [0, 0, 0, 0, np.nan]]),), {}, "class label nan in row 1"),
    ("weights_wrong_width", "cls", (), dict(weights=fill((6, 30), 1)), "weights must be"),
    ("weights_without_eta", "reg", (), dict(weights=W), "a regression's weights need eta"),
    ("chains_empty", "cls", (), dict(chains=[]), "chains"),
    ("label_swap", "cls_label", (), {}, "label_swap=True"),
    ("unfinished", "cls_unfinished", (), {}, "no finished run_chains"),
    ("no_sample", "cls", (), dict(burn_in=1.0), "holds no sample"),
    ("no_sample_regression", "reg", (), dict(weights=(W, [0] * 6), eta=ETA), "holds no sample"),
    ("too_many_percentiles", "cls", (), dict(percentiles=MANY_PCTS), "at most 16"),
    # pairs: the order of the checks -- handle, rows, percentiles, labels, sample source
    ("no_handle_and_bad_rows", "cls_none", ("valid",), {}, "needs the chains' device handle"),
    ("bad_rows_and_percentile", "cls", ("valid",), dict(percentiles=[101]), "data must be"),
    ("percentile_and_label", "cls", (np.array([[0, 0, 0, 0, 7.0]]),), dict(percentiles=[101]), "percentiles must lie in"),
    ("label_and_weights", "cls", (np.array([[0, 0, 0, 0, 7.0]]),), dict(weights=fill((6, 30), 1)), "class label 7.0 in row 0"),
    ("label_and_unfinished", "cls_unfinished", (np.array([[0, 0, 0, 0, 7.0]]),), {}, "class label 7.0 in row 0"),
    ("weights_and_too_many_percentiles", "cls", (), dict(weights=fill((6, 30), 1), percentiles=MANY_PCTS), "weights must be"),
]


@pytest.mark.parametrize("name, key, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, key, args, kw, text):
    refused(key, text, *args, **kw)


def test_a_regressions_target_is_no_label():
    pt, calls, u = run("reg", np.array([[0, 0, 0, 0, 7.5], [1, 0, 0, 0, -2.0]]), weights=W, eta=ETA)
    assert u.selective is not None and len(calls) == 1


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(uncertainty)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) == 2
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
        for _, key, args, kw, text in FAULTS:
            refused(key, text, *args, **kw)
        with pytest.raises(ValueError):
            uncertainty.risk_coverage([0.1, 0.2], [1.0])
    finally:
        sys.settrace(before)
    assert {t for ln, t in sites.items() if ln not in hit} == set()


# ---- the binding
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd.load_library()


def _spec(**kw):
    s = _lib.UncertaintySpec()
    s.struct_bytes = C.sizeof(_lib.UncertaintySpec)
    s.thin, s.nsteps, s.n_rows, s.x_source = 1, 10, 4, _lib.PREDICT_X_TRAIN
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_uncertainty(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device(lib):
    assert "ptnn_uncertainty" in _lib.SYMBOLS and lib.ptnn_uncertainty is not None
    assert lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4
    rc, msg = _err(lib, None)
    assert rc == -1 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc == -1 and f"expected {C.sizeof(_lib.UncertaintySpec)}" in msg
    rk = np.zeros(17, np.int64)
    rkp = rk.ctypes.data_as(C.POINTER(C.c_int64))
    one = np.zeros(4, np.float32)
    onep = one.ctypes.data_as(C.POINTER(C.c_float))
    for kw, word in ((dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(x_source=_lib.PREDICT_X_HOST), "needs x"),
                     (dict(n_rows=0), "n_rows"), (dict(n_ranks=17, ranks=rkp), "n_ranks = 17"), (dict(n_ranks=2), "ranks is NULL"),
                     (dict(nsteps=0), "no source"), (dict(w=onep, n_w=0), "n_w = 0"),
                     (dict(entropy_order_stats=onep), "order_stats requested without ranks")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # the order of adjacent checks: source, rows, n_rows, ranks
    for kw, word in ((dict(thin=0, x_source=7), "thin"), (dict(x_source=7, n_rows=0), "x_source"), (dict(n_rows=0, n_ranks=17, ranks=rkp), "n_rows")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # a consistent request reaches the handle check
    for kw in ({}, dict(n_ranks=16, ranks=rkp), dict(n_rows=65535 * 64 + 1), dict(w=onep, n_w=1, nsteps=0)):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and "null handle" in msg, (kw, msg)


# ---- the case grid of tests/test_gpu_uncertainty.py: what the oracle alone has to satisfy
@pytest.mark.parametrize("topo", cases.CLS_SHAPES, ids=cases.CLS_IDS)
def test_case_grid_conditions(topo):
    train, test, Wv, p = cases.report_cases.case(topo)
    K = topo[2]
    mult = cases.multiplicities(len(Wv))
    assert mult.min() == 0 and mult.max() == 3 and mult[1] == 0 and p.shape == (65, 53, K)
    mi_all = ref.classification(p)
    mi_sel = ref.classification(np.repeat(p, mult, axis=0))
    lo = min(float((r["total"] - r["aleatoric"]).min()) for r in (mi_all, mi_sel))
    print(f"{topo}: smallest oracle probability {p.min():.4f}; mutual information per row {lo:.3g} .. "
          f"{float((mi_all['total'] - mi_all['aleatoric']).max()):.3g}")
    assert p.min() >= cases.P_MIN
    assert lo >= cases.MI_MIN
    # the oracle-level bound of the GPU test stays well below the quantity it bounds
    bound = K * cases.MARGIN * (1 + abs(math.log(cases.P_MIN - cases.MARGIN)))
    assert bound < lo
