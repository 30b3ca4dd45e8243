"""The classification report, host side (no GPU): the float64 reference against hand-worked cases and against itself (the pair
count and the average ranks give one integer), the host helpers of report.py against the reference, the front on the drop-in
classification class of tests/test_analysis_front_cpu.py with a stand-in for `_lib.Sampler` that answers from the reference (bands,
NaN placement, every refusal, pickling), the binding, and the conditions the GPU tests' case grid has to satisfy."""
import ast
import ctypes as C
import inspect
import pickle
import sys

import numpy as np
import pytest

import report_cases as cases
import report_ref as ref
import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, CLS_ROWS, MANY_PCTS, WC, fill

from ptnn_amd import _lib, report, parallel_tempering as pt_module  # noqa: E402


# ---- the reference on hand-worked cases
def test_binary_auc_perfect_reversed_and_tied():
    y = np.array([0, 0, 1, 1, 1])
    pos = y == 1
    for s, want in (([0.1, 0.2, 0.7, 0.8, 0.9], 1.0), ([0.9, 0.8, 0.3, 0.2, 0.1], 0.0), ([0.5] * 5, 0.5)):
        s = np.array(s)
        a2 = ref.auc2_pairs(s, pos)
        assert a2 == ref.auc2_ranks(s, pos) == report.auc_pairs(s, pos)
        assert a2 / (2 * 3 * 2) == want
    # one tie between a positive and a negative among otherwise ordered scores: 5 wins and half a pair of 6
    s = np.array([0.1, 0.4, 0.4, 0.8, 0.9])
    assert ref.auc2_pairs(s, pos) == ref.auc2_ranks(s, pos) == 11
    fx = np.stack([1 - s, s], axis=1)[None]
    conf, a2 = ref.integers(fx, y, 2)
    assert conf[0].tolist() == [[2, 0], [1, 2]] and a2[0].tolist() == [11, 11]
    m = dict(zip(ref.names(2), ref.metrics(conf[0], a2[0])))
    assert m["accuracy"] == 4 / 5 and m["recall[1]"] == 2 / 3 and m["precision[0]"] == 2 / 3 and m["f1[1]"] == 4 / 5
    assert m["balanced_accuracy"] == (1.0 + 2 / 3) / 2 and m["auc[0]"] == m["auc[1]"] == m["macro_auc"] == 11 / 12


def test_three_classes_with_a_never_predicted_class():
    conf = np.array([[3, 1, 0], [1, 2, 0], [1, 1, 0]])                   # class 2 is never predicted: precision 0, recall 0, f1 0
    m = dict(zip(ref.names(3, auc=False), ref.metrics(conf)))
    assert m["precision[2]"] == 0.0 and m["recall[2]"] == 0.0 and m["f1[2]"] == 0.0
    assert m["accuracy"] == 5 / 9 and m["precision[0]"] == 3 / 5 and m["recall[0]"] == 3 / 4 and m["f1[0]"] == 6 / 9
    assert m["balanced_accuracy"] == (3 / 4 + 2 / 3 + 0.0) / 3
    assert m["macro_f1"] == (6 / 9 + 4 / 7 + 0.0) / 3
    assert len(m) == 3 + 3 * 3 and not np.isnan(list(m.values())).any()
    assert np.array_equal(report.scores_from_confusion(conf), ref.metrics(conf))


def test_an_absent_class_is_nan_and_left_out_of_the_macros():
    conf = np.array([[2, 1, 0], [0, 0, 0], [1, 0, 3]])                   # no row of class 1, which is predicted once
    a2 = np.array([14, 0, 20])
    m = dict(zip(ref.names(3), ref.metrics(conf, a2)))
    assert np.isnan([m["recall[1]"], m["f1[1]"], m["auc[1]"]]).all() and m["precision[1]"] == 0.0
    assert m["balanced_accuracy"] == (2 / 3 + 3 / 4) / 2 and m["macro_f1"] == (4 / 6 + 6 / 7) / 2
    assert m["auc[0]"] == 14 / (2 * 3 * 4) and m["auc[2]"] == 20 / (2 * 4 * 3) and m["macro_auc"] == (14 / 24 + 20 / 24) / 2
    got = report.scores_from_confusion(conf, a2)
    assert np.array_equal(got, ref.metrics(conf, a2), equal_nan=True)
    # all rows of one class: accuracy is defined, no auc is
    one = np.array([[4, 1], [0, 0]])
    m = dict(zip(ref.names(2), ref.metrics(one, np.array([0, 0]))))
    assert m["accuracy"] == 4 / 5 and m["balanced_accuracy"] == 4 / 5 and np.isnan([m["auc[0]"], m["auc[1]"], m["macro_auc"]]).all()
    assert report._undefined([5, 0], 5, True).tolist() == [False, False, False, True, False, False, False, True, False, True, True, True]


def test_pair_count_equals_average_ranks_as_integers():
    rng = np.random.default_rng(5)
    for n, levels in ((1, 2), (2, 2), (17, 3), (200, 8), (333, 1000), (64, 1)):
        s = rng.integers(0, levels, n).astype(np.float32) / np.float32(levels)
        for share in (0.0, 0.3, 1.0):
            pos = rng.uniform(size=n) < share
            a = ref.auc2_pairs(s, pos)
            assert a == ref.auc2_ranks(s, pos) == report.auc_pairs(s, pos)
            assert a + ref.auc2_pairs(s, ~pos) == 2 * int(pos.sum()) * int((~pos).sum())      # every pair counts 2 in all


def test_roc_area_equals_the_pair_count():
    rng = np.random.default_rng(6)
    for n, levels in ((9, 3), (120, 10), (250, 100000)):
        s = rng.integers(0, levels, n) / levels
        pos = rng.uniform(size=n) < 0.4
        fpr, tpr, thr = report.roc_curve(s, pos)
        assert fpr[0] == tpr[0] == 0.0 and thr[0] == np.inf and fpr[-1] == tpr[-1] == 1.0
        assert np.array_equal(thr[1:], np.unique(s)[::-1]) and np.all(np.diff(fpr) >= 0) and np.all(np.diff(tpr) >= 0)
        area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))
        assert abs(area - report.auc_pairs(s, pos) / (2 * int(pos.sum()) * int((~pos).sum()))) <= 1e-12
    assert report.roc_curve(np.array([0.2, 0.3]), np.array([True, True])) is None
    assert report.roc_curve(np.array([0.2, 0.3]), np.array([False, False])) is None
    y = np.array([0, 2, 2, 1])
    assert report.confusion_matrix(y, [0, 2, 1, 1], 3).tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 1]]
    assert report.report_names(2) == ref.names(2) and report.report_names(3, auc=False) == ref.names(3, auc=False)
    assert len(report.report_names(18)) == 4 + 4 * 18 and len(report.report_names(18, auc=False)) == 3 + 3 * 18


# ---- the front, with a stand-in sampler that answers from the reference
def _softmax_outputs(rows, W, I, K):
    """A stand-in forward pass: the softmax of a linear map made of every vector's first I K entries -> [U, N, K] float32."""
    z = np.einsum("ni,uik->unk", rows[:, :I].astype(np.float64), W[:, :I * K].reshape(-1, I, K).astype(np.float64) * 4)
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


class ReportStandIn(front.StandIn):
    def class_report(self, *args, **kw):
        self._log("class_report", args, kw)
        rows = np.asarray(self.rows[args[0]] if isinstance(args[0], str) else args[0])
        I, K, auc = self.I, self.O, kw["auc"]
        if kw.get("w") is not None:
            W = np.asarray(kw["w"])
            mult = np.ones(len(W), np.int64) if kw.get("multiplicity") is None else np.asarray(kw["multiplicity"])
        else:
            M = self._count(kw)
            W, mult = np.repeat(fill((-(-M // 2), self.P), 21, -1, 1), 2, axis=0)[:M], np.ones(M, np.int64)
        fx = _softmax_outputs(rows, W, I, K)
        y = rows[:, I].astype(np.int64)
        r = ref.report(fx, mult, y, K, auc)
        sm = np.nan_to_num(r["sample_metrics"], nan=0.0)                    # the device writes 0 where a column is undefined
        S = int(mult.sum())
        votes = np.stack([(np.repeat(np.argmax(fx, axis=2), mult, axis=0) == k).sum(axis=0) for k in range(K)], axis=1) / S
        self.last = dict(fx=fx, mult=mult, y=y, ref=r)
        return dict(p_mean=np.repeat(fx.astype(np.float64), mult, axis=0).mean(axis=0), vote=votes, p_correct=votes[np.arange(len(y)), y],
                    metric_mean=sm.astype(np.float64).mean(axis=0),
                    metric_order_stats=np.sort(sm, axis=0)[list(kw["ranks"])] if len(kw["ranks"]) else None,
                    confusion_sum=r["confusion_sum"], sample_metrics=sm.copy(),
                    sample_confusion=r["sample_confusion"] if kw["sample_confusion"] else None, n_samples=S, n_distinct=len(W))


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(ReportStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        s.rows = {"train": np.asarray(pt.traindata), "test": np.asarray(pt.testdata)}
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.classification_report(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).classification_report(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


PCTS = (0, 5, 50, 95, 100, 37.5)


@pytest.mark.parametrize("auc", [True, False])
def test_front_against_the_reference(auc):
    pt, calls, rep = run("cls", "test", percentiles=PCTS, auc=auc, weights=(WC, [1, 2, 0, 3, 1, 1]), return_samples=True)
    (_, fn, args, got), = calls
    spots, ranks = pt._band_ranks(8, list(PCTS))
    assert fn == "class_report" and args == ["test"]
    assert got == front.enc(dict(w=np.asarray(WC), multiplicity=[1, 2, 0, 3, 1, 1], ranks=ranks, auc=auc, sample_confusion=True))
    last = pt._sampler.last
    r, y, K = last["ref"], last["y"], 3
    Q = 4 + 4 * K if auc else 3 + 3 * K
    assert rep.names == ref.names(K, auc) and len(rep.names) == Q and rep.n_samples == 8 and rep.n_distinct == 6
    assert rep.support.tolist() == np.bincount(y, minlength=K).tolist() and rep.support.dtype == np.int64
    assert rep.sample_metrics.shape == (8, Q) and np.array_equal(rep.sample_metrics, r["sample_metrics"], equal_nan=True)
    assert np.array_equal(rep.sample_confusion, r["sample_confusion"])
    assert np.array_equal(rep.confusion_mean, r["confusion_sum"] / 8.0)
    expanded = rep.sample_metrics.astype(np.float64)
    flat = lambda d: np.concatenate([np.atleast_1d(d[n]) for n in ("accuracy", "balanced_accuracy", "macro_f1", "macro_auc", "precision",
                                                                   "recall", "f1", "auc") if n in d])
    assert sorted(rep.metric_percentiles) == sorted(PCTS)
    for q in PCTS:                                                      # the bands are np.percentile of the expanded metrics
        assert np.array_equal(flat(rep.metric_percentiles[q]), np.percentile(expanded, q, axis=0)), q
    np.testing.assert_allclose(flat(rep.metric_mean), expanded.mean(axis=0), rtol=1e-12)
    assert ("auc" in rep.metrics) == auc and ("macro_auc" in rep.metric_mean) == auc
    assert isinstance(rep.metrics["accuracy"], float) and rep.metrics["recall"].shape == (K,)
    # the pooled classifier: host arithmetic on p_mean
    pm = rep.p_mean
    conf = ref.confusion(pm, y, K)
    assert np.array_equal(rep.confusion, conf) and rep.confusion.dtype == np.int64
    a2 = [ref.auc2_pairs(pm[:, k], y == k) for k in range(K)] if auc else None
    assert np.array_equal(flat(rep.metrics), ref.metrics(conf, a2), equal_nan=True)
    for k in range(K):
        fpr, tpr, thr = rep.roc[k]
        assert np.array_equal(thr[1:], np.unique(pm[:, k])[::-1])
        if auc:
            assert abs(float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2)) - rep.metrics["auc"][k]) <= 1e-12
    right = np.repeat(np.argmax(last["fx"], axis=2) == y[None, :], last["mult"], axis=0)
    assert np.array_equal(rep.p_correct, right.sum(axis=0) / 8)
    back = pickle.loads(pickle.dumps(rep))                             # the tuple pickles
    assert type(back) is report.ClassificationReport and back.names == rep.names and np.array_equal(back.confusion, rep.confusion)
    assert pt_module.ClassificationReport is report.ClassificationReport and pt_module.auc_pairs is report.auc_pairs
    assert "ReportAnalysis" in [k.__name__ for k in pt_module.ParallelTemperingBase.__mro__]


def test_trace_source_and_rows_argument():
    pt, calls, rep = run("cls", chains="cold", thin=3)
    (_, fn, args, got), = calls
    spots, ranks = pt._band_ranks(10, [5, 95])
    assert args == ["test"] and got == front.enc(dict(replicas=[1], step0=10, nsteps=30, thin=3, ranks=ranks, auc=True, sample_confusion=False))
    assert rep.n_samples == 10 and rep.sample_confusion is None and sorted(rep.metric_percentiles) == [5, 95]
    # rows with extra columns: cut to n_in + 1, float32
    pt, calls, rep = run("cls", CLS_ROWS, percentiles=())
    assert calls[0][2] == front.enc([np.ascontiguousarray(CLS_ROWS[:, :5], dtype=np.float32)])
    assert rep.metric_percentiles == {} and rep.p_mean.shape == (12, 3) and dict(calls[0][3]["d"])["'ranks'"] == []


def test_nan_placement_follows_the_support():
    rows = np.array(CLS_ROWS[:, :5])
    rows[:, 4] = np.where(np.arange(12) % 2, 2.0, 0.0)                   # no row of class 1
    pt, calls, rep = run("cls", rows, return_samples=True)
    assert rep.support.tolist() == [6, 0, 6]
    for d in (rep.metrics, rep.metric_mean, rep.metric_percentiles[5], rep.metric_percentiles[95]):
        for name in ("recall", "f1", "auc"):
            assert np.isnan(d[name]).tolist() == [False, True, False], name
        assert not np.isnan(d["precision"]).any()
        assert not np.isnan([d["accuracy"], d["balanced_accuracy"], d["macro_f1"], d["macro_auc"]]).any()
    und = np.isnan(rep.sample_metrics)
    assert und.all(axis=0).tolist() == [n in ("recall[1]", "f1[1]", "auc[1]") for n in rep.names] and (und.all(axis=0) == und.any(axis=0)).all()
    assert rep.roc[1] is None and rep.roc[0] is not None
    # the macros of the samples run over the two classes that have rows
    sm = rep.sample_metrics.astype(np.float64)
    col = {n: sm[:, k] for k, n in enumerate(rep.names)}
    np.testing.assert_allclose(col["balanced_accuracy"], (col["recall[0]"] + col["recall[2]"]) / 2, rtol=1e-6)
    # all rows of one class: no auc anywhere, accuracy defined
    rows[:, 4] = 1.0
    pt, calls, rep = run("cls", rows)
    assert np.isnan(rep.metrics["auc"]).all() and np.isnan(rep.metric_mean["macro_auc"]) and np.isnan(rep.metric_percentiles[5]["auc"]).all()
    assert rep.metric_mean["accuracy"] == rep.metric_mean["accuracy"] and rep.roc == {0: None, 1: None, 2: None}
    assert np.isnan(rep.metric_mean["recall"]).tolist() == [True, False, True]


BIG = np.zeros((_lib.REPORT_MAX_AUC_ROWS + 1, 5), np.float32)
FAULTS = [
    ("data_unknown_name", "cls", ("valid",), {}, "data must be 'train', 'test' or an array, not 'valid'"),
    ("data_1d", "cls", (fill(5, 1),), {}, "data must be 2-D"),
    ("data_too_few_columns", "cls", (BAD_ROWS,), {}, r"at least n_in \+ 1 = 5 columns"),
    ("percentile_above_100", "cls", (), dict(percentiles=[5, 101]), "percentiles must lie in"),
    ("label_too_large", "cls", (np.array([[0, 0, 0, 0, 1], [0, 0, 0, 0, 3.0]]),), {}, r"class label 3.0 in row 1 is not an integer in \[0, 3\)"),
    ("label_fraction", "cls", (np.array([[0, 0, 0, 0, 0.5], [0, 0, 0, 0, 3.0]]),), {}, "class label 0.5 in row 0"),
    ("label_negative", "cls", (np.array([[0, 0, 0, 0, -1.0]]),), {}, "class label -1.0 in row 0"),
    ("label_nan", "cls", (np.array([[0, 0, 0, 0, 2.0], [0, 0, 0, 0, np.nan]]),), {}, "class label nan in row 1"),
    ("auc_row_cap", "cls", (BIG,), {}, "auc: 16385 rows, at most 16384 per call; auc=False has no cap"),
    ("weights_wrong_width", "cls", (), dict(weights=fill((6, 30), 1)), "weights must be"),
    ("chains_empty", "cls", (), dict(chains=[]), "chains"),
    ("no_sample", "cls", (), dict(burn_in=1.0), "holds no sample"),
    ("too_many_percentiles", "cls", (), dict(percentiles=MANY_PCTS), "at most 16"),
    ("regression", "reg", (), {}, "classification_report: a regression has no classes"),
    ("no_handle", "cls_none", (), {}, "classification_report needs the chains' device handle"),
    ("sharded", "cls_sharded", (), {}, "classification_report runs on one GPU"),
    ("sharded_with_weights", "cls_sharded", (), dict(weights=WC), "classification_report runs on one GPU"),
    ("unfinished", "cls_unfinished", (), {}, "no finished run_chains"),
    # pairs: the order of the checks
    ("regression_and_bad_rows", "reg", ("valid",), {}, "a regression has no classes"),
    ("bad_rows_and_percentile", "cls", ("valid",), dict(percentiles=[101]), "data must be"),
    ("percentile_and_label", "cls", (np.array([[0, 0, 0, 0, 7.0]]),), dict(percentiles=[101]), "percentiles must lie in"),
    ("label_and_row_cap", "cls", (np.vstack([BIG, [[0, 0, 0, 0, 9]]]),), {}, "class label 9.0 in row 16385"),
    ("row_cap_and_weights", "cls", (BIG,), dict(weights=fill((6, 30), 1)), "auc: 16385 rows"),
]


@pytest.mark.parametrize("name, key, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, key, args, kw, text):
    refused(key, text, *args, **kw)


def test_the_row_cap_holds_for_auc_only():
    big = np.array(BIG)
    big[::2, 4] = 1.0
    pt, calls, rep = run("cls", big, auc=False, weights=WC[:2], percentiles=())
    assert len(rep.names) == 12 and "auc" not in rep.metrics and rep.p_mean.shape == (16385, 3)


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(report)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) == 3
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
    s = _lib.ClassReportSpec()
    s.struct_bytes = C.sizeof(_lib.ClassReportSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source, s.auc = 1, 10, 4, _lib.PREDICT_X_TRAIN, 1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_class_report(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device(lib):
    assert "ptnn_class_report" in _lib.SYMBOLS and lib.ptnn_class_report is not None
    assert lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc < 0 and f"expected {C.sizeof(_lib.ClassReportSpec)}" in msg
    rk = np.zeros(17, np.int64)
    rkp = rk.ctypes.data_as(C.POINTER(C.c_int64))
    for kw, word in ((dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(x_source=_lib.PREDICT_X_HOST), "needs x"),
                     (dict(n_rows=0), "n_rows"), (dict(n_ranks=17, ranks=rkp), "n_ranks = 17"), (dict(n_ranks=2), "ranks is NULL"),
                     (dict(n_rows=16385), "auc=False"), (dict(n_rows=65535 * 64 + 1, auc=0), "65535 x 64")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # without auc the row cap does not apply; a consistent request reaches the handle check
    for kw in (dict(n_rows=16385, auc=0), dict(n_rows=16384), dict(n_ranks=16, ranks=rkp)):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and "null handle" in msg, (kw, msg)


# ---- the case grid of tests/test_gpu_report.py: what the oracle alone has to satisfy
@pytest.mark.parametrize("topo", cases.SHAPES, ids=cases.IDS)
def test_case_grid_conditions(topo):
    train, test, W, p = cases.case(topo)
    I, _, K = topo
    y = test[:, I].astype(np.int64)
    assert test.shape == (53, I + 1) and W.shape[0] == 65 and p.shape == (65, 53, K)
    excluded = float((cases.top_two_margin(p) <= cases.MARGIN).mean())
    near, pairs = cases.near_pairs(p, y, K)
    share = float(near.sum() / (65 * pairs.sum()))
    print(f"{topo}: excluded (sample, row) share {excluded:.3g}, near-tie pair share {share:.3g}, classes absent "
          f"{[k for k in range(K) if not (y == k).any()]}")
    assert excluded <= cases.EXCLUDED_CAP
    assert share <= cases.NEAR_CAP
    if topo in ((16, 12, 10), (6, 10, 18)):
        assert np.bincount(y, minlength=K).min() == 0                   # absent classes are wanted: undefined columns on the device
