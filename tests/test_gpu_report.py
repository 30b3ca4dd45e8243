"""The classification report on the GPU (ptnn_class_report / classification_report), against tests/report_ref.py:
1. the reductions alone, on the device's own outputs (posterior_predictive(..., return_samples=True) of the same selection): every
   integer and every fp32 metric bit for bit, at the seven shapes of tests/report_cases.py;
2. against the float64 oracle's forward pass, inside the bounds that a forward pass within 1e-5 of the oracle leaves;
3. the edges of the new kernels; 4. one multiset, one result (trace, expanded vectors, (distinct, multiplicity), any block size);
5. a known answer; 6. nothing is disturbed.
Vectors go in through weights=, so only the trace cases need a sampling run.

The integer behind an auc column is recovered as round(auc * 2 n_k (N - n_k)): exact while that product stays far below 2^23, which
holds everywhere but at the 16384-row case, where the fp32 value itself is compared.  auc=False drops macro_auc from the middle of
the summary columns, so its columns are compared with the others' by name."""
import warnings

import numpy as np
import pytest

import parity
import report_cases as cases
import report_ref as ref
from parity import orc
from test_gpu_predict import _pt, _runs

pytestmark = pytest.mark.gpu

CLS = orc.TASK_CLS
PCTS = (0, 5, 50, 95, 100, 37.5)


def _flat(d):
    """A dict by name -> [Q] in the device's column order."""
    return np.concatenate([np.atleast_1d(d[n]) for n in ref.SUMMARY + ref.PER_CLASS if n in d])


def _percentile(a, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # an undefined column is NaN in every sample
        return np.percentile(a, q, axis=0)


def _auc_integers(rep, y, K):
    """The Mann-Whitney integers behind the auc columns of sample_metrics -> [S, K] int64 (0 where undefined)."""
    N = y.size
    nk = np.bincount(y, minlength=K)
    first = rep.names.index("auc[0]")
    out = np.zeros((rep.sample_metrics.shape[0], K), np.int64)
    for k in range(K):
        if 0 < nk[k] < N:
            v = rep.sample_metrics[:, first + k].astype(np.float64) * (2 * nk[k] * (N - nk[k]))
            assert np.max(np.abs(v - np.rint(v))) < 1e-2
            out[:, k] = np.rint(v).astype(np.int64)
    return out


def _check_reduction(rep, pred, y, K, auc=True, pcts=PCTS):
    """A report against the reference on the device's own expanded outputs pred.samples [S, N, K]: integers exactly, metrics
    as the float64 value rounded to fp32, bands as np.percentile of the returned sample_metrics."""
    S = pred.samples.shape[0]
    r = ref.report(pred.samples, np.ones(S, np.int64), y, K, auc)
    assert rep.n_samples == S and rep.names == ref.names(K, auc)
    assert np.array_equal(rep.support, np.bincount(y, minlength=K))
    if rep.sample_confusion is not None:
        assert rep.sample_confusion.dtype == np.int32 and np.array_equal(rep.sample_confusion, r["conf"])
    assert np.array_equal(rep.confusion_mean, r["confusion_sum"] / float(S))
    if auc:
        defined = (rep.support > 0) & (rep.support < y.size)
        if 2 * int(rep.support.max()) * y.size < 1 << 20:
            assert np.array_equal(_auc_integers(rep, y, K)[:, defined], r["auc2"][:, defined])
    assert rep.sample_metrics.dtype == np.float32
    assert np.array_equal(rep.sample_metrics, r["sample_metrics"], equal_nan=True)          # no bit differs
    sm = rep.sample_metrics.astype(np.float64)
    for q in pcts:
        assert np.array_equal(_flat(rep.metric_percentiles[q]), _percentile(sm, q), equal_nan=True), q
    np.testing.assert_allclose(_flat(rep.metric_mean), sm.mean(axis=0), rtol=1e-12, atol=0)
    assert np.array_equal(rep.p_mean, pred.mean)
    assert np.array_equal(rep.p_correct, pred.vote[np.arange(y.size), y])
    assert np.array_equal(rep.confusion, ref.confusion(rep.p_mean, y, K))
    return r


def _make(topo, tmp_path, train, test):
    return _pt(CLS, topo, np.array(train), np.array(test), 4, 20, tmp_path, lr=0.01, maxtemp=10)


# ---- 1 and 2: the case grid
@pytest.fixture(scope="module", params=cases.SHAPES, ids=cases.IDS)
def grid(request, tmp_path_factory):
    topo = request.param
    train, test, W, p = cases.case(topo)
    pt = _make(topo, tmp_path_factory.mktemp("grid"), train, test)
    mult = np.random.default_rng(13).integers(0, 4, len(W)).astype(np.int32)
    mult[1], mult[0] = 0, max(mult[0], 1)
    rep = pt.classification_report("test", percentiles=PCTS, weights=(W, mult), return_samples=True)
    pred = pt.posterior_predictive("test", percentiles=PCTS, weights=(W, mult), return_samples=True)
    return dict(topo=topo, pt=pt, test=test, W=W, mult=mult, p=p, rep=rep, pred=pred)


def test_reduction_bitwise_at_every_shape(grid):
    I, _, K = grid["topo"]
    y = grid["test"][:, I].astype(np.int64)
    rep, pred, mult = grid["rep"], grid["pred"], grid["mult"]
    assert rep.n_samples == int(mult.sum()) and rep.n_distinct == pred.n_distinct
    _check_reduction(rep, pred, y, K)
    low = grid["pt"]._sampler.class_report("test", w=grid["W"], multiplicity=mult)
    assert np.array_equal(low["vote"], pred.vote) and np.array_equal(low["p_mean"], pred.mean)
    assert low["metric_order_stats"] is None and low["sample_confusion"] is None and low["confusion_sum"].dtype == np.int64


def test_against_the_oracle_forward_pass(grid):
    I, _, K = grid["topo"]
    y = grid["test"][:, I].astype(np.int64)
    rep, mult = grid["rep"], grid["mult"]
    p = np.repeat(grid["p"], mult, axis=0)                               # the oracle's probabilities, expanded as the samples are
    S = p.shape[0]
    sure = cases.top_two_margin(p) > cases.MARGIN                        # [S, N]
    assert 1.0 - sure.mean() <= cases.EXCLUDED_CAP
    for s in range(S):
        kept = ref.confusion(p[s][sure[s]], y[sure[s]], K)
        extra = rep.sample_confusion[s].astype(np.int64) - kept          # what the rows left out add, wherever their argmax fell
        assert (extra >= 0).all() and np.array_equal(extra.sum(axis=1), np.bincount(y[~sure[s]], minlength=K)), s
    # |auc_dev - auc_oracle| <= near / (n_k (N - n_k)), times 2 n_k (N - n_k): the integers differ by at most 2 per near pair
    near, pairs = cases.near_pairs(p, y, K)
    assert near.sum() / (S * pairs.sum()) <= cases.NEAR_CAP
    _, a2 = ref.integers(p, y, K)
    got = _auc_integers(rep, y, K)
    defined = pairs > 0
    assert (np.abs(got - a2)[:, defined] <= 2 * near[:, defined]).all()
    assert np.array_equal(np.isnan(rep.metric_mean["auc"]), ~defined)


# ---- 3: the edges of the new kernels
EDGE_TOPO = (4, 6, 3)


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    train, test, _, _ = cases.case(EDGE_TOPO)
    from test_gpu_analysis_shapes import _vectors
    return _make(EDGE_TOPO, tmp_path_factory.mktemp("edge"), train, test), np.array(train), _vectors(EDGE_TOPO, 257, 31)


@pytest.mark.parametrize("N,U", [(1, 65), (63, 1), (64, 63), (65, 257), (130, 65)])
def test_row_and_sample_counts_at_the_tile_edges(edge, N, U):
    pt, train, W = edge
    rows = train[:N, :5]
    rep = pt.classification_report(rows, percentiles=PCTS, weights=W[:U], return_samples=True)
    pred = pt.posterior_predictive(rows, weights=W[:U], return_samples=True)
    assert rep.n_distinct == U
    _check_reduction(rep, pred, rows[:, 4].astype(np.int64), 3)


def test_exact_ties_duplicated_rows_saturation_and_one_class(edge):
    pt, train, W = edge
    # every row twice, the copy with another label: a positive and a negative of every class share their score exactly
    rows = np.repeat(train[:40, :5], 2, axis=0)
    rows[1::2, 4] = (rows[1::2, 4] + 1) % 3
    y = rows[:, 4].astype(np.int64)
    rep = pt.classification_report(rows, weights=W[:33], return_samples=True, percentiles=PCTS)
    pred = pt.posterior_predictive(rows, weights=W[:33], return_samples=True)
    assert np.array_equal(pred.samples[:, 0::2], pred.samples[:, 1::2])
    _check_reduction(rep, pred, y, 3)
    # saturating vectors: exact ties among the class probabilities of a row, argmax takes the first; the zero vector gives every
    # row the same probabilities: all predictions class 0, every auc 0.5
    Ws = np.vstack([W[:20] * 50, np.zeros((1, W.shape[1]), np.float32)])
    rep = pt.classification_report(rows, weights=Ws, return_samples=True, percentiles=PCTS)
    pred = pt.posterior_predictive(rows, weights=Ws, return_samples=True)
    top = np.sort(pred.samples, axis=2)
    assert (top[:20, :, -1] == top[:20, :, -2]).any() and (pred.samples[20] == pred.samples[20, 0, 0]).all()
    _check_reduction(rep, pred, y, 3)
    auc0 = rep.names.index("auc[0]")
    assert (rep.sample_metrics[20, auc0:auc0 + 3] == 0.5).all() and rep.sample_metrics[20, rep.names.index("macro_auc")] == 0.5
    assert np.array_equal(rep.sample_confusion[20], np.stack([np.bincount(y, minlength=3), [0] * 3, [0] * 3], axis=1))
    # all rows of one class: accuracy is defined, no auc is
    one = np.array(train[:65, :5])
    one[:, 4] = 2.0
    rep = pt.classification_report(one, weights=W[:9], return_samples=True)
    pred = pt.posterior_predictive(one, weights=W[:9], return_samples=True)
    _check_reduction(rep, pred, one[:, 4].astype(np.int64), 3, pcts=(5, 95))
    assert np.isnan(rep.metric_mean["auc"]).all() and np.isnan(rep.metric_mean["macro_auc"]) and np.isnan(rep.metrics["auc"]).all()
    assert np.isnan(rep.metric_percentiles[95]["macro_auc"]) and np.isnan(rep.sample_metrics[:, auc0:]).all()
    assert 0.0 <= rep.metric_mean["accuracy"] <= 1.0 and rep.metric_mean["accuracy"] == rep.metric_mean["recall"][2]
    assert np.isnan(rep.metric_mean["recall"]).tolist() == [True, True, False] and rep.roc == {0: None, 1: None, 2: None}


def test_without_auc_the_other_columns_are_the_same(edge):
    pt, train, W = edge
    rows = train[:130, :5]
    full = pt.classification_report(rows, weights=W[:65], percentiles=PCTS, return_samples=True)
    part = pt.classification_report(rows, weights=W[:65], percentiles=PCTS, return_samples=True, auc=False)
    assert len(part.names) == 3 + 3 * 3 and len(full.names) == 4 + 4 * 3 and part.sample_metrics.shape == (65, 12)
    cols = [full.names.index(n) for n in part.names]
    assert np.array_equal(part.sample_metrics, full.sample_metrics[:, cols])
    assert np.array_equal(part.sample_confusion, full.sample_confusion) and np.array_equal(part.confusion_mean, full.confusion_mean)
    for d_part, d_full in [(part.metric_mean, full.metric_mean), (part.metrics, full.metrics)] + [(part.metric_percentiles[q],
                                                                                                full.metric_percentiles[q]) for q in PCTS]:
        assert sorted(d_part) == sorted(set(d_full) - {"auc", "macro_auc"})
        for n in d_part:
            assert np.array_equal(d_part[n], d_full[n]), n
    assert np.array_equal(part.p_mean, full.p_mean) and np.array_equal(part.p_correct, full.p_correct)


def test_one_vector_a_million_times(tmp_path):
    topo = (9, 5, 2)
    train, test, W, _ = cases.case(topo)
    pt = _make(topo, tmp_path, train, test)
    rep = pt.classification_report("test", weights=(W[:1], [10 ** 6]), percentiles=PCTS)
    one = pt.classification_report("test", weights=W[:1], percentiles=PCTS)
    assert rep.n_samples == 10 ** 6 and rep.n_distinct == 1 and rep.sample_metrics.shape == (10 ** 6, 12)
    assert (rep.sample_metrics == rep.sample_metrics[0]).all() and np.array_equal(rep.sample_metrics[0], one.sample_metrics[0])
    value = rep.sample_metrics[0].astype(np.float64)
    for q in PCTS:
        assert np.array_equal(_flat(rep.metric_percentiles[q]), value), q
    assert np.array_equal(_flat(rep.metric_mean), value) and np.array_equal(rep.confusion_mean, one.confusion_mean)
    assert np.array_equal(rep.p_mean, one.p_mean) and set(np.unique(rep.p_correct)) <= {0.0, 1.0}


def test_sixteen_thousand_rows_fill_the_lds_and_one_more_is_refused(tmp_path):
    from ptnn_amd import _lib
    topo, N = (9, 4, 2), 16384
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N + 1, 9)).astype(np.float32)
    X[N // 2:N] = X[:N // 2]                                             # every score twice: ties inside and across the classes
    y = (rng.uniform(size=N + 1) < 0.3).astype(np.float64)
    rows = np.hstack([X, y[:, None]]).astype(np.float32)
    from test_gpu_analysis_shapes import _vectors
    W = _vectors(topo, 3, 18)
    pt = _make(topo, tmp_path, rows[:150], rows[150:203])
    rep = pt.classification_report(rows[:N], weights=W, return_samples=True)
    pred = pt.posterior_predictive(rows[:N], weights=W, return_samples=True)
    r = _check_reduction(rep, pred, y[:N].astype(np.int64), 2, pcts=(5, 95))
    assert r["auc2"].min() > 1 << 24                                      # the counts need more than fp32's integers
    with pytest.raises(ValueError, match="auc=False has no cap"):
        pt.classification_report(rows, weights=W)
    with pytest.raises(_lib.PtnnError, match=r"auc: 16385 rows, at most 16384 .*auc=False\) has no cap"):
        pt._sampler.class_report(rows, w=W)
    more = pt.classification_report(rows, weights=W, auc=False, return_samples=True)
    pred = pt.posterior_predictive(rows, weights=W, return_samples=True)
    _check_reduction(more, pred, y.astype(np.int64), 2, auc=False, pcts=(5, 95))
    bad = rows[:70].copy()
    bad[66, 9] = 2.0
    with pytest.raises(_lib.PtnnError, match=r"class label 2 in row 66 is not an integer in \[0, 2\)"):
        pt._sampler.class_report(bad, w=W)
    with pytest.raises(_lib.PtnnError, match="rank 3 outside"):
        pt._sampler.class_report(rows[:70], w=W, ranks=[0, 3])


# ---- 4: one multiset, one result
def _same(a, b, samples=True):
    assert a.n_samples == b.n_samples and a.names == b.names
    for x, y in ((a.confusion, b.confusion), (a.p_mean, b.p_mean), (a.p_correct, b.p_correct), (a.confusion_mean, b.confusion_mean),
                 (_flat(a.metric_mean), _flat(b.metric_mean)), (_flat(a.metrics), _flat(b.metrics))):
        assert np.array_equal(x, y, equal_nan=True)
    for q in a.metric_percentiles:
        assert np.array_equal(_flat(a.metric_percentiles[q]), _flat(b.metric_percentiles[q]), equal_nan=True), q
    if samples:
        assert np.array_equal(a.sample_metrics, b.sample_metrics, equal_nan=True)
        assert np.array_equal(a.sample_confusion, b.sample_confusion)


@pytest.fixture(scope="module")
def iris(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path_factory.mktemp("iris"), lg=True, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    return pt, res, d


def test_one_multiset_one_result(iris, monkeypatch):
    pt, res, d = iris
    R, S = 8, 400
    base = pt.classification_report("test", percentiles=PCTS, return_samples=True)
    pred = pt.posterior_predictive("test", return_samples=True)
    y = d["iris_test"][:, 4].astype(np.int64)
    assert base.n_samples == R * (S - S // 2) and base.n_distinct == pred.n_distinct < base.n_samples
    _check_reduction(base, pred, y, 3)
    distinct, counts = _runs(res[0], R)
    expanded = pt.classification_report("test", percentiles=PCTS, weights=res[0].T, return_samples=True)
    merged = pt.classification_report("test", percentiles=PCTS, weights=(distinct, counts), return_samples=True)
    _same(base, expanded)
    _same(base, merged)
    assert merged.n_distinct == base.n_distinct
    # blocks of samples: the forward image of all rows no longer fits, so the pooled classifier comes from blocks of rows and the
    # rest from >= 3 blocks of samples
    n_rows, U = len(y), base.n_distinct
    monkeypatch.setenv("PTNN_REPORT_SCRATCH_BYTES", str(n_rows * 3 * 4 * (U // 3)))
    assert n_rows * 3 * 4 * U > n_rows * 3 * 4 * (U // 3) and -(-U // (U // 3)) >= 3
    for kw in ({}, dict(weights=res[0].T), dict(weights=(distinct, counts))):
        _same(base, pt.classification_report("test", percentiles=PCTS, return_samples=True, **kw))
    monkeypatch.setenv("PTNN_REPORT_SCRATCH_BYTES", "1")                   # one row, then one sample per block
    _same(base, pt.classification_report("test", percentiles=PCTS, return_samples=True, chains="all"))
    monkeypatch.delenv("PTNN_REPORT_SCRATCH_BYTES")
    for kw in (dict(chains="cold"), dict(thin=3), dict(chains=[5, 1], burn_in=0.25)):
        rep = pt.classification_report("test", **kw)
        pp = pt.posterior_predictive("test", return_samples=True, **kw)
        assert rep.n_samples == pp.n_samples and rep.n_distinct == pp.n_distinct, kw
        _check_reduction(rep, pp, y, 3, pcts=(5, 95))
    tr = pt.classification_report("train", percentiles=PCTS)
    _check_reduction(tr, pt.posterior_predictive("train", return_samples=True), d["iris_train"][:, 4].astype(np.int64), 3)


# ---- 5: a known answer
def test_known_answer(edge):
    pt, _, _ = edge
    from test_gpu_predict import _outputs
    I, H, K = EDGE_TOPO
    # a net whose class k answers to input k alone: hidden unit k follows x_k, output k follows hidden unit k against the others
    W1, W2 = np.zeros((I, H)), np.zeros((H, K))
    for k in range(K):
        W1[k, k] = 6.0
        W2[k] = -8.0
        W2[k, k] = 8.0
    w = np.concatenate([W1.ravel(), W2.ravel(), np.zeros(H + K)]).astype(np.float32)
    X = np.random.default_rng(23).standard_normal((3000, I))
    high, low = X[:, :K] > 0.5, X[:, :K] < -0.5
    keep = (high.sum(axis=1) == 1) & (low.sum(axis=1) == K - 1)          # one input well above 0, the others well below
    X, y = X[keep][:130], np.argmax(high[keep][:130], axis=1)
    assert len(y) == 130 and np.bincount(y, minlength=K).min() >= 20
    rows = np.hstack([X, y[:, None].astype(np.float64)])
    rng = np.random.default_rng(24)
    Wn = np.vstack([w[None], w[None] + (1e-3 * rng.standard_normal((30, w.size))).astype(np.float32)])
    p = _outputs(CLS, X, Wn.T.astype(np.float64), EDGE_TOPO)              # the oracle: every net puts its rows far apart
    for k in range(K):
        assert p[:, y == k, k].min() > 0.5 and p[:, y != k, k].max() < 0.3
    rep = pt.classification_report(rows, weights=Wn, return_samples=True)
    support = np.bincount(y, minlength=K)
    assert np.array_equal(rep.sample_confusion, np.broadcast_to(np.diag(support), (31, K, K)))
    assert np.array_equal(rep.confusion, np.diag(support)) and np.array_equal(rep.confusion_mean, np.diag(support).astype(np.float64))
    assert (rep.sample_metrics == 1.0).all() and (rep.p_correct == 1.0).all()
    for d in (rep.metrics, rep.metric_mean, rep.metric_percentiles[5], rep.metric_percentiles[95]):
        assert (_flat(d) == 1.0).all()


# ---- 6: nothing is disturbed
def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)
            rep = pt.classification_report("test", weights=w)
            assert rep.n_samples == 800
            assert pt._sampler.class_report("train", step0=50, nsteps=100, thin=2, ranks=[0, 399])["n_samples"] == 400
        res = pt.run_chains()
        outs.append((res, pt._sampler.traces(), pt._sampler.trace_rows(), pt._sampler.state(), pt._sampler.swap_stats()))
    (ra, ta, rwa, sa, wa), (rb, tb, rwb, sb, wb) = outs
    for x, y in zip(ra, rb):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    assert np.array_equal(rwa, rwb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert wa == wb
