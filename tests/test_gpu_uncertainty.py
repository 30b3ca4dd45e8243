"""Predictive uncertainty on the GPU (ptnn_uncertainty / predictive_uncertainty), against tests/uncertainty_ref.py:
1. the reductions alone, on the device's own outputs (posterior_predictive(..., return_samples=True) of the same selection), at the
   seven classification shapes of tests/report_cases.py and the three compiled regression input widths;
2. against the float64 oracle's forward pass, inside the bounds that a forward pass within 1e-5 of the oracle leaves;
3. the edges of the new kernels (T = 256 threads); 4. one multiset, one result (trace, expanded vectors, (distinct, multiplicity),
   any block size); 5. a known answer; 6. nothing is disturbed.
Vectors go in through weights=, so only the trace cases need a sampling run.

Level 1, the bounds and where they come from.  p_mean, vote, pred_mean: bitwise posterior_predictive's.  sample_entropy: float32 of
the reference's float64 H, except where H lies within 4 * 2^-53 * K of a float32 rounding boundary (the two float64 values may
then round apart): there within one float32 ulp, for at most 1e-4 of the entries.  entropy_percentiles: np.percentile of the
returned sample_entropy, exactly.  aleatoric: 1e-14 * K absolute -- a term p log p is at most 0.37 in size, a double log within 3 ulp
and one product rounding leave each below 5e-16, K terms, the fixed-point quantum 2^-62 is negligible, margin 20 x.  epistemic_var:
rtol 1e-12 against the reference centred on the device's own pred_mean.  aleatoric_var: rtol 1e-13.  The largest deviation seen of
every quantity is printed (and recorded in DESIGN.md section 28)."""
import math
import time

import numpy as np
import pytest

import parity
import uncertainty_cases as cases
import uncertainty_ref as ref
from parity import orc
from test_gpu_elpd import _runs as _runs_eta
from test_gpu_predict import _pt, _runs

pytestmark = pytest.mark.gpu

CLS, REG = orc.TASK_CLS, orc.TASK_REG
PCTS = (0, 5, 50, 95, 100, 37.5)
T = 256                                 # UNC_THREADS of csrc/ptnn_dev_uncertainty.hpp
SEEN = {}                               # quantity -> the largest deviation seen, as a share of its bound


def _note(name, value, bound):
    SEEN[name] = max(SEEN.get(name, 0.0), float(value))
    print(f"{name}: {float(value):.3g} (bound {bound:.3g})")


def _check_sample_entropy(got, H, K):
    """got [S, N] float32 against the reference's float64 H: equal to float32(H), or -- where H lies within 4 * 2^-53 * K of the
    midpoint of two adjacent float32 values -- one float32 ulp off; -> the share of the entries that took the second path."""
    assert got.dtype == np.float32 and got.shape == H.shape
    want = H.astype(np.float32)
    off = np.flatnonzero(got.ravel() != want.ravel())
    for i in off:
        h, w, g = H.ravel()[i], want.ravel()[i], got.ravel()[i]
        lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
        mids = [(float(w) + float(lo)) / 2.0, (float(w) + float(hi)) / 2.0]
        assert min(abs(h - m) for m in mids) <= 4 * 2.0 ** -53 * K and g in (lo, hi), (i, h, w, g)
    share = off.size / max(1, got.size)
    assert share <= 1e-4
    return share


def _check_cls(u, pred, K, pcts=PCTS):
    """A classification result against the reference on the device's own expanded outputs pred.samples [S, N, K]."""
    r = ref.classification(pred.samples, vote=pred.vote)
    assert u.n_samples == pred.n_samples == pred.samples.shape[0] and u.n_distinct == pred.n_distinct
    assert np.array_equal(u.p_mean, pred.mean) and np.array_equal(u.vote, pred.vote)
    for name in ("total", "aleatoric", "epistemic", "confidence", "variation_ratio", "disagreement"):
        v = getattr(u, name)
        assert v.dtype == np.float64 and v.shape == (pred.mean.shape[0],) and np.isfinite(v).all(), name
    if u.sample_entropy is not None:
        _note("sample_entropy: share of entries near a float32 boundary", _check_sample_entropy(u.sample_entropy, r["H"], K), 1e-4)
        sm = u.sample_entropy.astype(np.float64)
        assert sorted(u.entropy_percentiles) == sorted(pcts)
        for q in pcts:
            assert np.array_equal(u.entropy_percentiles[q], np.percentile(sm, q, axis=0)), q
    _note("aleatoric - reference", np.max(np.abs(u.aleatoric - r["aleatoric"])), 1e-14 * K)
    assert np.max(np.abs(u.aleatoric - r["aleatoric"])) <= 1e-14 * K
    # the host side: float64 arithmetic on the device's p_mean, vote and aleatoric
    assert np.max(np.abs(u.total - np.minimum(ref.entropy(pred.mean), math.log(K)))) <= 1e-14 * K
    assert np.array_equal(u.epistemic, np.maximum(u.total - u.aleatoric, 0.0))
    assert np.array_equal(u.confidence, pred.mean.max(axis=1)) and np.array_equal(u.variation_ratio, r["variation_ratio"])
    assert np.array_equal(u.disagreement, r["disagreement"])
    assert u.pred_mean is None and u.epistemic_var is None and u.aleatoric_var is None
    return r


def _check_reg(u, pred, eta):
    """A regression result against the reference on the device's own expanded outputs pred.samples [S, N, O] and eta [S]."""
    assert u.n_samples == pred.n_samples == pred.samples.shape[0] == len(eta) and u.n_distinct == pred.n_distinct
    assert np.array_equal(u.pred_mean, pred.mean)
    r = ref.regression(pred.samples, eta, centre=u.pred_mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(r["epistemic_var"] > 0, np.abs(u.epistemic_var - r["epistemic_var"]) / r["epistemic_var"], np.abs(u.epistemic_var))
    _note("epistemic_var: relative deviation", rel.max(), 1e-12)
    _note("aleatoric_var: relative deviation", abs(u.aleatoric_var - r["aleatoric_var"]) / r["aleatoric_var"], 1e-13)
    np.testing.assert_allclose(u.epistemic_var, r["epistemic_var"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(u.aleatoric_var, r["aleatoric_var"], rtol=1e-13, atol=0)
    assert np.array_equal(u.total_var, u.epistemic_var + u.aleatoric_var) and np.array_equal(u.epistemic_share, u.epistemic_var / u.total_var)
    assert u.p_mean is None and u.total is None and u.sample_entropy is None and u.entropy_percentiles is None
    return r


def _make(task, topo, tmp_path, train, test):
    kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
    return _pt(task, topo, np.array(train), np.array(test), 4, 20, tmp_path, **kw)


# ---- 1 and 2: the case grids
@pytest.fixture(scope="module", params=cases.CLS_SHAPES, ids=cases.CLS_IDS)
def grid(request, tmp_path_factory):
    topo = request.param
    train, test, W, p = cases.report_cases.case(topo)
    pt = _make(CLS, topo, tmp_path_factory.mktemp("grid"), train, test)
    mult = cases.multiplicities(len(W))
    u = pt.predictive_uncertainty("test", percentiles=PCTS, weights=(W, mult), return_samples=True)
    pred = pt.posterior_predictive("test", percentiles=PCTS, weights=(W, mult), return_samples=True)
    return dict(topo=topo, pt=pt, test=test, W=W, mult=mult, p=p, u=u, pred=pred)


def test_reductions_at_every_classification_shape(grid):
    I, _, K = grid["topo"]
    u, pred, mult = grid["u"], grid["pred"], grid["mult"]
    assert u.n_samples == int(mult.sum()) and u.n_distinct == 65 and u.sample_entropy.shape == (u.n_samples, 53)
    _check_cls(u, pred, K)
    # the targets of "test" give the selective risk; the low-level call leaves out what is not asked for
    y = grid["test"][:, I].astype(np.int64)
    loss = (np.argmax(u.p_mean, axis=1) != y).astype(np.float64)
    assert sorted(u.selective) == sorted(["total", "epistemic", "aleatoric", "confidence", "variation_ratio"])
    assert u.selective["epistemic"]["risk"][-1] == loss.mean() and u.selective["total"]["e_aurc"] >= 0.0
    low = grid["pt"]._sampler.uncertainty("test", w=grid["W"], multiplicity=mult)
    assert np.array_equal(low["entropy_mean"], u.aleatoric) and np.array_equal(low["mean"], pred.mean) and np.array_equal(low["vote"], pred.vote)
    assert low["entropy_order_stats"] is None and low["sample_entropy"] is None and low["epistemic_var"] is None


def test_classification_against_the_oracle_forward_pass(grid):
    K = grid["topo"][2]
    u = grid["u"]
    o = ref.classification(np.repeat(grid["p"], grid["mult"], axis=0))   # the oracle's probabilities, expanded as the samples are
    bound = K * cases.MARGIN * (1.0 + abs(math.log(cases.P_MIN - cases.MARGIN)))
    for name, b in (("aleatoric", bound), ("total", bound), ("epistemic", 2 * bound)):
        dev = np.max(np.abs(getattr(u, name) - o[name]))
        print(f"{name} - oracle: {dev:.3g} (bound {b:.3g})")
        assert dev <= b, name
    assert (u.epistemic >= cases.MI_MIN - 2 * bound).all()


@pytest.fixture(scope="module", params=cases.REG_SHAPES, ids=cases.REG_IDS)
def reg_grid(request, tmp_path_factory):
    topo = request.param
    train, test, W, eta, f = cases.regression_case(topo)
    pt = _make(REG, topo, tmp_path_factory.mktemp("reg"), train, test)
    mult = cases.multiplicities(len(W))
    u = pt.predictive_uncertainty("test", weights=(W, mult), eta=eta)
    pred = pt.posterior_predictive("test", weights=(W, mult), return_samples=True)
    return dict(topo=topo, pt=pt, test=test, W=W, eta=eta, mult=mult, f=f, u=u, pred=pred)


def test_reductions_at_every_regression_shape(reg_grid):
    g = reg_grid
    u = g["u"]
    assert u.n_samples == int(g["mult"].sum()) and u.n_distinct == 65 and u.epistemic_var.shape == (53, 1)
    _check_reg(u, g["pred"], np.repeat(g["eta"], g["mult"]))
    I = g["topo"][0]
    loss = ((u.pred_mean - g["test"][:, I:I + 1]) ** 2).sum(axis=1)
    assert list(u.selective) == ["epistemic"] and abs(u.selective["epistemic"]["risk"][-1] - loss.mean()) <= 1e-15
    assert (u.epistemic_var > 0).all() and ((u.epistemic_share > 0) & (u.epistemic_share < 1)).all()


def test_regression_against_the_oracle_forward_pass(reg_grid):
    g = reg_grid
    o = ref.regression(np.repeat(g["f"], g["mult"], axis=0), np.repeat(g["eta"], g["mult"]))
    d = cases.MARGIN
    bound = 4 * d * o["sd"] + 4 * d * d
    dev = np.abs(g["u"].epistemic_var - o["epistemic_var"])
    print(f"epistemic_var - oracle: largest share of the bound {float((dev / bound).max()):.3g}")
    assert (dev <= bound).all()
    np.testing.assert_allclose(g["u"].aleatoric_var, o["aleatoric_var"], rtol=1e-13, atol=0)


# ---- 3: the edges of the new kernels
EDGE_TOPO = (4, 6, 3)


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    from test_gpu_analysis_shapes import _vectors
    train, test, _, _ = cases.report_cases.case(EDGE_TOPO)
    return _make(CLS, EDGE_TOPO, tmp_path_factory.mktemp("edge"), train, test), np.array(train), _vectors(EDGE_TOPO, 2 * T + 1, 31)


@pytest.mark.parametrize("N,U", [(1, T + 1), (63, 1), (64, T - 1), (65, 2 * T + 1), (130, T)])
def test_row_and_sample_counts_at_the_work_group_edges(edge, N, U):
    pt, train, W = edge
    rows = train[:N, :4]
    u = pt.predictive_uncertainty(rows, percentiles=PCTS, weights=W[:U], return_samples=True)
    pred = pt.posterior_predictive(rows, weights=W[:U], return_samples=True)
    assert u.n_distinct == U and u.selective is None
    _check_cls(u, pred, 3)


@pytest.mark.parametrize("topo", [(9, 5, 2), (6, 10, 18)], ids=["K2", "K18"])
def test_one_sample_past_the_work_group_at_two_and_eighteen_classes(topo, tmp_path):
    from test_gpu_analysis_shapes import _vectors
    train, test, _, _ = cases.report_cases.case(topo)
    pt = _make(CLS, topo, tmp_path, train, test)
    W = _vectors(topo, T + 1, 32)
    u = pt.predictive_uncertainty("test", percentiles=PCTS, weights=W, return_samples=True)
    _check_cls(u, pt.posterior_predictive("test", weights=W, return_samples=True), topo[2])


def test_saturating_vectors_and_the_zero_vector(edge):
    """A class probability is the softmax of K sigmoid outputs, so it lies in [1 / (1 + (K - 1) e), e / (e + K - 1)] and is never
    0 or 1 in fp32 whatever the weights.  What saturating vectors do give: sigmoid outputs of exactly 0 or 1, hence probabilities
    at those two ends and exact ties among the classes of a row."""
    pt, train, W = edge
    rows = train[:65, :4]
    Ws = np.vstack([W[:20] * 50, np.zeros((1, W.shape[1]), np.float32)])
    u = pt.predictive_uncertainty(rows, percentiles=PCTS, weights=Ws, return_samples=True)
    pred = pt.posterior_predictive(rows, weights=Ws, return_samples=True)
    lo, hi = np.float32(1 / (1 + 2 * math.e)), np.float32(math.e / (math.e + 2))
    top = np.sort(pred.samples, axis=2)
    assert (top[:20, :, -1] == top[:20, :, -2]).any() and (pred.samples[20] == pred.samples[20, 0, 0]).all()
    assert (np.abs(pred.samples[:20] - hi) <= 1e-6).any()                 # sigmoid outputs of exactly (1, 0, 0)
    assert pred.samples.min() >= lo - 1e-6 and pred.samples.max() <= hi + 1e-6
    assert np.isfinite(u.sample_entropy).all() and (u.sample_entropy > 0).all()
    _check_cls(u, pred, 3)
    zero = pt.predictive_uncertainty(rows, weights=Ws[20:])
    print(f"the zero vector: p = {pred.samples[20, 0]!r}, aleatoric - log 3 = {float(np.max(np.abs(zero.aleatoric - math.log(3)))):.3g}")
    assert np.max(np.abs(zero.aleatoric - math.log(3))) <= 1e-14 and (zero.epistemic <= 3e-14).all()


def test_one_vector_a_million_times(tmp_path):
    topo = (9, 5, 2)
    train, test, W, _ = cases.report_cases.case(topo)
    pt = _make(CLS, topo, tmp_path, train, test)
    many = pt.predictive_uncertainty("test", weights=(W[:1], [10 ** 6]), percentiles=PCTS)
    one = pt.predictive_uncertainty("test", weights=W[:1], percentiles=PCTS, return_samples=True)
    assert many.n_samples == 10 ** 6 and many.n_distinct == 1 and many.sample_entropy is None
    assert np.array_equal(many.aleatoric, one.aleatoric) and np.array_equal(many.p_mean, one.p_mean)
    assert (many.epistemic <= 1e-14 * 2).all() and (one.epistemic <= 1e-14 * 2).all()
    for q in PCTS:
        assert np.array_equal(many.entropy_percentiles[q], one.sample_entropy[0].astype(np.float64)), q
    assert (many.variation_ratio == 0).all() and (many.disagreement == 0).all()
    # a regression: one vector has no spread, exactly
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    pt = _make(REG, (4, 5, 1), tmp_path / "reg", train, test)
    many = pt.predictive_uncertainty("test", weights=(W[:1], [10 ** 6]), eta=eta[:1])
    assert many.n_samples == 10 ** 6 and (many.epistemic_var == 0.0).all() and (many.epistemic_share == 0.0).all()
    np.testing.assert_allclose(many.aleatoric_var, math.exp(float(eta[0])), rtol=1e-13, atol=0)
    two = pt.predictive_uncertainty("test", weights=(W[[0, 0]], [3, 5]), eta=eta[[0, 0]])      # equal vectors merge: still no spread
    assert two.n_distinct == 1 and (two.epistemic_var == 0.0).all() and two.aleatoric_var == many.aleatoric_var


def test_refusals_of_the_low_level_call(edge):
    from ptnn_amd import _lib
    pt, train, W = edge
    with pytest.raises(_lib.PtnnError, match="rank 3 outside"):
        pt._sampler.uncertainty(train[:5, :4], w=W[:3], ranks=[0, 3])
    spec = _lib._spec(_lib.UncertaintySpec)
    spec.thin, spec.nsteps, spec.x_source, spec.n_rows = 1, 1, _lib.PREDICT_X_TEST, 53
    var = np.zeros((53, 3))
    spec.epistemic_var = var.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    assert pt._sampler.lib.ptnn_uncertainty(pt._sampler.h, _lib.C.byref(spec)) == -1
    assert "a classification has no output variance" in pt._sampler.lib.ptnn_last_error().decode()
    train, test, Wr, eta, _ = cases.regression_case((4, 5, 1))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rg = _make(REG, (4, 5, 1), tmp, train, test)
        with pytest.raises(_lib.PtnnError, match="a regression's host vectors need eta"):
            rg._sampler.uncertainty("test", w=Wr[:3])
        spec = _lib._spec(_lib.UncertaintySpec)
        spec.thin, spec.nsteps, spec.x_source, spec.n_rows = 1, 1, _lib.PREDICT_X_TEST, 53
        ent = np.zeros(53)
        spec.entropy_mean = ent.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
        assert rg._sampler.lib.ptnn_uncertainty(rg._sampler.h, _lib.C.byref(spec)) == -1
        assert "a regression has no class probabilities" in rg._sampler.lib.ptnn_last_error().decode()


# ---- 4: one multiset, one result
CLS_FIELDS = ("p_mean", "vote", "total", "aleatoric", "epistemic", "confidence", "variation_ratio", "disagreement", "sample_entropy")
REG_FIELDS = ("pred_mean", "epistemic_var", "aleatoric_var", "total_var", "epistemic_share")


def _same(a, b):
    assert a.n_samples == b.n_samples
    for name in CLS_FIELDS + REG_FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), name
    assert (a.entropy_percentiles is None) == (b.entropy_percentiles is None)
    for q in a.entropy_percentiles or {}:
        assert np.array_equal(a.entropy_percentiles[q], b.entropy_percentiles[q]), q
    assert (a.selective is None) == (b.selective is None)
    for name in a.selective or {}:
        assert np.array_equal(a.selective[name]["risk"], b.selective[name]["risk"]), name


@pytest.fixture(scope="module")
def iris(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path_factory.mktemp("iris"), lg=True, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    return pt, res, d


def test_one_multiset_one_result_classification(iris, monkeypatch):
    pt, res, d = iris
    R, S = 8, 400
    kw = dict(percentiles=PCTS, return_samples=True)
    t0 = time.perf_counter()
    base = pt.predictive_uncertainty("test", **kw)
    t1 = time.perf_counter()
    pred = pt.posterior_predictive("test", return_samples=True)
    t2 = time.perf_counter()
    print(f"Iris, {base.n_samples} samples ({base.n_distinct} distinct) x {len(d['iris_test'])} rows: predictive_uncertainty "
          f"{(t1 - t0) * 1e3:.1f} ms, posterior_predictive {(t2 - t1) * 1e3:.1f} ms (first calls, samples returned)")
    assert base.n_samples == R * (S - S // 2) and base.n_distinct == pred.n_distinct < base.n_samples
    _check_cls(base, pred, 3)
    distinct, counts = _runs(res[0], R)
    _same(base, pt.predictive_uncertainty("test", weights=res[0].T, **kw))
    merged = pt.predictive_uncertainty("test", weights=(distinct, counts), **kw)
    _same(base, merged)
    assert merged.n_distinct == base.n_distinct
    n_rows, U = len(d["iris_test"]), base.n_distinct
    image = n_rows * (3 + 1) * 4 * U                                      # the forward image and the entropy image of all rows
    monkeypatch.setenv("PTNN_UNC_SCRATCH_BYTES", str(image // 3))
    for src in ({}, dict(weights=res[0].T), dict(weights=(distinct, counts))):
        _same(base, pt.predictive_uncertainty("test", **kw, **src))
    monkeypatch.setenv("PTNN_UNC_SCRATCH_BYTES", "1")                      # one row per block
    _same(base, pt.predictive_uncertainty("test", **kw))
    monkeypatch.delenv("PTNN_UNC_SCRATCH_BYTES")
    for sel in (dict(chains="cold"), dict(thin=3), dict(chains=[5, 1], burn_in=0.25)):
        u = pt.predictive_uncertainty("test", return_samples=True, **sel)
        pp = pt.posterior_predictive("test", return_samples=True, **sel)
        assert u.n_samples == pp.n_samples and u.n_distinct == pp.n_distinct, sel
        _check_cls(u, pp, 3, pcts=(5, 95))
    _check_cls(pt.predictive_uncertainty("train", **kw), pt.posterior_predictive("train", return_samples=True), 3)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d, pt._sampler.eta_trace()


def test_one_multiset_one_result_regression(sunspot, monkeypatch):
    pt, res, d, et = sunspot
    R, S = 8, 400
    eta = et[:, S // 2:].reshape(-1)                                     # chain-major, as the columns of res[0]
    base = pt.predictive_uncertainty("test")
    pred = pt.posterior_predictive("test", return_samples=True)
    assert base.n_samples == R * (S - S // 2) and base.n_distinct == pred.n_distinct < base.n_samples
    _check_reg(base, pred, eta)
    wd, ed, counts = _runs_eta(res[0].T, eta)
    _same(base, pt.predictive_uncertainty("test", weights=res[0].T, eta=eta))
    merged = pt.predictive_uncertainty("test", weights=(wd, counts), eta=ed)
    _same(base, merged)
    assert merged.n_distinct == base.n_distinct
    n_rows, U = len(d["sunspot_test"]), base.n_distinct
    monkeypatch.setenv("PTNN_UNC_SCRATCH_BYTES", str(n_rows * 4 * U // 3))
    for src in ({}, dict(weights=res[0].T, eta=eta), dict(weights=(wd, counts), eta=ed)):
        _same(base, pt.predictive_uncertainty("test", **src))
    monkeypatch.setenv("PTNN_UNC_SCRATCH_BYTES", "1")
    _same(base, pt.predictive_uncertainty("test"))
    monkeypatch.delenv("PTNN_UNC_SCRATCH_BYTES")
    cold = int(np.argmin(pt.temperatures))
    for sel, sel_eta in ((dict(chains="cold"), et[cold, S // 2:]), (dict(thin=3), et[:, S // 2::3].reshape(-1)),
                         (dict(chains=[5, 1], burn_in=0.25), et[[5, 1], S // 4:].reshape(-1))):
        u = pt.predictive_uncertainty("test", **sel)
        pp = pt.posterior_predictive("test", return_samples=True, **sel)
        assert u.n_samples == pp.n_samples and u.n_distinct == pp.n_distinct, sel
        _check_reg(u, pp, sel_eta)


# ---- 5: a known answer
def _h(*p):
    return -sum(v * math.log(v) for v in p)


def test_known_answer(edge):
    """Net A: class k answers to input k alone; net B: the same with the classes shifted by one.  On rows with one input well
    above 0 and the others well below, each net's sigmoid outputs are within 2e-3 of (1, 0, 0) in its own order.  A class
    probability is the softmax of those sigmoid outputs: a = e / (e + 2) = 0.576 for the net's class and b = 1 / (e + 2) = 0.212
    for the two others -- as sure as a net of this architecture gets (its entropy H(a, b, b) = 0.9755 is the smallest three
    classes admit; no weights bring a sample's entropy below 0.05).  So the known answers are those of the pairs (a, b, b) and
    (b, a, b): the two nets pooled have p_mean = ((a + b) / 2, (a + b) / 2, b) and the mutual information H(p_mean) - H(a, b, b)
    = 0.0874 nats; the votes split exactly."""
    pt, _, _ = edge
    from test_gpu_predict import _outputs
    I, H, K = EDGE_TOPO
    W1, W2a, W2b = np.zeros((I, H)), np.zeros((H, K)), np.zeros((H, K))
    for k in range(K):
        W1[k, k] = 6.0
        W2a[k], W2b[k] = -8.0, -8.0
        W2a[k, k], W2b[k, (k + 1) % K] = 8.0, 8.0
    a, b = (np.concatenate([W1.ravel(), W2.ravel(), np.zeros(H + K)]).astype(np.float32) for W2 in (W2a, W2b))
    X = np.random.default_rng(23).standard_normal((3000, I))
    high, low = X[:, :K] > 0.5, X[:, :K] < -0.5
    keep = (high.sum(axis=1) == 1) & (low.sum(axis=1) == K - 1)          # one input well above 0, the others well below
    X = X[keep][:130]
    assert len(X) == 130
    AB = np.stack([a, b])
    pa, pb = math.e / (math.e + 2), 1 / (math.e + 2)
    tol = 0.01
    alea, total_ab = _h(pa, pb, pb), _h((pa + pb) / 2, (pa + pb) / 2, pb)
    o = ref.classification(_outputs(CLS, X, AB.T.astype(np.float64), EDGE_TOPO))
    assert np.max(np.abs(o["aleatoric"] - alea)) <= tol / 2                # the oracle first: each net is as sure as it can be
    u = pt.predictive_uncertainty(X, weights=AB)
    assert np.max(np.abs(u.total - total_ab)) <= tol and np.max(np.abs(u.aleatoric - alea)) <= tol
    assert np.max(np.abs(u.epistemic - (total_ab - alea))) <= tol
    assert (u.variation_ratio == 0.5).all() and (u.disagreement == 0.5).all() and u.selective is None
    u = pt.predictive_uncertainty(X, weights=(AB, [3, 1]))
    total_31 = _h(0.75 * pa + 0.25 * pb, 0.25 * pa + 0.75 * pb, pb)
    assert np.max(np.abs(u.total - total_31)) <= tol and np.max(np.abs(u.epistemic - (total_31 - alea))) <= tol
    assert (u.variation_ratio == 0.25).all() and (u.disagreement == 1 - (0.75 ** 2 + 0.25 ** 2)).all()
    u = pt.predictive_uncertainty(X, weights=AB[:1])
    assert (u.epistemic <= 1e-14 * K).all() and np.max(np.abs(u.aleatoric - alea)) <= tol


# ---- 6: nothing is disturbed
@pytest.mark.parametrize("task", [CLS, REG], ids=["cls", "reg"])
def test_no_side_effects(task, tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        if task == CLS:
            pt = _pt(CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        else:
            pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(60, 100)["pos_w"].reshape(-1, pt.num_param)
            e = pt._sampler.trace_rows(60, 100)[:, :, 3].reshape(-1) if task == REG else None
            u = pt.predictive_uncertainty("test", weights=w, eta=e, return_samples=True)
            assert u.n_samples == 800
            low = pt._sampler.uncertainty("train", step0=100, nsteps=60, thin=2, ranks=[0, 239] if task == CLS else ())
            assert low["n_samples"] == 240
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
