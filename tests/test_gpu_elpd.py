"""Predictive accuracy on the GPU (ptnn_elpd / predictive_accuracy): lppd, WAIC and PSIS-LOO per data row from the sampled
chains, checked against the float64 oracle (tests/elpd_ref.py) on the device's own vectors and on its own pointwise
log-likelihood, and for bitwise agreement between sources and block sizes."""
import math
import warnings

import numpy as np
import pytest

import elpd_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
ATOL = 1e-4          # absolute floor of the oracle comparison: the device's fp32 forward pass vs the oracle's float64 one


def _pt(task, topo, train, test, R, S, tmp_path, *, lg=True, lr=0.1, maxtemp=2, si=10, burn_in=0.5, **kw):
    path = str(tmp_path)
    if task == orc.TASK_REG:
        from ptnn_amd.pt_timeseries_regression import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, 0.5, path, seed=SEED, write_files=False, **kw)
    else:
        from ptnn_amd.pt_classification import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, path, seed=SEED, write_files=False, **kw)
    pt.initialize_chains(burn_in)
    return pt


def _oracle_ll(task, rows, cols, topo, eta=None):
    """float64 pointwise log-likelihood [M, n_rows] of the weight vectors cols [P, M] on data rows [n_rows, n_in + 1]."""
    X, y = rows[:, :topo[0]], rows[:, topo[0]]
    out = np.stack([orc.forward(X, cols[:, j].astype(np.float64), topo)[1] for j in range(cols.shape[1])])
    if task == orc.TASK_CLS:
        e = np.exp(out)
        p = e / e.sum(axis=2, keepdims=True)
        return np.log(p[:, np.arange(X.shape[0]), y.astype(np.int64)])
    tau2 = np.exp(np.asarray(eta, np.float32).astype(np.float64))[:, None]
    d = y[None, :] - out[:, :, 0]
    return -0.5 * np.log(2 * math.pi * tau2) - 0.5 * d * d / tau2


def _runs(w, eta):
    """Maximal runs of bitwise-equal consecutive (w, eta) -> (distinct w, distinct eta, counts) (one chain's block at a time is
    not needed: a run never spans two chains unless their vectors are equal, which merges nothing the multiset does not)."""
    w32 = np.ascontiguousarray(w, np.float32)
    e32 = np.ascontiguousarray(eta, np.float32)
    new = np.ones(w32.shape[0], bool)
    new[1:] = np.any(w32[1:].view(np.uint32) != w32[:-1].view(np.uint32), axis=1) | (e32[1:].view(np.uint32) != e32[:-1].view(np.uint32))
    starts = np.flatnonzero(new)
    return w32[starts], e32[starts], np.diff(np.append(starts, w32.shape[0])).astype(np.int32)


def _same(a, b):
    for k in ("lppd_i", "elpd_loo_i", "p_waic_i", "khat"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.n_samples == b.n_samples


def _check_oracle(pa, ll_ref):
    r = ref.elpd_rows(ll_ref)
    np.testing.assert_allclose(pa.lppd_i, r["lppd"], rtol=1e-5, atol=ATOL)
    np.testing.assert_allclose(pa.elpd_loo_i, r["elpd_loo"], rtol=1e-5, atol=ATOL)
    ok = np.isfinite(r["khat"]) & (r["khat"] < 0.7)
    assert np.max(np.abs(pa.khat[ok] - r["khat"][ok]), initial=0.0) <= 1e-3
    # the reduction alone: the oracle on the device's own log-likelihood
    own = ref.elpd_rows(pa.log_lik)
    for k, d in (("lppd", pa.lppd_i), ("p_waic", pa.p_waic_i), ("elpd_loo", pa.elpd_loo_i)):
        np.testing.assert_allclose(d, own[k], rtol=1e-9, atol=1e-12, err_msg=k)
    fin = np.isfinite(own["khat"])
    assert np.array_equal(np.isfinite(pa.khat), fin)
    assert np.max(np.abs(pa.khat[fin] - own["khat"][fin]), initial=0.0) <= 1e-9
    t = ref.totals(own)
    assert pa.elpd_loo == pytest.approx(t["elpd_loo"], rel=1e-9) and pa.se_elpd_loo == pytest.approx(t["se_elpd_loo"], rel=1e-6)
    assert pa.elpd_waic == pytest.approx(t["elpd_waic"], rel=1e-9) and pa.p_loo == pytest.approx(t["p_loo"], rel=1e-6, abs=1e-9)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)                     # chain-major, as the columns of res[0]
    return pt, res, d, eta


def test_regression_sunspot(sunspot):
    pt, res, d, eta = sunspot
    for data in ("train", "test"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa = pt.predictive_accuracy(data, return_pointwise=True)
        assert pa.n_samples == 8 * 300 and pa.log_lik.shape == (2400, len(d["sunspot_" + data]))
        assert pa.n_distinct < pa.n_samples
        _check_oracle(pa, _oracle_ll(orc.TASK_REG, d["sunspot_" + data], res[0], (4, 5, 1), eta))
    # sum over the train rows = ptnn_evaluate's untempered loglik_train for the same (w, tau^2)
    pa = pt.predictive_accuracy("train", return_pointwise=True)
    for j in (0, 777, 2399):
        ev = pt._sampler.evaluate(res[0][:, j], np.exp(np.float32(eta[j])))[0]
        assert pa.log_lik[j].sum() == pytest.approx(float(ev[0]), rel=1e-5)


def test_classification_iris(tmp_path):
    d = parity.datasets()
    topo = (4, 12, 3)
    pt = _pt(orc.TASK_CLS, topo, d["iris_train"], d["iris_test"], 8, 400, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    for data in ("train", "test"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa = pt.predictive_accuracy(data, return_pointwise=True)
        _check_oracle(pa, _oracle_ll(orc.TASK_CLS, d["iris_" + data], res[0], topo))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _same(pt.predictive_accuracy(data, weights=res[0].T), pa)
    # host rows: the test set as it is, labels out of range refused
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same(pt.predictive_accuracy(pt.testdata), pt.predictive_accuracy("test"))
    bad = np.array(pt.testdata, dtype=np.float64)
    bad[3, 4] = 3.0
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="class label"):
        pt.predictive_accuracy(bad)


def test_wide_net_compact_traces(tmp_path):
    d = parity.datasets()
    R, S, topo = 4, 200, (32, 256, 1)
    pt = _pt(orc.TASK_REG, topo, d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, S // 2:].reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa = pt.predictive_accuracy("test", return_pointwise=True)
        _check_oracle(pa, _oracle_ll(orc.TASK_REG, d["synth32_test"], res[0], topo, eta))
        _same(pt.predictive_accuracy("test", weights=res[0].T, eta=eta), pa)


def test_sources_agree(sunspot, monkeypatch):
    pt, res, _, eta = sunspot
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_pa = pt.predictive_accuracy("train", return_pointwise=True)
        # host vectors, expanded and as distinct (w, eta) with multiplicities
        _same(pt.predictive_accuracy("train", weights=res[0].T, eta=eta), ref_pa)
        w, e, c = _runs(res[0].T, eta)
        alt = pt.predictive_accuracy("train", weights=(w, c), eta=e)
        _same(alt, ref_pa)
        assert alt.n_distinct == ref_pa.n_distinct
        # the device's own log-likelihood through source 3
        _same(pt.predictive_accuracy(loglik=ref_pa.log_lik), ref_pa)
        # blocks of rows: one row per block
        monkeypatch.setenv("PTNN_ELPD_SCRATCH_BYTES", "1")
        one = pt.predictive_accuracy("train", return_pointwise=True)
        _same(one, ref_pa)
        assert np.array_equal(one.log_lik, ref_pa.log_lik)
        monkeypatch.delenv("PTNN_ELPD_SCRATCH_BYTES")
    # the same w with a different eta is another sample
    e2 = eta.copy()
    e2[1::2] += np.float32(0.25)
    out = pt._sampler.elpd("train", w=res[0].T, eta=e2)
    assert out["n_distinct"] > ref_pa.n_distinct


@pytest.mark.parametrize("xi", [0.2, 0.9])
def test_known_answer_gpd(sunspot, xi):
    st = pytest.importorskip("scipy.stats")
    pt = sunspot[0]
    rng = np.random.default_rng(int(xi * 10))
    ratios = st.genpareto.rvs(xi, size=20000, random_state=rng)               # the draws of test_elpd_cpu.py
    ll = np.stack([-np.log(ratios), -np.log(ratios[::-1]), np.full(20000, -0.5)], axis=1)   # a reordered copy, a constant row
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pa = pt.predictive_accuracy(loglik=ll)
    r = ref.elpd_rows(ll)
    assert np.max(np.abs(pa.khat[:2] - r["khat"][:2])) <= 1e-9 and np.isinf(r["khat"][2])
    assert np.all(np.abs(pa.khat[:2] - xi) < 0.1) and pa.khat[0] == pa.khat[1]
    assert np.isinf(pa.khat[2]) and pa.lppd_i[2] == -0.5 and pa.p_waic_i[2] == 0.0
    assert pa.elpd_loo_i[2] == pytest.approx(-0.5, rel=1e-14)
    np.testing.assert_allclose(pa.elpd_loo_i, r["elpd_loo"], rtol=1e-9)
    np.testing.assert_allclose(pa.p_waic_i, r["p_waic"], rtol=1e-9)
    assert pa.good_k == 0.7
    high = [w for w in caught if "k-hat" in str(w.message)]
    assert (pa.n_high_k > 0) == (len(high) > 0)
    if xi == 0.9:
        assert pa.n_high_k == 2 and high


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                pa = pt.predictive_accuracy("test", weights=w)
            assert pa.n_samples == 800
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


def test_refusals(tmp_path):
    from ptnn_amd import _lib
    d = parity.datasets()
    tr, te = d["sunspot_train"], d["sunspot_test"]
    pt = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path)
    with pytest.raises(ValueError, match="run_chains"):
        pt.predictive_accuracy("test")
    res = pt.run_chains()
    with pytest.raises(ValueError, match="eta"):
        pt.predictive_accuracy("test", weights=res[0].T)
    # rows before a chain's first accepted step carry no eta: row 0 always is one
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt.predictive_accuracy("test", burn_in=0)
    # the PSIS tail outgrows the LDS: M = ceil(min(0.2 S, 3 sqrt(S / r_eff))) > 4096 (S = 40 000 through multiplicities)
    ll = np.full((4, 3), -1.0)
    with pytest.raises(_lib.PtnnError, match="thin="):
        pt.predictive_accuracy(loglik=(ll, np.full(4, 10000)), r_eff=1e-6)
    assert pt.predictive_accuracy(loglik=(ll, np.full(4, 10000))).n_samples == 40000     # r_eff = 1: M = 600
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ok = pt.predictive_accuracy("test")                                  # the handle is still usable
    assert ok.n_samples == 400
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        ls.predictive_accuracy("test")
    st = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, trace_capacity=64)
    st.run_chains()
    with pytest.raises(ValueError, match="trace_capacity"):
        st.predictive_accuracy("test")
