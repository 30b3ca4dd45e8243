"""Calibration and proper scores on the GPU (ptnn_calibration / predictive_calibration): PIT, predictive mean and sd, quantiles
and the CRPS of the predictive mixture per data row, checked against the float64 oracle (tests/calibration_ref.py) on the
device's own network outputs and on the oracle's forward pass, for bitwise agreement between sources, block sizes and tilings,
against the existing analysis calls, and on a calibrated case with a known answer."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import calibration_ref as ref
import parity
from parity import orc
from test_gpu_elpd import ATOL, _pt, _runs

pytestmark = pytest.mark.gpu

REG_KEYS = ("pit", "crps_i", "pred_mean", "pred_sd")
QS = (0.025, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.975)       # symmetric pairs of the levels 0.95, 0.9, 0.8, 0.5


def _same(a, b):
    for k in REG_KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.quantiles.keys() == b.quantiles.keys()
    for p in a.quantiles:
        assert np.array_equal(a.quantiles[p], b.quantiles[p]), p
    assert a.n_samples == b.n_samples


def _check_reduction(cal, fx, eta, counts, y):
    """The reduction alone: the oracle on the device's own outputs fx [U, n_rows] (distinct samples with counts)."""
    r = ref.rows(fx, y, eta, counts)
    for k, d in (("pit", cal.pit), ("pred_mean", cal.pred_mean), ("pred_sd", cal.pred_sd), ("crps", cal.crps_i)):
        err = np.abs(d - r[k])
        worst = int(np.argmax(err / (1e-12 + 1e-9 * np.abs(r[k]))))
        print(f"{k}: max abs err {err.max():.3e}, max rel err {np.max(err / np.abs(r[k])):.3e} (row {worst}: {d[worst]!r} vs {r[k][worst]!r})")
    for k, d in (("pit", cal.pit), ("pred_mean", cal.pred_mean), ("pred_sd", cal.pred_sd), ("crps", cal.crps_i)):
        np.testing.assert_allclose(d, r[k], rtol=1e-9, atol=1e-12, err_msg=k)
    # quantiles by residual, and non-decreasing in p
    ps = sorted(cal.quantiles)
    for n in range(0, len(y), max(1, len(y) // 40)):
        for p in ps:
            assert abs(ref.mixture_cdf(cal.quantiles[p][n], fx[:, n], eta, counts) - p) <= 1e-12, (p, n)
    q = np.stack([cal.quantiles[p] for p in ps])
    assert np.all(np.diff(q, axis=0) >= 0.0)
    assert cal.crps == pytest.approx(float(np.mean(r["crps"])), rel=1e-9)
    assert cal.se_crps == pytest.approx(float(np.std(r["crps"], ddof=1) / math.sqrt(len(y))), rel=1e-6)


def _check_oracle_forward(cal, rows, cols, topo, eta, counts):
    """Against the float64 oracle's forward pass on the distinct vectors cols [P, U]."""
    X, y = rows[:, :topo[0]], rows[:, topo[0]].astype(np.float32).astype(np.float64)
    f_or = np.stack([orc.forward(X, cols[:, j].astype(np.float64), topo)[1][:, 0] for j in range(cols.shape[1])])
    tau2 = np.exp(np.asarray(eta, np.float32).astype(np.float64))
    c = np.asarray(counts, np.float64)
    S = c.sum()
    crps_or = np.empty(len(y))
    pit_or = np.empty(len(y))
    for n in range(len(y)):
        f = f_or[:, n]
        first = np.sum(c * ref.A(y[n] - f, tau2)) / S
        crps_or[n] = first - float(c @ ref.A(f[:, None] - f[None, :], tau2[:, None] + tau2[None, :]) @ c) / (2 * S * S)
        pit_or[n] = np.sum(c * ref.Phi((y[n] - f) / np.sqrt(tau2))) / S
    return f_or, crps_or, pit_or


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)                     # chain-major, as the columns of res[0]
    return pt, res, d, eta


def _device_outputs(pt, data, starts, **kw):
    """The device's own outputs of the distinct samples, [U, n_rows] fp32."""
    pp = pt.posterior_predictive(data, return_samples=True, **kw)
    return pp, pp.samples[starts, :, 0]


def _starts(w, eta):
    wd, ed, c = _runs(w, eta)
    return np.concatenate(([0], np.cumsum(c)[:-1])), wd, ed, c


def test_regression_sunspot(sunspot):
    pt, res, d, eta = sunspot
    starts, wd, ed, c = _starts(res[0].T, eta)
    for data in ("train", "test"):
        rows = d["sunspot_" + data]
        y = rows[:, 4].astype(np.float32).astype(np.float64)
        cal = pt.predictive_calibration(data, quantiles=QS)
        assert cal.n_samples == 8 * 300 and cal.n_distinct == len(c) < cal.n_samples
        pp, fx = _device_outputs(pt, data, starts)
        _check_reduction(cal, fx, ed, c, y)
        # the existing calls
        np.testing.assert_allclose(cal.pred_mean, pp.mean[:, 0], rtol=1e-12)
        # coverage from the PIT = coverage counted from the quantile pairs, away from the interval ends
        for lvl, share in cal.coverage.items():
            lo, hi = (1 - lvl) / 2, (1 + lvl) / 2
            ql = cal.quantiles[min(QS, key=lambda p: abs(p - lo))]
            qh = cal.quantiles[min(QS, key=lambda p: abs(p - hi))]
            safe = (np.abs(cal.pit - lo) > 1e-9) & (np.abs(cal.pit - hi) > 1e-9)
            inside_pit = (cal.pit >= lo) & (cal.pit <= hi)
            inside_q = (y >= ql) & (y <= qh)
            assert np.array_equal(inside_pit[safe], inside_q[safe]), lvl
            assert share == pytest.approx(np.mean(inside_pit))
        assert set(cal.intervals) == {(0.025, 0.975), (0.05, 0.95), (0.1, 0.9), (0.25, 0.75)}
        assert cal.pit_hist.sum() == len(y) and cal.brier is None and cal.p_mean is None
        # against the oracle's float64 forward pass
        f_or, crps_or, pit_or = _check_oracle_forward(cal, rows, wd.T, (4, 5, 1), ed, c)
        np.testing.assert_allclose(cal.crps_i, crps_or, rtol=1e-5, atol=ATOL)
        tau_min = math.sqrt(math.exp(float(np.min(ed))))
        bound = (1.0 / math.sqrt(2 * math.pi)) / tau_min * np.max(np.abs(fx.astype(np.float64) - f_or))
        print(f"{data}: max |pit - pit_oracle| = {np.max(np.abs(cal.pit - pit_or)):.3e}, derived bound {bound:.3e}")
        assert np.max(np.abs(cal.pit - pit_or)) <= bound


def test_sources_blocks_and_selections_agree(sunspot, monkeypatch):
    pt, res, d, eta = sunspot
    base = pt.predictive_calibration("train", quantiles=QS)
    _same(pt.predictive_calibration("train", quantiles=QS, weights=res[0].T, eta=eta), base)
    w, e, c = _runs(res[0].T, eta)
    alt = pt.predictive_calibration("train", quantiles=QS, weights=(w, c), eta=e)
    _same(alt, base)
    assert alt.n_distinct == base.n_distinct
    # several row blocks: one row per block
    monkeypatch.setenv("PTNN_CALIB_SCRATCH_BYTES", "1")
    _same(pt.predictive_calibration("train", quantiles=QS), base)
    monkeypatch.setenv("PTNN_CALIB_SCRATCH_BYTES", str(4 * base.n_distinct * 7))
    _same(pt.predictive_calibration("train", quantiles=QS), base)
    monkeypatch.delenv("PTNN_CALIB_SCRATCH_BYTES")
    # the same samples in another order and grouping: the sums are integer sums
    perm = np.random.default_rng(5).permutation(len(c))
    _same(pt.predictive_calibration("train", quantiles=QS, weights=(w[perm], c[perm]), eta=e[perm]), base)
    # crps=False leaves everything else as it is
    nc = pt.predictive_calibration("train", quantiles=QS, crps=False)
    assert nc.crps is None and nc.crps_i is None and np.array_equal(nc.pit, base.pit) and np.array_equal(nc.pred_sd, base.pred_sd)
    # selections: the cold chain, a chain list, thinning -- trace vs host vectors; U below one tile and not a multiple of it
    S, R = 600, 8
    et = pt._sampler.eta_trace()
    cols = res[0].T.reshape(R, 300, -1)
    cold = int(np.argmin(pt.temperatures))
    for kw, sel_w, sel_e in ((dict(chains="cold"), cols[cold], et[cold, 300:]),
                             (dict(chains=[1, 6]), cols[[1, 6]].reshape(-1, cols.shape[2]), et[[1, 6], 300:].reshape(-1)),
                             (dict(thin=3), cols[:, ::3].reshape(-1, cols.shape[2]), et[:, 300::3].reshape(-1)),
                             (dict(chains=[2], burn_in=0.9), cols[2, 240:], et[2, 540:])):
        a = pt.predictive_calibration("test", quantiles=QS, **kw)
        b = pt.predictive_calibration("test", quantiles=QS, weights=sel_w, eta=sel_e)
        _same(a, b)
        assert a.n_distinct == b.n_distinct
        print(kw, "n_distinct", a.n_distinct)
        starts, wd, ed, cc = _starts(sel_w, sel_e)
        _, fx = _device_outputs(pt, "test", starts, weights=sel_w)
        _check_reduction(a, fx, ed, cc, d["sunspot_test"][:, 4].astype(np.float32).astype(np.float64))
    assert pt.predictive_calibration("test", chains=[2], burn_in=0.9).n_distinct < 256


def test_classification_iris(tmp_path):
    d = parity.datasets()
    topo = (4, 12, 3)
    pt = _pt(orc.TASK_CLS, topo, d["iris_train"], d["iris_test"], 8, 400, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    import warnings
    for data in ("train", "test"):
        cal = pt.predictive_calibration(data)
        pp = pt.posterior_predictive(data)
        assert np.array_equal(cal.p_mean, pp.mean)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa = pt.predictive_accuracy(data)
        np.testing.assert_allclose(cal.log_score_i, -pa.lppd_i, rtol=1e-9)
        y = d["iris_" + data][:, 4].astype(np.int64)
        onehot = np.eye(3)[y]
        np.testing.assert_allclose(cal.brier_i, np.sum((pp.mean - onehot) ** 2, axis=1), rtol=1e-14)
        assert cal.brier == pytest.approx(float(np.mean(cal.brier_i)))
        assert np.array_equal(cal.correct, np.argmax(pp.mean, axis=1) == y)
        assert cal.reliability["count"].sum() == len(y) and 0.0 <= cal.ece <= cal.mce <= 1.0
        assert cal.pit is None and cal.crps is None and cal.quantiles is None
        alt = pt.predictive_calibration(data, weights=res[0].T)
        assert np.array_equal(alt.p_mean, cal.p_mean)
        assert np.array_equal(pt.predictive_calibration(data, thin=3, chains=[0, 3]).p_mean,
                              pt.posterior_predictive(data, thin=3, chains=[0, 3]).mean)


def test_wide_net_compact_traces(tmp_path):
    d = parity.datasets()
    R, S, topo = 4, 200, (32, 256, 1)
    pt = _pt(orc.TASK_REG, topo, d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, S // 2:].reshape(-1)
    cal = pt.predictive_calibration("test", quantiles=QS)
    _same(pt.predictive_calibration("test", quantiles=QS, weights=res[0].T, eta=eta), cal)
    starts, wd, ed, c = _starts(res[0].T, eta)
    _, fx = _device_outputs(pt, "test", starts)
    y = d["synth32_test"][:, 32].astype(np.float32).astype(np.float64)
    _check_reduction(cal, fx, ed, c, y)
    f_or, crps_or, pit_or = _check_oracle_forward(cal, d["synth32_test"], wd.T, topo, ed, c)
    np.testing.assert_allclose(cal.crps_i, crps_or, rtol=1e-5, atol=ATOL)
    bound = (1.0 / math.sqrt(2 * math.pi)) / math.sqrt(math.exp(float(np.min(ed)))) * np.max(np.abs(fx.astype(np.float64) - f_or))
    assert np.max(np.abs(cal.pit - pit_or)) <= bound


def test_calibrated_known_answer(tmp_path):
    """Vectors that all give the same constant output (zero weights, one output bias) with one eta, scored on targets bias-output
    + tau z: the mixture is one Gaussian, so PIT = Phi(z) and the CRPS is the single-Gaussian closed form."""
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    P = pt.num_param
    w = np.zeros((300, P), np.float32)
    w[:, P - 1] = 0.3                                             # the output bias
    eta = np.full(300, -3.0, np.float32)
    rng = np.random.default_rng(11)
    z = rng.standard_normal(500)
    x = rng.uniform(0, 1, (500, 4)).astype(np.float32)
    const = pt.posterior_predictive(x, weights=w[:1]).mean[0, 0]   # the device's fp32 output of the constant net
    assert np.all(pt.posterior_predictive(x, weights=w[:1]).mean[:, 0] == const)
    tau = math.exp(-1.5)
    y = (const + tau * z).astype(np.float32)
    cal = pt.predictive_calibration(np.column_stack([x, y]), weights=w, eta=eta, quantiles=(0.1, 0.5, 0.9))
    assert cal.n_distinct == 1 and cal.n_samples == 300
    zz = (y.astype(np.float64) - const) / tau
    nd = NormalDist()
    np.testing.assert_allclose(cal.pit, [nd.cdf(v) for v in zz], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cal.crps_i, [ref.crps_gaussian(float(v), const, tau) for v in y.astype(np.float64)], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cal.pred_mean, const, rtol=1e-12)
    np.testing.assert_allclose(cal.pred_sd, tau, rtol=1e-9)
    for p in (0.1, 0.5, 0.9):
        np.testing.assert_allclose(cal.quantiles[p], const + tau * nd.inv_cdf(p), rtol=1e-12)
    # several distinct vectors with the same output: still one Gaussian
    w2 = w.copy()
    w2[::2, 0] = 1.0                                              # an input weight into a hidden unit whose output weight is 0
    cal2 = pt.predictive_calibration(np.column_stack([x, y]), weights=w2, eta=eta)
    assert cal2.n_distinct == 300
    np.testing.assert_allclose(cal2.crps_i, cal.crps_i, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cal2.pit, cal.pit, rtol=1e-9, atol=1e-12)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(60, 100)["pos_w"].reshape(-1, pt.num_param)
            e = pt._sampler.trace_rows(60, 100)[:, :, 3].reshape(-1)          # eta of those rows
            cal = pt.predictive_calibration("test", weights=w, eta=e)
            assert cal.n_samples == 800 and np.all(np.isfinite(cal.crps_i))
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
        pt.predictive_calibration("test")
    res = pt.run_chains()
    with pytest.raises(ValueError, match="eta"):
        pt.predictive_calibration("test", weights=res[0].T)
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt.predictive_calibration("test", burn_in=0)
    # more distinct samples than the pair term takes: refused before the forward pass; crps=False has no such cap
    rng = np.random.default_rng(2)
    n = _lib.CALIB_MAX_DISTINCT + 1
    w = (0.1 * rng.standard_normal((n, pt.num_param))).astype(np.float32)
    eta = np.full(n, -3.0, np.float32)
    with pytest.raises(_lib.PtnnError, match=r"thin=.*chains=.*crps=False"):
        pt.predictive_calibration(te[:8], weights=w, eta=eta)
    big = pt.predictive_calibration(te[:8], weights=w, eta=eta, crps=False)
    assert big.n_distinct == n and big.crps is None and np.all((big.pit > 0) & (big.pit < 1))
    # the C entry itself: class probabilities of a regression
    import ctypes as C
    out = np.empty((len(te), 1))
    spec = _lib.CalibrationSpec()
    spec.struct_bytes = C.sizeof(_lib.CalibrationSpec)
    spec.thin, spec.step0, spec.nsteps, spec.n_rows, spec.x_source = 1, 100, 100, len(te), _lib.PREDICT_X_TEST
    spec.p_mean = out.ctypes.data_as(C.POINTER(C.c_double))
    with pytest.raises(_lib.PtnnError, match="p_mean"):
        pt._sampler._check(pt._sampler.lib.ptnn_calibration(pt._sampler.h, C.byref(spec)))
    ok = pt.predictive_calibration("test")                                # the handle is still usable
    assert ok.n_samples == 400
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        ls.predictive_calibration("test")


def test_sharded_ladder_is_refused(tmp_path):
    """A ladder sharded over several devices has no single handle: refused before anything is launched."""
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    pt.run_chains()
    one = pt._sampler
    pt._sampler = object()                                        # what a ladder over several devices keeps in its place
    try:
        with pytest.raises(ValueError, match="one GPU"):
            pt.predictive_calibration("test")
    finally:
        pt._sampler = one
    assert pt.predictive_calibration("test", crps=False).n_samples == 400
