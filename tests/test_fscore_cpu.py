"""Forecast verification, host side (no GPU): the series behind the shipped window rows, the truth layout,
the per-horizon summary, baselines and skill against hand-computable inputs, the energy score's two known properties,
forecast_compare's refusal, and the argument checks of ptnn_forecast_score, which run before the handle is looked at."""
import ctypes as C
import math

import numpy as np
import pytest

import calibration_ref as cref
import fscore_ref as ref
import parity


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


@pytest.fixture(scope="module")
def ver(pt):
    from ptnn_amd import verification
    return verification


@pytest.mark.parametrize("name,n_in", [("sunspot", 4), ("mackey", 4), ("sunspot5", 5)])
def test_series_from_windows_on_the_golden_rows(ver, name, n_in):
    te = parity.datasets()[name + "_test"]
    series, stride = ver.series_from_windows(te, n_in)
    assert stride == 2 and series.shape == (n_in + 1 + 2 * (te.shape[0] - 1),)
    if n_in == 4:
        assert series.shape == (399,)
    again = np.stack([series[2 * k:2 * k + n_in + 1] for k in range(te.shape[0])])
    assert again.tobytes() == np.ascontiguousarray(te[:, :n_in + 1]).tobytes()
    # shuffled rows are no windows of one series
    perm = np.random.default_rng(0).permutation(te.shape[0])
    with pytest.raises(ValueError, match="series="):
        ver.series_from_windows(te[perm], n_in)


def test_series_from_windows_edge_cases(ver):
    # a constant series: every stride fits, the smallest is taken
    rows = np.full((6, 5), 0.25, np.float32)
    series, stride = ver.series_from_windows(rows, 4)
    assert stride == 1 and np.array_equal(series, np.full(10, 0.25, np.float32))
    # delay-1 windows cut at every step, and one row alone
    x = np.arange(12, dtype=np.float64) / 7.0
    rows = np.stack([x[t:t + 4] for t in range(9)])
    series, stride = ver.series_from_windows(rows, 3)
    assert stride == 1 and np.array_equal(series, x)
    series, stride = ver.series_from_windows(rows[:1], 3)
    assert stride == 1 and np.array_equal(series, x[:4])
    # stride 3 of n_in = 3: the rows share one value
    rows = np.stack([x[t:t + 4] for t in range(0, 9, 3)])
    assert ver.series_from_windows(rows, 3)[1] == 3
    # -0.0 and 0.0 are different bits
    a = np.array([[0.0, 1.0, 2.0], [1.0, 2.0, 3.0]])
    b = a.copy()
    b[1, 0] = 1.0000000000000002
    with pytest.raises(ValueError, match="series="):
        ver.series_from_windows(b, 2)


def test_truth_layout_on_sunspot(ver):
    te = parity.datasets()["sunspot_test"]
    assert te.shape[0] == 198
    series, s = ver.series_from_windows(te.astype(np.float32), 4)
    org, truth = ver.windows_and_truth(series, 4, 6, s, n_origins=198)
    assert org.shape == (198, 4) and truth.shape == (198, 6) and truth.dtype == np.float32
    assert np.array_equal(org, te[:, :4].astype(np.float32))
    assert np.array_equal(truth[:, 0], te[:, 4].astype(np.float32))                  # step 1's truth is the row's own target
    assert np.isfinite(truth).sum(axis=0).tolist() == [198, 197, 197, 196, 196, 195]
    for r in (0, 57, 196, 197):
        for k in range(1, 7):
            j = r * 2 + 4 - 1 + k
            want = series[j] if j < series.size else np.nan
            assert (truth[r, k - 1] == want) or (math.isnan(want) and math.isnan(truth[r, k - 1]))
    # series= with a stride of its own
    x = np.arange(20, dtype=np.float32)
    org, truth = ver.windows_and_truth(x, 3, 4, 5)
    assert org.tolist() == [[0, 1, 2], [5, 6, 7], [10, 11, 12], [15, 16, 17]]
    assert truth[:3].tolist() == [[3, 4, 5, 6], [8, 9, 10, 11], [13, 14, 15, 16]]
    assert truth[3, :2].tolist() == [18, 19] and np.isnan(truth[3, 2:]).all()
    with pytest.raises(ValueError, match="holds no window"):
        ver.windows_and_truth(x[:3], 3, 2)


def test_summary_baselines_and_skill_by_hand(ver):
    nan = np.nan
    truth = np.array([[1.0, 2.0], [3.0, nan], [5.0, 4.0]], np.float32)
    mean = np.array([[1.5, 2.0], [2.0, 9.0], [5.0, 1.0]])
    crps = np.array([[0.1, 0.4], [0.2, nan], [0.6, 0.2]])
    logs = np.array([[-1.0, -2.0], [-2.0, nan], [-6.0, -4.0]])
    pit = np.array([[0.5, 0.04], [0.3, nan], [0.97, 0.6]])
    q = np.array([[[0.5, 1.0], [2.5, 0.0], [5.5, 3.0]], [[2.0, 3.0], [4.0, 0.0], [6.0, 3.5]]])     # 5 % and 95 %
    sm = ver.horizon_summary(truth, mean, crps=crps, log_score=logs, pit=pit, levels=(0.5, 0.9), bins=4,
                             quantile_levels=(0.05, 0.95), quantiles=q)
    assert sm["n"].tolist() == [3, 2]
    # errors at step 1: 0.5, -1, 0; at step 2: 0, -3
    np.testing.assert_allclose(sm["rmse"], [math.sqrt(1.25 / 3), math.sqrt(4.5)], rtol=1e-15)
    np.testing.assert_allclose(sm["mae"], [0.5, 1.5], rtol=1e-15)
    np.testing.assert_allclose(sm["bias"], [-1.0 / 6.0, -1.5], rtol=1e-15)
    np.testing.assert_allclose(sm["crps"], [0.3, 0.3], rtol=1e-15)
    np.testing.assert_allclose(sm["se_crps"], [math.sqrt(0.07 / 3), 0.1], rtol=1e-14)
    np.testing.assert_allclose(sm["log_score"], [-3.0, -3.0], rtol=1e-15)
    np.testing.assert_allclose(sm["se_log_score"], [math.sqrt(7.0 / 3), 1.0], rtol=1e-14)
    assert sm["coverage"][0.5].tolist() == [2 / 3, 0.5] and sm["coverage"][0.9].tolist() == [2 / 3, 0.5]
    assert sm["pit_hist"].tolist() == [[0, 1, 1, 1], [1, 0, 1, 0]]
    iv = sm["intervals"][(0.05, 0.95)]
    assert iv["level"] == pytest.approx(0.9)
    # a = 0.1, 2 / a = 20.  Step 1: widths 1.5, 1.5, 0.5; y = 1 and 3 lie inside, 5 below 5.5 by 0.5 -> + 20 * 0.5.  Step 2: widths
    # 2, 0.5; y = 2 inside, 4 above 3.5 by 0.5 -> + 20 * 0.5
    np.testing.assert_allclose(iv["width"], [3.5 / 3, 1.25], rtol=1e-15)
    np.testing.assert_allclose(iv["score"], [(1.5 + 1.5 + 0.5 + 10.0) / 3, (2.0 + 0.5 + 10.0) / 2], rtol=1e-15)
    # a step nobody observed
    none = ver.horizon_summary(np.array([[1.0, nan]], np.float32), np.array([[1.0, 2.0]]), crps=np.array([[0.1, nan]]))
    assert none["n"].tolist() == [1, 0] and math.isnan(none["rmse"][1]) and math.isnan(none["crps"][1]) and math.isnan(none["se_crps"][0])
    # baselines: persistence = the origin's last value; climatology = N(m, s^2) of the training targets
    last = np.array([0.0, 3.0, 4.0], np.float32)
    train = np.array([1.0, 2.0, 3.0, 6.0])
    m, s = 3.0, math.sqrt(14.0 / 3.0)
    base = ver.forecast_baselines(last, truth, train)
    np.testing.assert_allclose(base["rmse_persistence"], [math.sqrt(2.0 / 3), math.sqrt(2.0)], rtol=1e-15)
    np.testing.assert_allclose(base["mae_persistence"], [2.0 / 3, 1.0], rtol=1e-15)
    np.testing.assert_allclose(base["rmse_climatology"], [math.sqrt(8.0 / 3), math.sqrt(1.0)], rtol=1e-15)
    want = [np.mean([cref.crps_gaussian(y, m, s) for y in (1.0, 3.0, 5.0)]), np.mean([cref.crps_gaussian(y, m, s) for y in (2.0, 4.0)])]
    np.testing.assert_allclose(base["crps_climatology"], want, rtol=1e-13)
    # the closed form against quadrature of the definition
    quad = cref.crps_quadrature(1.0, np.array([m]), np.array([math.log(s * s)]))
    assert ver.crps_gaussian(1.0, m, s) == pytest.approx(quad, rel=1e-5)          # eta goes through fp32 in the quadrature
    # skill
    rs, cs, lead = ver.forecast_skill([1.0, 3.0, 2.0], [2.0, 2.0, 2.0], [0.2, 0.3, 0.5, 0.1], [0.4, 0.4, 0.4, 0.4])
    assert rs.tolist() == [0.5, -0.5, 0.0] and lead == 2
    np.testing.assert_allclose(cs, [0.5, 0.25, -0.25, 0.75], rtol=1e-15)
    assert ver.forecast_skill([1.0], [2.0])[1:] == (None, None)
    assert ver.forecast_skill([1.0], [2.0], [0.5], [0.4])[2] == 0


def test_energy_score_is_the_ensemble_crps_in_one_dimension(ver):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(40).astype(np.float32)
    c = rng.integers(1, 4, 40)
    y = 0.3
    # the ensemble CRPS: E|X - y| - E|X - X'| / 2 over the weighted members
    xs = np.repeat(x.astype(np.float64), c)
    want = np.mean(np.abs(xs - y)) - 0.5 * np.mean(np.abs(xs[:, None] - xs[None, :]))
    assert ver.energy_score_ensemble(x[:, None], [y], c) == pytest.approx(want, rel=1e-13)
    assert ref.energy_score(x[:, None], np.array([y], np.float32), c) == pytest.approx(want, rel=1e-6)   # y through fp32
    # a path with one observed step: the other steps do not count
    paths = rng.standard_normal((40, 3)).astype(np.float32)
    paths[:, 1] = x
    truth = np.array([np.nan, np.float32(y), np.nan], np.float32)
    assert ref.energy_score(paths, truth, c) == ref.energy_score(x[:, None], truth[1:2], c)
    assert math.isnan(ref.energy_score(paths, np.full(3, np.nan, np.float32)))


def test_energy_score_against_a_member_is_not_negative(ver):
    # ES(F, y) = E|Y - y| - E|Y - Y'| / 2 >= 0 by the triangle inequality |Y - Y'| <= |Y - y| + |Y' - y|
    rng = np.random.default_rng(4)
    paths = rng.standard_normal((30, 6)).astype(np.float32)
    for i in range(30):
        es = ref.energy_score(paths, paths[i])
        assert es >= 0.0
        assert es == pytest.approx(ver.energy_score_ensemble(paths, paths[i]), rel=1e-13)
    assert ref.energy_score(np.tile(paths[:1], (5, 1)), paths[0]) == 0.0             # a point mass on the truth


def test_reference_log_score_and_trajectories(ver):
    # one component: the Gaussian log density
    got = ref.log_score(0.4, [0.1], [math.log(0.25)])
    assert got == pytest.approx(-0.5 * math.log(2 * math.pi * 0.25) - 0.5 * 0.09 / 0.25, rel=1e-7)
    # multiplicities are repeats
    f, e = np.array([0.1, 0.5, 0.7], np.float32), np.array([-3.0, -2.0, -4.0], np.float32)
    assert ref.log_score(0.4, f, e, [2, 0, 3]) == pytest.approx(ref.log_score(0.4, f[[0, 0, 2, 2, 2]], e[[0, 0, 2, 2, 2]]), rel=1e-14)
    # the means are the paths without the last step's noise, and the noise is fed back
    import forecast_ref as fref
    topo = (4, 5, 1)
    w = np.random.default_rng(1).standard_normal((3, 31))
    org, truth = ver.windows_and_truth(np.random.default_rng(2).random(8), 4, 6, 3)     # the origins as the product lays them out
    assert org.shape == (2, 4) and np.isfinite(truth).sum(axis=1).tolist() == [4, 1]
    eta = np.array([-3.0, -2.5, -4.0])
    paths, mu = ref.trajectories(w, org, 6, topo, eta=eta, seed=77)
    assert np.array_equal(paths, fref.trajectories(w, org, 6, topo, eta=eta, seed=77))
    clean, mu0 = ref.trajectories(w, org, 6, topo)
    assert np.array_equal(clean, mu0) and np.array_equal(mu[:, :, 0], mu0[:, :, 0]) and not np.array_equal(mu[:, :, 1], mu0[:, :, 1])
    z = np.stack([[fref.noise_draws(6, i, r, 77) for r in range(2)] for i in range(3)])
    np.testing.assert_allclose(paths - mu, np.exp(0.5 * eta)[:, None, None] * z, rtol=0, atol=1e-15)
    # the reference's scores on them: NaN exactly where the product's truth layout has none; its energy score is the product's
    # host helper on the observed steps, and a column's log score the log of the mean Gaussian density
    sc = ref.scores(mu.astype(np.float32), paths.astype(np.float32), eta, truth, levels=(0.5,))
    assert np.array_equal(np.isnan(sc["log_score"]), np.isnan(truth)) and np.array_equal(np.isnan(sc["crps"]), np.isnan(truth))
    for r in range(2):
        K = np.isfinite(truth[r])
        assert sc["energy_score"][r] == pytest.approx(ver.energy_score_ensemble(paths.astype(np.float32)[:, r, K], truth[r, K]), rel=1e-13)
    f, e, y = mu.astype(np.float32).astype(np.float64)[:, 0, 0], eta.astype(np.float32).astype(np.float64), float(truth[0, 0])
    dens = np.exp(-0.5 * (y - f) ** 2 / np.exp(e)) / np.sqrt(2 * math.pi * np.exp(e))
    assert sc["log_score"][0, 0] == pytest.approx(math.log(np.mean(dens)), rel=1e-13)


def _result(ver, truth, crps, logs, es):
    none = dict.fromkeys(ver.ForecastAccuracy._fields)
    none.update(truth=np.asarray(truth, np.float32), crps_i=crps, log_score_i=logs, energy_score=es)
    return ver.ForecastAccuracy(**none)


def test_forecast_compare(ver, pt):
    from ptnn_amd.parallel_tempering import ParallelTemperingBase, forecast_compare
    assert forecast_compare is ver.forecast_compare and hasattr(ParallelTemperingBase, "forecast_accuracy")
    nan = np.nan
    truth = np.array([[1.0, 2.0], [3.0, nan], [5.0, 4.0]])
    a = _result(ver, truth, np.array([[0.1, 0.4], [0.2, nan], [0.6, 0.2]]), np.array([[-1.0, -2.0], [-2.0, nan], [-6.0, -4.0]]),
                np.array([1.0, 2.0, nan]))
    b = _result(ver, truth, np.array([[0.2, 0.1], [0.2, nan], [0.3, 0.1]]), np.array([[-1.5, -2.0], [-1.0, nan], [-3.0, -1.0]]),
                np.array([0.5, 1.0, 3.0]))
    d = forecast_compare(a, b)
    np.testing.assert_allclose(d["crps_diff"], [0.2 / 3, 0.2], rtol=1e-14)
    np.testing.assert_allclose(d["se_crps_diff"], [np.std([-0.1, 0.0, 0.3], ddof=1) / math.sqrt(3), np.std([0.3, 0.1], ddof=1) / math.sqrt(2)],
                               rtol=1e-13)
    np.testing.assert_allclose(d["log_score_diff"], [-3.5 / 3, -1.5], rtol=1e-14)
    assert d["energy_diff"] == pytest.approx(0.75) and d["se_energy_diff"] == pytest.approx(np.std([0.5, 1.0], ddof=1) / math.sqrt(2))
    # other truth -- a value, a NaN elsewhere, another shape -- is refused
    for other in (np.array([[1.0, 2.0], [3.0, nan], [5.0, 4.5]]), np.array([[1.0, 2.0], [3.0, 1.0], [5.0, 4.0]]), truth[:2]):
        with pytest.raises(ValueError, match="different truth"):
            forecast_compare(a, _result(ver, other, b.crps_i[:other.shape[0]], b.log_score_i[:other.shape[0]], None))
    # a result without the CRPS
    d = forecast_compare(a, _result(ver, truth, None, b.log_score_i, None))
    assert d["crps_diff"] is None and d["energy_diff"] is None and d["log_score_diff"] is not None


# ---- the argument checks of ptnn_forecast_score with a NULL handle ----
def _refusal(binding, lib, **fields):
    spec, keep, types = binding.ForecastScoreSpec(), [], dict(binding.ForecastScoreSpec._fields_)
    spec.struct_bytes = C.sizeof(binding.ForecastScoreSpec)
    for name, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v))
            v = keep[-1].ctypes.data_as(types[name])
        setattr(spec, name, v)
    rc = lib.ptnn_forecast_score(None, C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


TRUTH = np.array([[0.1, 0.2], [0.3, np.nan], [np.nan, np.nan]], np.float32)
BASE = dict(nsteps=8, thin=1, origin_source=1, n_origins=3, horizon=2, truth=TRUTH, noise=1)
HOST_W = dict(w=np.zeros((2, 31), np.float32), n_w=2)
d6, d3 = np.zeros(6), np.zeros(3)
REFUSALS = [
    (dict(), "null handle"),                                                        # every argument check passed
    (dict(HOST_W, eta=np.zeros(2, np.float32), pair_term=1, energy=1, crps=d6, energy_score=d3), "null handle"),
    (dict(HOST_W, noise=0), "null handle"),                                         # noise off: the eta is asked for with the handle
    (dict(thin=0), "thin = 0 must be >= 1"),
    (dict(origin_source=7), "origin_source = 7 is not PTNN_FORECAST_ORIGIN_HOST, _TRAIN or _TEST"),
    (dict(origin_source=0), "origin_source PTNN_FORECAST_ORIGIN_HOST needs origins"),
    (dict(n_origins=0), "n_origins = 0 must be >= 1"),
    (dict(horizon=0), "horizon = 0 must be >= 1"),
    (dict(n_origins=70000, horizon=70000), "70000 origins x horizon 70000 = 4900000000 columns: at most 2^31 - 1 per call"),
    (dict(truth=None), "truth is NULL: forecast verification needs the observed values [n_origins, horizon] (NaN = none)"),
    (dict(truth=np.array([[0.1, 0.2], [-np.inf, 0.1], [0.3, 0.3]], np.float32)),
     "truth[1, 0] = -inf is infinite: NaN marks a missing observation"),
    (dict(truth=np.full((3, 2), np.nan, np.float32)), "truth holds no finite entry: nothing to score"),
    (dict(n_levels=17), "n_levels = 17 outside [0, 16]"),
    (dict(n_levels=-1), "n_levels = -1 outside [0, 16]"),
    (dict(n_levels=1, levels_p=np.array([0.5]), levels_z=np.array([0.0])), "n_levels = 1 needs levels_p, levels_z and quantiles"),
    (dict(quantiles=d6), "quantiles requested without levels"),
    (dict(n_levels=1, levels_p=np.array([1.0]), levels_z=np.array([0.0]), quantiles=d6),
     "levels_p[0] = 1 (levels_z 0): a quantile level lies in (0, 1)"),
    (dict(crps=d6), "crps requested without pair_term"),
    (dict(energy_score=d3), "energy_score requested without energy"),
    (dict(energy=1, n_origins=1, horizon=2049, truth=np.zeros((1, 2049), np.float32)),
     "energy: horizon = 2049, the energy score takes paths of at most 2048 steps (energy=False)"),
    (dict(HOST_W), "noise: host vectors need eta = log tau^2 (one per vector)"),
    (dict(HOST_W, n_w=0, eta=np.zeros(2, np.float32)), "n_w = 0 host vectors: need at least one"),
    (dict(HOST_W, eta=np.zeros(2, np.float32), multiplicity=np.array([1, -2], np.int32)), "multiplicity[1] = -2 is negative"),
    # two faults at once: the order of the checks
    (dict(horizon=0, truth=None), "horizon = 0 must be >= 1"),
    (dict(truth=None, crps=d6), "truth is NULL: forecast verification needs the observed values [n_origins, horizon] (NaN = none)"),
    (dict(crps=d6, energy_score=d3), "crps requested without pair_term"),
]


def test_forecast_score_entry_point_is_exported(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_forecast_score is not None and "ptnn_forecast_score" in _lib.SYMBOLS and lib.ptnn_abi_version() == 4
    assert lib.ptnn_forecast_score(None, None) == -1 and lib.ptnn_last_error().decode() == "null argument"
    rc, msg = _refusal(_lib, lib, struct_bytes=8)
    assert (rc, msg) == (-1, f"ptnn_forecast_score_spec.struct_bytes = 8, expected {C.sizeof(_lib.ForecastScoreSpec)}")
    assert C.sizeof(_lib.ForecastScoreSpec) == 224 and _lib.ForecastScoreSpec.truth.offset == 80
    assert _lib.FSCORE_MAX_ENERGY_HORIZON == 2048


@pytest.mark.parametrize("fields,text", REFUSALS, ids=[f"{i}-{t[:28]}" for i, (_, t) in enumerate(REFUSALS)])
def test_forecast_score_refusals_without_a_handle(pt, fields, text):
    from ptnn_amd import _lib
    rc, msg = _refusal(_lib, pt.load_library(), **{**BASE, **fields})
    assert (rc, msg) == (-1, text)
