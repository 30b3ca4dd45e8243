"""Calibration, host side (no GPU): the float64 oracle's CRPS against a quadrature of its definition, its PIT and quantiles, the
accuracy of the closed form against 40-digit arithmetic, the host arithmetic of predictive_calibration on hand-made inputs, and
the argument checks, which run before anything touches a device."""
import ctypes as C
import math
from statistics import NormalDist

import numpy as np
import pytest

import calibration_ref as ref


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def _mixture(seed, U, spread=0.05, eta_lo=-6.0, eta_hi=-4.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.5, spread, U).astype(np.float32), rng.uniform(eta_lo, eta_hi, U).astype(np.float32),
            rng.integers(1, 6, U))


def test_crps_equals_the_threshold_integral():
    for seed, U in ((1, 50), (2, 7), (3, 23)):
        f, eta, c = _mixture(seed, U)
        for y in (0.5, 0.41, 0.9):
            assert ref.crps(y, f, eta, c) == pytest.approx(ref.crps_quadrature(y, f, eta, c), rel=1e-9)
            assert ref.crps(y, f, eta) == pytest.approx(ref.crps_quadrature(y, f, eta), rel=1e-9)
    # one component 100 times narrower than the spread of f
    f, eta, c = _mixture(4, 20, spread=0.1)
    eta[3] = np.float32(2.0 * math.log(0.001))
    assert ref.crps(0.55, f, eta, c) == pytest.approx(ref.crps_quadrature(0.55, f, eta, c, n=2000001), rel=1e-8)
    # U = 1: the single-Gaussian closed form
    f1, e1 = np.array([0.3], np.float32), np.array([-3.0], np.float32)
    mu, sd = float(f1[0]), math.exp(-1.5)
    for y in (0.3, 0.1, 1.4):
        assert ref.crps(y, f1, e1) == pytest.approx(ref.crps_gaussian(y, mu, sd), rel=1e-13)
        assert ref.crps(y, f1, e1, [7]) == pytest.approx(ref.crps_gaussian(y, mu, sd), rel=1e-13)
        assert ref.crps(y, f1, e1) == pytest.approx(ref.crps_quadrature(y, f1, e1), rel=1e-9)


def test_expanded_equals_distinct_with_multiplicity():
    f, eta, c = _mixture(5, 40)
    fe, ee = np.repeat(f, c), np.repeat(eta, c)
    for y in (0.45, 0.6):
        assert ref.pit(y, fe, ee) == pytest.approx(ref.pit(y, f, eta, c), rel=1e-14)
        assert ref.crps(y, fe, ee) == pytest.approx(ref.crps(y, f, eta, c), rel=1e-12)
    ma, mb = ref.moments(fe, ee), ref.moments(f, eta, c)
    assert ma[0] == pytest.approx(mb[0], rel=1e-14) and ma[1] == pytest.approx(mb[1], rel=1e-13)


def test_quantiles_solve_the_cdf_and_are_monotone():
    f, eta, c = _mixture(6, 50, spread=0.2)
    ps = (0.001, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 0.999)
    q = [ref.quantile(p, f, eta, c) for p in ps]
    for p, z in zip(ps, q):
        assert abs(ref.mixture_cdf(z, f, eta, c) - p) <= 1e-12
    assert np.all(np.diff(q) >= 0.0)
    # one component: the Gaussian quantile
    assert ref.quantile(0.9, [0.25], [-2.0]) == pytest.approx(0.25 + math.exp(-1.0) * NormalDist().inv_cdf(0.9), rel=1e-14)


def test_closed_form_accuracy_against_40_digits():
    """The float64 closed form against 40-digit arithmetic on three 80-component mixtures: the backing of the 1e-9 bound the
    GPU tests put on crps, a difference of two sums of similar size."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40

    def A(m, v):
        x = m / mp.sqrt(v)
        return m * mp.erf(x / mp.sqrt(2)) + 2 * mp.sqrt(v) * mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)

    for seed, spread, (elo, ehi) in ((11, 0.002, (-9.0, -8.0)), (12, 0.02, (-7.5, -6.0)), (13, 0.2, (-9.0, -6.0))):
        f, eta, c = _mixture(seed, 80, spread, elo, ehi)
        y = 0.5 + spread
        F = [mp.mpf(float(v)) for v in f]
        T = [mp.exp(mp.mpf(float(e))) for e in eta]
        S = int(np.sum(c))
        first = sum(int(c[s]) * A(mp.mpf(y) - F[s], T[s]) for s in range(80)) / S
        pair = sum(int(c[s]) * int(c[t]) * A(F[s] - F[t], T[s] + T[t]) for s in range(80) for t in range(80)) / (2 * S * S)
        exact = first - pair
        got = ref.crps(y, f, eta, c)
        rel = abs((mp.mpf(got) - exact) / exact)
        print(f"spread {spread}: crps {got!r}, relative error {float(rel):.2e}, first term / result {float(first / exact):.2f}")
        assert rel < 1e-12


def test_coverage_histogram_and_interval_score(pt):
    from ptnn_amd.parallel_tempering import crps_summary, interval_scores, pit_coverage, pit_histogram
    lo9, hi9 = (1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0
    pit = np.array([lo9, hi9, 0.5, 0.01, 0.99, 0.3, np.nextafter(lo9, 0.0), np.nextafter(hi9, 1.0)])
    cov = pit_coverage(pit, (0.5, 0.9))
    assert cov[0.9] == 4 / 8                        # both ends are inside, their neighbours outside
    assert cov[0.5] == 2 / 8                        # 0.5 and 0.3
    assert list(pit_histogram(pit, 4)) == [3, 1, 1, 3]
    assert list(pit_histogram([0.0, 1.0, 0.25], 4)) == [1, 1, 0, 1]
    # interval score: inside, below, above; a = 0.2
    q = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]])
    y = np.array([2.5, 0.5, 3.25])
    out = interval_scores((0.1, 0.5, 0.9), q, y)
    assert set(out) == {(0.1, 0.9)}
    r = out[(0.1, 0.9)]
    assert r["level"] == pytest.approx(0.8) and r["width"] == 2.0
    assert r["score"] == pytest.approx((2.0 + (2.0 + 10.0 * 0.5) + (2.0 + 10.0 * 0.25)) / 3.0)
    assert interval_scores((0.05, 0.5), q[:2], y) == {}
    m, se = crps_summary([1.0, 2.0, 3.0, 4.0])
    assert m == 2.5 and se == pytest.approx(np.std([1, 2, 3, 4], ddof=1) / 2.0)


def test_brier_reliability_ece(pt):
    from ptnn_amd.parallel_tempering import classification_scores, reliability_table
    p = np.array([[0.3, 0.7], [1.0, 0.0], [0.5, 0.5], [0.25, 0.75], [0.9, 0.1]])
    y = np.array([1, 0, 1, 0, 0])
    sc = classification_scores(p, y, bins=10)
    np.testing.assert_allclose(sc["brier_i"], [0.18, 0.0, 0.5, 1.125, 0.02], rtol=1e-14)
    np.testing.assert_allclose(sc["log_score_i"], -np.log([0.7, 1.0, 0.5, 0.25, 0.9]), rtol=1e-14)
    assert list(sc["confidence"]) == [0.7, 1.0, 0.5, 0.75, 0.9]
    assert list(sc["correct"]) == [True, True, False, False, True]     # the tie goes to class 0, which is wrong for row 2
    cnt = sc["reliability"]["count"]
    # 0.7 on the edge of bins 6 | 7 goes up; 1.0 goes to the last bin, with 0.9; 0.5 on an edge goes up; the rest are empty
    assert list(cnt) == [0, 0, 0, 0, 0, 1, 0, 2, 0, 2]
    acc, conf = sc["reliability"]["accuracy"], sc["reliability"]["confidence"]
    assert np.isnan(acc[0]) and np.isnan(conf[6])
    assert acc[5] == 0.0 and conf[5] == 0.5 and acc[7] == 0.5 and conf[7] == pytest.approx(0.725) and acc[9] == 1.0
    gaps = [0.5, 0.225, 0.05]
    assert sc["ece"] == pytest.approx((1 * gaps[0] + 2 * gaps[1] + 2 * gaps[2]) / 5) and sc["mce"] == pytest.approx(0.5)
    one = reliability_table([0.2, 0.2], [1, 0], bins=1)
    assert list(one["count"]) == [2] and one["ece"] == pytest.approx(0.3)
    with pytest.raises(ValueError, match="labels"):
        classification_scores(p, [0, 1, 2, 0, 0])


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.CalibrationSpec()
    s.struct_bytes = C.sizeof(_lib.CalibrationSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source = 1, 10, 4, _lib.PREDICT_X_TRAIN
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_calibration(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_calibration is not None and "ptnn_calibration" in _lib.SYMBOLS and lib.ptnn_abi_version() == 4
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc < 0 and f"expected {C.sizeof(_lib.CalibrationSpec)}" in msg
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    for kw, word in ((dict(nsteps=0), "no source"), (dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(n_rows=0), "n_rows"),
                     (dict(n_levels=17), "n_levels"), (dict(n_levels=2), "levels_p")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and word in msg, (kw, msg)
    dp = C.POINTER(C.c_double)
    q = np.empty((2, 4))
    z = np.zeros(2)
    for bad in ([0.5, 1.0], [0.0, 0.5], [0.5, float("nan")], [-0.1, 0.5]):
        lv = np.array(bad)
        rc, msg = _err(lib, _spec(n_levels=2, levels_p=lv.ctypes.data_as(dp), levels_z=z.ctypes.data_as(dp), quantiles=q.ctypes.data_as(dp)))
        assert rc < 0 and "(0, 1)" in msg
    rc, msg = _err(lib, _spec(quantiles=q.ctypes.data_as(dp)))
    assert rc < 0 and "without levels" in msg
    rc, msg = _err(lib, _spec(crps=q.ctypes.data_as(dp)))
    assert rc < 0 and "pair_term" in msg
    mu = np.array([1, -1], np.int32)
    w = np.zeros(8, np.float32)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(C.POINTER(C.c_float)), n_w=2, multiplicity=mu.ctypes.data_as(C.POINTER(C.c_int32))))
    assert rc < 0 and "negative" in msg
    # a consistent request reaches the handle check
    lv = np.array([0.05, 0.95])
    rc, msg = _err(lib, _spec(n_levels=2, levels_p=lv.ctypes.data_as(dp), levels_z=z.ctypes.data_as(dp), quantiles=q.ctypes.data_as(dp), pair_term=1))
    assert rc < 0 and "null handle" in msg


def test_public_call_validates_before_it_needs_a_device(pt, tmp_path):
    from ptnn_amd.parallel_tempering import check_probability_levels
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    import parity
    d = parity.datasets()
    obj = ParallelTempering(True, 0.1, d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 4, 2, 4 * 50, 10, 0.5, str(tmp_path),
                            seed=1, write_files=False)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        obj.predictive_calibration("test", quantiles=(0.05, 1.0))
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        obj.predictive_calibration("test", levels=(0.0, 0.9))
    with pytest.raises(ValueError, match="at most 16"):
        obj.predictive_calibration("test", quantiles=np.linspace(0.01, 0.99, 17))
    with pytest.raises(ValueError, match="eta"):
        obj.predictive_calibration("test", weights=np.zeros((3, obj.num_param), np.float32))
    with pytest.raises(ValueError, match="bins"):
        obj.predictive_calibration("test", bins=0)
    with pytest.raises(ValueError, match="data must be"):
        obj.predictive_calibration("validation")
    with pytest.raises(ValueError, match="run_chains"):
        obj.predictive_calibration("test")                         # no handle yet: before initialize_chains() / run_chains()
    assert check_probability_levels("levels", (0.5, 0.9)) == [0.5, 0.9]
