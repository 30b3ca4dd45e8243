"""Predictive accuracy, host side (no GPU): the float64 oracle's known answers and edge cases, the Pareto k-hat against draws of a
known shape, elpd_compare's arithmetic, the exported entry point and its argument checks, which run before anything touches a
device."""
import ctypes as C
import math

import numpy as np
import pytest

import elpd_ref as ref


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def test_oracle_known_answers():
    # two samples, two rows: by hand
    ll = np.array([[-1.0, -2.0],
                   [-3.0, -2.0]])
    r = ref.elpd_rows(ll)
    lppd0 = math.log((math.exp(-1.0) + math.exp(-3.0)) / 2)
    assert r["lppd"][0] == pytest.approx(lppd0, rel=1e-14)
    assert r["lppd"][1] == pytest.approx(-2.0, rel=1e-14)
    assert r["p_waic"][0] == pytest.approx(2.0, rel=1e-14)                 # var([-1, -3], ddof 1)
    assert r["p_waic"][1] == 0.0
    t = ref.totals(r)
    assert t["elpd_waic"] == pytest.approx(lppd0 - 2.0 - 2.0, rel=1e-14)
    assert t["lppd"] == pytest.approx(lppd0 - 2.0, rel=1e-14)
    # S = 2 leaves no tail: LOO is plain importance sampling, 1 / mean(1 / p)
    assert r["elpd_loo"][0] == pytest.approx(-math.log((math.exp(1.0) + math.exp(3.0)) / 2), rel=1e-14)
    assert np.all(np.isinf(r["khat"])) and np.all(r["tail_len"] <= 4)


@pytest.mark.parametrize("xi", [0.2, 0.5, 0.9])
def test_khat_recovers_the_gpd_shape(xi):
    st = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(int(xi * 10))
    ratios = st.genpareto.rvs(xi, size=20000, random_state=rng)
    ll = -np.log(ratios)[:, None]                                            # log ratios lr = -ll
    r = ref.elpd_rows(ll)
    assert abs(r["khat"][0] - xi) < 0.1
    assert r["tail_len"][0] == math.ceil(3 * math.sqrt(20000))


def test_oracle_edge_cases():
    # a constant log-likelihood: every estimate is the plain one, no penalty
    ll = np.full((50, 3), -1.25)
    r = ref.elpd_rows(ll)
    np.testing.assert_allclose(r["elpd_loo"], r["lppd"], rtol=1e-14)
    assert np.all(r["p_waic"] == 0.0)
    # a tail of at most 4 samples: no fit, k-hat = +inf
    r = ref.elpd_rows(np.random.default_rng(0).standard_normal((20, 2)))
    assert np.all(np.isinf(r["khat"])) and np.all(r["tail_len"] <= 4)
    # expanded vs (distinct, multiplicity): identical
    rng = np.random.default_rng(3)
    distinct = rng.standard_normal((60, 4)) - 2.0
    counts = rng.integers(1, 9, size=60)
    a = ref.elpd_rows(np.repeat(distinct, counts, axis=0))
    b = ref.elpd_rows(distinct, multiplicity=counts)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_elpd_compare_arithmetic(pt):
    from ptnn_amd.parallel_tempering import PredictiveAccuracy, elpd_compare

    def result(loo, lppd, pw):
        return PredictiveAccuracy(*([None] * 8), lppd_i=np.asarray(lppd), elpd_loo_i=np.asarray(loo), p_waic_i=np.asarray(pw),
                                  khat=None, good_k=0.7, n_high_k=0, log_lik=None, n_samples=0, n_distinct=0)
    a = result([-1.0, -2.0, -0.5], [-0.9, -1.8, -0.4], [0.1, 0.1, 0.2])
    b = result([-1.5, -1.0, -1.5], [-1.4, -0.9, -1.2], [0.05, 0.2, 0.1])
    c = elpd_compare(a, b)
    d = np.array([0.5, -1.0, 1.0])
    assert c["elpd_loo_diff"] == pytest.approx(0.5)
    assert c["se_loo_diff"] == pytest.approx(math.sqrt(3 * np.var(d, ddof=1)))
    dw = (np.array([-0.9, -1.8, -0.4]) - [0.1, 0.1, 0.2]) - (np.array([-1.4, -0.9, -1.2]) - [0.05, 0.2, 0.1])
    assert c["elpd_waic_diff"] == pytest.approx(dw.sum())
    assert c["se_waic_diff"] == pytest.approx(math.sqrt(3 * np.var(dw, ddof=1)))
    assert elpd_compare(a, a)["elpd_loo_diff"] == 0.0
    with pytest.raises(ValueError, match="different rows"):
        elpd_compare(a, result([-1.0], [-1.0], [0.0]))


def test_library_exports_elpd(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_elpd is not None and "ptnn_elpd" in _lib.SYMBOLS
    # the library's expected struct_bytes is the binding's sizeof
    s = _spec(struct_bytes=4)
    rc = lib.ptnn_elpd(None, C.byref(s))
    assert rc < 0 and f"expected {C.sizeof(_lib.ElpdSpec)}" in lib.ptnn_last_error().decode()


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.ElpdSpec()
    s.struct_bytes = C.sizeof(_lib.ElpdSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source, s.r_eff = 1, 10, 4, _lib.PREDICT_X_TRAIN, 1.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_elpd(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_elpd_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=8))
    assert rc < 0 and "struct_bytes" in msg
    for r_eff in (0.0, -1.0, float("nan")):
        rc, msg = _err(lib, _spec(r_eff=r_eff))
        assert rc < 0 and "r_eff" in msg
    rc, msg = _err(lib, _spec(nsteps=0))
    assert rc < 0 and "no source" in msg
    rc, msg = _err(lib, _spec(thin=0))
    assert rc < 0 and "thin" in msg
    rc, msg = _err(lib, _spec(x_source=7))
    assert rc < 0 and "x_source" in msg
    rc, msg = _err(lib, _spec(n_rows=0))
    assert rc < 0 and "n_rows" in msg
    w = np.zeros(8, np.float32)
    ll = np.zeros(8)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(fp), loglik=ll.ctypes.data_as(dp), n_w=2))
    assert rc < 0 and "not both" in msg
    rc, msg = _err(lib, _spec(loglik=ll.ctypes.data_as(dp), n_w=0))
    assert rc < 0 and "n_w" in msg
    bad = np.array([0.0, np.inf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    rc, msg = _err(lib, _spec(loglik=bad.ctypes.data_as(dp), n_w=2))
    assert rc < 0 and "not finite" in msg
    mu = np.array([1, -1], np.int32)
    rc, msg = _err(lib, _spec(loglik=ll.ctypes.data_as(dp), n_w=2, multiplicity=mu.ctypes.data_as(C.POINTER(C.c_int32))))
    assert rc < 0 and "negative" in msg
    # a consistent request reaches the handle check
    rc, msg = _err(lib, _spec())
    assert rc < 0 and "null handle" in msg
    rc, msg = _err(lib, _spec(loglik=ll.ctypes.data_as(dp), n_w=2))
    assert rc < 0 and "null handle" in msg
