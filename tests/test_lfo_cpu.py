"""Leave-future-out cross-validation, host side (no GPU): the identities that tie the float64 oracle to PSIS-LOO and lppd, the
oracle with refits against the exact LFO of a conjugate model, the walk on scripted k-hat tables, elpd_compare on two results,
and the argument checks, which run before anything touches a device."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import elpd_ref
import lfo_ref as ref


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


@pytest.fixture(scope="module")
def par(pt):
    from ptnn_amd import parallel_tempering
    return parallel_tempering


def _ll(seed, S=400, N=12):
    rng = np.random.default_rng(seed)
    return -0.5 * (rng.normal(0.0, 1.0, (S, 1)) + 0.3 * rng.normal(0.0, 1.0, (S, N))) ** 2 - 1.0


def test_identities_with_loo_and_lppd():
    ll = _ll(1)
    S, N = ll.shape
    loo = elpd_ref.elpd_rows(ll)
    for n_fit in (N, 7):
        # the origin just before the fit, block 1, removes exactly row n_fit - 1: PSIS-LOO of that row
        back = ref.lfo_rows(ll, n_fit, [n_fit - 1])
        assert back["elpd_lfo"][0] == pytest.approx(loo["elpd_loo"][n_fit - 1], rel=1e-10)
        assert back["khat"][0] == pytest.approx(loo["khat"][n_fit - 1], abs=1e-9) and back["tail_len"][0] == loo["tail_len"][n_fit - 1]
    # the origin at the fit: uniform weights, lppd of that row; no tail, k-hat +inf
    at = ref.lfo_rows(ll, 7, [7])
    assert at["elpd_lfo"][0] == pytest.approx(loo["lppd"][7], rel=1e-10)
    assert np.isinf(at["khat"][0]) and at["tail_len"][0] == 0
    # block > 1 at the fit: the joint density of the block
    at3 = ref.lfo_rows(ll, 7, [7], block=3)
    joint = ll[:, 7:10].sum(axis=1)
    assert at3["elpd_lfo"][0] == pytest.approx(np.log(np.mean(np.exp(joint))), rel=1e-10)
    # expanded vs (distinct, multiplicity)
    mult = np.random.default_rng(2).integers(0, 4, S)
    a = ref.lfo_rows(ll, 9, [3, 9, 10, 5], block=2, multiplicity=mult)
    b = ref.lfo_rows(np.repeat(ll, mult, axis=0), 9, [3, 9, 10, 5], block=2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- a conjugate model: y_n ~ N(mu, sigma^2), mu ~ N(0, s0^2); exact posterior draws for every prefix ----
SIGMA, S0 = 1.0, 3.0


def _posterior(y):
    prec = 1.0 / S0 ** 2 + y.size / SIGMA ** 2
    return (y.sum() / SIGMA ** 2) / prec, 1.0 / prec


def _norm_logpdf(x, m, v):
    return -0.5 * math.log(2 * math.pi * v) - 0.5 * (x - m) ** 2 / v


def test_reference_with_refits_against_exact_lfo(par):
    N, L, S, thr, reps = 40, 4, 1000, 0.5, 24
    y = np.random.default_rng(11).normal(0.4, SIGMA, N)
    y[[9, 21]] += 4.0                                                  # two surprises: rows whose removal moves the posterior
    origins = np.arange(L, N)
    exact = sum(_norm_logpdf(y[i], *(lambda m, v: (m, v + SIGMA ** 2))(*_posterior(y[:i]))) for i in origins)

    def estimate(seed):
        def draws(n_rows):
            m, v = _posterior(y[:n_rows])
            mu = np.random.default_rng([seed, n_rows]).normal(m, math.sqrt(v), S)
            return -0.5 * math.log(2 * math.pi * SIGMA ** 2) - 0.5 * (y[None, :] - mu[:, None]) ** 2 / SIGMA ** 2
        return par.lfo_walk(origins, N, draws(N), lambda ll, n_fit, og: ref.lfo_rows(ll, n_fit, og), draws, k_threshold=thr)

    runs = [estimate(seed) for seed in range(reps)]
    est = np.array([r["elpd_lfo"].sum() for r in runs])
    se = est.std(ddof=1)                                               # the standard error of one estimate, measured here
    print(f"exact LFO {exact:.6f}; PSIS-LFO with refits: first {est[0]:.6f}, mean {est.mean():.6f}, se {se:.6f}; "
          f"refits {[r['n_refits'] for r in runs]}")
    first = runs[0]
    assert first["n_refits"] >= 1 and np.count_nonzero(~first["exact"]) >= 1
    assert np.array_equal(first["exact"], np.isin(origins, first["refit_origins"]))
    assert abs(est[0] - exact) <= 4.0 * se
    # exact LFO itself through the walk: a threshold nothing passes refits at every origin, and every origin is then scored
    # by uniform weights from draws of its own prefix -- Monte Carlo error only
    every = par.lfo_walk(origins, N, None, lambda ll, n_fit, og: dict(elpd_lfo=np.zeros(len(og)), khat=np.full(len(og), 9.0),
                                                                      tail_len=np.zeros(len(og), np.int64)),
                         lambda i: None, k_threshold=0.0)
    assert every["n_refits"] == origins.size and np.all(every["exact"])


# ---- the walk on scripted k-hat tables ----
def _scripted(table, default=0.1):
    calls = []

    def score(fit, n_fit, og):
        assert fit == n_fit                                            # the fit object here is its own n_fit
        calls.append((n_fit, tuple(og)))
        kh = np.array([math.inf if i == n_fit else table.get((n_fit, i), default) for i in og])
        return dict(elpd_lfo=np.array([-(1000.0 * n_fit + i) for i in og]), khat=kh, tail_len=np.array([7 * i for i in og]))
    return score, calls


@pytest.mark.parametrize("n_fit, origins", [(20, range(5, 20)), (5, range(5, 20)), (12, range(5, 20))])
def test_walk_follows_the_script(par, n_fit, origins):
    origins = list(origins)
    # k-hat grows with the distance from the fit and crosses 0.7 at distance 4; one origin is bad from anywhere
    table = {(f, i): 0.2 * abs(f - i) for f in range(0, 25) for i in range(0, 25)}
    table.update({(f, 16): 0.95 for f in range(0, 25)})
    score, calls = _scripted(table)
    out = par.lfo_walk(origins, n_fit, n_fit, score, lambda i: i, k_threshold=0.7)
    fit_exp, refits_exp = ref.walk_expected(origins, n_fit, lambda f, i: table[(f, i)], 0.7)
    assert np.array_equal(out["origins"], np.array(sorted(origins))) and np.array_equal(out["fit_origin"], fit_exp)
    assert out["refit_origins"] == refits_exp and out["n_refits"] == len(refits_exp) >= 2
    assert np.array_equal(out["exact"], out["fit_origin"] == out["origins"]) and not out["max_refits_hit"]
    # every value is the one the scoring fit gave for that origin
    assert np.array_equal(out["elpd_lfo"], -(1000.0 * out["fit_origin"] + out["origins"]))
    assert np.array_equal(out["tail_len"], 7 * out["origins"])
    assert np.all(np.isinf(out["khat"][out["exact"]])) and np.all(out["khat"][~out["exact"]] <= 0.7)
    # one call per fit and direction, each over all the origins still open
    assert len(calls) == len(refits_exp) + (1 if n_fit in (5, 20) else 2)
    if n_fit == 20:
        assert refits_exp[0] == 16 and calls[0] == (20, tuple(range(19, 4, -1)))       # backward: descending from the fit
    if n_fit == 5:
        assert refits_exp[0] == 9 and calls[0] == (5, tuple(range(5, 20)))            # forward; origin 5 itself is exact
        assert out["exact"][0] and out["fit_origin"][0] == 5


def test_walk_max_refits_and_no_refit(par):
    origins = list(range(5, 20))
    table = {(f, i): 0.2 * abs(f - i) for f in range(0, 25) for i in range(0, 25)}
    score, calls = _scripted(table)
    full = par.lfo_walk(origins, 20, 20, score, lambda i: i, k_threshold=0.7)
    assert full["refit_origins"] == [16, 12, 8]
    one = par.lfo_walk(origins, 20, 20, score, lambda i: i, k_threshold=0.7, max_refits=1)
    fit_exp, refits_exp = ref.walk_expected(origins, 20, lambda f, i: table[(f, i)], 0.7, max_refits=1)
    assert one["refit_origins"] == refits_exp == [16] and np.array_equal(one["fit_origin"], fit_exp) and one["max_refits_hit"]
    # the origins past the last allowed refit keep their high k-hat
    assert np.array_equal(one["khat"][one["origins"] < 12], 0.2 * (16 - one["origins"][one["origins"] < 12]))
    zero = par.lfo_walk(origins, 20, 20, score, lambda i: i, k_threshold=0.7, max_refits=0)
    none = par.lfo_walk(origins, 20, 20, score, None, k_threshold=0.7)
    for k in ("elpd_lfo", "khat", "fit_origin", "exact"):
        assert np.array_equal(zero[k], none[k]), k
    assert none["n_refits"] == 0 and np.all(none["fit_origin"] == 20) and not none["max_refits_hit"] and zero["max_refits_hit"]
    fit_exp, refits_exp = ref.walk_expected(origins, 20, lambda f, i: table[(f, i)], 0.7, refit=False)
    assert refits_exp == [] and np.array_equal(none["fit_origin"], fit_exp)
    # the origins scored from the first fit are the same with and without refits
    first = full["fit_origin"] == 20
    assert first.sum() == 3 and np.array_equal(full["elpd_lfo"][first], none["elpd_lfo"][first])
    # a tail too short to diagnose (k-hat +inf) away from the fit counts as above the threshold
    t2 = dict(table)
    t2[(20, 18)] = math.inf
    inf = par.lfo_walk(origins, 20, 20, _scripted(t2)[0], lambda i: i, k_threshold=0.7)
    fit_exp, refits_exp = ref.walk_expected(origins, 20, lambda f, i: t2[(f, i)], 0.7)
    assert inf["refit_origins"] == refits_exp and refits_exp[0] == 18 and np.array_equal(inf["fit_origin"], fit_exp)
    # repeats and any order of the origins give one entry each, ascending
    rep = par.lfo_walk([9, 7, 9, 19], 20, 20, score, None, k_threshold=0.7)
    assert rep["origins"].tolist() == [7, 9, 19]
    with pytest.raises(ValueError, match="no origin"):
        par.lfo_walk([], 20, 20, score, None, k_threshold=0.7)
    with pytest.raises(ValueError, match="max_refits"):
        par.lfo_walk(origins, 20, 20, score, None, k_threshold=0.7, max_refits=-1)


def test_origins_and_seed(par):
    assert par.lfo_origins(20, 20, 1).tolist() == list(range(10, 20))              # train: N // 2 .. N - 1
    assert par.lfo_origins(20, 20, 3, 5).tolist() == list(range(5, 18))
    assert par.lfo_origins(30, 20, 2).tolist() == list(range(20, 29))              # rows after the fit: the sequential score
    for kw, msg in ((dict(n_rows=20, n_fit=20, block=0), "block"), (dict(n_rows=20, n_fit=0, block=1), "n_fit"),
                    (dict(n_rows=20, n_fit=21, block=1), "n_fit"), (dict(n_rows=20, n_fit=20, block=1, min_train=0), "min_train"),
                    (dict(n_rows=20, n_fit=20, block=4, min_train=17), "leaves no origin")):
        with pytest.raises(ValueError, match=msg):
            par.lfo_origins(**kw)
    seeds = {par.lfo_refit_seed(4242, i) for i in range(100)} | {par.lfo_refit_seed(4243, 0)}
    assert len(seeds) == 101 and all(0 <= s < 1 << 64 for s in seeds) and 4242 not in seeds
    assert par.good_k(2400) == 0.7 and par.good_k(100) == 0.5


def _result(par, vals, origins, block=1):
    vals = np.asarray(vals, np.float64)
    n = vals.size
    return par.LeaveFutureOut(elpd_lfo=float(vals.sum()), se_elpd_lfo=par._se_total(vals), elpd_lfo_i=vals, khat=np.zeros(n),
                              tail_len=np.zeros(n, np.int64), origins=np.asarray(origins), fit_origin=np.zeros(n, np.int64),
                              exact=np.zeros(n, bool), refit_origins=[], n_refits=0, k_threshold=0.7, n_samples=100, block=block)


def test_elpd_compare_on_two_results(par):
    a = _result(par, [-1.0, -2.0, -1.5, -0.5], [4, 5, 6, 7])
    b = _result(par, [-1.5, -2.0, -2.5, -0.25], [4, 5, 6, 7])
    d = par.elpd_compare(a, b)
    diff = np.array([0.5, 0.0, 1.0, -0.25])
    assert d["elpd_lfo_diff"] == pytest.approx(diff.sum(), rel=1e-14)
    assert d["se_lfo_diff"] == pytest.approx(math.sqrt(4 * np.var(diff, ddof=1)), rel=1e-14)
    assert set(d) == {"elpd_lfo_diff", "se_lfo_diff"}
    with pytest.raises(ValueError, match="different origins"):
        par.elpd_compare(a, _result(par, [-1.0, -2.0, -1.5, -0.5], [4, 5, 6, 8]))
    with pytest.raises(ValueError, match="different origins"):
        par.elpd_compare(a, _result(par, [-1.0, -2.0, -1.5], [4, 5, 6]))
    with pytest.raises(ValueError, match="different blocks"):
        par.elpd_compare(a, _result(par, [-1.0, -2.0, -1.5, -0.5], [4, 5, 6, 7], block=2))
    z = np.zeros(4)
    pa = par.PredictiveAccuracy(*([0.0] * 8), z, z, z, z, 0.7, 0, None, 100, 100)
    for x, y in ((a, pa), (pa, a)):
        with pytest.raises(ValueError, match="one kind"):
            par.elpd_compare(x, y)
    assert par.elpd_compare(pa, pa)["elpd_loo_diff"] == 0.0                         # the LOO comparison is what it was


def test_entry_point_and_argument_checks(pt):
    """ptnn_lfo refuses bad specs before it looks at the handle (NULL here): no GPU needed."""
    from ptnn_amd import _lib
    lib = _lib.load_library()
    spec = _lib.LfoSpec()

    def err():
        assert lib.ptnn_lfo(None, C.byref(spec)) < 0
        return lib.ptnn_last_error().decode()

    assert "struct_bytes" in err()
    spec.struct_bytes = C.sizeof(_lib.LfoSpec)
    ll = np.full((8, 6), -1.0)
    og = np.array([2, 3], np.int32)
    spec.loglik, spec.n_w, spec.n_rows = ll.ctypes.data_as(C.POINTER(C.c_double)), 8, 6
    spec.origins, spec.n_origins, spec.n_fit, spec.block, spec.r_eff = og.ctypes.data_as(C.POINTER(C.c_int32)), 2, 6, 1, 0.0
    assert "r_eff" in err()
    spec.r_eff = 1.0
    spec.block = 0
    assert "block = 0" in err()
    spec.block = 1
    for bad in (0, 7):
        spec.n_fit = bad
        assert f"n_fit = {bad}" in err()
    spec.n_fit = 6
    spec.n_origins = 0
    assert "n_origins = 0" in err()
    spec.n_origins = 2
    for bad in (0, 6, -1):
        og[1] = bad
        assert f"origin {bad} (origins[1])" in err()
    og[1] = 4
    spec.block = 3
    assert "i + block > n_rows" in err()
    spec.block = 1
    ll[5, 2] = math.nan
    assert "loglik[5, 2]" in err()
    ll[5, 2] = -1.0
    lo = np.empty((8, 6))
    spec.loglik_out = lo.ctypes.data_as(C.POINTER(C.c_double))
    assert "loglik_out" in err()
    spec.loglik_out = None
    w = np.zeros((8, 3), np.float32)
    spec.w = w.ctypes.data_as(C.POINTER(C.c_float))
    assert "not both" in err()
    spec.w = None
    assert "null" in err().lower() or "handle" in err().lower()                    # every argument check passed: the handle is next
