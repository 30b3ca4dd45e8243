"""Case influence without a GPU: the reference of the GPU tests (tests/influence_ref.py) against its np.longdouble variant inside
the bound of DESIGN.md section 30; what the covariance means, on exact posterior draws of a conjugate Gaussian linear model
(the closed form and the exact refit without a row); the host helpers of influence.py; the binding and the argument checks of
ptnn_influence that need no device."""
import ctypes as C

import numpy as np
import pytest

import influence_ref as ref
import test_analysis_front_cpu as front  # noqa: F401  (puts the package on the path)

from ptnn_amd import _lib, influence


# ---- the reference against its longdouble variant
@pytest.mark.parametrize("S, n_a, n_b, seed", [(2, 1, 1, 0), (65, 3, 70, 1), (1000, 7, 5, 2), (5000, 2, 33, 3)])
def test_reference_stays_inside_the_bound_of_its_longdouble_variant(S, n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((S, n_a)) * rng.uniform(0.1, 30, n_a) + rng.uniform(-50, 50, n_a)).astype(np.float32)
    B = rng.standard_normal((S, n_b)) * rng.uniform(0.01, 5, n_b) - rng.uniform(0, 40, n_b)
    B[:, 0] += 0.5 * A[:, 0]
    mult = rng.integers(0, 4, S)
    mult[0], mult[-1] = 1, 2
    got, want = ref.influence(A, B, mult), ref.influence_longdouble(A, B, mult)
    assert got["n_samples"] == want["n_samples"] == int(mult.sum())
    s_a, s_b = np.sqrt(want["target_var"].astype(np.float64)), np.sqrt(want["case_var"].astype(np.float64))
    share = np.abs(got["cov"] - want["cov"]).astype(np.float64) / ref.tol(S, s_a, s_b)
    print(f"S = {S}: largest |float64 - longdouble| as a share of the bound {share.max():.3g}")
    assert share.max() <= 1.0
    assert np.max(np.abs(got["target_var"] - want["target_var"]) / np.diag(ref.tol(S, s_a, s_a))) <= 1.0
    assert np.max(np.abs(got["case_var"] - want["case_var"]) / np.diag(ref.tol(S, s_b, s_b))) <= 1.0
    assert np.max(np.abs(got["target_mean"] - want["target_mean"]) / (16 * (S + 64) * 2.0 ** -53 * np.maximum(s_a, np.abs(want["target_mean"])))) <= 1.0
    # expanded samples and (distinct, multiplicity) describe one multiset
    rep = ref.influence(np.repeat(A, mult, axis=0), np.repeat(B, mult, axis=0))
    assert np.max(np.abs(rep["cov"] - got["cov"]) / ref.tol(int(mult.sum()), s_a, s_b)) <= 1.0


# ---- the meaning: a conjugate Gaussian linear model
N, D, SIGMA, PRIOR_VAR, S_DRAWS, N_TARGETS = 60, 3, 0.1, 25.0, 200_000, 5


def _posterior(X, y):
    C_ = np.linalg.inv(X.T @ X / SIGMA ** 2 + np.eye(D) / PRIOR_VAR)
    return C_, C_ @ X.T @ y / SIGMA ** 2


@pytest.fixture(scope="module")
def linear():
    rng = np.random.default_rng(20260)
    X = rng.standard_normal((N, D))
    y = X @ np.array([0.7, -0.4, 0.2]) + SIGMA * rng.standard_normal(N)
    y[7] += 0.6                                                # an outlier
    Xt = rng.standard_normal((N_TARGETS, D))
    C_, mu = _posterior(X, y)
    theta = mu + rng.standard_normal((S_DRAWS, D)) @ np.linalg.cholesky(C_).T
    f = theta @ Xt.T                                           # [S, n_targets]
    ll = -0.5 * np.log(2 * np.pi * SIGMA ** 2) - 0.5 * (y - theta @ X.T) ** 2 / SIGMA ** 2     # [S, N]
    return X, y, Xt, C_, mu, ref.influence(f, ll)


def test_covariance_matches_the_closed_form(linear):
    X, y, Xt, C_, mu, r = linear
    exact = (Xt @ C_ @ X.T) * ((y - X @ mu) / SIGMA ** 2)     # x_j' C x_i (y_i - x_i' mu) / sigma^2
    s2 = np.multiply.outer(r["target_var"], r["case_var"])
    se = np.sqrt((s2 + r["cov"] ** 2) / S_DRAWS)
    dev = np.abs(r["cov"] - exact) / se
    print(f"largest |cov - closed form| over {exact.size} elements: {dev.max():.2f} standard errors (bound 8)")
    assert exact.size == 300 and dev.max() <= 8.0


def test_deletion_shift_follows_the_exact_refit(linear):
    X, y, Xt, C_, mu, r = linear
    lev = np.einsum("ij,jk,ik->i", X, C_, X) / SIGMA ** 2
    refit = np.empty((N_TARGETS, N))
    for i in range(N):
        keep = np.arange(N) != i
        refit[:, i] = Xt @ (_posterior(X[keep], y[keep])[1] - mu)
    shift = 0.0 - r["cov"]
    corr = np.corrcoef(shift.ravel(), refit.ravel())[0, 1]
    gap = np.max(np.abs(shift - refit) / np.sqrt(r["target_var"])[:, None])
    print(f"leverage <= {lev.max():.3f}; corr(deletion_shift, exact refit shift) = {corr:.4f}; largest gap {gap:.3f} posterior sd")
    assert corr > 0.99


# ---- the host helpers
def _result(cov, t_var, c_var, shape, top=3):
    cov = np.asarray(cov, dtype=np.float64)
    return influence.finish_influence(cov, np.zeros(cov.shape[0]), np.asarray(t_var, float), np.zeros(cov.shape[1]), np.asarray(c_var, float),
                                      shape, top, 10, 7)


def test_top_cases_tie_rule_and_clipping():
    cov = np.array([[1.0, -3.0, 3.0, 0.5, -3.0], [0.0, 0.0, 0.0, 0.0, 0.0], [-1.0, 2.0, -2.0, 1.0, 0.0]])
    idx, shift = influence.top_cases(cov, 3)
    assert idx.dtype == np.int64 and idx.tolist() == [[1, 2, 4], [0, 1, 2], [1, 2, 0]]
    assert np.array_equal(shift, np.array([[3.0, -3.0, 3.0], [0.0, 0.0, 0.0], [-2.0, 2.0, 1.0]]))
    assert np.array_equal(idx, ref.top_cases(cov, 3))
    idx, shift = influence.top_cases(cov, 9)                   # clipped to the five cases
    assert idx.shape == shift.shape == (3, 5) and np.array_equal(idx, ref.top_cases(cov, 9))
    rng = np.random.default_rng(5)
    c3 = rng.integers(-3, 4, (4, 2, 11)).astype(np.float64)    # many ties, a target axis more
    assert np.array_equal(influence.top_cases(c3, 4)[0], ref.top_cases(c3, 4))


def test_result_arithmetic_nan_handling_and_flags():
    cov = np.array([[0.5, -1.0, 0.0, 2.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, -4.0]])
    r = _result(cov, [4.0, 0.0, 16.0], [1.0, 0.25, 0.0, 4.0], (3,), top=2)
    assert r.cov.shape == (3, 4) and np.array_equal(r.deletion_shift, 0.0 - cov) and np.array_equal(r.target_sd, [2.0, 0.0, 4.0])
    want = np.array([[0.25, -1.0, np.nan, 0.5], [np.nan] * 4, [0.25, 0.5, np.nan, -0.5]])
    assert np.array_equal(r.corr, want, equal_nan=True)
    assert np.array_equal(r.deletion_z, np.array([[-0.25, 0.5, 0.0, -1.0], [np.nan] * 4, [-0.25, -0.25, 0.0, 1.0]]), equal_nan=True)
    # case_importance: the mean of |corr| over the columns that have one; NaN where none has
    assert np.array_equal(r.case_importance, [0.25, 0.75, np.nan, 0.5], equal_nan=True)
    assert r.top_cases.tolist() == [[3, 1], [0, 1], [3, 0]] and np.array_equal(r.top_shift, [[-2.0, 1.0], [0.0, 0.0], [4.0, -1.0]])
    assert (r.n_samples, r.n_distinct) == (10, 7)
    assert influence.influence_flagged(r).tolist() == [[0, 1], [0, 3], [2, 3]] and influence.influence_flagged(r).dtype == np.int64
    assert influence.influence_flagged(r, z=0.25).tolist() == [[0, 0], [0, 1], [0, 3], [2, 0], [2, 1], [2, 3]]
    assert influence.influence_flagged(r, z=1.5).shape == (0, 2)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="z = "):
            influence.influence_flagged(r, z=bad)
    # with the output axis: [n_x, n_out, n_cases]
    r2 = _result(np.arange(24.0).reshape(6, 4), np.ones(6), np.ones(4), (3, 2))
    assert r2.cov.shape == (3, 2, 4) and r2.top_cases.shape == (3, 2, 3) and r2.target_sd.shape == (3, 2)
    assert influence.influence_flagged(r2, z=22.0).tolist() == [[2, 1, 2], [2, 1, 3]]
    assert np.array_equal(r2.case_importance, np.arange(24.0).reshape(6, 4).mean(axis=0))


# ---- the binding
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd.load_library()


def _spec(**kw):
    s = _lib.InfluenceSpec()
    s.struct_bytes = C.sizeof(_lib.InfluenceSpec)
    s.thin, s.nsteps, s.n_cases, s.case_source, s.n_targets, s.target_source = 1, 10, 4, _lib.PREDICT_X_TRAIN, 3, _lib.PREDICT_X_TEST
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_influence(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device(lib):
    assert "ptnn_influence" in _lib.SYMBOLS and lib.ptnn_influence is not None
    assert lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4
    rc, msg = _err(lib, None)
    assert rc == -1 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc == -1 and f"expected {C.sizeof(_lib.InfluenceSpec)}" in msg
    f4 = np.zeros((3, 2), np.float32)
    f4p = f4.ctypes.data_as(C.POINTER(C.c_float))
    ll = np.zeros((3, 2))
    ll[2, 1] = np.inf
    llp = ll.ctypes.data_as(C.POINTER(C.c_double))
    ok = np.zeros((3, 2))
    okp = ok.ctypes.data_as(C.POINTER(C.c_double))
    mu = np.array([1, 0, 0], np.int32)
    mup = mu.ctypes.data_as(C.POINTER(C.c_int32))
    neg = np.array([1, -1, 2], np.int32)
    negp = neg.ctypes.data_as(C.POINTER(C.c_int32))
    mat = dict(target_values=f4p, loglik=okp, n_w=3, n_a=2, n_b=2, nsteps=0)
    for kw, word in ((dict(thin=0), "thin"), (dict(nsteps=0), "no source"), (dict(target_kind=2), "target_kind = 2"),
                     (dict(case_source=7), "case_source = 7"), (dict(target_source=9), "target_source = 9"),
                     (dict(case_source=_lib.PREDICT_X_HOST), "needs case_x"), (dict(target_source=_lib.PREDICT_X_HOST), "needs target_x"),
                     (dict(n_cases=0), "n_cases = 0"), (dict(n_targets=0), "n_targets = 0"), (dict(w=f4p, n_w=0), "n_w = 0"),
                     (dict(target_values=f4p), "come together"), (dict(loglik=okp), "come together"),
                     (dict(mat, w=f4p), "not both"), (dict(mat, n_a=0), "n_a = 0"), (dict(mat, n_b=0), "n_b = 0"),
                     (dict(mat, n_w=0), "n_w = 0"), (dict(mat, n_a=1 << 14, n_b=(1 << 13) + 1), "at most 2^27 elements"),
                     (dict(mat, multiplicity=negp), "multiplicity[1] = -1"), (dict(mat, loglik=llp), "loglik[2, 1] = inf is not finite")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # the order of adjacent checks: the matrices, the source, the kind, the rows, the counts, the host values
    for kw, word in ((dict(target_values=f4p, thin=0), "come together"), (dict(thin=0, target_kind=2), "thin"),
                     (dict(target_kind=2, case_source=7), "target_kind"), (dict(case_source=7, target_source=9), "case_source"),
                     (dict(target_source=9, n_cases=0), "target_source"), (dict(mat, n_a=0, loglik=llp), "n_a = 0"),
                     (dict(mat, multiplicity=negp, loglik=llp), "multiplicity")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # a consistent request reaches the handle check (M < 2 is the handle's selection rule, as ptnn_elpd's)
    for kw in ({}, dict(target_kind=_lib.INFLUENCE_LOGLIK), mat, dict(mat, multiplicity=mup), dict(w=f4p, n_w=1, nsteps=0)):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and "null handle" in msg, (kw, msg)
    assert _lib.INFLUENCE_KCHUNK == 512 and _lib.INFLUENCE_MAX_ELEMENTS == 2 ** 27
