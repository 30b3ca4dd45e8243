"""Posterior predictive checks, host side (no GPU): the float64 oracle's statistics against independently written forms, the
host arithmetic of predictive_check (names, p-values, flagging), the binding, the argument checks that run before anything
touches a device, and the known-answer pair through the oracle alone."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import pytest

import ppc_ref as ref


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def test_draws_follow_the_counter_layout():
    from ptnn_amd import philox
    assert philox.STREAM_PPC == 6
    seed, i, N = 77, 5, 11
    z, u = ref.normals(seed, i, N), ref.uniforms(seed, i, N)
    assert z.shape == u.shape == (N,)
    for n in range(N):
        x = philox.philox4x32(n // 4, i, 0, 6, seed)
        assert u[n] == philox.uniform23(x[n % 4])
        u1, u2 = philox.uniform23(x[2 * ((n % 4) // 2)]), philox.uniform23(x[2 * ((n % 4) // 2) + 1])
        r, t = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        assert z[n] == pytest.approx(r * (np.cos(t) if n % 2 == 0 else np.sin(t)), rel=1e-14)
    assert np.all((u > 0) & (u < 1)) and np.array_equal(u, u.astype(np.float32).astype(np.float64))     # exact in fp32
    assert not np.array_equal(ref.normals(seed, i + 1, N), z) and not np.array_equal(ref.normals(seed + 1, i, N), z)


def test_regression_statistics_against_independent_forms():
    rng = np.random.default_rng(3)
    N, lags = 57, (1, 2, 7, 30, 56)
    f = rng.normal(0.5, 0.1, (3, N))
    eta = np.array([-3.0, -4.5, -2.0])
    y = rng.normal(0.5, 0.2, N)
    z = rng.standard_normal((3, N))
    t_obs, t_rep = ref.regression(f, eta, y, z, lags)
    assert t_obs.shape == t_rep.shape == (3, 7 + len(lags))
    for i in range(3):
        tau = np.exp(eta[i] / 2)
        for series, resid, t in ((y, (y - f[i]) / tau, t_obs[i]), (f[i] + tau * z[i], z[i], t_rep[i])):
            assert t[0] == pytest.approx(series.sum() / N) and t[1] == pytest.approx(np.sqrt(np.mean(series ** 2) - np.mean(series) ** 2))
            assert t[2] == series.min() and t[3] == series.max()
            assert t[4] == pytest.approx(float(resid @ resid)) and t[5] == np.abs(resid).max()
            c = resid - resid.mean()
            full = np.correlate(c, c, mode="full")[N - 1:]              # autocovariance sums at lags 0 .. N - 1
            r = full / full[0]
            for j, k in enumerate(lags):
                assert t[7 + j] == pytest.approx(r[k], rel=1e-12, abs=1e-15)
            assert t[6] == pytest.approx(N * (N + 2) * sum(r[k] ** 2 / (N - k) for k in lags), rel=1e-12)
    # data-level statistics do not depend on the sample
    assert np.all(t_obs[:, :4] == t_obs[0, :4])
    # a white series has a small Ljung-Box statistic, a trending one a large one
    white, trend = rng.standard_normal(400), np.linspace(-1, 1, 400)
    assert ref.resid_stats(white, (1, 2, 3))[2] < 20 < ref.resid_stats(trend, (1, 2, 3))[2]


def test_classification_statistics_against_independent_forms():
    rng = np.random.default_rng(4)
    N, O = 41, 3
    p = rng.dirichlet(np.ones(O), (2, N)).astype(np.float32).astype(np.float64)
    y = rng.integers(0, O, N)
    u = np.stack([ref.uniforms(9, i, N) for i in range(2)])
    t_obs, t_rep, y_rep = ref.classification(p, y, u)
    assert t_obs.shape == (2, 2 + O) and y_rep.shape == (2, N)
    for i in range(2):
        # inverse-cdf draw, written row by row
        for n in range(N):
            tot, cum, k = sum(p[i, n]), 0.0, O - 1
            for j in range(O):
                cum += p[i, n, j]
                if cum > u[i, n] * tot:
                    k = j
                    break
            assert y_rep[i, n] == k
        for lab, t in ((y, t_obs[i]), (y_rep[i], t_rep[i])):
            assert np.array_equal(t[2:], np.bincount(lab, minlength=O))
            assert t[0] == pytest.approx(-2.0 * sum(np.log(p[i, n, lab[n]]) for n in range(N)))
            assert t[1] == pytest.approx(sum(int(np.argmax(p[i, n]) == lab[n]) for n in range(N)) / N)
    # u just below / above a cumulative edge; no class satisfies the rule only when the sum rounds: then the last class
    assert list(ref.draw_classes([[0.25, 0.25, 0.5]] * 3, [0.2, 0.25, 0.9999999])) == [0, 1, 2]
    assert list(ref.draw_classes([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], [0.5, 0.5])) == [0, 2]
    # the draws follow p: class frequencies of many draws
    big = ref.draw_classes(np.tile([[0.2, 0.5, 0.3]], (40000, 1)), np.concatenate([ref.uniforms(1, i, 4000) for i in range(10)]))
    np.testing.assert_allclose(np.bincount(big) / 40000, [0.2, 0.5, 0.3], atol=0.01)


def test_reduction_and_host_p_values(pt):
    from ptnn_amd.parallel_tempering import PredictiveCheck, ppc_flagged, ppc_p_values, ppc_stat_names
    from ptnn_amd import _lib
    nan, inf = float("nan"), float("inf")
    t_obs = np.array([[1.0, 2.0, 0.0], [1.0, nan, 0.0], [1.0, 2.0, 0.0], [1.0, 2.0, 0.0]])
    t_rep = np.array([[2.0, 1.0, 0.0], [1.0, 5.0, inf], [0.0, 3.0, 0.0], [1.0, 4.0, 1.0]])
    r = ref.reduce(t_obs, t_rep)
    assert list(r["n_defined"]) == [4, 3, 3] and list(r["n_greater"]) == [1, 2, 1] and list(r["n_equal"]) == [2, 0, 2]
    # ties count half; the undefined occurrence is left out of the counts and of the moments
    assert list(r["p_value"]) == [0.5, 2 / 3, (1 + 1.0) / 3]
    assert r["mean_rep"][1] == pytest.approx(8 / 3) and r["var_rep"][1] == pytest.approx(np.var([1.0, 3.0, 4.0]))
    assert r["mean_obs"][1] == 2.0 and r["mean_rep"][2] == pytest.approx(1 / 3)
    p = ppc_p_values(r["n_greater"], r["n_equal"], r["n_defined"])
    assert np.array_equal(p, r["p_value"])
    assert np.isnan(ppc_p_values([0], [0], [0])[0])
    # names
    assert ppc_stat_names(_lib.TASK_REG, lags=(1, 3)) == ["mean", "sd", "min", "max", "chi2", "max_abs_resid", "ljung_box",
                                                         "resid_acf[1]", "resid_acf[3]"]
    assert ppc_stat_names(_lib.TASK_CLS, n_out=3) == ["deviance", "accuracy", "class_count[0]", "class_count[1]", "class_count[2]"]
    # flagging: outside [alpha / 2, 1 - alpha / 2]; nan is not flagged
    names = ["a", "b", "c", "d", "e"]
    chk = PredictiveCheck(names=names, p_value=dict(zip(names, [0.024, 0.025, 0.5, 0.9751, nan])), t_obs_mean=None, t_rep_mean=None,
                          t_rep_sd=None, n_defined=None, t_obs=None, t_rep=None, n_samples=0, n_distinct=0)
    assert ppc_flagged(chk) == ["a", "d"] and ppc_flagged(chk, alpha=0.01) == [] and ppc_flagged(chk, alpha=0.9) == ["a", "b", "d"]
    with pytest.raises(ValueError, match="alpha"):
        ppc_flagged(chk, alpha=1.0)


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.PpcSpec()
    s.struct_bytes = C.sizeof(_lib.PpcSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source = 1, 10, 8, _lib.PREDICT_X_TRAIN
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_ppc(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_binding_and_entry_point_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert "ptnn_ppc" in _lib.SYMBOLS and lib.ptnn_ppc is not None and lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4
    # the struct of include/ptnn.h on LP64: the trace source (32 bytes), the host source (32), the data (16), lags and seed (24),
    # 12 output pointers; the library reports its own sizeof below
    assert C.sizeof(_lib.PpcSpec) == 32 + 32 + 16 + 24 + 96 and _lib.PpcSpec.seed.offset % 8 == 0 and _lib.PPC_MAX_LAGS == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptnn.h")).read()
    assert "int ptnn_ppc(ptnn_handle *h, const ptnn_ppc_spec *spec);" in header and "#define PTNN_PPC_MAX_LAGS 16" in header
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc < 0 and f"expected {C.sizeof(_lib.PpcSpec)}" in msg
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    ip = C.POINTER(C.c_int32)

    def lags(v):
        a = np.array(v, np.int32)
        return dict(lags=a.ctypes.data_as(ip), n_lags=len(v)), a

    for kw, word in ((dict(nsteps=0), "no source"), (dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(n_rows=1), "at least 2"),
                     (dict(n_lags=17), "n_lags"), (dict(n_lags=2), "lags is NULL")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and word in msg, (kw, msg)
    for bad, word in (([0, 1], "outside"), ([1, 8], "outside"), ([2, 3, 2], "once"), ([-1], "outside")):
        kw, keep = lags(bad)
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and word in msg, (bad, msg)
    mu = np.array([1, -1], np.int32)
    w = np.zeros(8, np.float32)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(C.POINTER(C.c_float)), n_w=2, multiplicity=mu.ctypes.data_as(ip)))
    assert rc < 0 and "negative" in msg
    kw, keep = lags([1, 7])
    rc, msg = _err(lib, _spec(**kw))                                # a consistent request reaches the handle check
    assert rc < 0 and "null handle" in msg


def test_public_call_validates_before_it_needs_a_device(pt, tmp_path):
    from ptnn_amd.parallel_tempering import ppc_check_lags
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    import parity
    d = parity.datasets()
    obj = ParallelTempering(True, 0.1, d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 4, 2, 4 * 50, 10, 0.5, str(tmp_path),
                            seed=1, write_files=False)
    for bad, word in (((0, 1), "lie in"), ((1, 1), "distinct"), (tuple(range(1, 18)), "at most 16"), ((1.5,), "integers"),
                      ((len(d["sunspot_test"]),), "lie in")):
        with pytest.raises(ValueError, match=word):
            obj.predictive_check("test", lags=bad)
    assert ppc_check_lags((3, 1), 5) == [3, 1]
    with pytest.raises(ValueError, match="eta"):
        obj.predictive_check("test", weights=np.zeros((3, obj.num_param), np.float32))
    with pytest.raises(ValueError, match="data must be"):
        obj.predictive_check("validation")
    with pytest.raises(ValueError, match="at least 2"):
        obj.predictive_check(d["sunspot_test"][:1])
    with pytest.raises(ValueError, match="run_chains"):
        obj.predictive_check("test")                               # no handle yet: before initialize_chains() / run_chains()


def test_known_answer_pair_through_the_oracle():
    """One vector with constant output f repeated M = 2000 times on N = 300 rows, y = f + tau noise (ppc_ref.known_noise; numpy
    default_rng seeds 105 for the iid case and 202 for the AR(1) case with rho = 0.8; Philox key 20260101 for the replicates).
    The seeds were chosen so that the iid case is well inside the bounds: of the seeds 101 .. 108 tried, all but 101 gave
    p-values inside [0.01, 0.99]; 105 gives [0.12, 0.86]."""
    Check = namedtuple("Check", "names p_value")
    from ptnn_amd.parallel_tempering import ppc_flagged
    f0, tau = 0.5, np.exp(0.5 * ref.KNOWN_ETA)
    out = {}
    for case in ("iid", "ar1"):
        y = (f0 + tau * ref.known_noise(case)).astype(np.float32).astype(np.float64)
        names, r = ref.check_regression(np.full((1, ref.KNOWN_N), f0), [ref.KNOWN_ETA], [ref.KNOWN_M], y, ref.KNOWN_LAGS, ref.KNOWN_DRAW_SEED)
        assert np.all(r["n_defined"] == ref.KNOWN_M)
        out[case] = Check(names, dict(zip(names, r["p_value"])))
        print(case, {k: round(float(v), 4) for k, v in out[case].p_value.items()})
    assert out["ar1"].p_value["resid_acf[1]"] <= 0.01 and "ljung_box" in ppc_flagged(out["ar1"])
    assert all(0.005 <= p <= 0.995 for p in out["iid"].p_value.values()), out["iid"].p_value
    assert ppc_flagged(out["iid"]) == []
