"""Posterior predictive checks on the GPU (ptnn_ppc / predictive_check): the draws against philox.py, the reduction over the
rows against the float64 oracle (tests/ppc_ref.py) fed the device's own outputs, eta and draws, the reduction over the
occurrences against numpy on the returned samples, bitwise agreement between sources, block sizes and selections, consistency
with the existing analysis calls, the known-answer pair, and the refusals."""
import numpy as np
import pytest

import parity
import ppc_ref as ref
from parity import orc
from test_gpu_elpd import _pt, _runs

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0006
LAGS = (1, 2, 3, 4, 5, 11)
KEYS = ("n_defined", "n_greater", "n_equal", "mean_obs", "mean_rep", "var_rep", "t_obs", "t_rep")


def _low(pt, data, *, lags=(), seed=SEED, draws=True, burn_in=None, chains="all", thin=1, weights=None, eta=None):
    """The binding's call with the draws, on the selection predictive_check() would make."""
    I = int(pt.topology[0])
    ds = data if isinstance(data, str) else np.ascontiguousarray(np.asarray(data)[:, :I + 1], dtype=np.float32)
    if weights is not None:
        w, mult = pt._weights(weights)
        kw = dict(w=w, eta=eta, multiplicity=mult)
    else:
        kw, _ = pt._trace_selection(burn_in, chains, thin)
    return pt._sampler.ppc(ds, lags=lags, seed=seed, samples=True, draws=draws, **kw)


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["n_samples"] == b["n_samples"]


def _worst(name, got, want, rtol, atol):
    err = np.abs(got - want)
    k = np.unravel_index(int(np.argmax(err - rtol * np.abs(want))), err.shape)
    print(f"{name}: max abs diff {err.max():.3e}, max rel diff {np.max(err / np.maximum(np.abs(want), 1e-300)):.3e} "
          f"(at {k}: {got[k]!r} vs {want[k]!r})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=name)


def check_occurrences(out):
    """Check 3: the reduction over the occurrences against counts and numpy moments taken from the returned t_obs / t_rep."""
    r = ref.reduce(out["t_obs"], out["t_rep"])
    for k in ("n_defined", "n_greater", "n_equal"):
        assert np.array_equal(out[k], r[k]), k
    np.testing.assert_allclose(out["mean_obs"], r["mean_obs"], rtol=1e-12)
    np.testing.assert_allclose(out["mean_rep"], r["mean_rep"], rtol=1e-12)
    np.testing.assert_allclose(np.sqrt(out["var_rep"]), np.sqrt(r["var_rep"]), rtol=1e-12)


def check_regression(pt, data, y, eta, lags, seed=SEED, **sel):
    """Checks 1-3 of a regression: out = the device's call with draws; f = the device's own outputs of the same occurrences."""
    out = _low(pt, data, lags=lags, seed=seed, **sel)
    f = pt.posterior_predictive(data, return_samples=True, **sel).samples[:, :, 0]
    M, N = f.shape
    assert out["n_samples"] == M == len(eta) and out["z"].shape == (M, N) and out["t_rep"].shape == (M, 7 + len(lags))
    want_z = np.stack([ref.normals(seed, i, N) for i in range(M)])
    err = np.abs(out["z"] - want_z)
    print(f"z: max abs diff {err.max():.3e}, max rel diff {np.max(err / np.maximum(np.abs(want_z), 1e-30)):.3e}")
    np.testing.assert_allclose(out["z"], want_z, rtol=1e-4, atol=2e-6)            # test_gpu_forecast.py::test_noise's bound
    t_obs, t_rep = ref.regression(f, np.asarray(eta, np.float32), y, out["z"], lags)
    _worst("t_obs", out["t_obs"], t_obs, 1e-9, 1e-10)
    _worst("t_rep", out["t_rep"], t_rep, 1e-9, 1e-10)
    check_occurrences(out)
    return out, f


def check_classification(pt, data, y, seed=SEED, **sel):
    """Checks 1-3 of a classification: y_rep equals the oracle's draw from the device's own p and the exact u."""
    out = _low(pt, data, seed=seed, **sel)
    p = pt.posterior_predictive(data, return_samples=True, **sel).samples
    M, N, O = p.shape
    assert out["n_samples"] == M and out["y_rep"].shape == (M, N) and out["t_rep"].shape == (M, 2 + O) and out["z"] is None
    u = np.stack([ref.uniforms(seed, i, N) for i in range(M)])
    t_obs, t_rep, y_rep = ref.classification(p, y, u)
    assert np.array_equal(out["y_rep"], y_rep)
    _worst("t_obs", out["t_obs"], t_obs, 1e-9, 1e-10)
    _worst("t_rep", out["t_rep"], t_rep, 1e-9, 1e-10)
    check_occurrences(out)
    # the draws follow p: the mean replicated class counts against the summed probabilities
    np.testing.assert_allclose(out["mean_rep"][2:], p.astype(np.float64).sum(axis=1).mean(axis=0), rtol=0.05, atol=1.0)
    return out, p


def _targets(rows, col):
    return np.asarray(rows)[:, col].astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)                     # chain-major, as the columns of res[0]
    return pt, res, d, eta


def test_regression_sunspot(sunspot):
    """Checks 1, 2, 3 and 5 on train and test."""
    pt, res, d, eta = sunspot
    _, _, c = _runs(res[0].T, eta)
    for data in ("train", "test"):
        y = _targets(d["sunspot_" + data], 4)
        out, f = check_regression(pt, data, y, eta, LAGS)
        assert out["n_samples"] == 8 * 300 and out["n_distinct"] == len(c) < out["n_samples"]
        # the existing calls: chi2 on the data from posterior_predictive's samples; the data-level statistics from the targets
        tau = np.exp(0.5 * eta.astype(np.float32).astype(np.float64))
        np.testing.assert_allclose(out["t_obs"][:, 4], np.sum(((y[None, :] - f) / tau[:, None]) ** 2, axis=1), rtol=1e-9)
        np.testing.assert_allclose(out["mean_obs"][:4], [y.mean(), y.std(), y.min(), y.max()], rtol=1e-13)
        assert np.all(out["t_obs"][:, :4] == out["t_obs"][0, :4])
        # the public call: the same numbers by name
        chk = pt.predictive_check(data, lags=LAGS, seed=SEED, return_samples=True)
        assert chk.names[:7] == list(ref.REG_FIXED) and chk.names[7:] == [f"resid_acf[{k}]" for k in LAGS]
        assert np.array_equal(chk.t_rep, out["t_rep"]) and np.array_equal(chk.t_obs, out["t_obs"])
        r = ref.reduce(out["t_obs"], out["t_rep"])
        for j, n in enumerate(chk.names):
            assert chk.p_value[n] == r["p_value"][j] and chk.n_defined[n] == 2400 and chk.t_rep_sd[n] == np.sqrt(out["var_rep"][j])
        print(data, {n: round(v, 4) for n, v in chk.p_value.items()})
        slim = pt.predictive_check(data, lags=LAGS, seed=SEED)
        assert slim.t_obs is None and slim.t_rep is None and slim.p_value == chk.p_value
    # the seed defaults to the object's
    assert pt.predictive_check("test").p_value == pt.predictive_check("test", seed=pt.seed).p_value


def test_sources_blocks_and_selections_agree(sunspot, monkeypatch):
    pt, res, d, eta = sunspot
    base = _low(pt, "train", lags=LAGS)
    _same(_low(pt, "train", lags=LAGS, weights=res[0].T, eta=eta), base)
    w, e, c = _runs(res[0].T, eta)
    alt = _low(pt, "train", lags=LAGS, weights=(w, c), eta=e)
    _same(alt, base)
    assert np.array_equal(alt["z"], base["z"]) and alt["n_distinct"] == base["n_distinct"]
    # several blocks of distinct vectors: one vector per block, seven, all but one
    N = len(d["sunspot_train"])
    for vectors in (0, 7, base["n_distinct"] - 1):
        monkeypatch.setenv("PTNN_PPC_SCRATCH_BYTES", str(max(1, 4 * N * vectors)))
        _same(_low(pt, "train", lags=LAGS), base)
        _same(_low(pt, "train", lags=LAGS, weights=(w, c), eta=e), base)
    monkeypatch.delenv("PTNN_PPC_SCRATCH_BYTES")
    # the same seed twice; another seed changes the replicates and not the data's side
    _same(_low(pt, "train", lags=LAGS), base)
    other = _low(pt, "train", lags=LAGS, seed=SEED + 1)
    assert np.array_equal(other["t_obs"], base["t_obs"]) and not np.array_equal(other["t_rep"], base["t_rep"])
    assert np.array_equal(other["mean_obs"], base["mean_obs"])
    # the lag list's order only permutes the acf columns
    rev = _low(pt, "train", lags=LAGS[::-1])
    assert np.array_equal(rev["t_rep"][:, 7:], base["t_rep"][:, 7:][:, ::-1]) and np.array_equal(rev["t_rep"][:, :6], base["t_rep"][:, :6])
    # selections: the cold chain, a chain list, thinning -- trace vs the same vectors as weights=
    R = 8
    et = pt._sampler.eta_trace()
    cols = res[0].T.reshape(R, 300, -1)
    cold = int(np.argmin(pt.temperatures))
    yte = _targets(d["sunspot_test"], 4)
    for kw, sel_w, sel_e in ((dict(chains="cold"), cols[cold], et[cold, 300:]),
                             (dict(chains=[1, 6]), cols[[1, 6]].reshape(-1, cols.shape[2]), et[[1, 6], 300:].reshape(-1)),
                             (dict(thin=3), cols[:, ::3].reshape(-1, cols.shape[2]), et[:, 300::3].reshape(-1)),
                             (dict(chains=[2], burn_in=0.9), cols[2, 240:], et[2, 540:])):
        a = _low(pt, "test", lags=LAGS, **kw)
        b = _low(pt, "test", lags=LAGS, weights=sel_w, eta=sel_e)
        _same(a, b)
        assert a["n_distinct"] == b["n_distinct"] and a["n_samples"] == len(sel_e)
        print(kw, "n_distinct", a["n_distinct"])
        check_regression(pt, "test", yte, sel_e, LAGS, **kw)


def test_classification_iris(tmp_path):
    d = parity.datasets()
    pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    for data in ("train", "test"):
        y = d["iris_" + data][:, 4].astype(np.int64)
        out, p = check_classification(pt, data, y)
        assert out["n_samples"] == 8 * 200
        np.testing.assert_allclose(out["mean_obs"][2:], np.bincount(y, minlength=3), rtol=0)
        _same(_low(pt, data, weights=res[0].T), out)
        chk = pt.predictive_check(data, seed=SEED, return_samples=True)
        assert chk.names == ["deviance", "accuracy", "class_count[0]", "class_count[1]", "class_count[2]"]
        assert np.array_equal(chk.t_rep, out["t_rep"])
        print(data, {n: round(v, 4) for n, v in chk.p_value.items()})
    with pytest.raises(ValueError, match="lags"):
        pt.predictive_check("test", lags=(1, 2))
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="lags"):
        _low(pt, "test", lags=(1,))


def test_known_answer_pair(tmp_path):
    """The pair of tests/test_ppc_cpu.py through the device: vectors that give one constant output (zero weights, one output
    bias) with one eta, as one vector of multiplicity 2000, on host rows whose targets are that output + tau * noise."""
    from ptnn_amd.parallel_tempering import ppc_flagged
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    P = pt.num_param
    w = np.zeros((1, P), np.float32)
    w[:, P - 1] = 0.3                                             # the output bias
    eta = np.full(1, ref.KNOWN_ETA, np.float32)
    x = np.random.default_rng(11).uniform(0, 1, (ref.KNOWN_N, 4)).astype(np.float32)
    const = pt.posterior_predictive(x, weights=w).mean[0, 0]      # the device's fp32 output of the constant net
    tau = np.exp(0.5 * ref.KNOWN_ETA)
    out = {}
    for case in ("iid", "ar1"):
        rows = np.column_stack([x, (const + tau * ref.known_noise(case)).astype(np.float32)])
        out[case] = pt.predictive_check(rows, weights=(w, [ref.KNOWN_M]), eta=eta, lags=ref.KNOWN_LAGS, seed=ref.KNOWN_DRAW_SEED)
        assert out[case].n_samples == ref.KNOWN_M and out[case].n_distinct == 1
        assert all(v == ref.KNOWN_M for v in out[case].n_defined.values())
        print(case, {n: round(v, 4) for n, v in out[case].p_value.items()})
    assert out["ar1"].p_value["resid_acf[1]"] <= 0.01 and "ljung_box" in ppc_flagged(out["ar1"])
    assert all(0.005 <= p <= 0.995 for p in out["iid"].p_value.values()), out["iid"].p_value
    # the replicates depend on the seed and the occurrence only: the oracle's, from the same draws
    names, r = ref.check_regression(np.full((1, ref.KNOWN_N), float(const)), eta, [ref.KNOWN_M],
                                    _targets(rows, 4), ref.KNOWN_LAGS, ref.KNOWN_DRAW_SEED)
    for j, n in enumerate(names):
        assert out["ar1"].p_value[n] == pytest.approx(r["p_value"][j], abs=2.0 / ref.KNOWN_M), n


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(60, 100)["pos_w"].reshape(-1, pt.num_param)
            e = pt._sampler.trace_rows(60, 100)[:, :, 3].reshape(-1)          # eta of those rows
            chk = pt.predictive_check("test", weights=w, eta=e)
            assert chk.n_samples == 800 and all(np.isfinite(v) for v in chk.p_value.values())
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
        pt.predictive_check("test")
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 100:].reshape(-1)
    with pytest.raises(ValueError, match="eta"):                       # host vectors without eta on a regression
        pt.predictive_check("test", weights=res[0].T)
    with pytest.raises(_lib.PtnnError, match="need eta"):
        pt._sampler.ppc("test", w=res[0].T)
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):  # a trace row without eta
        pt.predictive_check("test", burn_in=0)
    for bad, word in (((0,), "lie in"), ((len(te),), "lie in"), ((2, 2), "distinct")):
        with pytest.raises(ValueError, match=word):
            pt.predictive_check("test", lags=bad)
    for bad, word in (((0,), "outside"), ((len(te),), "outside"), ((2, 2), "once"), (tuple(range(1, 18)), "n_lags")):
        with pytest.raises(_lib.PtnnError, match=word):
            pt._sampler.ppc("test", step0=100, lags=bad)
    with pytest.raises(ValueError, match="at least 2"):
        pt.predictive_check(te[:1], weights=res[0].T, eta=eta)
    with pytest.raises(_lib.PtnnError, match="at least 2"):
        pt._sampler.ppc(te[:1].astype(np.float32), w=res[0].T, eta=eta)
    two = pt.predictive_check(te[:2], weights=res[0].T, eta=eta)       # two rows are enough: lag 1 only
    assert two.names[7:] == ["resid_acf[1]"] and two.n_samples == 400
    # the C entry itself: classes of a regression
    import ctypes as C
    buf = np.empty((400, len(te)), np.int32)
    spec = _lib.PpcSpec()
    spec.struct_bytes = C.sizeof(_lib.PpcSpec)
    spec.thin, spec.step0, spec.nsteps, spec.n_rows, spec.x_source = 1, 100, 100, len(te), _lib.PREDICT_X_TEST
    spec.y_rep = buf.ctypes.data_as(C.POINTER(C.c_int32))
    with pytest.raises(_lib.PtnnError, match="y_rep"):
        pt._sampler._check(pt._sampler.lib.ptnn_ppc(pt._sampler.h, C.byref(spec)))
    ok = pt.predictive_check("test")                                   # the handle is still usable
    assert ok.n_samples == 400
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        ls.predictive_check("test")
    so = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, trace_capacity=64)
    so.run_chains()
    with pytest.raises(ValueError, match="streamed off"):
        so.predictive_check("test")
    assert so.predictive_check("test", weights=res[0].T, eta=eta).n_samples == 400


def test_sharded_ladder_is_refused(tmp_path):
    """A ladder sharded over several devices has no single handle: refused before anything is launched."""
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    pt.run_chains()
    one = pt._sampler
    pt._sampler = object()                                        # what a ladder over several devices keeps in its place
    try:
        with pytest.raises(ValueError, match="one GPU"):
            pt.predictive_check("test")
    finally:
        pt._sampler = one
    assert pt.predictive_check("test").n_samples == 400
