"""Power-scaling sensitivity on the GPU (ptnn_powerscale / powerscale_sensitivity): the components against the existing calls,
the smoothing, distances and moments against the float64 oracle (tests/powerscale_ref.py) fed the device's own quantities and
components, bitwise agreement between sources, block sizes and selections, the two known-answer cases, and the refusals.

Bounds: dist, mean and sd at rtol 1e-9 / atol 1e-10 (double sums over U <= 2^13 terms in a fixed order; the oracle is given the
device's fp32 quantities and double components, so only the order of the sums, exp and log2 differ)."""
import math
import warnings

import numpy as np
import pytest

import parity
import powerscale_ref as ref
from parity import orc
from test_gpu_elpd import _pt, _runs

pytestmark = pytest.mark.gpu

ALL = ("weights", "eta", "predictions", "loglik")
KEYS = ("sens", "dist", "mean", "sd", "base_mean", "base_sd", "khat", "tail_len", "logp")
# |D - QUADRATURE_D| of the oracle over seeds 0 .. 5 at n_w = 20 000 and P = 7 (net 4-1-1, the smallest compiled shape),
# measured on the CPU: 0.0401, 0.0392, 0.0390, 0.0375, 0.0394, 0.0406.  The margin is twice the largest.
QUADRATURE_MARGIN_P7 = 2 * 0.0406
# The sharp check (tests/test_powerscale_cpu.py says why): the quadrature over each coordinate's own sample range.  Largest
# |D - quadrature| of the oracle over seeds 0 .. 5 at P = 7: 0.00653, 0.00617, 0.00408, 0.00233, 0.00589, 0.00573; twice the largest.
RANGE_MARGIN_P7 = 2 * 0.00653


def _low(pt, data, *, groups=ALL, delta=0.01, burn_in=None, chains="all", thin=1, weights=None, eta=None, r_eff=1.0):
    """The binding's call on the selection powerscale_sensitivity() would make."""
    I = int(pt.topology[0])
    ds = data if isinstance(data, str) else np.ascontiguousarray(np.asarray(data)[:, :I], dtype=np.float32)
    groups = [g for g in ALL if g in groups and (g != "eta" or pt.task == orc.TASK_REG)]
    if weights is not None:
        w, mult = pt._weights(weights)
        kw = dict(w=w, eta=eta, multiplicity=mult)
    else:
        kw, _ = pt._trace_selection(burn_in, chains, thin)
    return pt._sampler.powerscale(ds, groups=groups, delta=delta, r_eff=r_eff, **kw)


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["n_samples"] == b["n_samples"] and a["n_distinct"] == b["n_distinct"]


def _worst(name, got, want, rtol, atol):
    err = np.abs(got - want)
    print(f"{name}: max abs diff {err.max():.3e}, max rel diff {np.max(err / np.maximum(np.abs(want), 1e-300)):.3e}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=name)


def check_oracle(pt, data, w, e, c, out, groups=ALL):
    """out = the device's call on the distinct vectors w (eta e, multiplicities c) -> the oracle's result from the device's own
    quantities (the vectors, eta, posterior_predictive's outputs, logp) and components."""
    U = len(c)
    assert out["n_distinct"] == U and out["n_samples"] == int(np.sum(c)) and out["logp"].shape == (2, U)
    vals = []
    if "weights" in groups:
        vals.append(np.asarray(w, np.float32).T)
    if "eta" in groups and pt.task == orc.TASK_REG:
        vals.append(np.asarray(e, np.float32)[None, :])
    if "predictions" in groups:
        f = pt.posterior_predictive(data, weights=w, return_samples=True).samples            # [U, N, O]
        vals.append(f.reshape(U, -1).T)
    if "loglik" in groups:
        vals.append(out["logp"][0].astype(np.float32)[None, :])
    vals = np.concatenate(vals, axis=0)
    assert out["n_quantities"] == vals.shape[0]
    r = ref.powerscale(vals, out["logp"], c, delta=0.01)
    assert np.array_equal(out["tail_len"], r["tail_len"])
    fin = np.isfinite(r["khat"])
    assert np.array_equal(np.isfinite(out["khat"]), fin)
    print("khat", out["khat"].ravel(), "tail", out["tail_len"].ravel())
    assert np.max(np.abs(out["khat"][fin] - r["khat"][fin]), initial=0.0) <= 1e-9
    for k in ("dist", "mean", "sd", "base_mean", "base_sd"):
        _worst(k, out[k], r[k], 1e-9, 1e-10)
    # sens = (d- + d+) / (2 log2 1.01): two dist errors of atol 1e-10 each over 0.0287 are 7e-9, rounded up
    _worst("sens", out["sens"], r["sens"], 1e-9, 1e-8)
    return r


def check_components(pt, out, w, e, c, sel):
    """logp[0] = the row sum of predictive_accuracy's train log-likelihood (summed in row order), logp[1] = evaluate's prior."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa = pt.predictive_accuracy("train", return_pointwise=True, **sel)
    own = np.repeat(np.arange(len(c)), c)
    rowsum = np.cumsum(pa.log_lik, axis=1)[:, -1]                                # sequential, as the device sums
    print("logp[0] exact:", np.array_equal(out["logp"][0][own], rowsum))
    np.testing.assert_allclose(out["logp"][0][own], rowsum, rtol=1e-12)
    tau = None if pt.task == orc.TASK_CLS else np.exp(np.asarray(e, np.float32))
    ev = pt._sampler.evaluate(w, tau)[:, 5]
    np.testing.assert_allclose(out["logp"][1], ev, rtol=2e-5)
    want = ref.prior_component(0 if pt.task == orc.TASK_REG else 1, w, e, tuple(pt.topology))
    np.testing.assert_allclose(out["logp"][1], want, rtol=1e-13)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)
    return pt, res, d, eta


def test_regression_sunspot(sunspot):
    pt, res, d, eta = sunspot
    w, e, c = _runs(res[0].T, eta)
    for data in ("train", "test"):
        out = _low(pt, data)
        assert out["n_samples"] == 2400 and out["n_distinct"] == len(c)
        check_oracle(pt, data, w, e, c, out)
        N = len(d["sunspot_" + data])
        assert out["n_quantities"] == 31 + 1 + N + 1
    check_components(pt, out, w, e, c, {})
    # the public call: the same numbers by name
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ps = pt.powerscale_sensitivity("test", quantities=ALL)
    assert ps.names[:32] == [f"w[{p}]" for p in range(31)] + ["eta"] and ps.names[-1] == "loglik" and ps.names[32] == "f[0]"
    assert [ps.likelihood[n] for n in ps.names] == out["sens"][0].tolist() and [ps.prior[n] for n in ps.names] == out["sens"][1].tolist()
    assert ps.khat["prior", "+"] == out["khat"][1, 1] and ps.n_samples == 2400
    j = ps.names.index("eta")
    assert ps.mean_shift["prior", "-"]["eta"] == (out["mean"][1, 0, j] - out["base_mean"][j]) / out["base_sd"][j]
    assert ps.sd_ratio["likelihood", "+"]["eta"] == out["sd"][0, 1, j] / out["base_sd"][j]
    from ptnn_amd.parallel_tempering import powerscale_flagged
    assert [n for n, _ in powerscale_flagged(ps)] == [n for n in ps.names if ps.diagnosis[n] != "-"]
    top = sorted(ps.names, key=lambda n: -ps.prior[n])[:5]
    print("prior-sensitive:", [(n, round(ps.prior[n], 4), round(ps.likelihood[n], 4), ps.diagnosis[n]) for n in top])
    print("flagged:", len(powerscale_flagged(ps)), "of", len(ps.names), "khat", ps.khat)
    dflt = pt.powerscale_sensitivity("test")
    assert dflt.names == ps.names[:-1] and dflt.prior == {n: ps.prior[n] for n in dflt.names}


def test_sources_blocks_and_selections_agree(sunspot, monkeypatch):
    pt, res, d, eta = sunspot
    base = _low(pt, "test")
    _same(_low(pt, "test"), base)                                            # the same call twice
    _same(_low(pt, "test", weights=res[0].T, eta=eta), base)
    w, e, c = _runs(res[0].T, eta)
    _same(_low(pt, "test", weights=(w, c), eta=e), base)
    U, Q = base["n_distinct"], base["n_quantities"]
    npow = 1 << max(1, (U - 1).bit_length())
    for nq in (1, 7, Q):
        monkeypatch.setenv("PTNN_POWERSCALE_SCRATCH_BYTES", str((8 * npow + 4 * U) * nq))
        _same(_low(pt, "test"), base)
        _same(_low(pt, "test", weights=(w, c), eta=e), base)
    monkeypatch.delenv("PTNN_POWERSCALE_SCRATCH_BYTES")
    # a group alone gives the same columns
    only = _low(pt, "test", groups=("predictions",))
    assert np.array_equal(only["dist"], base["dist"][:, :, 32:-1]) and np.array_equal(only["khat"], base["khat"])
    R = 8
    et = pt._sampler.eta_trace()
    cols = res[0].T.reshape(R, 300, -1)
    cold = int(np.argmin(pt.temperatures))
    for kw, sel_w, sel_e in ((dict(chains="cold"), cols[cold], et[cold, 300:]),
                             (dict(chains=[1, 6]), cols[[1, 6]].reshape(-1, cols.shape[2]), et[[1, 6], 300:].reshape(-1)),
                             (dict(thin=3), cols[:, ::3].reshape(-1, cols.shape[2]), et[:, 300::3].reshape(-1))):
        a = _low(pt, "test", **kw)
        _same(a, _low(pt, "test", weights=sel_w, eta=sel_e))
        assert a["n_samples"] == len(sel_e)
        ws, es, cs = _runs(sel_w, sel_e)
        check_oracle(pt, "test", ws, es, cs, a)


def test_classification_iris(tmp_path):
    d = parity.datasets()
    pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    w, e, c = _runs(res[0].T, np.zeros(res[0].shape[1], np.float32))
    for data in ("train", "test"):
        out = _low(pt, data)
        check_oracle(pt, data, w, e, c, out)
        _same(_low(pt, data, weights=res[0].T), out)
    check_components(pt, out, w, None, c, {})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ps = pt.powerscale_sensitivity("test")
    assert ps.names[:pt.num_param] == [f"w[{p}]" for p in range(pt.num_param)] and ps.names[pt.num_param] == "p[0,0]"
    with pytest.raises(ValueError, match="no eta"):
        pt.powerscale_sensitivity("test", quantities=("eta",))
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="no eta"):
        pt._sampler.powerscale("test", groups=("eta",), step0=200)


def test_known_answers(tmp_path):
    """The two cases of tests/test_powerscale_cpu.py through the device, at the smallest compiled shape 4-1-1 (P = 7)."""
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 1, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    P = pt.num_param
    assert P == 7
    rng = np.random.default_rng(3)
    w0 = rng.normal(0, 2, P).astype(np.float32)
    w = (rng.choice(np.array([-1.0, 1.0], np.float32), (500, P)) * w0[None, :]).astype(np.float32)
    w[0] = w0
    eta = np.full(500, -1.5, np.float32)
    out = _low(pt, "test", weights=w, eta=eta)
    assert np.all(out["logp"][1] == out["logp"][1][0])
    assert np.all(out["sens"][1] == 0.0) and np.all(out["dist"][1] == 0.0)
    assert np.all(np.isinf(out["khat"][1])) and np.all(out["tail_len"][1] == 0)          # the <= 4 rule: nothing above the cut
    assert np.array_equal(out["mean"][1, 0], out["base_mean"]) and np.array_equal(out["sd"][1, 1], out["base_sd"])
    assert np.any(out["sens"][0] > 0.0)
    # the Gaussian prior against the quadrature value
    wq, eq = ref.quadrature_case(0, 20000, P)
    out = _low(pt, "test", groups=("weights",), weights=wq, eta=eq, r_eff=1.0)
    print("D_prior", out["sens"][1], "khat", out["khat"][1])
    assert np.max(np.abs(out["sens"][1] - ref.QUADRATURE_D)) <= QUADRATURE_MARGIN_P7
    want = np.array([ref.quadrature_sensitivity(float(wq[:, p].min()), float(wq[:, p].max())) for p in range(P)])
    print("over the sample's range:", want, np.abs(out["sens"][1] - want).max())
    assert np.max(np.abs(out["sens"][1] - want)) <= RANGE_MARGIN_P7
    r = ref.powerscale(wq.T, out["logp"], np.ones(20000, np.int64))
    _worst("dist", out["dist"], r["dist"], 1e-9, 1e-10)


def test_several_sort_tiles_with_ties_and_multiplicities(tmp_path, monkeypatch):
    """U = 5 000 distinct vectors (8 192 sort words: two LDS tiles, one global step and one merge per quantity) with
    multiplicities 0 .. 3, tied values in every group (vectors that share their first weights, etas from a set of 40, rows whose
    prediction saturates), all four groups, and blocks of seven quantities."""
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path)
    rng = np.random.default_rng(17)
    U, P = 5000, pt.num_param
    w = rng.normal(0, 1.5, (U, P)).astype(np.float32)
    w[:, :3] = w[rng.integers(0, 50, U), :3]                                # 50 distinct values in the first three weights
    w[::7, P - 1] = 40.0                                                     # a saturated output: f == 1 on every row
    e = rng.choice(np.linspace(-4, -2, 40).astype(np.float32), U)
    c = rng.integers(0, 4, U).astype(np.int32)
    c[:2] = 1
    rows = d["sunspot_test"][:25]
    out = _low(pt, rows, weights=(w, c), eta=e)
    assert out["n_distinct"] == U and out["n_samples"] == int(c.sum())
    live = c > 0
    f = pt.posterior_predictive(rows[:, :4], weights=w, return_samples=True).samples[:, :, 0]
    assert np.unique(f[:, 0]).size < U and np.unique(w[:, 0]).size <= 50
    vals = np.concatenate([w.T, e[None, :], f.T, out["logp"][0].astype(np.float32)[None, :]], axis=0)
    r = ref.powerscale(vals[:, live], out["logp"][:, live], c[live])
    assert np.array_equal(out["tail_len"], r["tail_len"])
    for k in ("dist", "mean", "sd", "base_mean", "base_sd"):
        _worst(k, out[k], r[k], 1e-9, 1e-10)
    monkeypatch.setenv("PTNN_POWERSCALE_SCRATCH_BYTES", str((8 * 8192 + 4 * U) * 7))
    _same(_low(pt, rows, weights=(w, c), eta=e), out)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(60, 100)["pos_w"].reshape(-1, pt.num_param)
            e = pt._sampler.trace_rows(60, 100)[:, :, 3].reshape(-1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ps = pt.powerscale_sensitivity("test", weights=w, eta=e)
            assert ps.n_samples == 800 and all(np.isfinite(v) for v in ps.prior.values())
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


def test_refusals(tmp_path, monkeypatch):
    from ptnn_amd import _lib
    d = parity.datasets()
    tr, te = d["sunspot_train"], d["sunspot_test"]
    pt = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path)
    with pytest.raises(ValueError, match="run_chains"):
        pt.powerscale_sensitivity("test")
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 100:].reshape(-1)
    for bad in (0.0, -0.5, math.nan):
        with pytest.raises(ValueError, match="delta"):
            pt.powerscale_sensitivity("test", delta=bad)
        with pytest.raises(_lib.PtnnError, match="delta"):
            pt._sampler.powerscale("test", step0=100, delta=bad)
    with pytest.raises(ValueError, match="unknown"):
        pt.powerscale_sensitivity("test", quantities=("weights", "bias"))
    with pytest.raises(ValueError, match="eta"):
        pt.powerscale_sensitivity("test", weights=res[0].T)
    with pytest.raises(_lib.PtnnError, match="need eta"):
        pt._sampler.powerscale("test", w=res[0].T)
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt.powerscale_sensitivity("test", burn_in=0)
    with pytest.raises(_lib.PtnnError, match="at least 2"):
        pt._sampler.powerscale("test", w=res[0].T[:1], eta=eta[:1])
    # a component that is not finite for a selected sample; with multiplicity 0 the vector takes no part
    w = res[0].T.copy()
    w[3, 0] = np.inf
    with pytest.raises(_lib.PtnnError, match="prior component of distinct sample"):
        pt._sampler.powerscale("test", w=w, eta=eta)
    mult = np.ones(len(eta), np.int32)
    mult[3] = 0
    ok = pt._sampler.powerscale("test", w=w, eta=eta, multiplicity=mult)
    assert ok["n_samples"] == len(eta) - 1 and np.all(np.isfinite(ok["sens"]))
    # more distinct samples than the cap
    big = np.random.default_rng(0).normal(0, 1, (_lib.POWERSCALE_MAX_DISTINCT + 1, 31)).astype(np.float32)
    with pytest.raises(_lib.PtnnError, match="thin="):
        pt._sampler.powerscale("test", w=big, eta=np.zeros(len(big), np.float32), groups=("eta",), r_eff=100.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert pt.powerscale_sensitivity("test").n_samples == 400             # the handle is still usable
    # a handle with a communicator attached
    sh = parity.make_sampler(0, (4, 5, 1), tr, te, R_local=2, R_global=4, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    sh.set_state(np.zeros((2, 31), np.float32), np.ones(2, np.float32))
    one = dict(w=np.random.default_rng(1).normal(0, 1, (8, 31)).astype(np.float32), eta=np.zeros(8, np.float32))
    assert sh.powerscale("test", **one)["n_samples"] == 8
    sh.comm_init_host(0, 2, lambda b: None, lambda m: None)
    with pytest.raises(_lib.PtnnError, match="communicator"):
        sh.powerscale("test", **one)
