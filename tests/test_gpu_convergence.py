"""Convergence diagnostics on the GPU (ptnn_convergence / convergence_diagnostics): split-R-hat, split-ESS, the raw autocorrelation
and the pooled moments against the float64 oracle (tests/convergence_ref.py) on synthetic series and on the sampled traces of every
schedule, source agreement, blocking, absence of side effects and the refusals."""
import math

import numpy as np
import pytest

import convergence_ref as cr
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242


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


def _series(C, n, Q, seed):
    """fp32 draws [C, n, Q]: AR(1) with phi from -0.5 to 0.999 over the quantities; with Q > 2 quantity 0 is constant and
    quantity 1 constant within each chain but different between chains."""
    rng = np.random.default_rng(seed)
    phi = np.linspace(-0.5, 0.999, Q)
    y = np.empty((C, n, Q))
    y[:, 0] = rng.standard_normal((C, Q)) / np.sqrt(1 - phi ** 2)
    e = rng.standard_normal((C, n, Q))
    for i in range(1, n):
        y[:, i] = phi * y[:, i - 1] + e[:, i]
    y += rng.standard_normal(Q) * 3
    if Q > 2:
        y[:, :, 0] = 1.25
        y[:, :, 1] = np.arange(C)[:, None] * 0.5
    return y.astype(np.float32)


def _close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ok = same | (fin & (np.abs(got - want) <= tol * np.maximum(np.abs(want), 1.0)))
    return ok


def _check(out, want, *, per_chain=True, n_lags=0):
    """The issue's tolerances; quantities whose deciding pair sum lies within 1e-9 of 0 are exempt from ess / trunc_lag. -> exempt."""
    for k in ("mean", "var", "r_hat"):
        assert np.all(_close(out[k], want[k], 1e-12)), k
    exempt = np.abs(np.nan_to_num(want["deciding"], nan=1.0)) < 1e-9
    assert np.array_equal(out["trunc_lag"][~exempt], want["trunc_lag"][~exempt])
    ok = np.isnan(want["ess"]) & np.isnan(out["ess"]) | (np.abs(out["ess"] - want["ess"]) <= 1e-10 * np.abs(want["ess"]))
    assert np.all(ok | exempt), np.flatnonzero(~(ok | exempt))
    if per_chain:
        ex_c = np.abs(np.nan_to_num(want["deciding_chain"], nan=1.0)) < 1e-9
        ec, wc = out["ess_chain"], want["ess_chain"]
        okc = (np.isnan(wc) & np.isnan(ec)) | (np.abs(ec - wc) <= 1e-10 * np.abs(wc))
        assert np.all(okc | ex_c)
        exempt = exempt | ex_c.any(axis=0)
    if n_lags:
        assert np.all(_close(out["rho"], want["rho"][:n_lags], 1e-12))
    return int(exempt.sum())


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"), schedule=3)
    res = pt.run_chains()
    return pt, res, d


GRID = [(1, 4, 1), (2, 5, 63), (7, 101, 65), (64, 4, 300), (1, 4000, 63), (2, 4000, 65), (7, 5, 300), (64, 101, 1), (7, 4000, 1),
        (64, 4000, 65)]


@pytest.mark.parametrize("C,n,Q", GRID)
def test_host_draws_against_the_oracle(sunspot, C, n, Q):
    pt = sunspot[0]
    x = _series(C, n, Q, seed=C * 100003 + n * 7 + Q)
    h = n // 2
    n_lags = min(h, 40)
    out = pt._sampler.convergence(draws=x, per_chain=True, n_lags=n_lags)
    want = cr.diagnose_all(x)
    exempt = _check(out, want, n_lags=n_lags)
    assert exempt <= max(1, Q // 20), exempt
    assert out["n_chains"] == C and out["n_draws"] == n
    if Q > 2:
        assert math.isnan(out["r_hat"][0]) and math.isnan(out["ess"][0])   # constant quantity
        if C > 1:
            assert out["r_hat"][1] == math.inf                             # constant chains that differ
            if n == 4000:
                assert out["trunc_lag"].max() > 1000                       # phi = 0.999 reaches past 1 000 lags


def _trace_case(pt, *, replicas=None, step0, nsteps, thin, scalars=(0, 1, 2, 3, 4), n_lags=8):
    s = pt._sampler
    out = s.convergence(replicas=replicas, step0=step0, nsteps=nsteps, thin=thin, scalars=scalars, per_chain=True, n_lags=n_lags)
    tr = s.traces(step0, nsteps)["pos_w"]
    rows = s.trace_rows(step0, nsteps)
    reps = list(range(s.R)) if replicas is None else list(replicas)
    cols = [tr[reps, ::thin, :]] + [rows[reps, ::thin, c:c + 1] for c in scalars]
    x = np.concatenate(cols, axis=2).astype(np.float32)
    _check(out, cr.diagnose_all(x), n_lags=n_lags)
    # the same draws from the host: bitwise the same
    host = s.convergence(draws=x, per_chain=True, n_lags=n_lags)
    for k in ("mean", "var", "r_hat", "ess", "trunc_lag", "ess_chain", "rho"):
        assert np.array_equal(out[k], host[k], equal_nan=k != "trunc_lag"), k
    return out


def test_trace_source_packed(sunspot):
    pt = sunspot[0]
    assert "packed" in pt._sampler.describe()["schedule"]
    _trace_case(pt, step0=300, nsteps=300, thin=1)
    _trace_case(pt, replicas=[5, 1, 2], step0=101, nsteps=450, thin=3, scalars=(0, 3))


@pytest.mark.parametrize("name,topo,sched,label,lg", [("iris", (4, 12, 3), 4, "tree", False),
                                                      ("ions", (34, 50, 2), 1, "cooperative", True)])
def test_trace_source_classification(name, topo, sched, label, lg, tmp_path):
    d = parity.datasets()
    pt = _pt(orc.TASK_CLS, topo, d[name + "_train"], d[name + "_test"], 8, 400, tmp_path, lg=lg, lr=0.01, maxtemp=10, schedule=sched)
    assert label in pt._sampler.describe()["schedule"]
    pt.run_chains()
    _trace_case(pt, step0=200, nsteps=200, thin=1)
    _trace_case(pt, replicas=[7, 0], step0=50, nsteps=301, thin=2, scalars=(0, 4))


def test_trace_source_wide_compact(tmp_path):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (32, 256, 1), d["synth32_train"], d["synth32_test"], 4, 200, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    pt.run_chains()
    _trace_case(pt, step0=100, nsteps=100, thin=1)


def test_trace_source_ring(tmp_path):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path, trace_capacity=64)
    pt.run_chains()
    cur = 199
    _trace_case(pt, step0=cur + 1 - 64, nsteps=64, thin=1)
    _trace_case(pt, replicas=[3], step0=cur - 40, nsteps=41, thin=2)


def test_blocking_changes_nothing(sunspot, monkeypatch):
    pt = sunspot[0]
    ref = pt._sampler.convergence(step0=300, nsteps=300, scalars=(0, 1), per_chain=True, n_lags=20)
    x = _series(7, 101, 65, seed=9)
    ref_h = pt._sampler.convergence(draws=x, per_chain=True, n_lags=20)
    monkeypatch.setenv("PTNN_CONVERGENCE_SCRATCH_BYTES", "1")                 # one quantity per block
    got = pt._sampler.convergence(step0=300, nsteps=300, scalars=(0, 1), per_chain=True, n_lags=20)
    got_h = pt._sampler.convergence(draws=x, per_chain=True, n_lags=20)
    for a, b in ((ref, got), (ref_h, got_h)):
        for k in ("mean", "var", "r_hat", "ess", "trunc_lag", "ess_chain", "rho"):
            assert np.array_equal(a[k], b[k], equal_nan=k != "trunc_lag"), k
    # the per-chain ESS asked for or not: the combined figures are the same
    plain = pt._sampler.convergence(draws=x)
    for k in ("r_hat", "ess", "trunc_lag"):
        assert np.array_equal(plain[k], ref_h[k], equal_nan=k != "trunc_lag"), k


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            c = pt._sampler.convergence(step0=0, nsteps=100, scalars=(0, 1, 2, 3, 4), per_chain=True, n_lags=10)
            assert c["n_draws"] == 100
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
        pt.convergence_diagnostics()
    x = _series(4, 50, 3, seed=1)
    assert pt.convergence_diagnostics(draws=x).ess.shape == (3,)                 # draws= works before any run
    with pytest.raises(_lib.PtnnError, match="queued"):
        pt._sampler.convergence(step0=0, nsteps=50)
    pt.run_chains()
    s = pt._sampler
    with pytest.raises(_lib.PtnnError, match="at least 4"):
        s.convergence(step0=100, nsteps=3)
    with pytest.raises(_lib.PtnnError, match="parameter"):
        s.convergence(step0=100, nsteps=100, params=[s.P])
    with pytest.raises(_lib.PtnnError, match="replica"):
        s.convergence(step0=100, nsteps=100, replicas=[4])
    with pytest.raises(_lib.PtnnError, match="trace range"):
        s.convergence(step0=150, nsteps=100)
    with pytest.raises(_lib.PtnnError, match="n_lags"):
        s.convergence(step0=100, nsteps=100, n_lags=51)
    ok = pt.convergence_diagnostics()                                             # the handle is still usable
    assert ok.n_draws == 100 and len(ok.names) == s.P + 1
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        ls.convergence_diagnostics()
    assert ls.convergence_diagnostics(draws=x).n_chains == 4
    st = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, trace_capacity=64)
    st.run_chains()
    with pytest.raises(ValueError, match="trace_capacity"):
        st.convergence_diagnostics()
    assert st.convergence_diagnostics(draws=x).n_draws == 50


def test_convergence_diagnostics_end_to_end(sunspot):
    pt, res, _ = sunspot
    P, R, S = pt.num_param, 8, 600
    cd = pt.convergence_diagnostics(scalars=("likelihood", "rmse_train", "rmse_test", "eta", "acc_test"), per_chain=True, n_lags=5)
    assert cd.names == [f"w{p}" for p in range(P)] + ["likelihood", "rmse_train", "rmse_test", "eta", "acc_test"]
    Q = P + 5
    assert cd.n_chains == R and cd.n_draws == S // 2
    for k in ("mean", "sd", "r_hat", "ess", "mcse_mean", "trunc_lag"):
        assert getattr(cd, k).shape == (Q,), k
    assert cd.ess_chain.shape == (R, Q) and cd.rho.shape == (5, Q)
    # the weights' pooled moments are those of the posterior matrix run_chains() returned
    post = np.asarray(res[0], np.float64)                                        # [P, R (S - b)]
    np.testing.assert_allclose(cd.mean[:P], post.mean(axis=1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(cd.sd[:P], post.std(axis=1, ddof=1), rtol=1e-10)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(cd.mcse_mean, cd.sd / np.sqrt(cd.ess))
    assert math.isnan(cd.r_hat[-1])                                               # a regression's acc_test is 0 on every step
    cold = pt.convergence_diagnostics(chains="cold", per_chain=True, params=[0, 3])
    ci = int(np.argmin(pt.temperatures))
    assert cold.names == ["w0", "w3", "likelihood"] and cold.n_chains == 1 and cold.ess_chain.shape == (1, 3)
    tr = pt._sampler.traces(S // 2, S - S // 2)
    x = np.concatenate([tr["pos_w"][ci:ci + 1, :, [0, 3]], tr["likeh"][ci:ci + 1, :, None]], axis=2).astype(np.float32)
    want = cr.diagnose_all(x)
    np.testing.assert_allclose(cold.ess_chain[0], want["ess_chain"][0], rtol=1e-10)
    thin = pt.convergence_diagnostics(thin=4, chains=[1, 6])
    assert thin.n_chains == 2 and thin.n_draws == -(-(S - S // 2) // 4)
