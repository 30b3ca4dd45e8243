"""Log evidence on the GPU (ptnn_evidence / log_evidence): every draw's U against the float64 oracle (tests/evidence_ref.py) on
narrow and wide-net layouts of both tasks, U against the per-row values of predictive_accuracy / posterior_predictive, bitwise
agreement of the sources and of any block size, the prior draws against philox.prior_weights, side effects and refusals."""
import math
import warnings

import numpy as np
import pytest

import evidence_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
SIGMA = 5.0            # sqrt(sigma_squared = 25)


def _pt(task, topo, train, test, R, S, path, *, lg=True, lr=0.1, maxtemp=2, si=10, burn_in=0.5, seed=SEED, **kw):
    if task == orc.TASK_REG:
        from ptnn_amd.pt_timeseries_regression import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, 0.5, str(path), seed=seed, write_files=False, **kw)
    else:
        from ptnn_amd.pt_classification import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, str(path), seed=seed, write_files=False, **kw)
    pt.initialize_chains(burn_in)
    return pt


def _evidence(pt, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return pt.log_evidence(**kw)


def _rungs(pt, thin=1):
    """(betas ascending, vectors [K, n, P]) of the rows log_evidence selects by default."""
    S = pt.NumSamples
    step0 = int(S * pt.burn_in)
    sw = pt._pt_switch_step()
    end = sw if sw >= 0 else S
    betas = np.array([1.0 / float(np.float32(T)) for T in pt.temperatures])
    order = np.argsort(betas, kind="stable")
    w = pt._sampler.traces(step0, end - step0)["pos_w"][order][:, ::thin]
    return betas[order], np.ascontiguousarray(w)


def _oracle_u(task, rows, W, topo):
    U = np.empty(W.shape[0])
    for k in range(0, W.shape[0], 512):
        U[k:k + 512] = ref.u_and_b_batched(task, rows, W[k:k + 512], topo)[0]
    return U


def _same(a, b):
    for k in ("log_z_ss", "se_log_z_ss", "log_z_ti", "se_log_z_ti", "ti_discretisation", "prior_kish_ess"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("betas", "u_mean", "u_mcse", "ess", "log_stones", "n_draws"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k


LAYOUTS = {
    "iris_cls": (orc.TASK_CLS, (4, 12, 3), "iris", 8, 400, dict(lr=0.01, maxtemp=10)),
    "sunspot_reg": (orc.TASK_REG, (4, 5, 1), "sunspot", 8, 600, {}),
    "ions_wide_cls": (orc.TASK_CLS, (34, 100, 2), "ions", 4, 200, dict(lr=0.01, maxtemp=10)),
    "synth32_wide_reg": (orc.TASK_REG, (32, 256, 1), "synth32", 4, 200, {}),
}


@pytest.fixture(scope="module", params=list(LAYOUTS))
def run(request, tmp_path_factory):
    task, topo, name, R, S, kw = LAYOUTS[request.param]
    d = parity.datasets()
    pt = _pt(task, topo, d[name + "_train"], d[name + "_test"], R, S, tmp_path_factory.mktemp(request.param), **kw)
    pt.run_chains()
    return pt, task, topo, np.asarray(d[name + "_train"], np.float64)


def test_u_against_the_oracle(run):
    pt, task, topo, train = run
    ev = _evidence(pt, prior_draws=2048, return_draws=True)
    betas, W = _rungs(pt)
    assert np.array_equal(ev.betas[1:], betas) and ev.betas[0] == 0.0
    K, n, P = W.shape
    assert len(ev.u_draws) == K and all(u.size == n for u in ev.u_draws)
    assert np.array_equal(ev.n_draws, np.concatenate([[2048], np.full(K, n)]))
    assert 1 <= ev.n_distinct <= K * n
    U = np.concatenate(ev.u_draws)
    np.testing.assert_allclose(U, _oracle_u(task, train, W.reshape(-1, P), topo), rtol=1e-5, atol=1e-4)
    # the per-rung statistics on the device's own draws
    for k in range(K):
        st = ref.rung_stats(ev.u_draws[k], betas[k + 1] - betas[k] if k + 1 < K else 0.0)
        assert ev.u_mean[k + 1] == pytest.approx(st["mean"], rel=1e-12)
        if k + 1 < K:
            assert ev.log_stones[k + 1] == pytest.approx(st["log_stone"], rel=1e-12, abs=1e-12)
    assert np.all(np.isfinite([ev.log_z_ss, ev.log_z_ti, ev.se_log_z_ss, ev.se_log_z_ti, ev.ti_discretisation]))
    # the prior draws: philox.prior_weights through the oracle's forward pass
    from ptnn_amd import philox
    Wp = np.stack([philox.prior_weights(pt.seed, i, P, SIGMA) for i in range(64)])
    np.testing.assert_allclose(ev.u_prior_draws[:64], _oracle_u(task, train, Wp, topo), rtol=1e-4, atol=1e-3)
    Up = ev.u_prior_draws
    Bp = np.zeros(Up.size) if task == orc.TASK_CLS else 2.0 * Up / train.shape[0]          # b = -log SSE = 2 U / N
    p0 = ref.prior_stats(Up, Bp, 0.0)
    assert ev.u_mean[0] == pytest.approx(p0["u_mean"], rel=1e-9)
    assert ev.ess[0] == pytest.approx(p0["kish"], rel=1e-9)
    p1 = ref.prior_stats(Up, Bp, betas[0])
    assert ev.log_stones[0] == pytest.approx(p1["log_mean_exp"], rel=1e-9, abs=1e-9)
    assert ev.prior_kish_ess == pytest.approx(p1["kish"], rel=1e-9)


def test_sources_and_blocks_agree(run, monkeypatch):
    pt, task, topo, train = run
    ev = _evidence(pt, prior_draws=512, return_draws=True)
    betas, W = _rungs(pt)
    # host vectors of the same rows (given in any rung order): bitwise
    perm = np.arange(W.shape[0])[::-1]
    hv = _evidence(pt, prior_draws=512, return_draws=True, weights=(betas[perm], W[perm]))
    _same(hv, ev)
    assert all(np.array_equal(a, b) for a, b in zip(hv.u_draws, ev.u_draws))
    assert np.array_equal(hv.u_prior_draws, ev.u_prior_draws) and hv.n_distinct == ev.n_distinct
    # blocks of rows and of prior draws under a tiny scratch budget: bitwise
    monkeypatch.setenv("PTNN_EVIDENCE_SCRATCH_BYTES", "20000")
    bl = _evidence(pt, prior_draws=512, return_draws=True)
    monkeypatch.delenv("PTNN_EVIDENCE_SCRATCH_BYTES")
    _same(bl, ev)
    assert all(np.array_equal(a, b) for a, b in zip(bl.u_draws, ev.u_draws))
    assert np.array_equal(bl.u_prior_draws, ev.u_prior_draws)
    # host U: the reductions against numpy float64, the ESS against ptnn_convergence on the same draws
    U = np.stack(ev.u_draws)
    K, n = U.shape
    d = np.append(np.diff(betas), 0.0)
    out = pt._sampler.evidence(u=U, d=d)
    for k in range(K):
        st = ref.rung_stats(U[k], d[k])
        assert out["u_mean"][k] == pytest.approx(st["mean"], rel=1e-12)
        tiny = 1e-12 * max(1.0, st["mean"] ** 2)           # a rung stuck on one vector: its variance is rounding noise
        assert out["u_var"][k] == pytest.approx(st["var"], rel=1e-12, abs=tiny)
        assert out["log_stone"][k] == pytest.approx(st["log_stone"], rel=1e-12, abs=1e-12)
        assert out["stone_relvar"][k] == pytest.approx(st["relvar"], rel=1e-9, abs=1e-12)
    conv = pt._sampler.convergence(draws=np.ascontiguousarray(U.T[None].astype(np.float32)))
    np.testing.assert_array_equal(out["u_ess"], conv["ess"])
    assert np.array_equal(out["u_mean"], ev.u_mean[1:]) and np.array_equal(out["u_ess"], ev.ess[1:], equal_nan=True)
    # multiplicities: the distinct runs of every rung with their counts give the same statistics
    mult = np.zeros((K, n), np.int32)
    Uc = np.zeros((K, n))
    for k in range(K):
        starts = np.flatnonzero(np.r_[True, U[k, 1:] != U[k, :-1]])
        mult[k, :starts.size] = np.diff(np.r_[starts, n])
        Uc[k, :starts.size] = U[k, starts]
    alt = pt._sampler.evidence(u=Uc, multiplicity=mult, d=d)
    for key in ("u_mean", "u_var", "log_stone", "stone_relvar", "u_ess"):
        assert np.array_equal(alt[key], out[key], equal_nan=True), key


def test_u_equals_the_pointwise_analyses(run):
    pt, task, topo, train = run
    ev = _evidence(pt, prior_draws=16, return_draws=True)
    betas, W = _rungs(pt)
    flat = W.reshape(-1, W.shape[2])
    U = np.concatenate(ev.u_draws)
    if task == orc.TASK_CLS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa = pt.predictive_accuracy("train", weights=flat, return_pointwise=True)
        np.testing.assert_allclose(U, pa.log_lik.sum(axis=1), rtol=1e-12)
    else:
        pp = pt.posterior_predictive("train", weights=flat, return_samples=True)
        y = train[:, topo[0]].astype(np.float32).astype(np.float64)       # the device holds the targets in fp32
        sse = np.sum((y[None, :] - pp.samples[:, :, 0].astype(np.float64)) ** 2, axis=1)
        np.testing.assert_allclose(U, -0.5 * train.shape[0] * np.log(sse), rtol=1e-12)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            betas = np.array([1.0 / float(np.float32(T)) for T in pt.temperatures])
            W = pt._sampler.traces(100, 60)["pos_w"]
            _evidence(pt, prior_draws=256, weights=(betas, W))
        res = pt.run_chains()
        if call:
            before = pt._sampler.traces()
            st = pt._sampler.state()
            _evidence(pt, prior_draws=256)
            after = pt._sampler.traces()
            for k in before:
                assert np.array_equal(before[k], after[k]), k
            st2 = pt._sampler.state()
            for k in st:
                assert np.array_equal(np.asarray(st[k]), np.asarray(st2[k])), k
        outs.append(res)
    for a, b in zip(outs[0], outs[1]):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b)


def test_refusals(tmp_path):
    d = parity.datasets()
    args = (orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 4, 200)
    for sub in ("a", "b", "c"):
        (tmp_path / sub).mkdir()
    pt = _pt(*args, tmp_path / "a", lr=0.01, maxtemp=10)
    with pytest.raises(ValueError, match="no finished run_chains"):
        pt.log_evidence(prior_draws=64)
    pt.run_chains()
    with pytest.raises(ValueError, match="at least 4"):
        pt.log_evidence(burn_in=0.59, prior_draws=64)
    betas, W = _rungs(pt)
    dup = betas.copy()
    dup[0] = dup[1]
    with pytest.raises(ValueError, match="duplicate temperatures"):
        pt.log_evidence(prior_draws=64, weights=(dup, W))
    with pytest.raises(ValueError, match="temperature 1"):
        pt.log_evidence(prior_draws=64, weights=(betas * 0.5, W))
    with pytest.raises(ValueError, match="weights"):
        pt.log_evidence(prior_draws=64, weights=W)
    with pytest.raises(ValueError, match="prior_draws"):
        pt.log_evidence(prior_draws=1)
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="split ESS"):
        pt._sampler.evidence(u=np.zeros((2, 3)))
    with pytest.raises(_lib.PtnnError, match="exponents"):
        pt._sampler.evidence(u=np.zeros((2, 8)), n_prior=16)
    pl = _pt(*args, tmp_path / "b", lr=0.01, maxtemp=10, label_swap=True, swap_rule=1)
    pl.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        pl.log_evidence(prior_draws=64)
    pc = _pt(*args, tmp_path / "c", lr=0.01, maxtemp=10, trace_capacity=64)
    pc.run_chains()
    with pytest.raises(ValueError, match="trace_capacity"):
        pc.log_evidence(prior_draws=64)
    # the drop-in's defaults: a warning that names the causes and the exact settings
    with pytest.warns(UserWarning, match="swap_rule=1"):
        pt.log_evidence(prior_draws=64)


def test_log_z_against_naive_monte_carlo(tmp_path):
    """End to end on a 12-row regression 4-3-1: random-walk proposals, swap_rule=1, shared_noise=False, 16 chains, maxtemp 1000,
    S = 40 000 (the fixed random-walk step needs that many to cover a prior-dominated posterior), against
    log c + log mean e^{b + U} over 2^22 prior draws in numpy float64."""
    rng = np.random.default_rng(11)
    x = rng.random((12, 4))
    data = np.column_stack([x, 0.2 + 0.6 * x[:, 0] * x[:, 1] + 0.05 * rng.standard_normal(12)])
    topo = (4, 3, 1)
    pt = _pt(orc.TASK_REG, topo, data, data, 16, 40000, tmp_path, lg=False, maxtemp=1000, si=5, burn_in=0.25, swap_rule=1,
             shared_noise=False)
    pt.run_chains()
    ev = _evidence(pt, prior_draws=1 << 20)
    naive, se_naive = ref.naive_log_z(orc.TASK_REG, data, topo, 1 << 22, SIGMA, seed=9)
    print(f"naive {naive:.5f} +- {se_naive:.5f}; SS {ev.log_z_ss:.5f} +- {ev.se_log_z_ss:.5f}; TI {ev.log_z_ti:.5f} +- "
          f"{ev.se_log_z_ti:.5f}, discretisation {ev.ti_discretisation:.5f}")
    assert abs(ev.log_z_ss - naive) <= 4 * (ev.se_log_z_ss + se_naive)
    assert abs(ev.log_z_ti - naive) <= 4 * (ev.se_log_z_ti + se_naive) + 2 * ev.ti_discretisation
