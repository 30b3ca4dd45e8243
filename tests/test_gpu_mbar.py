"""MBAR on the GPU (ptnn_mbar / rung_reweighting): the host-U source against the float64 reference (tests/mbar_ref.py) at the
sizes of tests/mbar_cases.py, bitwise agreement of the trace and host-vector sources and of any scratch size, systematic
resampling against the reference on the device's own running sum, refusals, and log Z end to end against naive prior Monte Carlo."""
import warnings

import numpy as np
import pytest

import evidence_ref
import mbar_cases
import mbar_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
# The device differs from mbar_ref in the order of its sums (and in fused multiply-adds) only.  Largest deviation measured over
# the cases below, relative to the largest magnitude of each output: 9.4e-15 (the Gram matrix at 65 states; f: 6.8e-15; DESIGN.md
# section 32); the bound is 8 times that.
TOL = 8 * 9.4e-15


def _pt(task, topo, train, test, R, S, path, *, lg=True, lr=0.1, maxtemp=2, si=10, burn_in=0.5, seed=SEED, **kw):
    if task == orc.TASK_REG:
        from ptnn_amd.pt_timeseries_regression import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, 0.5, str(path), seed=seed, write_files=False, **kw)
    else:
        from ptnn_amd.pt_classification import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, str(path), seed=seed, write_files=False, **kw)
    pt.initialize_chains(burn_in)
    return pt


def _quiet(f, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **kw)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """A short classification run: the handle of the host-U cases, the trace of the source comparison."""
    d = parity.datasets()
    pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 4, 200, tmp_path_factory.mktemp("mbar"), lr=0.01, maxtemp=10)
    pt.run_chains()
    return pt


def _dev(a, b):
    """The largest deviation of a from b relative to the largest magnitude of b, over the finite entries (the others must agree)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin])
    return float(np.max(np.abs(a[fin] - b[fin])) / max(float(np.max(np.abs(b[fin]))), 1e-300)) if fin.any() else 0.0


def _reference(c, out, target_beta):
    """mbar_ref on the case with the device's N_k (effective: its ESS) and its sweep count."""
    R, n = c["u"].shape
    m = c["u_prior"].size
    mult = np.ones((R, n)) if c["multiplicity"] is None else c["multiplicity"].astype(np.float64)
    n_k = out["n_eff"]
    scale = n_k[1:] / mult.sum(axis=1)                                        # 1 without `effective`
    cw = np.concatenate([np.ones(m), (mult * scale[:, None]).reshape(-1)])
    u = np.concatenate([c["u_prior"], c["u"].reshape(-1)])
    b = np.zeros(u.size) if c["b"] is None else np.concatenate([c["b_prior"], c["b"].reshape(-1)])
    betas, g = np.concatenate([[0.0], c["betas"]]), np.concatenate([[0.0], np.ones(R)])
    f, D, n_iter, resid = ref.solve(u, b, cw, betas, g, n_k, tol=0.0, max_iter=out["n_iter"])
    W = ref.weight_matrix(u, b, betas, g, f, D)
    lw = ref.target_log_weights(u, b, cw, D, target_beta)
    return dict(f=f, gram=ref.gram(W, cw), lw=lw, stats=ref.weight_stats(lw, cw), resid=resid, cw=cw, W=W, n_k=n_k)


@pytest.mark.parametrize("effective", [False, True], ids=["counts", "effective"])
@pytest.mark.parametrize("with_mult", [False, True], ids=["plain", "multiplicities"])
@pytest.mark.parametrize("name", list(mbar_cases.SIZES))
def test_host_u_against_the_reference(run, name, with_mult, effective):
    c = mbar_cases.case(name, with_b=name.startswith("K5"), with_mult=with_mult)
    tb = 1.0 if name.startswith("K2") else float(c["betas"][-2])             # a rung other than the coldest, too
    out = run._sampler.mbar(c["betas"], u=c["u"], b=c["b"], multiplicity=c["multiplicity"], u_prior=c["u_prior"], b_prior=c["b_prior"],
                            effective=effective, target_beta=tb, item_map=True)
    R, n = c["u"].shape
    m0 = c["u_prior"].size
    assert np.array_equal(out["item_chain"], np.concatenate([np.full(m0, -1), np.repeat(np.arange(R), n)]))
    assert np.array_equal(out["item_step"], np.concatenate([np.arange(m0), np.tile(np.arange(n), R)]))
    assert np.array_equal(out["item_multiplicity"][m0:].reshape(R, n), np.ones((R, n), np.int32) if c["multiplicity"] is None else c["multiplicity"])
    assert out["n_items"] == c["u_prior"].size + R * n and out["n_distinct"] == 0
    assert out["residual"] <= 1e-10 and 8 <= out["n_iter"] <= 10000 and out["n_iter"] % 8 == 0
    if not effective:
        counts = np.full(R, n) if c["multiplicity"] is None else c["multiplicity"].sum(axis=1)
        assert np.array_equal(out["n_eff"], np.concatenate([[c["u_prior"].size], counts]))
    else:
        conv = run._sampler.convergence(draws=np.ascontiguousarray(c["u"].T[None].astype(np.float32))) if c["multiplicity"] is None else None
        if conv is not None:                                                  # the split ESS of the rung's U draws, or 1 without one
            ess = conv["ess"]
        else:                                                                 # rungs of unequal length: each one's expanded draws
            ess = np.array([run._sampler.convergence(draws=np.ascontiguousarray(
                np.repeat(c["u"][k], c["multiplicity"][k])[None, :, None].astype(np.float32)))["ess"][0] for k in range(R)])
        assert np.array_equal(out["n_eff"][1:], np.where(np.isfinite(ess) & (ess > 0), ess, 1.0))
        assert out["n_eff"][0] == c["u_prior"].size
    r = _reference(c, out, tb)
    dev = dict(f=_dev(out["f"], r["f"]), gram=_dev(out["gram"], r["gram"]), log_weight=_dev(out["log_weight"], r["lw"]),
               kish_ess=_dev(out["kish_ess"], r["stats"][1]), max_weight_share=_dev(out["max_weight_share"], r["stats"][2]),
               weight_sum=abs(out["weight_sum"] - 1.0), columns=float(np.max(np.abs(r["cw"] @ r["W"] - 1.0))))
    print(f"{name} mult={with_mult} eff={effective}: sweeps {out['n_iter']}, residual {out['residual']:.2e}, deviations "
          + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    assert out["f"][0] == 0.0 and np.array_equal(out["gram"], out["gram"].T)
    for k, v in dev.items():
        assert v <= (1e-12 if k == "columns" else TOL), (k, v)
    if c["multiplicity"] is not None:
        assert np.isneginf(out["log_weight"][c["u_prior"].size:][c["multiplicity"].reshape(-1) == 0]).all()


def test_items_of_multiplicity_zero_are_inert(run):
    """A host row of multiplicity 0 may hold anything: every output that is not its own stays bit for bit."""
    c = mbar_cases.case("K5_past_a_work_group", with_b=True, with_mult=True)
    zero = c["multiplicity"] == 0
    kw = dict(multiplicity=c["multiplicity"], u_prior=c["u_prior"], b_prior=c["b_prior"], n_resample=50, resample_seed=5)
    clean = run._sampler.mbar(c["betas"], u=c["u"], b=c["b"], **kw)
    dirty = run._sampler.mbar(c["betas"], u=np.where(zero, np.nan, c["u"]), b=np.where(zero, np.inf, c["b"]), **kw)
    for k in ("f", "gram", "n_eff", "log_weight", "cum_weight", "resample_item", "kish_ess", "max_weight_share", "weight_sum", "n_iter"):
        assert np.array_equal(clean[k], dirty[k]), k
    assert np.all(np.isfinite(dirty["gram"]))


def test_resampling_against_the_reference(run):
    from ptnn_amd import philox
    c = mbar_cases.case("K5_past_a_work_group", with_b=False, with_mult=True)
    for m in (1, 33, 700):
        out = run._sampler.mbar(c["betas"], u=c["u"], multiplicity=c["multiplicity"], u_prior=c["u_prior"], n_resample=m, resample_seed=77)
        assert out["resample_u"] == philox.resample_uniform(77)
        cum = out["cum_weight"]
        np.testing.assert_allclose(cum, np.cumsum(np.exp(out["log_weight"])), rtol=1e-13)
        assert np.all(np.diff(cum) >= 0) and cum[-1] == pytest.approx(1.0, abs=1e-12)
        assert np.array_equal(out["resample_item"], ref.systematic_resample(cum, out["resample_u"], m))
        assert np.all(np.isfinite(out["log_weight"][out["resample_item"]]))                 # no item of weight 0 is ever drawn
    # many draws: the counts follow the weights to within one draw per item
    counts = np.bincount(out["resample_item"], minlength=cum.size)
    assert np.all(np.abs(counts - 700 * np.exp(out["log_weight"])) < 1.0)


# The expectations differ from mbar_ref in the order of their sums only.  Largest deviation of mean and var measured on the case
# below, relative to the largest magnitude of each: 9.0e-16 for the mean, 5.6e-16 for the variance; the
# bound is 8 times the larger.
EXPECT_MEASURED = 9.0e-16
EXPECT_TOL = 8 * EXPECT_MEASURED


def test_expectations_and_vectors_against_the_reference(run):
    """mean / var on 7 rows against mbar_ref on the device's own outputs and log weights; the resampled vectors against the
    trace rows and the device's prior draws.  The target is the hottest rung, where prior draws carry weight."""
    pt = run
    S = pt.NumSamples
    step0, end = int(S * pt.burn_in), pt._pt_switch_step()
    betas = np.array([1.0 / float(np.float32(T)) for T in pt.temperatures])
    order = [int(k) for k in np.argsort(betas, kind="stable")]
    X7 = np.ascontiguousarray(np.asarray(parity.datasets()["iris_test"])[:7, :4], np.float32)
    src = dict(replicas=order, step0=step0, nsteps=end - step0, thin=1)
    NP = 300                                                                  # more than one chunk of 256, with a tail
    out = pt._sampler.mbar(betas[order], n_prior=NP, seed=SEED, target_beta=float(betas[order][0]), x=X7, n_resample=64, resample_seed=3,
                           resample_w=True, item_map=True, **src)
    # the items' outputs: the prior draws' vectors as the device forms them, then the rungs' rows, through ptnn_predict
    Wp = pt._sampler.prior_predictive(X7, n_draws=NP, seed=SEED, weights=True)["weights"][0]
    fp = pt._sampler.predict(X7, w=Wp, samples=True, mean=False)["samples"]
    fr = pt._sampler.predict(X7, samples=True, mean=False, **src)["samples"]
    mean, var = ref.weighted_moments(np.concatenate([fp, fr]), out["log_weight"])
    dev = dict(mean=_dev(out["mean"], mean), var=_dev(out["var"], var))
    n_from_prior = int(np.sum(out["resample_item"] < NP))
    print(f"expectations on 7 rows, {NP} prior draws + {fr.shape[0]} rows: deviations mean {dev['mean']:.2e}, var {dev['var']:.2e}; prior "
          f"weight {np.exp(out['log_weight'][:NP]).sum():.3f}, {n_from_prior} of 64 resampled draws are prior draws")
    for k, v in dev.items():
        assert v <= EXPECT_TOL, (k, v)
    full = pt._sampler.traces()["pos_w"]
    per = end - step0
    for v, it in zip(out["resample_w"], out["resample_item"]):
        want = Wp[it] if it < NP else full[order[(it - NP) // per], step0 + (it - NP) % per]
        assert np.array_equal(v, want)
    # the map of the items: prior draws first, then every rung's rows by (chain, step)
    assert np.array_equal(out["item_chain"], np.concatenate([np.full(NP, -1), np.repeat(order, per)]))
    assert np.array_equal(out["item_step"], np.concatenate([np.arange(NP), np.tile(np.arange(step0, end), 4)]))
    assert np.all(out["item_multiplicity"] == 1)
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="a classification has no sum of squared errors"):
        pt._sampler.mbar(betas[order], sse=True, **src)
    for bad in (dict(u=np.zeros((4, 8)), x=X7), dict(u=np.zeros((4, 8)), n_resample=3, resample_w=True)):
        with pytest.raises(_lib.PtnnError, match="need the items' weight vectors"):
            pt._sampler.mbar(betas[order], **bad)


def _same(a, b):
    for k in a._fields:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=True), k
        else:
            assert x == y or (x != x and y != y), k


def test_sources_and_scratch_sizes_agree(run, monkeypatch):
    pt = run
    S = pt.NumSamples
    step0, end = int(S * pt.burn_in), pt._pt_switch_step()
    betas = np.array([1.0 / float(np.float32(T)) for T in pt.temperatures])
    W = pt._sampler.traces(step0, end - step0)["pos_w"]
    X7 = np.asarray(parity.datasets()["iris_test"])[:7]
    kw = dict(x=X7, prior_draws=512, resample=40)                             # two blocks of prior draws under the small scratch
    tr = _quiet(pt.rung_reweighting, **kw)
    assert tr.mean.shape == tr.sd.shape == (7, 3) and np.all(tr.sd > 0)
    np.testing.assert_allclose(tr.mean.sum(axis=1), 1.0, atol=1e-6)           # class probabilities
    perm = np.arange(W.shape[0])[::-1]                                        # host vectors of the same rows, in any rung order
    hv = _quiet(pt.rung_reweighting, weights=(betas[perm], np.ascontiguousarray(W[perm])), **kw)
    monkeypatch.setenv("PTNN_EVIDENCE_SCRATCH_BYTES", "20000")
    small = _quiet(pt.rung_reweighting, **kw)
    monkeypatch.setenv("PTNN_EVIDENCE_SCRATCH_BYTES", "300000")
    mid = _quiet(pt.rung_reweighting, **kw)
    monkeypatch.delenv("PTNN_EVIDENCE_SCRATCH_BYTES")
    _same(small, tr)
    _same(mid, tr)
    _same(hv._replace(index=tr.index), tr)                                    # the index names rows of `weights` there
    from_rungs = tr.index[:, 0] >= 0
    assert np.array_equal(hv.index[from_rungs, 0], perm.argsort()[tr.index[from_rungs, 0]])
    assert np.array_equal(hv.index[from_rungs, 1], tr.index[from_rungs, 1] - step0)
    # what the result says: finite, normalised, the resampled vectors are the trace's rows
    assert np.isfinite(tr.log_z_mbar) and tr.se_log_z_mbar > 0 and tr.free_energy[0] == 0.0
    total = np.exp(tr.log_weights).sum() + np.exp(tr.prior_log_weights).sum()
    assert total == pytest.approx(1.0, abs=1e-9)
    assert tr.log_weights.shape == (4, end - step0) and tr.cold_draws == end - step0 and tr.vectors.shape == (40, pt.num_param)
    full = pt._sampler.traces()["pos_w"]
    for v, (chain, step) in zip(tr.vectors[from_rungs], tr.index[from_rungs]):
        assert np.array_equal(v, full[chain, step])
    assert tr.eta is None
    pp = pt.posterior_predictive("test", weights=tr.vectors)
    assert pp.n_samples == 40 and np.all(np.isfinite(pp.mean))
    # a target inside the ladder, and no prior state: differences of free energies only
    inner = _quiet(pt.rung_reweighting, include_prior=False, target_beta=float(np.sort(betas)[1]), effective=False)
    assert np.isnan(inner.log_z_mbar) and inner.prior_log_weights is None and inner.free_energy.shape == (4,)
    assert np.exp(inner.log_weights).sum() == pytest.approx(1.0, abs=1e-9)


def test_no_side_effects_and_refusals(run):
    pt = run
    from ptnn_amd import _lib
    before, st = pt._sampler.traces(), pt._sampler.state()
    _quiet(pt.rung_reweighting, prior_draws=128, resample=8)
    after, st2 = pt._sampler.traces(), pt._sampler.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for k in st:
        assert np.array_equal(np.asarray(st[k]), np.asarray(st2[k])), k
    u = np.zeros((2, 8))
    for kw, text in ((dict(betas=[0.5, 1.0], u=np.zeros((2, 3))), "split ESS"),
                     (dict(betas=[1.0, 0.5], u=u), "rise strictly"),
                     (dict(betas=[0.0, 1.0], u=u), "finite and > 0"),
                     (dict(betas=[0.5, 1.0], u=u, target_beta=0.25), "outside the ladder"),
                     (dict(betas=[0.5, 1.0], u=u, tol=0.0), "tol = 0"),
                     (dict(betas=[0.5, 1.0], u=u, max_iter=0), "max_iter = 0"),
                     (dict(betas=[0.5, 1.0], u=u, n_resample=-1), "n_resample = -1"),
                     (dict(betas=[0.5, 1.0], u=u, multiplicity=-np.ones((2, 8), np.int32)), "is negative"),
                     (dict(betas=[0.5, 1.0], u=np.full((2, 8), np.nan)), "not finite"),
                     (dict(betas=np.linspace(0.01, 1, 513), u=np.zeros((513, 4))), "at most 512"),
                     (dict(betas=[0.5, 1.0], replicas=[0, 1, 2]), "3 chains selected for 2 betas")):
        with pytest.raises((_lib.PtnnError, ValueError), match=text):
            pt._sampler.mbar(**kw)


def test_log_z_against_naive_monte_carlo(tmp_path):
    """End to end on the 12-row regression 4-3-1 problem of test_gpu_evidence.py, same settings (random walk, swap_rule=1,
    shared_noise=False, 16 chains, maxtemp 1000, S = 40 000), against log c + log mean e^{b + U} over 2^22 prior draws in numpy
    float64: within 4 combined standard errors, and the reweighted sample is worth at least the cold rung's."""
    rng = np.random.default_rng(11)
    x = rng.random((12, 4))
    data = np.column_stack([x, 0.2 + 0.6 * x[:, 0] * x[:, 1] + 0.05 * rng.standard_normal(12)])
    topo = (4, 3, 1)
    pt = _pt(orc.TASK_REG, topo, data, data, 16, 40000, tmp_path, lg=False, maxtemp=1000, si=5, burn_in=0.25, swap_rule=1,
             shared_noise=False)
    pt.run_chains()
    rw = _quiet(pt.rung_reweighting, prior_draws=1 << 20, resample=64)
    naive, se_naive = evidence_ref.naive_log_z(orc.TASK_REG, data, topo, 1 << 22, 5.0, seed=9)
    print(f"naive {naive:.5f} +- {se_naive:.5f}; MBAR {rw.log_z_mbar:.5f} +- {rw.se_log_z_mbar:.5f} after {rw.n_iter} sweeps (residual "
          f"{rw.residual:.2e}); Kish ESS {rw.kish_ess:.1f} against the cold rung's {rw.n_eff[-1]:.1f}: gain {rw.ess_gain:.2f}; largest "
          f"share {rw.max_weight_share:.2e}")
    assert rw.residual <= 1e-10
    assert abs(rw.log_z_mbar - naive) <= 4 * (rw.se_log_z_mbar + se_naive)
    assert rw.ess_gain >= 1
    # the resampled draws go straight into the analysis calls: vectors and the redrawn eta
    assert rw.vectors.shape == (64, pt.num_param) and rw.eta.shape == (64,) and rw.index.shape == (64, 2)
    pc = pt.predictive_calibration("train", weights=rw.vectors, eta=rw.eta)
    assert np.all(np.isfinite(pc.pit))
