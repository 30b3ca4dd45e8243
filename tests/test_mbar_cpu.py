"""MBAR without a GPU: the float64 reference (tests/mbar_ref.py) on the analytic Gaussian ladder -- log Z against the truth in
units of its own standard error, the K x K covariance against the N x N form, the normalisation of the weight matrix, expanded
draws against (distinct, multiplicity) -- and the host helpers of rungs.py: mbar_covariance, mbar_compare, the Gamma conditional
of a regression's eta, systematic resampling."""
import math

import numpy as np
import pytest

import mbar_ref as ref

from ptnn_amd import parallel_tempering as pt_module, rungs


def _solve_ladder(K, n=500, seed=5):
    u, betas, truth = ref.gaussian_ladder(K, n, seed)
    uu, b, c = u.reshape(-1), np.zeros(K * n), np.ones(K * n)
    g, n_k = np.ones(K), np.full(K, float(n))
    f, D, n_iter, resid = ref.solve(uu, b, c, betas, g, n_k)
    W = ref.weight_matrix(uu, b, betas, g, f, D)
    return dict(u=uu, b=b, c=c, betas=betas, g=g, n_k=n_k, f=f, D=D, W=W, n_iter=n_iter, resid=resid, truth=truth)


@pytest.mark.parametrize("K", [4, 16])
def test_gaussian_ladder(K):
    r = _solve_ladder(K)
    assert r["resid"] <= 1e-10 and r["n_iter"] <= 64
    theta = ref.theta_kk(ref.gram(r["W"], r["c"]), r["n_k"])
    log_z = -(r["f"][-1] - r["f"][0])
    se = math.sqrt(theta[0, 0] + theta[-1, -1] - 2 * theta[0, -1])
    print(f"K = {K}: log Z {log_z:.6f}, truth {r['truth']:.6f}, SE {se:.6f}, z {(log_z - r['truth']) / se:.3f}, sweeps {r['n_iter']}")
    assert 0 < se < 0.1 and abs(log_z - r["truth"]) <= 4 * se
    np.testing.assert_allclose(r["c"] @ r["W"], 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(rungs.mbar_covariance(ref.gram(r["W"], r["c"]), r["n_k"]), theta)
    # the weights at the coldest state are its column of W
    lw = ref.target_log_weights(r["u"], r["b"], r["c"], r["D"], r["betas"][-1])
    np.testing.assert_allclose(np.exp(lw), r["W"][:, -1], rtol=1e-12)


def test_theta_forms_agree():
    r = _solve_ladder(4)
    a, b = ref.theta_kk(ref.gram(r["W"], r["c"]), r["n_k"]), ref.theta_nn(r["W"], r["n_k"])
    print(f"largest |difference| of the two forms {np.max(np.abs(a - b)):.2e} at magnitude {np.max(np.abs(a)):.2e}")
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


def test_expanded_draws_equal_multiplicities():
    u, betas, _ = ref.gaussian_ladder(4, 60, 8)
    mult = (np.arange(240) * 7 % 4).reshape(4, 60)                # zeros included
    g = np.ones(4)
    n_k = mult.sum(axis=1).astype(np.float64)
    f_m, D_m, _, _ = ref.solve(u.reshape(-1), np.zeros(240), mult.reshape(-1), betas, g, n_k)
    ue = np.repeat(u.reshape(-1), mult.reshape(-1))
    f_e, D_e, _, _ = ref.solve(ue, np.zeros(ue.size), np.ones(ue.size), betas, g, n_k)
    np.testing.assert_allclose(f_m, f_e, rtol=0, atol=1e-12)
    lw_m = ref.target_log_weights(u.reshape(-1), np.zeros(240), mult.reshape(-1), D_m, 1.0)
    lw_e = ref.target_log_weights(ue, np.zeros(ue.size), np.ones(ue.size), D_e, 1.0)
    assert ref.weight_stats(lw_m, mult.reshape(-1))[1] == pytest.approx(ref.weight_stats(lw_e, np.ones(ue.size))[1], rel=1e-12)
    assert np.isneginf(lw_m[mult.reshape(-1) == 0]).all()


def test_covariance_and_compare_on_hand_made_inputs():
    # two states that never overlap: W is block-constant, M = diag(1 / N), I - N M = 0, Theta = 0 by the pseudo-inverse
    assert np.array_equal(rungs.mbar_covariance(np.diag([0.25, 0.1]), [4, 10]), np.zeros((2, 2)))
    # two identical states of 8 draws each: W = 1 / 16 everywhere, M = J / 16, I - N M = the projector [[.5, -.5], [-.5, .5]], its own
    # pseudo-inverse, which M annihilates: the free-energy difference of identical states is known exactly
    M = np.full((2, 2), 1 / 16)
    np.testing.assert_allclose(rungs.mbar_covariance(M, [8, 8]), np.zeros((2, 2)), atol=1e-15)
    # a general 2 x 2 case by the defining identity Theta A = M A^+ A, A = I - diag(N) M
    M3 = np.array([[0.20, 0.05], [0.05, 0.15]])
    N3 = np.array([4.0, 5.0])
    A = np.eye(2) - N3[:, None] * M3
    np.testing.assert_allclose(rungs.mbar_covariance(M3, N3) @ A, M3 @ (np.linalg.pinv(A) @ A), atol=1e-14)
    for bad in (dict(gram=np.zeros((2, 3)), n_eff=[1, 1]), dict(gram=np.full((2, 2), np.nan), n_eff=[1, 1]), dict(gram=M, n_eff=[0, 1])):
        with pytest.raises(ValueError):
            rungs.mbar_covariance(**bad)
    none = [None] * len(rungs.RungWeights._fields)
    a = rungs.RungWeights(*none)._replace(log_z_mbar=-10.0, se_log_z_mbar=0.3)
    b = rungs.RungWeights(*none)._replace(log_z_mbar=-12.5, se_log_z_mbar=0.4)
    assert rungs.mbar_compare(a, b) == dict(log_bf_mbar=2.5, se_log_bf_mbar=0.5)
    assert pt_module.mbar_compare is rungs.mbar_compare and pt_module.mbar_covariance is rungs.mbar_covariance
    assert pt_module.RungWeights is rungs.RungWeights


def test_eta_conditional_is_the_gamma():
    n_rows, sse, m = 12, 0.37, 20000
    eta = rungs.redraw_eta(np.full(m, sse), n_rows, seed=3)
    t = np.exp(-eta)
    shape, rate = n_rows / 2 + 1, sse / 2
    mc_se = math.sqrt(shape) / rate / math.sqrt(m)                                      # sd of a Gamma = sqrt(shape) / rate
    print(f"mean of exp(-eta) {t.mean():.5f}, Gamma mean {shape / rate:.5f}, MC SE {mc_se:.5f}")
    assert abs(t.mean() - shape / rate) <= 4 * mc_se
    assert np.array_equal(eta, rungs.redraw_eta(np.full(m, sse), n_rows, seed=3))       # the seed fixes the draws
    with pytest.raises(ValueError, match="sse must be > 0"):
        rungs.redraw_eta([1.0, 0.0], n_rows, seed=3)


def test_systematic_resampling():
    w = np.array([0.1, 0.0, 0.4, 0.0, 0.5, 0.0])
    cum = np.cumsum(w)
    assert ref.systematic_resample(cum, 0.5, 4).tolist() == [2, 2, 4, 4]                # thresholds 0.125, 0.375, 0.625, 0.875
    assert ref.systematic_resample(cum, 0.25, 1).tolist() == [2]
    assert ref.systematic_resample(cum, 0.5, 1).tolist() == [4]                         # item 2 holds [0.1, 0.5): its end is item 4's
    counts = np.bincount(ref.systematic_resample(cum, 0.25, 1000), minlength=6)
    assert counts.tolist() == [100, 0, 400, 0, 500, 0]
    assert ref.systematic_resample(np.array([0.5, 1.0, 1.0]), 1.0 - 1e-17, 1).tolist() == [1]   # past the end: the last positive item
    mean, var = ref.weighted_moments(np.array([[1.0], [5.0], [3.0]]), np.log([0.25, 0.25, 0.5]))
    assert mean[0] == 3.0 and var[0] == 2.0
