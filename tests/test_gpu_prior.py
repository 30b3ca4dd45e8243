"""Prior predictive checks on the GPU (ptnn_prior_predictive / prior_predictive) on the Sunspot 4-5-1 handle that
initialize_chains() makes: the drawn vectors against philox.py, the per-column results against posterior_predictive on the same
vectors (bitwise), the saturation counts, function statistics, summaries and counts against the float64 reference
(tests/prior_ref.py) fed the device's own outputs, bitwise independence of the block size, continuation with draw0, side effects,
the budget refusal, and the constructor's sigma_squared."""
import math

import numpy as np
import pytest

import parity
import prior_ref as ref
from parity import orc
from test_gpu_predict import _pt
from test_prior_cpu import ATOL, GPU_SEED, RTOL

pytestmark = pytest.mark.gpu

PCTS = (0, 5, 50, 95, 100, 37.5)
N_ROWS, N_DRAWS = 70, 100          # one 64-row tile and a ragged one; a multiple of neither 16 nor 64
SCALES = (1.0, 25.0)
EPS = 0.01
LOW_KEYS = ("mean", "order_stats", "vote", "sat_count", "t_obs", "stat_mean", "stat_sd", "stat_order_stats", "n_greater", "n_equal",
            "n_defined", "t_draw", "samples", "weights")


def _rows(d, name, I):
    return np.ascontiguousarray(np.asarray(d[name])[:N_ROWS, :I + 1], dtype=np.float32)


def _run(pt, x, scales, n=N_DRAWS, **kw):
    return pt.prior_predictive(x, n_draws=n, sigma_squared=scales, percentiles=PCTS, seed=GPU_SEED, eps=EPS, target=True,
                               return_draws=True, return_samples=True, return_weights=True, **kw)


def _low(pt, x, scales, n=N_DRAWS):
    from ptnn_amd.analysis import percentile_ranks
    ranks = sorted({r for lo, hi, _ in percentile_ranks(n, PCTS) for r in (lo, hi)})
    return pt._sampler.prior_predictive(x, n_draws=n, sigma_squared=scales, seed=GPU_SEED, ranks=ranks, eps=EPS, target=True,
                                        t_draw=True, samples=True, weights=True)


def check_columns(pt, x, res):
    """Check 2: mean, every percentile and the votes are posterior_predictive's on the same vectors, bit for bit."""
    I = int(pt.topology[0])
    for s in range(len(res.sigma_squared)):
        pp = pt.posterior_predictive(x[:, :I], weights=res.weights[s], percentiles=PCTS, return_samples=True)
        assert pp.n_distinct == pp.n_samples == res.n_draws
        assert np.array_equal(res.samples[s], pp.samples)
        assert np.array_equal(res.mean[s], pp.mean)
        for p in PCTS:
            assert np.array_equal(res.percentiles[p][s], pp.percentiles[p]), p
        if pt.task == orc.TASK_CLS:
            assert np.array_equal(res.vote[s], pp.vote)
        else:
            assert res.vote is None


def check_saturation(res):
    """Check 3: the saturation shares are the counts of the returned samples, exactly."""
    f = res.samples.astype(np.float64)
    count = np.sum((f < res.eps) | (f > 1.0 - res.eps), axis=1)
    assert np.array_equal(res.saturated, count / float(res.n_draws))


def check_statistics(pt, x, res):
    """Checks 4 and 5: the function statistics, their summaries and the counts against the reference on the returned samples."""
    I = int(pt.topology[0])
    y = x[:, I].astype(np.float64)
    fn = ref.regression if pt.task == orc.TASK_REG else ref.classification
    n_cls = 0 if pt.task == orc.TASK_REG else int(pt.topology[2])
    for s in range(len(res.sigma_squared)):
        t, t_obs = fn(res.samples[s], y, res.eps)
        assert res.t_draw[s].shape == t.shape == (res.n_draws, len(res.names))
        err = np.abs(res.t_draw[s] - t)
        print(f"scale {res.sigma_squared[s]}: t_draw max abs diff {np.nanmax(err):.3e}; undefined draws per statistic "
              f"{np.isnan(t).sum(axis=0).tolist()}")
        np.testing.assert_allclose(res.t_draw[s], t, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose([res.t_obs[n] for n in res.names], t_obs, rtol=RTOL, atol=ATOL)
        want = ref.summarise(t, t_obs)
        np.testing.assert_allclose([res.stat_mean[n][s] for n in res.names], want["mean"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose([res.stat_sd[n][s] for n in res.names], want["sd"], rtol=RTOL, atol=ATOL)
        # the order statistics over the draws: the fp32-rounded statistic, numpy's percentile of it
        for p in PCTS:
            for j, n in enumerate(res.names):
                col = res.t_draw[s][:, j].astype(np.float32)
                if not np.isnan(col).any():
                    assert res.stat_percentiles[p][n][s] == np.percentile(col.astype(np.float64), p), (p, n)
        # counts: equal to the reference's, but for draws within the tolerance of T(y) (at most 1 % per statistic);
        # class shares are integer counts over the same rows: exact
        close = ref.close_draws(t, t_obs, RTOL, ATOL).sum(axis=0)
        for j, n in enumerate(res.names):
            exact = j >= len(res.names) - n_cls
            slack = 0 if exact else int(close[j])
            assert slack <= res.n_draws // 100, (n, slack)
            assert res.n_defined[n][s] == want["n_defined"][j], n
            assert abs(int(res.n_greater[n][s]) - int(want["n_greater"][j])) <= slack, n
            assert abs(int(res.n_equal[n][s]) - int(want["n_equal"][j])) <= slack, n
            got_p = res.p_value[n][s]
            if math.isnan(t_obs[j]):
                assert math.isnan(got_p) and res.n_greater[n][s] == 0 and res.n_equal[n][s] == 0
            elif slack == 0:
                assert got_p == want["p_value"][j] or (math.isnan(got_p) and math.isnan(want["p_value"][j]))


def check_blocks(pt, x, scales, monkeypatch, n=N_DRAWS):
    """Check 6: draws generated in three blocks, the last one ragged, give every output bit for bit."""
    I, O = int(pt.topology[0]), int(pt.topology[2])
    whole = _low(pt, x, scales, n)
    assert whole["n_blocks"] == 1
    nb = 2 * n // 5
    assert n % nb and -(-n // nb) == 3
    per_draw = 4 * pt.num_param + 8 + 4 * N_ROWS * O               # include/ptnn.h: what a block holds per draw
    monkeypatch.setenv("PTNN_PRIOR_SCRATCH_BYTES", str(4 * N_ROWS * O * n + nb * per_draw))
    cut = _low(pt, x, scales, n)
    monkeypatch.delenv("PTNN_PRIOR_SCRATCH_BYTES")
    assert cut["n_blocks"] == 3 and cut["n_stats"] == whole["n_stats"]
    for k in LOW_KEYS:
        if whole[k] is None:
            assert cut[k] is None, k
        else:
            assert np.array_equal(whole[k], cut[k], equal_nan=True), k
    return whole


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path_factory.mktemp("sun"))
    x = _rows(d, "sunspot_train", 4)
    return pt, x, _run(pt, x, SCALES)


def test_drawn_vectors(sunspot):
    """Check 1: w = float32(sqrt(s)) z with philox.prior_weights' z; the wide scale is exactly 5 times the unit one."""
    from ptnn_amd import philox
    pt, x, res = sunspot
    assert res.sigma_squared == SCALES and res.weights.shape == (2, N_DRAWS, pt.num_param) and res.seed == GPU_SEED
    for s, s2 in enumerate(SCALES):
        want = np.stack([philox.prior_weights(GPU_SEED, i, pt.num_param, math.sqrt(s2)) for i in range(N_DRAWS)])
        err = np.abs(res.weights[s] - want)
        print(f"scale {s2}: max abs diff {err.max():.3e}, max rel diff {np.max(err / np.maximum(np.abs(want), 1e-30)):.3e}")
        # the constant tests/test_gpu_evidence.py holds the prior draws to -- there on U, a quantity derived from them, so it
        # is loose for weights of order 1 -- and the bound the same device Box-Muller is held to as a deviate (tests/test_gpu_ppc.py's
        # z, from tests/test_gpu_forecast.py::test_noise: rtol 1e-4, atol 2e-6), the absolute part scaled by sigma
        np.testing.assert_allclose(res.weights[s], want, rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(res.weights[s], want, rtol=1e-4, atol=2e-6 * math.sqrt(s2))
    assert np.array_equal(res.weights[1], np.float32(5) * res.weights[0])
    assert len({w.tobytes() for w in res.weights[0]}) == N_DRAWS


def test_columns_match_posterior_predictive(sunspot):
    pt, x, res = sunspot
    assert res.mean.shape == res.saturated.shape == (2, N_ROWS, 1) and res.samples.shape == (2, N_DRAWS, N_ROWS, 1)
    check_columns(pt, x, res)


def test_saturation(sunspot):
    _, _, res = sunspot
    check_saturation(res)
    print("saturated share per scale:", res.saturated.mean(axis=(1, 2)).tolist())
    assert res.saturated[1].mean() > res.saturated[0].mean()      # N(0, 25) saturates the sigmoid net far more often than N(0, 1)


def test_function_statistics_and_counts(sunspot):
    pt, x, res = sunspot
    assert res.names == list(ref.REG_STATS)
    check_statistics(pt, x, res)
    assert math.isnan(res.p_value["rmse"][0]) and math.isnan(res.p_value["saturated"][1]) and not math.isnan(res.p_value["acf1"][0])
    # "train" brings its targets along; an array without target: no rmse, no T(y), no p-value
    tr = pt.prior_predictive("train", n_draws=8, seed=GPU_SEED)
    assert tr.sigma_squared == (25.0,) and tr.mean.shape == (1, len(pt.traindata), 1) and tr.t_draw is None and tr.weights is None
    assert not math.isnan(tr.t_obs["mean"]) and not math.isnan(tr.stat_mean["rmse"][0])
    bare = pt.prior_predictive(x[:, :4], n_draws=8, seed=GPU_SEED, sigma_squared=25.0)
    assert all(math.isnan(v) for v in bare.t_obs.values()) and math.isnan(bare.stat_mean["rmse"][0]) and bare.n_defined["rmse"][0] == 0
    assert all(math.isnan(v[0]) for v in bare.p_value.values())
    assert np.array_equal(bare.mean[0], pt.prior_predictive(x, n_draws=8, seed=GPU_SEED, target=True).mean[0])
    # the seed defaults to the object's
    assert np.array_equal(pt.prior_predictive(x[:, :4], n_draws=8).mean, pt.prior_predictive(x[:, :4], n_draws=8, seed=pt.seed).mean)


def test_block_independence(sunspot, monkeypatch):
    pt, x, res = sunspot
    whole = check_blocks(pt, x, SCALES, monkeypatch)
    assert np.array_equal(whole["t_draw"], res.t_draw, equal_nan=True) and np.array_equal(whole["samples"], res.samples)


def test_continuation(sunspot):
    """Check 7: draws [0, 37) and [37, 100) are the per-draw outputs of draws [0, 100), bit for bit."""
    pt, x, res = sunspot
    a, b = _run(pt, x, SCALES, n=37), _run(pt, x, SCALES, n=N_DRAWS - 37, draw0=37)
    for k in ("weights", "samples", "t_draw"):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=1), getattr(res, k), equal_nan=True), k


def test_no_side_effects(tmp_path):
    """Check 8: a run continued after the call is the run without it, bit for bit (tests/test_gpu_predict.py's)."""
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path / str(call))
        assert pt.run_chains(max_steps=70) is None
        if call:
            res = _run(pt, _rows(d, "sunspot_train", 4), SCALES)
            assert res.n_draws == N_DRAWS
        res = pt.run_chains()
        outs.append((res, pt._sampler.traces(), pt._sampler.trace_rows(), pt._sampler.state(), pt._sampler.swap_stats()))
    (ra, ta, rwa, sa, wa), (rb, tb, rwb, sb, wb) = outs
    for u, v in zip(ra, rb):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    assert np.array_equal(rwa, rwb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert wa == wb


def test_budget_refusal(sunspot, monkeypatch):
    """Check 9: the refusal names the largest n_draws that fits."""
    from ptnn_amd import _lib
    pt, x, _ = sunspot
    monkeypatch.setenv("PTNN_PRIOR_SCRATCH_BYTES", str(4 * N_ROWS * 50 + 3))
    with pytest.raises(_lib.PtnnError, match="largest n_draws that fits is 50 "):
        _run(pt, x, SCALES)
    assert _run(pt, x, SCALES, n=50).n_draws == 50
    with pytest.raises(_lib.PtnnError, match="rank 7 outside \\[0, 5\\)"):
        pt._sampler.prior_predictive(x, n_draws=5, ranks=[0, 7], target=True)


def test_constructor_sigma_squared(tmp_path):
    """Check 10: sigma_squared=4 reaches the device's prior, in evaluate and in the chains' state, and is the scale
    prior_predictive draws at by default.  The 50 steps run without a swap round (swap_interval 100): a swap of the reference's
    cascade moves (w, eta) and leaves the receiving chain's prior_current stale until its next accepted step,
    whatever the prior's scale, so only a chain's own steps tie prior_current to its state."""
    d = parity.datasets()
    topo = (4, 5, 1)
    pt = _pt(orc.TASK_REG, topo, d["sunspot_train"], d["sunspot_test"], 4, 51, tmp_path, si=100, sigma_squared=4)
    rng = np.random.default_rng(7)
    W = rng.standard_normal((6, pt.num_param)).astype(np.float32)
    tau = np.array([0.5, 1.0, 2.0, 0.1, 0.03, 4.0], np.float32)
    want = [orc.prior_reg(4.0, 0.0, 0.0, W[k].astype(np.float64), float(tau[k]), topo) for k in range(6)]
    np.testing.assert_allclose(pt._sampler.evaluate(W, tau)[:, 5], want, rtol=2e-6, atol=1e-4)   # tests/test_gpu_parity.py's F3 bound
    assert not np.allclose(want, [orc.prior_reg(25.0, 0.0, 0.0, W[k].astype(np.float64), float(tau[k]), topo) for k in range(6)], rtol=1e-3)
    pt._sampler.run(50)
    pt._sampler.sync()
    st = pt._sampler.state()
    assert pt._sampler.steps_done() == 50
    print("accepted steps per chain:", st["num_accepted"].tolist(), "swap statistics:", pt._sampler.swap_stats())
    again = pt._sampler.evaluate(st["w"], np.exp(st["eta"].astype(np.float64)).astype(np.float32))[:, 5]
    np.testing.assert_allclose(st["prior"], again, rtol=2e-6, atol=1e-4)
    x = _rows(d, "sunspot_train", 4)
    own = pt.prior_predictive(x, n_draws=20, seed=GPU_SEED, target=True, return_weights=True)
    four = pt.prior_predictive(x, n_draws=20, seed=GPU_SEED, target=True, return_weights=True, sigma_squared=4.0)
    assert own.sigma_squared == (4.0,) and np.array_equal(own.weights, four.weights) and np.array_equal(own.mean, four.mean)
    from ptnn_amd import philox
    assert np.array_equal(own.weights[0], np.float32(2) * _run(pt, x, (1.0,), n=20).weights[0])
    np.testing.assert_allclose(own.weights[0, 3], philox.prior_weights(GPU_SEED, 3, pt.num_param, 2.0), rtol=1e-4, atol=1e-3)
