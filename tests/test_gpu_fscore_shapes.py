"""Forecast verification (ptnn_forecast_score) at every compiled regression shape, on both sides of the edge
between the two layouts of forecast_forward_kernel (P <= 96 parameters: one trajectory per lane; above: one vector per
work-group): the means and the noisy paths against ptnn_predict and ptnn_forecast bitwise, every score against the float64
restatement of tests/fscore_ref.py.  70 host vectors (one full wave and a partial one) with their own eta, so no case needs a
sampling run."""
import math

import numpy as np
import pytest

import parity
from test_gpu_forecast import _teacher
from test_gpu_fscore import QS, _check_against_ref

pytestmark = pytest.mark.gpu

H = 6
SEED = 0xF5C0_0000_0007
SHAPES = [(4, 15, 1), (4, 16, 1), (5, 13, 1), (5, 14, 1), (32, 2, 1), (32, 3, 1), (32, 96, 1)]


def _case(topo, seed):
    I, Hd, _ = topo
    P = I * Hd + Hd + Hd + 1
    rng = np.random.default_rng(seed)
    data = rng.uniform(0.05, 0.95, (40, I + 1))
    scale = np.concatenate([np.full(I * Hd, 2.0 / math.sqrt(I)), np.full(Hd, 2.0 / math.sqrt(Hd)), np.full(Hd, 0.5), np.full(1, 0.5)])
    w = ((rng.standard_normal(P)[None, :] + 0.5 * rng.standard_normal((70, P))) * scale[None, :]).astype(np.float32)
    eta = rng.uniform(-6.0, -3.0, 70).astype(np.float32)
    origins = rng.uniform(0.05, 0.95, (3, I)).astype(np.float32)
    truth = rng.uniform(0.1, 0.9, (3, H)).astype(np.float32)
    truth[1, 4] = np.nan
    return P, data, w, eta, origins, truth


@pytest.mark.parametrize("topo", SHAPES, ids=lambda t: "-".join(map(str, t)))
def test_shape(topo):
    P, data, w, eta, origins, truth = _case(topo, 100 + topo[0] * 1000 + topo[1])
    assert (P <= 96) == (topo in ((4, 15, 1), (5, 13, 1), (32, 2, 1)))                 # lane / split
    s = parity.make_sampler(0, topo, data[:30], data[30:], R_local=2, R_global=2, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    try:
        s.set_state(np.zeros((2, P), np.float32), np.ones(2, np.float32))
        out = s.forecast_score(H, origins, truth, w=w, eta=eta, noise=True, seed=SEED, quantiles=QS, samples=True, means=True)
        assert out["n_samples"] == out["n_trajectories"] == 70
        fc = s.forecast(H, origins, w=w, eta=eta, noise=True, seed=SEED, samples=True)
        assert np.array_equal(out["samples"], fc["samples"])
        want, _ = _teacher(s, w, origins, out["samples"])
        assert np.array_equal(out["means"], want)
        _check_against_ref(out, eta, truth, None, f"{topo} noise on")
        assert np.isnan(out["crps"]).sum() == 1
        # noise off, with multiplicities (one vector absent): one trajectory per vector, weighted
        cnt = np.random.default_rng(5).integers(1, 4, 70).astype(np.int32)
        cnt[3] = 0
        off = s.forecast_score(H, origins, truth, w=w, eta=eta, multiplicity=cnt, noise=False, quantiles=QS, samples=True, means=True)
        plain = s.forecast(H, origins, w=w, multiplicity=cnt, samples=True)
        assert off["n_samples"] == cnt.sum() and off["n_trajectories"] == plain["n_trajectories"]
        assert np.array_equal(off["samples"], off["means"]) and np.array_equal(off["samples"], plain["samples"])
        _check_against_ref(off, np.repeat(eta, cnt), truth, None, f"{topo} noise off")
    finally:
        s.close()


def _sampler_451(n_vec, seed):
    topo = (4, 5, 1)
    P, data, w70, _, origins, _ = _case(topo, seed)
    rng = np.random.default_rng(seed + 1)
    w = (w70[rng.integers(0, 70, n_vec)] + 0.3 * rng.standard_normal((n_vec, P))).astype(np.float32)
    eta = rng.uniform(-6.0, -3.0, n_vec).astype(np.float32)
    s = parity.make_sampler(0, topo, data[:30], data[30:], R_local=2, R_global=2, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    s.set_state(np.zeros((2, P), np.float32), np.ones(2, np.float32))
    return s, w, eta, np.ascontiguousarray(origins[:2]), rng


def _same_scores(a, b):
    for k in ("pit", "pred_mean", "pred_sd", "crps", "log_score", "quantiles", "energy_score", "samples", "means"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["n_samples"] == b["n_samples"]


def test_several_tiles_of_trajectories():
    """650 trajectories: three 256-wide tiles, the last one partial -- the triangle of tile pairs of the two pair kernels (six
    work-groups per column / origin, off-diagonal pairs counted twice, their limbs added by integer atomics), the dead lanes of
    the last tile, and more than one pass of every strided loop; then multiplicities (one of them 0) against the rows written
    out, bitwise, noise on (about 1300 trajectories, six tiles) and off."""
    s, w, eta, origins, rng = _sampler_451(650, 7)
    try:
        truth = rng.uniform(0.1, 0.9, (2, H)).astype(np.float32)
        truth[1, 3] = np.nan
        kw = dict(seed=SEED, quantiles=QS, samples=True, means=True)
        out = s.forecast_score(H, origins, truth, w=w, eta=eta, noise=True, **kw)
        assert out["n_trajectories"] == 650
        _check_against_ref(out, eta, truth, None, "650 trajectories, noise on")
        cnt = rng.integers(1, 4, 650).astype(np.int32)
        cnt[[5, 300, 649]] = 0
        we, ee = np.repeat(w, cnt, axis=0), np.repeat(eta, cnt)
        assert 1100 < we.shape[0] < 1536
        for noise in (True, False):
            a = s.forecast_score(H, origins, truth, w=w, eta=eta, multiplicity=cnt, noise=noise, **kw)
            b = s.forecast_score(H, origins, truth, w=we, eta=ee, noise=noise, **kw)
            _same_scores(a, b)
            assert a["n_trajectories"] == (we.shape[0] if noise else 650) and a["n_samples"] == we.shape[0]
            _check_against_ref(a, ee, truth, None, f"multiplicities, noise={noise}")
    finally:
        s.close()


def test_long_horizon_stages_the_j_paths_in_parts(monkeypatch):
    """h = 70 > 64: the energy pair kernel stages 128 j-paths at a time (all 70 steps of 256 would pass 64 KiB of LDS), two parts
    per full tile, with 300 trajectories in two tiles; every column and both origins against the reference, and one origin per block."""
    h = 70
    s, w, eta, origins, rng = _sampler_451(300, 11)
    try:
        truth = rng.uniform(0.1, 0.9, (2, h)).astype(np.float32)
        truth[0, 40] = np.nan
        truth[1, 66:] = np.nan
        kw = dict(w=w, eta=eta, noise=True, seed=SEED, quantiles=(0.5,), samples=True, means=True)
        out = s.forecast_score(h, origins, truth, **kw)
        assert out["n_trajectories"] == 300 and out["energy_score"].shape == (2,)
        _check_against_ref(out, eta, truth, None, "h = 70", levels=(0.5,))
        assert np.array_equal(out["samples"], s.forecast(h, origins, w=w, eta=eta, noise=True, seed=SEED, samples=True)["samples"])
        monkeypatch.setenv("PTNN_FSCORE_SCRATCH_BYTES", str(8 * 300 * h))
        _same_scores(out, s.forecast_score(h, origins, truth, **kw))
    finally:
        s.close()
