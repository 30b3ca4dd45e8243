"""Forecast verification on the GPU (ptnn_forecast_score / forecast_accuracy): the trajectories against
ptnn_forecast and ptnn_predict bitwise, step 1 against ptnn_calibration bitwise and ptnn_elpd, every column and origin against the
float64 restatement of tests/fscore_ref.py on the device's own means and samples, and the invariances (blocking, sources, repeats,
seeds, no side effects) and refusals with a live handle.

Largest differences to fscore_ref seen on an MI355X at this fixture (Sunspot 4-5-1, 8 chains x 600, rows 300.. every 10th: 240
trajectories, 7 origins, h = 6), as max |device - reference| / (1e-12 + 1e-9 |reference|), which the bound holds below 1:
quantiles 1.1e-5, crps 1.8e-6, log_score 8.9e-7, pit 6.8e-7, energy_score 6.0e-7, pred_mean 2.2e-7, pred_sd 1.6e-7 (DESIGN.md
section 27 has those of the shape grid as well)."""
import numpy as np
import pytest

import fscore_ref as ref
import parity
from test_gpu_forecast import SEED, _pt, _teacher

pytestmark = pytest.mark.gpu

H = 6                                   # crosses the Philox counter boundary at k = 4
QS = (0.05, 0.5, 0.95)
SEL = dict(step0=300, nsteps=300, thin=10)          # 8 chains x 30 rows = 240 samples
NOISE_SEED = 0x5EED_0000_0002
PER_COLUMN = ("pit", "pred_mean", "pred_sd", "crps", "log_score")


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    from ptnn_amd.verification import series_from_windows, windows_and_truth
    d = parity.datasets()
    pt = _pt((4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    pt.run_chains()
    te = d["sunspot_test"].astype(np.float32)
    series, s = series_from_windows(te, 4)
    org_all, truth_all = windows_and_truth(series, 4, H, s, n_origins=te.shape[0])
    idx = np.concatenate([np.arange(0, te.shape[0], 50), np.arange(te.shape[0] - 3, te.shape[0])])
    origins, truth = np.ascontiguousarray(org_all[idx]), np.ascontiguousarray(truth_all[idx])
    assert np.isnan(truth).sum() == 1 + 3 + 5 and np.isfinite(truth[:, 0]).all()      # the trailing columns of the last three rows
    tr = pt._sampler.traces()["pos_w"]
    w = np.ascontiguousarray(tr[:, 300::10].reshape(-1, pt.num_param))
    eta = np.ascontiguousarray(pt._sampler.eta_trace()[:, 300::10].reshape(-1))
    return pt, origins, truth, w, eta


def _score(s, origins, truth, **kw):
    args = dict(SEL, noise=True, seed=NOISE_SEED, quantiles=QS, samples=True, means=True)
    args.update(kw)
    if "w" in args:
        for k in SEL:
            args.pop(k)
    return s.forecast_score(H, origins, truth, **args)


def _same(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k in skip:
            continue
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def _merged(w, eta):
    """Maximal runs of bitwise-equal consecutive (w, eta) -> (distinct w, their eta, counts)."""
    key = np.column_stack([w.view(np.uint32), eta.view(np.uint32)[:, None]])
    new = np.ones(len(key), bool)
    new[1:] = np.any(key[1:] != key[:-1], axis=1)
    starts = np.flatnonzero(new)
    return w[starts], eta[starts], np.diff(np.append(starts, len(key))).astype(np.int32)


def _rel(got, want):
    """max |got - want| / (1e-12 + 1e-9 |want|) over the entries with a reference value; the NaN sets must be equal."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / (1e-12 + 1e-9 * np.abs(want[ok])))) if ok.any() else 0.0


def _check_against_ref(out, eta, truth, counts, label, levels=QS):
    """Every column and origin of `out` against fscore_ref on the device's own means / samples (one row per trajectory)."""
    r = ref.scores(out["means"], out["samples"], eta, truth, counts, levels=levels)
    worst = {k: _rel(out[k], r[k]) for k in PER_COLUMN + ("quantiles", "energy_score")}
    print(f"{label}: max |device - reference| / (1e-12 + 1e-9 |reference|): " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (label, k, v)
    nan_cols = np.isnan(truth)
    for k in PER_COLUMN:
        assert np.array_equal(np.isnan(out[k]), nan_cols), k
    assert np.array_equal(np.isnan(out["quantiles"]), np.broadcast_to(nan_cols, out["quantiles"].shape))
    assert np.array_equal(np.isnan(out["energy_score"]), nan_cols.all(axis=1))       # NaN only for an origin without any truth
    assert np.all(np.diff(out["quantiles"], axis=0)[:, ~nan_cols] >= 0.0)


def test_trajectories_are_forecasts_and_means_are_predictions(sunspot):
    pt, origins, truth, w, eta = sunspot
    s = pt._sampler
    out = _score(s, origins, truth)
    assert out["n_samples"] == out["n_trajectories"] == 240
    fc = s.forecast(H, origins, noise=True, seed=NOISE_SEED, samples=True, **SEL)
    assert np.array_equal(out["samples"], fc["samples"])
    # mu = ptnn_predict of each vector on the windows built from the device's own earlier noisy outputs
    want, _ = _teacher(s, w, origins, out["samples"])
    assert np.array_equal(out["means"], want)
    assert np.array_equal(out["means"][:, :, 0], s.predict(origins, samples=True, mean=False, **SEL)["samples"][:, :, 0])
    assert not np.array_equal(out["means"][:, :, 1:], out["samples"][:, :, 1:])
    # noise off: the mean paths are the paths, one per distinct (w, eta)
    off = _score(s, origins, truth, noise=False)
    assert np.array_equal(off["samples"], off["means"]) and off["n_samples"] == 240
    assert np.array_equal(off["samples"], s.forecast(H, origins, samples=True, **SEL)["samples"])
    assert off["n_trajectories"] == sum(len(_merged(w.reshape(8, 30, -1)[c], eta.reshape(8, 30)[c])[2]) for c in range(8))
    assert np.array_equal(off["means"][:, :, 0], out["means"][:, :, 0])


@pytest.mark.parametrize("noise", [True, False])
def test_step_one_is_the_calibration_of_the_origin_rows(sunspot, noise):
    pt, origins, truth, w, eta = sunspot
    s = pt._sampler
    out = _score(s, origins, truth, noise=noise)
    rows = np.ascontiguousarray(np.column_stack([origins, truth[:, 0]]), dtype=np.float32)
    cal = s.calibration(rows, quantiles=QS, crps=True, **SEL)
    assert cal["n_samples"] == out["n_samples"]
    assert (out["n_trajectories"] == 240) if noise else (out["n_trajectories"] == cal["n_distinct"])
    for k in ("pit", "pred_mean", "pred_sd", "crps"):
        assert np.array_equal(out[k][:, 0], cal[k]), k
    assert np.array_equal(out["quantiles"][:, :, 0], cal["quantiles"])
    lppd = s.elpd(rows, **SEL)["lppd"]
    err = np.abs(out["log_score"][:, 0] - lppd)
    print(f"noise={noise}: max |log_score - lppd| = {err.max():.3e}")
    assert np.all(err <= 1e-9 * np.maximum(1.0, np.abs(lppd)))


def test_every_column_against_the_reference(sunspot):
    pt, origins, truth, w, eta = sunspot
    s = pt._sampler
    out = _score(s, origins, truth)
    _check_against_ref(out, eta, truth, None, "noise on")
    off = _score(s, origins, truth, noise=False)
    # one row of `means` per selected sample: weights 1 each restate the multiplicities
    _check_against_ref(off, eta, truth, None, "noise off")
    # the fed-back noise widens the later steps, not the first
    assert np.array_equal(out["pred_sd"][:, 0], off["pred_sd"][:, 0])
    assert np.nanmean(out["pred_sd"][:, -1]) > np.nanmean(off["pred_sd"][:, -1])
    # |K_r| = 1: the last origin's energy score is the ensemble CRPS of its one observed column
    assert np.isfinite(truth[-1]).sum() == 1
    x = out["samples"][:, -1, 0].astype(np.float64)
    want = np.mean(np.abs(x - np.float64(truth[-1, 0]))) - 0.5 * np.mean(np.abs(x[:, None] - x[None, :]))
    assert out["energy_score"][-1] == pytest.approx(want, rel=1e-9)


def test_high_level_call(sunspot):
    from ptnn_amd.parallel_tempering import forecast_compare
    pt, origins, truth, w, eta = sunspot
    fa = pt.forecast_accuracy(H, "test", thin=10, seed=NOISE_SEED, quantiles=(0.05, 0.95))
    assert fa.n.tolist() == [198, 197, 197, 196, 196, 195] and fa.n_samples == fa.n_trajectories == 240
    assert fa.truth.shape == (198, H) and np.array_equal(fa.origins, parity.datasets()["sunspot_test"][:, :4].astype(np.float32))
    idx = np.concatenate([np.arange(0, 198, 50), np.arange(195, 198)])
    low = _score(pt._sampler, origins, truth, quantiles=(0.05, 0.95), samples=False, means=False)
    # trajectory i at origin r draws from counter (k / 4, i, r): the noise of an origin depends on its index in the call
    assert np.array_equal(fa.crps_i[0], low["crps"][0]) and np.array_equal(fa.pit[0], low["pit"][0])
    assert np.array_equal(fa.pit[idx][:, 0], low["pit"][:, 0])                       # step 1 sees no noise
    ok = np.isfinite(fa.truth)
    for k in range(H):
        e = fa.pred_mean[ok[:, k], k] - fa.truth[ok[:, k], k].astype(np.float64)
        assert fa.rmse[k] == pytest.approx(np.sqrt(np.mean(e * e)), rel=1e-14)
        assert fa.crps[k] == pytest.approx(np.mean(fa.crps_i[ok[:, k], k]), rel=1e-14)
        assert fa.log_score[k] == pytest.approx(np.mean(fa.log_score_i[ok[:, k], k]), rel=1e-14)
        assert fa.coverage[0.9][k] == pytest.approx(np.mean((fa.pit[ok[:, k], k] >= 0.05) & (fa.pit[ok[:, k], k] <= 0.95)))
    assert np.array_equal(np.isnan(fa.crps_i), ~ok) and fa.pit_hist.sum(axis=1).tolist() == fa.n.tolist()
    assert fa.energy_score.shape == (198,) and fa.energy_mean == pytest.approx(fa.energy_score.mean())
    assert 0 <= fa.skill_horizon <= H and fa.rmse_skill.shape == fa.crps_skill.shape == (H,)
    assert fa.intervals[(0.05, 0.95)]["width"].shape == (H,)
    # series= with the rows' own series and stride gives the same origins, truth and scores
    alt = pt.forecast_accuracy(H, series=_series(pt), stride=2, thin=10, seed=NOISE_SEED, quantiles=(0.05, 0.95))
    assert np.array_equal(alt.truth, fa.truth, equal_nan=True) and np.array_equal(alt.crps_i, fa.crps_i, equal_nan=True)
    off = pt.forecast_accuracy(H, "test", thin=10, noise=False, quantiles=(0.05, 0.95))
    d = forecast_compare(fa, off)
    assert d["crps_diff"].shape == (H,) and d["crps_diff"][0] == 0.0 and np.isfinite(d["se_crps_diff"][1:]).all()
    assert np.isfinite(d["energy_diff"])
    nc = pt.forecast_accuracy(H, "test", thin=10, crps=False, energy=False, seed=NOISE_SEED)
    assert nc.crps is None and nc.crps_i is None and nc.energy_score is None and nc.crps_skill is None and nc.skill_horizon is None
    assert np.array_equal(nc.pit, fa.pit, equal_nan=True) and np.array_equal(nc.log_score_i, fa.log_score_i, equal_nan=True)


def _series(pt):
    from ptnn_amd.verification import series_from_windows
    return series_from_windows(np.asarray(pt.testdata, np.float32), 4)[0]


@pytest.mark.parametrize("noise", [True, False])
def test_invariances(sunspot, monkeypatch, noise):
    pt, origins, truth, w, eta = sunspot
    s = pt._sampler
    base = _score(s, origins, truth, noise=noise)
    U, I = base["n_trajectories"], 4
    col = 4 * U * (2 if noise else 1)
    _same(base, _score(s, origins, truth, noise=noise))                              # two calls
    # several origin blocks: two origins per block
    monkeypatch.setenv("PTNN_FSCORE_SCRATCH_BYTES", str(col * H * 2))
    _same(base, _score(s, origins, truth, noise=noise))
    # without the energy score the horizon is split too: one origin, two steps per block, the windows carried
    plain = _score(s, origins, truth, noise=noise, energy=False)
    _same(base, plain, skip=("energy_score",))
    monkeypatch.setenv("PTNN_FSCORE_SCRATCH_BYTES", str(col * (I + 2)))
    _same(plain, _score(s, origins, truth, noise=noise, energy=False))
    monkeypatch.setenv("PTNN_FSCORE_SCRATCH_BYTES", "1")                             # one step per block
    _same(plain, _score(s, origins, truth, noise=noise, energy=False))
    monkeypatch.delenv("PTNN_FSCORE_SCRATCH_BYTES")
    # the trace against host vectors: every row with its eta, and (distinct, count) per chain
    _same(base, _score(s, origins, truth, noise=noise, w=w, eta=eta))
    parts = [_merged(w.reshape(8, 30, -1)[c], eta.reshape(8, 30)[c]) for c in range(8)]
    dw, de, cnt = (np.concatenate([p[j] for p in parts]) for j in range(3))
    assert cnt.sum() == 240 and len(cnt) < 240
    _same(base, _score(s, origins, truth, noise=noise, w=dw, eta=de, multiplicity=cnt))
    # seeds
    other = _score(s, origins, truth, noise=noise, seed=NOISE_SEED + 1)
    if noise:
        assert not np.array_equal(other["samples"], base["samples"]) and not np.array_equal(other["crps"][:, 1:], base["crps"][:, 1:])
        assert np.array_equal(other["crps"][:, 0], base["crps"][:, 0])               # step 1 is scored before any noise
    else:
        _same(base, other)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        pt = _pt((4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)[::4]
            eta = np.full(w.shape[0], -2.0, np.float32)
            fa = pt.forecast_accuracy(5, "test", weights=w, eta=eta)
            assert fa.n_samples == fa.n_trajectories == 200
            assert pt.forecast_accuracy(5, "test", weights=w, eta=eta, noise=False).n_samples == 200
        res = pt.run_chains()
        fc = pt.forecast(5, "end", noise=True, burn_in=0.75, return_samples=True)
        outs.append((res, pt._sampler.traces(), pt._sampler.trace_rows(), pt._sampler.state(), pt._sampler.swap_stats(), fc))
    (ra, ta, rwa, sa, wa, fa_), (rb, tb, rwb, sb, wb, fb_) = outs
    for x, y in zip(ra, rb):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    assert np.array_equal(rwa, rwb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert wa == wb
    assert np.array_equal(fa_.samples, fb_.samples) and np.array_equal(fa_.mean, fb_.mean)


def test_refusals(sunspot, tmp_path, monkeypatch):
    from ptnn_amd import _lib
    from ptnn_amd.pt_classification import ParallelTempering as ClsPT
    pt, origins, truth, w, eta = sunspot
    s = pt._sampler
    # the trajectory cap: 70 000 occurrences of two vectors, every one its own trajectory with noise on
    big = dict(w=w[:2], eta=eta[:2], multiplicity=np.array([40000, 30000], np.int32))
    with pytest.raises(_lib.PtnnError, match=r"70000 trajectories.*at most 65536.*thin=, chains=.*crps=False, energy=False"):
        _score(s, origins, truth, **big)
    with pytest.raises(_lib.PtnnError, match="at most 65536"):
        _score(s, origins, truth, crps=False, **big)
    # noise off they are two trajectories
    two = _score(s, origins, truth, noise=False, samples=False, means=False, **big)
    assert two["n_trajectories"] == 2 and two["n_samples"] == 70000
    # the energy score needs one origin's whole horizon in scratch
    monkeypatch.setenv("PTNN_FSCORE_SCRATCH_BYTES", str(8 * 240 * H - 1))
    with pytest.raises(_lib.PtnnError, match="energy: one origin's 6 steps of 240 trajectories need 11520 bytes"):
        _score(s, origins, truth)
    assert _score(s, origins, truth, energy=False)["energy_score"] is None
    monkeypatch.delenv("PTNN_FSCORE_SCRATCH_BYTES")
    # noise without eta, rows before the first accepted step (ptnn_forecast's texts), bad truth
    with pytest.raises(_lib.PtnnError, match="noise: host vectors need eta"):
        _score(s, origins, truth, w=w)
    with pytest.raises(_lib.PtnnError, match="a regression's host vectors need eta"):
        _score(s, origins, truth, w=w, noise=False)
    with pytest.raises(_lib.PtnnError, match="noise: .*first accepted MH step"):
        s.forecast_score(H, origins, truth, step0=0, nsteps=300)
    with pytest.raises(ValueError, match="truth must be"):
        s.forecast_score(H, origins, truth[:, :3])
    with pytest.raises(ValueError, match="eta"):
        pt.forecast_accuracy(H, "test", weights=w)
    with pytest.raises(ValueError, match="series="):
        pt.forecast_accuracy(H, parity.datasets()["sunspot_test"][::-1])
    ok = _score(s, origins, truth, samples=False, means=False)                       # the handle is still usable
    assert ok["n_samples"] == 240
    # a classification handle
    d = parity.datasets()
    cls = ClsPT(True, 0.01, d["iris_train"], d["iris_test"], [4, 12, 3], 4, 10, 4 * 100, 10, str(tmp_path), seed=SEED,
                write_files=False)
    cls.initialize_chains(0.5)
    cls.run_chains()
    with pytest.raises(ValueError, match="regression"):
        cls.forecast_accuracy(3)
    with pytest.raises(_lib.PtnnError, match="regression net with n_out == 1"):
        cls._sampler.forecast_score(2, "test", np.zeros((d["iris_test"].shape[0], 2), np.float32), step0=50, nsteps=50)
    # a handle with a communicator attached
    tr, te = d["sunspot_train"], d["sunspot_test"]
    sh = parity.make_sampler(0, (4, 5, 1), tr, te, R_local=2, R_global=4, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    sh.set_state(np.zeros((2, 31), np.float32), np.ones(2, np.float32))
    one = dict(w=np.zeros((1, 31), np.float32), eta=np.zeros(1, np.float32))
    assert sh.forecast_score(2, origins, truth[:, :2], **one)["n_samples"] == 1
    sh.comm_init_host(0, 2, lambda b: None, lambda m: None)
    with pytest.raises(_lib.PtnnError, match="communicator"):
        sh.forecast_score(2, origins, truth[:, :2], **one)
    sh.close()
