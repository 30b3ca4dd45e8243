"""Recursive multi-step forecasts on the GPU (ptnn_forecast / forecast): step 1 against posterior_predictive bitwise, every
later step against ptnn_predict on the window built from the device's own earlier outputs (teacher forcing), free runs against
the float64 oracle of tests/forecast_ref.py, the observation noise against philox.normals, and the invariants of DESIGN.md
section 14 (blocking, sources, seeds, no side effects), on both kernel layouts."""
import numpy as np
import pytest

import forecast_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
PCTS = (0, 5, 50, 95, 100, 37.5)


def _pt(topo, train, test, R, S, tmp_path, *, lg=True, lr=0.1, maxtemp=2, si=10, burn_in=0.5, **kw):
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, 0.5, str(tmp_path), seed=SEED, write_files=False,
                           **kw)
    pt.initialize_chains(burn_in)
    return pt


def _runs(pos_w_cols, R):
    """Maximal runs of bitwise-equal consecutive vectors per chain of a posterior matrix [P, R m] -> (distinct [U, P], counts)."""
    P, n = pos_w_cols.shape
    m = n // R
    w = np.ascontiguousarray(pos_w_cols.T.astype(np.float32))
    distinct, counts = [], []
    for c in range(R):
        blk = w[c * m:(c + 1) * m]
        new = np.ones(m, bool)
        new[1:] = np.any(blk[1:].view(np.uint32) != blk[:-1].view(np.uint32), axis=1)
        starts = np.flatnonzero(new)
        distinct.append(blk[starts])
        counts.append(np.diff(np.append(starts, m)))
    return np.concatenate(distinct), np.concatenate(counts).astype(np.int32)


def _same(a, b, pcts=PCTS):
    assert a.n_samples == b.n_samples and a.n_trajectories == b.n_trajectories
    assert np.array_equal(a.mean, b.mean)
    for q in pcts:
        assert np.array_equal(a.percentiles[q], b.percentiles[q]), q
    if a.samples is not None and b.samples is not None:
        assert np.array_equal(a.samples, b.samples)


def _teacher(sampler, w, origins, paths):
    """ptnn_predict of vector u on every window its trajectory read: [U, n_origins, h] (float32), and the windows themselves."""
    U, R, h = paths.shape
    I = origins.shape[1]
    wins = np.empty((U, R, h, I), np.float32)
    for u in range(U):
        for r in range(R):
            full = np.concatenate([origins[r].astype(np.float32), paths[u, r]])
            for k in range(h):
                wins[u, r, k] = full[k:k + I]
    out = np.empty((U, R, h), np.float32)
    blk = max(1, 4096 // (R * h))
    for u0 in range(0, U, blk):                     # each vector on its own windows only: a block of vectors at a time
        u1 = min(U, u0 + blk)
        got = sampler.predict(wins[u0:u1].reshape(-1, I), w=w[u0:u1], samples=True, mean=False)["samples"][:, :, 0]
        for u in range(u0, u1):
            out[u] = got[u - u0, (u - u0) * R * h:(u - u0 + 1) * R * h].reshape(R, h)
    return out, wins


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt((4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)                     # chain-major, as the columns of res[0]
    return pt, res, d, eta


# invariant 1: horizon step 1 from the test rows is posterior_predictive on them, bitwise -- on both layouts
@pytest.mark.parametrize("name,topo,R,S", [("sunspot", (4, 5, 1), 8, 600), ("mackey", (4, 10, 1), 8, 600),
                                           ("sunspot5", (5, 5, 1), 8, 600), ("synth32", (32, 96, 1), 4, 200)])
def test_step_one_is_the_posterior_predictive(name, topo, R, S, tmp_path):
    d = parity.datasets()
    pt = _pt(topo, d[name + "_train"], d[name + "_test"], R, S, tmp_path)
    if topo[1] > 64:
        assert pt._sampler.describe()["compact_traces"] == 1
    pt.run_chains()
    for x in ("test", "train"):
        pred = pt.posterior_predictive(x, percentiles=PCTS, return_samples=True)
        fc = pt.forecast(1, x, percentiles=PCTS, return_samples=True)
        assert fc.n_samples == pred.n_samples and fc.n_trajectories == pred.n_distinct
        assert fc.mean.shape == (pred.mean.shape[0], 1)
        assert np.array_equal(fc.mean, pred.mean)
        for q in PCTS:
            assert np.array_equal(fc.percentiles[q], pred.percentiles[q]), q
        assert np.array_equal(fc.samples, pred.samples)
    # a longer horizon leaves step 1 as it is
    pred = pt.posterior_predictive("test", return_samples=True)
    fc4 = pt.forecast(4, "test", return_samples=True)
    assert np.array_equal(fc4.samples[:, :, :1], pred.samples) and np.array_equal(fc4.mean[:, :1], pred.mean)


def test_teacher_forced_steps(sunspot):
    pt, res, d, _ = sunspot
    distinct, counts = _runs(res[0], 8)
    te = d["sunspot_test"]
    origins = np.concatenate([te[::50, :4], te[-1:, 1:5]]).astype(np.float32)
    h = 8
    fc = pt._sampler.forecast(h, origins, w=distinct, samples=True)
    assert fc["n_trajectories"] == distinct.shape[0] and fc["samples"].shape == (distinct.shape[0], origins.shape[0], h)
    paths = fc["samples"]
    want, wins = _teacher(pt._sampler, distinct, origins, paths)
    assert np.array_equal(paths, want)
    # the same steps in float64 on the same windows
    U, R = paths.shape[:2]
    for u in range(0, U, max(1, U // 40)):
        f64 = orc.forward(wins[u].reshape(-1, 4).astype(np.float64), distinct[u].astype(np.float64), (4, 5, 1))[1][:, 0]
        assert np.max(np.abs(paths[u].reshape(-1) - f64)) <= 1e-5
    # the trace source forecasts the same trajectories: weights=(distinct, counts) gives the same bands
    a = pt.forecast(h, origins, percentiles=PCTS, return_samples=True)
    b = pt.forecast(h, origins, percentiles=PCTS, weights=(distinct, counts), return_samples=True)
    _same(a, b)
    assert a.n_trajectories == distinct.shape[0]
    s64 = a.samples.astype(np.float64)
    np.testing.assert_allclose(a.mean, s64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(a.percentiles[q], np.percentile(s64, q, axis=0)), q


# Free run: the device's fp32 recursion against the oracle's float64 one.  Measured on an MI355X at this fixture (R = 8,
# S = 600, Sunspot 4-5-1, 424 distinct vectors from origin "end" and every 25th test row, h = 10): max |difference| = 1.1e-7;
# the bound is about ten times that.
FREE_RUN_BOUND = 1e-6


def test_free_run_against_the_oracle(sunspot):
    pt, res, d, _ = sunspot
    distinct, _ = _runs(res[0], 8)
    te = d["sunspot_test"]
    origins = np.concatenate([te[::25, :4], te[-1:, 1:5]]).astype(np.float32)
    h = 10
    fc = pt._sampler.forecast(h, origins, w=distinct, samples=True)
    want = ref.trajectories(distinct.astype(np.float64), origins.astype(np.float64), h, (4, 5, 1))
    err = np.max(np.abs(fc["samples"] - want))
    print(f"free run h={h}: max |device - oracle| = {err:.3e} over {distinct.shape[0]} trajectories x {origins.shape[0]} origins")
    assert err <= FREE_RUN_BOUND
    # "end" is the window after the last test row
    end = pt.forecast(h, "end", return_samples=True)
    alt = pt.forecast(h, te[-1:, 1:5], return_samples=True)
    assert end.mean.shape == (1, h)
    _same(end, alt, (5, 95))


def test_noise(sunspot):
    pt, res, d, eta_all = sunspot
    s = pt._sampler
    reps, step0, thin = [0, 5], 300, 10
    h, seed = 9, 0x5EED_0000_0001
    te = d["sunspot_test"]
    origins = np.concatenate([te[-1:, 1:5], te[:2, :4]]).astype(np.float32)
    fc = s.forecast(h, origins, replicas=reps, step0=step0, nsteps=300, thin=thin, noise=True, seed=seed, samples=True)
    M = len(reps) * 30
    assert fc["n_samples"] == M and fc["n_trajectories"] == M
    tr = s.traces()["pos_w"]
    w = tr[reps, step0::thin].reshape(-1, pt.num_param)
    eta = s.eta_trace()[reps, step0::thin].reshape(-1)
    paths = fc["samples"]
    f, _ = _teacher(s, w, origins, paths)
    got = paths.astype(np.float64) - f.astype(np.float64)
    sd = np.exp(0.5 * eta.astype(np.float32).astype(np.float64))
    want = np.stack([[sd[i] * ref.noise_draws(h, i, r, seed) for r in range(origins.shape[0])] for i in range(M)])
    # fp32 Box-Muller on the hardware log / sqrt / sin / cos against float64, plus the rounding of y + sd z
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-6)
    assert np.std(got / sd[:, None, None]) == pytest.approx(1.0, abs=0.2)
    # the trace vs the same vectors expanded with their eta: bitwise (occurrence i is trajectory i either way)
    alt = s.forecast(h, origins, w=w, eta=eta, noise=True, seed=seed, samples=True)
    assert np.array_equal(alt["samples"], paths) and np.array_equal(alt["mean"], fc["mean"])
    # host multiplicities expand into occurrences: the same as the rows written out
    dw, cnt = _runs(w.T, 1)
    de = eta[np.concatenate([[0], np.cumsum(cnt)[:-1]])]
    assert np.array_equal(np.repeat(de, cnt), eta)
    mul = s.forecast(h, origins, w=dw, eta=de, multiplicity=cnt, noise=True, seed=seed, samples=True)
    assert np.array_equal(mul["samples"], paths)
    # seeds: the same seed is bitwise the same, another seed differs, noise off ignores the seed
    again = s.forecast(h, origins, replicas=reps, step0=step0, nsteps=300, thin=thin, noise=True, seed=seed, samples=True)
    assert np.array_equal(again["samples"], paths)
    other = s.forecast(h, origins, replicas=reps, step0=step0, nsteps=300, thin=thin, noise=True, seed=seed + 1, samples=True)
    assert not np.array_equal(other["samples"], paths)
    off = [pt.forecast(h, "end", seed=sd_, percentiles=PCTS, return_samples=True) for sd_ in (1, 2)]
    _same(off[0], off[1])
    # the high-level call: seed=None is the object's seed, bands from the order statistics as numpy computes them
    hi = pt.forecast(h, "end", noise=True, percentiles=PCTS, return_samples=True)
    lo = pt.forecast(h, "end", noise=True, seed=pt.seed, percentiles=PCTS, return_samples=True)
    _same(hi, lo)
    assert hi.n_trajectories == hi.n_samples == 8 * 300
    s64 = hi.samples.astype(np.float64)
    for q in PCTS:
        assert np.array_equal(hi.percentiles[q], np.percentile(s64, q, axis=0)), q
    tr_hi = pt.forecast(h, "end", noise=True, percentiles=PCTS, weights=res[0].T, eta=eta_all, return_samples=True)
    _same(hi, tr_hi)


@pytest.mark.parametrize("noise", [False, True])
def test_blocking_changes_nothing(sunspot, monkeypatch, noise):
    pt, _, _, _ = sunspot
    h = 7
    kw = dict(percentiles=PCTS, noise=noise, return_samples=True, burn_in=0.8)
    ref_ = pt.forecast(h, "test", **kw)
    U, I = ref_.n_trajectories, 4
    # one origin per block, horizon blocks of 2 steps: 198 origin blocks x 4 horizon blocks, windows carried between them
    monkeypatch.setenv("PTNN_FORECAST_SCRATCH_BYTES", str(4 * U * (I + 2)))
    got = pt.forecast(h, "test", **kw)
    _same(got, ref_)
    monkeypatch.setenv("PTNN_FORECAST_SCRATCH_BYTES", str(4 * U * h * 50))          # 4 blocks of 50 origins
    _same(pt.forecast(h, "test", **kw), ref_)
    monkeypatch.setenv("PTNN_FORECAST_SCRATCH_BYTES", "1")                           # one step per block
    one = pt.forecast(h, "end", noise=noise, percentiles=PCTS)
    monkeypatch.delenv("PTNN_FORECAST_SCRATCH_BYTES")
    _same(one, pt.forecast(h, "end", noise=noise, percentiles=PCTS))


def test_split_layout_blocks_and_noise(tmp_path, monkeypatch):
    # the wide layout (one vector per work-group, hidden units over waves) with carried windows, noise and the oracle
    d = parity.datasets()
    R, S = 4, 200
    pt = _pt((32, 96, 1), d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    res = pt.run_chains()
    h = 6
    ref_ = pt.forecast(h, "test", percentiles=PCTS, return_samples=True)
    distinct, counts = _runs(res[0], R)
    _same(ref_, pt.forecast(h, "test", percentiles=PCTS, weights=(distinct, counts), return_samples=True))
    fc = pt._sampler.forecast(h, "test", w=distinct, samples=True)["samples"]
    want, _ = _teacher(pt._sampler, distinct, d["synth32_test"][:, :32].astype(np.float32), fc)
    assert np.array_equal(fc, want)
    # noise: from row 160 on, after every chain's first accepted step
    b = 160
    w = pt._sampler.traces()["pos_w"][:, b:].reshape(-1, pt.num_param)
    eta = pt._sampler.eta_trace()[:, b:].reshape(-1)
    noisy = pt.forecast(h, "test", noise=True, burn_in=b / S, percentiles=PCTS, return_samples=True)
    _same(noisy, pt.forecast(h, "test", noise=True, percentiles=PCTS, weights=w, eta=eta, return_samples=True))
    for n, U in ((False, ref_.n_trajectories), (True, noisy.n_trajectories)):
        monkeypatch.setenv("PTNN_FORECAST_SCRATCH_BYTES", str(4 * U * (32 + 2)))      # one origin, 2 steps per block
        got = pt.forecast(h, "test", noise=n, burn_in=b / S if n else None, percentiles=PCTS, return_samples=True)
        _same(got, noisy if n else ref_)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt((4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)
            eta = np.full(w.shape[0], -2.0, np.float32)
            assert pt.forecast(20, "test", weights=w).n_samples == 800
            assert pt.forecast(20, "end", weights=w, eta=eta, noise=True).n_trajectories == 800
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
    from ptnn_amd.pt_classification import ParallelTempering as ClsPT
    d = parity.datasets()
    tr, te = d["sunspot_train"], d["sunspot_test"]
    pt = _pt((4, 5, 1), tr, te, 4, 200, tmp_path)
    with pytest.raises(ValueError, match="run_chains"):
        pt.forecast(5)
    w = np.asarray(pt._w0, np.float32)
    assert pt.forecast(5, weights=w).n_samples == 4                            # weights= works before any run
    res = pt.run_chains()
    s = pt._sampler
    with pytest.raises(_lib.PtnnError, match="horizon"):
        s.forecast(0, "test")
    with pytest.raises(_lib.PtnnError, match="n_ranks"):
        s.forecast(3, "test", ranks=list(range(17)))
    with pytest.raises(_lib.PtnnError, match="eta"):
        s.forecast(3, "test", w=res[0].T, noise=True)
    with pytest.raises(ValueError, match="eta"):
        pt.forecast(3, weights=res[0].T, noise=True)
    # rows before a chain's first accepted step carry no eta: refused with noise, fine without
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt.forecast(3, burn_in=0, noise=True)
    assert pt.forecast(3, burn_in=0).n_samples == 4 * 200
    with pytest.raises(ValueError, match="n_in"):
        pt.forecast(3, te[:, :3])
    ok = pt.forecast(3)                                                           # the handle is still usable
    assert ok.n_samples == 400 and np.array_equal(ok.mean, pt.forecast(3, weights=res[0].T).mean)
    # not a one-step regression map
    cls = ClsPT(True, 0.01, d["iris_train"], d["iris_test"], [4, 12, 3], 4, 10, 4 * 100, 10, str(tmp_path), seed=SEED,
                write_files=False)
    cls.initialize_chains(0.5)
    cls.run_chains()
    with pytest.raises(ValueError, match="regression"):
        cls.forecast(3)
    with pytest.raises(_lib.PtnnError, match="regression net with n_out == 1"):
        cls._sampler.forecast(3, "test")
    for kw, msg in ((dict(label_swap=True), "label_swap"), (dict(trace_capacity=64), "trace_capacity")):
        other = _pt((4, 5, 1), tr, te, 4, 200, tmp_path, **kw)
        other_res = other.run_chains()
        with pytest.raises(ValueError, match=msg):
            other.forecast(3)
        assert other.forecast(3, weights=other_res[0].T).n_samples == 400
    # a handle with a communicator attached
    sh = parity.make_sampler(0, (4, 5, 1), tr, te, R_local=2, R_global=4, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    sh.set_state(np.zeros((2, 31), np.float32), np.ones(2, np.float32))
    assert sh.forecast(2, "test", w=np.zeros((1, 31), np.float32))["n_samples"] == 1
    sh.comm_init_host(0, 2, lambda b: None, lambda m: None)
    with pytest.raises(_lib.PtnnError, match="communicator"):
        sh.forecast(2, "test", w=np.zeros((1, 31), np.float32))
    sh.close()
