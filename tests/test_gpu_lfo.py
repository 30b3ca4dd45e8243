"""Leave-future-out cross-validation on the GPU (ptnn_lfo / leave_future_out): the device result against the float64 oracle
(tests/lfo_ref.py) on the call's own pointwise log-likelihood and on the oracle's forward pass, the identities that tie it to
PSIS-LOO and lppd, bitwise agreement between sources, budgets and splits of the origins, side effects, refusals, and the walk
with refits end to end."""
import math
import warnings

import numpy as np
import pytest

import elpd_ref
import lfo_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
ATOL = 1e-4          # per data row: the device's fp32 forward pass vs the oracle's float64 one (tests/test_gpu_elpd.py)


def _pt(task, topo, train, test, R, S, tmp_path, *, lg=True, lr=0.1, maxtemp=2, si=10, burn_in=0.5, seed=SEED, **kw):
    path = str(tmp_path)
    if task == orc.TASK_REG:
        from ptnn_amd.pt_timeseries_regression import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, 0.5, path, seed=seed, write_files=False, **kw)
    else:
        from ptnn_amd.pt_classification import ParallelTempering
        pt = ParallelTempering(lg, lr, train, test, list(topo), R, maxtemp, R * S, si, path, seed=seed, write_files=False, **kw)
    pt.initialize_chains(burn_in)
    return pt


def _oracle_ll(task, rows, cols, topo, eta=None):
    """float64 pointwise log-likelihood [M, n_rows] of the weight vectors cols [P, M] on data rows [n_rows, n_in + 1]."""
    X, y = rows[:, :topo[0]], rows[:, topo[0]]
    out = np.stack([orc.forward(X, cols[:, j].astype(np.float64), topo)[1] for j in range(cols.shape[1])])
    if task == orc.TASK_CLS:
        e = np.exp(out)
        p = e / e.sum(axis=2, keepdims=True)
        return np.log(p[:, np.arange(X.shape[0]), y.astype(np.int64)])
    tau2 = np.exp(np.asarray(eta, np.float32).astype(np.float64))[:, None]
    d = y[None, :] - out[:, :, 0]
    return -0.5 * np.log(2 * math.pi * tau2) - 0.5 * d * d / tau2


def _runs(w, eta):
    w32 = np.ascontiguousarray(w, np.float32)
    e32 = np.ascontiguousarray(eta, np.float32)
    new = np.ones(w32.shape[0], bool)
    new[1:] = np.any(w32[1:].view(np.uint32) != w32[:-1].view(np.uint32), axis=1) | (e32[1:].view(np.uint32) != e32[:-1].view(np.uint32))
    starts = np.flatnonzero(new)
    return w32[starts], e32[starts], np.diff(np.append(starts, w32.shape[0])).astype(np.int32)


def _same(a, b):
    for k in ("elpd_lfo", "khat", "tail_len"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_samples"] == b["n_samples"]


def _check_own(out, n_fit, origins, block, r_eff=1.0):
    """The reduction alone: the oracle on the call's own log-likelihood."""
    own = ref.lfo_rows(out["loglik"], n_fit, origins, block, r_eff=r_eff)
    err = np.max(np.abs(out["elpd_lfo"] - own["elpd_lfo"]) / np.abs(own["elpd_lfo"]))
    print(f"n_fit {n_fit} block {block}: max rel. difference to the oracle on the device's ll {err:.3e}")
    np.testing.assert_allclose(out["elpd_lfo"], own["elpd_lfo"], rtol=1e-9)
    fin = np.isfinite(own["khat"])
    assert np.array_equal(np.isfinite(out["khat"]), fin) and np.array_equal(out["tail_len"], own["tail_len"])
    assert np.max(np.abs(out["khat"][fin] - own["khat"][fin]), initial=0.0) <= 1e-9
    return own


def _check_oracle(out, ll_ref, n_fit, origins, block):
    """Against the float64 forward pass: K = |i - n_fit| + block rows enter an origin's sums, each with the floor ATOL."""
    r = ref.lfo_rows(ll_ref, n_fit, origins, block)
    K = np.abs(np.asarray(origins) - n_fit) + block
    diff = np.abs(out["elpd_lfo"] - r["elpd_lfo"])
    bound = 1e-5 * np.abs(r["elpd_lfo"]) + ATOL * K
    print(f"n_fit {n_fit} block {block}: max |device - oracle| {diff.max():.3e}, largest share of its bound {np.max(diff / bound):.3f}")
    assert np.all(diff <= bound)


def _cases(N, n_fit):
    """(origins, block) backward from and forward of n_fit, at distances 0 .. 31."""
    out = []
    for block in (1, 3):
        og = [n_fit - k for k in (1, 2, 4, 8, 16, 31) if n_fit - k > 0 and n_fit - k + block <= N]
        og += [n_fit + k for k in (0, 1, 3, 7, 15, 31) if n_fit + k + block <= N]
        out.append((np.array(og, np.int64), block))
    return out


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, 300:].reshape(-1)                     # chain-major, as the columns of res[0]
    rows = np.vstack([d["sunspot_train"], d["sunspot_test"]])
    return pt, res, d, eta, rows


def test_regression_sunspot(sunspot):
    pt, res, d, eta, rows = sunspot
    sel, n_s = pt._trace_selection(None, "all", 1)
    Ntr = len(d["sunspot_train"])
    ll_ref = _oracle_ll(orc.TASK_REG, rows, res[0], (4, 5, 1), eta)
    for og, block in _cases(Ntr, Ntr):                                    # backward: the training rows, the fit has seen them all
        out = pt._sampler.lfo("train", n_fit=Ntr, origins=og, block=block, loglik_out=True, **sel)
        assert out["n_samples"] == n_s == 2400 and out["loglik"].shape == (2400, Ntr) and out["n_distinct"] < 2400
        _check_own(out, Ntr, og, block)
        _check_oracle(out, ll_ref[:, :Ntr], Ntr, og, block)
    for og, block in _cases(len(rows), Ntr):                              # both directions over train + test rows
        out = pt._sampler.lfo(rows, n_fit=Ntr, origins=og, block=block, loglik_out=True, **sel)
        own = _check_own(out, Ntr, og, block)
        _check_oracle(out, ll_ref, Ntr, og, block)
        at = int(np.flatnonzero(og == Ntr)[0])
        assert np.isinf(out["khat"][at]) and out["tail_len"][at] == 0 and np.isinf(own["khat"][at])
    # the pointwise output is ptnn_elpd's
    assert np.array_equal(out["loglik"], pt._sampler.elpd(rows, loglik_out=True, **sel)["loglik"])


def test_classification_iris(tmp_path):
    d = parity.datasets()
    topo = (4, 12, 3)
    pt = _pt(orc.TASK_CLS, topo, d["iris_train"], d["iris_test"], 8, 400, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    sel, _ = pt._trace_selection(None, "all", 1)
    rows = np.vstack([d["iris_train"], d["iris_test"]])                   # rows in file order
    Ntr = len(d["iris_train"])
    ll_ref = _oracle_ll(orc.TASK_CLS, rows, res[0], topo)
    for og, block in _cases(len(rows), Ntr):
        out = pt._sampler.lfo(rows, n_fit=Ntr, origins=og, block=block, loglik_out=True, **sel)
        _check_own(out, Ntr, og, block)
        _check_oracle(out, ll_ref, Ntr, og, block)
        _same(pt._sampler.lfo(rows, n_fit=Ntr, origins=og, block=block, w=res[0].T), out)
    bad = np.array(rows[:, :5], dtype=np.float32)
    bad[3, 4] = 3.0
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="class label"):
        pt._sampler.lfo(bad, n_fit=Ntr, origins=[Ntr], **sel)


def test_wide_net_compact_traces(tmp_path):
    d = parity.datasets()
    R, S, topo = 4, 200, (32, 256, 1)
    pt = _pt(orc.TASK_REG, topo, d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, S // 2:].reshape(-1)
    sel, _ = pt._trace_selection(None, "all", 1)
    rows = np.vstack([d["synth32_train"], d["synth32_test"]])
    Ntr = len(d["synth32_train"])
    for og, block in _cases(len(rows), Ntr):
        out = pt._sampler.lfo(rows, n_fit=Ntr, origins=og, block=block, loglik_out=True, **sel)
        _check_own(out, Ntr, og, block)
        _same(pt._sampler.lfo(rows, n_fit=Ntr, origins=og, block=block, w=res[0].T, eta=eta), out)


def _gpd(xi, n, rng):
    """Draws of a generalised Pareto distribution of shape xi, scale 1, by its inverse cdf."""
    return np.expm1(-xi * np.log1p(-rng.random(n))) / xi


@pytest.mark.parametrize("xi", [0.2, 0.9])
def test_known_answer_gpd(sunspot, xi):
    pt = sunspot[0]
    rng = np.random.default_rng(int(xi * 10))
    ratios = _gpd(xi, 20000, rng)
    # three rows; with n_fit = 1 the origin 2 adds row 1 (lr = log ratio), with n_fit = 2 the origin 1 removes it (lr = -ll)
    t = rng.normal(-1.0, 0.3, 20000)
    fwd = np.stack([np.zeros(20000), np.log(ratios), t], axis=1)
    bwd = np.stack([np.zeros(20000), -np.log(ratios), t], axis=1)
    a = pt._sampler.lfo(loglik=fwd, n_fit=1, origins=[2, 1])
    b = pt._sampler.lfo(loglik=bwd, n_fit=2, origins=[1, 2])
    ra, rb = ref.lfo_rows(fwd, 1, [2, 1]), ref.lfo_rows(bwd, 2, [1, 2])
    for out, r in ((a, ra), (b, rb)):
        np.testing.assert_allclose(out["elpd_lfo"], r["elpd_lfo"], rtol=1e-9)
        assert abs(out["khat"][0] - r["khat"][0]) <= 1e-9 and abs(out["khat"][0] - xi) < 0.1
        assert np.isinf(out["khat"][1]) and out["tail_len"][1] == 0 and out["tail_len"][0] == math.ceil(3 * math.sqrt(20000))
    assert a["khat"][0] == b["khat"][0]                                   # the same ratios from either side
    # the target of fwd's origin 2 and of bwd's origin 2 is row 2; bwd's is at its fit: the plain mean
    assert b["elpd_lfo"][1] == pytest.approx(np.log(np.mean(np.exp(t))), rel=1e-12)


def test_identities_with_predictive_accuracy(sunspot):
    pt, res, d, eta, rows = sunspot
    sel, _ = pt._trace_selection(None, "all", 1)
    Ntr = len(d["sunspot_train"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa_tr = pt.predictive_accuracy("train")
        pa_all = pt.predictive_accuracy(rows)
    # origin n_fit - 1, block 1 = PSIS-LOO of row n_fit - 1
    back = pt._sampler.lfo("train", n_fit=Ntr, origins=[Ntr - 1], **sel)
    assert back["elpd_lfo"][0] == pytest.approx(pa_tr.elpd_loo_i[Ntr - 1], rel=1e-9)
    assert back["khat"][0] == pytest.approx(pa_tr.khat[Ntr - 1], abs=1e-9)
    # the same for any fit the caller states: row n_fit - 1 of the LOO over all rows
    for nf in (Ntr + 10, len(rows)):
        out = pt._sampler.lfo(rows, n_fit=nf, origins=[nf - 1, nf] if nf < len(rows) else [nf - 1], **sel)
        assert out["elpd_lfo"][0] == pytest.approx(pa_all.elpd_loo_i[nf - 1], rel=1e-9)
        if nf < len(rows):                                                # origin n_fit, block 1 = lppd of row n_fit
            assert out["elpd_lfo"][1] == pytest.approx(pa_all.lppd_i[nf], rel=1e-9)
    at = pt._sampler.lfo(rows, n_fit=Ntr, origins=[Ntr], **sel)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert at["elpd_lfo"][0] == pytest.approx(pt.predictive_accuracy("test").lppd_i[0], rel=1e-9)


def test_sources_agree(sunspot, monkeypatch):
    pt, res, d, eta, rows = sunspot
    sel, _ = pt._trace_selection(None, "all", 1)
    Ntr = len(d["sunspot_train"])
    og = np.array([Ntr - 30, Ntr + 5, Ntr - 1, Ntr, Ntr + 40, Ntr - 1, 7])       # any order, a repeat
    kw = dict(n_fit=Ntr, origins=og, block=2)
    base = pt._sampler.lfo(rows, loglik_out=True, **kw, **sel)
    assert base["elpd_lfo"][2] == base["elpd_lfo"][5]
    # host vectors, expanded and as distinct (w, eta) with multiplicities
    _same(pt._sampler.lfo(rows, w=res[0].T, eta=eta, **kw), base)
    w, e, c = _runs(res[0].T, eta)
    alt = pt._sampler.lfo(rows, w=w, eta=e, multiplicity=c, **kw)
    _same(alt, base)
    assert alt["n_distinct"] == base["n_distinct"]
    # the device's own log-likelihood through source 3
    _same(pt._sampler.lfo(loglik=base["loglik"], **kw), base)
    # the scratch budget: one row per block and one origin per pass; a budget in between
    for budget in ("1", str(80 * base["n_distinct"])):
        monkeypatch.setenv("PTNN_LFO_SCRATCH_BYTES", budget)
        one = pt._sampler.lfo(rows, loglik_out=True, **kw, **sel)
        _same(one, base)
        assert np.array_equal(one["loglik"], base["loglik"])
        _same(pt._sampler.lfo(loglik=base["loglik"], **kw), base)
    monkeypatch.delenv("PTNN_LFO_SCRATCH_BYTES")
    # the origins in one call or one call each
    for k, i in enumerate(og):
        single = pt._sampler.lfo(rows, n_fit=Ntr, origins=[i], block=2, **sel)
        assert single["elpd_lfo"][0] == base["elpd_lfo"][k] and single["khat"][0] == base["khat"][k], i
    # the same w with a different eta is another sample
    e2 = eta.copy()
    e2[1::2] += np.float32(0.25)
    assert pt._sampler.lfo(rows, w=res[0].T, eta=e2, **kw)["n_distinct"] > base["n_distinct"]


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)
            out = pt._sampler.lfo("train", n_fit=105, origins=np.arange(50, 105), w=w)
            assert out["n_samples"] == 800
            out = pt._sampler.lfo("train", n_fit=105, origins=[60, 100], step0=100, nsteps=70)
            assert out["n_samples"] == 8 * 70
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
        pt.leave_future_out()
    res = pt.run_chains()
    sel, _ = pt._trace_selection(None, "all", 1)
    N = len(tr)
    for kw, msg in ((dict(n_fit=0, origins=[5]), "n_fit = 0"), (dict(n_fit=N + 1, origins=[5]), "n_fit = 299"),
                    (dict(n_fit=N, origins=[0]), r"origin 0 \(origins\[0\]\)"), (dict(n_fit=N, origins=[5, N]), r"origin 298 \(origins\[1\]\)"),
                    (dict(n_fit=N, origins=[N - 2], block=3), "i \\+ block > n_rows"), (dict(n_fit=N, origins=[5], block=0), "block = 0"),
                    (dict(n_fit=N, origins=[]), "n_origins = 0"), (dict(n_fit=N, origins=[5], r_eff=0.0), "r_eff")):
        with pytest.raises(_lib.PtnnError, match=msg):
            pt._sampler.lfo("train", **kw, **sel)
    with pytest.raises(_lib.PtnnError, match="eta = log tau"):
        pt._sampler.lfo("train", n_fit=N, origins=[5], w=res[0].T)
    # rows before a chain's first accepted step carry no eta: row 0 always is one
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt._sampler.lfo("train", n_fit=N, origins=[5], step0=0, nsteps=200)
    with pytest.raises(_lib.PtnnError, match="first accepted MH step"):
        pt.leave_future_out(burn_in=0, refit=False)
    ll = np.full((4, 3), -1.0)
    ll[2, 1] = math.inf
    with pytest.raises(_lib.PtnnError, match=r"loglik\[2, 1\]"):
        pt._sampler.lfo(loglik=ll, n_fit=3, origins=[1])
    ll[2, 1] = -1.0
    # the PSIS tail outgrows the LDS: M = ceil(min(0.2 S, 3 sqrt(S / r_eff))) > 4096 (S = 40 000 through multiplicities)
    with pytest.raises(_lib.PtnnError, match="thin="):
        pt._sampler.lfo(loglik=ll, multiplicity=np.full(4, 10000), n_fit=3, origins=[1], r_eff=1e-6)
    assert pt._sampler.lfo(loglik=ll, multiplicity=np.full(4, 10000), n_fit=3, origins=[1])["n_samples"] == 40000
    # host-side refusals of the public call
    for kw, msg in ((dict(data="valid"), "data must be"), (dict(data="train", n_fit=5), "n_fit= goes with"), (dict(data=tr), "needs n_fit="),
                    (dict(block=0), "block = 0"), (dict(min_train=N), "leaves no origin"), (dict(refit=3), "refit must be"),
                    (dict(data=tr[:, :3], n_fit=5), "at least n_in")):
        with pytest.raises(ValueError, match=msg):
            pt.leave_future_out(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ok = pt.leave_future_out(min_train=N - 5, refit=False)               # the handle is still usable
    assert ok.n_samples == 400 and ok.origins.tolist() == list(range(N - 5, N)) and ok.n_refits == 0
    for kw, msg in ((dict(label_swap=True), "label_swap"), (dict(trace_capacity=64), "trace_capacity")):
        other = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, **kw)
        other.run_chains()
        with pytest.raises(ValueError, match=msg):
            other.leave_future_out()
    # a handle with a communicator attached
    sh = parity.make_sampler(0, (4, 5, 1), tr, te, R_local=2, R_global=4, first=0, S=20, si=5, use_lg=False, lr=0.1, seed=1)
    sh.set_state(np.zeros((2, 31), np.float32), np.ones(2, np.float32))
    one = dict(w=np.zeros((2, 31), np.float32), eta=np.zeros(2, np.float32), n_fit=N, origins=[N - 1])
    assert sh.lfo("train", **one)["n_samples"] == 2
    sh.comm_init_host(0, 2, lambda b: None, lambda m: None)
    with pytest.raises(_lib.PtnnError, match="communicator"):
        sh.lfo("train", **one)
    sh.close()


def test_leave_future_out_end_to_end(tmp_path):
    from ptnn_amd.parallel_tempering import elpd_compare, lfo_refit_seed
    d = parity.datasets()
    tr, te = d["sunspot_train"], d["sunspot_test"]
    N, L = len(tr), len(tr) - 12
    pt = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path)
    pt.run_chains()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = pt.leave_future_out(min_train=L, refit=False)
        good_k = pt.predictive_accuracy("train").good_k
    assert plain.n_refits == 0 and not np.any(plain.exact) and np.all(plain.fit_origin == N) and plain.k_threshold == good_k
    # a threshold low enough to force refits: the largest k-hat of the first origins of the walk that the next one exceeds
    kw = plain.khat[::-1]                                                   # walk order: backward from the fit
    j = next(j for j in range(1, kw.size) if kw[j] > np.max(kw[:j]))
    thr = float(np.max(kw[:j]))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lfo = pt.leave_future_out(min_train=L, k_threshold=thr, max_refits=2)
    # past the last allowed refit the origins keep their k-hat, and a warning says so when one is above the threshold
    left_high = bool(np.any(~(lfo.khat <= thr) & ~lfo.exact))
    assert left_high == any("max_refits = 2" in str(w.message) for w in caught)
    assert left_high <= (lfo.n_refits == 2) and np.all(lfo.khat[~lfo.exact & (lfo.origins > lfo.refit_origins[-1])] <= thr)
    assert 1 <= lfo.n_refits <= 2 and lfo.refit_origins[0] == N - 1 - j and lfo.k_threshold == thr
    print(f"end to end: threshold {thr:.4f}, refits at {lfo.refit_origins}, k-hat {np.round(lfo.khat, 3).tolist()}")
    assert np.array_equal(lfo.exact, np.isin(lfo.origins, lfo.refit_origins)) and np.all(np.isinf(lfo.khat[lfo.exact]))
    assert lfo.elpd_lfo == pytest.approx(np.sum(lfo.elpd_lfo_i), rel=1e-14) and lfo.se_elpd_lfo > 0 and lfo.block == 1
    # the origins scored from the first fit are those of refit=False
    first = lfo.fit_origin == N
    assert first.sum() == j and np.array_equal(lfo.elpd_lfo_i[first], plain.elpd_lfo_i[first]) and np.array_equal(lfo.khat[first], plain.khat[first])
    # every refit origin: lppd of that row from a sampler built by hand on the rows before it, with the derived seed
    for i in lfo.refit_origins:
        hand = _pt(orc.TASK_REG, (4, 5, 1), tr[:i], te, 4, 200, tmp_path, seed=lfo_refit_seed(SEED, i))
        hand.run_chains()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa = hand.predictive_accuracy(tr[i:i + 1])
        assert lfo.elpd_lfo_i[lfo.origins == i][0] == pytest.approx(pa.lppd_i[0], rel=1e-9)
    # reproducible from the seed
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = pt.leave_future_out(min_train=L, k_threshold=thr, max_refits=2)
        for k in ("elpd_lfo_i", "khat", "tail_len", "fit_origin", "exact"):
            assert np.array_equal(getattr(again, k), getattr(lfo, k)), k
        assert again.refit_origins == lfo.refit_origins
        # a fit the caller supplies; the sequential score of the test rows; a paired comparison
        mine = pt.leave_future_out(min_train=L, k_threshold=thr, max_refits=1,
                                   refit=lambda rows: (lambda p: (p.run_chains(), p)[1])(_pt(orc.TASK_REG, (4, 5, 1), rows, te, 4, 200, tmp_path, seed=7)))
        assert mine.refit_origins == lfo.refit_origins[:1] and np.array_equal(mine.elpd_lfo_i[first], lfo.elpd_lfo_i[first])
        seq = pt.leave_future_out(data="test", block=2, refit=False)
        assert seq.origins[0] == N and seq.origins[-1] == N + len(te) - 2 and seq.exact[0] and not np.any(seq.exact[1:])
        diff = elpd_compare(lfo, plain)
    assert diff["elpd_lfo_diff"] == pytest.approx(lfo.elpd_lfo - plain.elpd_lfo, rel=1e-12, abs=1e-12)
