"""Posterior predictive (ptnn_predict) and predictive accuracy (ptnn_elpd) at every compiled shape of PTNN_SHAPES: the per-shape
predict_forward_kernel<TASK, I, O> against the float64 oracle at hidden sizes that leave waves idle, give every vector-group
size NV the host picks, and take the wide-net path; the reductions at their edges (exact ties in the class vote, one sample,
one vector of multiplicity 10^6, the 16-rank limit, the PSIS tail cap); and more caller rows than one grid column of 64-row
tiles holds.  The vectors are uploaded through weights=, so no case needs a sampling run except the two trace-sourced ones."""
import math
import warnings

import numpy as np
import pytest

import elpd_ref as ref
import parity
from parity import orc
from test_gpu_elpd import _check_oracle, _oracle_ll, _same
from test_gpu_predict import PCTS, _outputs, _pt, _runs

pytestmark = pytest.mark.gpu

WAVE = 64
PRED_MAX_NV = 16
MAX_RANKS = 16                          # PTNN_PREDICT_MAX_RANKS
TAIL_CAP = 4096                         # PTNN_ELPD_TAIL_CAP


def _nv(topo):
    """Vectors per forward work-group, as ptnn_predict / ptnn_elpd pick it: 48 KiB of LDS over (staged vector + 4 waves' partial
    sums + the transposed tile)."""
    I, H, O = topo
    P = I * H + H * O + H + O
    per_vec = (P + 3) // 4 * 4 + 5 * O * WAVE
    return max(1, min(PRED_MAX_NV, 12288 // per_vec))


def _data(task, topo, seed, n_tr=150, n_te=53):
    """Seeded Gaussian inputs; classification labels from the argmax of a random projection, with classes 0 and O - 1 present in
    both sets; regression targets in (0, 1)."""
    I, _, O = topo
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_tr + n_te, I))
    if task == orc.TASK_CLS:
        proj = rng.standard_normal((I, O))
        y = np.argmax(X @ proj + 0.5 * rng.standard_normal((n_tr + n_te, O)), axis=1).astype(np.float64)
        y[[0, 1, n_tr, n_tr + 1]] = [0, O - 1, O - 1, 0]
    else:
        y = rng.uniform(0.1, 0.9, n_tr + n_te)
    data = np.hstack([X, y[:, None]])
    return data[:n_tr], data[n_tr:]


def _vectors(topo, n, seed, spread=0.5):
    """n weight vectors [n, P] float32 around one centre, scaled so that no unit saturates by much: every output stays above
    2^-20, where the device's double sums of fp32 outputs are exact (their order cannot change a bit)."""
    I, H, O = topo
    P = I * H + H * O + H + O
    rng = np.random.default_rng(seed)
    scale = np.concatenate([np.full(I * H, 2.0 / math.sqrt(I)), np.full(H * O, 2.0 / math.sqrt(H)), np.full(H, 0.5), np.full(O, 0.5)])
    centre = rng.standard_normal(P)
    w = (centre[None, :] + spread * rng.standard_normal((n, P))) * scale[None, :]
    return w.astype(np.float32)


def _make(task, topo, tmp_path, seed):
    train, test = _data(task, topo, seed)
    kw = dict(lr=0.01, maxtemp=10) if task == orc.TASK_CLS else {}
    return _pt(task, topo, train, test, 4, 20, tmp_path, **kw), train, test


def _check_predictive(pred, task, X, want, topo):
    """One posterior_predictive result with samples against the oracle outputs `want` [M, n_rows, O] and numpy on its samples."""
    O = topo[2]
    M = want.shape[0]
    assert pred.n_samples == M and pred.samples.shape == (M, X.shape[0], O)
    assert np.max(np.abs(pred.samples - want)) <= 1e-5
    s64 = pred.samples.astype(np.float64)
    np.testing.assert_allclose(pred.mean, s64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(pred.percentiles[q], np.percentile(s64, q, axis=0)), q
    if task == orc.TASK_CLS:
        assert np.max(np.abs(s64.sum(axis=2) - 1.0)) <= 1e-6
        am = np.argmax(pred.samples, axis=2)
        votes = np.stack([(am == c).sum(axis=0) for c in range(O)], axis=1) / M
        assert np.array_equal(pred.vote, votes)
        assert np.array_equal(pred.pred_class, np.argmax(pred.mean, axis=1))
    else:
        assert pred.vote is None and pred.pred_class is None


def _same_pred(a, b, samples=True):
    assert a.n_samples == b.n_samples
    assert np.array_equal(a.mean, b.mean)
    for q in a.percentiles:
        assert np.array_equal(a.percentiles[q], b.percentiles[q]), q
    if a.vote is not None or b.vote is not None:
        assert np.array_equal(a.vote, b.vote) and np.array_equal(a.pred_class, b.pred_class)
    if samples:
        assert np.array_equal(a.samples, b.samples)


# (task, I, O) of PTNN_SHAPES x hidden sizes: H < 4 (waves without a hidden unit), the problem table's H (the classification
# shapes' NV = 15, 2, 6, 3, 1), and a wide H in (64, 512] (100, 200 and 300 are not multiples of 32); five more regression
# sizes give the vector-group sizes NV no other case reaches, so that every NV in [1, 16] runs
REG, CLS = orc.TASK_REG, orc.TASK_CLS
OUTPUT_CASES = [
    (REG, (4, 2, 1)), (REG, (4, 5, 1)), (REG, (4, 100, 1)),
    (REG, (5, 3, 1)), (REG, (5, 10, 1)), (REG, (5, 256, 1)),
    (REG, (32, 1, 1)), (REG, (32, 64, 1)), (REG, (32, 300, 1)),
    (REG, (4, 88, 1)), (REG, (4, 140, 1)), (REG, (4, 160, 1)), (REG, (4, 190, 1)), (REG, (4, 220, 1)),   # NV = 14, 10, 9, 8, 7
    (CLS, (4, 3, 3)), (CLS, (4, 12, 3)), (CLS, (4, 200, 3)),
    (CLS, (34, 2, 2)), (CLS, (34, 50, 2)), (CLS, (34, 512, 2)),
    (CLS, (9, 3, 2)), (CLS, (9, 12, 2)), (CLS, (9, 96, 2)),
    (CLS, (11, 2, 10)), (CLS, (11, 50, 10)), (CLS, (11, 100, 10)),
    (CLS, (20, 3, 2)), (CLS, (20, 50, 2)), (CLS, (20, 160, 2)),
    (CLS, (16, 1, 10)), (CLS, (16, 30, 10)), (CLS, (16, 130, 10)),
    (CLS, (6, 3, 18)), (CLS, (6, 25, 18)), (CLS, (6, 200, 18)),
]


def test_output_cases_reach_every_vector_group_size():
    assert {_nv(topo) for _, topo in OUTPUT_CASES} == set(range(1, PRED_MAX_NV + 1))


@pytest.mark.parametrize("task,topo", OUTPUT_CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}" for t, (i, h, o) in OUTPUT_CASES])
def test_outputs_at_every_compiled_shape(task, topo, tmp_path, monkeypatch):
    I, H, O = topo
    seed = I * 1000 + H * 10 + O
    pt, train, _ = _make(task, topo, tmp_path, seed)
    NV = _nv(topo)
    U = NV * max(2, -(-4 // NV)) + 1                                  # not a multiple of NV (NV > 1), at least 5 vectors
    Wd = _vectors(topo, U, seed + 1)
    rng = np.random.default_rng(seed + 2)
    mult = rng.integers(0, 4, U).astype(np.int32)
    mult[1] = 0
    mult[0] = max(mult[0], 1)
    W = np.repeat(Wd, mult, axis=0)                                   # the expanded multiset, zero-multiplicity vectors dropped
    Xall = train[:, :I]
    fd = _outputs(task, Xall, Wd.T.astype(np.float64), topo)           # oracle outputs of the distinct vectors on every row
    want_all = np.repeat(fd, mult, axis=0)
    for n in (1, 63, 64, 65):                                         # caller rows at the 64-row tile edges
        pred = pt.posterior_predictive(Xall[:n], percentiles=PCTS, weights=W, return_samples=True)
        _check_predictive(pred, task, Xall[:n], want_all[:, :n], topo)
    full = pt.posterior_predictive("train", percentiles=PCTS, weights=W, return_samples=True)
    _check_predictive(full, task, Xall, want_all, topo)
    assert full.n_distinct == np.count_nonzero(mult)
    # the sums of the mean are exact in double when every output is above 2^-20: no summation order can change a bit
    assert full.samples.min() >= 2.0 ** -20
    # (distinct, multiplicity) with zero multiplicities: bit-identical to the expanded vectors
    alt = pt.posterior_predictive("train", percentiles=PCTS, weights=(Wd, mult), return_samples=True)
    assert alt.n_distinct == U
    _same_pred(alt, full)
    # blocks of 65 rows (tiles straddle the block starts), then one row per block: bit-identical to one block
    for rows_blk in (65, 1):
        monkeypatch.setenv("PTNN_PREDICT_SCRATCH_BYTES", str(full.n_distinct * 4 * O * rows_blk))
        _same_pred(pt.posterior_predictive("train", percentiles=PCTS, weights=W, return_samples=True), full)
    monkeypatch.delenv("PTNN_PREDICT_SCRATCH_BYTES")


# ---- ties, degenerate selections, the rank limit
MANY = [(6, 25, 18), (11, 50, 10)]


@pytest.mark.parametrize("topo", MANY, ids=["chess", "wine"])
@pytest.mark.parametrize("tie", ["3,7", "0,last", "all"])
def test_vote_ties_go_to_the_lowest_class(topo, tie, tmp_path):
    I, H, O = topo
    classes = {"3,7": [3, 7], "0,last": [0, O - 1], "all": list(range(O))}[tie]
    pt, train, _ = _make(CLS, topo, tmp_path, 7 * O + len(classes))
    W = _vectors(topo, 5, 11 + len(classes))
    W[:, [topo[0] * H + H * O + H + c for c in classes]] = -1.0e4     # B2: those outputs saturate to exactly 1.0f
    X = train[:, :I]
    pred = pt.posterior_predictive(X, weights=W, return_samples=True)
    s = pred.samples
    # the tie is real in fp32: every tied class holds the row's maximum, bit for bit
    assert np.all(s[:, :, classes] == s.max(axis=2, keepdims=True))
    assert np.max(np.abs(s - _outputs(CLS, X, W.T.astype(np.float64), topo))) <= 1e-5
    first = min(classes)
    assert np.all(np.argmax(s, axis=2) == first)
    want = np.zeros((X.shape[0], O))
    want[:, first] = 1.0
    assert np.array_equal(pred.vote, want)
    assert np.all(pred.pred_class == first)


@pytest.mark.parametrize("topo", MANY, ids=["chess", "wine"])
def test_degenerate_selections(topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(CLS, topo, tmp_path, 31 + O)
    X = train[:65, :I]
    w = _vectors(topo, 1, 5)
    one = pt.posterior_predictive(X, percentiles=PCTS, weights=w, return_samples=True)          # M = 1
    assert one.n_samples == 1 and one.n_distinct == 1
    f = one.samples[0]
    assert np.max(np.abs(f - _outputs(CLS, X, w.T.astype(np.float64), topo)[0])) <= 1e-5
    onehot = (np.arange(O)[None, :] == np.argmax(f, axis=1)[:, None]).astype(np.float64)
    for pred in (one, pt.posterior_predictive(X, percentiles=PCTS, weights=(w, [10 ** 6]))):   # one vector, 10^6 times
        assert np.array_equal(pred.mean, f.astype(np.float64))
        for q in PCTS:
            assert np.array_equal(pred.percentiles[q], f.astype(np.float64)), q
        assert np.array_equal(pred.vote, onehot)
    big = pt._sampler.predict(X, w=w, multiplicity=[10 ** 6], ranks=[0, 499999, 999999], vote=True)
    assert big["n_samples"] == 10 ** 6 and big["n_distinct"] == 1
    for k in range(3):
        assert np.array_equal(big["order_stats"][k], f)


@pytest.mark.parametrize("topo", MANY, ids=["chess", "wine"])
def test_rank_limit(topo, tmp_path):
    from ptnn_amd import _lib
    I, H, O = topo
    pt, train, _ = _make(CLS, topo, tmp_path, 57 + O)
    X = train[:65, :I]
    Wd = _vectors(topo, 41, 9)
    mult = np.resize(np.array([3, 1, 0, 2], np.int32), 41)
    M = int(mult.sum())
    assert M == 63
    # np.percentile(method="linear") at p interpolates the 0-based ranks floor(62 p / 100) and the one above
    p16 = [0, 10, 20, 30, 40, 50, 60, 70]
    ranks16 = [0, 1, 6, 7, 12, 13, 18, 19, 24, 25, 31, 32, 37, 38, 43, 44]
    assert len(ranks16) == MAX_RANKS
    pred = pt.posterior_predictive(X, percentiles=p16, weights=(Wd, mult), return_samples=True)
    s64 = pred.samples.astype(np.float64)
    assert np.max(np.abs(pred.samples - np.repeat(_outputs(CLS, X, Wd.T.astype(np.float64), topo), mult, axis=0))) <= 1e-5
    for q in p16:
        assert np.array_equal(pred.percentiles[q], np.percentile(s64, q, axis=0)), q
    # the same 16 ranks straight to the device: exactly the sorted samples at those ranks
    raw = pt._sampler.predict(X, w=Wd, multiplicity=mult, ranks=ranks16)
    srt = np.sort(pred.samples, axis=0)
    for k, r in enumerate(ranks16):
        assert np.array_equal(raw["order_stats"][k], srt[r]), r
    p17 = p16 + [100]                                                 # adds rank 62 alone: 17 ranks
    with pytest.raises(ValueError, match="17 order statistics"):
        pt.posterior_predictive(X, percentiles=p17, weights=(Wd, mult))
    with pytest.raises(_lib.PtnnError, match="n_ranks"):
        pt._sampler.predict(X, w=Wd, multiplicity=mult, ranks=ranks16 + [62])
    again = pt.posterior_predictive(X, percentiles=p16, weights=(Wd, mult))   # the handle is still usable
    _same_pred(again, pred, samples=False)


# ---- ELPD at the classification shapes the sampler tests cover and the predictive tests did not
ELPD_CASES = [(9, 12, 2), (11, 50, 10), (20, 50, 2), (16, 30, 10), (6, 25, 18), (16, 100, 10)]


@pytest.mark.parametrize("topo", ELPD_CASES, ids=["cancer", "wine", "bank", "pendigit", "chess", "pendigit-wide"])
def test_elpd_classification_shapes(topo, tmp_path, monkeypatch):
    I, H, O = topo
    seed = 3 * I + H + O
    pt, train, test = _make(CLS, topo, tmp_path, seed)
    for rows in (train, test):
        assert rows[:, I].min() == 0 and rows[:, I].max() == O - 1
    W = _vectors(topo, 60, seed + 1, spread=0.2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, rows in (("train", train), ("test", test)):
            pa = pt.predictive_accuracy(name, weights=W, return_pointwise=True)
            assert pa.n_samples == 60 and pa.log_lik.shape == (60, rows.shape[0])
            _check_oracle(pa, _oracle_ll(CLS, rows, W.T, topo))
            _same(pt.predictive_accuracy(rows, weights=W), pa)                   # the same rows from the host
        pa = pt.predictive_accuracy("train", weights=W, return_pointwise=True)
        # (distinct, multiplicity), zero multiplicities included, against the expanded vectors
        mult = np.resize(np.array([2, 0, 1, 3], np.int32), 60)
        expd = pt.predictive_accuracy("train", weights=np.repeat(W, mult, axis=0), return_pointwise=True)
        mlt = pt.predictive_accuracy("train", weights=(W, mult), return_pointwise=True)
        _same(mlt, expd)
        assert np.array_equal(mlt.log_lik, expd.log_lik)
        _check_oracle(expd, _oracle_ll(CLS, train, np.repeat(W, mult, axis=0).T, topo))
        # blocks of 65 rows, then one row per block: bit-identical to one block
        for rows_blk in (65, 1):
            monkeypatch.setenv("PTNN_ELPD_SCRATCH_BYTES", str(60 * (4 * O + 8) * rows_blk))
            blk = pt.predictive_accuracy("train", weights=W, return_pointwise=True)
            _same(blk, pa)
            assert np.array_equal(blk.log_lik, pa.log_lik)
        monkeypatch.delenv("PTNN_ELPD_SCRATCH_BYTES")


def _tail_m(S):
    return int(math.ceil(min(0.2 * S, 3.0 * math.sqrt(S))))


def test_elpd_tail_cap_edge(tmp_path):
    from ptnn_amd import _lib
    pt, _, _ = _make(CLS, (9, 12, 2), tmp_path, 5)
    S = int((TAIL_CAP / 3.0) ** 2) + 1
    while _tail_m(S + 1) <= TAIL_CAP:
        S += 1
    while _tail_m(S) > TAIL_CAP:
        S -= 1
    assert _tail_m(S) == TAIL_CAP and _tail_m(S + 1) == TAIL_CAP + 1
    rng = np.random.default_rng(17)
    n = 20000
    ll = rng.normal(-1.0, 0.6, (n, 3))
    mult = np.full(n, S // n, np.int32)
    mult[: S - int(mult.sum())] += 1
    assert int(mult.sum()) == S
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa = pt.predictive_accuracy(loglik=(ll, mult))
    assert pa.n_samples == S
    r = ref.elpd_rows(ll, mult)
    np.testing.assert_allclose(pa.lppd_i, r["lppd"], rtol=1e-9)
    np.testing.assert_allclose(pa.p_waic_i, r["p_waic"], rtol=1e-9)
    np.testing.assert_allclose(pa.elpd_loo_i, r["elpd_loo"], rtol=1e-9)
    assert np.all(np.isfinite(r["khat"])) and np.max(np.abs(pa.khat - r["khat"])) <= 1e-9
    out = pt._sampler.elpd(loglik=ll, multiplicity=mult)
    assert np.array_equal(out["tail_len"], r["tail_len"]) and out["tail_len"].max() <= TAIL_CAP
    mult[0] += 1                                                       # S + 1: M = 4097 must be refused, not truncated
    with pytest.raises(_lib.PtnnError, match="M = 4097"):
        pt.predictive_accuracy(loglik=(ll, mult))


# ---- the trace as the source at many-class shapes
@pytest.mark.parametrize("topo", [(6, 25, 18), (16, 30, 10)], ids=["chess", "pendigit"])
def test_trace_sourced_many_class(topo, tmp_path):
    I, H, O = topo
    train, test = _data(CLS, topo, 100 + O)
    R, S = 4, 100
    pt = _pt(CLS, topo, train, test, R, S, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    pred = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
    assert pred.n_samples == R * (S - S // 2)
    _check_predictive(pred, CLS, test[:, :I], _outputs(CLS, test[:, :I], res[0], topo), topo)
    for w in (res[0].T, _runs(res[0], R)):
        _same_pred(pt.posterior_predictive("test", percentiles=PCTS, weights=w, return_samples=True), pred)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa = pt.predictive_accuracy("test", return_pointwise=True)
        _check_oracle(pa, _oracle_ll(CLS, test, res[0], topo))
        _same(pt.predictive_accuracy("test", weights=res[0].T), pa)
        _same(pt.predictive_accuracy("test", weights=_runs(res[0], R)), pa)


# ---- more rows than one grid column of 64-row tiles holds (grid.y <= 65535)
def test_rows_past_one_grid_column(tmp_path, monkeypatch):
    topo = (4, 5, 1)
    d = parity.datasets()
    pt = _pt(REG, topo, d["sunspot_train"], d["sunspot_test"], 4, 20, tmp_path)
    n = 65535 * WAVE + 65
    rng = np.random.default_rng(65535)
    X = rng.standard_normal((n, 4)).astype(np.float32)
    w = _vectors(topo, 1, 3)
    f = orc.forward(X.astype(np.float64), w[0].astype(np.float64), topo)[1][:, 0]
    pred = pt.posterior_predictive(X, percentiles=(5, 95), weights=w)
    assert pred.n_samples == 1 and pred.mean.shape == (n, 1)
    err = np.abs(pred.mean[:, 0] - f)
    assert np.max(err[65535 * WAVE:]) <= 1e-5, "rows past the first 65535 tiles"
    assert np.max(err) <= 1e-5
    for q in (5, 95):
        assert np.array_equal(pred.percentiles[q], pred.mean), q
    # blocks of 2^21 rows instead of the default ones: bit-identical
    monkeypatch.setenv("PTNN_PREDICT_SCRATCH_BYTES", str(4 << 21))
    small = pt.posterior_predictive(X, percentiles=(5, 95), weights=w)
    _same_pred(small, pred, samples=False)
    # ELPD: the same rows with targets, two copies of the vector (p_waic needs S >= 2), eta given
    y = (f + 0.1 * rng.standard_normal(n)).astype(np.float32)
    eta = np.float32(-2.0)
    rows = np.hstack([X, y[:, None]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pa = pt.predictive_accuracy(rows, weights=(w, [2]), eta=[eta])
    assert pa.n_samples == 2 and pa.lppd_i.shape == (n,)
    tau2 = math.exp(float(eta))
    want = -0.5 * math.log(2 * math.pi * tau2) - 0.5 * (y.astype(np.float64) - f) ** 2 / tau2
    np.testing.assert_allclose(pa.lppd_i[65535 * WAVE:], want[65535 * WAVE:], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(pa.lppd_i, want, rtol=1e-5, atol=1e-4)
    assert np.all(pa.p_waic_i == 0.0)
    np.testing.assert_allclose(pa.elpd_loo_i, pa.lppd_i, rtol=1e-12, atol=1e-12)
    monkeypatch.setenv("PTNN_ELPD_SCRATCH_BYTES", str(4 << 21))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same(pt.predictive_accuracy(rows, weights=(w, [2]), eta=[eta]), pa)
