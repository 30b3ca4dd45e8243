"""Posterior predictive on the GPU (ptnn_predict / posterior_predictive): network outputs of the sampled chains on train, test
or caller rows, reduced to the mean, exact percentile bands and class votes -- checked against the oracle's forward pass in
float64 and against numpy on the device's own samples."""
import numpy as np
import pytest

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


def _outputs(task, X, cols, topo):
    """Oracle outputs (float64) of every weight vector in cols [P, M] on rows X: [M, n_rows, O]; CLS: softmax."""
    out = np.stack([orc.forward(X, cols[:, j].astype(np.float64), topo)[1] for j in range(cols.shape[1])])
    if task == orc.TASK_CLS:
        e = np.exp(out)
        out = e / e.sum(axis=2, keepdims=True)
    return out


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


PCTS = (0, 5, 50, 95, 100, 37.5)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def test_regression_sunspot(sunspot):
    pt, res, d = sunspot
    posterior = res[0]
    R, S = 8, 600
    b = int(S * 0.5)
    pred = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
    M = R * (S - b)
    assert pred.n_samples == M and pred.samples.shape == (M, 198, 1)
    want = _outputs(orc.TASK_REG, d["sunspot_test"][:, :4], posterior, (4, 5, 1))
    assert np.max(np.abs(pred.samples - want)) <= 1e-5
    distinct, counts = _runs(posterior, R)
    assert pred.n_distinct == len(counts) and pred.n_distinct < M
    s64 = pred.samples.astype(np.float64)
    np.testing.assert_allclose(pred.mean, s64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(pred.percentiles[q], np.percentile(s64, q, axis=0)), q
    assert pred.vote is None and pred.pred_class is None
    # the train rows, and caller rows given with extra columns (pt.testdata as it is)
    tr = pt.posterior_predictive("train", return_samples=True)
    assert tr.samples.shape == (M, 298, 1)
    assert np.max(np.abs(tr.samples - _outputs(orc.TASK_REG, d["sunspot_train"][:, :4], posterior, (4, 5, 1)))) <= 1e-5
    xh = pt.posterior_predictive(pt.testdata, percentiles=PCTS)
    assert np.array_equal(xh.mean, pred.mean)
    for q in PCTS:
        assert np.array_equal(xh.percentiles[q], pred.percentiles[q])


@pytest.mark.parametrize("name,topo", [("iris", (4, 12, 3)), ("ions", (34, 50, 2))])
def test_classification(name, topo, tmp_path):
    d = parity.datasets()
    R, S = 8, 400
    pt = _pt(orc.TASK_CLS, topo, d[name + "_train"], d[name + "_test"], R, S, tmp_path, lg=True, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    pred = pt.posterior_predictive("test", return_samples=True)
    M = R * (S - S // 2)
    assert pred.n_samples == M
    want = _outputs(orc.TASK_CLS, d[name + "_test"][:, :topo[0]], res[0], topo)
    assert np.max(np.abs(pred.samples - want)) <= 1e-5
    assert np.max(np.abs(pred.samples.astype(np.float64).sum(axis=2) - 1.0)) <= 1e-6
    am = np.argmax(pred.samples, axis=2)                                           # [M, n_rows]
    votes = np.stack([(am == c).sum(axis=0) for c in range(topo[2])], axis=1) / M
    assert np.array_equal(pred.vote, votes)
    assert np.array_equal(pred.pred_class, np.argmax(pred.mean, axis=1))
    # the same vectors through weights=, expanded and as distinct vectors with multiplicities: bit-identical
    for w in (res[0].T, _runs(res[0], R)):
        alt = pt.posterior_predictive("test", weights=w)
        assert np.array_equal(alt.vote, pred.vote) and np.array_equal(alt.mean, pred.mean)
        for q in (5, 95):
            assert np.array_equal(alt.percentiles[q], pred.percentiles[q])


@pytest.mark.parametrize("H", [256, 512])
def test_wide_net_compact_traces(H, tmp_path):
    d = parity.datasets()
    R, S = 4, 200
    pt = _pt(orc.TASK_REG, (32, H, 1), d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    res = pt.run_chains()
    pred = pt.posterior_predictive("test", return_samples=True)
    want = _outputs(orc.TASK_REG, d["synth32_test"][:, :32], res[0], (32, H, 1))
    assert np.max(np.abs(pred.samples - want)) <= 1e-4
    b = S // 2
    src = pt._sampler.trace_rows()[:, b:, 7].copy().view(np.int32)              # TR_SRC: the row holding the step's vector
    runs = sum(1 + int(np.count_nonzero(src[c, 1:] != src[c, :-1])) for c in range(R))
    assert pred.n_distinct == runs
    alt = pt.posterior_predictive("test", weights=res[0].T)
    assert np.array_equal(alt.mean, pred.mean)


def test_sources_agree(sunspot):
    pt, res, _ = sunspot
    ref = pt.posterior_predictive("test", percentiles=PCTS)
    for w in (res[0].T, res[0], _runs(res[0], 8)):
        alt = pt.posterior_predictive("test", percentiles=PCTS, weights=w)
        assert alt.n_samples == ref.n_samples and alt.n_distinct == ref.n_distinct
        assert np.array_equal(alt.mean, ref.mean)
        for q in PCTS:
            assert np.array_equal(alt.percentiles[q], ref.percentiles[q]), q


def test_selection(sunspot):
    pt, res, d = sunspot
    tr = pt._sampler.traces()["pos_w"]                                            # [R, S, P]
    S = 600
    cold = int(np.argmin(pt.temperatures))
    cases = [(dict(chains="cold"), tr[cold:cold + 1, S // 2:]), (dict(chains=[3]), tr[3:4, S // 2:]),
             (dict(chains=[5, 1]), tr[[5, 1], S // 2:]), (dict(thin=3), tr[:, S // 2::3]), (dict(burn_in=0.25), tr[:, S // 4:])]
    X = d["sunspot_test"][:, :4]
    for kw, sl in cases:
        pred = pt.posterior_predictive("test", return_samples=True, **kw)
        w = sl.reshape(-1, sl.shape[2])
        assert pred.n_samples == w.shape[0], kw
        assert np.max(np.abs(pred.samples - _outputs(orc.TASK_REG, X, w.T, (4, 5, 1)))) <= 1e-5, kw
        alt = pt.posterior_predictive("test", weights=w)
        assert np.array_equal(alt.mean, pred.mean), kw
        for q in (5, 95):
            assert np.array_equal(alt.percentiles[q], pred.percentiles[q]), kw


def test_chunking_changes_nothing(sunspot, monkeypatch):
    pt, _, _ = sunspot
    ref = pt.posterior_predictive("train", percentiles=PCTS, return_samples=True)
    n_rows = ref.mean.shape[0]
    monkeypatch.setenv("PTNN_PREDICT_SCRATCH_BYTES", str(ref.n_distinct * 4 * (n_rows // 5)))   # >= 5 blocks of rows
    got = pt.posterior_predictive("train", percentiles=PCTS, return_samples=True)
    assert np.array_equal(got.mean, ref.mean) and np.array_equal(got.samples, ref.samples)
    for q in PCTS:
        assert np.array_equal(got.percentiles[q], ref.percentiles[q])
    monkeypatch.setenv("PTNN_PREDICT_SCRATCH_BYTES", "1")                          # one row per block
    one = pt.posterior_predictive("train", percentiles=PCTS)
    assert np.array_equal(one.mean, ref.mean)


def test_no_side_effects(tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        pt = _pt(orc.TASK_CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        (tmp_path / str(call)).mkdir(exist_ok=True)
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(0, 100)["pos_w"].reshape(-1, pt.num_param)
            pred = pt.posterior_predictive("test", weights=w)
            assert pred.n_samples == 800
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
        pt.posterior_predictive("test")
    w = np.asarray(pt._w0, np.float32)
    assert pt.posterior_predictive("test", weights=w).n_samples == 4        # weights= works before any run
    res = pt.run_chains()
    with pytest.raises(ValueError, match="n_in"):
        pt.posterior_predictive(te[:, :3])
    M = 4 * 100
    with pytest.raises(_lib.PtnnError, match="rank"):
        pt._sampler.predict("test", step0=100, nsteps=100, ranks=[M])
    ok = pt.posterior_predictive("test")                                      # the handle is still usable
    assert ok.n_samples == M and np.array_equal(ok.mean, pt.posterior_predictive("test", weights=res[0].T).mean)
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls_res = ls.run_chains()
    with pytest.raises(ValueError, match="label_swap"):
        ls.posterior_predictive("test")
    assert ls.posterior_predictive("test", weights=ls_res[0].T).n_samples == M
    st = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, trace_capacity=64)
    st_res = st.run_chains()
    with pytest.raises(ValueError, match="trace_capacity"):
        st.posterior_predictive("test")
    assert st.posterior_predictive("test", weights=st_res[0].T).n_samples == M
