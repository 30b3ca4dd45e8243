"""Shapley attributions (ptnn_coalition_values, pt.shapley_values) on the GPU: exact and permutation tables against the float64
reference under the derived bound of tests/shapley_ref.py (K = 1, every case prints its worst err / bound); known answers; the
reductions exact on the device's own samples; the multiset of samples, the row block and the position of a coalition in the table
as things no value depends on; refusals by their text; untouched neighbours."""
import itertools

import numpy as np
import pytest

import parity
import shapley_ref as ref
from parity import orc
from test_gpu_analysis_shapes import _make, _vectors
from test_gpu_predict import PCTS, _pt, _runs

pytestmark = pytest.mark.gpu

U32 = ref.U32
REG, CLS = orc.TASK_REG, orc.TASK_CLS


def _worst_ratio(samples, X32, bg32, Wd, topo, task, masks, coef):
    """samples [U, n_rows, O, T] fp32 of the distinct vectors Wd -> max err / bound; asserts the bound element by element."""
    worst = 0.0
    for k in range(Wd.shape[0]):
        bound, want = ref.error_bound(X32, bg32, Wd[k], topo, task, masks, coef)
        err = np.abs(samples[k].astype(np.float64) - want)
        ratio = float(np.max(err / bound))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (k, ratio)
    return worst


# ---- exact Shapley values
@pytest.mark.parametrize("task,topo", [(REG, (4, 5, 1)), (REG, (5, 5, 1)), (CLS, (4, 12, 3)), (CLS, (6, 7, 18))],
                         ids=["reg-4-5-1", "reg-5-5-1", "cls-4-12-3", "cls-6-7-18"])
def test_exact_shapley(task, topo, tmp_path):
    from ptnn_amd.shapley import shapley_table
    I, H, O = topo
    pt, train, test = _make(task, topo, tmp_path, 50 + I + O)
    W = _vectors(topo, 4, 7 + I)
    X32, bg32 = test[:3, :I].astype(np.float32), train[:7, :I].astype(np.float32)
    sv = pt.shapley_values(X32, bg32, weights=W, percentiles=PCTS, return_samples=True)
    assert sv.method == "exact" and sv.n_coalitions == 1 << I and sv.samples.shape == (4, 3, O, I + 2) and np.array_equal(sv.background, bg32)
    masks, coef = shapley_table(I)
    worst = _worst_ratio(sv.samples, X32, bg32, W, topo, task, masks, coef)
    print(f"exact Shapley {'cls' if task else 'reg'}-{I}-{H}-{O}: worst err / bound = {worst:.4f}")
    own = pt.posterior_predictive(X32, weights=W, return_samples=True).samples
    for k in range(4):                                                  # and against the subset formula itself (1e-14: its own rounding)
        want = ref.shapley_exact(X32, bg32, W[k], topo, task)
        bound = ref.error_bound(X32, bg32, W[k], topo, task, masks, coef)[0]
        assert np.all(np.abs(sv.samples[k, :, :, :I].astype(np.float64) - want) <= bound[:, :, :I] + 1e-14)
        # v(all) is the net's own output on the row: two fp32 evaluations of one value, each within the bound
        assert np.all(np.abs(sv.samples[k, :, :, I + 1].astype(np.float64) - own[k]) <= 2 * bound[:, :, I + 1])
    # efficiency: sum_j phi_j = v(all) - v(empty), up to the I + 2 fp32 stores
    big = max(np.abs(sv.phi_mean).max(), np.abs(sv.fx_mean).max(), np.abs(sv.base).max())
    print(f"efficiency gap = {sv.efficiency_gap:.3e}, (I + 2) u max = {(I + 2) * U32 * big:.3e}")
    assert sv.efficiency_gap <= (I + 2) * U32 * big
    s64 = sv.samples.astype(np.float64)
    assert np.array_equal(sv.efficiency_gap, np.max(np.abs(sv.phi_mean.sum(axis=2) - (sv.fx_mean - sv.base))))
    np.testing.assert_allclose(sv.base, s64[:, 0, :, I].mean(axis=0), rtol=1e-12, atol=0)
    assert np.all(s64[:, :, :, I] == s64[:, :1, :, I])                  # v(empty) does not depend on the explained row
    # an input the nets do not read gets nothing; so does every input when every background row is the explained row
    W0 = W.copy()
    W0[:, 1 * H:2 * H] = 0.0                                            # W1[1, :] = 0
    z = pt.shapley_values(X32, bg32, weights=W0, return_samples=True)
    assert np.max(np.abs(z.samples[:, :, :, 1])) <= 1e-12 and np.max(np.abs(z.samples[:, :, :, 0])) > 1e-6
    assert np.all(z.importance[:, 1] <= 1e-12) and np.all(z.top_prob[:, 1] == 0)
    e = pt.shapley_values(X32[:1], np.repeat(X32[:1], 5, axis=0), weights=W, return_samples=True)
    assert np.max(np.abs(e.samples[:, :, :, :I])) <= 1e-12
    assert np.array_equal(e.samples[:, :, :, I], e.samples[:, :, :, I + 1])


# ---- permutation mode
@pytest.mark.parametrize("task,topo", [(CLS, (34, 3, 2)), (CLS, (16, 4, 10))], ids=["cls-34-3-2", "cls-16-4-10"])
def test_permutation_shapley(task, topo, tmp_path):
    from ptnn_amd.shapley import shapley_table
    I, H, O = topo
    pt, train, test = _make(task, topo, tmp_path, 90 + I)
    W = _vectors(topo, 3, 17 + I)
    X32, bg32 = test[:2, :I].astype(np.float32), train[:5, :I].astype(np.float32)
    rng = np.random.default_rng(I)
    a, b = rng.permutation(I), rng.permutation(I)
    orders = np.stack([a, a[::-1], b, b[::-1]])                          # two antithetic pairs
    sv = pt.shapley_values(X32, bg32, weights=W, permutations=orders, return_samples=True)
    masks, coef = shapley_table(I, permutations=orders)
    assert sv.method == "permutation" and sv.n_coalitions == masks.size <= 4 * (I - 1) + 2
    worst = _worst_ratio(sv.samples, X32, bg32, W, topo, task, masks, coef)
    print(f"permutation Shapley cls-{I}-{H}-{O}, {masks.size} coalitions: worst err / bound = {worst:.4f}")
    for k in range(3):
        want = ref.shapley_permutation(X32, bg32, W[k], topo, task, orders)
        bound = ref.error_bound(X32, bg32, W[k], topo, task, masks, coef)[0][:, :, :I]
        assert np.all(np.abs(sv.samples[k, :, :, :I].astype(np.float64) - want) <= bound + 1e-14)
    big = max(np.abs(sv.phi_mean).max(), np.abs(sv.fx_mean).max(), np.abs(sv.base).max())
    assert sv.efficiency_gap <= (I + 2) * U32 * big                     # every order telescopes


def test_all_orders_give_the_exact_values(tmp_path):
    from ptnn_amd.shapley import shapley_table
    topo = (4, 5, 1)
    pt, train, test = _make(REG, topo, tmp_path, 31)
    W = _vectors(topo, 4, 9)
    X32, bg32 = test[:3, :4].astype(np.float32), train[:6, :4].astype(np.float32)
    orders = np.array(list(itertools.permutations(range(4))))
    sv = pt.shapley_values(X32, bg32, weights=W, permutations=orders, return_samples=True)
    masks, coef = shapley_table(4, permutations=orders)
    assert sv.n_coalitions == 16
    worst = 0.0
    for k in range(4):
        want = ref.shapley_exact(X32, bg32, W[k], topo, REG)
        bound = ref.error_bound(X32, bg32, W[k], topo, REG, masks, coef)[0][:, :, :4]
        err = np.abs(sv.samples[k, :, :, :4].astype(np.float64) - want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound + 1e-14)
    print(f"all 24 orders at 4-5-1 against the exact values: worst err / bound = {worst:.4f}")


# ---- the reductions, and what the outputs depend on
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def _row_means_abs(s):
    """s [M, n_rows, O, T] fp32 -> a_s [M, O, T] fp32: |.| summed over the rows in ascending order in double, / n_rows."""
    a = np.zeros((s.shape[0],) + s.shape[2:])
    for n in range(s.shape[1]):
        a += np.abs(s[:, n].astype(np.float64))
    return (a / np.float64(s.shape[1])).astype(np.float32)


def _check_reductions(sv, M):
    s = sv.samples
    I = s.shape[3] - 2
    s64 = s.astype(np.float64)
    assert sv.n_samples == M == s.shape[0]
    # phi has both signs: its mean is held to 1e-12 of the mean magnitude of what was summed
    assert np.all(np.abs(sv.phi_mean - s64[..., :I].mean(axis=0)) <= 1e-12 * np.abs(s64[..., :I]).mean(axis=0))
    np.testing.assert_allclose(sv.fx_mean, s64[..., I + 1].mean(axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(sv.base, s64[:, 0, :, I].mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(sv.phi_percentiles[q], np.percentile(s64[..., :I], q, axis=0)), q
        assert np.array_equal(sv.base_percentiles[q], np.percentile(s64[:, 0, :, I], q, axis=0)), q
    assert np.array_equal(sv.prob_positive, (s[..., :I] > 0).sum(axis=0) / np.float64(M))
    a = _row_means_abs(s)[..., :I]
    assert np.array_equal(sv.sample_importance, a)
    a64 = a.astype(np.float64)
    np.testing.assert_allclose(sv.importance, _row_means_abs(s).astype(np.float64)[..., :I].mean(axis=0), rtol=1e-6, atol=0)
    for q in PCTS:
        assert np.array_equal(sv.importance_percentiles[q], np.percentile(a64, q, axis=0)), q
    best = np.argmax(a, axis=2)
    assert np.array_equal(sv.top_prob, np.stack([(best == i).sum(axis=0) for i in range(I)], axis=1) / np.float64(M))


def _same(a, b, same_distinct=True):
    assert a.n_samples == b.n_samples and a.method == b.method and a.n_coalitions == b.n_coalitions
    for f in ("phi_mean", "fx_mean", "base", "importance"):
        if same_distinct:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        else:
            np.testing.assert_allclose(getattr(a, f), getattr(b, f), rtol=1e-13, atol=1e-18)
    for f in ("prob_positive", "top_prob", "sample_importance", "samples", "background"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for q in a.phi_percentiles:
        for f in ("phi_percentiles", "base_percentiles", "importance_percentiles"):
            assert np.array_equal(getattr(a, f)[q], getattr(b, f)[q]), (f, q)


def test_reductions_and_invariance(sunspot, monkeypatch):
    pt, res, d = sunspot
    topo = (4, 5, 1)
    X = d["sunspot_test"][:6, :4]
    kw = dict(max_background=9, percentiles=PCTS, return_samples=True)
    base = pt.shapley_values(X, "train", **kw)
    M = 4 * 100
    assert base.n_samples == M and base.samples.shape == (M, 6, 1, 6) and base.n_distinct < M and base.background.shape == (9, 4)
    tr = np.asarray(d["sunspot_train"])
    assert np.array_equal(base.background, tr[np.rint(np.linspace(0, tr.shape[0] - 1, 9)).astype(np.int64), :4].astype(np.float32))
    _check_reductions(base, M)
    # the importance is the weighted mean of the double row means
    s64 = np.abs(base.samples.astype(np.float64))
    rows = np.zeros((M, 1, 6))
    for n in range(6):
        rows += s64[:, n]
    np.testing.assert_allclose(base.importance, (rows / 6.0).mean(axis=0)[:, :4], rtol=1e-12, atol=0)
    distinct, counts = _runs(res[0], 4)
    assert base.n_distinct == len(counts)
    at = np.cumsum(counts) - counts
    from ptnn_amd.shapley import shapley_table
    masks, coef = shapley_table(4)
    worst = _worst_ratio(base.samples[at][::7], X.astype(np.float32), base.background, distinct[::7], topo, REG, masks, coef)
    print(f"exact Shapley, sunspot trace: worst err / bound = {worst:.4f}")
    # the trace against the same samples as weights, and as distinct vectors with multiplicities
    for w in (res[0].T, (distinct, counts)):
        alt = pt.shapley_values(X, "train", weights=w, **kw)
        assert alt.n_distinct == base.n_distinct
        _same(alt, base)
    # one row and a few rows per block
    for rows_blk in (1, 4):
        monkeypatch.setenv("PTNN_SHAP_SCRATCH_BYTES", str(base.n_distinct * 4 * 6 * rows_blk))
        _same(pt.shapley_values(X, "train", **kw), base)
    monkeypatch.delenv("PTNN_SHAP_SCRATCH_BYTES")
    # "test" and the same rows from the host; the cold chain, thinned, against its trace rows as weights
    assert np.array_equal(pt.shapley_values("test", max_background=3).phi_mean,
                          pt.shapley_values(d["sunspot_test"], d["sunspot_train"], max_background=3).phi_mean)
    cold = int(np.argmin(pt.temperatures))
    rows_ = pt._sampler.traces()["pos_w"]
    _same(pt.shapley_values(X, weights=rows_[cold, 100::3], **kw), pt.shapley_values(X, chains="cold", thin=3, **kw))


def test_a_value_does_not_depend_on_its_place_in_the_table(tmp_path):
    topo = (9, 6, 2)
    pt, train, test = _make(CLS, topo, tmp_path, 23)
    W = _vectors(topo, 11, 4)                                           # more vectors than one work-group stages
    X32, bg32 = test[:6, :9].astype(np.float32), train[:70, :9].astype(np.float32)
    masks = np.array([0, 0x1ff, 0x155, 0x0f0, 0x003, 0x1fe], np.uint64)
    sm = pt._sampler
    a = sm.coalition_values(X32, background=bg32, masks=masks, coef=np.eye(6), w=W, samples=True)["samples"]
    order = [4, 1, 2, 3, 0, 5]                                          # two coalitions swapped
    b = sm.coalition_values(X32, background=bg32, masks=masks[order], coef=np.eye(6), w=W, samples=True)["samples"]
    assert np.array_equal(b, a[..., order])
    # a coalition alone, one vector alone, one row alone: the same bits
    c = sm.coalition_values(X32[4:5], background=bg32, masks=masks[2:3], coef=np.eye(1), w=W[9:10], samples=True)["samples"]
    assert np.array_equal(c[0, 0, :, 0], a[9, 4, :, 2])
    # a functional of several coalitions is the double sum of their values in table order, rounded once
    coef = np.array([[0.5, -1.0], [0.25, 0.0], [0.0, 2.0], [-0.75, 0.125], [0.0, 0.0], [1.0, -0.5]])
    f = sm.coalition_values(X32, background=bg32, masks=masks, coef=coef, w=W, samples=True)["samples"]
    want = np.zeros(f.shape)
    for k in range(6):
        want += a[..., k:k + 1].astype(np.float64) * coef[k][None, None, None, :]
    size = np.zeros(f.shape)
    for k in range(6):
        size += np.abs(a[..., k:k + 1].astype(np.float64)) * np.abs(coef[k])[None, None, None, :]
    assert np.all(np.abs(f.astype(np.float64) - want) <= U32 * size + U32 * np.abs(want) + 1e-30)     # the fp32 stores of a, and f's own


# ---- refusals that need a handle, and the spec's own through the sampler
def test_refusals(tmp_path):
    from ptnn_amd import _lib
    topo = (6, 25, 18)
    pt, train, _ = _make(CLS, topo, tmp_path, 3)
    X = train[:5, :6]
    W = _vectors(topo, 3, 1)
    bg = train[5:9, :6].astype(np.float32)
    sm = pt._sampler
    ok = dict(background=bg, masks=np.array([0, 63], np.uint64), coef=np.eye(2), w=W)
    cases = [
        (dict(coef=np.zeros((2, 15))), r"n_terms = 15 x n_out = 18 = 270 accumulators: at most 256"),
        (dict(masks=np.array([0, 64], np.uint64)), r"masks\[1\] = 0x40 has a bit at or above n_in = 6"),
        (dict(masks=np.array([1 << 63, 3], np.uint64)), r"masks\[0\] = 0x8000000000000000 has a bit at or above n_in = 6"),
        (dict(background=np.where(np.arange(24).reshape(4, 6) == 13, np.nan, bg)), r"background\[2, 1\] = nan is not finite"),
        (dict(background=np.where(np.arange(24).reshape(4, 6) == 23, np.inf, bg)), r"background\[3, 5\] = inf is not finite"),
        (dict(background=np.zeros((257, 6), np.float32)), r"n_background = 257 outside \[1, 256\]"),
        (dict(background=np.zeros((0, 6), np.float32)), r"n_background = 0 outside \[1, 256\]"),
        (dict(masks=np.zeros(4097, np.uint64), coef=np.zeros((4097, 2))), r"n_coalitions = 4097 outside \[1, 4096\]"),
        (dict(coef=np.zeros((2, 65))), r"n_terms = 65 outside \[1, 64\]"),
        (dict(coef=np.array([[1.0, 0.0], [np.nan, 1.0]])), r"coef\[1, 0\] = nan \(coalition 1, term 0\) is not finite"),
        (dict(multiplicity=[0, 0, 0]), "holds no sample"),
        (dict(ranks=[0, 3]), r"rank 3 outside \[0, 3\)"),
        (dict(ranks2=[7]), r"rank 7 outside \[0, 3\)"),
        (dict(ranks2=list(range(17))), "n_ranks = 17"),
    ]
    for over, text in cases:
        with pytest.raises(_lib.PtnnError, match=text):
            sm.coalition_values(X, **dict(ok, **over))
    many = (2 ** 31 - 1) // (14 * 18) + 1                               # x 252 columns per row: past 2^31 - 1
    with pytest.raises(_lib.PtnnError, match="at most 2\\^31 - 1"):
        sm.coalition_values(np.zeros((many, 6), np.float32), **dict(ok, coef=np.zeros((2, 14))))
    with pytest.raises(ValueError, match=r"background must be \[n_background, 6\]"):
        sm.coalition_values(X, **dict(ok, background=np.zeros((4, 5), np.float32)))
    with pytest.raises(ValueError, match=r"coef must be \[2, n_terms\]"):
        sm.coalition_values(X, **dict(ok, coef=np.eye(3)))
    with pytest.raises(ValueError, match="percentiles"):
        pt.shapley_values(X, weights=W, percentiles=(101,))
    res = pt.shapley_values(X, bg, weights=W)                           # the handle is still usable
    assert res.n_samples == 3 and res.phi_mean.shape == (5, 18, 6) and res.method == "exact" and res.samples is None
    np.testing.assert_allclose(res.top_prob.sum(axis=1), 1.0, rtol=1e-12)
    # an output costs device work only when it is asked for: nothing but the counters
    lean = sm.coalition_values(X, **ok, mean=False, abs_mean=False)
    assert all(lean[k] is None for k in ("mean", "order_stats", "pos_count", "neg_count", "abs_mean", "abs_order_stats", "sample_abs", "samples"))
    assert lean["n_samples"] == 3 and lean["n_distinct"] == 3


# ---- untouched neighbours
def test_leaves_the_chains_and_other_calls_alone(tmp_path):
    d = parity.datasets()
    W = _vectors((4, 5, 1), 7, 19)

    def run(between):
        pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 60, tmp_path)
        assert pt.run_chains(max_steps=25) is None                      # stopped in mid-run
        sm = pt._sampler
        snap = lambda: (sm.state(), sm.trace_rows(0, 26), sm.traces(0, 26)["pos_w"], sm.steps_done())     # noqa: E731
        before = snap()
        if between:
            pt.shapley_values(d["sunspot_test"][:9], weights=W, percentiles=PCTS, max_background=5)
            pt.shapley_values(d["sunspot_train"][:4], "test", weights=(W, [2, 0, 1, 1, 3, 1, 1]), method="permutation", n_permutations=4,
                              seed=3, max_background=70, return_samples=True)
        after = snap()
        assert before[3] == after[3] == 25
        for k in before[0]:
            assert np.array_equal(before[0][k], after[0][k]), k
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        res = pt.run_chains(max_steps=10 ** 6)                          # the continuation
        pred = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
        if between:
            pt.shapley_values(d["sunspot_test"][:5], percentiles=PCTS, max_background=4)
            again = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
            assert np.array_equal(pred.mean, again.mean) and np.array_equal(pred.samples, again.samples)
        return res[0], sm.state(), sm.trace_rows(), pred.samples
    w0, s0, t0, p0 = run(False)
    w1, s1, t1, p1 = run(True)
    assert np.array_equal(w0, w1) and np.array_equal(t0, t1) and np.array_equal(p0, p1)
    for k in s0:
        assert np.array_equal(s0[k], s1[k]), k
