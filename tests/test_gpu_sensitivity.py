"""Input sensitivity (ptnn_sensitivity, pt.input_sensitivity) on the GPU: the per-shape sensitivity_forward_kernel<TASK, I, O> against
the float64 reference at every compiled shape under a derived forward-error bound; the reductions exact on the device's own
gradients; the multiset of samples as the only thing the outputs depend on; known answers; untouched neighbours.

The error bound of a gradient: |g_dev - g_ref| <= K u T + 1e-30 with u = 2^-24, T = sensitivity_ref.error_bound (first order, from
the oracle's float64 intermediates) and K = 1; 1e-30 because fp32 cannot hold what float64 holds in a fully saturated net.  Every
shape prints its worst err / (u T)."""
import numpy as np
import pytest

import parity
import sensitivity_ref as ref
from parity import orc
from test_gpu_analysis_shapes import _make, _vectors
from test_gpu_predict import PCTS, _pt, _runs

pytestmark = pytest.mark.gpu

WAVE = 64
SENS_MAX_NV = 16
K = 1.0
U32 = ref.U32
REG, CLS = orc.TASK_REG, orc.TASK_CLS


def _nv(topo):
    """Vectors per forward work-group, as ptnn_sensitivity picks it: 64 KiB of LDS over (staged vector + its 64-row tile of
    O x I gradients + the pad)."""
    I, H, O = topo
    per_vec = (orc.num_param(topo) + 3) // 4 * 4 + (O * I + 1) * WAVE
    return max(1, min(SENS_MAX_NV, 16384 // per_vec))


def _worst_ratio(dev, X, Wd, topo, task):
    """dev [U, n_rows, O, I] fp32 gradients of the distinct vectors Wd -> max err / (u T); asserts the bound element by element."""
    worst = 0.0
    X = np.asarray(X, np.float32).astype(np.float64)                   # the rows as the device holds them
    for k in range(Wd.shape[0]):
        w = Wd[k].astype(np.float64)
        err = np.abs(dev[k].astype(np.float64) - ref.jacobian(X, w, topo, task))
        T = ref.error_bound(X, w, topo, task)
        worst = max(worst, float(np.max(err / (U32 * T + 1e-300))))
        assert np.all(err <= K * U32 * T + 1e-30), (k, float(np.max(err / (U32 * T + 1e-300))))
    return worst


def _check_reductions(pt, X, weights, samples, sens):
    """Every reduced output against numpy float64 on the device's own fp32 gradients `samples` [M, n_rows, O, I]."""
    M = samples.shape[0]
    s64 = samples.astype(np.float64)
    assert sens.n_samples == M
    np.testing.assert_allclose(sens.grad_mean, s64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(sens.percentiles[q], np.percentile(s64, q, axis=0)), q
    assert np.array_equal(sens.prob_positive, (samples > 0).sum(axis=0) / np.float64(M))
    assert np.array_equal(sens.prob_negative, (samples < 0).sum(axis=0) / np.float64(M))
    a, q2 = ref.row_means(samples)
    np.testing.assert_allclose(sens.importance, a.mean(axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(sens.importance_rms, np.sqrt(q2.mean(axis=0)), rtol=1e-12, atol=0)
    w, mult = weights if isinstance(weights, tuple) else (weights, None)
    spots, ranks = pt._band_ranks(M, list(PCTS))
    raw = pt._sampler.sensitivity(X, w=w, multiplicity=mult, ranks2=ranks, sample_abs=True)
    assert np.array_equal(raw["sample_abs"], a.astype(np.float32))
    a32 = raw["sample_abs"].astype(np.float64)
    for q in PCTS:
        assert np.array_equal(sens.importance_percentiles[q], np.percentile(a32, q, axis=0)), q
    from ptnn_amd.parallel_tempering import top_share
    assert np.array_equal(sens.top_prob, top_share(raw["sample_abs"]))
    srt = np.sort(raw["sample_abs"], axis=0)
    for k, r in enumerate(ranks):
        assert np.array_equal(raw["abs_order_stats"][k], srt[r]), r


def _same(a, b, samples=True, same_distinct=True):
    """Bitwise equal.  The two weighted means of double row sums have a fixed summation order for a given list of distinct vectors;
    when the lists differ (zero-multiplicity vectors in one of them) they are compared to rounding."""
    assert a.n_samples == b.n_samples
    for f in ("grad_mean", "prob_positive", "prob_negative", "top_prob"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("importance", "importance_rms"):
        if same_distinct:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        else:
            np.testing.assert_allclose(getattr(a, f), getattr(b, f), rtol=1e-14, atol=0, err_msg=f)
    for q in a.percentiles:
        assert np.array_equal(a.percentiles[q], b.percentiles[q]), q
        assert np.array_equal(a.importance_percentiles[q], b.importance_percentiles[q]), q
    if samples:
        assert np.array_equal(a.samples, b.samples)


# (task, I, O) of PTNN_SHAPES x hidden sizes: H < 4 (the pairs of a work-group do not fill its waves), the problem table's H, a
# wide H in (64, 512]; seven more 4-H-1 sizes give the vector-group sizes NV no other case reaches
CASES = [
    (REG, (4, 2, 1)), (REG, (4, 5, 1)), (REG, (4, 100, 1)),
    (REG, (5, 3, 1)), (REG, (5, 10, 1)), (REG, (5, 256, 1)),
    (REG, (32, 1, 1)), (REG, (32, 64, 1)), (REG, (32, 300, 1)),
    (REG, (4, 440, 1)), (REG, (4, 260, 1)), (REG, (4, 230, 1)), (REG, (4, 200, 1)), (REG, (4, 180, 1)), (REG, (4, 135, 1)),
    (REG, (4, 120, 1)),                                                                  # NV = 5, 8, 9, 10, 11, 14, 15
    (CLS, (4, 3, 3)), (CLS, (4, 12, 3)), (CLS, (4, 200, 3)),
    (CLS, (34, 2, 2)), (CLS, (34, 50, 2)), (CLS, (34, 512, 2)),
    (CLS, (9, 3, 2)), (CLS, (9, 12, 2)), (CLS, (9, 96, 2)),
    (CLS, (11, 2, 10)), (CLS, (11, 50, 10)), (CLS, (11, 100, 10)),
    (CLS, (20, 3, 2)), (CLS, (20, 50, 2)), (CLS, (20, 160, 2)),
    (CLS, (16, 1, 10)), (CLS, (16, 30, 10)), (CLS, (16, 130, 10)),
    (CLS, (6, 3, 18)), (CLS, (6, 25, 18)), (CLS, (6, 200, 18)),
]


def test_cases_reach_every_shape_and_vector_group_size():
    import re
    import os
    hpp = open(os.path.join(os.path.dirname(__file__), "..", "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", hpp, re.M).group(1)
    shapes = {tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)}
    assert {(t, topo[0], topo[2]) for t, topo in CASES} == shapes
    # the smallest plan: the largest vector with the largest tile (34-512-2) still takes one vector; the reachable NV are 1 .. 16
    assert {_nv(topo) for _, topo in CASES} == set(range(1, SENS_MAX_NV + 1))


@pytest.mark.parametrize("task,topo", CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}" for t, (i, h, o) in CASES])
def test_gradients_at_every_compiled_shape(task, topo, tmp_path, monkeypatch):
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
    first = np.flatnonzero(mult)                                      # the distinct vectors that are selected ...
    at = np.cumsum(mult)[first] - mult[first]                         # ... and where each starts in the expanded order
    X = train[:, :I]
    full = pt.input_sensitivity("train", percentiles=PCTS, weights=W, return_samples=True)
    assert full.samples.shape == (int(mult.sum()), X.shape[0], O, I) and full.n_distinct == first.size
    worst = _worst_ratio(full.samples[at], X, Wd[first], topo, task)
    print(f"sensitivity {'cls' if task else 'reg'}-{I}-{H}-{O}: NV = {NV}, worst err / (u T) = {worst:.4f}")
    assert np.array_equal(full.samples, np.repeat(full.samples[at], mult[first], axis=0))
    _check_reductions(pt, X, W, full.samples, full)
    if task == CLS:                                                    # the class probabilities sum to 1: their gradients to 0
        for k, d in enumerate(first):
            T = ref.error_bound(X, Wd[d].astype(np.float64), topo, task)
            assert np.all(np.abs(full.samples[at[k]].astype(np.float64).sum(axis=1)) <= K * U32 * T.sum(axis=1) + 1e-30)
    for n in (1, 65):                                                 # caller rows at the 64-row tile edges
        part = pt.input_sensitivity(X[:n], percentiles=PCTS, weights=W, return_samples=True)
        assert np.array_equal(part.samples, full.samples[:, :n])
        _check_reductions(pt, X[:n].astype(np.float32), W, part.samples, part)
    # (distinct, multiplicity) with zero multiplicities: bit-identical to the expanded vectors (the two means of doubles: to rounding)
    alt = pt.input_sensitivity("train", percentiles=PCTS, weights=(Wd, mult), return_samples=True)
    assert alt.n_distinct == U
    _same(alt, full, same_distinct=False)
    # blocks of 65 rows (tiles straddle the block starts), then one row per block: bit-identical to one block
    for rows_blk in (65, 1):
        monkeypatch.setenv("PTNN_SENSITIVITY_SCRATCH_BYTES", str(full.n_distinct * 4 * O * I * rows_blk))
        _same(pt.input_sensitivity("train", percentiles=PCTS, weights=W, return_samples=True), full)
    monkeypatch.delenv("PTNN_SENSITIVITY_SCRATCH_BYTES")


# ---- the outputs depend on the multiset of samples only
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def test_depends_on_the_multiset_only(sunspot, monkeypatch):
    pt, res, d = sunspot
    topo = (4, 5, 1)
    base = pt.input_sensitivity("test", percentiles=PCTS, return_samples=True)
    M = 8 * 300
    n_rows = d["sunspot_test"].shape[0]
    assert base.n_samples == M and base.samples.shape == (M, n_rows, 1, 4)
    assert base.n_distinct < base.n_samples
    distinct, counts = _runs(res[0], 8)
    assert base.n_distinct == len(counts)
    at = np.cumsum(counts) - counts
    X = d["sunspot_test"][:, :4]
    worst = _worst_ratio(base.samples[at], X, distinct, topo, REG)
    print(f"sensitivity sunspot trace: worst err / (u T) = {worst:.4f}")
    _check_reductions(pt, "test", res[0].T, base.samples, base)
    for w in (res[0].T, (distinct, counts)):
        alt = pt.input_sensitivity("test", percentiles=PCTS, weights=w, return_samples=True)
        assert alt.n_distinct == base.n_distinct
        _same(alt, base)
    for rows_blk in (1, 7, n_rows):                                    # one, a few and all rows fit a block
        monkeypatch.setenv("PTNN_SENSITIVITY_SCRATCH_BYTES", str(base.n_distinct * 4 * 4 * rows_blk))
        _same(pt.input_sensitivity("test", percentiles=PCTS, return_samples=True), base)
    monkeypatch.delenv("PTNN_SENSITIVITY_SCRATCH_BYTES")
    # a selection: the cold chain, thinned
    cold = int(np.argmin(pt.temperatures))
    tr = pt._sampler.traces()["pos_w"]
    sel = pt.input_sensitivity("test", percentiles=PCTS, chains="cold", thin=3, return_samples=True)
    _same(pt.input_sensitivity("test", percentiles=PCTS, weights=tr[cold, 300::3], return_samples=True), sel)


def test_rows_past_one_grid_column(tmp_path, monkeypatch):
    topo = (4, 5, 1)
    d = parity.datasets()
    pt = _pt(REG, topo, d["sunspot_train"], d["sunspot_test"], 4, 20, tmp_path)
    n = 65535 * WAVE + 65
    rng = np.random.default_rng(65535)
    X = rng.standard_normal((n, 4)).astype(np.float32)
    w = _vectors(topo, 1, 3)
    sens = pt.input_sensitivity(X, percentiles=(5, 95), weights=w)
    assert sens.n_samples == 1 and sens.grad_mean.shape == (n, 1, 4)
    g = ref.jacobian(X, w[0].astype(np.float64), topo, REG)
    T = ref.error_bound(X, w[0].astype(np.float64), topo, REG)
    ok = np.abs(sens.grad_mean - g) <= K * U32 * T + 1e-30
    assert np.all(ok[65535 * WAVE:]), "rows past the first 65535 tiles"
    assert np.all(ok)
    for q in (5, 95):
        assert np.array_equal(sens.percentiles[q], sens.grad_mean), q
    assert np.array_equal(sens.prob_positive, (sens.grad_mean > 0).astype(np.float64))
    np.testing.assert_allclose(sens.importance, np.abs(sens.grad_mean).mean(axis=0), rtol=1e-12, atol=0)
    # blocks of 2^21 rows instead of the default ones: bit-identical
    monkeypatch.setenv("PTNN_SENSITIVITY_SCRATCH_BYTES", str(4 * 4 << 21))
    _same(pt.input_sensitivity(X, percentiles=(5, 95), weights=w), sens, samples=False)


# ---- known answers
@pytest.mark.parametrize("task,topo", [(REG, (5, 10, 1)), (CLS, (11, 50, 10)), (CLS, (34, 50, 2))], ids=["reg-5", "wine", "ionosphere"])
def test_an_unused_input_has_no_sensitivity(task, topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(task, topo, tmp_path, 77 + I)
    W = _vectors(topo, 9, 21 + I)
    i0 = I - 2
    W[:, i0 * H:(i0 + 1) * H] = 0.0                                    # W1[i0, :] = 0: the nets do not read input i0
    sens = pt.input_sensitivity("train", weights=W, return_samples=True)
    assert np.all(sens.samples[..., i0] == 0)
    assert np.all(sens.grad_mean[..., i0] == 0) and np.all(sens.importance[:, i0] == 0) and np.all(sens.importance_rms[:, i0] == 0)
    assert np.all(sens.prob_positive[..., i0] == 0) and np.all(sens.prob_negative[..., i0] == 0)
    assert np.all(sens.top_prob[:, i0] == 0)
    for q in sens.percentiles:
        assert np.all(sens.percentiles[q][..., i0] == 0) and np.all(sens.importance_percentiles[q][:, i0] == 0)
    other = np.delete(np.arange(I), i0)
    assert np.all(sens.importance[:, other] > 0)
    np.testing.assert_allclose(sens.top_prob.sum(axis=1), 1.0, rtol=1e-12)


@pytest.mark.parametrize("task,topo", [(REG, (4, 5, 1)), (CLS, (6, 25, 18))], ids=["reg", "chess"])
def test_one_sample_a_million_times(task, topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(task, topo, tmp_path, 31 + O)
    X = train[:65, :I]
    w = _vectors(topo, 1, 5)
    one = pt.input_sensitivity(X, percentiles=PCTS, weights=w, return_samples=True)           # M = 1
    assert one.n_samples == 1 and one.n_distinct == 1
    g = one.samples[0].astype(np.float64)
    big = pt.input_sensitivity(X, percentiles=PCTS, weights=(w, [10 ** 6]))
    assert big.n_samples == 10 ** 6 and big.n_distinct == 1
    for s in (one, big):
        assert np.array_equal(s.grad_mean, g)
        for q in PCTS:
            assert np.array_equal(s.percentiles[q], g), q
            assert np.array_equal(s.importance_percentiles[q], s.importance_percentiles[PCTS[0]]), q
        assert np.array_equal(s.prob_positive, (g > 0).astype(np.float64))
        assert np.array_equal(s.prob_negative, (g < 0).astype(np.float64))
        assert np.array_equal(s.top_prob, (np.arange(I)[None, :] == np.argmax(one.importance_percentiles[50], axis=1)[:, None]))
    np.testing.assert_allclose(big.importance, one.importance, rtol=1e-12, atol=0)
    raw = pt._sampler.sensitivity(X, w=w, multiplicity=[10 ** 6], ranks=[0, 499999, 999999])
    for k in range(3):
        assert np.array_equal(raw["order_stats"][k], one.samples[0])


# ---- refusals that need a handle
def test_refusals(tmp_path):
    from ptnn_amd import _lib
    topo = (6, 25, 18)
    pt, train, _ = _make(CLS, topo, tmp_path, 3)
    X = train[:5, :6]
    W = _vectors(topo, 3, 1)
    with pytest.raises(_lib.PtnnError, match="holds no sample"):
        pt._sampler.sensitivity(X, w=W, multiplicity=[0, 0, 0])
    with pytest.raises(_lib.PtnnError, match=r"rank 3 outside \[0, 3\)"):
        pt._sampler.sensitivity(X, w=W, ranks=[0, 3])
    with pytest.raises(_lib.PtnnError, match=r"rank 7 outside \[0, 3\)"):
        pt._sampler.sensitivity(X, w=W, ranks2=[7])
    with pytest.raises(_lib.PtnnError, match="n_ranks"):
        pt._sampler.sensitivity(X, w=W, ranks2=list(range(17)))
    many = (2 ** 31 - 1) // (6 * 18) + 1                               # x 108 columns per row: one column too many
    with pytest.raises(_lib.PtnnError, match="at most 2\\^31 - 1"):
        pt._sampler.sensitivity(np.zeros((many, 6), np.float32), w=W)
    with pytest.raises(ValueError, match="percentiles"):
        pt.input_sensitivity(X, weights=W, percentiles=(101,))
    ok = pt.input_sensitivity(X, weights=W)                            # the handle is still usable
    assert ok.n_samples == 3 and ok.grad_mean.shape == (5, 18, 6) and ok.samples is None


# ---- untouched neighbours
def test_leaves_the_chains_and_other_calls_alone(sunspot):
    pt, _, _ = sunspot
    sm = pt._sampler
    before = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
    steps = sm.lib.ptnn_steps_done(sm.h)
    state = sm.state()
    pt.input_sensitivity("test", percentiles=PCTS)
    pt.input_sensitivity("train", chains="cold", thin=2, return_samples=True)
    after = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
    assert np.array_equal(before.mean, after.mean) and np.array_equal(before.samples, after.samples)
    for q in PCTS:
        assert np.array_equal(before.percentiles[q], after.percentiles[q]), q
    assert sm.lib.ptnn_steps_done(sm.h) == steps
    state2 = sm.state()
    assert state.keys() == state2.keys()
    for k in state:
        assert np.array_equal(state[k], state2[k]), k
