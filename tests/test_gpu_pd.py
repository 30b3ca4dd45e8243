"""Partial dependence and ICE curves (ptnn_partial_dependence, pt.partial_dependence) on the GPU: the per-shape
pd_forward_kernel<TASK, I, O> against the float64 reference at every compiled shape under a derived forward-error bound; the
reductions exact on the device's own ICE values; the multiset of samples as the only thing the outputs depend on; known answers;
refusals; untouched neighbours.

The error bound of an ICE value: |f_dev - f_ref| <= K u T + 1e-30 with u = 2^-24, T = pd_ref.error_bound (first order, from the
oracle's float64 intermediates at the substituted row) and K = 1, the convention of tests/test_gpu_sensitivity.py.  Every shape
prints its worst err / (u T)."""
import os
import re

import numpy as np
import pytest

import parity
import pd_ref as ref
from parity import orc
from test_gpu_analysis_shapes import _make, _vectors
from test_gpu_predict import PCTS, _pt, _runs

pytestmark = pytest.mark.gpu

WAVE = 64
PD_MAX_NV, PD_ACC, PD_MAX_GT = 16, 40, 16
K = 1.0
U32 = ref.U32
REG, CLS = orc.TASK_REG, orc.TASK_CLS


def _gt(O):
    """Grid values per pass over the hidden units (pd_grid_tile)."""
    return max(1, min(PD_MAX_GT, PD_ACC // O))


def _plan(topo, G):
    """(vectors per forward work-group, grid values per chunk) as ptnn_partial_dependence picks them (PdPlan): 64 KiB of LDS over
    (staged vector + its 64-row tile of the chunk + the pad); a longer chunk where fewer than four (vector, tile) pairs are left."""
    I, H, O = topo
    GT = _gt(O)
    tiles = -(-G // GT)
    PV = (orc.num_param(topo) + 3) // 4 * 4
    per_vec = lambda t: PV + (min(t * GT, G) * O + 1) * WAVE     # noqa: E731
    ct = min(tiles, max(1, PD_ACC // (O * GT)))
    NV = max(1, min(PD_MAX_NV, 16384 // per_vec(ct)))
    while NV * ct < 4 and ct < tiles and NV * per_vec(ct + 1) * 4 <= 152 * 1024:
        ct += 1
    return NV, min(ct * GT, G)


def _grid(X32, inputs, G):
    """[A, G] float32, unsorted: a row's own x_j first, one value below and one above the column's range, the rest inside."""
    rows = []
    for a, j in enumerate(inputs):
        lo, hi = float(X32[:, j].min()), float(X32[:, j].max())
        vals = [float(X32[3 + a, j]), lo - 1.5, hi + 2.0] + list(np.linspace(hi, lo, max(G - 3, 0)))
        rows.append(vals[:G])
    return np.array(rows, np.float32)


def _worst_ratio(dev, X32, Wd, topo, task, inputs, grid):
    """dev [U, n_rows, A, G, O] fp32 ICE of the distinct vectors Wd -> max err / (u T); asserts the bound element by element."""
    worst = 0.0
    g64 = grid.astype(np.float64)
    for k in range(Wd.shape[0]):
        w = Wd[k].astype(np.float64)
        err = np.abs(dev[k].astype(np.float64) - ref.ice_all(X32, w, topo, task, inputs, g64))
        T = ref.error_bound_all(X32, w, topo, task, inputs, g64)
        ratio = float(np.max(err / (U32 * T + 1e-300)))
        worst = max(worst, ratio)
        assert np.all(err <= K * U32 * T + 1e-30), (k, ratio)
    return worst


def _top(sample_range):
    """[M, A, O] -> [A, O]: the share of the samples in which input a has the largest range of output o (first index on a tie)."""
    M, A, O = sample_range.shape
    best = np.argmax(sample_range, axis=1)                             # [M, O]
    return np.stack([(best == a).sum(axis=0) for a in range(A)]) / np.float64(M)


def _check_reductions(pt, X, weights, inputs, grid, pd):
    """Every reduced output against numpy float64 on the device's own fp32 ICE values pd.samples [M, n_rows, A, G, O]."""
    s = pd.samples
    M = s.shape[0]
    s64 = s.astype(np.float64)
    assert pd.n_samples == M
    np.testing.assert_allclose(pd.ice_mean, s64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(pd.ice_percentiles[q], np.percentile(s64, q, axis=0)), q
    rm = ref.row_means(s)
    assert np.array_equal(pd.sample_pd, rm.astype(np.float32))
    np.testing.assert_allclose(pd.pd_mean, rm.mean(axis=0), rtol=1e-12, atol=0)
    p64 = pd.sample_pd.astype(np.float64)
    for q in PCTS:
        assert np.array_equal(pd.pd_percentiles[q], np.percentile(p64, q, axis=0)), q
    w, mult = weights if isinstance(weights, tuple) else (weights, None)
    src = dict(w=w, multiplicity=mult) if w is not None else {}
    raw = pt._sampler.partial_dependence(X, inputs=inputs, grid=grid, sample_range=True, **src, **pd_trace_kw(pt, w))
    sr = raw["sample_range"]
    assert np.array_equal(sr, ref.ranges(pd.sample_pd))
    assert raw["ice_mean"] is None and raw["samples"] is None and np.array_equal(raw["pd_mean"], pd.pd_mean)
    r64 = sr.astype(np.float64)
    np.testing.assert_allclose(pd.effect_range, r64.mean(axis=0), rtol=1e-12, atol=0)
    assert np.array_equal(raw["range_mean"], pd.effect_range)
    for q in PCTS:
        assert np.array_equal(pd.effect_range_percentiles[q], np.percentile(r64, q, axis=0)), q
    assert np.array_equal(pd.top_prob, _top(sr))


def pd_trace_kw(pt, w):
    """The trace selection of the object's default call, for the raw sampler call beside a trace-sourced one."""
    if w is not None:
        return {}
    S = pt.NumSamples
    return dict(step0=int(S * pt.burn_in), nsteps=S - int(S * pt.burn_in))


def _same(a, b, samples=True, same_distinct=True):
    """Bitwise equal.  pd_mean is a weighted mean of doubles with a fixed summation order for a given list of distinct vectors;
    when the lists differ (zero-multiplicity vectors in one of them) it is compared to rounding."""
    assert a.n_samples == b.n_samples
    assert np.array_equal(a.inputs, b.inputs) and np.array_equal(a.grid, b.grid)
    if same_distinct:
        assert np.array_equal(a.pd_mean, b.pd_mean)
    else:
        np.testing.assert_allclose(a.pd_mean, b.pd_mean, rtol=1e-14, atol=0)
    for f in ("effect_range", "top_prob", "sample_pd"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for q in a.pd_percentiles:
        assert np.array_equal(a.pd_percentiles[q], b.pd_percentiles[q]), q
        assert np.array_equal(a.effect_range_percentiles[q], b.effect_range_percentiles[q]), q
    if a.ice_mean is not None and b.ice_mean is not None:
        assert np.array_equal(a.ice_mean, b.ice_mean)
        for q in a.ice_percentiles:
            assert np.array_equal(a.ice_percentiles[q], b.ice_percentiles[q]), q
    if samples:
        assert np.array_equal(a.samples, b.samples)


# (task, topology, n_grid): every (task, I, O) of PTNN_SHAPES at an H < 4 and at a wide H in (64, 512], n_grid one past a tile of
# GT = 16, 16, 13, 4, 2 grid values (n_out = 1, 2, 3, 10, 18); per task one case with one grid value and one with 64; and the
# 4-H-1 sizes that give the vector-group sizes NV no other case reaches (NV = 15 and 16 need the one-value grid's small tile)
CASES = [
    (REG, (4, 2, 1), 17), (REG, (4, 100, 1), 17), (REG, (5, 3, 1), 17), (REG, (5, 256, 1), 17), (REG, (32, 1, 1), 17), (REG, (32, 300, 1), 17),
    (REG, (4, 5, 1), 1), (REG, (4, 150, 1), 1), (REG, (4, 5, 1), 64),                                                # NV = 16, 15, 7
    (REG, (4, 17, 1), 17), (REG, (4, 30, 1), 17), (REG, (4, 50, 1), 17), (REG, (4, 70, 1), 17), (REG, (4, 140, 1), 17),
    (REG, (4, 230, 1), 17), (REG, (4, 300, 1), 17), (REG, (4, 400, 1), 17), (REG, (4, 512, 1), 17),          # NV = 13 .. 10, 8, 6 .. 3
    (CLS, (4, 3, 3), 14), (CLS, (4, 200, 3), 14), (CLS, (34, 2, 2), 17), (CLS, (34, 512, 2), 17), (CLS, (9, 3, 2), 17), (CLS, (9, 96, 2), 17),
    (CLS, (11, 2, 10), 5), (CLS, (11, 100, 10), 5), (CLS, (20, 3, 2), 17), (CLS, (20, 160, 2), 17), (CLS, (16, 1, 10), 5),
    (CLS, (16, 130, 10), 5), (CLS, (6, 3, 18), 3), (CLS, (6, 200, 18), 3),
    (CLS, (4, 12, 3), 1), (CLS, (6, 25, 18), 64), (CLS, (34, 512, 2), 64),
]


def test_cases_reach_every_shape_and_plan():
    hpp = open(os.path.join(os.path.dirname(__file__), "..", "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", hpp, re.M).group(1)
    shapes = {tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)}
    assert {(t, topo[0], topo[2]) for t, topo, _ in CASES} == shapes
    for shape in shapes:                                                # a small and a wide H, one value past a tile
        mine = [(topo[1], G) for t, topo, G in CASES if (t, topo[0], topo[2]) == shape and G == _gt(shape[2]) + 1]
        assert any(H < 4 for H, _ in mine) and any(64 < H <= 512 for H, _ in mine), shape
    for task in (REG, CLS):
        assert {1, 64} <= {G for t, _, G in CASES if t == task}
    # every vector-group size, and chunks that are the whole grid, a cut of it, and grown past the first plan (34-512-2, 64 values)
    assert {_plan(topo, G)[0] for _, topo, G in CASES} == set(range(1, PD_MAX_NV + 1))
    assert _plan((34, 512, 2), 64) == (1, 64) and _plan((6, 25, 18), 64) == (5, 2) and _plan((4, 5, 1), 64) == (7, 32)
    # the largest request of a compiled shape stays under the LDS ceiling
    for t, I, O in shapes:
        NV, GC = _plan((I, 512, O), 64)
        PV = (orc.num_param((I, 512, O)) + 3) // 4 * 4
        assert NV * (PV + GC * O * WAVE + max(1, WAVE // NV)) * 4 <= 152 * 1024, (I, O)


@pytest.mark.parametrize("task,topo,G", CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}-g{g}" for t, (i, h, o), g in CASES])
def test_ice_at_every_compiled_shape(task, topo, G, tmp_path):
    I, H, O = topo
    seed = I * 1000 + H * 10 + O + G
    pt, train, _ = _make(task, topo, tmp_path, seed)
    NV, GC = _plan(topo, G)
    U = NV + 1
    Wd = _vectors(topo, U, seed + 1)
    rng = np.random.default_rng(seed + 2)
    mult = rng.integers(1, 4, U).astype(np.int32)
    mult[1] = 0
    first = np.flatnonzero(mult)                                      # the distinct vectors that are selected ...
    at = np.cumsum(mult)[first] - mult[first]                         # ... and where each starts in the expanded order
    X32 = train[:65, :I].astype(np.float32)                           # one full wave of rows plus one lane
    inputs = [I - 1, 0]
    grid = _grid(X32, inputs, G)
    assert grid.shape == (2, G) and grid[0, 0] == X32[3, I - 1]
    pd = pt.partial_dependence(X32, inputs=inputs, grid=grid, percentiles=PCTS, ice=True, weights=(Wd, mult), return_samples=True)
    M = int(mult.sum())
    assert pd.samples.shape == (M, 65, 2, G, O) and pd.n_distinct == U and pd.n_samples == M
    assert np.array_equal(pd.inputs, inputs) and np.array_equal(pd.grid, grid.astype(np.float64))
    worst = _worst_ratio(pd.samples[at], X32.astype(np.float64), Wd[first], topo, task, inputs, grid)
    print(f"partial dependence {'cls' if task else 'reg'}-{I}-{H}-{O}, {G} grid values: NV = {NV}, chunk = {GC}, worst err / (u T) = {worst:.4f}")
    assert np.array_equal(pd.samples, np.repeat(pd.samples[at], mult[first], axis=0))
    if task == CLS:
        assert np.max(np.abs(pd.samples.astype(np.float64).sum(axis=4) - 1.0)) <= 1e-6
    _check_reductions(pt, X32, (Wd, mult), inputs, grid, pd)
    # without ICE outputs and samples the column reduction is not launched: the curve's outputs are the same bits
    lean = pt.partial_dependence(X32, inputs=inputs, grid=grid, percentiles=PCTS, weights=(Wd, mult))
    assert lean.ice_mean is None and lean.ice_percentiles == {} and lean.samples is None
    _same(lean, pd, samples=False)


# ---- the outputs depend on the multiset of samples only
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def test_depends_on_the_multiset_only(sunspot, monkeypatch):
    pt, res, d = sunspot
    topo = (4, 5, 1)
    X = d["sunspot_test"][:40, :4]
    kw = dict(inputs=[2, 0, 3], grid=5, percentiles=PCTS, ice=True, return_samples=True)
    base = pt.partial_dependence(X, **kw)
    M = 4 * 100
    assert base.n_samples == M and base.samples.shape == (M, 40, 3, 5, 1) and base.n_distinct < M
    distinct, counts = _runs(res[0], 4)
    assert base.n_distinct == len(counts)
    at = np.cumsum(counts) - counts
    X32 = X.astype(np.float32)
    grid = base.grid.astype(np.float32)
    for a, j in enumerate((2, 0, 3)):                                   # the integer grid: percentiles of the rows' columns
        assert np.array_equal(grid[a], np.percentile(X32[:, j].astype(np.float64), np.linspace(5, 95, 5)).astype(np.float32))
    worst = _worst_ratio(base.samples[at], X32.astype(np.float64), distinct, topo, REG, [2, 0, 3], grid)
    print(f"partial dependence sunspot trace: worst err / (u T) = {worst:.4f}")
    _check_reductions(pt, X32, None, [2, 0, 3], grid, base)
    for w in (res[0].T, (distinct, counts)):
        alt = pt.partial_dependence(X, weights=w, **kw)
        assert alt.n_distinct == base.n_distinct
        _same(alt, base)
    for rows_blk in (1, 7):                                             # one row and a few rows per block
        monkeypatch.setenv("PTNN_PD_SCRATCH_BYTES", str(base.n_distinct * 4 * 3 * 5 * rows_blk))
        _same(pt.partial_dependence(X, **kw), base)
    monkeypatch.delenv("PTNN_PD_SCRATCH_BYTES")
    # a permuted input list gives the permuted result, a reordered grid row the reordered curve
    perm = pt.partial_dependence(X, **dict(kw, inputs=[3, 2, 0], grid=grid[[2, 0, 1]]))
    order = [2, 0, 1]
    assert np.array_equal(perm.samples, base.samples[:, :, order]) and np.array_equal(perm.pd_mean, base.pd_mean[order])
    assert np.array_equal(perm.effect_range, base.effect_range[order]) and np.array_equal(perm.top_prob, base.top_prob[order])
    for q in PCTS:
        assert np.array_equal(perm.pd_percentiles[q], base.pd_percentiles[q][order]), q
    g2 = grid.copy()
    g2[1] = grid[1, [4, 0, 3, 1, 2]]
    re_ = pt.partial_dependence(X, **dict(kw, grid=g2))
    assert np.array_equal(re_.samples[:, :, 1], base.samples[:, :, 1][:, :, [4, 0, 3, 1, 2]])
    assert np.array_equal(re_.samples[:, :, [0, 2]], base.samples[:, :, [0, 2]])
    assert np.array_equal(re_.pd_mean[1], base.pd_mean[1, [4, 0, 3, 1, 2]]) and np.array_equal(re_.effect_range, base.effect_range)
    # "test" and the same rows from the host; the cold chain, thinned, against its trace rows as weights
    assert np.array_equal(pt.partial_dependence("test", inputs=[1], grid=[0.25, 0.5]).pd_mean,
                          pt.partial_dependence(d["sunspot_test"], inputs=[1], grid=[0.25, 0.5]).pd_mean)
    cold = int(np.argmin(pt.temperatures))
    tr = pt._sampler.traces()["pos_w"]
    _same(pt.partial_dependence(X, weights=tr[cold, 100::3], **kw), pt.partial_dependence(X, chains="cold", thin=3, **kw))


# ---- known answers
@pytest.mark.parametrize("task,topo", [(REG, (5, 10, 1)), (CLS, (11, 50, 10)), (CLS, (34, 50, 2))], ids=["reg-5", "wine", "ionosphere"])
def test_an_unused_input_has_a_flat_curve(task, topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(task, topo, tmp_path, 77 + I)
    W = _vectors(topo, 9, 21 + I)
    j = I - 2
    W[:, j * H:(j + 1) * H] = 0.0                                      # W1[j, :] = 0: the nets do not read input j
    pd = pt.partial_dependence(train[:70], inputs=[0, j], grid=7, grid_range=(0, 100), weights=W, ice=True, return_samples=True)
    s = pd.samples
    assert np.all(s[:, :, 1] == s[:, :, 1, :1])                        # bit-identical across the grid
    assert np.all(pd.effect_range[1] == 0) and np.all(pd.top_prob[1] == 0) and np.all(pd.top_prob[0] == 1)
    assert np.all(pd.sample_pd[:, 1] == pd.sample_pd[:, 1, :1]) and np.all(pd.pd_mean[1] == pd.pd_mean[1, :1])
    for q in pd.pd_percentiles:
        assert np.all(pd.effect_range_percentiles[q][1] == 0) and np.all(pd.ice_percentiles[q][:, 1] == pd.ice_percentiles[q][:, 1, :1])
    assert np.all(pd.effect_range[0] > 0)
    # and the flat curve is the net's own output on the rows: the substituted value never enters
    own = pt.posterior_predictive(train[:70], weights=W, return_samples=True).samples
    T = np.stack([ref.error_bound(train[:70, :I].astype(np.float32).astype(np.float64), w.astype(np.float64), topo, task, j, 0.0) for w in W])
    assert np.all(np.abs(s[:, :, 1, 0].astype(np.float64) - own) <= 2 * K * U32 * T + 1e-30)


def test_one_hidden_unit_is_monotone(tmp_path):
    topo = (4, 1, 1)
    pt, train, _ = _make(REG, topo, tmp_path, 41)
    rng = np.random.default_rng(9)
    W = rng.standard_normal((12, 7)).astype(np.float32)                # W1 [4, 1], W2 [1, 1], B1, B2
    W[:, 2] = np.abs(W[:, 2]) + 0.1                                    # W1[2] > 0
    W[:, 4] = np.abs(W[:, 4]) + 0.1                                    # W2 > 0
    grid = np.sort(rng.uniform(-3, 3, 33)).astype(np.float32)
    pd = pt.partial_dependence("train", inputs=[2], grid=grid, weights=W, ice=True, return_samples=True)
    assert np.all(np.diff(pd.samples, axis=3) >= 0) and np.all(np.diff(pd.pd_mean[0, :, 0]) >= 0)
    assert np.all(np.diff(pd.sample_pd, axis=2) >= 0) and np.all(np.diff(pd.ice_mean, axis=2) >= 0)
    first_last = (pd.sample_pd[:, 0, -1, 0].astype(np.float64) - pd.sample_pd[:, 0, 0, 0].astype(np.float64)).astype(np.float32)
    np.testing.assert_allclose(pd.effect_range[0, 0], first_last.astype(np.float64).mean(), rtol=1e-12, atol=0)   # max - min = last - first
    assert pd.effect_range[0, 0] > 0 and pd.top_prob.tolist() == [[1.0]]


@pytest.mark.parametrize("task,topo", [(REG, (4, 5, 1)), (CLS, (16, 30, 10))], ids=["reg", "pendigit"])
def test_ice_is_the_prediction_on_substituted_rows(task, topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(task, topo, tmp_path, 13 + O)
    W = _vectors(topo, 6, 3 + O)
    X32 = train[:66, :I].astype(np.float32)
    rng = np.random.default_rng(5)
    inputs = list(range(I))
    grid = rng.uniform(-2.5, 2.5, (I, 6)).astype(np.float32)
    pd = pt.partial_dependence(X32, inputs=inputs, grid=grid, weights=W, return_samples=True)
    triples = [(int(rng.integers(66)), int(rng.integers(I)), int(rng.integers(6))) for _ in range(20)]
    sub = np.stack([np.where(np.arange(I) == j, grid[j, k], X32[n]) for n, j, k in triples]).astype(np.float32)
    pred = pt.posterior_predictive(sub, weights=W, return_samples=True).samples          # [6, 20, O]
    for t, (n, j, k) in enumerate(triples):
        for u in range(6):
            w = W[u].astype(np.float64)
            T = (ref.error_bound(X32[n:n + 1].astype(np.float64), w, topo, task, j, float(grid[j, k]))
                 + ref.error_bound(sub[t:t + 1].astype(np.float64), w, topo, task, j, float(grid[j, k])))[0]
            assert np.all(np.abs(pd.samples[u, n, j, k].astype(np.float64) - pred[u, t].astype(np.float64)) <= K * U32 * T + 1e-30), (n, j, k, u)


# ---- refusals that need a handle
def test_refusals(tmp_path):
    from ptnn_amd import _lib
    topo = (6, 25, 18)
    pt, train, _ = _make(CLS, topo, tmp_path, 3)
    X = train[:5, :6]
    W = _vectors(topo, 3, 1)
    g1 = np.zeros((1, 2), np.float32)
    sm = pt._sampler
    with pytest.raises(_lib.PtnnError, match=r"inputs\[0\] = 6 outside \[0, 6\)"):
        sm.partial_dependence(X, w=W, inputs=[6], grid=g1)
    with pytest.raises(_lib.PtnnError, match=r"inputs\[1\] = -1 outside \[0, 6\)"):
        sm.partial_dependence(X, w=W, inputs=[0, -1], grid=np.zeros((2, 2), np.float32))
    with pytest.raises(_lib.PtnnError, match=r"inputs\[2\] = 4 is given twice"):
        sm.partial_dependence(X, w=W, inputs=[4, 1, 4], grid=np.zeros((3, 2), np.float32))
    with pytest.raises(_lib.PtnnError, match=r"grid\[5, 1\] = nan \(input slot 5, position 1\)"):
        sm.partial_dependence(X, w=W, grid=np.where(np.arange(12).reshape(6, 2) == 11, np.nan, 0.0).astype(np.float32))
    with pytest.raises(_lib.PtnnError, match="holds no sample"):
        sm.partial_dependence(X, w=W, multiplicity=[0, 0, 0], inputs=[0], grid=g1)
    with pytest.raises(_lib.PtnnError, match=r"rank 3 outside \[0, 3\)"):
        sm.partial_dependence(X, w=W, inputs=[0], grid=g1, ranks=[0, 3])
    with pytest.raises(_lib.PtnnError, match=r"rank 7 outside \[0, 3\)"):
        sm.partial_dependence(X, w=W, inputs=[0], grid=g1, ranks2=[7])
    with pytest.raises(_lib.PtnnError, match="n_ranks"):
        sm.partial_dependence(X, w=W, inputs=[0], grid=g1, ranks2=list(range(17)))
    many = (2 ** 31 - 1) // (6 * 64 * 18) + 1                          # x 6912 columns per row: past 2^31 - 1
    with pytest.raises(_lib.PtnnError, match="at most 2\\^31 - 1"):
        sm.partial_dependence(np.zeros((many, 6), np.float32), w=W, grid=np.zeros((6, 64), np.float32))
    with pytest.raises(ValueError, match="percentiles"):
        pt.partial_dependence(X, weights=W, percentiles=(101,))
    with pytest.raises(ValueError, match="given twice"):
        pt.partial_dependence(X, weights=W, inputs=[1, 1])
    ok = pt.partial_dependence(X, weights=W, grid=3)                   # the handle is still usable
    assert ok.n_samples == 3 and ok.pd_mean.shape == (6, 3, 18) and ok.effect_range.shape == (6, 18) and ok.samples is None
    np.testing.assert_allclose(ok.top_prob.sum(axis=0), 1.0, rtol=1e-12)


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
            pt.partial_dependence("test", weights=W, percentiles=PCTS)
            pt.partial_dependence("train", inputs=[1], grid=64, weights=(W, [2, 0, 1, 1, 3, 1, 1]), ice=True, return_samples=True)
        after = snap()
        assert before[3] == after[3] == 25
        for k in before[0]:
            assert np.array_equal(before[0][k], after[0][k]), k
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        res = pt.run_chains(max_steps=10 ** 6)                          # the continuation
        pred = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
        if between:
            pt.partial_dependence("test", percentiles=PCTS, ice=True)
            again = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
            assert np.array_equal(pred.mean, again.mean) and np.array_equal(pred.samples, again.samples)
        return res[0], sm.state(), sm.trace_rows(), pred.samples
    w0, s0, t0, p0 = run(False)
    w1, s1, t1, p1 = run(True)
    assert np.array_equal(w0, w1) and np.array_equal(t0, t1) and np.array_equal(p0, p1)
    for k in s0:
        assert np.array_equal(s0[k], s1[k]), k
