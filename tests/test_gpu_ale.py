"""Accumulated local effects (ptnn_accumulated_effects, pt.accumulated_effects) on the GPU: the per-shape
ale_forward_kernel<TASK, I, O> against the float64 reference at every compiled shape under a derived forward-error bound; every
reduced output bitwise equal to numpy float64 in the stated order on the device's own local effects; the multiset of samples as
the only thing the outputs depend on; known answers; refusals; untouched neighbours.

The error bound of a local effect: |d_dev - d_ref| <= K u T + 1e-30 with u = 2^-24, T = ale_ref.bound1 / bound2 (first order, from
the oracle's float64 intermediates at the substituted rows, plus |d_ref| for the one rounding of the difference) and K = 1, the
convention of tests/test_gpu_pd.py.  Every shape prints its worst err / (u T)."""
import os
import re

import numpy as np
import pytest

import ale_ref as ref
import parity
import pd_ref
from parity import orc
from test_gpu_analysis_shapes import _make, _vectors
from test_gpu_predict import PCTS, _pt, _runs

pytestmark = pytest.mark.gpu

WAVE = 64
ALE_MAX_NV, PD_ACC, ALE_MAX_ST = 16, 40, 10
K = 1.0
U32 = ref.U32
REG, CLS = orc.TASK_REG, orc.TASK_CLS


def _st(O):
    """Slots per pass over the hidden units (ale_slot_tile)."""
    return max(1, min(ALE_MAX_ST, PD_ACC // (2 * O)))


def _cs(O):
    """Slots per chunk (ale_chunk_slots): whole terms, an even number."""
    return 2 if _st(O) < 2 else _st(O) // 2 * 2


def _plan(topo):
    """(vectors per forward work-group, bytes of LDS) as ptnn_accumulated_effects picks them (AlePlan): 64 KiB of LDS less the
    chunk's slot table over (staged vector + its 64-row tile of the chunk + the pad)."""
    I, H, O = topo
    PV = (orc.num_param(topo) + 3) // 4 * 4
    tile, table = _cs(O) * 2 * O * WAVE, _cs(O) * (3 * WAVE + 2)
    NV = max(1, min(ALE_MAX_NV, (16384 - table) // (PV + tile + WAVE)))
    return NV, (NV * (PV + tile + max(1, WAVE // NV)) + table) * 4


# (task, topology): every (task, I, O) of PTNN_SHAPES at an H < 4 and at a wide H in (64, 512], and the 4-H-1 and 5-H-1 sizes that
# give the vector-group sizes no other case reaches
CASES = [
    (REG, (4, 2, 1)), (REG, (4, 100, 1)), (REG, (5, 3, 1)), (REG, (5, 512, 1)), (REG, (32, 1, 1)), (REG, (32, 300, 1)),
    (REG, (4, 30, 1)), (REG, (4, 70, 1)), (REG, (4, 150, 1)), (REG, (4, 230, 1)), (REG, (4, 300, 1)), (REG, (4, 512, 1)),
    (CLS, (4, 3, 3)), (CLS, (4, 200, 3)), (CLS, (34, 2, 2)), (CLS, (34, 512, 2)), (CLS, (9, 3, 2)), (CLS, (9, 96, 2)),
    (CLS, (11, 2, 10)), (CLS, (11, 100, 10)), (CLS, (20, 3, 2)), (CLS, (20, 160, 2)), (CLS, (16, 1, 10)), (CLS, (16, 130, 10)),
    (CLS, (6, 3, 18)), (CLS, (6, 200, 18)),
]


def test_cases_reach_every_shape_and_plan():
    hpp = open(os.path.join(os.path.dirname(__file__), "..", "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", hpp, re.M).group(1)
    shapes = {tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)}
    assert {(t, topo[0], topo[2]) for t, topo in CASES} == shapes
    for shape in shapes:
        mine = [topo[1] for t, topo in CASES if (t, topo[0], topo[2]) == shape]
        assert any(H < 4 for H in mine) and any(64 < H <= 512 for H in mine), shape
    # every vector-group size the plan can produce: the slot table and a 10 KiB tile leave room for at most 10 of the shortest vectors
    reach = {_plan((I, H, O))[0] for _, I, O in shapes for H in range(1, 513)}
    assert reach == set(range(1, 11)) == {_plan(topo)[0] for _, topo in CASES}
    assert [_st(O) for O in (1, 2, 3, 10, 18)] == [10, 10, 6, 2, 1] and [_cs(O) for O in (1, 2, 3, 10, 18)] == [10, 10, 6, 2, 2]
    # the largest request of a compiled shape stays under the LDS ceiling
    assert max(_plan((I, 512, O))[1] for _, I, O in shapes) == _plan((34, 512, 2))[1] == 94048 <= 152 * 1024


def _design(X32, I, O):
    """The terms of a case and its edited rows: A = min(n_in, slot tile + 1) inputs in descending order; the first with five
    distinct edges of which (z_1, z_2] holds no row, the others with four (one padded edge at E = 5); two pairs that share input 0,
    three edges per side; cell (2, 1) of the first pair emptied; row r on an edge of every selected input, rows below z_0 and
    above the last edge (the 10th and 90th percentiles are the outer edges).  -> (rows, r, inputs, edges, pairs, pair_edges)."""
    X = X32.copy()
    pairs = [(I - 1, 0), (0, 1)]
    pair_edges = [tuple(np.percentile(X32[:, j].astype(np.float64), [5, 50, 95]).astype(np.float32) for j in p) for p in pairs]
    u, v = pair_edges[0]
    r = int(np.flatnonzero(X[:, I - 1] <= u[1])[0])                    # stays in the first pair's row k = 1 whatever its x_0 becomes
    hit = (X[:, I - 1] > u[1]) & (X[:, 0] <= v[1])                      # cell (2, 1) of the first pair -> (2, 2), the last on its edge
    X[hit, 0] = (v[1] + (v[2] - v[1]) * np.linspace(0.5, 1.0, int(hit.sum()))).astype(np.float32)
    A = min(I, _st(O) + 1)
    inputs = list(range(A))[::-1]
    edges = []
    for a, j in enumerate(inputs):
        col = np.sort(X[:, j].astype(np.float64))
        z = list(np.percentile(col, [10, 40, 70, 90]))
        if a == 0:
            above = col[col > z[1]][0]
            z.insert(2, (z[1] + above) / 2)                             # between the 40th percentile and the next row above it
        edges.append(np.array(z).astype(np.float32))
        assert np.all(np.diff(edges[-1]) > 0)
        X[r, j] = edges[-1][1]                                          # a row on an edge: the lower bin
    return X, r, inputs, edges, pairs, pair_edges


def _padded(edges):
    E = max(e.size for e in edges)
    return np.stack([np.concatenate([e, np.full(E - e.size, e[-1], np.float32)]) for e in edges])


def _reference(X32, Wd, topo, task, inputs, e32, pairs, pe32):
    """(d_ref, T) [U, n_rows, A + Q, O] float64, and the bins [A][n] and cells [Q] -> (bk, bm) of the rows."""
    X = X32.astype(np.float64)
    d, T = [], []
    for w in Wd.astype(np.float64):
        dw = [ref.local1(X, w, topo, task, j, e32[a].astype(np.float64))[0] for a, j in enumerate(inputs)]
        Tw = [ref.bound1(X, w, topo, task, j, e32[a].astype(np.float64)) for a, j in enumerate(inputs)]
        for q, (j, l) in enumerate(pairs):
            u, v = pe32[q][0].astype(np.float64), pe32[q][1].astype(np.float64)
            dw.append(ref.local2(X, w, topo, task, j, l, u, v)[0])
            Tw.append(ref.bound2(X, w, topo, task, j, l, u, v))
        d.append(np.stack(dw, axis=1))
        T.append(np.stack(Tw, axis=1))
    b = [ref.bins(X[:, j], e32[a]) for a, j in enumerate(inputs)]
    cells = [(ref.bins(X[:, j], pe32[q][0]), ref.bins(X[:, l], pe32[q][1])) for q, (j, l) in enumerate(pairs)]
    return np.stack(d), np.stack(T), b, cells


def _top(sample_range):
    M, A, O = sample_range.shape
    best = np.argmax(sample_range, axis=1)
    return np.stack([(best == a).sum(axis=0) for a in range(A)]) / np.float64(M)


def _check_reductions(res, b, cells, K1, K2):
    """Every reduced output against numpy float64, in the stated order, on the device's own fp32 local effects res.samples
    [M, n_rows, A + Q, O]: bitwise, the weighted double means to rounding."""
    s = res.samples
    A, Q = len(b), len(cells)
    ale32 = np.stack([ref.curve(s[:, :, a], b[a], K1).astype(np.float32) for a in range(A)], axis=1)
    assert np.array_equal(res.sample_ale, ale32)
    assert np.array_equal(res.bin_count, np.stack([ref.counts(b[a], K1) for a in range(A)]))
    for a in range(A):                                                  # sum_k n_k ALE[k] = 0, to the rounding of the stored curve
        nk = res.bin_count[a].astype(np.float64)
        assert np.all(np.abs(np.einsum("k,mko->mo", nk, ale32[:, a, 1:].astype(np.float64))) <= len(b[a]) * (K1 + 2) * U32 * np.abs(ale32[:, a]).max() + 1e-30)
    rng = ref.ranges(ale32)
    a64, r64 = ale32.astype(np.float64), rng.astype(np.float64)
    np.testing.assert_allclose(res.ale_mean, a64.mean(axis=0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(res.effect_range, r64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(res.ale_percentiles[q], np.percentile(a64, q, axis=0)), q
        assert np.array_equal(res.effect_range_percentiles[q], np.percentile(r64, q, axis=0)), q
    assert np.array_equal(res.top_prob, _top(rng))
    ale2 = np.stack([ref.surface(s[:, :, A + q], cells[q][0], cells[q][1], K2).astype(np.float32) for q in range(Q)], axis=1)
    inter = np.stack([ref.interaction(ale2[:, q], cells[q][0], cells[q][1], K2) for q in range(Q)], axis=1)
    assert np.array_equal(res.sample_ale2, ale2) and np.array_equal(res.sample_interaction, inter)
    assert np.array_equal(res.cell_count, np.stack([ref.cell_counts(cells[q][0], cells[q][1], K2) for q in range(Q)]))
    s64, i64 = ale2.astype(np.float64), inter.astype(np.float64)
    np.testing.assert_allclose(res.ale2_mean, s64.mean(axis=0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(res.interaction, i64.mean(axis=0), rtol=1e-12, atol=0)
    for q in PCTS:
        assert np.array_equal(res.ale2_percentiles[q], np.percentile(s64, q, axis=0)), q
        assert np.array_equal(res.interaction_percentiles[q], np.percentile(i64, q, axis=0)), q
    l64 = s.astype(np.float64)
    np.testing.assert_allclose(res.local_mean, l64.mean(axis=0), rtol=1e-12, atol=1e-300)
    for q in PCTS:
        assert np.array_equal(res.local_percentiles[q], np.percentile(l64, q, axis=0)), q


CURVES = ("bin_count", "ale_mean", "effect_range", "top_prob", "sample_ale", "cell_count", "ale2_mean", "interaction", "sample_ale2",
          "sample_interaction")
BANDS = ("ale_percentiles", "effect_range_percentiles", "ale2_percentiles", "interaction_percentiles")


def _same(a, b, local=True):
    """Bitwise equal (the same list of distinct vectors on both sides)."""
    assert a.n_samples == b.n_samples
    for f in CURVES + (("local_mean", "samples") if local else ()):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in BANDS + (("local_percentiles",) if local else ()):
        for q in getattr(a, f):
            assert np.array_equal(getattr(a, f)[q], getattr(b, f)[q]), (f, q)


@pytest.mark.parametrize("task,topo", CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}" for t, (i, h, o) in CASES])
def test_local_effects_at_every_compiled_shape(task, topo, tmp_path):
    I, H, O = topo
    seed = I * 1000 + H * 10 + O
    pt, train, _ = _make(task, topo, tmp_path, seed)
    NV = _plan(topo)[0]
    U = NV + 1
    Wd = _vectors(topo, U, seed + 1)
    rng = np.random.default_rng(seed + 2)
    mult = rng.integers(1, 4, U).astype(np.int32)
    mult[1] = 0
    first = np.flatnonzero(mult)
    at = np.cumsum(mult)[first] - mult[first]
    X32, r, inputs, edges, pairs, pair_edges = _design(train[:65, :I].astype(np.float32), I, O)
    e32 = _padded(edges)
    assert e32.shape == (len(inputs), 5) and len(inputs) == min(I, _st(O) + 1) and sum(e.size == 4 for e in edges) == len(inputs) - 1
    kw = dict(inputs=inputs, edges=edges, pairs=pairs, pair_edges=pair_edges, percentiles=PCTS, weights=(Wd, mult))
    res = pt.accumulated_effects(X32, local=True, return_samples=True, **kw)
    M, T = int(mult.sum()), len(inputs) + 2
    assert res.samples.shape == (M, 65, T, O) and res.n_distinct == U and res.n_samples == M
    assert np.array_equal(res.inputs, inputs) and np.array_equal(res.pairs, pairs)
    assert all(np.array_equal(a, b.astype(np.float64)) for a, b in zip(res.edges, edges))
    d_ref, Tb, b, cells = _reference(X32, Wd[first], topo, task, inputs, e32, pairs, pair_edges)
    # the design: an empty bin and an empty cell, rows on, below and above the edges
    assert res.bin_count[0, 1] == 0 and res.cell_count[0, 1, 0] == 0 and np.all(res.bin_count[1:, 3] == 0)
    for a, j in enumerate(inputs):
        assert X32[r, j] == edges[a][1] and b[a][r] == 1 and np.any(X32[:, j] < edges[a][0]) and np.any(X32[:, j] > edges[a][-1])
    err = np.abs(res.samples[at].astype(np.float64) - d_ref)
    worst = [float(np.max(err[:, :, :T - 2] / (U32 * Tb[:, :, :T - 2] + 1e-300))), float(np.max(err[:, :, T - 2:] / (U32 * Tb[:, :, T - 2:] + 1e-300)))]
    print(f"accumulated effects {'cls' if task else 'reg'}-{I}-{H}-{O}: NV = {NV}, worst err / (u T1) = {worst[0]:.4f}, err / (u T2) = {worst[1]:.4f}")
    assert np.all(err <= K * U32 * Tb + 1e-30), worst
    assert np.array_equal(res.samples, np.repeat(res.samples[at], mult[first], axis=0))
    _check_reductions(res, b, cells, 4, 2)
    # without the local outputs the column reduction is not launched: the curves' and surfaces' outputs are the same bits
    lean = pt.accumulated_effects(X32, **kw)
    assert lean.local_mean is None and lean.local_percentiles == {} and lean.samples is None
    _same(lean, res, local=False)


# ---- the outputs depend on the multiset of samples only
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 200, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def test_depends_on_the_multiset_only(sunspot, monkeypatch):
    pt, res, d = sunspot
    X = d["sunspot_test"][:40, :4]
    kw = dict(inputs=[2, 0, 3], bins=5, pairs=[(2, 0), (1, 3)], pair_bins=3, percentiles=PCTS, local=True, return_samples=True)
    base = pt.accumulated_effects(X, **kw)
    M = 4 * 100
    assert base.n_samples == M and base.samples.shape == (M, 40, 5, 1) and base.n_distinct < M
    distinct, counts = _runs(res[0], 4)
    assert base.n_distinct == len(counts)
    X32 = X.astype(np.float32)
    from ptnn_amd.ale import ale_edges
    e32 = ale_edges(X32, [2, 0, 3], 5)
    assert all(np.array_equal(a, b[:a.size].astype(np.float64)) for a, b in zip(base.edges, e32))
    pe32 = ale_edges(X32, [2, 0, 1, 3], 3, 16).reshape(2, 2, -1)
    b = [ref.bins(X32[:, j], e32[a]) for a, j in enumerate((2, 0, 3))]
    cells = [(ref.bins(X32[:, j], pe32[q][0]), ref.bins(X32[:, l], pe32[q][1])) for q, (j, l) in enumerate(((2, 0), (1, 3)))]
    _check_reductions(base, b, cells, 5, 3)
    for w in (res[0].T, (distinct, counts)):
        alt = pt.accumulated_effects(X, weights=w, **kw)
        assert alt.n_distinct == base.n_distinct
        _same(alt, base)
    for rows_blk in (1, 7):                                             # one row and a few rows per block
        monkeypatch.setenv("PTNN_ALE_SCRATCH_BYTES", str(base.n_distinct * 4 * 5 * rows_blk))
        _same(pt.accumulated_effects(X, **kw), base)
    monkeypatch.delenv("PTNN_ALE_SCRATCH_BYTES")
    # a permuted input list gives the permuted result
    order = [2, 0, 1]
    perm = pt.accumulated_effects(X, **dict(kw, inputs=[3, 2, 0]))
    assert np.array_equal(perm.samples[:, :, :3], base.samples[:, :, order]) and np.array_equal(perm.samples[:, :, 3:], base.samples[:, :, 3:])
    for f in ("bin_count", "ale_mean", "effect_range", "top_prob"):
        assert np.array_equal(getattr(perm, f), getattr(base, f)[order]), f
    assert np.array_equal(perm.sample_ale, base.sample_ale[:, order]) and np.array_equal(perm.sample_ale2, base.sample_ale2)
    for q in PCTS:
        assert np.array_equal(perm.ale_percentiles[q], base.ale_percentiles[q][order]), q
    # a pair given as (l, j) gives the transposed surface: the four corners are differenced, and the surface summed, in the other
    # order, so to rounding and not to the bit
    tr = pt.accumulated_effects(X, **dict(kw, pairs=[(0, 2), (1, 3)]))
    assert np.array_equal(tr.cell_count[0], base.cell_count[0].T) and np.array_equal(tr.sample_ale2[:, 1], base.sample_ale2[:, 1])
    scale = float(np.abs(base.sample_ale2[:, 0]).max())
    np.testing.assert_allclose(tr.sample_ale2[:, 0], np.swapaxes(base.sample_ale2[:, 0], 1, 2), rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(tr.sample_interaction[:, 0], base.sample_interaction[:, 0], rtol=1e-7, atol=0)
    # "test" and the same rows from the host; the cold chain, thinned, against its trace rows as weights
    assert np.array_equal(pt.accumulated_effects("test", inputs=[1], bins=4).ale_mean,
                          pt.accumulated_effects(d["sunspot_test"], inputs=[1], bins=4).ale_mean)
    cold = int(np.argmin(pt.temperatures))
    trw = pt._sampler.traces()["pos_w"]
    _same(pt.accumulated_effects(X, weights=trw[cold, 100::3], **kw), pt.accumulated_effects(X, chains="cold", thin=3, **kw))


# ---- known answers
@pytest.mark.parametrize("task,topo", [(REG, (5, 10, 1)), (CLS, (11, 50, 10))], ids=["reg-5", "wine"])
def test_an_unused_input_has_no_effect(task, topo, tmp_path):
    I, H, O = topo
    pt, train, _ = _make(task, topo, tmp_path, 77 + I)
    W = _vectors(topo, 9, 21 + I)
    j = I - 2
    W[:, j * H:(j + 1) * H] = 0.0                                      # W1[j, :] = 0: the nets do not read input j
    res = pt.accumulated_effects(train[:70], inputs=[0, j], bins=6, pairs=[(0, j), (j, 1), (0, 1)], pair_bins=3, weights=W, local=True,
                                 return_samples=True)
    s = res.samples
    assert np.all(s[:, :, 1] == 0) and np.all(s[:, :, 2:4] == 0) and np.any(s[:, :, 0] != 0) and np.any(s[:, :, 4] != 0)
    assert np.all(res.sample_ale[:, 1] == 0) and np.all(res.ale_mean[1] == 0) and np.all(res.effect_range[1] == 0)
    assert np.all(res.top_prob[1] == 0) and np.all(res.top_prob[0] == 1) and np.all(res.effect_range[0] > 0)
    assert np.all(res.sample_ale2[:, :2] == 0) and np.all(res.interaction[:2] == 0) and np.all(res.sample_interaction[:, :2] == 0)
    assert np.all(res.interaction[2] > 0)
    for q in res.ale_percentiles:
        assert np.all(res.ale_percentiles[q][1] == 0) and np.all(res.interaction_percentiles[q][:2] == 0)


def test_one_hidden_unit_is_monotone(tmp_path):
    topo = (4, 1, 1)
    pt, train, _ = _make(REG, topo, tmp_path, 41)
    rng = np.random.default_rng(9)
    W = rng.standard_normal((12, 7)).astype(np.float32)                # W1 [4, 1], W2 [1, 1], B1, B2
    W[:, 2] = np.abs(W[:, 2]) + 0.1                                    # W1[2] > 0
    W[:, 4] = np.abs(W[:, 4]) + 0.1                                    # W2 > 0
    res = pt.accumulated_effects("train", inputs=[2], bins=33, weights=W, local=True, return_samples=True)
    assert np.all(res.samples >= 0) and np.all(np.diff(res.sample_ale, axis=2) >= 0) and np.all(np.diff(res.ale_mean[0, :, 0]) >= 0)
    assert res.effect_range[0, 0] > 0 and res.top_prob.tolist() == [[1.0]]


def test_one_bin_is_the_partial_dependence_step(tmp_path):
    """Two edges, every row in the one bin: ALE[1] - ALE[0] = the row mean of f(z_1) - f(z_0) = PD(z_1) - PD(z_0).  The tolerance: per
    row K u T1 on this side (T_hi + T_lo + |d|) and K u (T_hi + T_lo) on partial dependence's, averaged over the rows, plus the four
    fp32 roundings of the stored curves."""
    topo = (5, 10, 1)
    pt, train, _ = _make(REG, topo, tmp_path, 23)
    W = _vectors(topo, 6, 5)
    X32 = train[:65, :5].astype(np.float32)
    X = X32.astype(np.float64)
    z = np.array([X32[:, 3].min(), X32[:, 3].max()], np.float32)
    res = pt.accumulated_effects(X32, inputs=[3], edges=[z], weights=W)
    pd = pt.partial_dependence(X32, inputs=[3], grid=z, weights=W)
    assert res.bin_count.tolist() == [[65]]
    for k in range(6):
        w = W[k].astype(np.float64)
        T = pd_ref.error_bound(X, w, topo, REG, 3, float(z[1])) + pd_ref.error_bound(X, w, topo, REG, 3, float(z[0]))
        T1 = ref.bound1(X, w, topo, REG, 3, z.astype(np.float64))
        a, p = res.sample_ale[k, 0, :, 0].astype(np.float64), pd.sample_pd[k, 0, :, 0].astype(np.float64)
        tol = K * U32 * float((T + T1).mean()) + U32 * float(np.abs(a).sum() + np.abs(p).sum())
        assert abs((a[1] - a[0]) - (p[1] - p[0])) <= tol, (k, (a[1] - a[0]) - (p[1] - p[0]), tol)


# ---- refusals that need a handle
def test_refusals(tmp_path):
    from ptnn_amd import _lib
    topo = (6, 25, 18)
    pt, train, _ = _make(CLS, topo, tmp_path, 3)
    X = train[:5, :6]
    W = _vectors(topo, 3, 1)
    e1, e2 = np.array([[0.0, 1.0]], np.float32), np.array([[[0.0, 1.0], [0.0, 1.0]]], np.float32)
    sm = pt._sampler
    with pytest.raises(_lib.PtnnError, match=r"inputs\[0\] = 6 outside \[0, 6\)"):
        sm.accumulated_effects(X, w=W, inputs=[6], edges=e1)
    with pytest.raises(_lib.PtnnError, match=r"inputs\[2\] = 4 is given twice"):
        sm.accumulated_effects(X, w=W, inputs=[4, 1, 4], edges=np.repeat(e1, 3, axis=0))
    with pytest.raises(_lib.PtnnError, match=r"edges\[5, 1\] = nan \(row 5, position 1\)"):
        sm.accumulated_effects(X, w=W, edges=np.where(np.arange(12).reshape(6, 2) == 11, np.nan, np.arange(12).reshape(6, 2) % 2).astype(np.float32))
    with pytest.raises(_lib.PtnnError, match=r"pairs\[0, 1\] = 6 outside \[0, 6\)"):
        sm.accumulated_effects(X, w=W, pairs=[(0, 6)], edges2=e2)
    with pytest.raises(_lib.PtnnError, match=r"pairs\[0, 0\] = -1 outside \[0, 6\)"):
        sm.accumulated_effects(X, w=W, inputs=[0], edges=e1, pairs=[(-1, 2)], edges2=e2)
    with pytest.raises(_lib.PtnnError, match="holds no sample"):
        sm.accumulated_effects(X, w=W, multiplicity=[0, 0, 0], inputs=[0], edges=e1)
    with pytest.raises(_lib.PtnnError, match=r"rank 3 outside \[0, 3\)"):
        sm.accumulated_effects(X, w=W, inputs=[0], edges=e1, ranks=[0, 3])
    with pytest.raises(_lib.PtnnError, match=r"rank 7 outside \[0, 3\)"):
        sm.accumulated_effects(X, w=W, inputs=[0], edges=e1, ranks2=[7])
    many = (2 ** 31 - 1) // (21 * 18) + 1                              # x (6 + 15 terms) x 18 outputs per row: past 2^31 - 1
    allp = [(j, l) for j in range(6) for l in range(j + 1, 6)]
    with pytest.raises(_lib.PtnnError, match="at most 2\\^31 - 1"):
        sm.accumulated_effects(np.zeros((many, 6), np.float32), w=W, edges=np.repeat(e1, 6, axis=0), pairs=allp, edges2=np.repeat(e2, 15, axis=0))
    with pytest.raises(ValueError, match="given twice"):
        pt.accumulated_effects(X, weights=W, inputs=[1, 1])
    # pairs alone (no first-order term) through the low-level call, then the handle is still usable
    only = sm.accumulated_effects(X, w=W, pairs=[(0, 1)], edges2=e2, sample_inter=True)
    assert only["ale_mean"] is None and only["bin_count"] is None and only["inter_mean"].shape == (1, 18) and only["cell_count"].sum() == 5
    ok = pt.accumulated_effects(X, weights=W, bins=3, pairs="all", pair_bins=2)
    assert ok.n_samples == 3 and ok.ale_mean.shape == (6, 4, 18) and ok.interaction.shape == (15, 18) and ok.samples is None
    assert np.all(ok.bin_count.sum(axis=1) == 5) and np.all(ok.cell_count.sum(axis=(1, 2)) == 5)
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
            pt.accumulated_effects("test", weights=W, percentiles=PCTS)
            pt.accumulated_effects("train", inputs=[1], bins=63, pairs=[(0, 1)], pair_bins=15, weights=(W, [2, 0, 1, 1, 3, 1, 1]), local=True,
                                   return_samples=True)
        after = snap()
        assert before[3] == after[3] == 25
        for k in before[0]:
            assert np.array_equal(before[0][k], after[0][k]), k
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        res = pt.run_chains(max_steps=10 ** 6)                          # the continuation
        pred = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
        if between:
            pt.accumulated_effects("test", percentiles=PCTS, pairs="all", local=True)
            again = pt.posterior_predictive("test", percentiles=PCTS, return_samples=True)
            assert np.array_equal(pred.mean, again.mean) and np.array_equal(pred.samples, again.samples)
        return res[0], sm.state(), sm.trace_rows(), pred.samples
    w0, s0, t0, p0 = run(False)
    w1, s1, t1, p1 = run(True)
    assert np.array_equal(w0, w1) and np.array_equal(t0, t1) and np.array_equal(p0, p1)
    for k in s0:
        assert np.array_equal(s0[k], s1[k]), k
