"""Posterior modes on the GPU (ptnn_modes / posterior_modes), against tests/modes_ref.py:
1. the distances on the device's own outputs (posterior_predictive(..., return_samples=True) of the same selection), at regression
   (4,5,1) and the classification shapes of tests/report_cases.py with the fewest and the most outputs;
2. an exact-integer known answer through values=, over the tile and column-step edges and three scratch budgets;
3. the clustering stage is exact: the reference fed the device's own matrix returns the device's rho and parent and the method's
   labels bit for bit; 4. the planted modes proven in tests/test_modes_cpu.py; 5. one multiset, one result (trace, expanded
   vectors, (distinct, counts), any block size); 6. the edges (U = 1 comes from one vector given seven times and, in 5, from one
   selected trace row: a run whose every step is rejected is not constructed); 7. nothing is disturbed.

The bound of 1, derived and not measured: |got - ref| <= 2 (n + 4) 2^-53 ref.  All terms are non-negative;
there is one rounding in the widened difference, hence two relative to its square, and one per accumulation; (n + 2) u covers any
order, and the factor leaves 2 x.  The reference is the np.longdouble sum on the device's own fp32 outputs, so the whole bound is
the device's.  The largest deviation seen is printed as a share of the bound."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import modes_cases
import modes_ref as ref
import parity
import uncertainty_cases as cases
from parity import orc
from test_gpu_predict import _pt, _runs

pytestmark = pytest.mark.gpu

CLS, REG = orc.TASK_CLS, orc.TASK_REG
COMMON = ("n_modes", "sample_labels", "centres", "mass", "mode_mean", "mode_sd", "between", "within", "rho", "delta", "parent", "spread",
          "n_samples", "n_distinct")
CHAINS = ("labels", "centre_rows", "occupancy", "hops", "hop_matrix")


def _make(task, topo, tmp_path, train, test):
    kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
    return _pt(task, topo, np.array(train), np.array(test), 4, 20, tmp_path, **kw)


def _same(a, b, fields=COMMON):
    for name in fields:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


# ---- 1: the distances on the device's own outputs
GRID = [(REG, (4, 5, 1)), (CLS, min(cases.CLS_SHAPES, key=lambda t: t[2])), (CLS, max(cases.CLS_SHAPES, key=lambda t: t[2]))]


@pytest.fixture(scope="module", params=GRID, ids=["-".join(map(str, t)) for _, t in GRID])
def grid(request, tmp_path_factory):
    task, topo = request.param
    if task == REG:
        train, test, W, _, _ = cases.regression_case(topo)
    else:
        train, test, W, _ = cases.report_cases.case(topo)
    pt = _make(task, topo, tmp_path_factory.mktemp("grid"), train, test)
    mult = cases.multiplicities(len(W))
    pred = pt.posterior_predictive("test", weights=(W, mult), return_samples=True)
    n = pred.samples.shape[1] * pred.samples.shape[2]
    radius = 0.025
    low = pt._sampler.modes("test", radius_sq_sum=radius * radius * n, w=W, multiplicity=mult, sq_dist=True, outputs=True)
    return dict(task=task, topo=topo, pt=pt, W=W, mult=mult, pred=pred, n=n, radius=radius, low=low)


def test_distances_on_the_devices_own_outputs(grid):
    g = grid
    low, mult, n = g["low"], g["mult"], g["n"]
    U = len(g["W"])
    assert low["n_distinct"] == U == 65 and low["n_samples"] == int(mult.sum()) and np.array_equal(low["count"], mult)
    assert low["sq_dist"].shape == (U, U) and low["outputs"].shape == (U, n) and low["outputs"].dtype == np.float32
    assert np.array_equal(low["item_sample"], np.arange(U))
    # the outputs are the predictive samples' distinct rows, bit for bit
    start = np.concatenate([[0], np.cumsum(mult)[:-1]])
    present = mult > 0
    assert np.array_equal(low["outputs"][present], g["pred"].samples.reshape(-1, n)[start[present]])
    want = ref.sq_longdouble(low["outputs"])
    dev = np.abs(low["sq_dist"].astype(np.longdouble) - want).astype(np.float64)
    bound = ref.bound(n, want.astype(np.float64))
    share = float(np.max(np.where(bound > 0, dev / np.where(bound > 0, bound, 1.0), np.where(dev == 0, 0.0, np.inf))))
    print(f"{g['topo']}: largest deviation of sq as a share of its bound 2 (n + 4) 2^-53 ref, n = {n}: {share:.3g}")
    assert share <= 1.0
    assert (np.diag(low["sq_dist"]) == 0.0).all() and np.array_equal(low["sq_dist"], low["sq_dist"].T)
    assert low["spread_sq"] == pytest.approx(float(ref.spread_sq(low["sq_dist"], mult)), rel=1e-12)
    # the low-level call leaves out what is not asked for, and the same numbers come back
    bare = g["pt"]._sampler.modes("test", radius_sq_sum=g["radius"] ** 2 * n, w=g["W"], multiplicity=mult)
    assert bare["sq_dist"] is None and bare["outputs"] is None
    for k in ("rho", "delta_sq", "parent", "count", "item_sample"):
        assert np.array_equal(bare[k], low[k]), k
    assert bare["spread_sq"] == low["spread_sq"]


# ---- 3 (on 1): the clustering stage is exact
def test_clustering_stage_is_exact_on_the_devices_matrix(grid):
    g = grid
    low, mult, n, radius = g["low"], g["mult"], g["n"], g["radius"]
    rho, delta, parent = ref.density_peaks(low["sq_dist"], mult, radius * radius * n)
    assert np.array_equal(low["rho"], rho) and np.array_equal(low["parent"], parent) and np.array_equal(low["delta_sq"], delta)
    assert low["rho"].dtype == np.int64 and low["parent"].dtype == np.int32 and low["rho"][1] == 0 and low["parent"][1] == -1
    sep = 2 * radius
    pm = g["pt"].posterior_modes("test", separation=sep, weights=(g["W"], mult), return_distances=True)
    lab, centres, mass = ref.labels_of(rho, delta, parent, mult, sep * sep * n, int(np.ceil(0.02 * mult.sum())))
    assert np.array_equal(pm.sample_labels, lab) and np.array_equal(pm.centres, centres) and np.array_equal(pm.mass, mass / mult.sum())
    assert pm.n_modes == len(centres) and np.array_equal(pm.rho, rho) and np.array_equal(pm.parent, parent)
    assert np.array_equal(pm.delta, np.sqrt(delta / n)) and np.array_equal(pm.distances, np.sqrt(low["sq_dist"] / n))
    assert pm.occupancy is None and pm.hops is None and pm.hop_matrix is None and np.array_equal(pm.labels, lab)
    assert pm.spread == np.sqrt(low["spread_sq"] / n) and pm.sample_labels[1] == -1 and pm.mode_mean.shape == (pm.n_modes,) + g["pred"].mean.shape


def test_duplicates_that_are_not_neighbours(grid):
    g = grid
    pick = np.array([0, 2, 3, 0, 4, 2, 0, 5, 5, 6, 3])                      # 5, 5 merge into one run; the other repeats stay distinct samples
    W, n = g["W"][pick], g["n"]
    mult = np.array([1, 2, 1, 1, 3, 2, 1, 1, 1, 2, 1], np.int32)
    low = g["pt"]._sampler.modes("test", radius_sq_sum=0.0, w=W, multiplicity=mult, sq_dist=True)
    assert low["n_distinct"] == 10 and low["item_sample"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9]
    count = low["count"]
    assert count.tolist() == [1, 2, 1, 1, 3, 2, 1, 2, 2, 1]
    sq = low["sq_dist"]
    assert sq[0, 3] == 0.0 and sq[3, 6] == 0.0 and sq[1, 5] == 0.0 and sq[2, 9] == 0.0 and sq[0, 1] > 0.0
    rho, delta, parent = ref.density_peaks(sq, count, 0.0)                   # radius 0: only duplicates are near
    assert rho.tolist() == [3, 4, 2, 3, 3, 4, 3, 2, 2, 2]
    assert np.array_equal(low["rho"], rho) and np.array_equal(low["parent"], parent) and np.array_equal(low["delta_sq"], delta)
    assert parent[5] == 1 and delta[5] == 0.0 and parent[3] == 0 and parent[6] == 0 and parent[1] == -1
    pm = g["pt"].posterior_modes("test", separation=1e-6, radius=0.0, min_mass=0.0, weights=(W, mult))
    lab, centres, mass = ref.labels_of(rho, delta, parent, count, 1e-12 * n, 0)
    assert np.array_equal(pm.sample_labels, lab) and pm.n_modes == 6 and np.array_equal(pm.centres, centres)
    assert np.array_equal(pm.labels, lab[low["item_sample"]]) and pm.labels.shape == (11,)
    assert pm.centre_rows[:, 0].tolist() == [-1] * 6 and pm.centre_rows[:, 1].tolist() == [int(np.flatnonzero(low["item_sample"] == c)[0]) for c in centres]


# ---- 2: an exact-integer known answer through values=
N_U, N_COLS = (1, 2, 63, 64, 65, 129), (1, 31, 32, 33, 65)
SIZES = list(itertools.product(N_U, N_COLS))                               # two axes: every pair is the product


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    return _make(REG, (4, 5, 1), tmp_path_factory.mktemp("handle"), train, test)


@pytest.mark.parametrize("U, n_a", SIZES, ids=lambda v: str(v))
def test_exact_integer_known_answer(handle, monkeypatch, U, n_a):
    rng = np.random.default_rng(1000 + 10 * U + n_a)
    A0 = rng.integers(-8, 9, (U, n_a))
    if U >= 4:
        A0[3] = A0[0]                                                       # a duplicate that is no neighbour
    off = rng.integers(-100, 101, n_a)
    values = (A0 + off).astype(np.float32)
    mult = rng.integers(0, 4, U).astype(np.int32)
    mult[0] = max(mult[0], 1)
    if U >= 2:
        mult[1] = 0
    M = int(mult.sum())
    sq = ((A0[:, None, :] - A0[None, :, :]) ** 2).sum(axis=2)
    near = int(np.median(sq))
    rho, delta, parent = ref.density_peaks(sq.astype(np.float64), mult, float(near))
    total = int((mult[:, None].astype(np.int64) * mult[None, :] * sq).sum())
    want_spread = Fraction(total, M * M)
    for budget in (None, 4 * U * max(1, n_a // 3), 1):
        if budget is not None:
            monkeypatch.setenv("PTNN_MODES_SCRATCH_BYTES", str(budget))
        out = handle._sampler.modes(radius_sq_sum=float(near), values=values, multiplicity=mult, sq_dist=True, outputs=True)
        assert out["n_samples"] == M and out["n_distinct"] == U and np.array_equal(out["item_sample"], np.arange(U))
        assert np.array_equal(out["sq_dist"], sq.astype(np.float64)), (np.argwhere(out["sq_dist"] != sq)[:5], budget)
        assert np.array_equal(out["rho"], rho) and np.array_equal(out["parent"], parent) and np.array_equal(out["delta_sq"], delta)
        assert np.array_equal(out["count"], mult) and np.array_equal(out["outputs"], values)
        if total % (M * M) == 0:
            assert out["spread_sq"] == float(want_spread)
        else:
            assert abs(out["spread_sq"] - float(want_spread)) <= 2 * np.spacing(float(want_spread))


# ---- 4: planted modes
@pytest.mark.parametrize("topo", [modes_cases.REG_TOPO, modes_cases.CLS_TOPO], ids=lambda t: "-".join(map(str, t)))
def test_planted_modes(topo, tmp_path):
    task, train, test, W, mult, group, base, sep, radius = modes_cases.planted(topo)
    pt = _make(task, topo, tmp_path, train, test)
    pm = pt.posterior_modes("test", separation=sep, weights=(W, mult), return_distances=True)
    want, mass = modes_cases.planted_labels(group, mult)
    assert pm.n_modes == 3 and np.array_equal(pm.sample_labels, want) and np.array_equal(pm.labels, want) and np.array_equal(pm.mass, mass)
    assert all(want[c] == k for k, c in enumerate(pm.centres)) and pm.n_distinct == len(W) and pm.n_samples == int(mult.sum())
    for u in np.flatnonzero(base >= 0):                                     # a permuted copy: the same function up to fp32 rounding
        assert pm.sample_labels[u] == pm.sample_labels[base[u]] and pm.distances[u, base[u]] <= modes_cases.report_cases.MARGIN
    assert (pm.between[~np.eye(3, dtype=bool)] >= 4 * sep - 2 * modes_cases.report_cases.MARGIN).all() and (pm.within <= radius / 4 + 2 * modes_cases.report_cases.MARGIN).all()
    assert (np.diag(pm.between) == 0).all() and np.array_equal(pm.between, pm.between.T)
    for k in range(3):
        mem = want == k
        pred = pt.posterior_predictive("test", weights=(W[mem], mult[mem]), return_samples=True)
        assert np.allclose(pm.mode_mean[k], pred.mean, rtol=0, atol=1e-12)
        assert np.allclose(pm.mode_sd[k], pred.samples.astype(np.float64).std(axis=0), rtol=0, atol=1e-9)


# ---- 5: one multiset, one result
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 400, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d


def test_one_multiset_one_result(sunspot, monkeypatch):
    pt, res, d = sunspot
    R, S = 4, 400
    x = d["sunspot_test"][:37]
    base = pt.posterior_modes(x)
    assert base.n_samples == R * (S - S // 2) and 1 < base.n_distinct < base.n_samples and base.labels.shape == (4, 200)
    assert base.occupancy.shape == (4, base.n_modes) and base.hops.shape == (4,) and base.hop_matrix.shape == (base.n_modes,) * 2
    assert (base.labels >= 0).all() and np.allclose(base.occupancy.sum(axis=1), 1.0) and abs(base.mass.sum() - 1.0) < 1e-12
    occ, hops, hm = ref.chain_figures(base.labels, base.n_modes)
    assert np.array_equal(base.occupancy, occ) and np.array_equal(base.hops, hops) and np.array_equal(base.hop_matrix, hm)
    assert np.array_equal(base.labels[base.centre_rows[:, 0], base.centre_rows[:, 1]], np.arange(base.n_modes))
    wd, counts = _runs(res[0], R)
    assert len(wd) == base.n_distinct
    expanded = pt.posterior_modes(x, weights=res[0].T)
    distinct = pt.posterior_modes(x, weights=(wd, counts))
    _same(base, expanded)
    _same(base, distinct)
    assert np.array_equal(expanded.labels, base.labels.reshape(-1)) and np.array_equal(distinct.labels, base.sample_labels)
    for budget in (37 * base.n_distinct * 4 // 3, 1):
        monkeypatch.setenv("PTNN_MODES_SCRATCH_BYTES", str(budget))
        _same(base, pt.posterior_modes(x), COMMON + CHAINS)
        _same(base, pt.posterior_modes(x, weights=res[0].T))
        _same(base, pt.posterior_modes(x, weights=(wd, counts)))
    monkeypatch.delenv("PTNN_MODES_SCRATCH_BYTES")
    cold = pt.posterior_modes("test", chains="cold", thin=3)
    m = -(-(S - S // 2) // 3)
    assert cold.n_samples == m and cold.labels.shape == (1, m) and cold.occupancy.shape == (1, cold.n_modes) and cold.hops.shape == (1,)
    assert cold.mode_mean.shape == (cold.n_modes, 198, 1)
    one = pt.posterior_modes("test", chains="cold", thin=10 ** 6)           # one selected row: U = 1 through the trace
    assert one.n_distinct == 1 and one.n_samples == 1 and one.n_modes == 1 and one.mass.tolist() == [1.0] and one.hops.tolist() == [0]
    assert one.labels.tolist() == [[0]] and one.occupancy.tolist() == [[1.0]] and one.centre_rows.tolist() == [[0, 0]] and one.spread == 0.0
    from ptnn_amd.parallel_tempering import modes_stuck
    stuck = modes_stuck(base, min_mass=0.0)
    assert stuck.shape[1] == 2 and all(base.occupancy[c, k] == 0 for c, k in stuck)


# ---- 6: the edges
def test_edges(handle):
    pt = handle
    from ptnn_amd import _lib
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    # one distinct sample: one mode of mass 1
    one = pt.posterior_modes("test", weights=np.repeat(W[:1], 7, axis=0))
    assert one.n_distinct == 1 and one.n_samples == 7 and one.n_modes == 1 and one.mass.tolist() == [1.0] and (one.labels == 0).all()
    assert one.spread == 0.0 and one.within.tolist() == [0.0] and one.rho.tolist() == [7] and one.parent.tolist() == [-1]
    # U past the cap: refused before the device, the way down named
    with pytest.raises(_lib.PtnnError, match=r"11586 distinct samples.*thin=, chains="):
        pt.posterior_modes(values=np.zeros((11586, 1), np.float32))
    # radius 0: only duplicates are near
    v = np.array([[0.0], [1.0], [0.0], [2.0]], np.float32)
    z = pt.posterior_modes(values=(v, [1, 1, 2, 1]), radius=0.0, separation=0.5)
    assert z.rho.tolist() == [3, 1, 3, 1] and z.parent.tolist() == [-1, 0, 0, 1] and z.n_modes == 3 and z.sample_labels.tolist() == [0, 1, 0, 2]
    assert z.mass.tolist() == [0.6, 0.2, 0.2] and (z.centre_rows == -1).all() and z.mode_mean.shape == (3, 1) and z.occupancy is None
    # NaN weights: refused, the sample named
    bad = W[:6].copy()
    bad[4, 0] = np.nan
    with pytest.raises(_lib.PtnnError, match="not finite: sample 4 is the first"):
        pt.posterior_modes("test", weights=bad)
    with pytest.raises(_lib.PtnnError, match="near_sq = -1 must be a finite number >= 0"):
        pt._sampler.modes("test", radius_sq_sum=-1.0, w=W[:3])
    with pytest.raises(_lib.PtnnError, match="holds no sample"):
        pt._sampler.modes("test", radius_sq_sum=1.0, w=W[:3], multiplicity=[0, 0, 0])
    again = pt.posterior_modes("test", weights=W[:6])                       # a refused call leaves the handle usable
    assert again.n_distinct == 6


# ---- 7: nothing is disturbed
@pytest.mark.parametrize("task", [CLS, REG], ids=["cls", "reg"])
def test_no_side_effects(task, tmp_path):
    d = parity.datasets()
    outs = []
    for call in (True, False):
        (tmp_path / str(call)).mkdir(exist_ok=True)
        if task == CLS:
            pt = _pt(CLS, (4, 12, 3), d["iris_train"], d["iris_test"], 8, 400, tmp_path / str(call), lr=0.01, maxtemp=10)
        else:
            pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 400, tmp_path / str(call))
        assert pt.run_chains(max_steps=170) is None
        if call:
            w = pt._sampler.traces(60, 100)["pos_w"].reshape(-1, pt.num_param)
            pm = pt.posterior_modes("test", weights=w)
            assert pm.n_samples == 800 and pm.n_modes >= 1
            low = pt._sampler.modes("train", radius_sq_sum=1.0, step0=100, nsteps=60, thin=2, sq_dist=True)
            assert low["n_samples"] == 240 and np.isfinite(low["sq_dist"]).all() and low["item_sample"].shape == (240,)
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
