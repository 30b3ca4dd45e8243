"""Posterior compression on the GPU (ptnn_compress / posterior_compress), against tests/compress_ref.py:
1. exact through values=: the known answer and integer points on a line -- every distance an integer, every order defined -- bit for
   bit against the float64 replay, over the strides of the two kernels (256, 1024), m = 1 and m = present, absent samples, and
   three scratch budgets;
2. on the device's own matrix, real nets: regression (4,5,1) and the classification shapes of tests/report_cases.py with the fewest
   and the most outputs; the reference replays in np.longdouble from the device's own sq_dist;
3. one multiset, one result (trace, expanded vectors, (distinct, counts)); 4. the round trip through the public method;
5. nothing is disturbed; 6. the edges.

The bound of 2, derived and not measured: with u = 2^-53, tol_j = 4 (U + j + 4) u (max mu + max d).  mu and r
are sums of at most U and j non-negative terms; each term carries one rounding of the square root and one of the product, each
addition one more; the factor 4 leaves 2 x.  At every step the device's pick must score within tol_j of the reference's minimum,
so wherever the reference's runner-up is more than 2 tol_j away the pick is the reference's.  The same count bounds the other
outputs: mu by (U + 2) u max d, D0 by (2 U + 4) u max mu, and energy_n = 2 musum / n - pair / n^2 - D0 by u ((2 (U + n + 4) +
2 U + 4) max mu + (2 n + 4) max d), each below tol_n.  The largest deviation seen is printed as a share of the bound."""
import numpy as np
import pytest

import compress_cases
import compress_ref as ref
import parity
import uncertainty_cases as cases
from parity import orc
from test_gpu_predict import _pt, _runs

pytestmark = pytest.mark.gpu

CLS, REG = orc.TASK_CLS, orc.TASK_REG
U53 = 2.0 ** -53


def _make(task, topo, tmp_path, train, test, R=4, S=20):
    kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
    return _pt(task, topo, np.array(train), np.array(test), R, S, tmp_path, **kw)


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    return _make(REG, (4, 5, 1), tmp_path_factory.mktemp("handle"), train, test)


# ---- 1: exact through values=
def _exact(pt, values, count, m, subsets, want):
    out = pt._sampler.compress(values=values, multiplicity=count, m=m, subsets=subsets, sq_dist=True, outputs=True)
    U = len(values)
    assert out["n_distinct"] == U and out["n_samples"] == int(np.sum(count)) and np.array_equal(out["item_sample"], np.arange(U))
    assert np.array_equal(out["count"], count) and np.array_equal(out["outputs"], values) and np.array_equal(out["sq_dist"], want["sq"])
    assert np.array_equal(out["mu"], want["mu"]), np.flatnonzero(out["mu"] != want["mu"])[:5]
    assert out["d0"] == want["d0"]
    assert np.array_equal(out["picks"], want["picks"][:m]), (np.flatnonzero(out["picks"] != want["picks"][:m])[:5], m)
    assert np.array_equal(out["energy"], want["energy"][:m]) and np.array_equal(out["pick_score"], want["pick_score"][:m])
    if subsets is not None:
        assert np.array_equal(out["subset_energy"], want["subset_energy"])
    return out


def test_known_answer_bit_for_bit(handle, monkeypatch):
    values, count, m = compress_cases.KNOWN_VALUES, compress_cases.KNOWN_COUNTS, compress_cases.KNOWN_M
    sq = ref.sq_of(values)
    want = dict(ref.herd(sq, count, m), sq=sq)
    assert want["picks"].tolist() == compress_cases.KNOWN_PICKS
    subsets = np.array([[3, 6, 1], [0, 0, 7], [2, 4, 6]], np.int32)
    want["subset_energy"] = np.array([ref.subset_energy(sq, count, s, mu=want["mu"], d0=want["d0"]) for s in subsets])
    assert want["subset_energy"][0] == pytest.approx(want["energy"][2], rel=1e-12)
    for budget in (None, 16, 1):
        if budget is not None:
            monkeypatch.setenv("PTNN_MODES_SCRATCH_BYTES", str(budget))
        out = _exact(handle, values, count, m, subsets, want)
        assert 5 not in out["picks"] and out["energy"][4] > out["energy"][3] and out["energy"][6] > out["energy"][5]
        for got, expect in zip(out["energy"], compress_cases.KNOWN_ENERGY):
            assert abs(got - expect) <= 1e-12 * expect
    monkeypatch.delenv("PTNN_MODES_SCRATCH_BYTES")
    pc = handle.posterior_compress(m, values=(values, count), evaluate=subsets, return_distances=True)
    assert pc.picks.tolist() == compress_cases.KNOWN_PICKS and np.array_equal(pc.energy, want["energy"]) and pc.spread == want["d0"]
    assert np.array_equal(pc.evaluated, want["subset_energy"]) and np.array_equal(pc.distances, np.sqrt(sq)) and pc.vectors is None
    assert np.array_equal(pc.items, pc.picks) and (pc.rows == -1).all() and np.array_equal(pc.equivalent_draws, want["d0"] / want["energy"])


@pytest.mark.parametrize("U", compress_cases.LINE_U)
def test_integer_points_on_a_line_bit_for_bit(handle, monkeypatch, U):
    values = compress_cases.line(U)
    count = cases.multiplicities(U) if U > 1 else np.array([2], np.int32)
    present = int((count > 0).sum())
    assert present < U or U == 1                                            # some samples are absent
    sq = ref.sq_of(values)
    want = dict(ref.herd(sq, count, present), sq=sq)
    assert not set(want["picks"].tolist()) & set(np.flatnonzero(count == 0).tolist()) and len(set(want["picks"].tolist())) == present
    rng = np.random.default_rng(U)
    live = np.flatnonzero(count > 0)
    subsets = live[rng.integers(0, present, (2, min(present, 19)))].astype(np.int32)
    want["subset_energy"] = np.array([ref.subset_energy(sq, count, s, mu=want["mu"], d0=want["d0"]) for s in subsets])
    for budget in (None, 4 * max(1, U // 3), 1):
        if budget is not None:
            monkeypatch.setenv("PTNN_MODES_SCRATCH_BYTES", str(budget))
        for m in sorted({1, present}):
            _exact(handle, values, count, m, subsets, want)


# ---- 2: on the device's own matrix, real nets
GRID = [(REG, (4, 5, 1)), (CLS, min(cases.CLS_SHAPES, key=lambda t: t[2])), (CLS, max(cases.CLS_SHAPES, key=lambda t: t[2]))]


@pytest.mark.parametrize("task, topo", GRID, ids=["-".join(map(str, t)) for _, t in GRID])
def test_on_the_devices_own_matrix(task, topo, tmp_path):
    if task == REG:
        train, test, W, _, _ = cases.regression_case(topo)
    else:
        train, test, W, _ = cases.report_cases.case(topo)
    pt = _make(task, topo, tmp_path, train, test)
    mult = cases.multiplicities(len(W))
    U, m = len(W), 16
    assert U == 65
    live = np.flatnonzero(mult > 0)
    subsets = live[np.random.default_rng(3).integers(0, len(live), (3, 11))].astype(np.int32)
    low = pt._sampler.compress("test", m=m, subsets=subsets, w=W, multiplicity=mult, sq_dist=True, outputs=True)
    modes = pt._sampler.modes("test", radius_sq_sum=1.0, w=W, multiplicity=mult, sq_dist=True, outputs=True)
    for k in ("sq_dist", "outputs", "count", "item_sample"):
        assert np.array_equal(low[k], modes[k]), k                          # the shared helper: ptnn_modes' bits
    assert low["n_distinct"] == U and low["n_samples"] == int(mult.sum()) == modes["n_samples"]
    sq = low["sq_dist"]
    L = np.longdouble
    want = ref.herd(sq, mult, m, dtype=L, follow=low["picks"])
    scale = float(want["mu"].max() + np.sqrt(sq.max()))
    tol = np.array([4 * (U + j + 4) * U53 * scale for j in range(m + 1)])
    assert len(set(low["picks"].tolist())) == m and (mult[low["picks"]] > 0).all()
    shares = dict(pick=float((want["gap"].astype(np.float64) / tol[:m]).max()),
                  mu=float(np.abs(low["mu"].astype(L) - want["mu"]).max() / tol[0]), d0=float(abs(L(low["d0"]) - want["d0"]) / tol[0]),
                  energy=float((np.abs(low["energy"].astype(L) - want["energy"]).astype(np.float64) / tol[1:]).max()),
                  score=float((np.abs(low["pick_score"].astype(L) - want["pick_score"]).astype(np.float64) / tol[:m]).max()))
    sub = np.array([ref.subset_energy(sq, mult, s, dtype=L, mu=want["mu"], d0=want["d0"]) for s in subsets])
    shares["subset"] = float(np.abs(low["subset_energy"].astype(L) - sub).max() / (4 * (U + 11 + 4) * U53 * scale))
    print(f"{topo}: largest deviations as shares of tol_j = 4 (U + j + 4) 2^-53 (max mu + max d), U = {U}: "
          + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))
    assert (want["gap"] >= 0).all() and max(shares.values()) <= 1.0
    # wherever the reference's own runner-up is more than 2 tol_j away, the pick is the reference's: the float64 replay agrees
    same = ref.herd(sq, mult, m)
    assert np.array_equal(same["picks"], low["picks"]) and np.array_equal(same["energy"], low["energy"]) and np.array_equal(same["mu"], low["mu"])
    assert same["d0"] == low["d0"] and low["mu"][1] == 0.0 and 1 not in low["picks"]
    # the public method on the same selection
    pc = pt.posterior_compress(m, "test", weights=(W, mult), evaluate=subsets)
    assert np.array_equal(pc.picks, low["picks"]) and np.array_equal(pc.energy, low["energy"]) and np.array_equal(pc.evaluated, low["subset_energy"])
    assert np.array_equal(pc.vectors, W[pc.picks].astype(np.float32)) and pc.eta is None and (pc.energy > -tol[1:]).all()


# ---- 3 and 4: a short run
@pytest.fixture(scope="module")
def short(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 20, tmp_path_factory.mktemp("short"))
    res = pt.run_chains()
    return pt, res


def test_one_multiset_one_result(short):
    pt, res = short
    base = pt.posterior_compress(6, "train")
    assert base.n_samples == 4 * 10 and 6 <= base.n_distinct <= base.n_samples and base.rows.shape == (6, 2)
    wd, counts = _runs(res[0], 4)
    assert len(wd) == base.n_distinct
    expanded = pt.posterior_compress(6, "train", weights=res[0].T)
    distinct = pt.posterior_compress(6, "train", weights=(wd, counts))
    for other in (expanded, distinct):
        assert np.array_equal(other.vectors, base.vectors) and np.array_equal(other.picks, base.picks)
        for name in ("energy", "spread", "mu", "equivalent_draws", "energy_thinned", "mean_gap", "sd_ratio", "pick_score"):
            assert np.array_equal(getattr(other, name), getattr(base, name)), name
    assert np.array_equal(expanded.items, base.items) and np.array_equal(distinct.items, base.picks)
    assert np.array_equal(base.vectors, wd[base.picks])


def test_round_trip_through_the_public_method(short):
    pt, res = short
    pc = pt.posterior_compress(8, "train")
    kw, M = pt._trace_selection(None, "all", 1)
    low = pt._sampler.compress("train", m=8, sq_dist=True, outputs=True, **kw)
    assert np.array_equal(pc.picks, low["picks"]) and pc.n_samples == M == 40
    n = low["outputs"].shape[1]
    pred = pt.posterior_predictive("train", weights=pc.vectors)
    assert pred.n_samples == 8
    assert np.allclose(pred.mean.reshape(-1), low["outputs"][pc.picks].astype(np.float64).mean(axis=0), rtol=1e-6, atol=1e-7)
    eta = pt._sampler.eta_trace()
    step0 = kw["step0"]
    assert pc.eta.dtype == np.float32 and np.array_equal(pc.eta, eta[pc.rows[:, 0], step0 + pc.rows[:, 1]])
    assert np.array_equal(pc.vectors, pt._sampler.traces()["pos_w"][pc.rows[:, 0], step0 + pc.rows[:, 1]])
    assert np.array_equal(low["item_sample"][pc.items], pc.picks) and np.array_equal(pc.items, pc.rows[:, 0] * 10 + pc.rows[:, 1])
    held = pt.posterior_compress(0, "train", evaluate=pc.items)
    assert held.evaluated.shape == (1,) and held.evaluated[0] == pytest.approx(pc.energy[-1], rel=1e-12) and held.picks.shape == (0,)
    thinned = (np.arange(8) * 40) // 8
    want = ref.subset_energy(low["sq_dist"], low["count"], low["item_sample"][thinned], mu=low["mu"], d0=low["d0"])
    assert pc.energy_thinned == want
    assert pc.spread == low["d0"] and pc.spread_rms == low["d0"] / np.sqrt(n) and np.array_equal(pc.energy_rms, low["energy"] / np.sqrt(n))
    # judged on rows the picks were not chosen on, and taken by another analysis call with their eta
    other = pt.posterior_compress(0, "test", evaluate=pc.items)
    assert other.evaluated[0] > 0 and np.isfinite(other.evaluated[0])
    cal = pt.predictive_calibration("test", weights=pc.vectors, eta=pc.eta)
    assert cal is not None


# ---- 5: nothing is disturbed
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
            pc = pt.posterior_compress(5, "test", weights=w)
            assert pc.n_samples == 800 and pc.picks.shape == (5,)
            low = pt._sampler.compress("train", m=7, subsets=np.array([[0, 1, 2]], np.int32), step0=100, nsteps=60, thin=2, sq_dist=True)
            assert low["n_samples"] == 240 and np.isfinite(low["energy"]).all() and low["item_sample"].shape == (240,)
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


# ---- 6: the edges
def test_edges(handle):
    pt = handle
    from ptnn_amd import _lib
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    # m = 0 with evaluate= only
    z = pt.posterior_compress(0, "test", weights=W[:9], evaluate=[[0, 4, 8], [2, 2, 2]])
    assert z.picks.shape == (0,) and z.energy.shape == (0,) and z.evaluated.shape == (2,) and z.energy_thinned is None and z.spread > 0
    low = pt._sampler.compress("test", m=0, w=W[:9], sq_dist=True)
    assert z.evaluated[0] == ref.subset_energy(low["sq_dist"], low["count"], [0, 4, 8]) and z.evaluated[1] == ref.subset_energy(low["sq_dist"], low["count"], [2, 2, 2])
    # one distinct sample, one vector given seven times: the spread is 0 and so is the energy
    one = pt.posterior_compress(1, "test", weights=np.repeat(W[:1], 7, axis=0))
    assert one.n_distinct == 1 and one.n_samples == 7 and one.picks.tolist() == [0] and one.energy.tolist() == [0.0] and one.spread == 0.0
    assert one.items.tolist() == [0] and np.array_equal(one.vectors, W[:1].astype(np.float32)) and one.energy_thinned == 0.0
    # U past the cap: refused before the device, the way down named
    with pytest.raises(_lib.PtnnError, match=r"11586 distinct samples.*thin=, chains="):
        pt.posterior_compress(2, values=np.zeros((11586, 1), np.float32))
    # more picks than present samples: both numbers in the text
    with pytest.raises(_lib.PtnnError, match="m = 3 picks but the selection has 2 present distinct samples"):
        pt.posterior_compress(3, "test", weights=np.repeat(W[:2], 2, axis=0))
    # a subset that holds an absent sample, an entry out of range
    v = np.array([[0.0], [1.0], [3.0]], np.float32)
    with pytest.raises(_lib.PtnnError, match="subset 1 holds item 1, whose sample 1 is absent"):
        pt._sampler.compress(values=v, multiplicity=[1, 0, 2], m=1, subsets=np.array([[0, 2], [2, 1]], np.int32))
    with pytest.raises(_lib.PtnnError, match=r"subset 0 holds item 3 outside \[0, 3\)"):
        pt._sampler.compress(values=v, m=1, subsets=np.array([[0, 3]], np.int32))
    # NaN weights: refused, the sample named
    bad = W[:6].copy()
    bad[4, 0] = np.nan
    with pytest.raises(_lib.PtnnError, match="not finite: sample 4 is the first"):
        pt.posterior_compress(2, "test", weights=bad)
    again = pt.posterior_compress(2, "test", weights=W[:6])                 # a refused call leaves the handle usable
    assert again.n_distinct == 6 and again.picks.shape == (2,)
