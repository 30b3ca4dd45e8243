"""Rank-normalised convergence diagnostics on the GPU (ptnn_rank_convergence / rank_diagnostics): z-scores, rank histograms, bulk and
tail R-hat, bulk / tail / quantile ESS and the per-chain figures against the float64 reference (tests/rank_ref.py) on host draws,
source agreement on a sampled trace, blocking, absence of side effects and the refusals.

Tolerances.  z: the device and the reference evaluate the same AS241 rationals; Z_MEASURED is the largest |z_dev - z_ref| seen over
the grid below on an MI355X and the bound is four times that, under the 1e-12 the project allows moments.
Ranks recovered from the histogram are exact.  R-hat within 1e-12 relative, ESS within 1e-10 relative, NaN and inf matched
exactly, a truncation compared only where the deciding pair sum is at least 1e-9 in size (at most one quantity per case), as in
test_gpu_convergence.py.  One more case is decided within rounding, and by the reference alone: where every split chain of a
series is constant but the chains differ, W is mathematically 0 and R-hat +inf, and in floating point W is whatever the rounding
of the mean of h equal numbers leaves (exactly 0 when h is a power of two, else of the order (1e-16 z)^2, R-hat of the order
1e16).  So for h a power of two +inf is matched by +inf alone, on the device as in the reference ((64, 4, 300) "special" is such a
case); for any other h a reference R-hat above 1e12 -- no series that varies within a chain gets near it -- is matched by +inf or
by any value above 1e12."""
import math

import numpy as np
import pytest

import parity
import rank_cases as rc
import rank_ref as rr
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 4242
Z_MEASURED = 1.332e-15      # max |z_dev - z_ref| over GRID x KINDS, measured on an MI355X (3 ulp of the largest |z|, 3.9)
Z_BOUND = 4 * Z_MEASURED
PROBS, KINDS, GRID = rc.PROBS, rc.KINDS, rc.GRID


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


def _same(got, want, tol):
    """|got - want| <= tol |want|, or both NaN, or the same infinity."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want)) | (np.isfinite(want) & (np.abs(got - want) <= tol * np.abs(want)))


def _r_hat_ok(got, want, h):
    """R-hat of split chains of h draws within 1e-12; where h is no power of two, W = 0 holds within rounding only (the module
    docstring)."""
    ok = _same(got, want, 1e-12)
    if h & (h - 1):
        with np.errstate(invalid="ignore"):
            ok = ok | ((want > 1e12) & (got > 1e12))
    return ok


def _check(out, want, per_chain):
    """The tolerances of the module docstring -> (quantities exempt from an ESS comparison, max |z - z_ref|)."""
    C, B, Q = out["rank_hist"].shape
    h = want["z"].shape[1] // 2
    bad = np.isnan(want["z"]).any(axis=(0, 1))
    assert np.array_equal(np.isnan(out["z"]), np.isnan(want["z"]))
    zerr = float(np.max(np.abs(out["z"][:, :, ~bad] - want["z"][:, :, ~bad]), initial=0.0))
    print(f"max |z_dev - z_ref| = {zerr:.3e}")
    assert zerr <= Z_BOUND, zerr
    assert out["rank_hist"].dtype == np.int64 and np.array_equal(out["rank_hist"], want["rank_hist"])
    assert np.all(out["rank_hist"].sum(axis=1)[:, ~bad] == want["z"].shape[1]) and not out["rank_hist"][:, :, bad].any()
    if B == 2 * want["ranks"].size // Q:                                          # a bin per half rank: the histogram holds the ranks
        for q in np.flatnonzero(~bad):
            for c in range(C):
                r2 = np.repeat(np.arange(B), out["rank_hist"][c, :, q]) + 2
                assert np.array_equal(np.sort(2 * want["ranks"][c, :, q]), r2)
    for k in ("r_hat_bulk", "r_hat_tail"):
        assert np.all(_r_hat_ok(out[k], want[k], h)), (k, np.flatnonzero(~_r_hat_ok(out[k], want[k], h)))
    dec, dc, exempt = rc.undecided(want, per_chain)
    got_ess = np.stack([out["ess_bulk"], out["ess_tail"], out["ess_median"], *out["ess_quantile"]])
    ref_ess = np.stack([want["ess_bulk"], want["ess_tail"], want["ess_median"], *want["ess_quantile"]])
    ok = _same(got_ess, ref_ess, 1e-10)
    assert np.all(ok | dec), np.argwhere(~(ok | dec))
    if per_chain:
        okb = _same(out["ess_bulk_chain"], want["ess_bulk_chain"], 1e-10) | dc[:, 0]
        okt = _same(out["ess_tail_chain"], want["ess_tail_chain"], 1e-10) | dc[:, 1] | dc[:, 2]
        assert np.all(okb) and np.all(okt), (np.argwhere(~okb), np.argwhere(~okt))
    return int(exempt.sum()), zerr


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 40, tmp_path_factory.mktemp("rank"))
    return pt


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,n,Q", GRID)
def test_host_draws_against_the_reference(handle, C, n, Q, kind):
    x, per_chain, bins = rc.case(C, n, Q, kind)
    out = handle._sampler.rank_convergence(draws=x, probs=PROBS, n_bins=bins, per_chain=per_chain, z=True)
    want = rr.diagnose_all(x, PROBS, bins, per_chain)
    exempt, _ = _check(out, want, per_chain)
    assert exempt <= 1, exempt
    assert out["n_chains"] == C and out["n_draws"] == n and out["z"].shape == (C, 2 * (n // 2), Q)
    if kind == "special" and Q >= 5:
        assert math.isnan(out["r_hat_bulk"][0]) and math.isnan(out["ess_bulk"][0]) and math.isnan(out["ess_tail"][0])
        assert np.all(out["z"][:, :, 0] == 0.0)
        if C > 1:                                                                 # the mean of h equal numbers is exact for h a power of two
            h = n // 2
            assert (out["r_hat_bulk"][1] == math.inf) if h & (h - 1) == 0 else (out["r_hat_bulk"][1] > 1e12)
        for q in (2, 3):
            assert all(math.isnan(out[k][q]) for k in ("r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median"))
            assert np.all(np.isnan(out["ess_quantile"][:, q])) and not out["rank_hist"][:, :, q].any()


def test_z_bound_is_the_measured_one():
    assert 0.0 < Z_BOUND <= 1e-12


def test_outputs_not_asked_for(handle):
    """per_chain, z and probs select outputs only: the others are the same bits."""
    x = rc.draws(7, 101, 65, "ties", 5)
    full = handle._sampler.rank_convergence(draws=x, probs=PROBS, per_chain=True, z=True)
    plain = handle._sampler.rank_convergence(draws=x)
    assert plain["z"] is None and plain["ess_quantile"] is None and plain["ess_bulk_chain"] is None
    for k in ("r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median", "rank_hist"):
        assert np.array_equal(plain[k], full[k], equal_nan=True), k


def test_blocking_changes_nothing(handle, monkeypatch):
    x = rc.draws(7, 101, 65, "ties", 9)
    x[:, :, 3] = rc.draws(7, 101, 1, "special", 2)[:, :, 0]                          # a quantity with a NaN among the blocks
    ref = handle._sampler.rank_convergence(draws=x, probs=PROBS, per_chain=True, z=True)
    for budget in ("1", "200000"):                                               # one quantity per block; a few, the last block short
        monkeypatch.setenv("PTNN_CONVERGENCE_SCRATCH_BYTES", budget)
        got = handle._sampler.rank_convergence(draws=x, probs=PROBS, per_chain=True, z=True)
        for k in ("r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median", "ess_quantile", "ess_bulk_chain", "ess_tail_chain",
                  "rank_hist", "z"):
            assert np.array_equal(ref[k], got[k], equal_nan=True), (budget, k)


@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(orc.TASK_REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 8, 600, tmp_path_factory.mktemp("sun"), schedule=3)
    res = pt.run_chains()
    return pt, res


FIELDS = ("r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median", "ess_bulk_chain", "ess_tail_chain", "rank_hist", "z")


def _equal(a, b):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), k
    assert a.ess_quantile.keys() == b.ess_quantile.keys()
    for p in a.ess_quantile:
        assert np.array_equal(a.ess_quantile[p], b.ess_quantile[p], equal_nan=True), p
    assert (a.n_chains, a.n_draws) == (b.n_chains, b.n_draws)


def test_trace_source_is_the_draws_source(sunspot):
    pt, _ = sunspot
    s, S, P = pt._sampler, 600, pt.num_param
    tr = s.traces(S // 2, S - S // 2)["pos_w"]
    rows = s.trace_rows(S // 2, S - S // 2)
    ci = int(np.argmin(pt.temperatures))

    def host(reps, thin, params, cols):
        return np.concatenate([tr[reps, ::thin][:, :, params]] + [rows[reps, ::thin, c:c + 1] for c in cols], axis=2).astype(np.float32)
    a = pt.rank_diagnostics(probs=PROBS, return_z=True)
    assert a.names == [f"w{p}" for p in range(P)] + ["likelihood"] and a.n_chains == 8 and a.n_draws == 300
    assert a.rank_hist.shape == (8, 20, P + 1) and a.z.shape == (8, 300, P + 1) and sorted(a.ess_quantile) == sorted(PROBS)
    _equal(a, pt.rank_diagnostics(draws=host(list(range(8)), 1, list(range(P)), [0]), probs=PROBS, return_z=True))
    b = pt.rank_diagnostics(chains="cold", per_chain=True, thin=3, params=[0, 3], scalars=("eta", "likelihood"), bins=7)
    assert b.names == ["w0", "w3", "likelihood", "eta"] and b.n_chains == 1 and b.ess_bulk_chain.shape == (1, 4)
    _equal(b, pt.rank_diagnostics(draws=host([ci], 3, [0, 3], [0, 3]), per_chain=True, bins=7))
    # one chain: its own ranks are the pooled ranks
    assert np.array_equal(b.ess_bulk_chain[0], b.ess_bulk, equal_nan=True) and np.array_equal(b.ess_tail_chain[0], b.ess_tail, equal_nan=True)
    want = rr.diagnose_all(host([ci], 3, [0, 3], [0, 3]), (), 7, True)
    assert np.all(_r_hat_ok(b.r_hat_bulk, want["r_hat_bulk"], 50)) and np.array_equal(b.rank_hist, want["rank_hist"])
    from ptnn_amd.parallel_tempering import rank_flagged, rank_uniformity
    assert rank_uniformity(a).shape == (8, P + 1) and set(rank_flagged(a)) <= set(a.names)


def test_no_side_effects(sunspot):
    pt, _ = sunspot
    s = pt._sampler

    def snapshot():
        return s.traces(), s.trace_rows(), s.state(), s.swap_stats()
    before, cd = snapshot(), pt.convergence_diagnostics(per_chain=True, n_lags=5)
    pt.rank_diagnostics(per_chain=True, probs=PROBS, return_z=True)
    after, cd2 = snapshot(), pt.convergence_diagnostics(per_chain=True, n_lags=5)
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    assert np.array_equal(before[1], after[1])
    for k in before[2]:
        assert np.array_equal(before[2][k], after[2][k]), k
    assert before[3] == after[3]
    for k in cd._fields:
        x, y = getattr(cd, k), getattr(cd2, k)
        assert x == y if k in ("names", "n_chains", "n_draws") else np.array_equal(x, y, equal_nan=True), k


def test_refusals(tmp_path):
    from ptnn_amd import _lib
    d = parity.datasets()
    tr, te = d["sunspot_train"], d["sunspot_test"]
    pt = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path)
    with pytest.raises(ValueError, match="run_chains"):
        pt.rank_diagnostics()
    x = rc.draws(4, 50, 3, "ar1", 1)
    assert pt.rank_diagnostics(draws=x).ess_bulk.shape == (3,)                   # draws= works before any run
    s = pt._sampler
    with pytest.raises(_lib.PtnnError, match="at least 4"):
        s.rank_convergence(draws=x[:, :3])
    with pytest.raises(_lib.PtnnError, match=r"n_probs = 17 outside \[0, 16\]"):
        s.rank_convergence(draws=x, probs=[(k + 1) / 20 for k in range(17)])
    with pytest.raises(_lib.PtnnError, match=r"probs\[1\] = 1 must lie in \(0, 1\)"):
        s.rank_convergence(draws=x, probs=[0.5, 1.0])
    for bins in (1, 65):
        with pytest.raises(_lib.PtnnError, match=r"n_bins = \d+ outside \[2, 64\]"):
            s.rank_convergence(draws=x, n_bins=bins)
    with pytest.raises(ValueError, match="17 probs: at most 16"):
        pt.rank_diagnostics(draws=x, probs=[(k + 1) / 20 for k in range(17)])
    with pytest.raises(ValueError, match=r"probs must lie in \(0, 1\)"):
        pt.rank_diagnostics(draws=x, probs=[0.0])
    with pytest.raises(ValueError, match=r"bins = 65 must be an integer in \[2, 64\]"):
        pt.rank_diagnostics(draws=x, bins=65)
    pt.run_chains()
    with pytest.raises(_lib.PtnnError, match="at least 4"):
        s.rank_convergence(step0=100, nsteps=3)
    with pytest.raises(_lib.PtnnError, match="trace range"):
        s.rank_convergence(step0=150, nsteps=100)
    ok = pt.rank_diagnostics()                                                    # the handle is still usable
    assert ok.n_draws == 100 and len(ok.names) == s.P + 1
    sharded = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path)
    sharded._sampler = object()                                                  # what a ladder over several devices holds is no Sampler
    with pytest.raises(ValueError, match="rank_diagnostics runs on one GPU: a ladder sharded over several devices"):
        sharded.rank_diagnostics(draws=x)
    ls = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, label_swap=True)
    ls.run_chains()
    with pytest.raises(ValueError, match="label_swap=True.*pass draws="):
        ls.rank_diagnostics()
    assert ls.rank_diagnostics(draws=x).n_chains == 4
    st = _pt(orc.TASK_REG, (4, 5, 1), tr, te, 4, 200, tmp_path, trace_capacity=64)
    st.run_chains()
    with pytest.raises(ValueError, match="trace_capacity = 64.*pass draws="):
        st.rank_diagnostics()
    assert st.rank_diagnostics(draws=x).n_draws == 50
