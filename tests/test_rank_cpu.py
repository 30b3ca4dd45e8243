"""The rank-normalised convergence diagnostics without a GPU: the float64 reference tests/rank_ref.py against brute force and
against the properties that define it, the host helpers rank_uniformity and rank_flagged, and rank_diagnostics' refusals that
need no handle."""
import ctypes as C
import math
import os
from statistics import NormalDist

import numpy as np
import pytest

import rank_cases as rc
import rank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ar1(C, n, phi, seed):
    rng = np.random.default_rng(seed)
    y = np.empty((C, n))
    y[:, 0] = rng.standard_normal(C) / math.sqrt(1 - phi * phi)
    e = rng.standard_normal((C, n))
    for i in range(1, n):
        y[:, i] = phi * y[:, i - 1] + e[:, i]
    return y


@pytest.mark.parametrize("seed", range(4))
def test_average_ranks_against_a_count(seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-3, 4, size=57).astype(np.float32) * 0.5                     # many ties, and zeros of both signs
    v[5], v[6] = -0.0, 0.0
    less = (v[None, :] < v[:, None]).sum(axis=1)
    equal = (v[None, :] == v[:, None]).sum(axis=1)
    brute = less + (equal + 1) / 2.0                                              # the mean of the ranks less + 1 .. less + equal
    r = rr.average_ranks(v)
    assert np.array_equal(r, brute)
    assert np.array_equal(2 * r, np.rint(2 * r)) and r.sum() == v.size * (v.size + 1) / 2
    p = rng.permutation(60)
    assert np.array_equal(rr.average_ranks(p.astype(np.float64)), p + 1.0)        # no ties: the ranks themselves


def test_z_scores_are_the_normal_quantiles():
    S = 40
    z = rr.z_scores(np.arange(1, S + 1), S)
    assert np.all(np.diff(z) > 0) and np.allclose(z, -z[::-1], rtol=0, atol=1e-15)
    assert z[0] == NormalDist().inv_cdf(0.625 / 40.25)
    assert rr.z_scores(np.array([(S + 1) / 2]), S)[0] == 0.0                       # the rank every draw gets when all are equal


@pytest.mark.parametrize("name,f", [("exp", np.exp), ("cube", lambda v: v ** 3)])
def test_invariant_under_an_increasing_map(name, f):
    """Bulk figures depend on the draws through their ranks only.  Draws on a coarse grid of fp32 values whose images are distinct
    fp32 values where the originals are; the folded figures need the map to keep the order of |x - med| too, which an increasing
    map does not: they are compared under the affine map 2x + 1, exact in fp32."""
    x = np.round(_ar1(4, 200, 0.7, 3) * 64) / 64                                   # |x| < 8, multiples of 2^-6: ties occur
    x32 = x.astype(np.float32)
    y32 = f(x.astype(np.float64)).astype(np.float32)
    assert np.unique(x32).size == np.unique(y32).size
    a, b = rr.diagnose(x32, probs=(0.25,)), rr.diagnose(y32, probs=(0.25,))
    for k in ("r_hat_bulk", "ess_bulk", "ess_tail", "ess_median", "ess_quantile", "rank_hist", "z"):
        assert np.array_equal(a[k], b[k]), k
    c = rr.diagnose((2 * x32 + 1).astype(np.float32))
    for k in ("r_hat_bulk", "r_hat_tail", "r_hat", "ess_bulk", "ess_tail", "rank_hist"):
        assert np.array_equal(a[k], c[k]), k


def test_cauchy_draws_have_finite_figures():
    x = np.random.default_rng(5).standard_cauchy((4, 500)).astype(np.float32)
    d = rr.diagnose(x, per_chain=True)
    for k in ("r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median"):
        assert math.isfinite(d[k]), k
    assert d["r_hat"] < 1.02 and d["ess_bulk"] > 1000 and d["ess_tail"] > 500
    assert np.all(np.isfinite(d["ess_bulk_chain"])) and np.all(np.isfinite(d["ess_tail_chain"]))


def test_scale_differences_show_in_the_tail_r_hat():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((4, 1000)) * np.array([1.0, 1.0, 3.0, 3.0])[:, None]).astype(np.float32)
    d = rr.diagnose(x)
    assert d["r_hat_bulk"] < 1.01 and d["r_hat_tail"] > 1.1 and d["r_hat"] == d["r_hat_tail"]
    import convergence_ref as cr
    assert cr.diagnose(x)["r_hat"] < 1.01                                          # the classic figure does not see it


def test_degenerate_quantities():
    nan = math.nan
    const = rr.diagnose(np.full((3, 9), 1.25, np.float32), probs=(0.3,), per_chain=True)
    assert np.all(const["z"] == 0.0)
    for k in ("r_hat_bulk", "r_hat_tail", "r_hat", "ess_bulk", "ess_tail", "ess_median"):
        assert math.isnan(const[k]), k
    assert np.all(np.isnan(const["ess_quantile"])) and np.all(np.isnan(const["ess_bulk_chain"])) and np.all(np.isnan(const["ess_tail_chain"]))
    # constant split chains that differ: W = 0 exactly where the chain means are (two draws per split chain), R-hat = +inf
    chain = rr.diagnose((np.arange(64)[:, None] * 0.5 * np.ones((64, 4))).astype(np.float32))
    assert chain["r_hat_bulk"] == math.inf and chain["r_hat_tail"] == math.inf and chain["r_hat"] == math.inf
    assert math.isfinite(chain["ess_bulk"])
    # an indicator that is constant: every draw is <= the largest
    two = rr.diagnose(np.array([[0, 1, 0, 1, 0, 0, 1, 1]], np.float32))            # x_(lo) of p = 0.95 is 1
    assert math.isnan(two["ess_tail"]) and math.isfinite(two["ess_median"])
    for bad in (nan, math.inf, -math.inf):
        x = _ar1(2, 9, 0.3, 1).astype(np.float32)
        x[1, 4] = bad                                                             # the middle draw, which the split drops
        d = rr.diagnose(x, probs=(0.3,), bins=7, per_chain=True)
        for k in ("r_hat_bulk", "r_hat_tail", "r_hat", "ess_bulk", "ess_tail", "ess_median"):
            assert math.isnan(d[k]), k
        assert not d["rank_hist"].any() and d["rank_hist"].shape == (2, 7) and np.all(np.isnan(d["z"]))
        assert np.all(np.isnan(d["ess_bulk_chain"])) and np.all(np.isnan(d["ess_tail_chain"]))


@pytest.mark.parametrize("C,n,bins", [(3, 11, 20), (2, 40, 7), (5, 8, 64), (1, 4, 2)])
def test_histogram_rows_and_bins(C, n, bins):
    x = np.round(_ar1(C, n, 0.5, C + n) * 2).astype(np.float32)                    # ties
    d = rr.diagnose(x, bins=bins)
    h, S = n // 2, 2 * C * (n // 2)
    assert d["rank_hist"].shape == (C, bins) and np.all(d["rank_hist"].sum(axis=1) == 2 * h)
    r = d["ranks"]
    for c in range(C):
        want = np.zeros(bins, np.int64)
        for v in r[c]:
            want[int((2 * v - 2) * bins) // (2 * S)] += 1
        assert np.array_equal(d["rank_hist"][c], want)
    assert d["rank_hist"][:, 0].sum() >= 1 and ((2 * S - 2) * bins) // (2 * S) == min(bins - 1, ((S - 1) * bins) // S)   # ranks 1 and S


def test_folded_ties_rank_equal():
    x = np.array([[-3, -1, 1, 3, -2, 2, 0.5, -0.5]], np.float32)                    # symmetric about 0: pairs of equal |x - med|
    f = rr.folded(rr.keep(x))
    r = rr.average_ranks(f)
    assert np.array_equal(np.sort(r), [1.5, 1.5, 3.5, 3.5, 5.5, 5.5, 7.5, 7.5])


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("C,n,Q", rc.GRID)
def test_the_seeds_leave_no_truncation_within_rounding(C, n, Q, kind):
    """What tests/test_gpu_rank.py relies on, from the reference alone: on every case of its grid at most one quantity has a pair
    sum under 1e-9 deciding a truncation, and no other quantity's truncation moves when the z-scores change by one part in 10^13
    (scaled up, scaled down, and every draw up or down at random), 100 times what the device may differ by.  The indicator series
    are exact 0 / 1 on either side and need no such check."""
    x, per_chain, bins = rc.case(C, n, Q, kind)
    want = rr.diagnose_all(x, rc.PROBS, bins, per_chain)
    _, _, exempt = rc.undecided(want, per_chain)
    assert exempt.sum() <= 1, np.flatnonzero(exempt)
    sign = np.random.default_rng(C + n + Q).choice([-1.0, 1.0], size=want["z"].shape[:2])
    factors = (1 + 1e-13, 1 - 1e-13, 1 + 1e-13 * sign)
    for q in np.flatnonzero(~exempt & ~np.isnan(want["z"]).any(axis=(0, 1))):
        zs = [want["z"][:, :, q]] + ([want["z_chain"][c:c + 1, :, q] for c in range(C)] if per_chain else [])
        for z in zs:
            lag = rr.trunc_lag(z)
            assert all(rr.trunc_lag(z * (f if np.ndim(f) == 0 else f[:z.shape[0]])) == lag for f in factors), (q, lag)


def _result(**kw):
    from ptnn_amd.parallel_tempering import RankConvergence
    base = dict(names=["a", "b", "c"], r_hat=np.array([1.0, 1.0, 1.0]), r_hat_bulk=None, r_hat_tail=None, ess_bulk=np.array([900.0] * 3),
                ess_tail=np.array([900.0] * 3), ess_median=None, ess_quantile={}, ess_bulk_chain=None, ess_tail_chain=None,
                rank_hist=np.full((4, 5, 3), 10, np.int64), z=None, n_chains=4, n_draws=25)
    base.update(kw)
    return RankConvergence(**base)


def test_rank_flagged():
    from ptnn_amd.parallel_tempering import rank_flagged
    assert rank_flagged(_result()) == []
    assert rank_flagged(_result(r_hat=np.array([1.0, 1.011, math.nan]))) == ["b", "c"]
    assert rank_flagged(_result(ess_bulk=np.array([399.0, 400.0, 900.0]))) == ["a"]
    assert rank_flagged(_result(ess_tail=np.array([900.0, math.nan, 399.9]))) == ["b", "c"]
    assert rank_flagged(_result(ess_bulk=np.array([math.nan, 500.0, 900.0])), ess_per_chain=200) == ["a", "b"]
    assert rank_flagged(_result(r_hat=np.array([1.04, 1.06, 1.0])), r_hat=1.05) == ["b"]


def test_rank_uniformity():
    from ptnn_amd.parallel_tempering import rank_uniformity
    hist = np.full((2, 4, 3), 5, np.int64)
    hist[1, :, 1] = [20, 0, 0, 0]
    hist[:, :, 2] = 0                                                             # a quantity with a draw that is not finite
    u = rank_uniformity(_result(rank_hist=hist))
    assert u.shape == (2, 3) and u[0, 0] == 0.0 and u[1, 0] == 0.0
    assert u[1, 1] == (15 ** 2 + 3 * 5 ** 2) / 5 and np.all(np.isnan(u[:, 2]))


def test_names_are_exported_and_the_library_has_the_call():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    from ptnn_amd import _lib, parallel_tempering as pt
    assert pt.RankConvergence._fields == ("names", "r_hat", "r_hat_bulk", "r_hat_tail", "ess_bulk", "ess_tail", "ess_median", "ess_quantile",
                                          "ess_bulk_chain", "ess_tail_chain", "rank_hist", "z", "n_chains", "n_draws")
    assert callable(pt.rank_uniformity) and callable(pt.rank_flagged) and callable(pt.ParallelTemperingBase.rank_diagnostics)
    lib = ptnn_amd.load_library()
    assert lib.ptnn_rank_convergence is not None and "ptnn_rank_convergence" in _lib.SYMBOLS and lib.ptnn_abi_version() == 4
    # the struct of include/ptnn.h on LP64: the trace source (48 bytes), the host source (24), probs and bins (16), ten outputs
    assert C.sizeof(_lib.RankConvergenceSpec) == 48 + 24 + 16 + 80
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    assert "PTNN_RANK_MAX_PROBS 16" in header and "PTNN_RANK_MAX_BINS 64" in header
    assert (_lib.RANK_MAX_PROBS, _lib.RANK_MAX_BINS) == (16, 64)


def _object(**kw):
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    t = (np.arange(30 * 5) % 17 / 17.0).reshape(30, 5)
    pt = ParallelTempering(True, 0.01, t, t[:20], [4, 5, 1], 4, 4.0, 160, 5, 0.5, "unused", seed=11, write_files=False, **kw)
    pt._finished, pt.burn_in, pt.temperatures = True, 0.25, [2.0, 1.0, 4.0, 1.5]    # as after a finished run
    return pt


class _Refuses:
    """A handle that must not be reached."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal should precede Sampler.{name}")


def test_refusals_that_need_no_handle():
    from ptnn_amd import _lib
    pt = _object()
    with pytest.raises(ValueError, match=r"rank_diagnostics needs the chains' device handle"):
        pt.rank_diagnostics()
    pt._sampler = object()
    with pytest.raises(ValueError, match="rank_diagnostics runs on one GPU: a ladder sharded"):
        pt.rank_diagnostics()
    pt._sampler = object.__new__(_lib.Sampler)
    pt._sampler.__class__ = type("S", (_lib.Sampler,), {"__getattr__": _Refuses.__getattr__, "close": lambda self: None})
    with pytest.raises(ValueError, match=r"draws must be \[n_chains, n_draws, n_quantities\]"):
        pt.rank_diagnostics(draws=np.zeros((3, 8)))
    d = np.zeros((3, 8, 2))
    with pytest.raises(ValueError, match="17 probs: at most 16"):
        pt.rank_diagnostics(draws=d, probs=[(k + 1) / 20 for k in range(17)])
    for bad in ([0.0], [1.0], [0.5, 1.5], [math.nan]):
        with pytest.raises(ValueError, match=r"probs must lie in \(0, 1\)"):
            pt.rank_diagnostics(draws=d, probs=bad)
    for bad in (1, 65, 0, 2.5):
        with pytest.raises(ValueError, match=r"bins = .* must be an integer in \[2, 64\]"):
            pt.rank_diagnostics(draws=d, bins=bad)
    with pytest.raises(ValueError, match="chains"):
        pt.rank_diagnostics(chains=[4])
    with pytest.raises(ValueError, match="params: weight indices"):
        pt.rank_diagnostics(params=[31])
    with pytest.raises(ValueError, match="scalar 'acc_train'"):
        pt.rank_diagnostics(scalars=("acc_train",))
    with pytest.raises(ValueError, match="no quantity selected"):
        pt.rank_diagnostics(params=[], scalars=())
    for kw, text in ((dict(label_swap=True), "label_swap=True.*pass draws="), (dict(trace_capacity=5), "trace_capacity = 5.*pass draws=")):
        other = _object(**kw)
        other._sampler = pt._sampler
        with pytest.raises(ValueError, match=text):
            other.rank_diagnostics()
