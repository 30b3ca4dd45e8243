"""Case influence on the GPU (ptnn_influence / case_influence), against tests/influence_ref.py:
1. the reduction alone, on the device's own numbers (posterior_predictive(..., return_samples=True) on the target rows and
   predictive_accuracy(..., return_pointwise=True) on the case rows of the same selection), at regression (4,5,1) and the
   classification shapes of tests/report_cases.py with the fewest and the most outputs, both `of` kinds;
2. the tie to WAIC; 3. an exact-integer known answer through the host matrices, over the tile, chunk and sample edges;
4. one multiset, one result (trace, expanded vectors, (distinct, multiplicity), any block size); 5. the edges; 6. nothing is
   disturbed.

The bound, derived and not measured: with exact inputs, a two-pass centred float64 sum of U weighted
products in any order errs by at most tol(a, b) = 16 (U + 64) 2^-53 s_a s_b, s the expanded ddof-1 standard deviations: at most 4
roundings per term, U 2^-53 from the sum, sum m |a| |b| <= (M - 1) s_a s_b by Cauchy-Schwarz, an inexact mean enters at second
order, and the factor 16 leaves about 3 x.  The reference in the bound checks is the np.longdouble variant, so the whole bound
is the device's.  A weighted mean of U values gets 16 (U + 64) 2^-53 max(s, |mean|) by the same count.  The largest deviation
seen is printed as a share of the bound."""
import itertools
import warnings

import numpy as np
import pytest

import influence_ref as ref
import parity
import uncertainty_cases as cases
from parity import orc
from test_gpu_elpd import _runs as _runs_eta
from test_gpu_predict import _pt

pytestmark = pytest.mark.gpu

CLS, REG = orc.TASK_CLS, orc.TASK_REG
KCHUNK = 512                            # INFL_KCHUNK of csrc/ptnn_dev_influence.hpp
FIELDS = ("cov", "corr", "deletion_shift", "deletion_z", "target_mean", "target_sd", "case_loglik_mean", "case_loglik_var", "top_cases",
          "top_shift", "case_importance")


def _make(task, topo, tmp_path, train, test):
    kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
    return _pt(task, topo, np.array(train), np.array(test), 4, 20, tmp_path, **kw)


def _same(a, b):
    assert (a.n_samples, a.n_distinct) == (b.n_samples, b.n_distinct)
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=name in ("corr", "deletion_z", "case_importance")), name


def _accuracy(pt, data, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # high k-hat rows: not this test's subject
        return pt.predictive_accuracy(data, return_pointwise=True, **kw)


def _share(got, want, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(got - np.asarray(want, dtype=np.float64)) / bound
    return float(np.max(np.where(bound > 0, s, np.where(got == want, 0.0, np.inf))))


def _check(ci, A, B, U, name):
    """A result against the longdouble reference on the expanded sample matrices A [S, n_a] and B [S, n_b]; -> the reference."""
    r = ref.influence_longdouble(A, B)
    s_a, s_b = np.sqrt(r["target_var"].astype(np.float64)), np.sqrt(r["case_var"].astype(np.float64))
    n_b = B.shape[1]
    shares = dict(cov=_share(ci.cov.reshape(-1, n_b), r["cov"], ref.tol(U, s_a, s_b)),
                  target_var=_share(ci.target_sd.ravel() ** 2, r["target_var"], np.diag(ref.tol(U, s_a, s_a))),
                  case_var=_share(ci.case_loglik_var, r["case_var"], np.diag(ref.tol(U, s_b, s_b))),
                  case_mean=_share(ci.case_loglik_mean, r["case_mean"], 16 * (U + 64) * 2.0 ** -53 * np.maximum(s_b, np.abs(ci.case_loglik_mean))))
    for k, v in shares.items():
        print(f"{name}: largest deviation of {k} as a share of its bound: {v:.3g}")
    assert max(shares.values()) <= 1.0, shares
    assert ci.n_samples == A.shape[0] == r["n_samples"]
    return r, s_a, s_b


# ---- 1: the reduction alone, on the device's own numbers
GRID = [(REG, (4, 5, 1)), (CLS, min(cases.CLS_SHAPES, key=lambda t: t[2])), (CLS, max(cases.CLS_SHAPES, key=lambda t: t[2]))]


@pytest.fixture(scope="module", params=GRID, ids=["-".join(map(str, t)) for _, t in GRID])
def grid(request, tmp_path_factory):
    task, topo = request.param
    if task == REG:
        train, test, W, eta, _ = cases.regression_case(topo)
    else:
        train, test, W, _ = cases.report_cases.case(topo)
        eta = None
    pt = _make(task, topo, tmp_path_factory.mktemp("grid"), train, test)
    mult = cases.multiplicities(len(W))
    src = dict(weights=(W, mult), eta=eta)
    pred = pt.posterior_predictive("test", weights=(W, mult), return_samples=True)
    return dict(task=task, topo=topo, pt=pt, src=src, mult=mult, pred=pred, ll_train=_accuracy(pt, "train", **src), ll_test=_accuracy(pt, "test", **src))


def test_prediction_targets_on_the_devices_own_numbers(grid, monkeypatch):
    g = grid
    pt, pred, O = g["pt"], g["pred"], g["topo"][2]
    ci = pt.case_influence("test", "train", **g["src"])
    S, N = pred.samples.shape[:2]
    n_b = g["ll_train"].log_lik.shape[1]
    assert ci.n_distinct == 65 and ci.n_samples == S == int(g["mult"].sum()) and ci.cov.shape == (N, O, n_b) and ci.top_cases.shape == (N, O, 5)
    A = pred.samples.reshape(S, N * O).astype(np.float64)                 # column n * O + o, as the device orders them
    r, s_a, s_b = _check(ci, A, g["ll_train"].log_lik, ci.n_distinct, f"{g['topo']} prediction")
    mean_share = _share(ci.target_mean.ravel(), pred.mean.ravel(), 16 * (ci.n_distinct + 64) * 2.0 ** -53 * s_a)
    print(f"{g['topo']} prediction: largest |target_mean - predictive mean| as a share of its bound: {mean_share:.3g}")
    assert mean_share <= 1.0
    # the host side: float64 arithmetic on the device's matrix
    assert np.array_equal(ci.deletion_shift, 0.0 - ci.cov) and np.array_equal(ci.top_cases, ref.top_cases(ci.cov, 5))
    assert np.array_equal(ci.corr, ci.cov / (ci.target_sd[..., None] * np.sqrt(ci.case_loglik_var)))
    # row blocks of any size change no bit
    whole = N * O * ci.n_distinct * 12
    for budget in (whole // 3, 1):
        monkeypatch.setenv("PTNN_INFLUENCE_SCRATCH_BYTES", str(budget))
        _same(ci, pt.case_influence("test", "train", **g["src"]))


def test_loglik_targets_on_the_devices_own_numbers(grid):
    g = grid
    ci = g["pt"].case_influence("test", "train", of="loglik", **g["src"])
    N, n_b = g["ll_test"].log_lik.shape[1], g["ll_train"].log_lik.shape[1]
    assert ci.cov.shape == (N, n_b) and ci.target_sd.shape == (N,) and ci.n_distinct == 65
    _check(ci, g["ll_test"].log_lik, g["ll_train"].log_lik, ci.n_distinct, f"{g['topo']} loglik")
    # the low-level call leaves out what is not asked for
    W, mult = g["src"]["weights"]
    low = g["pt"]._sampler.influence("test", "train", of="loglik", w=W, eta=g["src"]["eta"], multiplicity=mult, cov=False)
    assert low["cov"] is None and np.array_equal(low["case_var"], ci.case_loglik_var) and np.array_equal(low["target_mean"], ci.target_mean)


# ---- 2: the tie to WAIC
def test_the_diagonal_is_the_waic_penalty(grid):
    g = grid
    ci = g["pt"].case_influence("train", "train", of="loglik", **g["src"])
    acc = g["ll_train"]
    r = ref.influence_longdouble(acc.log_lik, acc.log_lik)
    s_b = np.sqrt(r["case_var"].astype(np.float64))
    bound = ref.tol(ci.n_distinct, s_b, s_b)
    d = np.diag(bound)
    shares = dict(diag_vs_var=_share(np.diag(ci.cov), ci.case_loglik_var, d), diag_vs_p_waic=_share(np.diag(ci.cov), acc.p_waic_i, d),
                  var_vs_p_waic=_share(ci.case_loglik_var, acc.p_waic_i, d), symmetry=_share(ci.cov, ci.cov.T, bound))
    print(f"{g['topo']}: {shares}")
    assert max(shares.values()) <= 1.0
    assert np.array_equal(ci.target_sd, np.sqrt(ci.case_loglik_var)) and np.array_equal(ci.target_mean, ci.case_loglik_mean)


# ---- 3: an exact-integer known answer through the host matrices
N_A, N_B = (1, 63, 64, 65), (1, 63, 64, 65, 129)
N_U = (2, 63, 64, 65, KCHUNK - 1, KCHUNK, KCHUNK + 1, 2 * KCHUNK + 3)


def _pairwise(*axes):
    """A subset of the product of `axes` in which every pair of values of two axes occurs: greedy, in product order."""
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(axes)), 2) for a in axes[i] for b in axes[j]}
    picked = []
    while need:
        best = max(itertools.product(*axes), key=lambda c: sum((i, c[i], j, c[j]) in need for i, j in itertools.combinations(range(len(c)), 2)))
        picked.append(best)
        need -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(best)), 2)}
    return picked


SIZES = _pairwise(N_A, N_B, N_U)


def _integers(n_a, n_b, U, identity, seed):
    """Sample matrices whose every mean, centred value, product and sum is an integer: h = U // 2 base samples with entries in
    [-8, 8], each mirrored as its negation with the same multiplicity (0..3; entry 1 and its mirror 0 when h >= 2), a sample of
    zeros when U is odd, and integer column offsets in [-100, 100].  -> (values float32, loglik float64, mult, A0, B0)."""
    rng = np.random.default_rng(seed)
    h = U // 2
    u = np.arange(h)
    if identity:                                                          # a shifted identity pattern: sample u lights column u + 1
        A0 = np.where((u[:, None] + 1) % n_a == np.arange(n_a)[None, :], 8, 0).astype(np.int64)
    else:
        A0 = rng.integers(-8, 9, (h, n_a))
    B0 = ((3 * u[:, None] + 5 * np.arange(n_b)[None, :]) % 17 - 8).astype(np.int64)           # visibly not symmetric
    B0[rng.random((h, n_b)) < 0.25] = 7
    m = rng.integers(0, 4, h)
    m[0] = max(m[0], 1)
    if h >= 2:
        m[1] = 0
    A0 = np.concatenate([A0, -A0] + ([np.zeros((1, n_a), np.int64)] if U % 2 else []))
    B0 = np.concatenate([B0, -B0] + ([np.zeros((1, n_b), np.int64)] if U % 2 else []))
    mult = np.concatenate([m, m] + ([[2]] if U % 2 else [])).astype(np.int32)
    off_a, off_b = rng.integers(-100, 101, n_a), rng.integers(-100, 101, n_b)
    return (A0 + off_a).astype(np.float32), (B0 + off_b).astype(np.float64), mult, A0, B0


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    return _make(REG, (4, 5, 1), tmp_path_factory.mktemp("handle"), train, test)


@pytest.mark.parametrize("n_a, n_b, U", SIZES, ids=lambda v: str(v))
def test_exact_integer_known_answer(handle, monkeypatch, n_a, n_b, U):
    k = SIZES.index((n_a, n_b, U))
    values, loglik, mult, A0, B0 = _integers(n_a, n_b, U, identity=k % 2 == 1, seed=100 + k)
    M = int(mult.sum())
    assert values.shape == (U, n_a) and loglik.shape == (U, n_b) and M >= 2
    want = ((A0 * mult[:, None]).T @ B0).astype(np.float64) / (M - 1)
    want_va = ((A0 * A0) * mult[:, None]).sum(axis=0).astype(np.float64) / (M - 1)
    want_vb = ((B0 * B0) * mult[:, None]).sum(axis=0).astype(np.float64) / (M - 1)
    assert np.abs(want).max() > 0 and (n_a != n_b or n_a == 1 or not np.array_equal(want, want.T))
    budgets = [None] + ([4 * max(n_a, n_b) * U * 8] if U <= 65 else [])    # the second: whole blocks, one tile per launch
    for budget in budgets:
        if budget is not None:
            monkeypatch.setenv("PTNN_INFLUENCE_SCRATCH_BYTES", str(budget))
        out = handle._sampler.influence(values=values, loglik=loglik, multiplicity=mult)
        assert out["n_samples"] == M and out["n_distinct"] == U
        assert np.array_equal(out["cov"], want), (np.argwhere(out["cov"] != want)[:5], budget)
        assert np.array_equal(out["target_var"], want_va) and np.array_equal(out["case_var"], want_vb)
        assert np.array_equal(out["target_mean"], (values[0] - A0[0]).astype(np.float64))
        assert np.array_equal(out["case_mean"], loglik[0] - B0[0])


def test_the_size_table_covers_every_pair():
    for i, j in itertools.combinations(range(3), 2):
        axes = (N_A, N_B, N_U)
        assert {(c[i], c[j]) for c in SIZES} == set(itertools.product(axes[i], axes[j]))
    assert len(SIZES) <= 60


# ---- 4: one multiset, one result
@pytest.fixture(scope="module")
def sunspot(tmp_path_factory):
    d = parity.datasets()
    pt = _pt(REG, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], 4, 400, tmp_path_factory.mktemp("sun"))
    res = pt.run_chains()
    return pt, res, d, pt._sampler.eta_trace()


def test_one_multiset_one_result(sunspot, monkeypatch):
    pt, res, d, et = sunspot
    R, S = 4, 400
    eta = et[:, S // 2:].reshape(-1)                                     # chain-major, as the columns of res[0]
    x, cs = d["sunspot_test"][:37], d["sunspot_train"][:70]
    for of in ("prediction", "loglik"):
        base = pt.case_influence(x, cs, of=of)
        assert base.n_samples == R * (S - S // 2) and 1 < base.n_distinct < base.n_samples
        wd, ed, counts = _runs_eta(res[0].T, eta)
        assert len(wd) == base.n_distinct
        sources = ({}, dict(weights=res[0].T, eta=eta), dict(weights=(wd, counts), eta=ed))
        for src in sources[1:]:
            _same(base, pt.case_influence(x, cs, of=of, **src))
        monkeypatch.setenv("PTNN_INFLUENCE_SCRATCH_BYTES", str(37 * base.n_distinct * 12 // 3))
        for src in sources:
            _same(base, pt.case_influence(x, cs, of=of, **src))
        monkeypatch.setenv("PTNN_INFLUENCE_SCRATCH_BYTES", "1")          # every block holds one row
        small = pt.case_influence(x[:5], cs[:9], of=of)
        monkeypatch.delenv("PTNN_INFLUENCE_SCRATCH_BYTES")
        whole = pt.case_influence(x[:5], cs[:9], of=of)
        _same(small, whole)
        assert np.array_equal(whole.cov, base.cov[:5, ..., :9])          # an element's bits depend on its two columns only
    # the device's own numbers of the trace selection, and the named row sets
    ci = pt.case_influence("test", "train")
    pred = pt.posterior_predictive("test", return_samples=True)
    acc = _accuracy(pt, "train")
    _check(ci, pred.samples.reshape(pred.samples.shape[0], -1).astype(np.float64), acc.log_lik, ci.n_distinct, "sunspot trace")
    cold = pt.case_influence("test", "train", chains="cold", thin=3)
    assert cold.n_samples == -(-(S - S // 2) // 3) and cold.cov.shape == (198, 1, 298)


# ---- 5: the edges
def test_constant_columns_two_samples_and_ties(handle):
    pt = handle
    rng = np.random.default_rng(3)
    values = rng.standard_normal((40, 3)).astype(np.float32)
    values[:, 1] = np.float32(0.1)                                        # a constant target column
    loglik = rng.standard_normal((40, 6)) - 3.0
    loglik[:, 4] = loglik[:, 2]                                           # two cases with equal columns: equal |cov|
    loglik[:, 5] = -2.5                                                   # a constant case
    ci = pt.case_influence(values=values, loglik=(loglik, rng.integers(1, 4, 40)), top=9)
    assert (ci.cov[1] == 0.0).all() and ci.target_sd[1] == 0.0 and ci.target_mean[1] == np.float64(np.float32(0.1))
    assert np.isnan(ci.corr[1]).all() and np.isnan(ci.deletion_z[1]).all() and np.isfinite(ci.corr[[0, 2]][:, :5]).all()
    assert (ci.cov[:, 5] == 0.0).all() and ci.case_loglik_var[5] == 0.0 and np.isnan(ci.corr[:, 5]).all() and np.isnan(ci.case_importance[5])
    assert np.array_equal(ci.cov[:, 4], ci.cov[:, 2])
    assert ci.top_cases.shape == (3, 6)                                   # top = 9 clipped to the six cases
    assert np.array_equal(ci.top_cases, ref.top_cases(ci.cov, 9)) and ci.top_cases[1].tolist() == [0, 1, 2, 3, 4, 5]
    for row in ci.top_cases[[0, 2]]:
        assert list(row).index(2) + 1 == list(row).index(4)              # the tie: the lower index first
    # a network whose output does not depend on the sample: two zero vectors with different eta
    train, test, W, eta, _ = cases.regression_case((4, 5, 1))
    zero = pt.case_influence("test", "train", weights=np.zeros((2, W.shape[1]), np.float32), eta=eta[:2])
    assert zero.n_distinct == 2 and (zero.cov == 0.0).all() and (zero.target_sd == 0.0).all() and np.isnan(zero.corr).all()
    assert (zero.case_loglik_var > 0).all()
    # M = 2 works, by distinct samples or by one sample twice; M = 1 is refused
    two = pt.case_influence("test", "train", weights=W[:2], eta=eta[:2])
    pred = pt.posterior_predictive("test", weights=W[:2], return_samples=True)
    _check(two, pred.samples.reshape(2, -1).astype(np.float64), _accuracy(pt, "train", weights=W[:2], eta=eta[:2]).log_lik, 2, "M = 2")
    twice = pt.case_influence("test", "train", weights=(W[:1], [2]), eta=eta[:1])
    assert twice.n_samples == 2 and twice.n_distinct == 1 and (twice.cov == 0.0).all()
    from ptnn_amd import _lib
    with pytest.raises(_lib.PtnnError, match="holds 1 samples: a covariance"):
        pt._sampler.influence("test", "train", w=W[:1], eta=eta[:1])
    with pytest.raises(_lib.PtnnError, match="holds 1 samples: a covariance"):
        pt._sampler.influence(values=values[:3], loglik=loglik[:3], multiplicity=[0, 1, 0])
    with pytest.raises(ValueError, match="holds 1 samples"):
        pt.case_influence("test", "train", weights=W[:1], eta=eta[:1])
    with pytest.raises(_lib.PtnnError, match="a regression's host vectors need eta"):
        pt._sampler.influence("test", "train", w=W[:3])


# ---- 6: nothing is disturbed
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
            e = pt._sampler.trace_rows(60, 100)[:, :, 3].reshape(-1) if task == REG else None
            ci = pt.case_influence("test", "train", weights=w, eta=e)
            assert ci.n_samples == 800
            low = pt._sampler.influence("train", "test", of="loglik", step0=100, nsteps=60, thin=2)
            assert low["n_samples"] == 240 and np.isfinite(low["cov"]).all()
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
