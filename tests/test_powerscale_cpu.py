"""Power-scaling sensitivity without a GPU: the float64 oracle (tests/powerscale_ref.py) on two known-answer cases, and the
pure-Python helpers of powerscale_sensitivity (names, groups, diagnosis, flagging, refusals)."""
import math

import numpy as np
import pytest

import powerscale_ref as ref
from ptnn_amd.parallel_tempering import (PowerScaling, TASK_CLS, TASK_REG, powerscale_check_delta, powerscale_diagnosis,
                                         powerscale_flagged, powerscale_groups, powerscale_names)

# |D - QUADRATURE_D| of the oracle over seeds 0 .. 5 at n_w = 20 000 (measured on the CPU): P = 4
# (net 1-1-1): 0.0389, 0.0374, 0.0396, 0.0363, 0.0399, 0.0390.  The margin is twice the largest.
QUADRATURE_MARGIN_P4 = 2 * 0.0399
# That value integrates over +-12 sigma and the normalised distance depends on the range (+-4 sigma gives 0.0772), so the margin
# above cannot fail for a plausible error.  The sharp check takes the same quadrature over each coordinate's own sample range
# [min w_p, max w_p] (powerscale_ref.quadrature_sensitivity).  Largest |D - quadrature| over the coordinates, oracle, seeds
# 0 .. 5 at n_w = 20 000, P = 4: 0.00448, 0.00340, 0.00306, 0.00247, 0.00289, 0.00137.  The margin is twice the largest:
# 12 % of D, which a wrong normaliser, log base (x 1.44) or scale does not fit in.
RANGE_MARGIN_P4 = 2 * 0.00448


def test_sign_flips_give_exact_zero():
    """Vectors that differ by the signs of their entries have bit-equal sum w^2, so every prior log ratio is equal: the cut is
    the common value, no sample lies above it (T = 0 <= 4: the tail rule, not the fit, gives khat = +inf), the weights stay
    uniform and every distance is exactly 0."""
    rng = np.random.default_rng(3)
    w0 = rng.normal(0, 2, 31).astype(np.float32)
    signs = rng.choice(np.array([-1.0, 1.0], np.float32), (500, 31))
    w = (signs * w0[None, :]).astype(np.float32)
    eta = np.full(500, -1.5, np.float32)
    pr = ref.prior_component(0, w, eta, (4, 5, 1))
    assert np.all(pr == pr[0])
    counts = rng.integers(1, 4, 500)
    lik = rng.normal(-50, 3, 500)
    r = ref.powerscale(w.T, np.stack([lik, pr]), counts)
    assert np.all(r["sens"][1] == 0.0) and np.all(r["dist"][1] == 0.0)
    assert np.all(np.isinf(r["khat"][1])) and np.all(r["tail_len"][1] == 0)
    assert np.array_equal(r["q"][1, 0], counts / counts.sum()) and np.array_equal(r["q"][1, 1], counts / counts.sum())
    assert np.array_equal(r["mean"][1, 0], r["base_mean"]) and np.array_equal(r["sd"][1, 1], r["base_sd"])
    assert np.all(r["sens"][0] > 0.0) and np.all(np.isfinite(r["khat"][0]))     # the likelihood does move them


@pytest.mark.parametrize("seed", range(6))
def test_gaussian_prior_against_quadrature(seed):
    w, eta = ref.quadrature_case(seed, 20000, 4)
    pr = ref.prior_component(0, w, eta, (1, 1, 1))
    r = ref.powerscale(w.T, np.stack([np.zeros(w.shape[0]), pr]), np.ones(w.shape[0], np.int64))
    print(seed, r["sens"][1], r["khat"][1])
    assert np.max(np.abs(r["sens"][1] - ref.QUADRATURE_D)) <= QUADRATURE_MARGIN_P4
    want = np.array([ref.quadrature_sensitivity(float(w[:, p].min()), float(w[:, p].max())) for p in range(4)])
    print("over the sample's range:", want, np.abs(r["sens"][1] - want).max())
    assert np.max(np.abs(r["sens"][1] - want)) <= RANGE_MARGIN_P4
    assert np.all(r["sens"][0] == 0.0)                                       # a constant likelihood component: no ratio
    # alpha > 1 narrows the marginals, alpha < 1 widens them
    assert np.all(r["sd"][1, 1] < r["base_sd"]) and np.all(r["sd"][1, 0] > r["base_sd"])


def test_quadrature_depends_on_the_range():
    """The two figures DESIGN.md section 21 quotes: the issue's value is the +-12 sigma quadrature; +-4 sigma gives 0.0772."""
    assert ref.quadrature_sensitivity(-60.0, 60.0, n=400001) == pytest.approx(ref.QUADRATURE_D, abs=5e-6)
    assert ref.quadrature_sensitivity(-20.0, 20.0) == pytest.approx(0.07721, abs=5e-5)


def test_multiplicities_equal_repeats():
    rng = np.random.default_rng(5)
    U = 300
    x = rng.normal(0, 1, (3, U)).astype(np.float32)
    x[1, 10:20] = x[1, 10]                                                   # ties
    logp = np.stack([rng.normal(-40, 4, U), rng.normal(-20, 3, U)])
    counts = rng.integers(1, 5, U)
    a = ref.powerscale(x, logp, counts)
    own = np.repeat(np.arange(U), counts)
    b = ref.powerscale(x[:, own], logp[:, own], np.ones(own.size, np.int64))
    for k in ("dist", "mean", "sd", "sens", "base_mean", "base_sd", "khat"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-12, err_msg=k)
    assert np.array_equal(a["tail_len"], b["tail_len"])


def test_names_and_groups():
    assert powerscale_groups(("predictions", "weights"), TASK_REG) == ["weights", "predictions"]
    assert powerscale_groups(None, TASK_REG) == ["weights", "eta", "predictions"]
    assert powerscale_groups(None, TASK_CLS) == ["weights", "predictions"]
    with pytest.raises(ValueError, match="no eta"):                          # the default's tuple given explicitly is taken at its word
        powerscale_groups(("weights", "eta", "predictions"), TASK_CLS)
    assert powerscale_names(["weights", "eta", "predictions", "loglik"], n_param=3, n_rows=2) == \
        ["w[0]", "w[1]", "w[2]", "eta", "f[0]", "f[1]", "loglik"]
    assert powerscale_names(["predictions"], n_param=3, n_rows=2, n_out=2, task=TASK_CLS) == ["p[0,0]", "p[0,1]", "p[1,0]", "p[1,1]"]
    with pytest.raises(ValueError, match="unknown quantity group"):
        powerscale_groups(("weights", "bias"), TASK_REG)
    with pytest.raises(ValueError, match="no eta"):
        powerscale_groups(("eta",), TASK_CLS)
    with pytest.raises(ValueError, match="no quantity"):
        powerscale_groups((), TASK_REG)
    for bad in (0, -0.01, math.inf, math.nan):
        with pytest.raises(ValueError, match="delta"):
            powerscale_check_delta(bad)
    assert powerscale_check_delta(0.01) == 0.01


def test_diagnosis_and_flagging():
    assert powerscale_diagnosis(0.06, 0.07) == "prior-data conflict"
    assert powerscale_diagnosis(0.05, 0.049) == "strong prior / weak likelihood"
    assert powerscale_diagnosis(0.049, 0.9) == "-" and powerscale_diagnosis(0.0, 0.0) == "-"
    names = ["a", "b", "c"]
    res = PowerScaling(names=names, prior=dict(a=0.2, b=0.06, c=0.01), likelihood=dict(a=0.3, b=0.01, c=0.5), mean_shift={},
                       sd_ratio={}, khat={}, diagnosis={}, delta=0.01, threshold=0.05, good_k=0.7, n_samples=10, n_distinct=10)
    assert powerscale_flagged(res) == [("a", "prior-data conflict"), ("b", "strong prior / weak likelihood")]
    assert powerscale_flagged(res, threshold=0.1) == [("a", "prior-data conflict")]
    with pytest.raises(ValueError, match="threshold"):
        powerscale_flagged(res, threshold=0)
