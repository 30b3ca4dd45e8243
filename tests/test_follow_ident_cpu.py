"""The identical-input class on EVERY step (tests/parity.py: follow_device_run(ident_all=True)), checked without a GPU: the float32
fmaf helper the device's proposals are rebuilt with, the evaluation entry of the C oracle against the oracle's own runs, and the
teeth of the new check -- defects of a rejected step that the own-proposal bound lets through."""
from fractions import Fraction

import numpy as np
import pytest

import parity
from parity import orc

import ptnn_oracle_c as orc_c  # noqa: E402


def round_f32(fr):
    """A rational rounded ONCE to the nearest float32 (ties to even), normal range; exact integer arithmetic."""
    if fr == 0:
        return np.float32(0.0)
    sign, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while a / Fraction(2) ** e < 2 ** 23:
        e -= 1
    assert -149 < e < 104, "outside the normal range"
    q = a / Fraction(2) ** e                                 # in [2^23, 2^24)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** e)           # n <= 2^24: exact in float64, and the product too


def fmaf_exact(a, x, b):
    return np.array([round_f32(Fraction(float(np.float32(a))) * Fraction(float(xj)) + Fraction(float(bj))) for xj, bj in zip(x, b)],
                    dtype=np.float32)


def test_fmaf_helper_rounds_once_on_random_inputs():
    rng = np.random.default_rng(7)
    for a in (0.025, 0.2, 1.0 / 3.0, -1.75):
        x = rng.standard_normal(500).astype(np.float32)
        b = (rng.standard_normal(500) * 10.0 ** rng.integers(-3, 3, 500)).astype(np.float32)
        got, want = orc_c.fmaf(a, x, b), fmaf_exact(a, x, b)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fmaf_helper_on_constructed_double_rounding_cases():
    """a = 1 + 2^-23 and x = (1 - 2^-23) 2^k multiply to 2^k (1 - 2^-46): with k = -24 and b in [1, 2) of ODD last bit, a x + b lies
    2^-70 BELOW the tie between b and its upper neighbour -- the one rounding of fmaf goes down to b, but the float64 sum (ulp 2^-52)
    lands ON the tie and float32's ties-to-even then goes up.  Both signs, several binades."""
    a = np.float32(1.0 + 2.0 ** -23)
    xs, bs = [], []
    for j in (0, 1, 5, 1000, 2 ** 22 - 1):
        for k in (-3, 0, 4):
            for sgn in (1.0, -1.0):
                b = sgn * (2 ** 23 + 2 * j + 1) * 2.0 ** (k - 23)          # odd significand, in +-[2^k, 2^(k+1))
                xs.append(sgn * (1.0 - 2.0 ** -23) * 2.0 ** (k - 24))
                bs.append(b)
    x, b = np.array(xs, dtype=np.float32), np.array(bs, dtype=np.float32)
    assert np.array_equal(x.astype(np.float64), xs) and np.array_equal(b.astype(np.float64), bs)     # the cases ARE float32 numbers
    got, want = orc_c.fmaf(a, x, b), fmaf_exact(a, x, b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, b)                           # below the tie: b itself
    twice = (np.float64(a) * x.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    assert (twice != want).all(), "the float64 multiply-add rounded to float32 should round twice on every constructed case"


CPU_CASES = ["cooperative", "tree", "classification_langevin"]       # 4-5-1 Sunspot Langevin; 4-12-3 Iris random-walk and Langevin


@pytest.fixture(scope="module")
def alone():
    """The oracle run alone on each case, once: (PTOracle, per-step arrays).  Left unchanged by the tests."""
    out = {}
    for name in CPU_CASES:
        pt = parity.ident_case(name)[0]
        out[name] = (pt, parity.oracle_alone_run(pt))
    return out


def classes(o):
    import collections
    return collections.Counter(parity.step_class(d, s, l_) for d, s, l_ in zip(o["dec"].ravel(), o["stale"].ravel(), o["lg"].ravel()))


@pytest.mark.parametrize("name", CPU_CASES)
def test_evaluation_entry_returns_the_runs_own_values_on_every_step(alone, name):
    """orc_replica_eval_at at the run's OWN float64 proposals, from the per-step records alone, must give back the log alpha and the
    likeh entry the run itself formed -- accepted and rejected, fresh and stale, Langevin and random-walk, before and after the
    temperature switch.  1e-12 relative: of the likeh entry itself; of log alpha, a difference of terms of size `scale` each formed to
    float64 round-off, relative to that scale (the only float64 operation the two paths do not share is second = -|noise|^2 / 2
    against -|w' - sgd(w)|^2 / 2 step^2)."""
    pt, o = alone[name]
    recs = {k: o[k] for k in ("w_before", "eta_before", "lik_cur", "prior_cur", "adapttemp", "lg")}
    la, sc, lik = parity.ident_all_eval(pt, recs, o["w_prop"], o["eta_pro"], o["noise"])
    c = classes(o)
    lg_on = bool(o["lg"].any())
    assert np.isfinite(la).all() and la.size == parity.IDENT_R * (pt.S - 1)
    want = [parity.step_class(d, s, l_) for d in (0, 1) for s in (0, 1) for l_ in ((0, 1) if lg_on else (0,))]
    assert all(c[k] > 0 for k in want), c                    # every class occurs
    switch = int(pt.S * 0.6)
    assert (o["adapttemp"][1:, :switch] > 1.0).all() and (o["adapttemp"][:, switch:] == 1.0).all()
    assert np.abs(la - o["logalpha"]).max() <= 1e-12 * o["scale"].max() and (np.abs(la - o["logalpha"]) <= 1e-12 * o["scale"]).all()
    assert (np.abs(sc - o["scale"]) <= 1e-12 * o["scale"]).all()
    assert (np.abs(lik - o["likeh"]) <= 1e-12 * np.abs(o["likeh"])).all()


def old_bound_violations(la_dev, o, task):
    """The own-proposal check of follow_device_run: every step within LOGALPHA_REL_SYNCED of the scale of the oracle's own log alpha."""
    return int((np.abs(la_dev - o["logalpha"]) > parity.LOGALPHA_REL_SYNCED[task] * o["scale"] + parity.LOGALPHA_ABS).sum())


def new_check(la_dev, lik_dev, pt, o, la_id, sc_id, lik_id, strict):
    return parity.ident_all_check(la_dev, lik_dev, la_id, sc_id, lik_id, o["dec"], o["stale"], o["lg"], pt.train.shape[0], strict=strict)


def test_all_steps_check_has_teeth_where_the_own_proposal_bound_has_none(alone):
    """The Sunspot run's own per-step log alpha and likeh taken as "the device's", with three defects of REJECTED steps only:

      (a) log alpha off by 2e-5 of the scale (a likelihood sum wrong by ~1e-5 relative);
      (b) eta' replaced by the previous step's eta' (a neighbour's eta read for a rejected slot);
      (c) rejected Langevin steps proposed from w instead of sgd(w).

    The all-steps identical-input check (ident_all_check, the very function the GPU tests run) refuses each.  The own-proposal
    bound (LOGALPHA_REL_SYNCED: 1e-4 of the scale for regression) lets (a) through -- and so does the accepted-steps-only class, which
    never sees a rejected step.  (b) and (c) are caught by the own-proposal bound TOO: a neighbour's eta' differs by 0.2 x a normal
    difference and moves the Gaussian log-likelihood by tens of nats, and one SGD epoch at lr 0.1 moves the proposal by far more than
    the half ulp that bound allows for; they stay here because the new check must refuse them as well."""
    name = "cooperative"
    pt, o = alone[name]
    task = pt.task
    recs = {k: o[k] for k in ("w_before", "eta_before", "lik_cur", "prior_cur", "adapttemp", "lg")}
    la_id, sc_id, lik_id = parity.ident_all_eval(pt, recs, o["w_prop"], o["eta_pro"], o["noise"])
    rej = o["dec"] == 0
    rej_lg = rej & (o["lg"] != 0)
    assert rej.sum() > 500 and rej_lg.sum() > 100
    # no defect: both checks pass
    assert old_bound_violations(o["logalpha"], o, task) == 0
    rep = new_check(o["logalpha"], o["likeh"], pt, o, la_id, sc_id, lik_id, strict=True)
    assert rep["ident_all_steps"] == parity.IDENT_R * (pt.S - 1) and rep["ident_all_max_ratio"] < 1e-12
    # (a)
    la_a = o["logalpha"] + np.where(rej, 2e-5 * o["scale"], 0.0)
    assert old_bound_violations(la_a, o, task) == 0          # invisible to the own-proposal bound
    rep = new_check(la_a, o["likeh"], pt, o, la_id, sc_id, lik_id, strict=False)
    assert rep["ident_all_over_bound"] == int(rej.sum())     # every defective step refused, no other
    assert all(v["over_bound"] == (v["steps"] if k.startswith("rej") else 0) for k, v in rep["ident_all_by_class"].items()), rep
    with pytest.raises(AssertionError):
        new_check(la_a, o["likeh"], pt, o, la_id, sc_id, lik_id, strict=True)
    # (b), (c): the defective device evaluated by the same float64 entry at ITS (wrong) proposal
    eta_b = o["eta_pro"].copy()
    eta_b[:, 1:] = np.where(rej[:, 1:], o["eta_pro"][:, :-1], o["eta_pro"][:, 1:])
    w_c = np.where(rej_lg[:, :, None], o["w_before"].astype(np.float64) + pt.replicas[0].c.step_w * o["noise"], o["w_prop"])
    for what, w_dev, eta_dev, hit in (("b", o["w_prop"], eta_b, rej & (eta_b != o["eta_pro"])), ("c", w_c, o["eta_pro"], rej_lg)):
        la_d, _, lik_d = parity.ident_all_eval(pt, recs, w_dev, eta_dev, o["noise"])
        rep = new_check(la_d, lik_d, pt, o, la_id, sc_id, lik_id, strict=False)
        assert rep["ident_all_over_bound"] >= 0.9 * hit.sum() and rep["ident_all_lik_over_bound"] >= 0.9 * hit.sum(), (what, rep)
        assert all(v["over_bound"] == 0 for k, v in rep["ident_all_by_class"].items() if k.startswith("acc")), (what, rep)
        assert old_bound_violations(la_d, o, task) > 0, what  # caught by the own-proposal bound too (see the docstring)
