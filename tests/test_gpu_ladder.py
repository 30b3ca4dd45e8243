"""Ladder adaptation on the GPU (ptnn_set_ladder_adaptation): the device's ladder history against the
float64 replay of the update fed its own recorded acceptances on every schedule, bitwise repeatability and launch-split invariance,
label swapping against state moves, checkpoint and resume, the effect on a badly spaced ladder (recorded), refusals."""
import warnings

import numpy as np
import pytest

import ladder_ref as ref
import parity
from parity import orc

pytestmark = pytest.mark.gpu

KAPPA0, T0 = 0.5, 20.0


def _ds():
    return parity.datasets()


def _case(task):
    if task == 0:
        return (4, 5, 1), "sunspot", True, 0.1, 10
    if task == 2:                                                        # wide regression net (wide body)
        return (32, 512, 1), "synth32", True, 0.01, 10
    return (4, 12, 3), "iris", False, 0.01, 10


def _sampler(task, R=8, S=200, si=5, A=20, seed=71, adapt=True, ladder=None, **kw):
    topo, name, lg, lr, mt = _case(task)
    task = min(task, 1) if task != 2 else 0
    d = _ds()
    s = parity.make_sampler(task, topo, d[name + "_train"], d[name + "_test"], R_local=R, R_global=R, first=0, S=S, si=si,
                            use_lg=lg, lr=lr, seed=seed, swap_rule=1, **kw)
    from ptnn_amd import ladder as geo
    T = np.asarray(ladder if ladder is not None else geo.temperatures(R, mt), np.float32)
    P = topo[0] * topo[1] + topo[1] * topo[2] + topo[1] + topo[2]
    w0 = np.random.default_rng(seed).standard_normal((R, P)).astype(np.float32)
    s.set_state(w0, T)
    s.set_ladder(T)
    if adapt:
        s.set_ladder_adaptation(A, KAPPA0, T0)
    return s, T, w0


def _run(s, per_interval=None):
    if per_interval:
        while s.steps_done() < s.S - 1:
            s.run(per_interval)
        s.run(-1)
    else:
        s.run(-1)
    s.sync()
    lad, acc = s.ladder_history()
    return dict(lad=lad, acc=acc, log=s.swap_log(), tr=s.traces(), stats=s.swap_stats())


def _same(a, b, label):
    assert np.array_equal(a["lad"], b["lad"], equal_nan=True), f"{label}: ladder history"
    assert np.array_equal(a["acc"], b["acc"], equal_nan=True), f"{label}: acceptances"
    assert np.array_equal(a["log"], b["log"]), f"{label}: swap log"
    assert a["stats"] == b["stats"], f"{label}: swap counters"
    for k in a["tr"]:
        if a["tr"][k] is not None:
            assert np.array_equal(a["tr"][k], b["tr"][k], equal_nan=True), f"{label}: trace {k}"


@pytest.mark.parametrize("task", [0, 1])
def test_replay_matches_float64(task):
    A = 20
    s, T, _ = _sampler(task, A=A)
    out = _run(s)
    lad, acc = out["lad"], out["acc"]
    assert lad.shape == (A + 1, 8) and acc.shape[0] == out["stats"][2] == orc.count_handoffs(task, 200, 5)
    assert np.isfinite(acc).all() and (acc >= 0).all() and (acc <= 1).all()
    assert np.array_equal(lad[0], T)
    want = ref.replay(T, acc.astype(np.float64), A, KAPPA0, T0)
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(lad.astype(np.float64) - want.astype(np.float64)) <= ulp), np.abs(lad - want).max()
    assert (lad[:, 0] == 1.0).all() and (lad[:, -1] == T[-1]).all() and (np.diff(lad, axis=1) > 0).all()
    assert not np.array_equal(lad[-1], T)                                # the ladder moved


@pytest.mark.parametrize("label", [0, 1], ids=["state", "label"])
def test_accept_and_tempering_against_the_weights(label):
    """Independent of the kernel's own records: Iris with random-walk proposals (no eta), untempered log-likelihoods of the
    chains' weights from ptnn_evaluate.  (1) Stopped a few steps after rounds 2, 10 (adapting) and 22 (frozen, A = 20), every
    chain's likelihood times the temperature its slot holds in the NEW ladder is the untempered likelihood of its weights: a
    chain that rejected since the round carries the re-tempered likelihood (stale SF_LIK: L T_new / T_old), one that accepted
    computed it at its temperature (stale temps_local: L T_old / T_new).  (2) Every recorded a_k(t) is ref.pair_accept of the
    round's ladder (history row min(t, A)) and the hand-off likelihoods of the chains that held temperatures k, k+1 (label mode:
    through the swap log's slot mapping)."""
    A, S, R = 20, 200, 8
    s, T, _ = _sampler(1, A=A, S=S, label_swap=label)
    hand = [i for i in range(S - 1) if (i + 1) % 5 == 0]               # CLS hand-off rule (switch at step 120)
    for r in (2, 10, 22):
        s.run(hand[r] + 4 - s.steps_done())                            # the round after step hand[r], then 3 more steps
        s.sync()
        st = s.state()
        lad, _ = s.ladder_history()
        Tn = lad[min(r + 1, A)].astype(np.float64)
        t_of_slot = s.labels() if label else np.arange(R)
        ll = s.evaluate(st["w"])[:, 0].astype(np.float64)
        np.testing.assert_allclose(st["likelihood"].astype(np.float64) * Tn[t_of_slot], ll, rtol=1e-4, atol=1e-3,
                                   err_msg=f"after round {r}: chain likelihood x new temperature != evaluate(w)")
    out = _run(s)
    lad, acc, log, tr = out["lad"].astype(np.float64), out["acc"], out["log"], out["tr"]
    ll = s.evaluate(tr["pos_w"].reshape(-1, tr["pos_w"].shape[2]))[:, 0].astype(np.float64).reshape(R, S)
    holder = np.arange(R)                                             # holder[t] = slot of the chain at temperature t
    for r, h in enumerate(hand):
        want = ref.pair_accept(lad[min(r, A)], ll[holder, h + 1])
        np.testing.assert_allclose(acc[r], want, rtol=0.02, atol=2e-3, err_msg=f"round {r}: a_k")
        if label:
            holder = holder[log[r]]
    assert np.abs(lad[A] / lad[0] - 1.0).max() > 0.05                    # the ladder moved, so (1) and (2) tell the ladders apart


def test_acceptance_rows_follow_the_posted_likelihoods():
    """Record only (rounds = 0): the ladder stays and the run is bit for bit the run without a spec."""
    s, T, _ = _sampler(0, A=0)
    out = _run(s)
    assert out["lad"].shape == (1, 8) and np.array_equal(out["lad"][0], T)
    base, _, _ = _sampler(0, adapt=False)
    b = _run_plain(base)
    assert np.array_equal(out["log"], b["log"])                          # recording changes nothing
    for k in out["tr"]:
        if out["tr"][k] is not None:
            assert np.array_equal(out["tr"][k], b["tr"][k], equal_nan=True)


def _run_plain(s):
    s.run(-1)
    s.sync()
    return dict(log=s.swap_log(), tr=s.traces(), stats=s.swap_stats())


@pytest.mark.parametrize("task,kw", [(0, dict(schedule=1)), (0, dict(schedule=2, groups=1)), (0, dict(schedule=2, groups=2)),
                                     (0, dict(schedule=3)), (1, dict(schedule=4)), (2, dict())],
                         ids=["coop", "spec1", "spec2", "packed", "tree", "wide"])
def test_every_schedule(task, kw):
    """Every schedule that runs rule 1 for the shape: its ladder history is the replay of its own acceptances (the update does
    not depend on the body or the block size), repeated runs are bitwise identical, and it follows the cooperative schedule's
    ladder to fp32 level (the schedules' likelihoods differ in the last bits, so do their a_k)."""
    runs = [_run(_sampler(task, **kw)[0]) for _ in range(2)]
    _same(runs[0], runs[1], f"{kw} twice")
    lad, acc = runs[0]["lad"], runs[0]["acc"]
    want = ref.replay(lad[0], acc.astype(np.float64), lad.shape[0] - 1, KAPPA0, T0)
    assert np.all(np.abs(lad.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))
    if task == 0:
        coop = _run(_sampler(0, schedule=1)[0])
        assert np.allclose(lad[:6], coop["lad"][:6], rtol=1e-4)
    assert not np.array_equal(lad[-1], lad[0])


def test_invariant_over_launch_split():
    a = _run(_sampler(1)[0])
    b = _run(_sampler(1)[0], per_interval=5)
    _same(a, b, "run(-1) vs one interval per call")


def test_label_mode_close_to_state_moves():
    a = _run(_sampler(0, seed=72)[0])
    b = _run(_sampler(0, seed=72, label_swap=1)[0])
    # round 0 sees the same posted likelihoods and gives the same ladder; from there the two modes part by the fp32 rounding of
    # the re-tempered likelihoods (label mode keeps a chain's own, state moves re-temper the arriving one), as they do today
    assert np.allclose(a["acc"][0], b["acc"][0], rtol=1e-5, atol=1e-7)
    assert np.allclose(a["lad"][1], b["lad"][1], rtol=1e-5)
    for out in (a, b):
        want = ref.replay(out["lad"][0], out["acc"].astype(np.float64), out["lad"].shape[0] - 1, KAPPA0, T0)
        assert np.all(np.abs(out["lad"].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))


def test_checkpoint_resume_bitwise():
    full = _run(_sampler(0)[0])
    s, _, _ = _sampler(0)
    s.run(52)                                  # mid-adaptation: 10 rounds done
    s.sync()
    blob = s.checkpoint()
    s2, _, _ = _sampler(0, adapt=False)
    s2.set_ladder_adaptation(20, KAPPA0, T0)
    s2.restore(blob)
    s2.run(-1)
    s2.sync()
    lad, acc = s2.ladder_history()
    assert np.array_equal(lad, full["lad"], equal_nan=True)
    assert np.array_equal(acc, full["acc"])
    assert np.array_equal(s2.swap_log(), full["log"])
    tr = s2.traces(53, 200 - 53)
    for k in tr:
        if tr[k] is not None:
            assert np.array_equal(tr[k], full["tr"][k][:, 53:], equal_nan=True), k


def test_checkpoint_spec_mismatch_refused():
    from ptnn_amd._lib import PtnnError
    s, _, _ = _sampler(0)
    s.run(52)
    s.sync()
    blob = s.checkpoint()
    s2, _, _ = _sampler(0, A=10)                                 # a different adaptation: refused, nothing overflows
    with pytest.raises(PtnnError, match="adapts the ladder over 20 rounds"):
        s2.restore(blob)
    s3, _, _ = _sampler(0, adapt=False)                          # none set: the checkpoint's spec is taken, and reported
    s3.restore(blob)
    assert s3.ladder_adaptation() == (20, KAPPA0, T0)
    assert s3.ladder_history()[0].shape == (21, 8)
    plain, _, _ = _sampler(0, adapt=False)
    plain.run(52)
    plain.sync()
    with pytest.raises(PtnnError, match="without ladder adaptation"):
        _sampler(0)[0].restore(plain.checkpoint())


def test_two_blocks_on_one_gpu(tmp_path):
    """Two blocks of one ladder on one GPU (LadderGroup, host-staged): the same history as one handle; both ranks agree."""
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    d = _ds()
    out = []
    for devices in (None, [0, 0]):
        kw = dict(devices=devices, transport="host") if devices else {}
        pt = ParallelTempering(True, 0.1, d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 8, 10, 8 * 200, 5, 0.5,
                               str(tmp_path), seed=9, write_files=False, swap_rule=1, schedule=1,
                               adapt_ladder=dict(rounds=19, kappa0=KAPPA0, t0=T0), **kw)
        pt.initialize_chains(0.5)
        pt.run_chains()
        out.append(pt)
    one, two = out
    ranks = [sh.ladder_history() for sh in two._sampler.shards]
    assert np.array_equal(ranks[0][0], ranks[1][0], equal_nan=True) and np.array_equal(ranks[0][1], ranks[1][1])
    assert np.array_equal(one.ladder_history, two.ladder_history, equal_nan=True)
    assert one.temperatures == two.temperatures
    assert not np.array_equal(one.ladder_history[-1], one.ladder_history[0])


def test_refusals():
    from ptnn_amd._lib import PtnnError
    s, T, _ = _sampler(0, adapt=False)
    with pytest.raises(PtnnError, match="rounds"):
        s.set_ladder_adaptation(10 ** 4, KAPPA0, T0)
    with pytest.raises(PtnnError, match="kappa0"):
        s.set_ladder_adaptation(5, -1.0, T0)
    with pytest.raises(PtnnError, match="kappa0"):
        s.set_ladder_adaptation(5, KAPPA0, float("nan"))
    s.set_ladder(T * 2)                                           # does not start at 1
    with pytest.raises(PtnnError, match="start at exactly 1"):
        s.set_ladder_adaptation(5, KAPPA0, T0)
    s.set_ladder(T[::-1].copy())
    with pytest.raises(PtnnError):
        s.set_ladder_adaptation(5, KAPPA0, T0)
    s.set_ladder(T)
    s.run(5)
    s.sync()
    with pytest.raises(PtnnError, match="after MH steps"):
        s.set_ladder_adaptation(5, KAPPA0, T0)
    # swap_rule 0
    topo, name, lg, lr, _ = _case(0)
    d = _ds()
    s0 = parity.make_sampler(0, topo, d[name + "_train"], d[name + "_test"], R_local=8, R_global=8, first=0, S=200, si=5,
                             use_lg=lg, lr=lr, seed=1, swap_rule=0)
    s0.set_ladder(T)
    with pytest.raises(PtnnError, match="swap_rule 1"):
        s0.set_ladder_adaptation(5, KAPPA0, T0)
    # no ladder
    s1 = parity.make_sampler(0, topo, d[name + "_train"], d[name + "_test"], R_local=8, R_global=8, first=0, S=200, si=5,
                             use_lg=lg, lr=lr, seed=1, swap_rule=1)
    with pytest.raises(PtnnError, match="ptnn_set_ladder"):
        s1.set_ladder_adaptation(5, KAPPA0, T0)
    # past the switch: S = 100 -> switch at step 60, round 12 hands off at step 60, round 13 at 65
    s2 = parity.make_sampler(0, topo, d[name + "_train"], d[name + "_test"], R_local=8, R_global=8, first=0, S=100, si=5,
                             use_lg=lg, lr=lr, seed=1, swap_rule=1)
    s2.set_ladder(T)
    s2.set_ladder_adaptation(12, KAPPA0, T0)
    with pytest.raises(PtnnError, match="temperature switch"):
        s2.set_ladder_adaptation(13, KAPPA0, T0)


def _stationary_pt(tmp_path, adapt, seed=7):
    """The 12-row 4-3-1 regression of test_gpu_evidence.py: random-walk proposals, swap_rule 1, shared_noise False, 16 chains,
    maxtemp 1000, si = 5, S = 40 001 (0.6 S not an integer: no switch), burn_in 0.5 -> 4000 adapted rounds."""
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    rng = np.random.default_rng(11)
    x = rng.random((12, 4))
    data = np.column_stack([x, 0.2 + 0.6 * x[:, 0] * x[:, 1] + 0.05 * rng.standard_normal(12)])
    tmp_path.mkdir(parents=True, exist_ok=True)
    pt = ParallelTempering(False, 0.1, data, data, [4, 3, 1], 16, 1000, 16 * 40001, 5, 0.5, str(tmp_path), seed=seed,
                           write_files=False, swap_rule=1, shared_noise=False, adapt_ladder=adapt)
    pt.initialize_chains(0.5)
    pt.run_chains()
    return pt


def test_effect_and_python_surface(tmp_path):
    """With the default kappa0 / t0 the spread (max - min over the pairs) of the mean Rao-Blackwellised acceptance after the freeze
    is at most half that of the same run with rounds = 0 (fixed seed; measured 0.114 against 0.532 -- over three seeds 0.20
    against 0.53, profiles/ladder_probe_effect.jsonl).  Also: the adapted rounds, the frozen ladder as
    `temperatures`, the diagnostics and log_evidence's refusal of a window before the freeze; ti_discretisation is recorded."""
    fixed = _stationary_pt(tmp_path / "f", dict(rounds=0))
    adapt = _stationary_pt(tmp_path / "a", True)
    df, da = fixed.ladder_diagnostics(), adapt.ladder_diagnostics()
    sf, sa = np.ptp(df["pair_accept_rb"]), np.ptp(da["pair_accept_rb"])
    print(f"\nspread of mean a_k after burn-in: fixed {sf:.4f}, adapted {sa:.4f}")
    print("fixed   ", np.round(df["pair_accept_rb"], 3).tolist())
    print("adapted ", np.round(da["pair_accept_rb"], 3).tolist())
    print("ladder  ", np.round(da["temperatures"], 3).tolist())
    print("round trips fixed", int(df["round_trips"].sum()), "adapted", int(da["round_trips"].sum()))
    assert sa <= 0.5 * sf
    A = adapt.ladder_history.shape[0] - 1
    assert A == adapt._ladder_adapt_spec()[0] == 3999
    assert np.array_equal(np.asarray(adapt.temperatures, np.float32), adapt.ladder_history[-1])
    assert adapt.temperatures[0] == 1.0 and adapt.temperatures[-1] == 1000.0
    assert df["history"] is not None and da["pair_accept"].shape == (15,) and da["round_trips"].shape == (16,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ef = fixed.log_evidence(prior_draws=1 << 16)
        ea = adapt.log_evidence(prior_draws=1 << 16)
    print("ti_discretisation fixed", ef.ti_discretisation, "adapted", ea.ti_discretisation)
    with pytest.raises(ValueError, match="froze"):
        adapt.log_evidence(burn_in=0.25)
