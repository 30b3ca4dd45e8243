"""The swap round (cascade_lds_prefix, csrc/ptnn_dev_spec.hpp) held to the float64 oracle past one wave of pairs: 65 .. 1024 rungs,
rounds 0, 1 and 7, both launch widths of swap_kernel, and the rounds the segment kernels run inside their own launches.  The cases,
the 8-unit decision margin and its derivation are in tests/swap_cases.py; tests/test_swap_cases_cpu.py shows from the oracle alone
that every case clears the margin and that a scan with one of its corner cases broken fails them.

a. THE KERNEL ALONE (rule 0): swap_set_L + swap_cascade on one handle per R (4-5-1, 7 training rows, R_local = 1, R_global = R,
   S = 10).  swap_kernel keys its uniforms with the handle's round counter; the point-to-point flow advances it without a run
   (ptnn_swap_apply; with phantom = 1 it counts the round on the final-scalar buffer and moves nothing), set_state puts it back to 0,
   and swap_stats() is asked for the round before the uniforms are trusted.  Every case: the permutation from both scalar buffers
   (the other buffer holds a decoy ladder), element for element, and the accepted-swap count the round adds to the counters -- the
   kernel forms it from its ballots, not from the permutation.  R = 130 is repeated on a 32-16-1 handle whose padded row of 548 floats
   makes launch_swap take 256 threads at a short ladder.

b. THE ROUNDS INSIDE THE KERNELS, REPLAYED.  After a finished run (S = 41, si = 8: no temperature switch, five rounds; 7 training and
   3 test rows) the scalars every round decided on are rebuilt from the device's own traces (swap_cases.replay_rule0: a slot keeps the
   likelihood of the last proposal it accepted; REG posts likelihood * T as one fp32 product, CLS the tempered likelihood, the
   phantom round the final one), the oracle's cascade is run on them with the round's uniforms, and swap_log()[n] and the swap
   counters must agree for every round whose margin is at least 8 units (at most one round in ten may fall below and be skipped).
   Regression scalars are rebuilt bit for bit -- the replayed final likelihood equals state()'s; classification traces record
   likelihood * T, so the quotient is known to 1.5 ulp, which comes off the margin.  The start-up likelihood of a chain that accepts
   nothing before the first round is not in the trace: one MH step is run, state() read, and the run restarted.
   Label swapping is replayed through the slot maps: the chains stay, a round hands temperature t to the chain that held src[t] and
   re-tempers its likelihood by To / Tn (swap_block); the replayed labels equal labels().

c. THE EVEN/ODD RULE (swap_rule 1), R = 131 and 515: the strided pair loop of swap_kernel makes a second pass (64 threads: R > 129;
   256 threads: R > 513).  One launch per interval against one launch per run bit for bit, the log's structure (a permutation, only
   pairs of the round's parity move), and the oracle's rule on the replayed untempered scalars (swap_cases.replay_rule1) for every
   round that clears the rule-1 margin.

The float64 oracle at the same configurations and seeds (its own chains on this file's data, starts and tape) clears the margin in
every round; worst round of each run, in units: packed 4-5-1 R = 66: 8.7e+05, R = 130: 4.1e+06; label swapping R = 130: 3.6e+06;
cooperative 4-12-3 R = 130: 5.6e+05; tree 4-12-3 R = 66: 2.4e+05; packed over several CUs 4-10-1 R = 66: 2.3e+06; even/odd
R = 131: 856, R = 515: 104 (rule-1 units, bound 3.2).  (With seven training rows most pairs of these rounds are far from their
boundary -- 286 to 640 of the 325 / 645 pairs of a run swap; the uniform-decided ladders are part a's.)

Worst margins of the device's own rounds, measured on MI355X (no round fell below the margin): packed 4-5-1 R = 66: 8.64e+05 and
R = 130: 4.07e+06 in all three modes; cooperative 4-12-3 R = 130: 5.56e+05; tree 4-12-3 R = 66: 2.41e+05; packed over 2 CUs 4-10-1
R = 66: 2.26e+06; label swapping R = 130: 4.01e+06; even/odd R = 131: 856, R = 515: 104 rule-1 units.

Not reachable on an MI355X (256 CUs): 4-10-1 over 4 CUs per replica at R = 66 (264 work-groups, one to a CU: the plan keeps one
launch per interval, so the in-launch round is tested over 2 CUs, the largest resident choice); one launch per run at R = 515 under
the even/odd rule (two packed work-groups fit a CU: 512 < 515), where both modes are one launch per interval."""
import math

import numpy as np
import pytest

import parity
import swap_cases as sc
from parity import orc
from test_gpu_analysis_shapes import _data

pytestmark = pytest.mark.gpu

TAPE = orc.PhiloxTape(sc.SEED)
S, SI, NTR, NTE = 41, 8, 7, 3
ENV_VARS = ("PTNN_PERSISTENT", "PTNN_SWAP_PIPELINE", "PTNN_SWAP_DELAY", "PTNN_PACK_FIXED_H")
ENV = {"interval": {"PTNN_PERSISTENT": "0"}, "barrier": {"PTNN_SWAP_PIPELINE": "0"}, "pipelined": {}, "default": {}}
SWAP_ROUNDS = {"interval": "between launches", "barrier": "grid barrier", "pipelined": "pipelined (ring 4)"}


# ---- a. the kernel alone ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles():
    """One handle per (R, wide row) for the module."""
    made = {}

    def get(R, wide=False):
        if (R, wide) not in made:
            if wide:
                topo = (32, 16, 1)
                train, test = _data(orc.TASK_REG, topo, 5, n_tr=NTR, n_te=NTE)
            else:
                topo = (4, 5, 1)
                d = parity.datasets()
                train, test = d["sunspot_train"][:NTR], d["sunspot_test"][:NTE]
            s = parity.make_sampler(orc.TASK_REG, topo, train, test, R_local=1, R_global=R, first=0, S=10, si=100, use_lg=False, lr=0.1,
                                    seed=sc.SEED)
            assert (s.state_row_floats() > 256) == wide
            w0 = TAPE.w_init(0, orc.num_param(topo)).astype(np.float32)[None, :]
            made[(R, wide)] = (s, w0, np.ones(1, dtype=np.float32))
        return made[(R, wide)]
    yield get
    for s, _, _ in made.values():
        s.close()


def kernel_alone(handle, R):
    s, w0, T1 = handle
    nothing = np.zeros(R, dtype=np.int32)
    for rnd in sc.ROUNDS:
        u = TAPE.swap_uniforms(rnd, R - 1)
        for name, L, drops in sc.cases(R, rnd):
            decoy = sc.scripted(R, [] if name == "scripted-all" else range(R - 1))
            s.set_state(w0, T1)                              # round counter and swap counters back to 0
            for _ in range(rnd):
                s.swap_apply(nothing, 1)                     # counts a round, moves nothing
            before = s.swap_stats()
            assert before[2] == rnd, (before, rnd)
            want, nsw = orc.swap_cascade([float(v) for v in L], u)
            if drops is not None:
                assert [k for k in range(R - 1) if want[k] != k + 1] == list(drops)
            for phantom in (0, 1):
                s.swap_set_L(L, phantom)
                s.swap_set_L(decoy, 1 - phantom)
                got = s.swap_cascade(phantom).tolist()
                assert got == want, (R, rnd, name, phantom, next(k for k in range(R) if got[k] != want[k]))
            s.swap_apply(nothing, 1)                         # the same round, counted: the final-scalar buffer holds L
            after = s.swap_stats()
            assert (after[0] - before[0], after[1] - before[1], after[2]) == (nsw, R - 1, rnd + 1), (R, rnd, name, before, after, nsw)


@pytest.mark.parametrize("R", sc.SIZES)
def test_kernel_alone_against_the_oracle(R, handles):
    kernel_alone(handles(R), R)


def test_kernel_alone_256_threads_at_a_short_ladder(handles):
    kernel_alone(handles(130, wide=True), 130)


# ---- b. the rounds inside the kernels -----------------------------------------------------------------------------------------
def device_run(monkeypatch, mode, task, topo, train, test, R, seed, *, lg, lr, maxtemp, expect=None, kernel=None, probe=False, **kw):
    """One finished run -> dict(tr, log, stats, state, T, lik0, info[, labels]).  lik0: the likelihood every chain holds after MH step 0
    of a first, discarded launch -- its start-up likelihood unless it accepted that step, which the trace then records.  probe: nothing
    is run, -> describe()."""
    with monkeypatch.context() as m:
        for var in ENV_VARS:
            m.delenv(var, raising=False)
        for var, val in ENV[mode].items():
            m.setenv(var, val)
        P = orc.num_param(topo)
        tape = orc.PhiloxTape(seed)
        w0 = np.stack([tape.w_init(r, P) for r in range(R)]).astype(np.float32)
        T = np.array(orc.temperature_ladder(R, maxtemp), dtype=np.float32)
        s = parity.make_sampler(task, topo, train, test, R_local=R, R_global=R, first=0, S=S, si=SI, use_lg=lg, lr=lr, seed=seed, **kw)
        try:
            info = s.describe()
            if probe:
                return info
            if expect is not None:
                assert info["swap_rounds"] == expect, (mode, info)
            if kernel is not None:
                assert kernel in info["kernel"], info
            ladder = bool(kw.get("swap_rule") or kw.get("label_swap"))

            def restart():
                s.set_state(w0, T)
                if ladder:
                    s.set_ladder(T)
            restart()
            s.run(1)
            s.sync()
            lik0 = s.state()["likelihood"].copy()
            restart()
            s.run(-1)
            s.sync()                                         # raises when a bounded wait of the launch ran out
            out = dict(tr=s.traces(), log=s.swap_log(), stats=s.swap_stats(), state=s.state(), T=T, lik0=lik0, info=info, tape=tape)
            if kw.get("label_swap"):
                out["labels"] = s.labels()
            return out
        finally:
            s.close()


def replayed(run, task, label):
    """Part b's assertion for a run of the cascade rule without label swapping."""
    tr, st, R = run["tr"], run["state"], len(run["T"])
    rounds = sc.replay_rule0(task, run["T"], tr["likeh"], tr["accept"], st["num_accepted"], run["lik0"], S, SI, dtype=np.float32)
    assert len(rounds) == 5 == run["stats"][2], (label, run["stats"])
    if rounds[-1][2]:                                        # the phantom round's scalars are the final state's, bit for bit
        assert np.array_equal(rounds[-1][0], st["likelihood"]), label
    nsw, worst, skipped = sc.check_rounds(rounds, run["log"], run["tape"], label + " ")
    print(f"{label}: worst margin {worst:.3g} units, rounds below the margin {skipped}")
    assert run["stats"] == (nsw, len(rounds) * (R - 1), len(rounds)), (label, run["stats"], nsw)
    assert nsw > 0, label
    return worst


def sunspot(name="sunspot"):
    d = parity.datasets()
    return d[name + "_train"][:NTR], d[name + "_test"][:NTE]


@pytest.mark.parametrize("mode", ["interval", "barrier", "pipelined"])
@pytest.mark.parametrize("R", [66, 130])
def test_packed_rounds_replayed(R, mode, monkeypatch):
    run = device_run(monkeypatch, mode, orc.TASK_REG, (4, 5, 1), *sunspot(), R, 21, lg=True, lr=0.1, maxtemp=2, schedule=3,
                     expect=SWAP_ROUNDS[mode], kernel="segment_pack_kernel<0,4,1,5>")
    replayed(run, orc.TASK_REG, f"packed 4-5-1 R = {R} {mode}")


def test_cooperative_grid_barrier_rounds_replayed(monkeypatch):
    d = parity.datasets()
    run = device_run(monkeypatch, "default", orc.TASK_CLS, (4, 12, 3), d["iris_train"][:NTR], d["iris_test"][:NTE], 130, 22, lg=False,
                     lr=0.01, maxtemp=10, schedule=1, expect="grid barrier", kernel="segment_kernel")
    replayed(run, orc.TASK_CLS, "cooperative 4-12-3 R = 130")


def test_tree_in_launch_rounds_replayed(monkeypatch):
    """TREE_PERSIST_MAX_R = 85: 66 rungs have room in the record area."""
    d = parity.datasets()
    try:
        run = device_run(monkeypatch, "default", orc.TASK_CLS, (4, 12, 3), d["iris_train"][:NTR], d["iris_test"][:NTE], 66, 23, lg=False,
                         lr=0.01, maxtemp=10, schedule=4, groups=3, expect="in-kernel exchange", kernel="segment_tree_kernel")
    except Exception as e:                                   # noqa: BLE001
        if "cannot all be resident" not in str(e):
            raise
        pytest.skip(f"the residency check refuses 66 x 3 work-groups: {e}")
    replayed(run, orc.TASK_CLS, "tree 4-12-3 R = 66")


def test_packed_over_several_cus_in_launch_rounds_replayed(monkeypatch):
    """The largest groups_per_replica whose 66 x groups work-groups describe() reports resident (the rounds then run inside the launch)."""
    d = parity.datasets()
    args = (orc.TASK_REG, (4, 10, 1), d["mackey_train"][:NTR], d["mackey_test"][:NTE], 66, 24)
    kw = dict(lg=True, lr=0.1, maxtemp=2)
    refused = []
    for groups in (4, 2):
        try:
            info = device_run(monkeypatch, "default", *args, probe=True, groups=groups, **kw)
        except Exception as e:                               # noqa: BLE001
            if "resident" not in str(e) and "LDS" not in str(e):
                raise
            refused.append(f"groups = {groups}: {e}")
            continue
        if info["swap_rounds"] != "in-kernel exchange":
            refused.append(f"groups = {groups}: {info['grid_blocks']} work-groups are not resident, the rounds run {info['swap_rounds']}")
            continue
        run = device_run(monkeypatch, "default", *args, groups=groups, expect="in-kernel exchange", kernel="segment_packm_kernel", **kw)
        assert run["info"]["groups_per_replica"] == groups, run["info"]
        replayed(run, orc.TASK_REG, f"packed over {groups} CUs 4-10-1 R = 66")
        return
    pytest.skip("; ".join(refused))


def test_label_swapping_rounds_replayed(monkeypatch):
    R = 130
    run = device_run(monkeypatch, "default", orc.TASK_REG, (4, 5, 1), *sunspot(), R, 21, lg=True, lr=0.1, maxtemp=2, schedule=3,
                     label_swap=1, expect="grid barrier")
    tr, st, T = run["tr"], run["state"], run["T"]
    dec = sc.accepted_steps(tr["accept"], st["num_accepted"])
    lik = [np.float32(v) for v in run["lik0"]]
    label, slot_of = list(range(R)), list(range(R))          # label[slot] = temperature index it holds; slot_of = the inverse
    rounds, done = [], 0

    def advance(upto):
        for r in range(R):
            for i in range(done, upto + 1):
                if dec[r, i]:
                    lik[r] = np.float32(tr["likeh"][r][i + 1])
    for i in sc.handoff_steps(orc.TASK_REG, S, SI):
        advance(i)
        done = i + 1
        L = np.array([np.float32(lik[slot_of[t]] * T[t]) for t in range(R)], dtype=np.float32)
        rounds.append((L, np.zeros(R), False))
        src = run["log"][len(rounds) - 1]
        new_slot_of = [slot_of[int(src[t])] for t in range(R)]
        for t, slot in enumerate(new_slot_of):
            if label[slot] != t:
                lik[slot] = np.float32(lik[slot] * np.float32(T[label[slot]] / T[t]))
                label[slot] = t
        slot_of = new_slot_of
    advance(S - 2)
    rounds.append((np.array([lik[slot_of[t]] for t in range(R)], dtype=np.float32), np.zeros(R), True))
    assert label == run["labels"].tolist() and sorted(label) == list(range(R))
    assert np.array_equal(np.array(lik, dtype=np.float32), st["likelihood"])
    nsw, worst, skipped = sc.check_rounds(rounds, run["log"], run["tape"], "label swapping ")
    print(f"label swapping R = {R}: worst margin {worst:.3g} units, rounds below the margin {skipped}")
    assert run["stats"] == (nsw, 5 * (R - 1), 5) and nsw > 0, (run["stats"], nsw)


# ---- c. the even/odd rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [131, 515])
def test_even_odd_rounds(R, monkeypatch):
    args = (orc.TASK_REG, (4, 5, 1), *sunspot(), R, sc.EVENODD_SEED)
    kw = dict(lg=True, lr=0.1, maxtemp=2, schedule=3, swap_rule=1)
    # One launch per run needs every work-group resident.  On an MI355X (256 CUs, two of these work-groups each) 515 are not: the
    # default then is one launch per interval too, the comparison below is of that path with itself, and what R = 515 adds is
    # swap_kernel's 256-thread second pass against the oracle.
    info = device_run(monkeypatch, "default", *args, probe=True, **kw)
    resident = info["grid_blocks"] <= info["blocks_per_cu"] * info["num_cus"]
    assert resident or R > 500, info
    runs = {mode: device_run(monkeypatch, mode, *args, expect=expect, **kw)
            for mode, expect in (("interval", "between launches"), ("default", "grid barrier" if resident else "between launches"))}
    a, b = runs["interval"], runs["default"]
    for k in a["tr"]:
        assert np.array_equal(a["tr"][k].view(np.uint32), b["tr"][k].view(np.uint32)), k
    for k in a["state"]:
        assert np.array_equal(a["state"][k].view(np.uint32), b["state"][k].view(np.uint32)), k
    assert np.array_equal(a["log"], b["log"]) and a["stats"] == b["stats"]
    log, T, tape = a["log"], a["T"], a["tape"]
    assert len(log) == 4 == a["stats"][2]                    # no phantom round under this rule
    for n, row in enumerate(log):
        row = row.tolist()
        assert sorted(row) == list(range(R))
        moved = [k for k in range(R) if row[k] != k]
        assert all(abs(row[k] - k) == 1 and min(row[k], k) % 2 == n % 2 and row[row[k]] == k for k in moved), n
    final = []
    Lr = sc.replay_rule1(T, a["tr"]["likeh"], a["tr"]["accept"], a["state"]["num_accepted"], a["lik0"], S, SI, tape, dtype=np.float32,
                         src_log=log, final=final)
    assert np.array_equal(np.array(final, dtype=np.float32), a["state"]["likelihood"])     # the replay holds the device's own numbers
    nsw, worst, skipped = 0, math.inf, []
    for n, L in enumerate(Lr):
        u = tape.swap_uniforms(n, R - 1)
        m = sc.rule1_margin(L, T, u, n)
        if m < sc.RULE1_MARGIN_UNITS:
            skipped.append(n)
            nsw += sum(1 for k in range(R - 1) if log[n][k] == k + 1)
            continue
        worst = min(worst, m)
        src, k = sc.rule1_round(L, T, u, n)
        assert log[n].tolist() == src, (R, n, m)
        nsw += k
    print(f"even/odd R = {R}: worst margin {worst:.3g} rule-1 units, rounds below the margin {skipped}")
    assert 10 * len(skipped) <= len(Lr), skipped
    assert a["stats"] == (nsw, sum((R - (n & 1)) // 2 for n in range(4)), 4) and nsw > 0, (a["stats"], nsw)
