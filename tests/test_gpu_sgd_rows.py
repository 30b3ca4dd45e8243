"""The SGD row loop of the 4-H-1 nets (sweep_rows_reg41) held BIT FOR BIT to the outputs recorded before its scalar side was
rescheduled (tests/golden/sgd_rows_parent.npz, written by profiles/tools/record_sgd_rows.py on the commit before that change):
the loop may move scalar loads, waits and branches, never a floating-point operation or its order.

Epoch bits: Sampler.langevin_gradient for 4-5-1 / 4-10-1, lr 0.1 / 0.01, 8 weight vectors, training sets of the first Ntr rows
with Ntr such that the 8-row pass runs zero, one and several times, the 4-row pass is present and absent, the generic remainder
has 0 and 3 rows, and the SGPR ring of rows wraps.  The same outputs are also held to the float64 oracle, so a golden recorded
from a broken build fails here on its own account.
Chain bits: whole packed / packed-multi-CU runs (traces and final state)."""
import os

import numpy as np
import pytest

import parity
from parity import orc

pytestmark = pytest.mark.gpu

GOLDEN_FILE = "sgd_rows_parent.npz"
NTRS = (4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 27)       # ptnn_set_data accepts every one of them
EPOCH_CASES = [("sunspot", (4, 5, 1), 0.1), ("sunspot", (4, 5, 1), 0.01), ("mackey", (4, 10, 1), 0.1), ("mackey", (4, 10, 1), 0.01)]
# (key, data set, topology, schedule, groups, shared_noise, the schedule describe() must report)
CHAIN_CASES = [("pack_own", "sunspot", (4, 5, 1), 3, 0, 0, "segment_pack_kernel"),
               ("pack_shared", "sunspot", (4, 5, 1), 3, 0, 1, "segment_pack_kernel"),
               ("packm_own", "mackey", (4, 10, 1), 3, 2, 0, "segment_packm_kernel"),
               ("packm_shared", "mackey", (4, 10, 1), 3, 2, 1, "segment_packm_kernel")]
CHAIN_R, CHAIN_S, CHAIN_SI, CHAIN_NTR, CHAIN_SEED = 4, 60, 20, 27, 77
TRACE_KEYS = ("pos_w", "likeh", "accept")
STATE_KEYS = ("w", "eta", "likelihood", "prior", "num_accepted", "langevin_count", "langevin_accepted")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def epoch_key(name, topo, lr, ntr):
    return f"epoch_{name}_{topo[1]}_lr{lr}_n{ntr}"


def epoch_weights(topo):
    from ptnn_amd import philox
    P = orc.num_param(topo)
    return np.stack([philox.initial_weights(5, r, P) for r in range(8)]).astype(np.float32)


def run_epochs(name, topo, lr):
    """{Ntr: langevin_gradient of the 8 weight vectors [8, P] float32} on training sets of the first Ntr rows."""
    d = parity.datasets()
    train, test = d[name + "_train"], d[name + "_test"]
    w = epoch_weights(topo)
    out = {}
    for ntr in NTRS:
        s = parity.make_sampler(orc.TASK_REG, topo, train[:ntr], test, R_local=2, R_global=2, first=0, S=10, si=100, use_lg=True,
                                lr=lr, seed=3)
        out[ntr] = s.langevin_gradient(w).copy()
        s.close()
    return w, out


def run_chain(case):
    """Traces and final state of one packed run; checks that describe() reports the schedule the case is about."""
    _, name, topo, schedule, groups, shared, kernel = case
    d = parity.datasets()
    P = orc.num_param(topo)
    tape = orc.PhiloxTape(CHAIN_SEED)
    w0 = np.stack([tape.w_init(r, P) for r in range(CHAIN_R)]).astype(np.float32)
    T = np.array(orc.temperature_ladder(CHAIN_R, 2), dtype=np.float32)
    s = parity.make_sampler(orc.TASK_REG, topo, d[name + "_train"][:CHAIN_NTR], d[name + "_test"], R_local=CHAIN_R, R_global=CHAIN_R,
                            first=0, S=CHAIN_S, si=CHAIN_SI, use_lg=True, lr=0.1, seed=CHAIN_SEED, l_prob=0.5, schedule=schedule,
                            groups=groups, shared_noise=shared)
    info = s.describe()
    assert info["schedule"] == "packed-speculative" and info["kernel"].startswith("ptnn::" + kernel), info
    if groups:
        assert info["groups_per_replica"] == groups, info
    s.set_state(w0, T)
    s.run(-1)
    s.sync()
    tr, st = s.traces(), s.state()
    s.close()
    return w0, {k: tr[k] for k in TRACE_KEYS}, {k: st[k] for k in STATE_KEYS}


def record():
    """Everything the golden file holds: inputs as they are, outputs as uint32 bit patterns."""
    rec = {"ntrs": np.array(NTRS, np.int32)}
    for name, topo, lr in EPOCH_CASES:
        w, out = run_epochs(name, topo, lr)
        rec[f"epoch_w_{topo[1]}"] = w
        for ntr, v in out.items():
            rec[epoch_key(name, topo, lr, ntr)] = bits(v)
    for case in CHAIN_CASES:
        w0, tr, st = run_chain(case)
        rec[f"chain_{case[0]}_w0"] = w0
        for k, v in tr.items():
            rec[f"chain_{case[0]}_trace_{k}"] = bits(v)
        for k, v in st.items():
            rec[f"chain_{case[0]}_state_{k}"] = bits(v)
    return rec


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = parity.golden(GOLDEN_FILE)
    return _GOLDEN


@pytest.mark.parametrize("name,topo,lr", EPOCH_CASES, ids=[f"{n}-{t[1]}-lr{lr}" for n, t, lr in EPOCH_CASES])
def test_epoch_bits_equal_the_parent_commit(name, topo, lr):
    g = golden()
    d = parity.datasets()
    train = d[name + "_train"]
    w, out = run_epochs(name, topo, lr)
    assert (bits(w) == bits(g[f"epoch_w_{topo[1]}"])).all(), "the inputs are not the recorded ones"
    for ntr in NTRS:
        got, want = bits(out[ntr]), g[epoch_key(name, topo, lr, ntr)]
        assert got.shape == want.shape
        diff = np.argwhere(got != want)
        assert diff.size == 0, f"{name} H={topo[1]} lr={lr} Ntr={ntr}: {len(diff)} of {got.size} words differ, first at {diff[0]}"
        # ... and the float64 oracle at the tolerance of test_sgd_epoch_row_counts_and_lane_groups: a golden recorded from a broken
        # build does not pass
        for k in range(w.shape[0]):
            ref = orc.langevin_gradient(train[:ntr], w[k].astype(np.float64), topo, lr, orc.TASK_REG)
            np.testing.assert_allclose(out[ntr][k], ref, rtol=1e-4, atol=2e-5, err_msg=f"{name} H={topo[1]} lr={lr} Ntr={ntr} w{k}")


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_chain_bits_equal_the_parent_commit(case):
    g = golden()
    w0, tr, st = run_chain(case)
    assert (bits(w0) == bits(g[f"chain_{case[0]}_w0"])).all(), "the inputs are not the recorded ones"
    assert tr["accept"].sum() > 0 and st["langevin_count"].sum() > 0, "the run took no Langevin step: it does not exercise the epoch"
    for k, v in tr.items():
        got, want = bits(v), g[f"chain_{case[0]}_trace_{k}"]
        assert got.shape == want.shape and (got == want).all(), (case[0], "trace", k, int((got != want).sum()))
    for k, v in st.items():
        got, want = bits(v), g[f"chain_{case[0]}_state_{k}"]
        assert got.shape == want.shape and (got == want).all(), (case[0], "state", k, int((got != want).sum()))
