"""The edges of a packed window's SGD epochs -- the proposal elements read in front of the hand-scheduled row loop, the rows
behind it, the write-out -- and the operand reads of the Metropolis-Hastings verdict, against the cooperative schedule at one
wave per replica, which forms none of them that way: every trace, the final state and the swap statistics bit for bit.

Sunspot rows, 4 replicas, 200 samples, swaps every 20, Langevin p = 0.5, seed 78.  The cases are the smallest that reach every
path of those edges:
  training rows 3, 4, 7, 8, 13, 26, 30 (4-5-1, eight waves): no pass of the row loop; its four-row pass alone; 4 + 3 generic
    rows; one eight-row pass and no tail; 8 + 4 + 1; three passes + a tail of 2, as Sunspot's 298 = 8 x 37 + 2; three passes +
    the four-row pass + a tail of 2 (ptnn_set_data takes 3 rows: nothing had to start higher);
  topologies at 26 rows: 4-1-1 (seven dead lanes per group, lane 0 holds the unit and B2; P = 7), 4-5-1, 4-8-1 (no dead lane,
    P = 49: all four 16-lane rows of the verdict's sum hold data), 4-10-1 (16-lane groups, whichever packed kernel the plan
    resolves to);
  four-wave work-groups for 4-5-1, and both noise modes for 4-5-1.

A swap interval of 20 cuts the windows below 16 slots.  The kernel's window rule is replayed from the accept trace as in
test_gpu_pack_tail.py, and every run of 16-slot windows must contain windows of fewer than 8 slots (the second sweep wave has
no group) and of 9 to 15 (it is partly filled)."""
import functools

import numpy as np
import pytest

import parity
from parity import orc

pytestmark = pytest.mark.gpu

R, S, SI, SEED = 4, 200, 20, 78
SWITCH = int(S * 0.6)                                   # parity.make_sampler: pt_switch_step = 0.6 S
TRACES = ("pos_w", "likeh", "rmse_train", "rmse_test", "accept")
STATE = ("w", "eta", "likelihood", "prior", "num_accepted", "langevin_count", "langevin_accepted")
BASE_ROWS = 26

CASES = [pytest.param((4, 5, 1), 8, 0, n, id=f"4-5-1-w8-rows{n}") for n in (3, 4, 7, 8, 13, 26, 30)] + [
    pytest.param((4, 1, 1), 8, 0, BASE_ROWS, id="4-1-1-w8"),
    pytest.param((4, 8, 1), 8, 0, BASE_ROWS, id="4-8-1-w8"),
    pytest.param((4, 10, 1), 0, 0, BASE_ROWS, id="4-10-1"),
    pytest.param((4, 5, 1), 4, 0, BASE_ROWS, id="4-5-1-w4"),
    pytest.param((4, 5, 1), 8, 1, BASE_ROWS, id="4-5-1-w8-shared-noise"),
]


def make(topo, noise, ntr, schedule, waves):
    d = parity.datasets()
    P = orc.num_param(topo)
    tape = orc.PhiloxTape(SEED)
    w0 = np.stack([tape.w_init(r, P) for r in range(R)]).astype(np.float32)
    s = parity.make_sampler(0, topo, d["sunspot_train"][:ntr], d["sunspot_test"], R_local=R, R_global=R, first=0, S=S, si=SI,
                            use_lg=True, lr=0.1, seed=SEED, l_prob=0.5, waves=waves, schedule=schedule, shared_noise=noise)
    s.set_state(w0, np.array(orc.temperature_ladder(R, 2), dtype=np.float32))
    return s


def whole_run(s):
    s.run(-1)
    s.sync()
    got = (s.traces(), s.state(), s.swap_stats())
    s.close()
    return got


@functools.lru_cache(maxsize=None)
def reference(topo, noise, ntr):
    """The same configuration under the cooperative schedule, one wave per replica; computed once per configuration and never
    written to."""
    tr, st, sw = whole_run(make(topo, noise, ntr, 1, 1))
    for a in list(tr.values()) + list(st.values()):
        if a is not None:
            a.setflags(write=False)
    return tr, st, sw


def same(got, ref, label):
    tr, st, sw = got
    for k in TRACES:
        assert tr[k].shape == ref[0][k].shape and (tr[k] == ref[0][k]).all(), (label, k)
    for k in STATE:
        assert (st[k] == ref[1][k]).all(), (label, k)
    assert sw == ref[2], label


def interval_end(i):
    """One past the last step of the swap interval that holds step i: the first interval is steps 0 .. si, the run has S - 1."""
    return min((max(i, 1) + SI - 1) // SI * SI + 1, S - 1)


def accept_flags(accept, num_accepted):
    """accept[r, i + 1] counts the steps replica r accepted before step i, num_accepted after the last: -> flags [R, S - 1]."""
    counts = np.concatenate([accept[:, 1:], np.asarray(num_accepted).reshape(-1, 1)], axis=1).astype(np.int64)
    flags = np.diff(counts, axis=1)
    assert ((flags == 0) | (flags == 1)).all()
    return flags


def windows(flags, slots):
    """The kernel's window rule on one replica's accept flags (one per step) -> [(slots, first accepted slot or -1)]."""
    out, i = [], 0
    while i < S - 1:
        kt = min(slots, interval_end(i) - i)
        if SWITCH > i:
            kt = min(kt, SWITCH - i)
        acc = np.flatnonzero(flags[i:i + kt])
        m = int(acc[0]) if acc.size else -1
        out.append((kt, m))
        i += m + 1 if m >= 0 else kt
    return out


def check_windows(accept, num_accepted, slots, label):
    flags = accept_flags(accept, num_accepted)
    w = [x for r in range(R) for x in windows(flags[r], slots)]
    assert sum(kt if m < 0 else m + 1 for kt, m in w) == R * (S - 1), label
    if slots == 16:                                     # two sweep waves of eight lane groups each
        have = {
            "fewer than 8 slots": any(kt < 8 for kt, m in w),
            "9 to 15 slots": any(9 <= kt <= 15 for kt, m in w),
            "16 slots": any(kt == 16 for kt, m in w),
        }
        assert all(have.values()), (label, have)


@pytest.mark.parametrize("topo,waves,noise,ntr", CASES)
def test_packed_edges_commit_the_cooperative_chain(topo, waves, noise, ntr):
    s = make(topo, noise, ntr, 3, waves)
    info = s.describe()
    assert info["kernel"].startswith("ptnn::segment_pack"), info
    if topo[1] <= 8:
        assert info["kernel"].startswith("ptnn::segment_pack_kernel") and info["slots_per_round"] == 16, info
    got = whole_run(s)
    label = (topo, waves, noise, ntr)
    same(got, reference(topo, noise, ntr), label)
    check_windows(got[0]["accept"], got[1]["num_accepted"], info["slots_per_round"], label)
