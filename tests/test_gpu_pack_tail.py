"""The tail of a packed window -- Metropolis-Hastings verdict, commit by the sweep waves, trace rows by the forward waves behind
the commit barrier -- against the cooperative schedule, which runs none of that code: every trace and the final state bit for bit.

Sunspot, first 27 training rows, 4 replicas, 400 samples, swaps every 20, Langevin p = 0.5, seed 78.  Topologies 4-5-1 and 4-8-1:
P = 31 and 49; at 49 the third and fourth 16-lane rows of |w - epoch(proposal)|^2 hold data, at 31 they are exact zeros.  Eight
waves per work-group (four forward waves write the trace rows) and four (two forward waves).

From the accept trace the kernel's window rule is replayed (16 slots, cut at the interval end and at the switch step), and every
base run must contain the windows that take the tail's different paths."""
import functools

import numpy as np
import pytest

import parity
from parity import orc

pytestmark = pytest.mark.gpu

R, S, SI, SEED, NTR, SLOTS = 4, 400, 20, 78, 27, 16
SWITCH = int(S * 0.6)                                   # parity.make_sampler: pt_switch_step = 0.6 S
TRACES = ("pos_w", "likeh", "rmse_train", "rmse_test", "accept")
STATE = ("w", "eta", "likelihood", "prior", "num_accepted", "langevin_count", "langevin_accepted")


def make(topo, noise, schedule, waves=0, use_lg=True, trace_capacity=0):
    d = parity.datasets()
    P = orc.num_param(topo)
    tape = orc.PhiloxTape(SEED)
    w0 = np.stack([tape.w_init(r, P) for r in range(R)]).astype(np.float32)
    s = parity.make_sampler(0, topo, d["sunspot_train"][:NTR], d["sunspot_test"], R_local=R, R_global=R, first=0, S=S, si=SI,
                            use_lg=use_lg, lr=0.1, seed=SEED, l_prob=0.5, waves=waves, schedule=schedule, shared_noise=noise,
                            trace_capacity=trace_capacity)
    s.set_state(w0, np.array(orc.temperature_ladder(R, 2), dtype=np.float32))
    return s


def packed(s):
    """The sampler, once it says that the packed kernel of one CU runs it."""
    info = s.describe()
    assert info["kernel"].startswith("ptnn::segment_pack_kernel") and info["slots_per_round"] == SLOTS, info
    return s


def whole_run(s):
    s.run(-1)
    s.sync()
    got = (s.traces(), s.state(), s.swap_stats())
    s.close()
    return got


@functools.lru_cache(maxsize=None)
def reference(topo, noise, use_lg=True):
    """The same configuration under the cooperative schedule, one wave per replica (with several its row sums associate
    otherwise and agree within round-off only); computed once per configuration and never written to."""
    tr, st, sw = whole_run(make(topo, noise, 1, waves=1, use_lg=use_lg))
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


def windows(flags):
    """The kernel's window rule on one replica's accept flags (one per step) -> [(slots, first accepted slot or -1)]."""
    out, i = [], 0
    while i < S - 1:
        kt = min(SLOTS, interval_end(i) - i)
        if SWITCH > i:
            kt = min(kt, SWITCH - i)
        acc = np.flatnonzero(flags[i:i + kt])
        m = int(acc[0]) if acc.size else -1
        out.append((kt, m))
        i += m + 1 if m >= 0 else kt
    return out


def check_windows(accept, num_accepted, label):
    flags = accept_flags(accept, num_accepted)
    w = [x for r in range(R) for x in windows(flags[r])]
    assert sum(kt if m < 0 else m + 1 for kt, m in w) == R * (S - 1), label
    have = {
        "first accepted slot 0": any(m == 0 for kt, m in w),
        "first accepted slot >= 12": any(m >= 12 for kt, m in w),
        "full window, none accepted": any(kt == SLOTS and m < 0 for kt, m in w),
        "partial window, none accepted": any(kt < SLOTS and m < 0 for kt, m in w),
        "partial window accepted in its last slot": any(kt < SLOTS and m == kt - 1 for kt, m in w),
    }
    assert all(have.values()), (label, have)


@pytest.mark.parametrize("noise", [0, 1], ids=["own-noise", "shared-noise"])
@pytest.mark.parametrize("topo,waves", [((4, 5, 1), 8), ((4, 8, 1), 8), ((4, 5, 1), 4)], ids=["4-5-1-w8", "4-8-1-w8", "4-5-1-w4"])
def test_packed_tail_commits_the_cooperative_chain(topo, waves, noise):
    got = whole_run(packed(make(topo, noise, 3, waves=waves)))
    same(got, reference(topo, noise), (topo, waves, noise))
    check_windows(got[0]["accept"], got[1]["num_accepted"], (topo, waves, noise))


def test_packed_tail_random_walk_only():
    """use_lg = False: every wave is a forward wave, nothing is summed, and every thread writes trace rows before the barrier."""
    same(whole_run(packed(make((4, 5, 1), 0, 3, waves=8, use_lg=False))), reference((4, 5, 1), 0, use_lg=False), "random walk")


def test_packed_tail_trace_ring_wraps():
    """trace_capacity = 64 < S: the trace position wraps inside windows; drained in chunks, the rows are the full traces."""
    cap = 64
    ref = reference((4, 5, 1), 0)
    s = packed(make((4, 5, 1), 0, 3, waves=8, trace_capacity=cap))
    parts, row, k = [], 0, 0
    chunks = [cap - 1, 7, cap - 1, 1, cap - 1]
    while s.steps_done() < S - 1:
        s.run(min(chunks[k % len(chunks)], S - 1 - s.steps_done()))
        k += 1
        s.sync()
        hi = s.steps_done() + 1
        parts.append(s.traces(row, hi - row))
        row = hi
    s.run(-1)
    s.sync()
    tr = {k_: np.concatenate([p[k_] for p in parts], axis=1) for k_ in TRACES}
    same((tr, s.state(), s.swap_stats()), ref, "trace ring")
    s.close()


def test_packed_tail_chunks_end_inside_intervals():
    """run(7) chunks against run(-1): most chunks end in the middle of an interval (all but those that end with steps 20, 160
    and 300) and cut a window there, so the trace rows of a chunk's last window must all have been stored when the launch ends."""
    s = packed(make((4, 5, 1), 0, 3, waves=8))
    while s.steps_done() < S - 1:
        s.run(min(7, S - 1 - s.steps_done()))
    same(whole_run(s), reference((4, 5, 1), 0), "chunks of 7")
