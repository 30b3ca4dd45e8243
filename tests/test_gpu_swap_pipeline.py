"""Pipelined swap rounds (swap_handoff in csrc/ptnn_dev_kernels.hpp: replica k posts its row into a ring of four rounds and waits for
replicas 0 .. k+1 only) against the grid-barrier rounds ($PTNN_SWAP_PIPELINE=0) and against one launch per interval + swap_kernel
($PTNN_PERSISTENT=0).  The round changes no arithmetic, so everything is compared bit for bit: every trace array, the swap log, the
swap counters and every entry of state().  describe() says which path a run took."""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

DS = None
ENV = {"interval": {"PTNN_PERSISTENT": "0"}, "barrier": {"PTNN_SWAP_PIPELINE": "0"}, "default": {}}
SWAP_ROUNDS = {"interval": "between launches", "barrier": "grid barrier", "default": "pipelined (ring 4)"}
_REFERENCE = {}


def ds():
    global DS
    if DS is None:
        DS = parity.datasets()
    return DS


def run(monkeypatch, mode, R, S, si, *, chunks=False, delay=None, name="sunspot", topo=(4, 5, 1), expect=None, adapt=False, **kw):
    """One run of `mode` (a key of ENV); returns (traces, swap_log, swap_stats, state, describe)."""
    from ptnn_amd import ladder, philox
    for var in ("PTNN_PERSISTENT", "PTNN_SWAP_PIPELINE", "PTNN_SWAP_DELAY"):
        monkeypatch.delenv(var, raising=False)
    for var, val in ENV[mode].items():
        monkeypatch.setenv(var, val)
    if delay is not None:
        monkeypatch.setenv("PTNN_SWAP_DELAY", delay)
    d = ds()
    s = parity.make_sampler(0, topo, d[name + "_train"], d[name + "_test"], R_local=R, R_global=R, first=0, S=S, si=si, use_lg=True,
                            lr=0.1, seed=7, **kw)
    Pw = topo[0] * topo[1] + topo[1] * topo[2] + topo[1] + topo[2]
    T = ladder.temperatures(R, 2)
    s.set_state(np.stack([philox.initial_weights(7, r, Pw) for r in range(R)]), T)
    if kw.get("swap_rule") or kw.get("label_swap"):
        s.set_ladder(T)
    if adapt:
        s.set_ladder_adaptation(3, 0.5, 20.0)
    desc = s.describe()
    want = expect if expect is not None else SWAP_ROUNDS[mode]
    assert desc["swap_rounds"] == want, (mode, desc)
    assert desc["swap_ring_depth"] == (4 if want.startswith("pipelined") else 0), desc
    if chunks:
        s.run(si + 7)
        s.run(2 * si)
    s.run(-1)
    s.sync()                                                # raises when the launch set its error flag (a bounded wait ran out)
    out = (s.traces(), s.swap_log(), s.swap_stats(), s.state(), desc)
    s.close()
    return out


def reference(monkeypatch, R, S, si, **kw):
    """The run of one launch per interval, computed once per shape and shared."""
    key = (R, S, si, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        _REFERENCE[key] = run(monkeypatch, "interval", R, S, si, **kw)
    return _REFERENCE[key]


def same(got, want, label):
    for k in want[0]:
        assert np.array_equal(got[0][k], want[0][k]), (label, "trace", k)
    assert np.array_equal(got[1], want[1]), (label, "swap_log")
    assert got[2] == want[2], (label, "swap_stats", got[2], want[2])
    for k in want[3]:
        assert np.array_equal(got[3][k], want[3][k]), (label, "state", k)


@pytest.mark.parametrize("chunks", [False, True])
def test_existing_shape_in_one_piece_and_in_chunks(chunks, monkeypatch):
    """R = 16, S = 163, si = 20; the chunks si + 7, 2 si, rest end inside an interval: every launch starts its round count, its
    counters and its ring anew."""
    want = reference(monkeypatch, 16, 163, 20)
    assert want[2][0] > 0                                    # swaps happened
    assert "segment_pack_kernel<0,4,1,5>" in want[4]["kernel"]
    for mode in ("barrier", "default"):
        same(run(monkeypatch, mode, 16, 163, 20, chunks=chunks), want, (mode, chunks))


@pytest.mark.parametrize("R", [2, 3, 70])
def test_ladder_ends_and_more_than_a_wave_of_replicas(R, monkeypatch):
    """R = 2, 3: k + 1 is clipped at the top of the ladder, and with R = 3 only the middle replica has a prefix of its own.
    R = 70: the poll and the cascade cross a 64-lane chunk, and the 8 rounds wrap the ring of 4 twice."""
    want = reference(monkeypatch, R, 83, 10)
    assert want[2][2] >= 8 and want[2][0] > 0, want[2]
    for mode in ("barrier", "default"):
        same(run(monkeypatch, mode, R, 83, 10), want, (mode, R))


def test_shortest_interval_the_persistent_launch_takes(monkeypatch):
    """si = 8 (10 rounds): the shortest interval that runs in one launch; shorter ones keep one launch per interval on both paths."""
    want = reference(monkeypatch, 16, 83, 8)
    for mode in ("barrier", "default"):
        same(run(monkeypatch, mode, 16, 83, 8), want, mode)


@pytest.mark.parametrize("straggler", [15, 0, 7])
def test_one_replica_held_back_every_round(straggler, monkeypatch):
    """$PTNN_SWAP_DELAY: one replica posts every round about five intervals late (200 us; an interval of 10 steps is one to three
    windows of 18 us).  Held back at the top (15), replicas 0 .. 13 run ahead until the ring's back-pressure stops them; held back at
    the bottom (0), it gates everybody; in the middle (7), the lower half runs ahead of the upper.  A stale ring slot or a missing
    fence shows as a different chain; a wait that ran out would raise in sync()."""
    want = reference(monkeypatch, 16, 83, 10)
    for mode in ("barrier", "default"):
        same(run(monkeypatch, mode, 16, 83, 10, delay=f"{straggler}:200"), want, (mode, straggler))


@pytest.mark.parametrize("case", ["swap_rule", "label_swap", "adaptation"])
def test_rounds_that_stay_at_the_grid_barrier(case, monkeypatch):
    """Even/odd exchange, label swapping and ladder adaptation (it needs the whole round's statistics) keep the barrier."""
    kw = dict(label_swap=1) if case == "label_swap" else dict(swap_rule=1)
    adapt = case == "adaptation"
    want = run(monkeypatch, "interval", 16, 83, 10, adapt=adapt, **kw)
    same(run(monkeypatch, "default", 16, 83, 10, adapt=adapt, expect="grid barrier", **kw), want, case)


def test_mackey_glass_keeps_its_own_rounds(monkeypatch):
    """4-10-1 over several CUs per replica (segment_packm_kernel) exchanges granules inside its body: unchanged."""
    kw = dict(name="mackey", topo=(4, 10, 1))
    want = run(monkeypatch, "interval", 16, 83, 10, **kw)
    got = run(monkeypatch, "default", 16, 83, 10, expect="in-kernel exchange", **kw)
    assert "segment_packm_kernel" in got[4]["kernel"]
    same(got, want, "mackey")
