"""What the one-CU packed kernel keeps in LDS across a pipelined swap round (segment_pack_body behind swap_handoff,
csrc/ptnn_dev_pack.hpp, ptnn_dev_kernels.hpp): the data image is staged once per launch, the random tape ring and ring_hi are
carried from one interval into the next, the hand-off's scratch lies in the body's slot area, and the round's uniforms are drawn
ahead of the wait.  None of it changes an operand of a floating-point operation, so a run with the pipelined rounds in one launch
is compared bit for bit (as 32-bit patterns) with one launch per interval ($PTNN_PERSISTENT=0: every interval stages and draws
everything anew) and with the grid-barrier rounds ($PTNN_SWAP_PIPELINE=0: one launch, everything rebuilt behind every round):
every trace array, the scalar rows with log alpha, pos_w, the final state, the cached gradient and its flag, the last recorded row,
the float and int state words, the counters, the swap log and the swap statistics.

S = 101 (no temperature switch: 0.6 S is no whole step) with intervals of 8 (12 rounds, three turns of the ring of four) and of 20
(the intervals end in the middle of the tape ring of 32 steps).  Shapes, the smallest at which each part can go wrong:
  4-5-1 and 5-5-1 (hidden width compiled in) and 4-8-1 (run-time width);
  7 and 30 training rows with 3 test rows: an image of 96 / 264 floats, smaller than the 3 R + 1 = 211 words of scratch at R = 70,
    which would reach over the image into the state rows if it still lay at the base of LDS;
  R = 2, 3 (the ladder's ends), 16, 70 (more than a wave of replicas), and 350 on four waves: 1051 words do not fit into the slot
    area of a 4-5-1 net (1024), so the scratch stays on the image and its prefix is staged again on every entry;
  Langevin and random-walk proposals (without epochs every wave refills the ring), own and shared noise, eight and four waves;
  a run cut by run() at a step that is no multiple of the interval: the second launch enters in the middle of an interval with a
    ring that holds nothing;
  $PTNN_SWAP_DELAY holding back replica 0, 7 or R - 1 by about five intervals in every round."""
import numpy as np
import pytest

import parity
from parity import orc
from test_gpu_pack_fixed_h import SEED, finished, same

pytestmark = pytest.mark.gpu

ENV = {"interval": {"PTNN_PERSISTENT": "0"}, "barrier": {"PTNN_SWAP_PIPELINE": "0"}, "pipelined": {}}
SWAP_ROUNDS = {"interval": "between launches", "barrier": "grid barrier", "pipelined": "pipelined (ring 4)"}
S, NTE = 101, 3
_REFERENCE = {}

#                                   topology   waves lg   noise rows R  si
CASES = {
    "4-5-1-rows30-r16-si20": ((4, 5, 1), 8, True, 0, 30, 16, 20),
    "4-5-1-rows7-r70-si8": ((4, 5, 1), 8, True, 0, 7, 70, 8),
    "4-5-1-rows30-r3-si8-w4-shared-noise": ((4, 5, 1), 4, True, 1, 30, 3, 8),
    "4-5-1-rows7-r350-si20-w4": ((4, 5, 1), 4, True, 0, 7, 350, 20),
    "4-5-1-random-walk-rows30-r16-si8": ((4, 5, 1), 8, False, 0, 30, 16, 8),
    "4-5-1-random-walk-rows7-r3-si20-w4-shared-noise": ((4, 5, 1), 4, False, 1, 7, 3, 20),
    "5-5-1-rows7-r3-si8-w4-shared-noise": ((5, 5, 1), 4, True, 1, 7, 3, 8),
    "5-5-1-rows30-r16-si20": ((5, 5, 1), 8, True, 0, 30, 16, 20),
    "5-5-1-random-walk-rows30-r2-si20": ((5, 5, 1), 8, False, 0, 30, 2, 20),
    "4-8-1-rows30-r2-si20": ((4, 8, 1), 8, True, 0, 30, 2, 20),
    "4-8-1-rows7-r70-si20-w4": ((4, 8, 1), 4, True, 0, 7, 70, 20),
    "4-8-1-random-walk-rows7-r16-si8-shared-noise": ((4, 8, 1), 8, False, 1, 7, 16, 8),
}
KERNEL = {(4, 5, 1): "segment_pack_kernel<0,4,1,5>", (5, 5, 1): "segment_pack_kernel<0,5,1,5>", (4, 8, 1): "segment_pack_kernel<0,4,1>"}


def run(monkeypatch, mode, case, *, chunk=0, delay=None):
    """One finished run of `mode` (a key of ENV): (everything it leaves behind as 32-bit patterns, swap statistics)."""
    topo, waves, lg, noise, ntr, R, si = case
    with monkeypatch.context() as m:
        for var in ("PTNN_PERSISTENT", "PTNN_SWAP_PIPELINE", "PTNN_SWAP_DELAY", "PTNN_PACK_FIXED_H"):
            m.delenv(var, raising=False)
        for var, val in ENV[mode].items():
            m.setenv(var, val)
        if delay is not None:
            m.setenv("PTNN_SWAP_DELAY", delay)
        d = parity.datasets()
        name = "sunspot5" if topo[0] == 5 else "sunspot"
        P = orc.num_param(topo)
        tape = orc.PhiloxTape(SEED)
        w0 = np.stack([tape.w_init(r, P) for r in range(R)]).astype(np.float32)
        s = parity.make_sampler(0, topo, d[name + "_train"][:ntr], d[name + "_test"][:NTE], R_local=R, R_global=R, first=0, S=S, si=si,
                                use_lg=lg, lr=0.1, seed=SEED, l_prob=0.5, waves=waves, schedule=3, shared_noise=noise)
        s.set_state(w0, np.array(orc.temperature_ladder(R, 2), dtype=np.float32))
        info = s.describe()
        assert info["swap_rounds"] == SWAP_ROUNDS[mode], (mode, info)
        assert info["kernel"] == "ptnn::" + KERNEL[topo] and info["block_threads"] == 64 * waves, info
        return finished(s, R, S, si, chunk)               # sync() raises when a bounded wait of the launch ran out


def reference(monkeypatch, case):
    """One launch per interval, computed once per case and shared."""
    if case not in _REFERENCE:
        _REFERENCE[case] = run(monkeypatch, "interval", case)
        swaps, _, rounds = _REFERENCE[case][1]
        assert rounds == (S - 1) // case[6] and (case[5] < 16 or swaps > 0), _REFERENCE[case][1]     # on a ladder of 16 or more some swap happened
    return _REFERENCE[case]


@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_against_one_launch_per_interval(name, monkeypatch):
    want = reference(monkeypatch, CASES[name])
    for mode in ("barrier", "pipelined"):
        same(run(monkeypatch, mode, CASES[name]), want, (name, mode))


@pytest.mark.parametrize("name,chunk", [("4-5-1-rows30-r16-si20", 27), ("4-8-1-rows7-r70-si20-w4", 53), ("5-5-1-rows7-r3-si8-w4-shared-noise", 13),
                                        ("4-5-1-random-walk-rows30-r16-si8", 35)])
def test_second_launch_enters_inside_an_interval(name, chunk, monkeypatch):
    """run(chunk), run(rest): the second launch's first entry lies inside an interval and finds no ring; it fills all of it."""
    assert chunk % CASES[name][6] not in (0, 1, CASES[name][6] - 1)
    want = reference(monkeypatch, CASES[name])
    for mode in ("barrier", "pipelined"):
        same(run(monkeypatch, mode, CASES[name], chunk=chunk), want, (name, mode, chunk))


@pytest.mark.parametrize("name,straggler", [("4-5-1-rows30-r16-si20", 0), ("4-5-1-rows30-r16-si20", 7), ("4-5-1-rows30-r16-si20", 15),
                                            ("4-8-1-random-walk-rows7-r16-si8-shared-noise", 7), ("4-5-1-rows7-r70-si8", 69)])
def test_one_replica_held_back_every_round(name, straggler, monkeypatch):
    """The straggler posts 200 us late in every round: the others sit in the wait with their uniforms drawn and their scratch in the
    slot area, and those below it run up to four rounds ahead with rings of their own."""
    want = reference(monkeypatch, CASES[name])
    same(run(monkeypatch, "pipelined", CASES[name], delay=f"{straggler}:200"), want, (name, straggler))
