"""The packed kernels with the hidden width compiled in (segment_pack_kernel<T, I, O, 5>: 4-5-1 and 5-5-1; over several CUs
segment_packm_kernel<0, 4, 1, 10>: 4-10-1) against the same kernels with the width as a run-time value ($PTNN_PACK_FIXED_H=0): the two differ in loop bounds, guards and addresses that are
literals in one and registers in the other, never in a floating-point operation, so every trace (the scalar rows with log alpha,
pos_w), the final state, the cached gradient, the counters and the swap statistics agree bit for bit, NaNs and signed zeros
included (compared as 32-bit patterns).

Sunspot rows (sunspot5 for five inputs), 2 - 4 replicas, 40 - 130 samples with the 0.6 S temperature switch and swap intervals
of 8 - 13 steps, so that every run holds several swap rounds and windows cut at an interval's end and at the switch.  The cases
are the smallest that reach every path on which a literal replaced a register:
  training rows 3, 4, 7, 8, 13, 30 (the edges of the SGD row loop: no pass; the four-row pass alone; 4 + 3; one eight-row pass;
    8 + 4 + 1; three passes + the four-row pass + a tail of 2);
  eight and four waves (four and two forward waves write the trace rows);
  Langevin and random-walk proposals (without epochs all waves run forward passes and write trace rows before the barrier);
  own and shared noise; one launch per run and one per swap interval ($PTNN_PERSISTENT=0);
  a run in two chunks, so that a launch starts from saved state in the middle of an interval;
  4-10-1 over four CUs per replica (the automatic choice) and over two: windows of 32 and 16 steps, whose verdicts and accepted
    steps cross CUs, with the swap rounds inside the launch and one launch per interval.
The dispatch case creates handles of 4, 5 and 8 hidden units side by side: only the 5 may take the fixed-width kernel, and each
commits the chain of the cooperative schedule at one wave per replica."""
import struct

import numpy as np
import pytest

import parity
from parity import orc

pytestmark = pytest.mark.gpu

SEED = 78
TRACES = ("pos_w", "likeh", "rmse_train", "rmse_test", "acc_train", "acc_test", "accept")
STATE = ("w", "eta", "likelihood", "prior", "num_accepted", "langevin_count", "langevin_accepted")
CHAIN = ("pos_w", "likeh", "rmse_train", "rmse_test", "accept") + STATE
SF_COUNT, SI_COUNT = 8, 4                               # per-replica float / int state words of a checkpoint

#                 topology   waves lg  noise rows R  S    si  persistent chunk
CASES = {
    "rows3": ((4, 5, 1), 8, True, 0, 3, 4, 60, 10, True, 0),
    "rows4": ((4, 5, 1), 8, True, 0, 4, 3, 50, 8, True, 0),
    "rows7": ((4, 5, 1), 8, True, 0, 7, 4, 60, 10, True, 0),
    "rows8": ((4, 5, 1), 8, True, 0, 8, 2, 40, 8, True, 0),
    "rows13": ((4, 5, 1), 8, True, 0, 13, 4, 60, 10, True, 0),
    "rows30": ((4, 5, 1), 8, True, 0, 30, 4, 130, 13, True, 0),
    "rows30-w4": ((4, 5, 1), 4, True, 0, 30, 4, 60, 10, True, 0),
    "rows13-shared-noise": ((4, 5, 1), 8, True, 1, 13, 3, 60, 10, True, 0),
    "rows30-launch-per-interval": ((4, 5, 1), 8, True, 0, 30, 4, 60, 10, False, 0),
    "rows13-two-chunks": ((4, 5, 1), 8, True, 0, 13, 4, 60, 10, True, 23),
    "rows30-two-chunks-launch-per-interval": ((4, 5, 1), 4, True, 1, 30, 2, 50, 8, False, 17),
    "random-walk-w8": ((4, 5, 1), 8, False, 0, 13, 4, 60, 10, True, 0),
    "random-walk-w4-shared-noise": ((4, 5, 1), 4, False, 1, 30, 3, 50, 8, True, 0),
    "5-5-1-rows30": ((5, 5, 1), 8, True, 0, 30, 4, 60, 10, True, 0),
    "5-5-1-rows7-w4-shared-noise": ((5, 5, 1), 4, True, 1, 7, 3, 50, 8, True, 0),
    "5-5-1-rows13-launch-per-interval-two-chunks": ((5, 5, 1), 8, True, 0, 13, 2, 40, 8, False, 11),
    "5-5-1-random-walk": ((5, 5, 1), 8, False, 0, 8, 4, 60, 10, True, 0),
}


def make(topo, R, S, si, ntr, *, schedule=3, waves=0, use_lg=True, noise=0, groups=0):
    d = parity.datasets()
    name = "sunspot5" if topo[0] == 5 else "sunspot"
    P = orc.num_param(topo)
    tape = orc.PhiloxTape(SEED)
    w0 = np.stack([tape.w_init(r, P) for r in range(R)]).astype(np.float32)
    s = parity.make_sampler(0, topo, d[name + "_train"][:ntr], d[name + "_test"], R_local=R, R_global=R, first=0, S=S, si=si,
                            use_lg=use_lg, lr=0.1, seed=SEED, l_prob=0.5, waves=waves, schedule=schedule, shared_noise=noise, groups=groups)
    s.set_state(w0, np.array(orc.temperature_ladder(R, 2), dtype=np.float32))
    return s


def chain_words(s, R, S, si):
    """What a checkpoint holds beside the state vectors: the cached gradient and the last recorded row (their P elements), the
    float and int state words, the flag of the cached gradient and the swap counters."""
    blob = s.checkpoint()
    P = s.P
    PS = (P + 1 + 3) & ~3
    logr = min(s.swap_stats()[2], S // si + 2)
    nf, ni = 3 * R * PS + R * SF_COUNT + R + 5 * R, R + R * SI_COUNT + logr * R + 2 * R
    head = len(blob) - 4 * (nf + ni)
    tail = struct.unpack("<8i2q", blob[head - 48:head])                # P, PS, cur, rounds, finalized, ladder, logged rounds, -, counters
    assert tail[0] == P and tail[1] == PS and tail[6] == logr, (tail, P, PS, logr)
    f = np.frombuffer(blob, np.uint32, nf, head)
    i = np.frombuffer(blob, np.int32, ni, head + 4 * nf)
    vec = f[:3 * R * PS].reshape(3, R, PS)
    return dict(gd_w=vec[1][:, :P].copy(), rec_w=vec[2][:, :P].copy(), st_f=f[3 * R * PS:3 * R * PS + R * SF_COUNT].copy(),
                gd_valid=i[:R].copy(), st_i=i[R:R + R * SI_COUNT].copy(), counters=np.array(tail[8:]))


def finished(s, R, S, si, chunk=0):
    """Everything a finished run leaves behind, floats as their 32-bit patterns."""
    if chunk:
        s.run(chunk)
        s.sync()
        assert s.steps_done() == chunk
    s.run(-1)
    s.sync()
    tr = s.traces()
    out = {k: tr[k].view(np.uint32) for k in TRACES}
    out["rows"] = s.trace_rows(1, S - 1).view(np.uint32)                # likeh .. log alpha, source row of every MH step
    out.update({k: v.view(np.uint32) for k, v in s.state().items()})
    out.update(chain_words(s, R, S, si))
    out["swap_log"] = s.swap_log()
    stats = s.swap_stats()
    s.close()
    return out, stats


def same(a, b, label, keys=None):
    assert a[1] == b[1], (label, "swap statistics", a[1], b[1])
    assert a[0].keys() == b[0].keys()
    for k in keys or a[0]:
        x, y = np.asarray(a[0][k]), np.asarray(b[0][k])
        assert x.shape == y.shape and (x == y).all(), (label, k)


def kernel_of(s, slots=16):
    info = s.describe()
    assert info["schedule"] == "packed-speculative" and info["slots_per_round"] == slots, info
    return info["kernel"], info["launches"]


def fixed_against_run_time_width(monkeypatch, name, case, stem, width, groups=0):
    topo, waves, lg, noise, ntr, R, S, si, persistent, chunk = case
    assert S * 0.6 == int(S * 0.6) and si >= 8 and (S - 1) // si >= 2
    shape = f"{0},{topo[0]},{topo[2]}"
    slots, threads = (16, 64 * waves) if stem == "segment_pack_kernel" else (8 * (groups or 4), 512)
    runs = {}
    for fixed in (True, False):
        with monkeypatch.context() as m:
            if not fixed:
                m.setenv("PTNN_PACK_FIXED_H", "0")
            if not persistent:
                m.setenv("PTNN_PERSISTENT", "0")
            s = make(topo, R, S, si, ntr, waves=waves, use_lg=lg, noise=noise, groups=groups)
            kernel, launches = kernel_of(s, slots)
            assert kernel == f"ptnn::{stem}<{shape}{',' + str(width) if fixed else ''}>", (name, fixed, kernel)
            assert launches.startswith("one per ptnn_run" if persistent else "one per swap interval"), (name, launches)
            assert s.describe()["block_threads"] == threads
            runs[fixed] = finished(s, R, S, si, chunk)
    assert runs[True][1][2] >= 2, (name, "swap rounds", runs[True][1])
    if lg:
        assert runs[True][0]["langevin_count"].view(np.int32).sum() > 0, name
    same(runs[True], runs[False], name)


@pytest.mark.parametrize("name", list(CASES))
def test_fixed_width_kernel_commits_the_run_time_width_chain(name, monkeypatch):
    fixed_against_run_time_width(monkeypatch, name, CASES[name], "segment_pack_kernel", 5)


# the kernel over several CUs at 4-10-1 (16-lane groups, 8 slots per CU): four CUs per replica (the automatic choice) and two
#                 topology    waves lg  noise rows R  S   si  persistent chunk   CUs
CASES_SEVERAL = {
    "rows13-4cus": (((4, 10, 1), 0, True, 0, 13, 4, 60, 10, True, 0), 0),
    "rows30-2cus-shared-noise": (((4, 10, 1), 0, True, 1, 30, 3, 50, 8, True, 0), 2),
    "rows7-4cus-launch-per-interval-two-chunks": (((4, 10, 1), 0, True, 0, 7, 2, 40, 8, False, 11), 0),
    "rows30-4cus-two-chunks": (((4, 10, 1), 0, True, 0, 30, 4, 130, 13, True, 47), 4),
}


@pytest.mark.parametrize("name", list(CASES_SEVERAL))
def test_fixed_width_kernel_over_several_cus_commits_the_run_time_width_chain(name, monkeypatch):
    case, groups = CASES_SEVERAL[name]
    fixed_against_run_time_width(monkeypatch, name, case, "segment_packm_kernel", 10, groups)


def test_only_the_compiled_width_takes_the_fixed_kernel():
    """Handles of 4, 5 and 8 hidden units on shape (0, 4, 1), alive together: the list of the shape holds 5 alone."""
    R, S, si, ntr = 4, 60, 10, 13
    widths = (4, 5, 8)
    packed = {H: make((4, H, 1), R, S, si, ntr, waves=8) for H in widths}
    for H, s in packed.items():
        assert kernel_of(s)[0] == "ptnn::segment_pack_kernel<0,4,1" + (",5>" if H == 5 else ">"), (H, s.describe())
    got = {H: finished(packed[H], R, S, si) for H in widths}
    for H in widths:
        ref = make((4, H, 1), R, S, si, ntr, schedule=1, waves=1)
        assert ref.describe()["schedule"] == "cooperative" and ref.describe()["block_threads"] == 64, ref.describe()
        # the chain: what test_gpu_pack_edges.py holds the packed kernel to (the schedules cache gradients at different times)
        same(got[H], finished(ref, R, S, si), f"4-{H}-1 against the cooperative schedule", CHAIN)
