"""Rejected MH steps held to the identical-input bound, not only accepted ones (tests/parity.py: follow_device_run(ident_all=True)).

A synced follow compares an ACCEPTED step with the float64 oracle evaluated at the device's own recorded proposal -- identical
inputs, 4e-6 of the scale -- but a REJECTED step (98 % of a Sunspot run) leaves no proposal behind and was compared with the
oracle's own proposal half a float32 ulp away, 25 times looser.  The rejected steps are where the hand-scheduled kernels do their
special work: speculative slots evaluated from a base an earlier slot may replace, MH operands prefetched ahead of the verdict,
cached gradients reused after cross-slot moves, likelihoods left stale by a swap, the deciding epoch of the wide kernel.  Here the
device's proposal of EVERY step is rebuilt bit for bit -- w' = fmaf(step_w, noise, base), eta' = fmaf(step_eta, n_eta, eta) from
the library's own tape (ptnn_tape) and epoch (ptnn_langevin_gradient) and the common float32 state -- the oracle is evaluated there,
and the recorded log alpha and likeh of every step are held to the identical-input bound, under every schedule."""
import json
import os

import numpy as np
import pytest

import parity
from parity import orc  # noqa: F401

pytestmark = pytest.mark.gpu


def run_case(name, seed=None):
    """One IDENT_CASES entry on the device, followed with the identical-input class on every step.  -> report."""
    task, topo, dname, lg, lr, maxtemp, S, si, seed0, kw, want = parity.IDENT_CASES[name]
    seed = seed0 if seed is None else seed
    R = parity.IDENT_R
    assert R * S <= 1500 and si < S / 4 and int(0.6 * S) < S - 1
    pt, w0, train, test = parity.ident_case(name, seed)
    s = parity.make_sampler(task, topo, train, test, R_local=R, R_global=R, first=0, S=S, si=si, use_lg=lg, lr=lr, seed=seed, **kw)
    info = s.describe()
    assert want["schedule"] in info["schedule"] and want.get("kernel", "") in info["kernel"], info       # not silently another schedule
    assert all(info[k] == v for k, v in want.items() if k not in ("schedule", "kernel")), info
    temps = np.array(pt.temperatures, dtype=np.float32)
    eta0 = parity.device_startup_eta(s, w0, temps)
    s.set_state(w0, temps)
    s.run(-1)
    s.sync()
    tr = s.traces()
    rep = parity.follow_device_run(s, tr, pt, f"{name} ", ident_all=True, eta0=eta0)
    s.close()
    print(name, json.dumps(rep))
    if os.environ.get("PTNN_FOLLOW_REPORT"):
        with open(os.environ["PTNN_FOLLOW_REPORT"], "a") as f:
            f.write(json.dumps(dict(case=name, seed=seed, R=R, S=S, swap_interval=si, topology=list(topo), data=dname,
                                    schedule=info["schedule"], kernel=info["kernel"], **rep)) + "\n")
    return rep


@pytest.mark.parametrize("name", list(parity.IDENT_CASES))
def test_every_step_at_the_devices_own_proposal(name):
    task, topo, dname, lg, lr, maxtemp, S, si, seed, kw, want = parity.IDENT_CASES[name]
    R = parity.IDENT_R
    rep = run_case(name)
    if os.environ.get("PTNN_PARITY_PROBE"):
        return                                               # measurement mode: figures recorded, nothing judged
    by = rep["ident_all_by_class"]
    n = lambda *pre: sum(v["steps"] for k, v in by.items() if all(p in k for p in pre))       # noqa: E731
    # not vacuous: no step left out, and the classes the check exists for all occur
    assert rep["ident_all_steps"] == R * (S - 1) and rep["ident_all_over_bound"] == 0 and rep["ident_all_lik_over_bound"] == 0, rep
    assert n("rej", "fresh") >= 1 and n("rej", "stale") >= 1, by
    if lg:
        assert n("rej", "_lg") >= 1 and n("acc", "_lg") >= 1, by                     # accepted ones: the self-check of the rebuilt epoch
    assert rep["rebuild_accepted"] == rep["accepted"] >= 10, rep
