"""Cost of the ladder adaptation per swap round and the choice of its defaults.

cost: Sunspot 4-5-1, swap_rule 1, random-walk proposals, swap_interval 5, R = 64 / 256 / 1024 on one GPU.  The same fixed-seed
run with and without a spec (rounds = every round of the run).  These runs take one launch per interval and a swap_kernel per
round, so the segment time ptnn_kernel_time reports holds no swap round: run `--cost` under rocprofv3 --kernel-trace --stats
and reduce the two databases with `--reduce` (swap_kernel's mean duration per R; the "on" runs' kernels carry the adaptation,
the "off" ones do not).
defaults: random-walk regressions with 16 chains, maxtemp 1000, si = 5, burn_in 0.5 -- the 12-row 4-3-1 problem of
tests/test_gpu_evidence.py (S = 40 001) and Sunspot 4-5-1 (S = 2001) -- for a grid of kappa0, t0 and three seeds: the spread
(max - min) over the pairs of the mean Rao-Blackwellised acceptance after the freeze, round trips, ti_discretisation."""
import json
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity                                      # noqa: E402
from ptnn_amd import ladder                        # noqa: E402


def cost(R, adapt, S=2001, si=5, reps=3):
    d = parity.datasets()
    best = None
    for _ in range(reps):
        s = parity.make_sampler(0, (4, 5, 1), d["sunspot_train"], d["sunspot_test"], R_local=R, R_global=R, first=0, S=S, si=si,
                                use_lg=False, lr=0.1, seed=3, swap_rule=1, shared_noise=1)
        T = np.asarray(ladder.temperatures(R, 1000), np.float32)
        P = 4 * 5 + 5 + 5 + 1
        s.set_state(np.random.default_rng(3).standard_normal((R, P)).astype(np.float32), T)
        s.set_ladder(T)
        if adapt:
            s.set_ladder_adaptation((S - 2) // si, 0.1, 20.0)
        s.kernel_time(True)
        s.run(-1)
        s.sync()
        n, ms = s.kernel_time(True)
        rounds = s.swap_stats()[2]
        best = ms if best is None else min(best, ms)
        s.close()
    return best, rounds, n


def stationary_data():
    """The 12-row regression of tests/test_gpu_evidence.py (4-3-1, near-stationary random-walk chains after a short burn-in)."""
    rng = np.random.default_rng(11)
    x = rng.random((12, 4))
    return np.column_stack([x, 0.2 + 0.6 * x[:, 0] * x[:, 1] + 0.05 * rng.standard_normal(12)])


def effect_run(problem, spec, seed):
    """One run of an effect problem -> its ladder_diagnostics() (after burn-in) and ti_discretisation."""
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    if problem == "stationary12":
        data = stationary_data()
        train, test, topo, S = data, data, [4, 3, 1], 40001
    else:                                        # "sunspot": the problem the feature was first tried on
        d = parity.datasets()
        train, test, topo, S = d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 2001
    with tempfile.TemporaryDirectory() as tmp:
        pt = ParallelTempering(False, 0.1, train, test, topo, 16, 1000, 16 * S, 5, 0.5, tmp, seed=seed, write_files=False,
                               swap_rule=1, shared_noise=False, adapt_ladder=spec)
        pt.initialize_chains(0.5)
        pt.run_chains()
        dg = pt.ladder_diagnostics()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev = pt.log_evidence(prior_draws=1 << 16)
        pt._sampler.close()
    return dict(spread=float(np.ptp(dg["pair_accept_rb"])), rb=np.round(dg["pair_accept_rb"], 3).tolist(),
                ladder=np.round(dg["temperatures"], 3).tolist(), round_trips=int(dg["round_trips"].sum()),
                ti_discretisation=float(ev.ti_discretisation))


def reduce_rocprof(dir_off, dir_on):
    """swap_kernel's mean duration per ladder size from the rocprofv3 databases of `--cost off` and `--cost on` (grid size /
    work-group size = R work-groups: one per replica)."""
    import glob
    import sqlite3
    mean = {}
    for mode, d in (("off", dir_off), ("on", dir_on)):
        for db in glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True):
            c = sqlite3.connect(db)
            for gx, wx, n, avg in c.execute("select grid_x, workgroup_x, count(*), avg(duration) from kernels "
                                            "where name like '%swap_kernel%' group by grid_x, workgroup_x"):
                mean[(mode, gx // wx)] = (avg, n)
    out = []
    for R in sorted({R for _, R in mean}):
        (off, n), (on, _) = mean[("off", R)], mean[("on", R)]
        out.append(dict(kind="swap_kernel", R=R, rounds_per_run=n, workgroups=R, mean_ns_off=round(off, 1), mean_ns_on=round(on, 1),
                        added_ns_per_round=round(on - off, 1)))
    return out


def main():
    """  --cost off|on        the runs to profile:  rocprofv3 --kernel-trace --stats -d DIR -o run -- python ladder_probe.py --cost off
         --reduce DOFF DON    swap_kernel records (JSON lines) from the two rocprofv3 output directories
         [OUT]                the effect grid (JSON lines to OUT, default profiles/ladder_probe_effect.jsonl)"""
    if len(sys.argv) > 2 and sys.argv[1] == "--cost":
        for R in (64, 256, 1024):
            print(json.dumps(dict(kind="cost", R=R, adapt=sys.argv[2], rounds=cost(R, sys.argv[2] == "on", reps=1)[1])), flush=True)
        return
    if len(sys.argv) > 3 and sys.argv[1] == "--reduce":
        for rec in reduce_rocprof(sys.argv[2], sys.argv[3]):
            print(json.dumps(rec))
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ladder_probe_effect.jsonl")
    with open(path, "w") as f:
        for problem in ("stationary12", "sunspot"):
            for seed in (5, 6, 7):
                grid = [("fixed", dict(rounds=0))] + [(f"k{k}_t{t}", dict(kappa0=k, t0=t))
                                                      for k in (0.05, 0.2, 1.0) for t in (100.0, 1000.0)]
                for name, spec in grid:
                    rec = dict(kind="effect", problem=problem, seed=seed, setting=name, **spec, **effect_run(problem, spec, seed))
                    print(json.dumps({k: rec[k] for k in ("problem", "seed", "setting", "spread", "round_trips", "ti_discretisation")}),
                          flush=True)
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
