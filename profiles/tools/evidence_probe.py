"""Log evidence (ParallelTemperingBase.log_evidence) timed after a bench-shaped run of each of the five bench.py workloads.

For each workload (bench.WORKLOADS: chains, S, proposals, maxtemp as bench.py runs them; seed 7), burn-in 0.5, thin 1, 2^20 prior
draws: wall time of the whole call (host clock around a call that synchronises; one untimed call first; minimum and median of
--reps calls), the same with 2 prior draws (the rungs alone), prior draws per second from the difference, the draws per rung,
n_distinct / all rung draws, and the estimates.
One JSON line per workload; --out writes them to a file as well.

    python profiles/tools/evidence_probe.py [--workloads sunspot64,...] [--reps 3] [--out profiles/evidence_probe.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402


def _timed(fn, reps):
    fn()                                                          # first call: code objects, allocations
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                                # returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return out, min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(bench.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prior-draws", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for key in a.workloads.split(","):
        c = bench.WORKLOADS[key]
        train, test, _ = bench.load_data(c["data"])
        R, S = c["R"], c["S"]
        with tempfile.TemporaryDirectory() as tmp:
            if c["task"] == 0:
                from ptnn_amd.pt_timeseries_regression import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, c["si"], 0.5, tmp,
                                       seed=7, write_files=False)
            else:
                from ptnn_amd.pt_classification import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, c["si"], tmp, seed=7,
                                       write_files=False)
            pt.initialize_chains(0.5)
            pt.run_chains()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ev, t_min, t_med = _timed(lambda: pt.log_evidence(prior_draws=a.prior_draws), a.reps)
                _, r_min, _ = _timed(lambda: pt.log_evidence(prior_draws=2), a.reps)
            n_rung = int(ev.n_draws[1:].sum())
            prior_s = max(t_min - r_min, 1e-9)
            line = dict(workload=key, chains=R, S=S, n_train=int(np.asarray(train).shape[0]), P=int(pt.num_param),
                        draws_per_rung=int(ev.n_draws[1]), n_distinct=int(ev.n_distinct), distinct_ratio=round(ev.n_distinct / n_rung, 5),
                        prior_draws=a.prior_draws, wall_s_min=round(t_min, 6), wall_s_median=round(t_med, 6),
                        wall_s_rungs_only_min=round(r_min, 6), prior_draws_per_s=round(a.prior_draws / prior_s, 1),
                        log_z_ss=round(ev.log_z_ss, 4), se_log_z_ss=round(ev.se_log_z_ss, 4), log_z_ti=round(ev.log_z_ti, 4),
                        se_log_z_ti=round(ev.se_log_z_ti, 4), ti_discretisation=round(ev.ti_discretisation, 4),
                        prior_kish_ess=round(ev.prior_kish_ess, 2))
            print(json.dumps(line), flush=True)
            lines.append(line)
            pt._sampler.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
